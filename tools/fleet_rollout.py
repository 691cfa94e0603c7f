"""Fleet closed loop: the host-driven loop against the device rollout, in ego-steps/s.

  (a) host loop  tools/closed_loop_host.c closed_loop_fleet_run, resort = 2: per fleet tick rda_fleet_scene_resort + ONE rda_fleet_step_tracked + one host
                 wait + every member's kinematics on the host
  (b) rollout    ONE rda_fleet_rollout of K ticks: the same launches per tick plus rollout::k_rollout_advance, one host wait after the K ticks

on the same members: BASELINE config C5 (T = 25, N = 100 polygons per ego, every ego its own seeded scene, re-sorted about its robot on every tick, the
members of bench.py's `c_abi_closed_loop` leg), B = 16 and 64.  A measurement: --warm host-driven ticks, then TWO windows of K = 100 ticks by the leg's own
method - the first one warms what the method uses (the rollout's tables and log block are made on first use), the second one is the figure.  Every
measurement runs in a process of its own (fresh handles); the legs are interleaved (a b a b a b), medians over --repeats.  --baseline-so: another build of librda_hip.so for leg (a) - the
parent commit's, so that the host loop is timed on the code it had before the rollout existed.

    python tools/fleet_rollout.py [--fleets 16,64] [--K 100] [--repeats 3] [--warm 6] [--baseline-so PATH]

--moving: the same comparison for scenes that MOVE (C5 shape with `scene_polygons(moving=True)` members: BASELINE C4's obstacles in a fleet).
  (a) host loop  closed_loop_fleet_run_moving: per tick every member's geometry put forward on the host, ONE rda_fleet_upload_scenes, ONE
                 rda_fleet_step_tracked + one host wait, the plants on the host
  (b) rollout    ONE rda_fleet_rollout_moving of K ticks (no clearance log): the motion by scene::k_move_fleet, one host wait after the K ticks
Both legs exist only from the commit that added the moving rollout on, so both run on this build (--baseline-so is not used).

    python tools/fleet_rollout.py --moving [--fleets 16,64] [--K 100] [--repeats 3] [--warm 6]         (output: profiles/fleet_rollout_moving.txt)

--gears: the parking fleet of examples/reverse_headless.py (forward / back / forward on a path with gear pieces, two boxes beside every bay; legs long
enough for the ticks asked for), through the Python interface on the same `MPC` members:
  (a) host loop  per tick ONE Fleet.control (every piece brought to the device when it comes into force, MPC._end on the host) + the plants on the host
  (b) rollout    ONE Fleet.rollout(gears=True) of K ticks: all pieces resident, the piece bookkeeping by rollout::k_rollout_advance_gears, one host wait
The host loop is the yardstick and exists before the gear rollout did.  Both rates and their ratio also go to --out.

    python tools/fleet_rollout.py --gears [--fleets 16,64] [--K 100] [--repeats 3] [--warm 6]          (output: profiles/fleet_rollout_gears.txt)

One measurement alone (what a kernel trace is taken of: the launches per tick are those of the host loop plus k_rollout_advance):
    python tools/fleet_rollout.py --leg rollout --B 16        (or --leg host)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
T, N = 25, 100


def members(api, B, n_steps, moving=False):
    """B fresh solvers of the C5 shape with their paths and raw scenes resident, and their fleet (+ the members' raw scenes, concatenated)"""
    from benchlib.workload import build_workload
    from rda_planner_amd._capi import dptr, iptr
    from rda_planner_amd.rda_solver import RDA_solver
    svs, states, plen, raw = [], np.zeros((B, 3)), np.zeros(B, np.int32), []
    for e in range(B):
        car_t, path, obstacles, kw = build_workload(seed_offset=e, n_obs=N, T=T, n_steps=n_steps + 10, moving=moving)
        sv = RDA_solver(T, car_t, kw["max_edge_num"], N, iter_num=kw["iter_num"], step_time=0.1, time_print=False, ro1=kw["ro1"])
        n_sc, kind, nvert, geom, vel = sv.flatten_scene(list(obstacles))
        kind, nvert = np.ascontiguousarray(kind, np.int32), np.ascontiguousarray(nvert, np.int32)
        geom, vel = np.ascontiguousarray(geom, float), np.ascontiguousarray(vel, float)
        P = np.ascontiguousarray(np.hstack(path)[0:3, :].T, dtype=float)
        states[e] = np.ascontiguousarray(path[0], float).ravel()[0:3]
        plen[e] = P.shape[0]
        assert api.upload_path(sv._be.handle, int(P.shape[0]), dptr(P)) == 0
        assert api.upload_scene(sv._be.handle, int(n_sc), iptr(kind), iptr(nvert), dptr(geom), dptr(vel), dptr(states[e]), 1, None) == 0
        svs.append(sv)
        raw.append((kind, nvert, geom, vel))
    scene = dict(counts=np.array([len(r[0]) for r in raw], np.int32), maxv=int(raw[0][2].shape[1]))
    scene.update({key: np.ascontiguousarray(np.concatenate([r[j] for r in raw])) for j, key in enumerate(("kind", "nvert", "geom0", "vel"))})
    scene["geom"], scene["order"] = scene["geom0"].copy(), np.ones(B, np.int32)
    arr = (C.c_void_p * B)(*[sv._be.handle for sv in svs])
    F = C.c_void_p()
    assert api.fleet_create(arr, B, C.byref(F)) == 0
    return svs, arr, F, np.ascontiguousarray(states), plen, car_t, scene


def leg(name, B, K, warm, moving=False):
    """one measurement in this process: `warm` host-driven ticks, then K timed ticks by the host loop or by the rollout -> dict"""
    from rda_planner_amd._capi import Info, dptr, iptr
    from rda_planner_amd._lib import hip_api
    import closed_loop_host as clh
    api = hip_api()
    host = clh.Host(api.lib)
    n_all = warm + 2 * K
    svs, arr, F, states, plen, car_t, sc = members(api, B, n_all, moving)
    cur, nom0 = np.zeros(B, np.int32), np.zeros((B, 2, T))
    u_log, t_log = np.zeros((n_all, B, 2)), np.zeros(n_all)
    it_log, ipm_log = np.zeros((n_all, B), np.int32), np.zeros((n_all, B), np.int32)

    def host_ticks(k0, n):
        if moving:
            rc = host.fleet_run_moving(C.byref(host.fleet_moving_api), F, B, T, 0, float(car_t.wheelbase), 0.1, 4.0, 0.1, 10, iptr(plen), iptr(sc["counts"]),
                                       sc["maxv"], iptr(sc["kind"]), iptr(sc["nvert"]), dptr(sc["geom"]), dptr(sc["geom0"]), dptr(sc["vel"]), iptr(sc["order"]),
                                       k0, n, dptr(nom0), dptr(states), iptr(cur), dptr(u_log[k0:]), dptr(t_log[k0:]), iptr(it_log[k0:]), iptr(ipm_log[k0:]))
            assert rc == 0, rc
            return
        rc = host.fleet_run(C.byref(host.fleet_api), F, arr, B, T, 0, float(car_t.wheelbase), 0.1, 4.0, 0.1, 10, iptr(plen), 2, k0, n, dptr(nom0), dptr(states),
                            iptr(cur), dptr(u_log[k0:]), dptr(t_log[k0:]), iptr(it_log[k0:]), iptr(ipm_log[k0:]))
        assert rc == 0, rc
    host_ticks(0, warm)
    els = []
    for win in range(2):
        k0 = warm + win * K
        t0 = time.perf_counter()
        if name == "host":
            host_ticks(k0, K)
            els.append(time.perf_counter() - t0)
            u, iters = u_log[k0:k0 + K], it_log[k0:k0 + K]
        else:
            s_log, u, i_log = np.zeros((K + 1, B, 3)), np.zeros((K, B, 2)), np.zeros((K, B), np.int32)
            infos, arrived = (Info * (K * B))(), np.zeros(B, np.int32)
            if moving:
                if win == 0:        # the host-driven ticks left the geometry of tick warm - 1 on the device: stage tick `warm`; from then on it is resident
                    full = sc["geom0"] + sc["vel"][:, None, :] * (0.1 * k0)
                    live = np.arange(sc["maxv"])[None, :] < sc["nvert"][:, None]
                    sc["geom"][live] = full[live]
                    rob = np.ascontiguousarray(states[:, 0:2])
                    assert api.fleet_upload_scenes(F, iptr(sc["counts"]), iptr(sc["kind"]), iptr(sc["nvert"]), dptr(sc["geom"]), dptr(sc["vel"]), dptr(rob),
                                                   iptr(sc["order"])) == 0
                rc = api.fleet_rollout_moving(F, K, dptr(states), dptr(np.full(B, 4.0)), iptr(cur), 0.1, 10, 1, 1, None, dptr(s_log), dptr(u), iptr(i_log),
                                              infos, iptr(arrived), None)
            else:
                rc = api.fleet_rollout(F, K, dptr(states), dptr(np.full(B, 4.0)), iptr(cur), 0.1, 10, 1, 1, None, dptr(s_log), dptr(u), iptr(i_log), infos,
                                       iptr(arrived))
            els.append(time.perf_counter() - t0)
            assert rc == 0, rc
            assert np.all(arrived == -1)
            states, cur = np.ascontiguousarray(s_log[K]), np.ascontiguousarray(i_log[K - 1])
            iters = np.array([i.iters for i in infos]).reshape(K, B)
    el = els[1]
    out = {"leg": name, "B": B, "K": K, "ego_steps_per_s": B * K / el, "ms_per_tick": 1e3 * el / K, "first_window_ego_steps_per_s": B * K / els[0],
           "mean_admm_iters": float(iters.mean()), "u_last": [float(x) for x in u[-1, 0]]}
    api.fleet_destroy(F)
    return out


def gears_leg(name, B, K, warm):
    """one measurement of the parking fleet in this process: `warm` ticks of Fleet.control, then two windows of K ticks by the leg's method -> dict"""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import reverse_headless as rh
    from rda_planner_amd import scenarios as scn
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    reach = 0.3 * (warm + 2 * K) / 3 + 4.0                 # three legs that outlast the run at 3 m/s
    made = [rh.parking(lane, forward=reach + 2.0, back=reach, out=reach + 2.0) for lane in range(B)]
    fleet = Fleet([MPC(car, path, sample_time=rh.DT, **rh.MPC_KW) for car, path, _, _ in made])
    cars, obs = [m[0] for m in made], [m[2] for m in made]
    states = [m[3] for m in made]
    pieces = []

    def host_ticks(n):
        nonlocal states
        for _ in range(n):
            for m in fleet.members:
                if m.curve_index >= len(m.curve_list):
                    rh.hold_arrived(m)
            pieces.append([m.curve_index for m in fleet.members])
            res = fleet.control(states, rh.SPEED, obs)
            states = [scn.kinematic_step(states[i], res[i][0], cars[i], rh.DT) for i in range(B)]
    host_ticks(warm)
    els = []
    for win in range(2):
        t0 = time.perf_counter()
        if name == "host":
            host_ticks(K)
        else:
            out = fleet.rollout(states, rh.SPEED, K, gears=True)
            states = [out["states"][K, i].reshape(3, 1) for i in range(B)]
            pieces.extend(out["piece"].tolist())
        els.append(time.perf_counter() - t0)
    el = els[1]
    fleet.close()
    return {"leg": name, "B": B, "K": K, "ego_steps_per_s": B * K / el, "ms_per_tick": 1e3 * el / K, "first_window_ego_steps_per_s": B * K / els[0],
            "pieces_seen": sorted({p for row in pieces for p in row}), "x_last": float(np.asarray(states[0], float).ravel()[0])}


def gears_main(args):
    lines = ["parking fleet (examples/reverse_headless.py: forward / back / forward on gear pieces, T = 10, N = 4 slots, 2 boxes per member): %d ticks of "
             "Fleet.control, a first window of K = %d ticks, then the timed window of K ticks; %d interleaved repeats, every measurement in a process of its own"
             % (args.warm, args.K, args.repeats),
             "(a) host loop: Fleet.control + the plants per tick; (b) ONE Fleet.rollout(gears=True) of K ticks",
             "%4s | %-34s | %-34s | %s" % ("B", "(a) host loop ego-steps/s", "(b) gear rollout ego-steps/s", "median (b) / (a)")]
    for B in args.fleets:
        a, b = [], []
        for _ in range(args.repeats):
            a.append(child("host", B, args))
            b.append(child("rollout", B, args))
        ra, rb = [x["ego_steps_per_s"] for x in a], [x["ego_steps_per_s"] for x in b]
        fmt = lambda v: " ".join("%9.0f" % x for x in v)        # noqa: E731
        lines.append("%4d | %-34s | %-34s | %.2fx" % (B, fmt(ra), fmt(rb), np.median(rb) / np.median(ra)))
        lines.append("       ms per fleet tick (medians): host %.3f, rollout %.3f; first window (one-time set-up included): host %.0f, rollout %.0f ego-steps/s"
                     % (np.median([x["ms_per_tick"] for x in a]), np.median([x["ms_per_tick"] for x in b]),
                        np.median([x["first_window_ego_steps_per_s"] for x in a]), np.median([x["first_window_ego_steps_per_s"] for x in b])))
        lines.append("       pieces in force during the run: host %s, rollout %s; x of member 0 at the end: host %.6f, rollout %.6f"
                     % (a[0]["pieces_seen"], b[0]["pieces_seen"], a[0]["x_last"], b[0]["x_last"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


def child(name, B, args):
    env = dict(os.environ)
    if name == "host" and args.baseline_so and not args.moving:
        env["RDA_HIP_SO"] = os.path.abspath(args.baseline_so)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--B", str(B), "--K", str(args.K), "--warm", str(args.warm)] + (["--moving"] if args.moving else []) + (["--gears"] if args.gears else [])
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.leg_timeout)
    if res.returncode != 0:
        raise RuntimeError(f"leg {name} B={B} ended with {res.returncode}: {res.stderr[-400:]}")
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])


def print_static_head(args):
    print("fleet closed loop, C5 shape (T = %d, N = %d, own seeded scene per ego, re-sorted every tick): %d host-driven ticks, a first window of K = %d ticks, then the "
          "timed window of K ticks; %d interleaved repeats" % (T, N, args.warm, args.K, args.repeats))
    print("host loop: closed_loop_fleet_run (resort = 2) on %s" % ("the baseline library (the parent commit's build)" if args.baseline_so else "this library"))


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(x) for x in s.split(",")]             # noqa: E731
    ap.add_argument("--fleets", type=ints, default=[16, 64])
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-so", default=None)
    ap.add_argument("--moving", action="store_true", help="scenes that move: closed_loop_fleet_run_moving against rda_fleet_rollout_moving, both on this build")
    ap.add_argument("--gears", action="store_true", help="the parking fleet: Fleet.control + plant per tick against ONE Fleet.rollout(gears=True)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_rollout_gears.txt"), help="--gears: where the table is written as well")
    ap.add_argument("--leg-timeout", type=float, default=300.0)
    ap.add_argument("--leg", choices=["host", "rollout"], default=None, help="(internal) run one measurement in this process and print it as JSON")
    ap.add_argument("--B", type=int, default=16)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    if args.leg:
        print(json.dumps(gears_leg(args.leg, args.B, args.K, args.warm) if args.gears else leg(args.leg, args.B, args.K, args.warm, args.moving)))
        return
    assert args.repeats >= 3
    if args.gears:
        gears_main(args)
        return
    if args.moving:
        print("fleet closed loop with MOVING scenes, C5 shape (T = %d, N = %d moving polygons per ego, velocities U[-1,1]^2 m/s, own seeded scene per ego, re-sorted every "
              "tick): %d host-driven ticks, a first window of K = %d ticks, then the timed window of K ticks; %d interleaved repeats" % (T, N, args.warm, args.K, args.repeats))
        print("host loop: closed_loop_fleet_run_moving (geometry forward on the host, rda_fleet_upload_scenes, rda_fleet_step_tracked per tick) on this library; "
              "(b) = rda_fleet_rollout_moving without a clearance log")
    else:
        print_static_head(args)
    print("%4s | %-40s | %-40s | %s" % ("B", "(a) host loop ego-steps/s", "(b) rda_fleet_rollout_moving ego-steps/s" if args.moving else "(b) rda_fleet_rollout ego-steps/s", "median (b) / (a)"))
    verdicts = []
    for B in args.fleets:
        a, b = [], []
        for _ in range(args.repeats):
            a.append(child("host", B, args))
            b.append(child("rollout", B, args))
        ra, rb = [x["ego_steps_per_s"] for x in a], [x["ego_steps_per_s"] for x in b]
        fmt = lambda v: " ".join("%9.0f" % x for x in v)        # noqa: E731
        print("%4d | %-40s | %-40s | %.2fx" % (B, fmt(ra), fmt(rb), np.median(rb) / np.median(ra)))
        print("       ms per fleet tick (medians): host %.3f, rollout %.3f; mean ADMM iterations per ego-step: host %.3f, rollout %.3f"
              % (np.median([x["ms_per_tick"] for x in a]), np.median([x["ms_per_tick"] for x in b]), a[0]["mean_admm_iters"], b[0]["mean_admm_iters"]))
        print("       first window (one-time set-up included), medians: host %.0f, rollout %.0f ego-steps/s"
              % (np.median([x["first_window_ego_steps_per_s"] for x in a]), np.median([x["first_window_ego_steps_per_s"] for x in b])))
        print("       last applied control of ego 0: host %s, rollout %s (the two loops differ in the last bits of sin / cos / tan of the plant step)"
              % (a[0]["u_last"], b[0]["u_last"]))
        spread = max(ra) - min(ra)
        verdicts.append((B, np.median(rb) >= np.median(ra) - spread, np.median(ra), np.median(rb), spread))
    for B, ok, ma, mb, spread in verdicts:
        print("  B = %2d: rollout median %.0f vs host-loop median %.0f ego-steps/s (host loop's own spread over the repeats: %.0f) - %s"
              % (B, mb, ma, spread, "not slower than the host loop" if ok else "SLOWER than the host loop by more than its spread"))


if __name__ == "__main__":
    main()
