"""Fleets in the interior-point LamMuZ mode (`lmz_central=1e-3`, the robust mode): the corridor from 16 perturbed starts as ONE fleet rollout against the
loop of 16 solo `MPC` loops, and the LamMuZ time per executed launch of the fleet kernels.

  corridor   BASELINE C2 (`scenarios.scene_corridor(n_extra=0)`, max_edge_num = 4, max_obs_num = 6, speed 4, at most 300 ticks) from the 16 starts of
             tests/test_gpu_central.py::test_robust_mode_reaches_the_goal_from_perturbed_starts (the same `default_rng(11)` draws):
             (a) fleet  ONE `Fleet.rollout(..., steps=300, moving=True, clearance=True)` of 16 members - the device clearance log on the static scene
             (b) solo   the 16 `MPC.control` loops one after the other, clearance by `scenarios.clearance` on the host: what the test runs, and all a user
                        could do before fleets took members in this mode (the baseline)
             success = goal reached and the clearance stayed positive up to the arrival; wall time of each leg in a process of its own, a short warm-up
             (code objects, first-use tables) before the clock starts, `--repeats` interleaved repeats
  kernels    `rocprofv3 --kernel-trace` of leg (a) and of K ticks of `rda_fleet_rollout` on the C5 shape (T = 25, N = 100 polygons per ego, own seeded
             scene per ego, re-sorted every tick) with B = 16 and 64 members, each in a run of its own.  Per LamMuZ kernel: the dispatches and their time by
             ADMM iteration index.  The launch of iteration 0 runs every member (no member has stopped yet: the full grid, B x T x ceil(N / 8) workgroups);
             in a later launch the members that stopped early return at once, so its time falls with the members still iterating, down to a launch that
             every member skips.  "executed": a launch longer than a tenth of the median iteration-0 launch.  Beside it the untraced rate of the same C5
             run.

    python tools/fleet_central.py [--repeats 3] [--fleets 16,64] [--K 100] [--so PATH] [--no-trace]        (output: profiles/fleet_central.txt)

--so: another build of librda_hip.so for every leg (an A/B of a build switch such as -DLMZ_FLEET_IP_OCC=2).  No speed-up is asserted anywhere.
One leg alone, as JSON:  python tools/fleet_central.py --leg fleet | solo | c5 [--B 16]
"""
import argparse
import collections
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
MU, STEPS, SPEED = 1e-3, 300, 4
T5, N5 = 25, 100


def corridor():
    from rda_planner_amd import scenarios as sc
    rng = np.random.default_rng(11)
    starts = [(0.0, 0.0, 0.0)] + [(rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.08, 0.08)) for _ in range(15)]
    car = sc.rectangle_robot(dynamics="acker")
    path = sc.line_path([0, 20, 0], [60, 20, 0], 0.1)
    return car, path, sc.scene_corridor(n_extra=0), [np.array([[0.0 + dx], [20.0 + dy], [0.0 + dth]]) for dx, dy, dth in starts]


def planner(car, path):
    from rda_planner_amd.mpc import MPC
    return MPC(car, [p.copy() for p in path], sample_time=0.1, time_print=False, max_edge_num=4, max_obs_num=6, lmz_central=MU)


def leg_fleet():
    from rda_planner_amd.fleet import Fleet
    car, path, obs, states = corridor()
    warm = Fleet([planner(car, path) for _ in states[:2]])          # code objects and first-use set-up, on members of their own
    warm.rollout(states[:2], SPEED, steps=3, obstacle_lists=[list(obs)] * 2, moving=True, clearance=True)
    warm.close()
    fleet = Fleet([planner(car, path) for _ in states])
    t0 = time.perf_counter()
    out = fleet.rollout(states, SPEED, steps=STEPS, obstacle_lists=[list(obs) for _ in states], moving=True, clearance=True)
    el = time.perf_counter() - t0
    at = out["arrived_at"]
    ok = [bool(at[i] >= 0 and out["clearance"][:at[i] + 1, i].min() > 0.0) for i in range(len(states))]
    ticks = int(sum(at[i] + 1 if at[i] >= 0 else STEPS for i in range(len(states))))
    res = {"leg": "fleet", "ok": int(sum(ok)), "of": len(ok), "seconds": el, "kernel": fleet.lammuz_kernel(), "ego_ticks_to_arrival": ticks,
           "mean_admm_iters": float(out["iters"].mean())}
    fleet.close()
    return res


def leg_solo():
    from rda_planner_amd import scenarios as sc
    car, path, obs, states = corridor()
    w = planner(car, path)
    for _ in range(3):
        w.control(states[0].copy(), SPEED, list(obs))
    w.rda._be.close()
    ok, ticks, t0 = 0, 0, time.perf_counter()
    for s0 in states:
        mpc, state, minc, arrived = planner(car, path), s0.copy(), np.inf, False
        for _ in range(STEPS):
            u, info = mpc.control(state, SPEED, list(obs))
            state = sc.kinematic_step(state, u, car, 0.1)
            minc = min(minc, sc.clearance(car, state, obs))
            ticks += 1
            if info["arrive"]:
                arrived = True
                break
        ok += int(arrived and minc > 0.0)
        mpc.rda._be.close()
    return {"leg": "solo", "ok": ok, "of": len(states), "seconds": time.perf_counter() - t0, "ego_ticks_to_arrival": ticks}


def leg_c5(B, K):
    """K ticks of rda_fleet_rollout (re-sorted every tick) of B members of the C5 shape in the interior-point mode, after a first window of K"""
    from benchlib.workload import build_workload
    from rda_planner_amd._capi import Info, dptr, iptr
    from rda_planner_amd._lib import hip_api
    from rda_planner_amd.rda_solver import RDA_solver
    api = hip_api()
    svs, states = [], np.zeros((B, 3))
    for e in range(B):
        car_t, path, obstacles, kw = build_workload(seed_offset=e, n_obs=N5, T=T5, n_steps=2 * K + 10)
        sv = RDA_solver(T5, car_t, kw["max_edge_num"], N5, iter_num=kw["iter_num"], step_time=0.1, time_print=False, ro1=kw["ro1"], lmz_central=MU)
        n_sc, kind, nvert, geom, vel = sv.flatten_scene(list(obstacles))
        kind, nvert = np.ascontiguousarray(kind, np.int32), np.ascontiguousarray(nvert, np.int32)
        P = np.ascontiguousarray(np.hstack(path)[0:3, :].T, dtype=float)
        states[e] = np.ascontiguousarray(path[0], float).ravel()[0:3]
        assert api.upload_path(sv._be.handle, int(P.shape[0]), dptr(P)) == 0
        assert api.upload_scene(sv._be.handle, int(n_sc), iptr(kind), iptr(nvert), dptr(np.ascontiguousarray(geom, float)), dptr(np.ascontiguousarray(vel, float)),
                                dptr(states[e]), 1, None) == 0
        svs.append(sv)
    F = C.c_void_p()
    assert api.fleet_create((C.c_void_p * B)(*[sv._be.handle for sv in svs]), B, C.byref(F)) == 0
    kernel = api.fleet_lammuz_kernel(F).decode()
    cur, els, nom0 = np.zeros(B, np.int32), [], np.zeros((B, 2, T5))
    for win in range(2):
        s_log, u, i_log = np.zeros((K + 1, B, 3)), np.zeros((K, B, 2)), np.zeros((K, B), np.int32)
        infos, arrived = (Info * (K * B))(), np.zeros(B, np.int32)
        t0 = time.perf_counter()
        rc = api.fleet_rollout(F, K, dptr(states), dptr(np.full(B, 4.0)), iptr(cur), 0.1, 10, 1, 1, dptr(nom0) if win == 0 else None, dptr(s_log), dptr(u),
                               iptr(i_log), infos, iptr(arrived))
        els.append(time.perf_counter() - t0)
        assert rc == 0 and np.all(arrived == -1), rc
        states, cur = np.ascontiguousarray(s_log[K]), np.ascontiguousarray(i_log[K - 1])
    iters = np.array([i.iters for i in infos])
    fails = int(sum(i.lmz_fail for i in infos))
    api.fleet_destroy(F)
    return {"leg": "c5", "B": B, "K": K, "kernel": kernel, "ego_steps_per_s": B * K / els[1], "ms_per_tick": 1e3 * els[1] / K, "mean_admm_iters": float(iters.mean()),
            "lmz_fail": fails}


def child(args, leg, B=0, trace_dir=None):
    env = dict(os.environ)
    if args.so:
        env["RDA_HIP_SO"] = os.path.abspath(args.so)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--B", str(B), "--K", str(args.K)]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "-o", "f", "--"] + cmd
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.leg_timeout)
    if res.returncode != 0:
        raise RuntimeError(f"leg {leg} B={B} ended with {res.returncode}: {res.stderr[-600:]}")
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])


def lammuz_table(trace_dir, iter_num, lead=0):
    """per LamMuZ kernel of a kernel trace, in dispatch order without the first `lead` ADMM iterations: (name, dispatches, executed, mean us of the
    executed ones, ms in all, [(mean us, median us) per ADMM iteration index] or None where the dispatches are not one per iteration)"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise RuntimeError("no kernel trace was written")
    d = collections.defaultdict(list)
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"].split("(")[0].replace("void ", "")
        if name.startswith("k_lammuz") or name.startswith("k_lmz_finalize_fleet"):
            d[name].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    rows = []
    for name, v in sorted(d.items()):
        dur = np.array([x[1] for x in sorted(v)])[lead:]
        by_it = None
        if len(dur) and len(dur) % iter_num == 0:
            per = dur.reshape(-1, iter_num)
            by_it = [(float(per[:, i].mean()), float(np.median(per[:, i]))) for i in range(iter_num)]
        ex = dur[dur > 0.1 * (by_it[0][1] if by_it else np.percentile(dur, 98))]
        rows.append((name, len(dur), len(ex), float(ex.mean()), float(dur.sum()) / 1e3, by_it))
    return rows


def traced(args, leg, iter_num, lead=0, B=0):
    tmp = tempfile.mkdtemp(prefix="fleet_central_")
    try:
        res = child(args, leg, B, trace_dir=tmp)
        return res, lammuz_table(tmp, iter_num, lead)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def print_table(rows):
    for name, n, nex, mean, tot, by_it in rows:
        print("       %-24s dispatches %5d, executed %5d at a mean of %8.2f us (%.1f ms in all)" % (name, n, nex, mean, tot))
        if by_it:
            print("       %-24s us by ADMM iteration index, mean (median): %s" % ("", "  ".join("it %d %8.2f (%8.2f)" % (i, m, md) for i, (m, md) in enumerate(by_it))))


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(x) for x in s.split(",")]             # noqa: E731
    ap.add_argument("--fleets", type=ints, default=[16, 64])
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--so", default=None, help="another build of librda_hip.so for every leg")
    ap.add_argument("--no-trace", action="store_true", help="wall times only (no rocprofv3 runs)")
    ap.add_argument("--leg-timeout", type=float, default=300.0)
    ap.add_argument("--leg", choices=["fleet", "solo", "c5"], default=None, help="(internal) run one leg in this process and print it as JSON")
    ap.add_argument("--B", type=int, default=16)
    args = ap.parse_args()
    if args.leg:
        print(json.dumps({"fleet": leg_fleet, "solo": leg_solo, "c5": lambda: leg_c5(args.B, args.K)}[args.leg]()))
        return
    print("corridor (C2) from 16 perturbed starts, lmz_central = %g, at most %d ticks each, library: %s" % (MU, STEPS, args.so or "this build"))
    a, b = [], []
    for _ in range(args.repeats):
        a.append(child(args, "fleet"))
        b.append(child(args, "solo"))
    print("  (a) ONE fleet rollout of 16 members (moving=True, clearance=True): success %s of 16, wall s %s   [LamMuZ launches: %s]"
          % ("/".join(str(x["ok"]) for x in a), " ".join("%.3f" % x["seconds"] for x in a), a[0]["kernel"]))
    print("  (b) 16 solo MPC.control loops, one after the other:                success %s of 16, wall s %s"
          % ("/".join(str(x["ok"]) for x in b), " ".join("%.3f" % x["seconds"] for x in b)))
    ma, mb = np.median([x["seconds"] for x in a]), np.median([x["seconds"] for x in b])
    print("      medians: fleet %.3f s, solo loop %.3f s (%.1fx); ego-ticks until arrival: fleet %d (it steps all 16 for %d ticks: %d ego-ticks), solo %d; "
          "mean ADMM iterations per fleet ego-tick %.2f" % (ma, mb, mb / ma, a[0]["ego_ticks_to_arrival"], STEPS, 16 * STEPS, b[0]["ego_ticks_to_arrival"],
                                                          a[0]["mean_admm_iters"]))
    if args.no_trace:
        return
    print("LamMuZ time per executed launch (rocprofv3 --kernel-trace, each run of its own):")
    res, rows = traced(args, "fleet", 4, lead=3 * 4)            # (MPC's default iter_num = 4; without the 3 warm-up ticks of the 2-member fleet)
    print("  corridor, B = 16, T = 10, N = 6, iter_num = 4 (leg (a): 300 ticks, %d ego-ticks of them before the arrivals):" % res["ego_ticks_to_arrival"])
    print_table(rows)
    for B in args.fleets:
        plain = child(args, "c5", B)
        res, rows = traced(args, "c5", 4, B=B)                   # (build_workload: iter_num = 4)
        print("  C5 shape, B = %d, T = %d, N = %d, 2 x %d ticks of rda_fleet_rollout [%s]: untraced %.0f ego-steps/s, %.3f ms per fleet tick, mean ADMM iterations "
              "%.2f, lmz_fail %d" % (B, T5, N5, args.K, plain["kernel"], plain["ego_steps_per_s"], plain["ms_per_tick"], plain["mean_admm_iters"], plain["lmz_fail"]))
        print_table(rows)


if __name__ == "__main__":
    main()
