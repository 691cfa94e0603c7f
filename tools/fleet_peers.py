"""Fleet members that avoid each other: the device rollout against the host loop it replaces, and against the rollout of a blind fleet.

  (a) host loop  per tick, in Python: every member's own obstacles put forward, `scenarios.peer_obstacles` for every member (B * (B - 1) obstacle
                 objects), ONE `Fleet.control` (one flatten pass, rda_fleet_upload_scenes, rda_fleet_step_tracked, one host wait), the plants on the host
  (b) peers      ONE `Fleet.rollout(peers=True)` of K ticks (rda_fleet_rollout_peers): per tick scene::k_peers_fleet, the re-sort, the tick, the obstacle
                 motion and rollout::k_peer_clearance_fleet on the device, one host wait after the K ticks
  (c) blind      ONE `Fleet.rollout(moving=True)` of K ticks (rda_fleet_rollout_moving) on the same members without peer rows: (b) / (c) is the cost of
                 the B - 1 extra rows per member and of the two extra launches per tick

on BASELINE config C5's shape with moving obstacles (T = 25, N = 100 slots, 100 moving polygons per ego, every ego its own seeded scene, re-sorted about
its robot on every tick; the members of tools/fleet_rollout.py --moving), the egos' worlds laid side by side as lanes 6 m apart so that the members are
each other's neighbours, B = 16 and 64.  A measurement: --warm ticks by the leg's own method, then the timed window of K = 100 ticks; the rollouts run a
first window of K ticks instead (their tables and log blocks are made on first use).  Every measurement runs in a process of its own (fresh handles); the
legs are interleaved (a b c a b c ...), medians over --repeats.  No ratio is asked of this tool: it reports what it measures.

    python tools/fleet_peers.py [--fleets 16,64] [--K 100] [--repeats 3] [--warm 6]         (output: profiles/fleet_peers.txt)
    python tools/fleet_peers.py --leg peers --B 16                                           (one measurement alone)
    python tools/fleet_peers.py --plan                                                       (output: profiles/fleet_peers_plan.txt)

--plan: the rollout with the peers predicted along their planned trajectories, `Fleet.rollout(peers="plan")` (rda_fleet_rollout_peers_plan:
scene::k_build_plan_fleet in k_build_fleet's place, the same number of launches per tick), beside leg (b), the constant-velocity peers rollout, on the
same members, shapes and windows; legs interleaved (b p b p ...).  No ratio is asked of it either.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
T, N, DT, SPEED, LANE = 25, 100, 0.1, 4.0, 6.0


def fleet(B, n_steps):
    """B `MPC` members of the C5 shape with moving scenes, member e's world shifted by e lanes -> (Fleet, cars, start states, own obstacle lists)"""
    from benchlib.workload import build_workload
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    ms, cars, states, own = [], [], [], []
    for e in range(B):
        car_t, path, obstacles, kw = build_workload(seed_offset=e, n_obs=N, T=T, n_steps=n_steps + 10, moving=True)
        shift = np.array([[0.0], [LANE * e]])
        path = [p + np.vstack((shift, [[0.0]])) for p in path]
        own.append([sc.Obstacle(None, None, o.vertex + shift, o.cone_type, o.velocity) for o in obstacles])
        ms.append(MPC(car_t, path, sample_time=DT, time_print=False, **kw))
        cars.append(car_t)
        states.append(path[0].copy())
    return Fleet(ms), cars, states, own


def leg(name, B, K, warm):
    """one measurement in this process -> dict"""
    from rda_planner_amd import scenarios as sc
    f, cars, states, own = fleet(B, warm + 2 * K)
    if name == "host":
        controls = [np.zeros((2, 1)) for _ in range(B)]
        sep, t0 = np.inf, None
        for k in range(warm + K):
            if k == warm:
                t0 = time.perf_counter()
            t = DT * k
            lists = [[sc.Obstacle(None, None, o.vertex + o.velocity * t, o.cone_type, o.velocity) for o in own[i]] + sc.peer_obstacles(cars, states, controls, i)
                     for i in range(B)]
            res = f.control(states, SPEED, lists)
            controls = [r[0] for r in res]
            states = [sc.kinematic_step(states[i], controls[i], cars[i], DT) for i in range(B)]
        el = time.perf_counter() - t0
        first = el
        iters = float(np.mean([r[1]["iters"] for r in res]))
        sep = float(sc.peer_clearance(cars, states).min())
        u_last = [float(x) for x in controls[0].ravel()]
    else:
        kw = dict(peers=True) if name == "peers" else dict(peers="plan") if name == "plan" else dict(moving=True)
        els = []
        for win in range(2):
            t0 = time.perf_counter()
            out = f.rollout(states, SPEED, K, **(dict(obstacle_lists=own) if win == 0 else {}), **kw)
            els.append(time.perf_counter() - t0)
            assert np.all(out["arrived_at"] == -1)
            states = [out["states"][K, i].reshape(3, 1) for i in range(B)]
        el, first = els[1], els[0]
        iters = float(out["iters"].mean())
        sep = float(out["peer_clearance"].min()) if name in ("peers", "plan") else float(sc.peer_clearance(cars, states).min())
        u_last = [float(x) for x in out["controls"][-1, 0]]
    f.close()
    return {"leg": name, "B": B, "K": K, "ego_steps_per_s": B * K / el, "ms_per_tick": 1e3 * el / K, "first_window_ego_steps_per_s": B * K / first,
            "mean_admm_iters": iters, "min_separation": sep, "u_last": u_last}


def child(name, B, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--B", str(B), "--K", str(args.K), "--warm", str(args.warm)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.leg_timeout)
    if res.returncode != 0:
        raise RuntimeError(f"leg {name} B={B} ended with {res.returncode}: {res.stderr[-400:]}")
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])


def plan_table(args):
    print("peers predicted along their planned trajectories against peers at constant velocity, C5 shape with moving scenes (T = %d, N = %d slots, %d moving "
          "polygons per ego, lanes %.0f m apart, re-sorted every tick): timed window of K = %d ticks behind a first window of K ticks; %d interleaved repeats"
          % (T, N, N, LANE, args.K, args.repeats))
    print('(b) Fleet.rollout(peers=True), the constant-velocity mode (the baseline);  (p) Fleet.rollout(peers="plan")')
    print("%4s | %-32s | %-32s | %s" % ("B", "(b) peers rollout ego-steps/s", "(p) plan rollout ego-steps/s", "(p) / (b)"))
    for B in args.fleets:
        runs = {"peers": [], "plan": []}
        for _ in range(args.repeats):
            for name in runs:
                runs[name].append(child(name, B, args))
        rate = {name: [x["ego_steps_per_s"] for x in v] for name, v in runs.items()}
        med = {name: float(np.median(v)) for name, v in rate.items()}
        fmt = lambda v: " ".join("%9.0f" % x for x in v)        # noqa: E731
        print("%4d | %-32s | %-32s | %.3fx" % (B, fmt(rate["peers"]), fmt(rate["plan"]), med["plan"] / med["peers"]))
        print("       ms per fleet tick (medians): peers %.3f, plan %.3f; mean ADMM iterations per ego-step: peers %.3f, plan %.3f"
              % tuple([np.median([x["ms_per_tick"] for x in runs[n]]) for n in runs] + [runs[n][0]["mean_admm_iters"] for n in runs]))
        print("       first window (one-time set-up and the staging of the scenes included), medians: peers %.0f, plan %.0f ego-steps/s"
              % tuple(np.median([x["first_window_ego_steps_per_s"] for x in runs[n]]) for n in runs))
        print("       smallest member-to-member separation over the last window: peers %.3f m, plan %.3f m" % tuple(runs[n][0]["min_separation"] for n in runs))


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(x) for x in s.split(",")]             # noqa: E731
    ap.add_argument("--fleets", type=ints, default=[16, 64])
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=400.0)
    ap.add_argument("--plan", action="store_true", help="the plan rollout beside the constant-velocity peers rollout")
    ap.add_argument("--leg", choices=["host", "peers", "blind", "plan"], default=None, help="(internal) run one measurement in this process and print it as JSON")
    ap.add_argument("--B", type=int, default=16)
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args.leg, args.B, args.K, args.warm)))
        return
    if args.plan:
        plan_table(args)
        return
    print("fleet members that avoid each other, C5 shape with moving scenes (T = %d, N = %d slots, %d moving polygons per ego, lanes %.0f m apart, re-sorted every tick): "
          "timed window of K = %d ticks behind %d host-driven ticks (host loop) or a first window of K ticks (rollouts); %d interleaved repeats"
          % (T, N, N, LANE, args.K, args.warm, args.repeats))
    print("(a) host loop: per tick own obstacles forward + scenarios.peer_obstacles for every member + Fleet.control + the plants, in Python;  "
          "(b) Fleet.rollout(peers=True);  (c) Fleet.rollout(moving=True), a blind fleet")
    print("%4s | %-32s | %-32s | %-32s | %s" % ("B", "(a) host loop ego-steps/s", "(b) peers rollout ego-steps/s", "(c) blind rollout ego-steps/s", "(b) / (a)   (b) / (c)"))
    for B in args.fleets:
        runs = {"host": [], "peers": [], "blind": []}
        for _ in range(args.repeats):
            for name in runs:
                runs[name].append(child(name, B, args))
        rate = {name: [x["ego_steps_per_s"] for x in v] for name, v in runs.items()}
        med = {name: float(np.median(v)) for name, v in rate.items()}
        fmt = lambda v: " ".join("%9.0f" % x for x in v)        # noqa: E731
        print("%4d | %-32s | %-32s | %-32s | %.1fx      %.2fx" % (B, fmt(rate["host"]), fmt(rate["peers"]), fmt(rate["blind"]), med["peers"] / med["host"],
                                                                 med["peers"] / med["blind"]))
        print("       ms per fleet tick (medians): host %.2f, peers %.3f, blind %.3f; mean ADMM iterations per ego-step: host %.3f, peers %.3f, blind %.3f"
              % tuple([np.median([x["ms_per_tick"] for x in runs[n]]) for n in runs] + [runs[n][0]["mean_admm_iters"] for n in runs]))
        print("       first window of the rollouts (one-time set-up and the staging of the scenes included), medians: peers %.0f, blind %.0f ego-steps/s"
              % tuple(np.median([x["first_window_ego_steps_per_s"] for x in runs[n]]) for n in ("peers", "blind")))
        print("       smallest member-to-member separation: host loop (after its last tick) %.3f m, peers rollout (over its last window) %.3f m, blind rollout "
              "(after its last tick) %.3f m" % tuple(runs[n][0]["min_separation"] for n in runs))
        print("       last applied control of ego 0: host %s, peers %s (the host loop's window is %d ticks, the rollout's second window ends at tick %d)"
              % (runs["host"][0]["u_last"], runs["peers"][0]["u_last"], args.warm + args.K, 2 * args.K))


if __name__ == "__main__":
    main()
