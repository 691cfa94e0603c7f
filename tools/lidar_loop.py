"""Lidar front end: host (`lidar.scan_box`, numpy) against device (`rda_scan_boxes` / `rda_upload_scan`, csrc/lidar_device.h).

  1. the front end alone, on scans ray-cast by rda_planner_amd.world in random scenes (circles and rotated boxes around the robot) at 100, 360,
     1080 and 2048 beams: per scan the host `scan_box`, the C call `rda_scan_boxes` (wall clock, its synchronisation included), the Python
     drop-in `lidar.scan_box_device`, and the hipEvent time of the scan kernel (a run of its own: `rda_timing_reset(h, 1)`, launches 3).
     Median over the scans after a warm-up pass, repeated --repeats times.
  2. the closed loop of examples/lidar_path_track_headless.py (tests/golden/world_lidar_track.yaml) driven three ways: host front end,
     `scan_box_device` + obstacle list, `MPC.control(scan=)`; at the world's own 100 beams and at --loop-beams.

  3. --fleet B: a fleet of B planners that each carry a lidar.  Per tick, on the same members, in the same process, with the same scans:
     (a) the loop of B `rda_upload_scan` calls followed by `rda_fleet_sync`, (b) ONE `rda_fleet_upload_scans` followed by `rda_fleet_sync`
     (wall clock of the C calls, median over the ticks after a warm-up pass, --repeats times), at --fleet-beams; then a short
     `Fleet.control(scans=)` closed loop in ego-steps/s.  With --fleet only this part runs.

    python tools/lidar_loop.py [--scans 50] [--repeats 3] [--steps 150] [--beams 100,360,1080,2048] [--loop-beams 1080]
    python tools/lidar_loop.py --fleet 16,64 [--fleet-beams 360,1080] [--fleet-ticks 30] [--fleet-steps 40]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from rda_planner_amd import lidar                               # noqa: E402
from rda_planner_amd import scenarios as sc                     # noqa: E402
from rda_planner_amd import world as irsim                      # noqa: E402
from rda_planner_amd._capi import dptr, iptr                    # noqa: E402
from rda_planner_amd.mpc import MPC                             # noqa: E402


def random_scan(seed, beams):
    """(state, scan) seen from a random pose among 8-13 circles and rotated boxes, 15 m range, full or half field of view"""
    rng = np.random.default_rng(seed)
    state = [float(rng.uniform(10, 40)), float(rng.uniform(10, 40)), float(rng.uniform(-np.pi, np.pi))]
    obstacles = []
    for _ in range(int(rng.integers(8, 14))):
        d, a = rng.uniform(3.0, 14.0), rng.uniform(-np.pi, np.pi)
        pos = [state[0] + d * np.cos(a), state[1] + d * np.sin(a), float(rng.uniform(-np.pi, np.pi))]
        shape = {"name": "circle", "radius": float(rng.uniform(0.3, 1.5))} if rng.random() < 0.4 else \
                {"name": "rectangle", "length": float(rng.uniform(0.5, 5.0)), "width": float(rng.uniform(0.3, 2.5))}
        obstacles.append({"number": 1, "distribution": {"name": "manual"}, "state": [pos], "shape": [shape]})
    fov = np.pi if seed % 2 else 2 * np.pi - 0.01
    cfg = {"world": {"step_time": 0.1},
           "robot": [{"kinematics": {"name": "acker"}, "shape": {"name": "rectangle", "length": 4.6, "width": 1.6, "wheelbase": 3}, "state": state,
                      "sensors": [{"type": "lidar2d", "range_max": 15.0, "angle_range": fov, "number": beams}]}],
           "obstacle": obstacles}
    env = irsim.World(cfg)
    return env.robot.state.copy(), env.get_lidar_scan()


def median_ms(fn, items, repeats):
    """[median over items of the wall clock of fn(item), in ms] per repeat, after one warm-up pass"""
    for it in items[:8]:
        fn(it)
    out = []
    for _ in range(repeats):
        ts = []
        for it in items:
            t0 = time.perf_counter()
            fn(it)
            ts.append(time.perf_counter() - t0)
        out.append(1e3 * float(np.median(ts)))
    return out


def front_end(args):
    mpc = MPC(sc.rectangle_robot(), sc.line_path([0, 20, 0], [60, 20, 0]), receding=10, max_edge_num=4, max_obs_num=5, iter_num=2)
    api, h = mpc.rda._be.api, mpc.rda._be.handle
    lib = api.lib
    print("front end alone: ms per scan, median over %d scans, %d repeats" % (args.scans, args.repeats))
    print("%6s %6s %6s | %-26s | %-26s | %-26s | %-26s" % ("beams", "hits", "boxes", "host scan_box", "rda_scan_boxes (C call)", "scan_box_device (Python)",
                                                             "k_scan (hipEvent)"))
    fmt = lambda v: " ".join("%8.4f" % x for x in v)            # noqa: E731
    verdicts = []
    for beams in args.beams:
        items = [random_scan(9000 + k, beams) for k in range(args.scans)]
        hits = [int((np.asarray(s["ranges"]) < s["range_max"] - 0.01).sum()) for _, s in items]
        packed = []
        for state, scan in items:
            r = np.ascontiguousarray(np.asarray(scan["ranges"], float))
            st = np.ascontiguousarray(state.ravel()[0:3])
            packed.append((r, st, float(scan["angle_min"]), float(scan["angle_max"]), float(scan["range_max"])))
        boxes, n, labels = np.zeros((beams, 4, 2)), np.zeros(1, np.int32), np.zeros(beams, np.int32)

        def c_call(p):
            rc = api.scan_boxes(h, len(p[0]), dptr(p[0]), p[2], p[3], p[4], dptr(p[1]), 2.0, 6, iptr(n), dptr(boxes), beams, iptr(labels))
            assert rc == 0, rc
        nbox = []
        for p, (state, scan) in zip(packed, items):                 # same boxes on both sides before anything is timed
            c_call(p)
            nbox.append(int(n[0]))
            assert int(n[0]) == len(lidar.scan_box(state, scan))
        t_host = median_ms(lambda it: lidar.scan_box(it[0], it[1]), items, args.repeats)
        t_c = median_ms(c_call, packed, args.repeats)
        t_py = median_ms(lambda it: lidar.scan_box_device(mpc, it[0], it[1]), items, args.repeats)
        t_ev = []
        for _ in range(args.repeats):
            per = []
            for p in packed:
                lib.rda_timing_reset(h, 1)
                c_call(p)
                ms, k = np.zeros(1), np.zeros(1, np.int32)
                assert lib.rda_timing_read(h, 3, dptr(ms), iptr(k)) == 0 and k[0] == 1
                per.append(float(ms[0]))
            lib.rda_timing_reset(h, 0)
            t_ev.append(float(np.median(per)))
        print("%6d %6d %6.1f | %s | %s | %s | %s" % (beams, int(np.median(hits)), float(np.mean(nbox)), fmt(t_host), fmt(t_c), fmt(t_py), fmt(t_ev)))
        verdicts.append((beams, max(t_c) < min(t_host), min(t_host) / max(t_c)))
    for beams, faster, ratio in verdicts:
        print("  %5d beams: device call %s than the host front end in every repeat (slowest device median vs fastest host median: %.1fx)"
              % (beams, "FASTER" if faster else "NOT faster", ratio))


def closed_loop(mode, beams, steps):
    env = irsim.make(os.path.join(ROOT, "tests", "golden", "world_lidar_track.yaml"))
    if beams:
        env.lidar.number = beams
    ri = env.get_robot_info()
    car = sc.car(ri.G, ri.h, ri.cone_type, ri.wheelbase, [10, 1], [10, 0.5], "acker")
    mpc = MPC(car, sc.path_track_ref(), receding=10, sample_time=env.step_time, process_num=4, iter_num=2, max_edge_num=4, max_obs_num=4,
              obstacle_order=True, wu=1.0, slack_gain=13)
    t_plan, done = 0.0, 0
    t0 = time.perf_counter()
    for i in range(steps):
        scan = env.get_lidar_scan()
        t1 = time.perf_counter()
        if mode == "host":
            u, info = mpc.control(env.robot.state, 4, lidar.scan_box_split(env.robot.state, scan, tol=SPLIT) if SPLIT else lidar.scan_box(env.robot.state, scan))
        elif mode == "scan_box_device":
            u, info = mpc.control(env.robot.state, 4, lidar.scan_box_split_device(mpc, env.robot.state, scan, tol=SPLIT) if SPLIT
                                  else lidar.scan_box_device(mpc, env.robot.state, scan))
        else:
            u, info = mpc.control(env.robot.state, 4, scan=scan, **({"scan_split": SPLIT} if SPLIT else {}))
        t_plan += time.perf_counter() - t1
        env.step(u)
        done += 1
        if env.done() or info["arrive"]:
            break
    wall = time.perf_counter() - t0
    return done, done / wall, 1e3 * t_plan / done


def loops(args):
    print("closed loop of the lidar example (world_lidar_track.yaml; the ray-cast world and the plant run on the host in every mode)")
    print("%6s %-18s %6s %12s %28s" % ("beams", "front end", "steps", "steps/s", "front end + control ms/step"))
    for beams in (0, args.loop_beams):
        for mode in ("host", "scan_box_device", "scan="):
            closed_loop(mode, beams, 10)                            # warm-up: first launches, allocations
            n, rate, ms = closed_loop(mode, beams, args.steps)
            print("%6d %-18s %6d %12.0f %28.3f" % (beams or 100, mode, n, rate, ms))


def fleet_world(k, beams):
    """member k's world: the robot near the head of the line path (0, 20) -> (60, 20), circles and boxes on both sides of the path ahead"""
    rng = np.random.default_rng(7000 + k)
    state = [1.0 + 0.05 * (k % 16), 20.0 + 0.05 * (k // 16), 0.01 * (k % 5)]
    obstacles = []
    for j in range(8):
        pos = [7.0 + 4.0 * j + float(rng.uniform(-1, 1)), 20.0 + (4.5 if j % 2 else -4.5) + float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-np.pi, np.pi))]
        shape = {"name": "circle", "radius": 1.0} if j % 3 == 0 else {"name": "rectangle", "length": 2.5, "width": 1.2}
        obstacles.append({"number": 1, "distribution": {"name": "manual"}, "state": [pos], "shape": [shape]})
    cfg = {"world": {"step_time": 0.1},
           "robot": [{"kinematics": {"name": "acker"}, "shape": {"name": "rectangle", "length": 4.6, "width": 1.6, "wheelbase": 3}, "state": state,
                      "sensors": [{"type": "lidar2d", "range_max": 15.0, "angle_range": np.pi, "number": beams}]}],
           "obstacle": obstacles}
    return irsim.World(cfg)


def fleet_part(args):
    from rda_planner_amd.fleet import Fleet
    fmt = lambda v: " ".join("%8.4f" % x for x in v)            # noqa: E731
    print("fleet lidar: ms per fleet tick (all B scans staged and the fleet synchronised), median over %d ticks, %d repeats" % (args.fleet_ticks, args.repeats))
    print("%4s %6s %6s | %-30s | %-30s | %s" % ("B", "beams", "boxes", "(a) B x rda_upload_scan + sync", "(b) rda_fleet_upload_scans + sync", "(a) / (b)"))
    verdicts, cache = [], {}
    for B in args.fleet:
        memb = [MPC(sc.rectangle_robot(), sc.line_path([0, 20, 0], [60, 20, 0]), receding=10, max_edge_num=4, max_obs_num=5, iter_num=2) for _ in range(B)]
        fleet = Fleet(memb)
        api, fh = fleet.api, fleet._handle
        handles = [m.rda._be.handle for m in memb]
        for beams in args.fleet_beams:
            if beams not in cache:                                  # per tick: 16 (state, scan) from random poses in random scenes
                cache[beams] = [[random_scan(20000 + 97 * t + k, beams) for k in range(16)] for t in range(args.fleet_ticks)]
            ticks = cache[beams]
            packed = []
            for items in ticks:
                items = [items[i % len(items)] for i in range(B)]   # (B > 16: the scans repeat, the work per scan does not change)
                rs = [np.ascontiguousarray(np.asarray(s["ranges"], float)) for _, s in items]
                nb = np.full(B, beams, np.int32)
                allr = np.ascontiguousarray(np.concatenate(rs))
                lo, hi, rmax = (np.array([float(s[k]) for _, s in items]) for k in ("angle_min", "angle_max", "range_max"))
                st = np.ascontiguousarray(np.array([x.ravel()[0:3] for x, _ in items]))
                packed.append((rs, nb, allr, lo, hi, rmax, st))
            order, n1, nB = np.ones(B, np.int32), np.zeros(1, np.int32), np.zeros(B, np.int32)

            def looped(p):
                rs, nb, allr, lo, hi, rmax, st = p
                for i in range(B):
                    rc = api.upload_scan(handles[i], beams, dptr(rs[i]), lo[i], hi[i], rmax[i], dptr(st[i]), 2.0, 6, 1, iptr(n1))
                    assert rc == 0, rc
                assert api.fleet_sync(fh) == 0                      # (a member's staging still queued on its own stream is waited for by its next scan)

            def batched(p):
                rs, nb, allr, lo, hi, rmax, st = p
                rc = api.fleet_upload_scans(fh, iptr(nb), dptr(allr), dptr(lo), dptr(hi), dptr(rmax), dptr(st), 2.0, 6, iptr(order), iptr(nB))
                assert rc == 0, rc
                assert api.fleet_sync(fh) == 0
            t_a = median_ms(looped, packed, args.repeats)
            t_b = median_ms(batched, packed, args.repeats)
            print("%4d %6d %6.1f | %-30s | %-30s | %.1fx" % (B, beams, float(nB.mean()), fmt(t_a), fmt(t_b), np.median(t_a) / np.median(t_b)))
            verdicts.append((B, beams, max(t_b) < min(t_a), min(t_a) / max(t_b)))
        fleet.close()
    for B, beams, faster, ratio in verdicts:
        print("  B = %2d, %4d beams: one fleet call %s than the loop of solo calls in every repeat (fastest loop median vs slowest fleet median: %.1fx)"
              % (B, beams, "FASTER" if faster else "NOT faster", ratio))
    print("closed loop Fleet.control(scans=): every member in a world of its own (the ray casting and the plants run on the host and are not counted)")
    print("%4s %6s %6s %14s %22s" % ("B", "beams", "ticks", "ego-steps/s", "Fleet.control ms/tick"))
    for B in args.fleet:
        for beams in args.fleet_beams:
            envs = [fleet_world(k, beams) for k in range(B)]
            memb = [MPC(sc.rectangle_robot(), sc.line_path([0, 20, 0], [60, 20, 0]), receding=10, max_edge_num=4, max_obs_num=5, iter_num=2) for _ in range(B)]
            fleet = Fleet(memb)
            per = []
            for t in range(args.fleet_steps + 5):
                states = [e.robot.state.copy() for e in envs]
                scans = [e.get_lidar_scan() for e in envs]
                t0 = time.perf_counter()
                res = fleet.control(states, 4.0, scans=scans, **({"scan_split": SPLIT} if SPLIT else {}))
                if t >= 5:                                          # (warm-up: first launches, allocations)
                    per.append(time.perf_counter() - t0)
                for e, (u, _) in zip(envs, res):
                    e.step(u)
            ms = 1e3 * float(np.median(per))
            print("%4d %6d %6d %14.0f %22.3f" % (B, beams, len(per), B / (1e-3 * ms), ms))
            fleet.close()


SPLIT = 0.0             # --split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--beams", type=lambda s: [int(x) for x in s.split(",")], default=[100, 360, 1080, 2048])
    ap.add_argument("--loop-beams", type=int, default=1080)
    ap.add_argument("--skip-loops", action="store_true")
    ints = lambda s: [int(x) for x in s.split(",")]             # noqa: E731
    ap.add_argument("--fleet", type=ints, default=[], help="fleet sizes, e.g. 16,64: time the fleet lidar instead of parts 1 and 2")
    ap.add_argument("--fleet-beams", type=ints, default=[360, 1080])
    ap.add_argument("--fleet-ticks", type=int, default=30)
    ap.add_argument("--fleet-steps", type=int, default=40)
    ap.add_argument("--split", type=float, default=0.0, metavar="TOL",
                    help="the closed loops (part 2, and the Fleet.control loop of --fleet) with the clusters split into straight runs at TOL metres")
    args = ap.parse_args()
    global SPLIT
    SPLIT = args.split
    if args.fleet:
        assert args.fleet_ticks >= 8 and args.repeats >= 3
        return fleet_part(args)
    assert args.scans >= 8
    front_end(args)
    if not args.skip_loops:
        loops(args)


if __name__ == "__main__":
    main()
