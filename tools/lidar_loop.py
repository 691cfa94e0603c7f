"""Lidar front end: host (`lidar.scan_box`, numpy) against device (`rda_scan_boxes` / `rda_upload_scan`, csrc/lidar_device.h).

  1. the front end alone, on scans ray-cast by rda_planner_amd.world in random scenes (circles and rotated boxes around the robot) at 100, 360,
     1080 and 2048 beams: per scan the host `scan_box`, the C call `rda_scan_boxes` (wall clock, its synchronisation included), the Python
     drop-in `lidar.scan_box_device`, and the hipEvent time of the scan kernel (a run of its own: `rda_timing_reset(h, 1)`, launches 3).
     Median over the scans after a warm-up pass, repeated --repeats times.
  2. the closed loop of examples/lidar_path_track_headless.py (tests/golden/world_lidar_track.yaml) driven three ways: host front end,
     `scan_box_device` + obstacle list, `MPC.control(scan=)`; at the world's own 100 beams and at --loop-beams.

    python tools/lidar_loop.py [--scans 50] [--repeats 3] [--steps 150] [--beams 100,360,1080,2048] [--loop-beams 1080]
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
            u, info = mpc.control(env.robot.state, 4, lidar.scan_box(env.robot.state, scan))
        elif mode == "scan_box_device":
            u, info = mpc.control(env.robot.state, 4, lidar.scan_box_device(mpc, env.robot.state, scan))
        else:
            u, info = mpc.control(env.robot.state, 4, scan=scan)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--beams", type=lambda s: [int(x) for x in s.split(",")], default=[100, 360, 1080, 2048])
    ap.add_argument("--loop-beams", type=int, default=1080)
    ap.add_argument("--skip-loops", action="store_true")
    args = ap.parse_args()
    assert args.scans >= 8
    front_end(args)
    if not args.skip_loops:
        loops(args)


if __name__ == "__main__":
    main()
