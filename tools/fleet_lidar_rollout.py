"""The simulated lidar of a fleet on the device, against the host code it replaces.  Two tables (output: profiles/fleet_lidar_rollout.txt):

  (a) the sensor alone, per scan: Fleet.raycast (rda_fleet_raycast: lidar::k_raycast_fleet, one launch for the fleet, one wait) against the loop of
      World.get_lidar_scan over the members, at B = 16 / 64, 360 / 1080 beams and 50 / 200 world obstacles per member (circles and rectangles);
  (b) the closed loop, in ego-steps/s: Fleet.rollout(lidar=, world=) (rda_fleet_rollout_lidar: K ticks, one wait for the B box counts per tick) against the
      host loop World.get_lidar_scan -> Fleet.control(scans=) -> World.step on the same members, K = 100 ticks.

Every member has a world of its own (obstacles on both sides of its straight path, none on it) and a full-turn lidar of 15 m.  The baseline is the host loop
on the same box; medians over --repeats.

--see-peers (output: profiles/fleet_lidar_rollout_peers.txt): the members that see each other against the blind ones.  The same fleet for both - member k
on a lane of its own, LANE m from the next, so that a 15 m lidar reaches the neighbours - and the same windows, the repeats interleaved:

  (c) the sensor alone, ms per call (one launch, one wait): Fleet.raycast (lidar::k_raycast_fleet) | Fleet.raycast_peers (lidar::k_raycast_fleet_peers);
  (d) the closed loop of K ticks, in ego-steps/s: Fleet.rollout(lidar=, world=) | the same with see_peers=True.

--track (output: profiles/fleet_lidar_rollout_track.txt): the rollout that tracks its boxes against the one that does not, the same scene for both (a
world per member, as in (b)), the repeats interleaved:

  (e) the closed loop of K ticks, in ego-steps/s: Fleet.rollout(lidar=, world=) | the same with track=True.  The baseline is the untracked rollout.  A
      tracked tick has one launch more (lidar::k_track_boxes_fleet, behind the scan kernel) and builds and solves slots for T + 1 stages instead of one.
      The tracker's own time per launch comes from a run under `rocprofv3 --kernel-trace --stats` (--track --profile-run: one short tracked rollout).

    python tools/fleet_lidar_rollout.py [--fleets 16,64] [--beams 360,1080] [--obstacles 50,200] [--K 100] [--repeats 3] [--see-peers | --track [--profile-run] | --split TOL [--corridor] [--profile-run]]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
T, N = 10, 10
LANE = 10.0             # --see-peers: metres between two members' lanes


def world(k, beams, n_obs, y0=20.0):
    """member k's world: a robot at the head of the line (0, y0) -> (60, y0), n_obs circles and rectangles 4 .. 12 m to both sides of it"""
    from rda_planner_amd import world as irsim
    rng = np.random.default_rng(71000 + k)
    obstacles = []
    for j in range(n_obs):
        side = 1.0 if j % 2 else -1.0
        pos = [float(rng.uniform(2.0, 70.0)), y0 + side * float(rng.uniform(4.0, 12.0)), float(rng.uniform(-np.pi, np.pi))]
        shape = {"name": "circle", "radius": float(rng.uniform(0.3, 0.8))} if j % 3 == 0 else \
                {"name": "rectangle", "length": float(rng.uniform(0.5, 2.0)), "width": float(rng.uniform(0.3, 1.2))}
        obstacles.append({"number": 1, "distribution": {"name": "manual"}, "state": [pos], "shape": [shape]})
    cfg = {"world": {"step_time": 0.1, "width": 100, "height": max(100, y0 + 50)},
           "robot": [{"kinematics": {"name": "acker"}, "shape": {"name": "rectangle", "length": 4.6, "width": 1.6, "wheelbase": 3}, "state": [1.0, y0, 0.0],
                      "sensors": [{"type": "lidar2d", "range_max": 15.0, "angle_range": 2 * np.pi - 0.01, "number": beams}]}],
           "obstacle": obstacles}
    return irsim.World(cfg)


def fleet(B, beams, n_obs, lane=0.0):
    """lane: metres between the members' lanes (0: every member in a world of its own at the same place)"""
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    ys = [20.0 + lane * k for k in range(B)]
    envs = [world(k, beams, n_obs, y) for k, y in enumerate(ys)]
    ms = [MPC(sc.rectangle_robot(), sc.line_path([0, y, 0], [90, y, 0]), receding=T, max_edge_num=4, max_obs_num=N, iter_num=2) for y in ys]
    return Fleet(ms), envs


def sensor_table(args):
    print("(a) one scan of every member, ms per fleet scan (medians of %d): World.get_lidar_scan in a loop | Fleet.raycast" % args.repeats)
    print("%4s %6s %9s | %12s | %12s | %s" % ("B", "beams", "obstacles", "host loop", "Fleet.raycast", "host / device"))
    for B in args.fleets:
        for beams in args.beams:
            for n_obs in args.obstacles:
                f, envs = fleet(B, beams, n_obs)
                f.upload_worlds([e.obstacles for e in envs])
                states, sensors = [e.robot.state for e in envs], [e.lidar for e in envs]
                dev = f.raycast(states, sensors)                                   # first use: the ranges buffer
                host = [e.get_lidar_scan() for e in envs]
                worst = max(float(np.abs(d["ranges"] - h["ranges"]).max()) for d, h in zip(dev, host))
                th, td = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter(); [e.get_lidar_scan() for e in envs]; th.append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); f.raycast(states, sensors); td.append(time.perf_counter() - t0)
                print("%4d %6d %9d | %12.3f | %12.3f | %7.1fx   (largest |device - host| %.1e m)"
                      % (B, beams, n_obs, 1e3 * np.median(th), 1e3 * np.median(td), np.median(th) / np.median(td), worst))
                f.close()


def loop_table(args):
    beams, n_obs, K = args.beams[0], args.obstacles[0], args.K
    print("(b) closed loop of K = %d ticks, %d beams, %d world obstacles per member, ego-steps/s (medians of %d): get_lidar_scan -> Fleet.control(scans=) -> "
          "World.step | Fleet.rollout(lidar=, world=)" % (K, beams, n_obs, args.repeats))
    print("%4s | %12s | %12s | %s" % ("B", "host loop", "rollout", "rollout / host loop"))
    for B in args.fleets:
        ra, rb = [], []
        for _ in range(args.repeats):
            f, envs = fleet(B, beams, n_obs)
            t0 = time.perf_counter()
            for _k in range(K):
                res = f.control([e.robot.state.copy() for e in envs], 4.0, scans=[e.get_lidar_scan() for e in envs])
                for e, (u, _info) in zip(envs, res):
                    e.step(u)
            ra.append(B * K / (time.perf_counter() - t0))
            f.close()
            f, envs = fleet(B, beams, n_obs)
            kw = dict(lidar=[e.lidar for e in envs], world=[e.obstacles for e in envs])
            out = f.rollout([e.robot.state.copy() for e in envs], 4.0, 2, **kw)    # first use: tables, logs and the members' raw scenes
            t0 = time.perf_counter()
            out = f.rollout([out["states"][-1, i].reshape(3, 1) for i in range(B)], 4.0, K, lidar=kw["lidar"])
            rb.append(B * K / (time.perf_counter() - t0))
            f.close()
        print("%4d | %12.0f | %12.0f | %.1fx   (boxes seen per tick and member: %.1f)" % (B, np.median(ra), np.median(rb), np.median(rb) / np.median(ra), out["boxes"].mean()))


def peers_tables(args):
    n_obs, K, calls = args.obstacles[0], args.K, 20
    print("(c) one scan of every member, %d world obstacles per member, lanes %g m apart, ms per call = one launch + one wait (medians of %d x %d calls, "
          "interleaved): Fleet.raycast | Fleet.raycast_peers" % (n_obs, LANE, args.repeats, calls))
    print("%4s %6s | %12s | %12s | %s" % ("B", "beams", "blind", "seeing", "seeing / blind"))
    for B in args.fleets:
        for beams in args.beams:
            f, envs = fleet(B, beams, n_obs, LANE)
            f.upload_worlds([e.obstacles for e in envs])
            states, sensors = [e.robot.state for e in envs], [e.lidar for e in envs]
            blind, seeing = f.raycast(states, sensors), f.raycast_peers(states, sensors)      # first use: the ranges buffer, the peer table
            hit = sum(int((s["ranges"] < b["ranges"]).sum()) for s, b in zip(seeing, blind))
            tb, ts = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter(); [f.raycast(states, sensors) for _c in range(calls)]; tb.append((time.perf_counter() - t0) / calls)
                t0 = time.perf_counter(); [f.raycast_peers(states, sensors) for _c in range(calls)]; ts.append((time.perf_counter() - t0) / calls)
            print("%4d %6d | %12.3f | %12.3f | %.2fx   (beams that end on a member: %d of %d)"
                  % (B, beams, 1e3 * np.median(tb), 1e3 * np.median(ts), np.median(ts) / np.median(tb), hit, B * beams))
            f.close()
    print()
    print("(d) closed loop of K = %d ticks, %d world obstacles per member, lanes %g m apart, ego-steps/s (medians of %d, interleaved): "
          "Fleet.rollout(lidar=, world=) | ... see_peers=True" % (K, n_obs, LANE, args.repeats))
    print("%4s %6s | %12s | %12s | %s" % ("B", "beams", "blind", "seeing", "seeing / blind"))
    for B in args.fleets:
        for beams in args.beams:
            rate, boxes, sep = {False: [], True: []}, {}, None
            for _ in range(args.repeats):
                for see in (False, True):
                    f, envs = fleet(B, beams, n_obs, LANE)
                    kw = dict(lidar=[e.lidar for e in envs], world=[e.obstacles for e in envs], see_peers=see)
                    out = f.rollout([e.robot.state.copy() for e in envs], 4.0, 2, **kw)    # first use: tables, logs and the members' raw scenes
                    t0 = time.perf_counter()
                    out = f.rollout([out["states"][-1, i].reshape(3, 1) for i in range(B)], 4.0, K, lidar=kw["lidar"], see_peers=see)
                    rate[see].append(B * K / (time.perf_counter() - t0))
                    boxes[see] = out["boxes"].mean()
                    if see:
                        sep = out["peer_clearance"].min()
                    f.close()
            print("%4d %6d | %12.0f | %12.0f | %.2fx   (boxes per tick and member: %.1f | %.1f; least member-to-member separation %.2f m)"
                  % (B, beams, np.median(rate[False]), np.median(rate[True]), np.median(rate[True]) / np.median(rate[False]), boxes[False], boxes[True], sep))


def track_table(args):
    n_obs, K = args.obstacles[0], args.K
    if args.profile_run:                                                         # for the profiler: one fleet, one short tracked rollout, no timing
        B, beams = args.fleets[-1], args.beams[-1]
        f, envs = fleet(B, beams, n_obs)
        out = f.rollout([e.robot.state.copy() for e in envs], 4.0, K, lidar=[e.lidar for e in envs], world=[e.obstacles for e in envs], track=True)
        print("tracked rollout of K = %d ticks, B = %d, %d beams: boxes per tick and member %.1f" % (K, B, beams, out["boxes"].mean()))
        f.close()
        return
    print("(e) closed loop of K = %d ticks, %d world obstacles per member, ego-steps/s (medians of %d, interleaved): Fleet.rollout(lidar=, world=) | "
          "... track=True" % (K, n_obs, args.repeats))
    print("%4s %6s | %12s | %12s | %s" % ("B", "beams", "untracked", "tracked", "tracked / untracked"))
    for B in args.fleets:
        for beams in args.beams:
            rate, boxes, tracks, fast = {False: [], True: []}, {}, 0.0, 0.0
            for _ in range(args.repeats):
                for track in (False, True):
                    f, envs = fleet(B, beams, n_obs)
                    kw = dict(lidar=[e.lidar for e in envs], world=[e.obstacles for e in envs], track=track)
                    out = f.rollout([e.robot.state.copy() for e in envs], 4.0, 2, **kw)    # first use: tables, logs and the members' raw scenes
                    t0 = time.perf_counter()
                    out = f.rollout([out["states"][-1, i].reshape(3, 1) for i in range(B)], 4.0, K, lidar=kw["lidar"], track=track)
                    rate[track].append(B * K / (time.perf_counter() - t0))
                    boxes[track] = out["boxes"].mean()
                    if track:
                        tb = f.box_tracks()
                        tracks = float(np.mean([len(t["age"]) for t in tb]))
                        fast = float(np.mean([(np.hypot(t["velocities"][:, 0], t["velocities"][:, 1]) > 0.01).mean() if len(t["age"]) else 0.0 for t in tb]))
                    f.close()
            print("%4d %6d | %12.0f | %12.0f | %.2fx   (boxes per tick and member: %.1f | %.1f; tracks per member after the run %.1f, of them predicted %.0f%%)"
                  % (B, beams, np.median(rate[False]), np.median(rate[True]), np.median(rate[True]) / np.median(rate[False]), boxes[False], boxes[True],
                     tracks, 100 * fast))


def corridor_fleet(B, beams):
    """every member in the L-shaped corridor of tests/golden/world_lidar_corridor.yaml, 5 m before the bend, on a path round it"""
    import yaml
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd import world as irsim
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    with open(os.path.join(ROOT, "tests", "golden", "world_lidar_corridor.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    cfg["robot"][0]["sensors"][0]["number"] = beams
    cfg["robot"][0]["state"] = [25.0, 0.0, 0.0]
    envs = [irsim.World(cfg) for _ in range(B)]
    car = sc.rectangle_robot(1.0, 0.6, 0, "diff", max_speed=(2, 1), max_acce=(2, 1))
    path = sc.line_path([25, 0, 0], [30, 0, 0]) + sc.line_path([30, 0, np.pi / 2], [30, 20, np.pi / 2])[1:]
    ms = [MPC(car, [p.copy() for p in path], receding=T, max_edge_num=4, max_obs_num=N, iter_num=2) for _ in range(B)]
    return Fleet(ms), envs


def split_table(args):
    """(f) the rollout with the clusters split into straight runs (scan_split=TOL) against the one box per cluster, interleaved"""
    n_obs, K, tol = args.obstacles[0], args.K, args.split
    speed = 2.0 if args.corridor else 4.0
    if args.profile_run:                                                         # for the profiler: one fleet, one rollout, no timing
        B, beams = args.fleets[-1], args.beams[-1]
        f, envs = corridor_fleet(B, beams) if args.corridor else fleet(B, beams, n_obs)
        kw = dict(scan_split=tol) if tol > 0 else {}
        out = f.rollout([e.robot.state.copy() for e in envs], speed, K, lidar=[e.lidar for e in envs], world=[e.obstacles for e in envs], **kw)
        print("rollout of K = %d ticks, B = %d, %d beams, split %g: boxes per tick and member %.1f" % (K, B, beams, tol, out["boxes"].mean()))
        f.close()
        return
    print("(f) closed loop of K = %d ticks, %s, ego-steps/s (medians of %d, interleaved): Fleet.rollout(lidar=, world=) | ... scan_split=%g"
          % (K, "the L-shaped corridor" if args.corridor else "%d world obstacles per member" % n_obs, args.repeats, tol))
    print("%4s %6s | %12s | %12s | %s" % ("B", "beams", "unsplit", "split", "split / unsplit"))
    for B in args.fleets:
        for beams in args.beams:
            rate, boxes = {False: [], True: []}, {}
            for _ in range(args.repeats):
                for on in (False, True):
                    f, envs = corridor_fleet(B, beams) if args.corridor else fleet(B, beams, n_obs)
                    kw = dict(lidar=[e.lidar for e in envs], world=[e.obstacles for e in envs], **(dict(scan_split=tol) if on else {}))
                    out = f.rollout([e.robot.state.copy() for e in envs], speed, 2, **kw)  # first use: tables, logs and the members' raw scenes
                    kw.pop("world")
                    t0 = time.perf_counter()
                    out = f.rollout([out["states"][-1, i].reshape(3, 1) for i in range(B)], speed, K, **kw)
                    rate[on].append(B * K / (time.perf_counter() - t0))
                    boxes[on] = out["boxes"].mean()
                    f.close()
            print("%4d %6d | %12.0f | %12.0f | %.2fx   (boxes per tick and member: %.1f | %.1f)"
                  % (B, beams, np.median(rate[False]), np.median(rate[True]), np.median(rate[True]) / np.median(rate[False]), boxes[False], boxes[True]))


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(x) for x in s.split(",")]             # noqa: E731
    ap.add_argument("--fleets", type=ints, default=[16, 64])
    ap.add_argument("--beams", type=ints, default=[360, 1080])
    ap.add_argument("--obstacles", type=ints, default=[50, 200])
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--see-peers", action="store_true", help="the members that see each other against the blind ones (tables c, d)")
    ap.add_argument("--track", action="store_true", help="the rollout that tracks its boxes against the one that does not (table e)")
    ap.add_argument("--profile-run", action="store_true", help="with --track / --split: one short rollout of that kind and nothing else, for a profiler")
    ap.add_argument("--split", type=float, default=None, metavar="TOL",
                    help="the rollout that splits its clusters into straight runs at TOL metres against the one that does not (table f); with --profile-run, 0 = unsplit")
    ap.add_argument("--corridor", action="store_true", help="with --split: every member in the L-shaped corridor instead of the obstacle field")
    args = ap.parse_args()
    if args.split is not None:
        split_table(args)
        return
    if args.see_peers:
        peers_tables(args)
        return
    if args.track:
        track_table(args)
        return
    sensor_table(args)
    print()
    loop_table(args)


if __name__ == "__main__":
    main()
