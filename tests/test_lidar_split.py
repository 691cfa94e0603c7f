"""Clusters split into straight runs (lidar.split_runs, lidar.scan_box_split; rda_set_scan_split, rda_fleet_set_scan_split; `scan_split=` of
MPC.control, Fleet.control, Fleet.rollout): what can be checked without a GPU - the rule on crafted sequences, decision by decision; the clearance of the
robot against the staged boxes in the L-shaped corridor of tests/golden/world_lidar_corridor.yaml and in a closed room, with and without the split;
the entry points declared, exported, documented and bound like the header; and the refusals of the Python interface before any library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import yaml

from rda_planner_amd import lidar
from rda_planner_amd import scenarios as sc
from rda_planner_amd import world as irsim

from capi_lib import LIDAR_FLAGS, RDA_ERR_ARG, ROOT, SENSOR, Binding, bare_fleet, header, integration_rows, lib, pipeline_member

CORRIDOR = os.path.join(ROOT, "tests", "golden", "world_lidar_corridor.yaml")
TOL_SPLIT = 0.15


def corridor_cfg():
    with open(CORRIDOR) as f:
        return yaml.safe_load(f)


def room_cfg():
    """a closed room, 12 x 8 m between the wall centre lines, about the origin; the corridor's robot and lidar"""
    cfg = corridor_cfg()
    cfg["obstacle"][0]["shape"] = [{"name": "polygon", "vertices": v} for v in (
        [[-6.15, -4.15], [6.15, -4.15], [6.15, -3.85], [-6.15, -3.85]], [[5.85, -3.85], [6.15, -3.85], [6.15, 3.85], [5.85, 3.85]],
        [[-6.15, 3.85], [6.15, 3.85], [6.15, 4.15], [-6.15, 4.15]], [[-6.15, -3.85], [-5.85, -3.85], [-5.85, 3.85], [-6.15, 3.85]])]
    return cfg


def world_at(cfg, pose, beams=None):
    if beams is not None:
        cfg["robot"][0]["sensors"][0]["number"] = beams
    env = irsim.World(cfg)
    env.robot.state = np.array(pose, float).reshape(3, 1)
    return env


# the five poses of the table in DESIGN.md: (world, pose)
POSES = [(corridor_cfg(), (20, 0.5, 0.1)), (corridor_cfg(), (29, 0, 0.6)), (corridor_cfg(), (30, 5, 1.57)), (room_cfg(), (0, 0, 0)), (room_cfg(), (3, 1, 0.7))]


def _runs(points, labels=None, eps=2.0, tol=TOL_SPLIT):
    P = np.asarray(points, float)
    return lidar.split_runs(P, np.zeros(len(P), int) if labels is None else np.asarray(labels), eps, tol).tolist()


# ---- the rule, decision by decision ---------------------------------------------------------------------------------------------------------------
def test_a_straight_run_is_one_segment_and_an_l_starts_its_second_run_at_the_corner():
    assert _runs([[k, 0.0] for k in range(7)]) == [0] * 7
    assert _runs([[k, 0.001 * (k % 2)] for k in range(7)]) == [0] * 7                      # within tol
    L = [[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [3, 2], [3, 3]]
    assert _runs(L) == [0, 0, 0, 1, 1, 1, 1]                                                # the corner (3, 0) is the first point of run 1
    assert len(set(zip(_runs(L), range(7)))) == 7                                           # no point in two runs


def test_two_equal_maxima_the_lowest_index_wins():
    P = [[0, 0], [1, 1], [2, 0.5], [3, 1], [4, 0]]                                          # s is equal at indices 1 and 3
    s, _ = lidar.end_point_fit(np.array(P, float)[:, 0], np.array(P, float)[:, 1], 0, 4, TOL_SPLIT ** 2)
    assert s[0] == s[2] == s.max()
    seg = _runs(P)
    assert seg[0] == 0 and seg[1] == 1                                                      # split at index 1, not at 3


def test_deviation_exactly_at_tol_does_not_split_one_ulp_above_does():
    # chord (0,0)-(4,0): L2 = 16, s = (h * 4)^2, bound = tol^2 * 16; with tol = 0.25 and h = 0.25 both sides are 1.0 exactly
    tol = 0.25
    assert _runs([[0, 0], [2, tol], [4, 0]], eps=10.0, tol=tol) == [0, 0, 0]                          # the test is >, not >=
    assert _runs([[0, 0], [2, np.nextafter(tol, 1.0)], [4, 0]], eps=10.0, tol=tol) == [0, 1, 1]
    assert _runs([[0, 0], [2, -np.nextafter(tol, 1.0)], [4, 0]], eps=10.0, tol=tol) == [0, 1, 1]      # either side of the chord


def test_neighbour_distance_exactly_eps_stays_one_ulp_beyond_ends_the_run():
    eps = 2.0
    assert _runs([[0, 0], [1, 0], [3, 0], [4, 0]], eps=eps) == [0, 0, 0, 0]                 # dx * dx = 4 <= eps * eps
    far = np.nextafter(3.0, 4.0)
    assert (far - 1.0) ** 2 > eps * eps
    assert _runs([[0, 0], [1, 0], [far, 0], [4, 0]], eps=eps) == [0, 0, 1, 1]


def test_first_equals_last_point_is_measured_from_that_point():
    loop = [[0, 0], [1, 0], [1, 1], [0, 1], [0, 0]]                                          # L2 == 0: s = |q_i - q_a|^2, the far corner first
    assert _runs(loop) == [0, 0, 1, 1, 1] or _runs(loop) == [0, 0, 1, 2, 2]
    seg = _runs(loop)
    assert seg[2] != seg[1]                                                                  # (1, 1), index 2, starts a run
    tiny = [[0, 0], [0.1, 0], [0.1, 0.1], [0, 0.1], [0, 0]]                                  # every s <= tol^2 = 0.0225: no split
    assert _runs(tiny) == [0] * 5


def test_runs_of_one_and_two_points_are_final():
    assert _runs([[0, 0]]) == [0]
    assert _runs([[0, 0], [1, 1]]) == [0, 0]
    assert _runs([[0, 0], [5, 5]], eps=1.0) == [0, 1]                                        # the gap rule alone
    assert _runs([[0, 0], [0, 1], [1, 1]]) == [0, 1, 1]                                      # three points split into 1 + 2, both final


def test_interleaved_clusters_noise_and_numbering_across_clusters():
    #          c1        c0       noise     c1        c0       c0        c1       c1
    P = [[0, 10], [0, 0], [50, 50], [1, 10], [1, 0], [2, 0], [2, 10], [2, 11]]
    labels = [1, 0, -1, 1, 0, 0, 1, 1]
    seg = _runs(P, labels)
    assert seg[2] == -1                                                                      # noise untouched
    assert [seg[i] for i in (1, 4, 5)] == [0, 0, 0]                                          # cluster 0 first, in beam order, one straight run
    assert [seg[i] for i in (0, 3, 6, 7)] == [1, 1, 1, 2] or [seg[i] for i in (0, 3, 6, 7)] == [1, 1, 2, 2]
    assert max(seg) == 2
    # the segments of a cluster are numbered by the position of their first point
    two = _runs([[0, 0], [1, 0], [2, 0], [2, 1], [2, 2], [9, 9], [10, 9], [11, 9]], [0] * 5 + [1] * 3)
    assert two == [0, 0, 1, 1, 1, 2, 2, 2]


def test_a_scan_of_straight_clusters_gives_the_boxes_of_scan_box_bit_for_bit():
    """three short straight walls seen from the origin: every cluster is one run within tol, so the split changes nothing - corner for corner"""
    cfg = corridor_cfg()
    cfg["obstacle"][0]["number"] = 3
    cfg["obstacle"][0]["shape"] = [{"name": "polygon", "vertices": v} for v in (
        [[5, -2], [5.3, -2], [5.3, 2], [5, 2]], [[-2, 6], [2, 6], [2, 6.3], [-2, 6.3]], [[-7, -1.5], [-6.7, -1.5], [-6.7, 1.5], [-7, 1.5]])]
    env = world_at(cfg, (0, 0, 0.3))
    scan, state = env.get_lidar_scan(), env.robot.state
    pts = lidar.scan_points(scan)
    labels = lidar.dbscan(pts)
    assert labels.max() == 2
    assert np.array_equal(lidar.split_runs(pts, labels, 2.0, TOL_SPLIT), labels)            # the property first
    a, b = lidar.scan_box(state, scan), lidar.scan_box_split(state, scan, tol=TOL_SPLIT)
    assert len(a) == len(b) == 3 and all(np.array_equal(x.vertex, y.vertex) for x, y in zip(a, b))


def test_bad_tol_and_few_hits():
    env = world_at(corridor_cfg(), (20, 0.5, 0.1))
    scan, state = env.get_lidar_scan(), env.robot.state
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            lidar.scan_box_split(state, scan, tol=bad)
        with pytest.raises(ValueError):
            lidar.split_runs(np.zeros((3, 2)), np.zeros(3, int), 2.0, bad)
    few = np.full(len(scan["ranges"]), float(scan["range_max"]))
    few[:3] = 4.0
    assert lidar.scan_box_split(state, dict(scan, ranges=few)) == []
    for word in ("seam", "interleave", "corner-on"):
        assert word in lidar.split_runs.__doc__


# ---- the clearance table ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(POSES)))
def test_split_boxes_restore_the_clearance_one_box_per_cluster_hides(k):
    """robot 1.0 x 0.6 m, 360 beams over a full turn, 15 m: one box per cluster puts the robot INSIDE an obstacle; split at 0.15 m the clearance is the
    true walls' to within tol + one beam spacing at full range (a run's rectangle protrudes by at most tol, the hits are a beam spacing apart)"""
    cfg, pose = POSES[k]
    env = world_at(cfg, pose)
    scan, state, car = env.get_lidar_scan(), env.robot.state, env._car
    plain, split = lidar.scan_box(state, scan), lidar.scan_box_split(state, scan, tol=TOL_SPLIT)
    c_plain, c_split, c_true = (sc.clearance(car, state, obs) for obs in (plain, split, env.obstacles))
    bound = TOL_SPLIT + scan["range_max"] * scan["angle_increment"]
    print(f"pose {pose}: one box per cluster {c_plain:+.3f} m ({len(plain)}), split {c_split:+.3f} m ({len(split)}), true {c_true:+.3f} m, "
          f"|split - true| = {abs(c_split - c_true):.4f} m (bound {bound:.4f})")
    assert c_plain < 0.0
    assert c_split > 0.0
    assert abs(c_split - c_true) <= bound


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,first", [("rda_set_scan_split", "rda_handle *"), ("rda_fleet_set_scan_split", "rda_fleet *")])
def test_entries_are_declared_exported_documented_and_bound(name, first):
    from rda_planner_amd._capi import CApi
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header(), re.S)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == [first + ("h" if "handle" in first else "f"), "double tol"]
    so = lib()
    assert hasattr(so, name), f"{name} declared in include/rda_hip.h but not exported"
    assert integration_rows(name), name
    api = CApi(so, "rda")
    assert api.has_scan_split is True
    fn = getattr(api, name[len("rda_"):])
    assert list(fn.argtypes) == [C.c_void_p, C.c_double] and fn.restype is C.c_int
    for tol in (0.0, 0.15, -1.0, float("nan")):
        assert fn(None, tol) == RDA_ERR_ARG                                                  # no handle: an argument error, no device touched


# ---- the Python interface -----------------------------------------------------------------------------------------------------------------------------
def test_python_interface_and_refusals_before_any_device_call():
    import inspect
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    from oracle.oracle_backend import oracle_backend
    assert list(inspect.signature(lidar.split_runs).parameters) == ["points", "labels", "eps", "tol"]
    p = inspect.signature(lidar.scan_box_split).parameters
    assert list(p) == ["state", "scan_data", "eps", "min_samples", "tol"] and (p["eps"].default, p["min_samples"].default, p["tol"].default) == (2.0, 6, 0.15)
    assert list(inspect.signature(lidar.scan_box_split_device).parameters) == ["solver", "state", "scan_data", "eps", "min_samples", "tol"]
    assert list(inspect.signature(lidar.scan_box_split_device_fleet).parameters) == ["fleet", "states", "scans", "eps", "min_samples", "tol"]
    for fn in (Fleet.control, Fleet.rollout):
        assert "scan_split" in fn.__doc__ and "rda_fleet_set_scan_split" in fn.__doc__

    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    f = bare_fleet(Binding(**LIDAR_FLAGS, has_scan_split=True, has_fleet_scans=True), [pipeline_member(), pipeline_member()])      # no device: a binding that fails on any use
    with pytest.raises(ValueError, match="scan_split splits the clusters of lidar="):
        f.rollout(states, 4.0, 5, scan_split=0.15)
    with pytest.raises(ValueError, match="scan_split splits the clusters of scans="):
        f.control(states, 4.0, scan_split=0.15)
    for bad in (0.0, -0.15, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scan_split must be finite and greater than 0"):
            f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], scan_split=bad)
        with pytest.raises(ValueError, match="scan_split must be finite and greater than 0"):
            f.control(states, 4.0, scans=[None, None], scan_split=bad)
    f.api = Binding(**LIDAR_FLAGS, has_scan_split=False, has_fleet_scans=True)                             # a library without the two entries
    for call in (lambda: f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], scan_split=0.15), lambda: f.control(states, 4.0, scans=[None, None], scan_split=0.15),
                 lambda: f.set_scan_split(0.15)):
        with pytest.raises(RuntimeError, match="rda_set_scan_split, rda_fleet_set_scan_split"):
            call()
    f.set_scan_split(0.0)                                                                    # off on a fleet that is off: no library call
    # scan_split never reaches the tracking check: with it popped, these calls get as far as the next refusal
    f.api = Binding(**LIDAR_FLAGS, has_scan_split=True)
    with pytest.raises(ValueError, match="scan_eps"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], scan_split=0.15, scan_eps=0.0)
    # MPC.control on the CPU checker backend: the same ValueErrors before anything else, and no host fallback behind scan=
    mpc = MPC(sc.rectangle_robot(), sc.line_path([0, 20, 0], [60, 20, 0]), receding=5, max_edge_num=4, max_obs_num=3, iter_num=1, time_print=False,
              _backend=oracle_backend)
    state = np.array([[0.0], [20.0], [0.0]])
    scan = {"ranges": np.full(10, 5.0), "angle_min": -1.0, "angle_max": 1.0, "range_max": 10.0}
    with pytest.raises(ValueError, match="scan_split splits the clusters of scan="):
        mpc.control(state, 4.0, [], scan_split=0.15)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scan_split must be finite"):
            mpc.control(state, 4.0, scan=scan, scan_split=bad)
    assert not mpc.rda.has_scan
    with pytest.raises(RuntimeError):
        mpc.control(state, 4.0, scan=scan, scan_split=0.15)
    with pytest.raises(RuntimeError, match="rda_set_scan_split, rda_fleet_set_scan_split"):
        mpc.rda.set_scan_split(0.15)                                                         # the oracle library has no such entry
    mpc.rda.set_scan_split(0.0)
    u, info = mpc.control(state, 4.0, [sc.circle(10.0, 24.0, 1.0)])                          # the path without scan is what it was
    assert u.shape == (2, 1) and np.isfinite(u).all()


# ---- the closed loop round the bend, on the CPU checker ---------------------------------------------------------------------------------------------
BEND_T, BEND_N, BEND_E, BEND_ITER, BEND_DT, BEND_SPEED, BEND_TICKS, BEND_START = 5, 6, 4, 2, 0.1, 2.0, 80, (25.0, 0.0, 0.0)


def bend_car():
    return sc.rectangle_robot(1.0, 0.6, 0, "diff", max_speed=(2, 1), max_acce=(2, 1))


def bend_path():
    """along the first leg to the bend, then up the second leg: 5 m + 7 m"""
    return sc.line_path([25, 0, 0], [30, 0, 0]) + sc.line_path([30, 0, np.pi / 2], [30, 7, np.pi / 2])[1:]


def oracle_bend_loop(split):
    """the host loop of the corridor: World's scan, scan_box(_split), the oracle-backed MPC, the kinematic step -> (arrival tick, minimum clearance
    against the true walls)"""
    from oracle.oracle_backend import oracle_backend
    from rda_planner_amd.mpc import MPC
    env, car = world_at(corridor_cfg(), BEND_START), bend_car()
    m = MPC(car, bend_path(), receding=BEND_T, sample_time=BEND_DT, iter_num=BEND_ITER, max_edge_num=BEND_E, max_obs_num=BEND_N, time_print=False,
            _backend=oracle_backend)
    state, worst = env.robot.state.copy(), np.inf
    for k in range(BEND_TICKS):
        env.robot.state = state
        scan = env.get_lidar_scan()
        obstacles = lidar.scan_box_split(state, scan, tol=TOL_SPLIT) if split else lidar.scan_box(state, scan)
        u, info = m.control(state, BEND_SPEED, obstacles)
        if info["arrive"]:
            return k, worst
        state = sc.kinematic_step(state, u, car, BEND_DT)
        worst = min(worst, sc.clearance(car, state, env.obstacles))
    return -1, worst


def test_oracle_loop_round_the_bend():
    """T = 5, N = 6, E = 4, iter_num = 2, dt = 0.1, 2 m/s, 360 beams, eps 2.0, min_samples 6.  With the committed specification: split at 0.15 m the
    robot arrives at tick 68 with a minimum clearance of +0.917 m against the true walls; with one box per cluster it arrives at tick 64 with +0.367 m
    - it stands inside its only obstacle all the way, so the planner's constraints cannot hold and it follows the path with whatever the solver
    returns; nothing is asserted about that twin beyond what is printed."""
    tick, worst = oracle_bend_loop(True)
    plain = oracle_bend_loop(False)
    print(f"split: arrives at tick {tick}, minimum clearance {worst:+.3f} m; one box per cluster: tick {plain[0]}, {plain[1]:+.3f} m")
    assert 0 < tick < BEND_TICKS and worst > 0.0
