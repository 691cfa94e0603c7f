"""-m gpu : the lidar front end on the device (rda_scan_boxes / rda_upload_scan, csrc/lidar_device.h) against its specification, the host
module rda_planner_amd/lidar.py (scan_points, dbscan, min_area_rect, scan_box).

Scans are ray-cast by rda_planner_amd.world.World in random scenes of 3-13 circles and rotated boxes around the robot.  Labels must be EQUAL
(DBSCAN decisions are taken on the same numbers up to an ulp of cos / sin, and the scans are asserted to hold no pair of points within 1e-9 of
eps); box corners within 1e-9 m (coordinates <= ~50 m: ulps of cos / sin and of the order of a dot product); staged obstacle slots and controls
bit for bit between the two device routes (scan staged on the device / boxes fetched and uploaded as a scene)."""
import ctypes as C
import os

import numpy as np
import pytest

from rda_planner_amd import lidar
from rda_planner_amd import scenarios as sc
from rda_planner_amd import world as irsim
from rda_planner_amd._capi import dptr, iptr
from rda_planner_amd.mpc import MPC

pytestmark = pytest.mark.gpu

RDA_ERR_UNSUPPORTED, RDA_ERR_HIP = -2, -3
BEAMS = (100, 181, 360, 720, 1080)
N_SCANS = 110
TOL = 1e-9


def _world(rng, beams, fov):
    state = [float(rng.uniform(10, 40)), float(rng.uniform(10, 40)), float(rng.uniform(-np.pi, np.pi))]
    obstacles = []
    for _ in range(int(rng.integers(3, 14))):
        d, a = rng.uniform(3.0, 14.0), rng.uniform(-np.pi, np.pi)
        pos = [state[0] + d * np.cos(a), state[1] + d * np.sin(a), float(rng.uniform(-np.pi, np.pi))]
        if rng.random() < 0.4:
            shape = {"name": "circle", "radius": float(rng.uniform(0.3, 1.5))}
        else:
            shape = {"name": "rectangle", "length": float(rng.uniform(0.5, 5.0)), "width": float(rng.uniform(0.3, 2.5))}
        obstacles.append({"number": 1, "distribution": {"name": "manual"}, "state": [pos], "shape": [shape]})
    cfg = {"world": {"step_time": 0.1},
           "robot": [{"kinematics": {"name": "acker"}, "shape": {"name": "rectangle", "length": 4.6, "width": 1.6, "wheelbase": 3}, "state": state,
                      "sensors": [{"type": "lidar2d", "range_max": 15.0, "angle_range": fov, "number": beams}]}],
           "obstacle": obstacles}
    return irsim.World(cfg)


def _eps_margin(pts, eps_values):
    """smallest | distance - eps | over all pairs of points and the given eps"""
    if len(pts) < 2:
        return np.inf
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2))
    return min(float(np.abs(d - e).min()) for e in eps_values)


def _beam_labels(scan, eps, min_samples):
    """lidar.dbscan of the scan's hits, re-expanded to beams (misses -2)"""
    ranges = np.asarray(scan["ranges"], float)
    hit = ranges < scan["range_max"] - 0.01
    out = np.full(len(ranges), -2, np.int64)
    out[hit] = lidar.dbscan(lidar.scan_points(scan), eps, min_samples)
    return out


@pytest.fixture(scope="module")
def scans():
    """[(state (3,1), scan dict)]: fixed seeds, every beam count, half and (just under) full field of view"""
    out = []
    for k in range(N_SCANS):
        rng = np.random.default_rng(52000 + k)
        env = _world(rng, BEAMS[k % len(BEAMS)], np.pi if (k // len(BEAMS)) % 2 == 0 else 2 * np.pi - 0.01)
        out.append((env.robot.state.copy(), env.get_lidar_scan()))
    return out


@pytest.fixture(scope="module")
def host(scans):
    """the host side of every scan, computed once: per-beam labels and the boxes of lidar.scan_box ((n, 4, 2), world frame)"""
    out = []
    for state, scan in scans:
        boxes = np.array([o.vertex.T for o in lidar.scan_box(state, scan)]).reshape(-1, 4, 2)
        out.append((_beam_labels(scan, 2.0, 6), boxes))
    return out


@pytest.fixture(scope="module")
def planner(hip):
    car = sc.rectangle_robot()
    return MPC(car, sc.line_path([0, 20, 0], [60, 20, 0]), receding=10, max_edge_num=4, max_obs_num=5, iter_num=2)


def _mpc(N, E=4, T=10):
    return MPC(sc.rectangle_robot(), sc.line_path([0, 20, 0], [60, 20, 0]), receding=T, max_edge_num=E, max_obs_num=N, iter_num=2)


def _scan_c(scan, state):
    ranges = np.ascontiguousarray(np.asarray(scan["ranges"], float))
    st = np.ascontiguousarray(np.asarray(state, float).ravel()[0:3])
    return ranges, st, (len(ranges), dptr(ranges), float(scan["angle_min"]), float(scan["angle_max"]), float(scan["range_max"]), dptr(st))


def _device(mpc, state, scan, eps=2.0, min_samples=6, cap=None):
    """rda_scan_boxes -> (return code, boxes (n, 4, 2), per-beam labels)"""
    api, h = mpc.rda._be.api, mpc.rda._be.handle
    ranges, st, head = _scan_c(scan, state)
    cap = len(ranges) if cap is None else cap
    boxes, n, labels = np.zeros((max(cap, 1), 4, 2)), np.zeros(1, np.int32), np.full(max(len(ranges), 1), -9, np.int32)
    rc = api.scan_boxes(h, *head, float(eps), int(min_samples), iptr(n), dptr(boxes), cap, iptr(labels))
    return rc, boxes[:min(int(n[0]), cap)], labels[:len(ranges)], int(n[0])


def _slots(mpc):
    api, h = mpc.rda._be.api, mpc.rda._be.handle
    T, N, E = mpc.rda.T, mpc.rda.max_obs_num, mpc.rda.max_edge_num
    A = np.zeros((N, T + 1, E, 2)); b = np.zeros((N, T + 1, E)); cone = np.zeros(N, np.int32); nt = np.zeros(1, np.int32)
    assert api.get_obstacles(h, dptr(A), dptr(b), iptr(cone), iptr(nt)) == 0
    k = int(nt[0])
    return A.ravel()[: N * k * E * 2].copy(), b.ravel()[: N * k * E].copy(), cone.copy(), k


def _same_slots(a, b):
    return a[3] == b[3] and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def _upload_scan(mpc, state, scan, order, eps=2.0, min_samples=6):
    api, h = mpc.rda._be.api, mpc.rda._be.handle
    ranges, st, head = _scan_c(scan, state)
    n = np.zeros(1, np.int32)
    rc = api.upload_scan(h, *head, float(eps), int(min_samples), int(order), iptr(n))
    return rc, int(n[0])


def _upload_boxes(mpc, boxes, robot_xy, order):
    """rda_upload_scene of (n, 4, 2) boxes as 4-vertex polygons without velocity"""
    api, h = mpc.rda._be.api, mpc.rda._be.handle
    n, E = len(boxes), mpc.rda.max_edge_num
    geom = np.zeros((n, E, 2)); geom[:, 0:4, :] = boxes
    kind, nvert, vel = np.zeros(n, np.int32), np.full(n, 4, np.int32), np.zeros((n, 2))
    rob = np.ascontiguousarray(np.asarray(robot_xy, float).ravel()[0:2])
    return api.upload_scene(h, n, iptr(kind), iptr(nvert), dptr(geom), dptr(vel), dptr(rob), int(order), None)


# ---- 1. labels ------------------------------------------------------------------------------------------------------------------------------------
def test_labels_equal_host_dbscan(planner, scans, host):
    assert len(scans) >= 100 and {len(s["ranges"]) for _, s in scans} == set(BEAMS)
    clusters = 0
    for i, ((state, scan), (want, _)) in enumerate(zip(scans, host)):
        assert _eps_margin(lidar.scan_points(scan), (2.0,)) > TOL, i          # a condition on the test's own inputs, not a skip
        rc, _, labels, n = _device(planner, state, scan)
        assert rc == 0
        assert np.array_equal(labels, want), (i, np.flatnonzero(labels != want)[:8])
        assert n == (want.max() + 1 if (want >= 0).any() and (want > -2).sum() >= 4 else 0)
        clusters += n
    assert clusters >= 300


@pytest.mark.parametrize("eps", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("min_samples", [3, 6, 10])
def test_labels_other_parameters(planner, scans, eps, min_samples):
    seen = set()
    for i in range(0, len(scans), 9):                                      # 13 scans, every beam count among them
        state, scan = scans[i]
        assert _eps_margin(lidar.scan_points(scan), (eps,)) > TOL, i
        rc, _, labels, n = _device(planner, state, scan, eps, min_samples)
        want = _beam_labels(scan, eps, min_samples)
        assert rc == 0 and np.array_equal(labels, want), (i, eps, min_samples)
        seen.update(want[want > -2].tolist())
    assert -1 in seen and max(seen) >= 2                                   # noise, border and several clusters all occur


# ---- 2. boxes -------------------------------------------------------------------------------------------------------------------------------------
def _cyclic_error(dev, ref):
    return min(float(np.abs(np.roll(dev, s, axis=0) - ref).max()) for s in range(4))


def _edge_rectangles(hull):
    """(area, corners) of the enclosing rectangle on every hull edge, as lidar.min_area_rect forms them"""
    out, m = [], len(hull)
    for i in range(m if m > 2 else 1):
        e = hull[(i + 1) % m] - hull[i]
        u = e / np.linalg.norm(e)
        v = np.array([-u[1], u[0]])
        a, b = hull @ u, hull @ v
        out.append(((a.max() - a.min()) * (b.max() - b.min()),
                    np.array([a.min() * u + b.min() * v, a.max() * u + b.min() * v, a.max() * u + b.max() * v, a.min() * u + b.max() * v])))
    return out


def _property_check(dev, ref, pts):
    """the fall-back for a cluster with two DIFFERENT rectangles within 1e-6 relative area of the best: the device's box must still be a
    minimum-area rectangle of the points `pts` (all in the world frame)"""
    hull = lidar.convex_hull(pts)
    if len(hull) < 3:
        return False
    rects = _edge_rectangles(hull)
    best = min(a for a, _ in rects)
    rivals = [r for a, r in rects if a <= best * (1 + 1e-6) and _cyclic_error(r, ref) > 1e-6]
    if not rivals:
        return False                                                       # no near tie: the corners had to match
    e = np.roll(dev, -1, axis=0) - dev
    n = np.stack((e[:, 1], -e[:, 0]), axis=1) / np.linalg.norm(e, axis=1, keepdims=True)      # outward normals of a CCW box
    inside = all(((pts - dev[k]) @ n[k]).max() <= TOL for k in range(4))
    on_edge = any(np.abs((hull[[i, (i + 1) % len(hull)]] - dev[k]) @ n[k]).max() <= TOL for i in range(len(hull)) for k in range(4))
    area = np.linalg.norm(e[0]) * np.linalg.norm(e[1])
    ref_e = np.roll(ref, -1, axis=0) - ref
    return inside and on_edge and area <= np.linalg.norm(ref_e[0]) * np.linalg.norm(ref_e[1]) * (1 + 1e-9)


def test_boxes_equal_host_scan_box(planner, scans, host):
    total, by_property, degenerate, worst = 0, 0, 0, 0.0
    for i, ((state, scan), (labels, want)) in enumerate(zip(scans, host)):
        rc, boxes, _, n = _device(planner, state, scan)
        assert rc == 0 and n == len(want) and boxes.shape == want.shape, (i, n, len(want))
        pts = lidar.scan_points(scan)
        hit_labels = labels[labels > -2]
        th = state[2, 0]
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        for c in range(n):
            e = np.roll(boxes[c], -1, axis=0) - boxes[c]
            assert all(e[k][0] * e[(k + 1) % 4][1] - e[k][1] * e[(k + 1) % 4][0] > 0 for k in range(4)), (i, c)      # counter-clockwise
            sides = np.linalg.norm(np.roll(want[c], -1, axis=0) - want[c], axis=1)
            degenerate += bool(sides.min() < 0.01 * (1 + 1e-6))
            total += 1
            err = _cyclic_error(boxes[c], want[c])
            if err < TOL:
                worst = max(worst, err)
                continue
            world_pts = (state[0:2] + R @ pts[hit_labels == c].T).T
            assert _property_check(boxes[c], want[c], world_pts), (i, c, err, boxes[c], want[c])
            by_property += 1
    print(f"{total} clusters, {degenerate} degenerate (widened to 1 cm), {by_property} by the property check, worst corner error {worst:.3g} m")
    assert total >= 300 and degenerate >= 10
    assert by_property <= 0.02 * total


# ---- 3. the same obstacles either way -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("N", [2, 16])
def test_upload_scan_equals_upload_scene_of_the_boxes(scans, host, order, N):
    a, b = _mpc(N), _mpc(N)
    done = 0
    for i in range(3, len(scans), 7):
        state, scan = scans[i]
        n_host = len(host[i][1])
        if n_host < 3:
            continue
        assert (n_host > N) if N == 2 else (n_host < N)                    # more boxes than slots / fewer
        rc, boxes, _, n = _device(b, state, scan)
        assert rc == 0 and n == n_host
        assert _upload_boxes(b, boxes, state[0:2], order) == 0
        rc, n2 = _upload_scan(a, state, scan, order)
        assert rc == 0 and n2 == n
        assert _same_slots(_slots(a), _slots(b)), (i, order, N)
        done += 1
    assert done >= 8


def test_scene_resort_after_upload_scan(scans, host):
    a, b = _mpc(3), _mpc(3)
    i = next(k for k in range(len(scans)) if len(host[k][1]) >= 6)
    state, scan = scans[i]
    assert _upload_scan(a, state, scan, 1)[0] == 0
    rc, boxes, _, n = _device(b, state, scan)
    for shift in ([6.0, -4.0], [-9.0, 7.5]):
        there = np.ascontiguousarray(state[0:2, 0] + np.array(shift))
        assert a.rda._be.api.scene_resort(a.rda._be.handle, dptr(there)) == 0
        assert _upload_boxes(b, boxes, there, 1) == 0
        assert _same_slots(_slots(a), _slots(b))


def _few_hits(scan, hits):
    ranges = np.full(len(scan["ranges"]), float(scan["range_max"]))
    ranges[:hits] = 4.0
    return dict(scan, ranges=ranges)


@pytest.mark.parametrize("hits", [0, 3])
def test_scan_without_boxes_leaves_slots_and_skips_the_dual_side(scans, host, hits):
    i = next(k for k in range(len(scans)) if len(host[k][1]) >= 2)
    state, scan = scans[i]
    empty = _few_hits(scan, hits)
    assert lidar.scan_box(state, empty) == []
    a = _mpc(5)
    assert _upload_scan(a, state, scan, 1)[0] == 0
    before = _slots(a)
    rc, n = _upload_scan(a, state, empty, 1)
    assert rc == 0 and n == 0
    assert _same_slots(_slots(a), before)
    # the step behind it is the n == 0 step of tests/test_gpu_scene.py::test_empty_scene_skips_dual_side: same control, same info
    p, q = _mpc(5), _mpc(5)
    st = np.array([[0.0], [20.0], [0.0]])
    for _ in range(3):
        u1, i1 = p.control(st, 4.0, [])
        u2, i2 = q.control(st, 4.0, scan=empty)
        assert np.array_equal(u1, u2) and np.isfinite(u2).all() and i2["iters"] >= 1
        assert all(i1[k] == i2[k] for k in ("resi_dual", "resi_pri", "iters", "status", "su_ipm_iters", "lmz_fail", "arrive"))
        st = sc.kinematic_step(st, u1, sc.rectangle_robot(), 0.1)


# ---- 4. the same control either way ---------------------------------------------------------------------------------------------------------------
def _example(start=(0.0, 0.0, 0.0)):
    env = irsim.make(os.path.join(os.path.dirname(__file__), "golden", "world_lidar_track.yaml"))
    for k in range(3):
        env.robot.state[k, 0] += start[k]
    ri = env.get_robot_info()
    car = sc.car(ri.G, ri.h, ri.cone_type, ri.wheelbase, [10, 1], [10, 0.5], "acker")

    def make():
        return MPC(car, sc.path_track_ref(), receding=10, sample_time=env.step_time, process_num=4, iter_num=2, max_edge_num=4, max_obs_num=4,
                   obstacle_order=True, wu=1.0, slack_gain=13)
    return env, make


def test_control_with_scan_equals_control_with_device_boxes():
    env, make = _example()
    a, b = make(), make()
    assert a.device_track and a.rda.has_pipeline                          # scan= keeps the tick in its two halves
    boxes_seen = 0
    for i in range(60):
        scan = env.get_lidar_scan()
        state = env.robot.state.copy()
        ua, ia = a.control(state.copy(), 4, scan=scan)
        obs = lidar.scan_box_device(b, state.copy(), scan)
        ub, ib = b.control(state.copy(), 4, obs)
        boxes_seen = max(boxes_seen, len(obs))
        assert np.array_equal(ua, ub), (i, ua.ravel(), ub.ravel())
        assert a.cur_index == b.cur_index and np.array_equal(a.cur_vel_array, b.cur_vel_array)
        for k in ("resi_dual", "resi_pri", "iters", "status", "su_ipm_iters", "lmz_fail", "arrive"):
            assert ia[k] == ib[k], (i, k)
        assert all(np.array_equal(x, y) for x, y in zip(ia["opt_state_list"], ib["opt_state_list"]))
        assert all(np.array_equal(x, y) for x, y in zip(ia["ref_traj_list"], ib["ref_traj_list"]))
        env.step(ua)
        if env.done() or ia["arrive"]:
            break
    assert i >= 30 and boxes_seen >= 2


def test_untracked_control_with_scan_equals_host_staged_boxes():
    """device_track=False: host pre_process, rda_upload_scan, then the step on the staged obstacles == rda_step_scene of the boxes"""
    env, make = _example()
    a, b = make(), make()
    a.device_track = b.device_track = False
    for i in range(12):
        scan, state = env.get_lidar_scan(), env.robot.state.copy()
        ua, ia = a.control(state.copy(), 4, scan=scan)
        ub, ib = b.control(state.copy(), 4, lidar.scan_box_device(b, state.copy(), scan))
        assert np.array_equal(ua, ub) and ia["iters"] == ib["iters"] and ia["resi_pri"] == ib["resi_pri"], i
        env.step(ua)


def test_scan_loop_reaches_the_goal_from_most_starts():
    """the closed loop of the lidar example driven by scan= alone; the RATE of test_host_api.py::test_lidar_example_reaches_the_goal_from_most_starts
    (the loop is chaotic: see there)"""
    from test_host_api import LIDAR_STARTS
    runs = []
    for start in LIDAR_STARTS:
        env, make = _example(start)
        mpc, min_clear, arrived = make(), np.inf, False
        for i in range(500):
            u, info = mpc.control(env.robot.state, 4, scan=env.get_lidar_scan())
            env.step(u)
            min_clear = min(min_clear, env.clearance())
            if env.done() or info["arrive"]:
                arrived = info["arrive"]
                break
        runs.append((bool(arrived), bool(env.collided), float(min_clear)))
    assert sum(a and not c and mc > 0.0 for a, c, mc in runs) >= 3, runs


# ---- 5. limits and errors -------------------------------------------------------------------------------------------------------------------------
def _dense_scan(n=4096):
    """a synthetic scan of n beams: six wavy arcs (~ 360 hits each) with gaps between them"""
    ang = np.linspace(-np.pi + 0.005, np.pi - 0.005, n)
    r = 6.0 + np.sin(3 * ang) + 0.3 * np.sin(17 * ang)
    ranges = np.where(np.mod(ang + np.pi, 2 * np.pi / 6) < 0.52, r, 15.0)
    return {"ranges": ranges, "angle_min": float(ang[0]), "angle_max": float(ang[-1]), "range_max": 15.0}


def test_4096_beams_with_more_than_2000_hits(planner):
    scan, state = _dense_scan(), np.array([[12.0], [-7.0], [0.8]])
    pts = lidar.scan_points(scan)
    assert len(pts) >= 2000 and _eps_margin(pts, (0.5,)) > TOL
    want = _beam_labels(scan, 0.5, 6)
    ref = np.array([o.vertex.T for o in lidar.scan_box(state, scan, 0.5, 6)])
    assert len(ref) >= 6 and max(np.bincount(want[want >= 0])) > 300
    rc, boxes, labels, n = _device(planner, state, scan, 0.5, 6)
    assert rc == 0 and np.array_equal(labels, want) and n == len(ref)
    assert max(_cyclic_error(boxes[c], ref[c]) for c in range(n)) < TOL


def test_limits_are_refused(planner, scans):
    state, scan = scans[0]
    big = dict(_dense_scan(4097))
    assert _device(planner, state, big)[0] == RDA_ERR_UNSUPPORTED and _upload_scan(planner, state, big, 1)[0] == RDA_ERR_UNSUPPORTED
    e3 = _mpc(4, E=3)
    assert _device(e3, state, scan)[0] == RDA_ERR_UNSUPPORTED and _upload_scan(e3, state, scan, 1)[0] == RDA_ERR_UNSUPPORTED
    for eps, ms in ((0.0, 6), (-1.0, 6), (float("nan"), 6), (2.0, 0)):
        assert _device(planner, state, scan, eps, ms)[0] == -1 and _upload_scan(planner, state, scan, 1, eps, ms)[0] == -1
    api, h = planner.rda._be.api, planner.rda._be.handle
    ranges, st, head = _scan_c(scan, state)
    n = np.zeros(1, np.int32)
    assert api.scan_boxes(h, -1, *head[1:], 2.0, 6, iptr(n), None, 0, None) == -1
    assert api.scan_boxes(h, head[0], None, *head[2:], 2.0, 6, iptr(n), None, 0, None) == -1
    assert api.scan_boxes(h, *head, 2.0, 6, None, None, 0, None) == -1
    assert api.upload_scan(h, *head[:5], None, 2.0, 6, 1, None) == -1
    # more clusters than the caller's room: the count is the whole number, the first `cap` boxes are written
    i = 3
    rc, boxes, _, n_all = _device(planner, *scans[i])
    rc2, first, _, n2 = _device(planner, *scans[i], cap=1)
    assert rc == 0 and rc2 == 0 and n_all >= 2 and n2 == n_all and np.array_equal(first, boxes[:1])


def test_nan_and_negative_ranges(planner, scans):
    state, scan = scans[7]
    ranges = np.asarray(scan["ranges"], float).copy()
    hits = np.flatnonzero(ranges < scan["range_max"] - 0.01)
    assert len(hits) > 20
    ranges[hits[::3]] = np.nan                                             # a NaN range is a miss
    ranges[hits[1::7]] *= -1.0                                             # a negative range is a hit behind the sensor, as on the host
    bad = dict(scan, ranges=ranges)
    assert _eps_margin(lidar.scan_points(bad), (2.0,)) > TOL
    rc, boxes, labels, n = _device(planner, state, bad)
    want = _beam_labels(bad, 2.0, 6)
    ref = np.array([o.vertex.T for o in lidar.scan_box(state, bad)]).reshape(-1, 4, 2)
    assert rc == 0 and np.array_equal(labels, want) and (labels[hits[::3]] == -2).all() and n == len(ref)
    assert all(_cyclic_error(boxes[c], ref[c]) < TOL for c in range(n))
    for fill in (np.nan, -np.inf, -3.0):
        rc, boxes, labels, n = _device(planner, state, dict(scan, ranges=np.full(len(ranges), fill)))
        assert rc == 0 and (n == 0 if np.isnan(fill) else n >= 0)
    rc, n = _upload_scan(planner, state, dict(scan, ranges=np.full(len(ranges), np.nan)), 1)
    assert rc == 0 and n == 0


def _live(hip):
    n, b = C.c_longlong(0), C.c_longlong(0)
    assert hip.debug_alloc_stats(C.byref(n), C.byref(b)) == 0
    return n.value, b.value


def test_refused_allocation_changes_and_leaks_nothing(hip, scans, host):
    """every allocation of a first rda_upload_scan on a handle (the lidar buffers, then a larger raw scene) refused in turn by the host-side hook:
    RDA_ERR_HIP, the live-allocation counters and the staged slots as they were; then the call goes through"""
    import gc
    gc.collect()                                                           # no handle of an earlier test is released while this one counts
    i = next(k for k in range(len(scans)) if len(host[k][1]) >= 2)
    state, scan = scans[i]
    a = _mpc(4)
    assert _upload_boxes(a, host[i][1][:2], state[0:2], 1) == 0            # a small resident scene: the scan below needs a larger one
    before = _slots(a)
    refused = 0
    for k in range(40):
        live = _live(hip)
        hip.debug_alloc_fail(k)
        try:
            rc, n = _upload_scan(a, state, scan, 1, eps=1e-3, min_samples=1)      # every hit a cluster of its own: more boxes than reserved
        finally:
            hip.debug_alloc_fail(-1)
        if rc != RDA_ERR_HIP:
            break
        refused += 1
        assert _live(hip) == live, (k, live, _live(hip))
        assert _same_slots(_slots(a), before), k
    assert rc == 0 and n > 19 and refused >= 6, (rc, n, refused)
    assert _live(hip)[0] > live[0] and not _same_slots(_slots(a), before)
    b = _mpc(4)
    rc, boxes, _, nb = _device(b, state, scan, 1e-3, 1)
    assert rc == 0 and nb == n and _upload_boxes(b, boxes, state[0:2], 1) == 0 and _same_slots(_slots(a), _slots(b))
