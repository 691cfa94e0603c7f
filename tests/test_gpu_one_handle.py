"""-m gpu : the single-handle entry points that keep, regrow and rebind a handle's resident tables, in sequence on ONE handle (A), against a twin (B) that
restages everything from the host on every tick.  Each pair of routes is asserted bit-identical on its own elsewhere (test_pipelined_tick_is_bit_identical,
test_upload_scan_equals_upload_scene_of_the_boxes, test_scene_resort_after_upload_scan, test_slots_bit_identical); here they follow each other on one handle,
so that the raw-scene blocks, the lidar set and the path are made, regrown, rebound and reused.  Everything either side returns must be equal bit for bit.

Shape and `solver` are those of tests/test_gpu_fleet_rollout_moving.py (T = 8, N = 4, E = 4, iter_num = 2; member 0, the Ackermann car); path, scenes and the
allocation counters are the helpers of tests/test_gpu_lifecycle.py (a straight path on y = 0, polygons around it).  One tick each unless noted:
  1  a raw scene of 3 obstacles         A: rda_tracked_begin + rda_upload_scene_async + rda_tracked_finish    B: rda_upload_scene, rda_step_tracked
  2  a scene of 40 obstacles (the device and pinned blocks regrow: the capacity after step 1 is 3 + 1 + 16 = 20), routes as in 1
  3  two ticks re-ranked about new robot positions    A: rda_scene_resort inside the tick    B: the 40 uploaded again with the new robot_xy
  4  a lidar tick, 64 beams (A's first use of its lidar set)    A: rda_upload_scan inside the tick    B: rda_scan_boxes, rda_upload_scene of the boxes
  5  re-ranked after the scan           A: rda_scene_resort    B: the boxes uploaded again
  6  a longer path (30 -> 200 points) through rda_upload_path on both, then a tick on the resident slots
  7  the 3 obstacles of step 1 again (the larger blocks are reused), routes as in 1"""
import ctypes as C
import gc

import numpy as np
import pytest

from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import Info, dptr, iptr

from fleet_twin_lib import E, N, T, info_tuple, solver
from lidar_world_lib import numpy_scan
from test_gpu_lifecycle import live, path_array, scene_arrays

pytestmark = pytest.mark.gpu

SPEED, THRESHOLD, IND_RANGE = 3.0, 0.1, 10
EPS, MIN_SAMPLES = 0.4, 3                              # DBSCAN of step 4's scan: six clusters, no pair of hits within 2 mm of EPS apart
SENSOR = dict(number=64, angle_min=-0.5 * np.pi, angle_max=0.5 * np.pi, range_min=0.0, range_max=10.0)
SHIFTS = ([5.0, 1.5], [9.0, -2.0], [4.0, -1.0])         # where steps 3 and 5 re-rank about, from the robot


def world():
    """what the sensor of step 4 sees: the 40 polygons of step 2 as obstacle objects (the same call as scene_arrays makes)"""
    return sc.scene_polygons(40, lo=(1, -4), hi=(12, 4), seed=12)


def sequence(hip):
    """the seven steps on a fresh pair of handles -> (A's ticks, B's ticks, allocation counters before and after); a tick: [(name, value)]"""
    gc.collect()
    gc.disable()                                        # the counters are process-wide: no solver of an earlier test may be collected in between
    try:
        start = live(hip)
        sides = [solver(hip, 0, path=False, scene=False)[0] for _ in range(2)]
        ha, hb = (s._be.handle for s in sides)
        for h in (ha, hb):
            assert hip.upload_path(h, 30, dptr(path_array(0.0, 30))) == 0
        small, big = scene_arrays(3, 11), scene_arrays(40, 12)
        assert small[0] == 3 and big[0] == 40
        cur, k, ticks = [0, 0], [0], ([], [])

        def state():
            return np.array([0.25 * k[0], 0.02 * k[0], 0.0])

        def scene_c(scn, xy):
            m, kind, nvert, geom, vel = scn
            return m, iptr(kind), iptr(nvert), dptr(geom), dptr(vel), dptr(np.ascontiguousarray(xy, float)), 1

        def boxes_scene(boxes):
            n = len(boxes)
            geom = np.zeros((n, E, 2)); geom[:, 0:4, :] = boxes
            return n, np.zeros(n, np.int32), np.full(n, 4, np.int32), geom, np.zeros((n, 2))

        def slots(h):
            A, b, cone, nt = np.zeros((N, T + 1, E, 2)), np.zeros((N, T + 1, E)), np.zeros(N, np.int32), np.zeros(1, np.int32)
            assert hip.get_obstacles(h, dptr(A), dptr(b), iptr(cone), iptr(nt)) == 0
            m = N * int(nt[0]) * E
            return [("slots_A", A.ravel()[:2 * m].copy()), ("slots_b", b.ravel()[:m].copy()), ("cone", cone), ("nt", int(nt[0]))]

        def tick(side, h, stage, inside):
            """one tracked tick of handle h; stage(): this tick's staging call -> rc, made inside the open tick (A) or before the serial step (B)"""
            st, nom = state(), dptr(np.zeros((2, T))) if k[0] == 0 else None
            u, s, info, mi, eh = np.full((2, T), np.nan), np.full((3, T + 1), np.nan), Info(), C.c_int32(-1), C.c_double(np.nan)
            if inside:
                assert hip.tracked_begin(h, dptr(st), SPEED, cur[side], THRESHOLD, IND_RANGE, nom) == 0
                assert stage() == 0
                rc = hip.tracked_finish(h, dptr(u), dptr(s), C.byref(info), None, None, C.byref(mi), C.byref(eh))
            else:
                assert stage() == 0
                rc = hip.step_tracked(h, dptr(st), SPEED, cur[side], THRESHOLD, IND_RANGE, nom, dptr(u), dptr(s), C.byref(info), None, None,
                                      C.byref(mi), C.byref(eh))
            assert rc >= 0, rc
            cur[side] = mi.value
            ticks[side].append([("rc", rc), ("out_u", u), ("out_s", s), ("info", info_tuple(info)), ("min_index", mi.value),
                                ("end_heading", eh.value)] + slots(h))

        def both(stage_a, stage_b):
            tick(0, ha, stage_a, True)
            tick(1, hb, stage_b, False)
            k[0] += 1

        def upload(scn):
            xy = state()[0:2]
            both(lambda: hip.upload_scene_async(ha, *scene_c(scn, xy)), lambda: hip.upload_scene(hb, *scene_c(scn, xy), None))

        def resort(scn, shift):
            there = np.ascontiguousarray(state()[0:2] + np.array(shift))
            both(lambda: hip.scene_resort(ha, dptr(there)), lambda: hip.upload_scene(hb, *scene_c(scn, there), None))

        upload(small)                                                                    # 1
        upload(big)                                                                      # 2
        for shift in SHIFTS[0:2]:                                                        # 3
            resort(big, shift)
        st = state()                                                                     # 4
        ranges = np.ascontiguousarray(np.asarray(numpy_scan(st, SENSOR, world())["ranges"], float))
        head = (len(ranges), dptr(ranges), SENSOR["angle_min"], SENSOR["angle_max"], SENSOR["range_max"], dptr(st), EPS, MIN_SAMPLES)
        n_a, n_b, boxes = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros((len(ranges), 4, 2))

        def scan_b():
            rc = hip.scan_boxes(hb, *head, iptr(n_b), dptr(boxes), len(boxes), None)
            return rc or hip.upload_scene(hb, *scene_c(boxes_scene(boxes[:int(n_b[0])]), st[0:2]), None)

        both(lambda: hip.upload_scan(ha, *head, 1, iptr(n_a)), scan_b)
        assert n_a[0] == n_b[0] and n_b[0] > N, (n_a, n_b)          # more boxes than slots
        resort(boxes_scene(boxes[:int(n_b[0])]), SHIFTS[2])                              # 5
        for h in (ha, hb):                                                               # 6
            assert hip.upload_path(h, 200, dptr(path_array(0.0, 200))) == 0
        both(lambda: 0, lambda: 0)
        upload(small)                                                                    # 7
        for s in sides:
            s._be.close()
        return ticks[0], ticks[1], start, live(hip)
    finally:
        gc.enable()


@pytest.fixture(scope="module")
def run(hip):
    return sequence(hip)


def test_one_handle_equals_restaging_twin_bit_for_bit(run):
    """out_u, out_s, rda_info, min_index, end_heading and the staged slots of every tick; both handles give back everything they allocated"""
    a, b, start, end = run
    assert len(a) == len(b) == 8
    for k, (ta, tb) in enumerate(zip(a, b)):
        assert [name for name, _ in ta] == [name for name, _ in tb]
        for (name, x), (_, y) in zip(ta, tb):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (k, name)
    assert end == start


def test_the_sequence_is_not_trivial(run):
    """the handle is driven on every tick, the 40-obstacle scene has more obstacles than slots, and the re-ranking rebinds the slots"""
    a = [dict(t) for t in run[0]]
    for k, t in enumerate(a):
        assert np.abs(t["out_u"]).max() > 0.1 and np.all(np.isfinite(t["out_u"])) and np.all(np.isfinite(t["out_s"])), k
    assert scene_arrays(40, 12)[0] > N
    for k in (1, 2, 4, 5, 7):                           # the scene of step 1 -> 2, the re-ranking of 3 and 5, the boxes of 4, the scene of 7: other slots than the tick before
        assert not np.array_equal(a[k]["slots_A"], a[k - 1]["slots_A"]), k
