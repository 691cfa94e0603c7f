"""-m gpu : the split stage of the lidar front end (rda_set_scan_split / rda_fleet_set_scan_split, lidar::split_stage of csrc/lidar_device.h) against
its specification lidar.split_runs / lidar.scan_box_split, and against the unsplit routes it must leave untouched.

Scans are ray-cast by rda_planner_amd.world.World in the L-shaped corridor of tests/golden/world_lidar_corridor.yaml and in a closed room of 12 x 8 m
(wall centre lines; walls 0.3 m thick), both seen by a full-turn lidar.  Segment labels and counts must be EQUAL to the specification's; box corners
within TOL = 1e-9 m, the bound tests/test_gpu_lidar.py uses for rda_scan_boxes ("box corners within 1e-9 m (coordinates <= ~50 m: ulps of cos / sin
and of the order of a dot product)").  Every other comparison is device against device, bit for bit."""
import numpy as np
import pytest

from rda_planner_amd import lidar
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import dptr, iptr
from rda_planner_amd.fleet import Fleet
from rda_planner_amd.mpc import MPC

from test_lidar_split import POSES, TOL_SPLIT, room_cfg, world_at

pytestmark = pytest.mark.gpu

TOL = 1e-9                    # tests/test_gpu_lidar.py: TOL
RDA_ERR_ARG = -1
EPS, MIN_SAMPLES = 2.0, 6


def _mpc(N=8, E=4, T=10):
    return MPC(sc.rectangle_robot(), sc.line_path([0, 20, 0], [60, 20, 0]), receding=T, max_edge_num=E, max_obs_num=N, iter_num=2)


def _split(mpc, tol):
    return mpc.rda._be.api.set_scan_split(mpc.rda._be.handle, float(tol))


def _device(mpc, state, scan):
    """rda_scan_boxes with the handle's split setting -> (boxes (n, 4, 2), per-beam labels, n)"""
    api, h = mpc.rda._be.api, mpc.rda._be.handle
    ranges = np.ascontiguousarray(np.asarray(scan["ranges"], float))
    st = np.ascontiguousarray(np.asarray(state, float).ravel()[0:3])
    cap = max(len(ranges), 1)
    boxes, n, labels = np.zeros((cap, 4, 2)), np.zeros(1, np.int32), np.full(cap, -9, np.int32)
    rc = api.scan_boxes(h, len(ranges), dptr(ranges), float(scan["angle_min"]), float(scan["angle_max"]), float(scan["range_max"]), dptr(st), EPS,
                        MIN_SAMPLES, iptr(n), dptr(boxes), cap, iptr(labels))
    assert rc == 0, rc
    return boxes[:int(n[0])].copy(), labels[:len(ranges)].copy(), int(n[0])


def _spec(state, scan, tol=TOL_SPLIT):
    """lidar.split_runs re-expanded to beams (misses -2) and the boxes of lidar.scan_box_split"""
    ranges = np.asarray(scan["ranges"], float)
    hit = ranges < scan["range_max"] - 0.01
    pts = lidar.scan_points(scan)
    out = np.full(len(ranges), -2, np.int64)
    out[hit] = lidar.split_runs(pts, lidar.dbscan(pts, EPS, MIN_SAMPLES), EPS, tol)
    boxes = np.array([o.vertex.T for o in lidar.scan_box_split(state, scan, EPS, MIN_SAMPLES, tol)]).reshape(-1, 4, 2)
    return out, boxes


def _cyclic_error(dev, ref):
    return min(float(np.abs(np.roll(dev, s, axis=0) - ref).max()) for s in range(4))


def _few_hits(scan, hits):
    ranges = np.full(len(scan["ranges"]), float(scan["range_max"]))
    ranges[:hits] = 4.0
    return dict(scan, ranges=ranges)


@pytest.fixture(scope="module")
def scans():
    """{name: (state (3, 1), scan)}: the five poses of the table at 360 beams, the room at 4096 beams, 3 hits, none"""
    out = {}
    for k, (cfg, pose) in enumerate(POSES):
        env = world_at(cfg, pose)
        out[f"pose{k}"] = (env.robot.state.copy(), env.get_lidar_scan())
    env = world_at(room_cfg(), (3, 1, 0.7), beams=4096)
    out["room4096"] = (env.robot.state.copy(), env.get_lidar_scan())
    st, scan = out["pose0"]
    out["hits3"], out["hits0"] = (st, _few_hits(scan, 3)), (st, _few_hits(scan, 0))
    return out


@pytest.fixture(scope="module")
def spec(scans):
    return {k: _spec(st, s) for k, (st, s) in scans.items()}


@pytest.fixture(scope="module")
def planner(hip):
    return _mpc()


# ---- (a) the device against the specification ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pose0", "pose1", "pose2", "pose3", "pose4", "room4096", "hits3", "hits0"])
def test_segments_and_boxes_equal_the_specification(planner, scans, spec, name):
    state, scan = scans[name]
    want, ref = spec[name]
    assert _split(planner, TOL_SPLIT) == 0
    boxes, labels, n = _device(planner, state, scan)
    assert _split(planner, 0.0) == 0
    differ = np.flatnonzero(labels != want)
    print(f"{name}: {len(scan['ranges'])} beams, {(want > -2).sum()} hits, segments {n} / {len(ref)}, labels differ at {differ[:8].tolist()}")
    if name == "room4096":
        assert (want >= 0).all() and len(want) == 4096                     # every beam hits, one cluster: the LDS worst case
    if name.startswith("hits"):
        assert n == 0 and len(ref) == 0
    assert np.array_equal(labels, want)
    assert n == len(ref)
    worst = max([_cyclic_error(boxes[c], ref[c]) for c in range(n)] + [0.0])
    print(f"{name}: worst corner error {worst:.3g} m")
    assert worst < TOL


# ---- (b) off is off ---------------------------------------------------------------------------------------------------------------------------------
def test_tol_zero_after_a_split_call_is_the_unsplit_kernel_and_bad_tol_changes_nothing(scans):
    a, b = _mpc(), _mpc()                                                   # b never splits
    for name in ("pose1", "pose3", "room4096", "hits3"):
        state, scan = scans[name]
        assert _split(a, TOL_SPLIT) == 0
        on = _device(a, state, scan)
        assert _split(a, 0.0) == 0
        off, never = _device(a, state, scan), _device(b, state, scan)
        assert off[2] == never[2] and np.array_equal(off[1], never[1]) and np.array_equal(off[0], never[0]), name
        if not name.startswith("hits"):
            assert on[2] > off[2], name
    state, scan = scans["pose1"]
    assert _split(a, TOL_SPLIT) == 0
    on = _device(a, state, scan)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        assert _split(a, bad) == RDA_ERR_ARG
        again = _device(a, state, scan)                                     # the previous value is still in force
        assert again[2] == on[2] and np.array_equal(again[1], on[1]) and np.array_equal(again[0], on[0]), bad
    assert a.rda._be.api.set_scan_split(None, 0.1) == RDA_ERR_ARG and a.rda._be.api.fleet_set_scan_split(None, 0.1) == RDA_ERR_ARG
    # the Python route: split=tol, and the next call without it is unsplit again
    obs = lidar.scan_box_split_device(a, state, scan)
    assert len(obs) == on[2] and all(np.array_equal(o.vertex.T, on[0][c]) for c, o in enumerate(obs))
    assert len(lidar.scan_box_device(a, state, scan)) == _device(b, state, scan)[2]


# ---- (c) a fleet of three --------------------------------------------------------------------------------------------------------------------------
def _slots(mpc):
    api, h = mpc.rda._be.api, mpc.rda._be.handle
    T, N, E = mpc.rda.T, mpc.rda.max_obs_num, mpc.rda.max_edge_num
    A = np.zeros((N, T + 1, E, 2)); b = np.zeros((N, T + 1, E)); cone = np.zeros(N, np.int32); nt = np.zeros(1, np.int32)
    assert api.get_obstacles(h, dptr(A), dptr(b), iptr(cone), iptr(nt)) == 0
    k = int(nt[0])
    return A.ravel()[: N * k * E * 2].copy(), b.ravel()[: N * k * E].copy(), cone.copy(), k


def test_fleet_of_three_equals_the_solo_calls_and_stages_the_same_boxes(hip, scans):
    names = ("pose1", "pose4", "pose2")
    states, scs = [scans[k][0] for k in names], [scans[k][1] for k in names]
    memb, solo = [_mpc() for _ in names], [_mpc() for _ in names]
    fleet, twin_members = Fleet(memb), [_mpc() for _ in names]
    twin = Fleet(twin_members)
    want = []
    for m, st, s in zip(solo, states, scs):
        assert _split(m, TOL_SPLIT) == 0
        want.append(_device(m, st, s))
    # the members' own values are not read by fleet calls: member 0 is split, the fleet is not
    assert _split(memb[0], TOL_SPLIT) == 0
    plain = fleet.scan_boxes(states, scs)
    assert len(plain[0]) == len(lidar.scan_box(states[0], scs[0])) < want[0][2]
    got = fleet.scan_boxes(states, scs, split=TOL_SPLIT)
    assert len({w[2] for w in want}) >= 2
    for i, (wb, _, wn) in enumerate(want):
        assert len(got[i]) == wn and np.array_equal(got[i], wb), i
    # labels too, through the C entry
    nb = np.array([len(s["ranges"]) for s in scs], np.int32)
    allr = np.ascontiguousarray(np.concatenate([np.asarray(s["ranges"], float) for s in scs]))
    lo, hi, rmax = (np.array([float(s[k]) for s in scs]) for k in ("angle_min", "angle_max", "range_max"))
    st = np.ascontiguousarray(np.array([np.asarray(x, float).ravel()[0:3] for x in states]))
    n, labels = np.zeros(3, np.int32), np.full(int(nb.sum()), -9, np.int32)
    fleet.set_scan_split(TOL_SPLIT)
    assert hip.fleet_scan_boxes(fleet._handle, iptr(nb), dptr(allr), dptr(lo), dptr(hi), dptr(rmax), dptr(st), EPS, MIN_SAMPLES, iptr(n), None, 0,
                                iptr(labels)) == 0
    assert np.array_equal(n, [w[2] for w in want]) and np.array_equal(labels, np.concatenate([w[1] for w in want]))
    # staged: rda_fleet_upload_scans with split == rda_fleet_upload_scenes of the device's boxes as polygons, slots and then a whole tick
    counts = fleet.upload_scans(states, scs, split=TOL_SPLIT)
    fleet.sync()
    assert np.array_equal(counts, [w[2] for w in want])
    lists = [[lidar.Obstacle(None, None, np.ascontiguousarray(b.T), "Rpositive", np.zeros((2, 1))) for b in w[0]] for w in want]
    assert twin._stage_all(lists, np.ascontiguousarray(st))
    twin.sync()
    for i in range(3):
        sa, sb = _slots(memb[i]), _slots(twin_members[i])
        assert sa[3] == sb[3] and all(np.array_equal(x, y) for x, y in zip(sa[:3], sb[:3])), i
    path_states = [np.array([[1.0 + i], [20.0], [0.0]]) for i in range(3)]
    res = fleet.control([s.copy() for s in path_states], 4, scans=scs, scan_split=TOL_SPLIT)
    lists = [lidar.scan_box_split_device(solo[i], path_states[i], scs[i]) for i in range(3)]
    ref = twin.control([s.copy() for s in path_states], 4, lists)
    for i in range(3):
        assert np.array_equal(res[i][0], ref[i][0]) and res[i][1]["iters"] == ref[i][1]["iters"] and res[i][1]["resi_pri"] == ref[i][1]["resi_pri"], i
    # ... and the next tick without scan_split is unsplit again
    res = fleet.control([s.copy() for s in path_states], 4, scans=scs)
    ref = twin.control([s.copy() for s in path_states], 4, [lidar.scan_box_device(solo[i], path_states[i], scs[i]) for i in range(3)])
    for i in range(3):
        assert np.array_equal(res[i][0], ref[i][0]) and res[i][1]["iters"] == ref[i][1]["iters"], i
    fleet.close(); twin.close()


# ---- (d) the rollout --------------------------------------------------------------------------------------------------------------------------------
def test_rollout_ticks_equal_host_driven_ticks_under_the_same_setting(hip):
    """K = 3 ticks of rda_fleet_rollout_lidar with split, B = 2: every tick == rda_fleet_raycast + rda_fleet_upload_scans + rda_fleet_step_tracked of a
    twin fleet with the same setting (box count, first control, min_index, rda_info), and the split changes the box counts of these lanes"""
    from fleet_twin_lib import compare_ticks
    from test_gpu_fleet_rollout_lidar import TICK, Twin
    a, b, c = Twin(hip, which=(0, 1)), Twin(hip, which=(0, 1)), Twin(hip, which=(0, 1))
    assert hip.fleet_set_scan_split(a.F, TOL_SPLIT) == 0 and hip.fleet_set_scan_split(b.F, TOL_SPLIT) == 0
    rc, logs = a.rollout(3, 0)
    assert rc == 0, rc
    ticks = b.forced(logs, 3, b.base, lambda k: 0.0, b.cur0, True)
    assert compare_ticks(logs, ticks, 3, TICK) == 6
    rc, plain = c.rollout(3, 0)
    assert rc == 0
    print("boxes per tick, split:", logs["boxes"].T.tolist(), " unsplit:", plain["boxes"].T.tolist())
    assert (logs["boxes"] >= plain["boxes"]).all() and (logs["boxes"] > plain["boxes"]).any()
    a.close(); b.close(); c.close()


# ---- (e) the closed loop round the bend --------------------------------------------------------------------------------------------------------------
def _device_bend_loop(split):
    from test_lidar_split import BEND_DT, BEND_E, BEND_ITER, BEND_N, BEND_SPEED, BEND_START, BEND_T, BEND_TICKS, bend_car, bend_path, corridor_cfg
    env = world_at(corridor_cfg(), BEND_START)
    m = MPC(bend_car(), bend_path(), receding=BEND_T, sample_time=BEND_DT, iter_num=BEND_ITER, max_edge_num=BEND_E, max_obs_num=BEND_N)
    fleet = Fleet([m])
    kw = {"scan_split": TOL_SPLIT} if split else {}
    out = fleet.rollout([env.robot.state.copy()], BEND_SPEED, BEND_TICKS, lidar=[env.lidar], world=[env.obstacles], clearance=True, **kw)
    fleet.close()
    tick = int(out["arrived_at"][0])
    moved = out["clearance"][:tick if tick >= 0 else BEND_TICKS, 0]
    return tick, float(moved.min()), out["boxes"][:, 0]


def test_device_loop_round_the_bend():
    """Fleet.rollout(lidar=, world=, clearance=True, scan_split=0.15) of one differential robot (1.0 x 0.6 m) through the L-shaped corridor, 5 m before
    the bend to 7 m behind it: T = 5, N = 6, E = 4, iter_num = 2, dt = 0.1, 2 m/s, 80 ticks at most, 360 beams, 15 m, eps 2.0, min_samples 6.
    The same loop on the CPU checker fed by lidar.scan_box_split (tests/test_lidar_split.py::test_oracle_loop_round_the_bend): arrival at tick 68,
    minimum clearance +0.917 m against the true walls.  Asserted of the device: it arrives, with a positive minimum clearance, as the checker does.
    The unsplit twin (one box per cluster: the robot stands inside its obstacle) arrives on the checker too, at tick 64 with +0.367 m - the loop is
    then driven by constraints that cannot hold, so its outcome is printed and nothing is asserted about it."""
    tick, worst, boxes = _device_bend_loop(True)
    print(f"split: arrives at tick {tick}, minimum clearance {worst:+.3f} m, boxes per tick {int(boxes.min())} .. {int(boxes.max())}")
    plain = _device_bend_loop(False)
    print(f"one box per cluster: tick {plain[0]}, minimum clearance {plain[1]:+.3f} m, boxes per tick {int(plain[2].min())} .. {int(plain[2].max())}")
    assert tick > 0 and worst > 0.0
