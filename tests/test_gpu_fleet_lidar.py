"""-m gpu : the fleet lidar (rda_fleet_scan_boxes / rda_fleet_upload_scans, lidar::k_scan_fleet, k_scene_fill_fleet, Fleet.control(scans=)) against the
per-member calls it batches (rda_scan_boxes / rda_upload_scan, MPC.control(scan=)): the same device code runs per member, so counts, boxes, labels,
staged slots and controls are compared BIT FOR BIT (np.array_equal) - there is no tolerance in this file.  The per-member calls themselves are held
against the host specification by tests/test_gpu_lidar.py.

Scans are ray-cast by rda_planner_amd.world.World with fixed seeds; T = 10, N = 5, E = 4, iter_num = 2 unless stated."""
import ctypes as C
import gc

import numpy as np
import pytest

from rda_planner_amd import lidar
from rda_planner_amd import scenarios as sc
from rda_planner_amd import world as irsim
from rda_planner_amd._capi import dptr, iptr
from rda_planner_amd.fleet import Fleet
from rda_planner_amd.mpc import MPC

pytestmark = pytest.mark.gpu

RDA_ERR_ARG, RDA_ERR_UNSUPPORTED, RDA_ERR_HIP = -1, -2, -3
BEAMS = (7, 100, 181, 360, 1080)
ORDER = (1, 0, 1, 0, 1)
N_SLOTS = 5


# ---- helpers copied from tests/test_gpu_lidar.py (_world, _scan_c, _slots) ---------------------------------------------------------------------------
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


def _scan_c(scan, state):
    ranges = np.ascontiguousarray(np.asarray(scan["ranges"], float))
    st = np.ascontiguousarray(np.asarray(state, float).ravel()[0:3])
    return ranges, st, (len(ranges), dptr(ranges), float(scan["angle_min"]), float(scan["angle_max"]), float(scan["range_max"]), dptr(st))


def _slots(mpc):
    api, h = mpc.rda._be.api, mpc.rda._be.handle
    T, N, E = mpc.rda.T, mpc.rda.max_obs_num, mpc.rda.max_edge_num
    A = np.zeros((N, T + 1, E, 2)); b = np.zeros((N, T + 1, E)); cone = np.zeros(N, np.int32); nt = np.zeros(1, np.int32)
    assert api.get_obstacles(h, dptr(A), dptr(b), iptr(cone), iptr(nt)) == 0
    k = int(nt[0])
    return A.ravel()[: N * k * E * 2].copy(), b.ravel()[: N * k * E].copy(), cone.copy(), k


def _same_slots(a, b):
    return a[3] == b[3] and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


# ---- this file's own ---------------------------------------------------------------------------------------------------------------------------------
def _slot_src(mpc):
    lib = mpc.rda._be.api.lib
    N = mpc.rda.max_obs_num
    src, used = (C.c_int32 * N)(), C.c_int32(0)
    assert lib.rda_debug_slot_src(mpc.rda._be.handle, src, C.byref(used)) == 0
    return list(src[:used.value])


def _staged(mpc):
    return _slots(mpc), _slot_src(mpc)


def _same_staged(a, b):
    return _same_slots(a[0], b[0]) and a[1] == b[1]


def _mpc(N=N_SLOTS, E=4, T=10, **kw):
    return MPC(sc.rectangle_robot(), sc.line_path([0, 20, 0], [60, 20, 0]), receding=T, max_edge_num=E, max_obs_num=N, iter_num=2, **kw)


def _pack(items):
    """[(state, scan)] -> the member-major arrays of the fleet calls (kept alive by the caller)"""
    ranges = [np.asarray(s["ranges"], float).ravel() for _, s in items]
    nb = np.array([len(r) for r in ranges], np.int32)
    allr = np.ascontiguousarray(np.concatenate(ranges + [np.zeros(1)]))
    lo, hi, rmax = (np.array([float(s[k]) for _, s in items]) for k in ("angle_min", "angle_max", "range_max"))
    st = np.ascontiguousarray(np.array([np.asarray(x, float).ravel()[0:3] for x, _ in items]))
    return nb, allr, lo, hi, rmax, st


def _fleet_boxes(fleet, items, eps=2.0, min_samples=6, cap=None):
    """rda_fleet_scan_boxes -> (rc, n_boxes [B], boxes [B][cap][4][2] on a NaN ground, labels on a -9 ground)"""
    nb, allr, lo, hi, rmax, st = _pack(items)
    B = len(items)
    cap = int(nb.max()) if cap is None else cap
    boxes, n, labels = np.full((B, max(cap, 1), 4, 2), np.nan), np.zeros(B, np.int32), np.full(int(nb.sum()) + 1, -9, np.int32)
    rc = fleet.api.fleet_scan_boxes(fleet._handle, iptr(nb), dptr(allr), dptr(lo), dptr(hi), dptr(rmax), dptr(st), float(eps), int(min_samples),
                                    iptr(n), dptr(boxes), cap, iptr(labels))
    return rc, n, boxes, np.split(labels[:-1], np.cumsum(nb)[:-1])


def _fleet_upload(fleet, items, order, eps=2.0, min_samples=6, sync=True):
    nb, allr, lo, hi, rmax, st = _pack(items)
    order = np.array(order, np.int32)
    n = np.full(len(items), -7, np.int32)
    rc = fleet.api.fleet_upload_scans(fleet._handle, iptr(nb), dptr(allr), dptr(lo), dptr(hi), dptr(rmax), dptr(st), float(eps), int(min_samples),
                                      iptr(order), iptr(n))
    if rc == 0 and sync:
        assert fleet.api.fleet_sync(fleet._handle) == 0
    return rc, n


def _solo_boxes(mpc, state, scan, eps=2.0, min_samples=6):
    api, h = mpc.rda._be.api, mpc.rda._be.handle
    ranges, st, head = _scan_c(scan, state)
    cap = max(len(ranges), 1)
    boxes, n, labels = np.zeros((cap, 4, 2)), np.zeros(1, np.int32), np.full(cap, -9, np.int32)
    assert api.scan_boxes(h, *head, float(eps), int(min_samples), iptr(n), dptr(boxes), cap, iptr(labels)) == 0
    return int(n[0]), boxes[:int(n[0])], labels[:len(ranges)]


def _solo_upload(mpc, state, scan, order, eps=2.0, min_samples=6):
    api, h = mpc.rda._be.api, mpc.rda._be.handle
    ranges, st, head = _scan_c(scan, state)
    n = np.zeros(1, np.int32)
    assert api.upload_scan(h, *head, float(eps), int(min_samples), int(order), iptr(n)) == 0
    return int(n[0])


def _upload_boxes(mpc, boxes, robot_xy, order):
    """rda_upload_scene of (n, 4, 2) boxes as 4-vertex polygons without velocity"""
    api, h = mpc.rda._be.api, mpc.rda._be.handle
    n, E = len(boxes), mpc.rda.max_edge_num
    geom = np.zeros((n, E, 2)); geom[:, 0:4, :] = boxes
    kind, nvert, vel = np.zeros(n, np.int32), np.full(n, 4, np.int32), np.zeros((n, 2))
    rob = np.ascontiguousarray(np.asarray(robot_xy, float).ravel()[0:2])
    return api.upload_scene(h, n, iptr(kind), iptr(nvert), dptr(geom), dptr(vel), dptr(rob), int(order), None)


def _few_hits(scan, hits):
    ranges = np.full(len(scan["ranges"]), float(scan["range_max"]))
    ranges[:hits] = 4.0
    return dict(scan, ranges=ranges)


def _dense_scan(n=4096):
    """a synthetic scan of n beams: six wavy arcs (~ 360 hits each) with gaps between them (tests/test_gpu_lidar.py)"""
    ang = np.linspace(-np.pi + 0.005, np.pi - 0.005, n)
    r = 6.0 + np.sin(3 * ang) + 0.3 * np.sin(17 * ang)
    ranges = np.where(np.mod(ang + np.pi, 2 * np.pi / 6) < 0.52, r, 15.0)
    return {"ranges": ranges, "angle_min": float(ang[0]), "angle_max": float(ang[-1]), "range_max": 15.0}


@pytest.fixture(scope="module")
def scans():
    """five (state (3, 1), scan): 7, 100, 181, 360, 1080 beams, distinct poses, half and (just under) full field of view in turn;
    lidar.scan_box finds 0, 3, 3, 6, 3 boxes in them (asserted on the device counts where it matters)"""
    out = []
    for k, beams in enumerate(BEAMS):
        env = _world(np.random.default_rng(61200 + k), beams, np.pi if k % 2 == 0 else 2 * np.pi - 0.01)
        out.append((env.robot.state.copy(), env.get_lidar_scan()))
    return out


@pytest.fixture(scope="module")
def twins(hip):
    """a fleet of five members and five solo planners of the same make"""
    memb, solo = [_mpc() for _ in BEAMS], [_mpc() for _ in BEAMS]
    fleet = Fleet(memb)
    yield fleet, memb, solo
    fleet.close()


@pytest.fixture(scope="module")
def solo_staged(twins, scans):
    """the reference of tests 2 and 8, computed once: what rda_upload_scan(ORDER[i]) of scan i leaves on solo planner i"""
    _, _, solo = twins
    out = []
    for i, (state, scan) in enumerate(scans):
        n = _solo_upload(solo[i], state, scan, ORDER[i])
        out.append((n, _staged(solo[i])))
    return out


# ---- 1. the kernel against the solo kernel -----------------------------------------------------------------------------------------------------------
def test_fleet_scan_boxes_equal_solo_scan_boxes(twins, scans):
    fleet, _, solo = twins
    assert {len(s["ranges"]) for _, s in scans} == set(BEAMS) and len({tuple(st.ravel()) for st, _ in scans}) == len(BEAMS)
    assert len({round(s["angle_max"] - s["angle_min"], 3) for _, s in scans}) == 2               # both fields of view
    want = [_solo_boxes(solo[i], st, s) for i, (st, s) in enumerate(scans)]
    rc, n, boxes, labels = _fleet_boxes(fleet, scans)
    assert rc == 0
    assert np.array_equal(n, [w[0] for w in want]) and n.max() >= 3
    for i, (wn, wb, wl) in enumerate(want):
        assert np.array_equal(labels[i], wl), i
        assert np.array_equal(boxes[i, :wn], wb), i
        assert np.isnan(boxes[i, wn:]).all(), i                                                  # nothing written behind a member's boxes
    # fewer rows than one member has boxes: the counts stay, only the first `cap` boxes are written
    cap = int(n.max()) - 2
    assert cap >= 1 and (n > cap).any() and (n < cap).any()
    rc, n2, few, labels2 = _fleet_boxes(fleet, scans, cap=cap)
    assert rc == 0 and np.array_equal(n2, n) and few.shape[1] == cap
    for i, (wn, wb, wl) in enumerate(want):
        k = min(wn, cap)
        assert np.array_equal(few[i, :k], wb[:k]) and np.isnan(few[i, k:]).all() and np.array_equal(labels2[i], wl), i
    # the Python drop-in
    obs = lidar.scan_box_device_fleet(fleet, [st for st, _ in scans], [s for _, s in scans])
    assert [len(o) for o in obs] == list(n)
    assert all(np.array_equal(o.vertex.T, wb[c]) for o_list, (_, wb, _) in zip(obs, want) for c, o in enumerate(o_list))


# ---- 2. staging against solo staging -----------------------------------------------------------------------------------------------------------------
def test_fleet_upload_scans_equal_solo_upload_scan(twins, scans, solo_staged):
    fleet, memb, _ = twins
    rc, n = _fleet_upload(fleet, scans, ORDER)
    assert rc == 0 and np.array_equal(n, [w[0] for w in solo_staged])
    assert (n > N_SLOTS).any() and ((n > 0) & (n < N_SLOTS)).any()                               # truncation; padding quirk Q3
    for i, (wn, want) in enumerate(solo_staged):
        if wn > 0:
            assert _same_staged(_staged(memb[i]), want), i
            assert want[0][3] == 1 and len(want[1]) == min(wn, N_SLOTS)


# ---- 3. empty and ragged members ---------------------------------------------------------------------------------------------------------------------
def test_members_without_boxes_keep_their_slots_and_skip_the_dual_side(scans):
    memb, solo = [_mpc() for _ in range(5)], [_mpc() for _ in range(5)]
    fleet = Fleet(memb)
    first = [scans[k] for k in (1, 2, 3, 4, 3)]                                                  # boxes for every member
    state = np.array([[0.0], [20.0], [0.0]])                                                     # on the members' path, for the step below
    first = [(state, s) for _, s in first]
    rc, n = _fleet_upload(fleet, first, ORDER)
    assert rc == 0 and (n > 0).all()
    for i, (st, s) in enumerate(first):
        assert _solo_upload(solo[i], st, s, ORDER[i]) == n[i]
    before = [_staged(m) for m in memb]
    assert all(_same_staged(b, _staged(s)) for b, s in zip(before, solo))
    miss = _few_hits(scans[3][1], 0)
    none = dict(scans[1][1], ranges=np.zeros(0))                                                 # n_beams = 0
    three = _few_hits(scans[2][1], 3)
    second = [(state, miss), (state, none), (state, three), (state, scans[1][1]), (state, scans[4][1])]
    rc, n = _fleet_upload(fleet, second, ORDER)
    assert rc == 0 and list(n[:3]) == [0, 0, 0] and (n[3:] > 0).all()
    for i, (st, s) in enumerate(second):
        s = miss if i == 1 else s                                                                # (the solo call's ctypes binding wants a non-empty array)
        assert _solo_upload(solo[i], st, s, ORDER[i]) == n[i]
    after = [_staged(m) for m in memb]
    assert all(_same_slots(after[i][0], before[i][0]) for i in range(3))                         # old slots stay
    assert all(_same_staged(after[i], _staged(solo[i])) and not _same_slots(after[i][0], before[i][0]) for i in (3, 4))
    # the step behind it: obstacle-free (dual side skipped) for members 0 - 2, as on the solo route
    for tick in range(2):
        res = fleet.control([state.copy() for _ in memb], 4.0, scans=[s for _, s in second])
        for i in range(5):
            u, info = solo[i].control(state.copy(), 4.0, scan=miss if i == 1 else second[i][1])
            uf, inf = res[i]
            assert np.array_equal(u, uf) and (i > 2 or np.isfinite(uf).all()), (tick, i)
            assert all(info[k] == inf[k] for k in ("resi_dual", "resi_pri", "iters", "status", "su_ipm_iters", "lmz_fail", "arrive")), (tick, i)
    free = _mpc()
    u0, i0 = free.control(state.copy(), 4.0, [])                                                 # no obstacles at all: the same first tick
    fresh_f = _mpc()
    ff = Fleet([fresh_f])
    uf, inf = ff.control([state.copy()], 4.0, scans=[miss])[0]
    assert np.array_equal(u0, uf) and i0["iters"] == inf["iters"] and i0["resi_pri"] == inf["resi_pri"]
    ff.close(); fleet.close()


# ---- 4. control --------------------------------------------------------------------------------------------------------------------------------------
def _track_world(k):
    """member k's own world: it starts near the head of the line path of `_mpc` ((0, 20) -> (60, 20)) and sees, with a 15 m / 180 degree lidar of 100
    beams, circles and boxes on both sides of the path ahead"""
    rng = np.random.default_rng(63000 + k)
    state = [1.0 + 0.5 * k, 20.0 + 0.2 * k, 0.02 * k]
    obstacles = []
    for j in range(5):
        pos = [7.0 + 4.0 * j + float(rng.uniform(-1, 1)), 20.0 + (4.5 if j % 2 else -4.5) + float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-np.pi, np.pi))]
        shape = {"name": "circle", "radius": 1.0} if j % 3 == 0 else {"name": "rectangle", "length": 2.5, "width": 1.2}
        obstacles.append({"number": 1, "distribution": {"name": "manual"}, "state": [pos], "shape": [shape]})
    cfg = {"world": {"step_time": 0.1},
           "robot": [{"kinematics": {"name": "acker"}, "shape": {"name": "rectangle", "length": 4.6, "width": 1.6, "wheelbase": 3}, "state": state,
                      "sensors": [{"type": "lidar2d", "range_max": 15.0, "angle_range": np.pi, "number": 100}]}],
           "obstacle": obstacles}
    return irsim.World(cfg)


@pytest.mark.parametrize("tracked", [True, False], ids=["tracked", "untracked"])
def test_fleet_control_with_scans_equals_member_control_with_scan(hip, tracked):
    envs = [_track_world(k) for k in range(4)]
    memb, solo = [_mpc() for _ in envs], [_mpc() for _ in envs]
    for m in memb + solo:
        m.device_track = tracked
    assert all(m._tracks({}) == tracked for m in memb)
    fleet = Fleet(memb)
    seen, scans0 = 0, None
    for tick in range(6):
        states = [e.robot.state.copy() for e in envs]
        scans_t = [e.get_lidar_scan() for e in envs]
        if tick == 0:
            scans0 = [np.asarray(s["ranges"], float).copy() for s in scans_t]
        res = fleet.control([s.copy() for s in states], 4, scans=scans_t)
        for i, env in enumerate(envs):
            u, info = solo[i].control(states[i].copy(), 4, scan=scans_t[i])
            uf, inf = res[i]
            assert np.array_equal(u, uf), (tick, i, u.ravel(), uf.ravel())
            assert all(np.array_equal(x, y) for x, y in zip(info["opt_state_list"], inf["opt_state_list"])), (tick, i)
            assert memb[i].cur_index == solo[i].cur_index and info["arrive"] == inf["arrive"] and info["iters"] == inf["iters"], (tick, i)
            assert np.array_equal(memb[i].cur_vel_array, solo[i].cur_vel_array)
            env.step(u)
        seen = max(seen, max(len(lidar.scan_box(states[i], scans_t[i])) for i in range(len(envs))))
    assert seen >= 2                                                                             # there was something to avoid
    assert all(not np.array_equal(np.asarray(e.get_lidar_scan()["ranges"], float), r0) for e, r0 in zip(envs, scans0))     # the robots moved
    fleet.close()


# ---- 5. resort afterwards ----------------------------------------------------------------------------------------------------------------------------
def _fleet_resort(fleet, xy):
    st = np.ascontiguousarray(np.hstack([xy, np.zeros((len(xy), 1))]))
    rc = fleet.api.fleet_scene_resort(fleet._handle, dptr(st), 3)
    assert fleet.api.fleet_sync(fleet._handle) == 0
    return rc


def test_resort_after_fleet_upload_scans_and_on_host_uploaded_scenes(twins, scans):
    fleet, memb, solo = twins
    items = [scans[k] for k in (1, 2, 3, 4, 3)]                                                  # every member has boxes
    rc, n = _fleet_upload(fleet, items, ORDER)
    assert rc == 0 and (n > 0).all()
    for i, (st, s) in enumerate(items):
        _solo_upload(solo[i], st, s, ORDER[i])
    for shift in ([6.0, -4.0], [-9.0, 7.5]):
        xy = np.array([st[0:2, 0] + np.array(shift) * (1 + 0.1 * i) for i, (st, _) in enumerate(items)])
        assert _fleet_resort(fleet, xy) == 0
        for i in range(5):
            there = np.ascontiguousarray(xy[i])
            assert solo[i].rda._be.api.scene_resort(solo[i].rda._be.handle, dptr(there)) == 0
            assert _same_staged(_staged(memb[i]), _staged(solo[i])), (shift, i)
    # a member's own re-sort after the fleet has synchronised works on the staged scene too
    there = np.ascontiguousarray(items[2][0][0:2, 0] + 3.0)
    for m in (memb[2], solo[2]):
        assert m.rda._be.api.scene_resort(m.rda._be.handle, dptr(there)) == 0
    assert _same_staged(_staged(memb[2]), _staged(solo[2]))
    # scenes uploaded from the host (the route the fleet re-sort had before this file's feature): still the per-member call's slots
    for i, (st, s) in enumerate(items):
        _, boxes, _ = _solo_boxes(solo[i], st, s)
        for m in (memb[i], solo[i]):
            assert _upload_boxes(m, boxes, st[0:2], 1) == 0
    xy = np.array([st[0:2, 0] + np.array([-5.0, 2.0 + i]) for i, (st, _) in enumerate(items)])
    assert _fleet_resort(fleet, xy) == 0
    for i in range(5):
        there = np.ascontiguousarray(xy[i])
        assert solo[i].rda._be.api.scene_resort(solo[i].rda._be.handle, dptr(there)) == 0
        assert _same_staged(_staged(memb[i]), _staged(solo[i])), i


# ---- 6. full width -----------------------------------------------------------------------------------------------------------------------------------
def test_64_members_and_a_4096_beam_member(hip):
    B, big = 64, 17
    handful = []
    for k in range(6):
        env = _world(np.random.default_rng(62000 + k), 360, np.pi if k % 2 else 2 * np.pi - 0.01)
        handful.append(env.get_lidar_scan())
    dense = _dense_scan()
    assert int((dense["ranges"] < 15.0 - 0.01).sum()) > 2000
    items = []
    for i in range(B):
        state = np.array([[10.0 + 0.37 * i], [12.0 + 0.21 * ((7 * i) % 64)], [-3.0 + 0.09 * i]])
        items.append((state, dense if i == big else handful[i % len(handful)]))
    memb = [_mpc() for _ in range(B)]
    fleet = Fleet(memb)
    order = [(i // 2) % 2 for i in range(B)]
    rc, n, boxes, labels = _fleet_boxes(fleet, items, eps=0.5, cap=64)
    assert rc == 0 and n[big] >= 6 and len(set(n.tolist())) >= 3
    rc, n2 = _fleet_upload(fleet, items, order, eps=0.5)
    assert rc == 0 and np.array_equal(n, n2)
    for i in (0, 31, 63, big):
        ref = _mpc()
        wn, wb, wl = _solo_boxes(ref, *items[i], eps=0.5)
        assert wn == n[i] and np.array_equal(boxes[i, :wn], wb) and np.array_equal(labels[i], wl), i
        assert _solo_upload(ref, *items[i], order[i], eps=0.5) == wn
        assert wn > 0 and _same_staged(_staged(memb[i]), _staged(ref)), i
    fleet.close()


# ---- 7. limits ---------------------------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_and_stage_nothing(twins, scans):
    fleet, memb, _ = twins
    good = [scans[k] for k in (1, 2, 3, 4, 3)]
    rc, n = _fleet_upload(fleet, good, ORDER)
    assert rc == 0
    before = [_staged(m) for m in memb]
    other = [scans[k] for k in (4, 3, 2, 1, 1)]                                                  # what a call that went through would stage instead
    big = (scans[2][0], _dense_scan(4097))

    def refused(code, items, **kw):
        rc_u, _ = _fleet_upload(fleet, items, ORDER, **kw)
        rc_b = _fleet_boxes(fleet, items, **kw)[0]
        assert (rc_u, rc_b) == (code, code), (code, rc_u, rc_b, kw)
        assert all(_same_staged(_staged(m), b) for m, b in zip(memb, before))

    refused(RDA_ERR_UNSUPPORTED, other[:2] + [big] + other[3:])
    refused(RDA_ERR_ARG, other, eps=0.0)
    refused(RDA_ERR_ARG, other, eps=float("nan"))
    refused(RDA_ERR_ARG, other, min_samples=0)
    # a missing array, a negative beam count
    nb, allr, lo, hi, rmax, st = _pack(other)
    order, out = np.array(ORDER, np.int32), np.zeros(5, np.int32)
    api, h = fleet.api, fleet._handle
    full = [iptr(nb), dptr(allr), dptr(lo), dptr(hi), dptr(rmax), dptr(st)]
    for k in range(6):
        args = list(full); args[k] = None
        assert api.fleet_upload_scans(h, *args, 2.0, 6, iptr(order), iptr(out)) == RDA_ERR_ARG, k
        assert api.fleet_scan_boxes(h, *args, 2.0, 6, iptr(out), None, 0, None) == RDA_ERR_ARG, k
    assert api.fleet_upload_scans(h, *full, 2.0, 6, None, iptr(out)) == RDA_ERR_ARG
    assert api.fleet_scan_boxes(h, *full, 2.0, 6, None, None, 0, None) == RDA_ERR_ARG
    neg = nb.copy(); neg[1] = -1
    assert api.fleet_upload_scans(h, iptr(neg), *full[1:], 2.0, 6, iptr(order), iptr(out)) == RDA_ERR_ARG
    assert all(_same_staged(_staged(m), b) for m, b in zip(memb, before))
    # the count array may be left out
    assert api.fleet_upload_scans(h, *full, 2.0, 6, iptr(order), None) == 0 and api.fleet_sync(h) == 0
    assert not _same_staged(_staged(memb[0]), before[0])


@pytest.mark.parametrize("what", ["E3", "duals_follow"])
def test_unsupported_fleets_are_refused(hip, scans, what):
    if what == "E3":
        memb = [_mpc(E=3) for _ in range(2)]
    else:
        memb = [_mpc(), _mpc(duals_follow_obstacles=True)]
    fleet = Fleet(memb)
    before = [_slots(m) for m in memb]
    items = [scans[3], scans[4]]
    rc, _ = _fleet_upload(fleet, items, (1, 1))
    assert rc == RDA_ERR_UNSUPPORTED
    assert _fleet_boxes(fleet, items)[0] == (RDA_ERR_UNSUPPORTED if what == "E3" else 0)         # duals follow the STAGED scene: a plain scan is fine
    assert all(_same_slots(_slots(m), b) for m, b in zip(memb, before))
    fleet.close()


# ---- 8. refused allocation ---------------------------------------------------------------------------------------------------------------------------
def _live(hip):
    n, b = C.c_longlong(0), C.c_longlong(0)
    assert hip.debug_alloc_stats(C.byref(n), C.byref(b)) == 0
    return n.value, b.value


def test_refused_allocation_changes_and_leaks_nothing(hip, scans, solo_staged):
    """every allocation of a first rda_fleet_upload_scans on a fleet (the fleet's lidar tables and buffers, then a larger raw scene for every member
    whose boxes do not fit the one it has) refused in turn by the host-side hook: RDA_ERR_HIP, the live-allocation counters and every member's
    staged slots as they were; then the call goes through and stages what test 2 pins"""
    gc.collect()                                                           # no handle of an earlier test is released while this one counts
    memb = [_mpc() for _ in BEAMS]
    fleet = Fleet(memb)
    for m, (st, _) in zip(memb, scans):                                    # a resident scene of ONE box: every scan with more boxes needs a larger one
        assert _upload_boxes(m, np.array([[[1.0, 1.0], [2.0, 1.0], [2.0, 2.0], [1.0, 2.0]]]) + st[0:2, 0], st[0:2], 1) == 0
    before = [_staged(m) for m in memb]
    refused, rc, live = 0, None, None
    for k in range(80):
        live = _live(hip)
        hip.debug_alloc_fail(k)
        try:
            rc, n = _fleet_upload(fleet, scans, ORDER, eps=1e-3, min_samples=1)      # every hit a cluster of its own: more boxes than reserved
        finally:
            hip.debug_alloc_fail(-1)
        if rc != RDA_ERR_HIP:
            break
        refused += 1
        assert _live(hip) == live, (k, live, _live(hip))
        assert all(_same_staged(_staged(m), b) for m, b in zip(memb, before)), k
    assert rc == 0 and refused >= 9 + 3 * 4, (rc, refused)                 # 9 of the fleet, 3 device buffers for each of the four larger scenes
    assert n[4] > 19 and _live(hip)[0] > live[0]
    ref = _mpc()
    for i in (1, 4):
        assert _solo_upload(ref, *scans[i], ORDER[i], eps=1e-3, min_samples=1) == n[i]
        assert _same_staged(_staged(memb[i]), _staged(ref)), i
    # the retry with the parameters of test 2: equal to the solo staging pinned there
    rc, n = _fleet_upload(fleet, scans, ORDER)
    assert rc == 0 and np.array_equal(n, [w[0] for w in solo_staged])
    assert all(_same_staged(_staged(m), want) for m, (wn, want) in zip(memb, solo_staged) if wn > 0)
    fleet.close()
