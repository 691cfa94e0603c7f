"""-m gpu : the lidar rollout (rda_fleet_rollout_lidar: lidar::k_raycast_fleet -> k_scan_fleet_at -> the staging of rda_fleet_upload_scans -> ADMM ->
rollout::k_rollout_advance, the world moved by scene::k_move_fleet; Fleet.rollout(lidar=, world=)) against the host-driven loop it replaces.  A twin fleet is fed
the logged states and the world advanced in numpy (base + vel * (dt * k), the `advanced` rule of tests/test_gpu_fleet_rollout_moving.py) and runs, per tick,
rda_fleet_upload_worlds -> rda_fleet_raycast -> rda_fleet_upload_scans -> rda_fleet_step_tracked: every control, path index, rda_info, box count and the staged
slots must come out bit for bit.  The world after the call equals the numpy-advanced one; the clearance log is within 1e-9 m of scenarios.clearance against
the world (the project's bound for device geometry against its numpy specification, as in that file).

Shapes (those of that file): T = 8, N = 4, E = 4, iter_num = 2, dt = 0.1; B = 3 (Ackermann, differential, omni) on their lanes, the 7 obstacles per member as
the WORLD (we = 4), member 2's standing; sensors (beams, field of view, range_max): (100, pi, 10), (257, 2 pi, 10), (64, 2 pi, 3); eps 2.0, min_samples 6;
K = 12, then a second rollout of 5, with `moving` on and off.  With the numpy front end along the lanes member 0 sees 2 - 4 boxes (<= N), member 1 5 - 7
(> N: truncation), member 2 alternates between 0 and 1 (the zero-box rule and the flip of the LamMuZ launch form)."""
import ctypes as C

import numpy as np
import pytest

from fleet_twin_lib import (DT, E, ITER, MARGIN, N, NOBS, RDA_ERR_ARG, RDA_ERR_HIP, RDA_ERR_UNSUPPORTED, SPEED, T, FleetTwin, advanced, car, compare_ticks,
                            info_tuple, same_logs, solver)
from lidar_world_lib import EPS, MIN_SAMPLES, SENSORS, WE, lane, numpy_scan, sensor_c
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import Info, dptr, iptr

pytestmark = pytest.mark.gpu

K, K2 = 12, 5
LOGS = ("states", "controls", "index", "arrived_at", "boxes", "clearance")
TICK = ("boxes", "controls", "index", "info")          # what a rollout tick is compared for with a host-driven one


class Twin(FleetTwin):
    """a fleet of fresh handles of the three lane members (paths uploaded, nothing staged), the flattened worlds, and what a caller keeps beside it"""
    def __init__(self, hip, which=(0, 1, 2), world=True, **kw):
        self.which = which
        made = [solver(hip, e, scene=False, **kw) for e in which]
        self.make_fleet(hip, [m[0] for m in made])
        self.states = np.ascontiguousarray(np.array([m[1] for m in made]))
        self.plen = [m[2] for m in made]
        self.kind, self.nvert, self.base, self.vel = (np.ascontiguousarray(np.concatenate([m[3][j] for m in made])) for j in range(4))
        self.counts = np.full(self.B, NOBS, np.int32)
        self.sensors = sensor_c([SENSORS[e] for e in which])
        self.order = np.ones(self.B, np.int32)
        if world:
            self.upload_world(self.base)

    def upload_world(self, geom, vel=True):
        assert self.hip.fleet_upload_worlds(self.F, iptr(self.counts), WE, iptr(self.kind), iptr(self.nvert), dptr(np.ascontiguousarray(geom)),
                                            dptr(self.vel) if vel else None) == 0

    def world(self):
        g, n, we = np.full((self.B * NOBS, WE, 2), np.nan), np.zeros(1, np.int32), np.zeros(1, np.int32)
        assert self.hip.debug_fleet_world(self.F, dptr(g), iptr(n), iptr(we)) == 0 and n[0] == self.B * NOBS and we[0] == WE
        return g

    def rollout(self, k, moving, clearance=True, **over):
        """rda_fleet_rollout_lidar -> (rc, dict of logs); over: arguments replaced (None = a missing array)"""
        out = self.logs(k, boxes=np.int32, clearance=float if clearance else None)
        nb, lo, hi, rmin, rmax = self.sensors
        a = dict(states=self.states, ref_speed=self.speed, cur_index=self.cur0, threshold=0.1, ind_range=10, goal_margin=MARGIN, nom_u=self.nom0,
                 n_beams=nb, angle_min=lo, angle_max=hi, range_min=rmin, range_max=rmax, eps=EPS, min_samples=MIN_SAMPLES, order=self.order,
                 states_log=out["states"], u_log=out["controls"], index_log=out["index"], info_log=out["info"], arrived_at=out["arrived_at"],
                 nbox_log=out["boxes"])
        a.update(over)
        rc = self.hip.fleet_rollout_lidar(self.F, k, dptr(a["states"]), dptr(a["ref_speed"]), iptr(a["cur_index"]), a["threshold"], a["ind_range"],
                                          a["goal_margin"], dptr(a["nom_u"]), iptr(a["n_beams"]), dptr(a["angle_min"]), dptr(a["angle_max"]),
                                          dptr(a["range_min"]), dptr(a["range_max"]), a["eps"], a["min_samples"], iptr(a["order"]), moving,
                                          dptr(a["states_log"]), dptr(a["u_log"]), iptr(a["index_log"]), a["info_log"], iptr(a["arrived_at"]),
                                          iptr(a["nbox_log"]), dptr(out["clearance"]))
        out["info"] = [info_tuple(i) for i in out["info"]]
        return rc, out

    def host_tick(self, st, cur, first, geom=None):
        """one host-driven tick: (the world uploaded at `geom`,) rda_fleet_raycast, rda_fleet_upload_scans of those ranges at that state,
        rda_fleet_step_tracked -> controls, states, infos, min_index, end_heading, box counts"""
        B, hip = self.B, self.hip
        st, cur = np.ascontiguousarray(st, float), np.ascontiguousarray(cur, np.int32)
        if geom is not None:
            self.upload_world(geom)
        nb, lo, hi, rmin, rmax = self.sensors
        ranges, boxes = np.zeros(int(nb.sum()) + 1), np.full(B, -7, np.int32)
        assert hip.fleet_raycast(self.F, iptr(nb), dptr(lo), dptr(hi), dptr(rmin), dptr(rmax), dptr(st), dptr(ranges)) == 0
        assert hip.fleet_upload_scans(self.F, iptr(nb), dptr(ranges), dptr(lo), dptr(hi), dptr(rmax), dptr(st), EPS, MIN_SAMPLES, iptr(self.order),
                                      iptr(boxes)) == 0
        return (*self.step_tracked(st, cur, first), boxes)

    def forced(self, logs, n, base, t_of, cur0, first):
        """n host-driven ticks fed with the logged states and indices of a rollout and the world of every tick, advanced in numpy"""
        return [self.host_tick(logs["states"][k], cur0 if k == 0 else logs["index"][k - 1], first and k == 0,
                               geom=advanced(self.kind, self.nvert, base, self.vel, t_of(k))[0]) for k in range(n)]


@pytest.fixture(scope="module", params=[1, 0], ids=["moving", "standing"])
def run(hip, request):
    """ONE rollout of K ticks, a second one of K2, a host-driven tick behind them - and the teacher-forced twin of all of it, shared by the tests below"""
    moving = request.param
    t_of = (lambda k: DT * k) if moving else (lambda k: 0.0)
    a, b = Twin(hip), Twin(hip)
    out = dict(moving=moving, kind=a.kind, nvert=a.nvert, base=a.base, vel=a.vel)
    rc, logs = a.rollout(K, moving)
    assert rc == 0, rc
    out.update(logs=logs, world1=a.world(), slots_a=a.slots())
    rc, logs2 = a.rollout(K2, moving, states=np.ascontiguousarray(logs["states"][K]), cur_index=np.ascontiguousarray(logs["index"][K - 1]), nom_u=None)
    assert rc == 0, rc
    out.update(logs2=logs2, world2=a.world())
    out["cont_a"] = a.host_tick(logs2["states"][K2], logs2["index"][K2 - 1], False)
    out["ticks"] = b.forced(logs, K, b.base, t_of, b.cur0, True)
    out["slots_b"] = b.slots()
    base2 = advanced(b.kind, b.nvert, b.base, b.vel, t_of(K))[0]
    out["ticks2"] = b.forced(logs2, K2, base2, t_of, logs["index"][K - 1], False)
    out["cont_b"] = b.host_tick(logs2["states"][K2], logs2["index"][K2 - 1], False, geom=advanced(b.kind, b.nvert, base2, b.vel, t_of(K2))[0])
    a.close(); b.close()
    return out


def test_world_moves_by_the_rule_or_stands(run):
    """after K ticks the resident world is base + vel * (dt * K) on every polygon vertex and circle centre, for equality (moving), or untouched; a second
    rollout takes what it finds as its base"""
    kind, nvert, base, vel = run["kind"], run["nvert"], run["base"], run["vel"]
    if not run["moving"]:
        assert np.array_equal(run["world1"], base) and np.array_equal(run["world2"], base)
        return
    want1, mask = advanced(kind, nvert, base, vel, DT * K)
    assert np.array_equal(run["world1"], want1) and np.array_equal(run["world1"][~mask], base[~mask])
    assert np.abs(want1 - base).max() > 0.5
    want2, _ = advanced(kind, nvert, want1, vel, DT * K2)
    assert np.array_equal(run["world2"], want2)
    assert np.array_equal(run["world2"][2 * NOBS:], base[2 * NOBS:])                          # member 2's world stands


def test_teacher_forced_twin_bit_for_bit(run):
    """every tick of both rollouts against rda_fleet_raycast + rda_fleet_upload_scans + rda_fleet_step_tracked from the same logged state on the same
    world: box count, first control, min_index, the whole rda_info; after the last tick of the first rollout the staged slots of every member"""
    logs = run["logs"]
    moved = compare_ticks(logs, run["ticks"], K, TICK) + compare_ticks(run["logs2"], run["ticks2"], K2, TICK)
    assert moved == 3 * (K + K2) and np.all(logs["arrived_at"] == -1)
    assert np.abs(logs["controls"][:, :, 0]).max() > 1.0 and np.all(logs["states"][K, :, 0] - logs["states"][0, :, 0] > 1.0)       # the members drive
    boxes = np.concatenate([logs["boxes"], run["logs2"]["boxes"]])
    print("boxes per tick:", boxes.T.tolist())
    assert any((boxes[:, i] == 0).any() and (boxes[:, i] > 0).any() for i in range(3))          # the zero-box rule and the launch-form flip, both ways
    assert (boxes > N).any() and ((boxes > 0) & (boxes < N)).any()                               # truncation; padding quirk Q3
    for i, (sa, sb) in enumerate(zip(run["slots_a"], run["slots_b"])):
        assert sa[3] == sb[3] == 1, i
        for x, y in zip(sa[:3], sb[:3]):
            assert np.array_equal(x, y), i


def test_host_loop_continues_after_the_rollouts(run):
    """an ordinary host tick (ray cast, upload, tracked step) from the last logged state on the world the rollouts left: what the twin's tick on the
    numpy-advanced world gives, everything it returns"""
    for x, y in zip(run["cont_a"], run["cont_b"]):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y


def test_clearance_log_is_against_the_world(run):
    """clearance_log[k][i] against scenarios.clearance(car, states[k+1], the world's obstacles, t = (k+1) dt | 0), 1e-9 m"""
    logs, worst = run["logs"], 0.0
    assert logs["clearance"].shape == (K, 3)
    for k in range(K):
        for i in range(3):
            want = sc.clearance(car(i), np.asarray(logs["states"][k + 1, i], float), lane(i)[1], t=(k + 1) * DT if run["moving"] else 0.0)
            worst = max(worst, abs(logs["clearance"][k, i] - want))
    print(f"largest |clearance_log - scenarios.clearance| = {worst:.3e}  (values {logs['clearance'].min():.3f} .. {logs['clearance'].max():.3f})")
    assert worst <= 1e-9


def test_logs_that_are_left_out_and_an_empty_world(hip):
    a, b = Twin(hip), Twin(hip)
    (rc1, l1), (rc2, l2) = a.rollout(3, 1), b.rollout(3, 1, clearance=False, nbox_log=None, info_log=None)
    assert rc1 == 0 and rc2 == 0 and l2["clearance"] is None and np.all(np.isfinite(l1["clearance"])) and np.all(l2["boxes"] == -7)
    same_logs(l1, dict(l2, info=l1["info"]), keys=("states", "controls", "index", "arrived_at"))
    assert np.array_equal(a.world(), b.world())
    # member 1 in an empty world: it sees nothing, plans without obstacles, and its clearance is +inf
    counts = a.counts.copy(); counts[1] = 0
    keep = np.r_[0:NOBS, 2 * NOBS:3 * NOBS]
    assert hip.fleet_upload_worlds(a.F, iptr(counts), WE, iptr(np.ascontiguousarray(a.kind[keep])), iptr(np.ascontiguousarray(a.nvert[keep])),
                                   dptr(np.ascontiguousarray(a.base[keep])), None) == 0
    rc, l3 = a.rollout(2, 1, states=np.ascontiguousarray(l1["states"][3]), cur_index=np.ascontiguousarray(l1["index"][2]), nom_u=None)
    assert rc == 0 and np.all(l3["boxes"][:, 1] == 0) and np.all(np.isinf(l3["clearance"][:, 1])) and np.all(np.isfinite(l3["clearance"][:, [0, 2]]))
    assert np.all(np.isfinite(l3["controls"]))
    a.close(); b.close()


def test_refusals_queue_and_change_nothing(hip):
    """every refusal returns its code and leaves the world as it was; the fleet that was refused then rolls out exactly like a twin that never was"""
    a, b = Twin(hip), Twin(hip)
    B, w0 = a.B, a.world()

    def refused(code, k=2, **over):
        assert a.rollout(k, 1, **over)[0] == code, (k, list(over))
        assert np.array_equal(a.world(), w0)
    for k in (0, -1, 4097):
        refused(RDA_ERR_ARG, k=k)
    for key in ("states", "ref_speed", "cur_index", "states_log", "u_log", "index_log", "arrived_at", "n_beams", "angle_min", "angle_max", "range_min",
                "range_max", "order"):
        refused(RDA_ERR_ARG, **{key: None})
    refused(RDA_ERR_ARG, ind_range=0)
    refused(RDA_ERR_ARG, goal_margin=0)
    refused(RDA_ERR_ARG, eps=0.0)
    refused(RDA_ERR_ARG, eps=float("nan"))
    refused(RDA_ERR_ARG, min_samples=0)
    for bad in (-1, a.plen[1]):
        cur = np.zeros(B, np.int32); cur[1] = bad
        refused(RDA_ERR_ARG, cur_index=cur)
    nb = a.sensors[0].copy(); nb[2] = -1
    refused(RDA_ERR_ARG, n_beams=nb)
    nb = a.sensors[0].copy(); nb[0] = 4097
    refused(RDA_ERR_UNSUPPORTED, n_beams=nb)
    rc, la = a.rollout(2, 1)
    assert rc == 0
    rc, lb = b.rollout(2, 1)
    assert rc == 0
    same_logs(la, lb, LOGS)
    assert np.array_equal(a.world(), b.world()) and not np.array_equal(a.world(), w0)
    a.close(); b.close()
    f = Twin(hip, world=False)                                          # no uploaded world
    assert f.rollout(2, 1)[0] == RDA_ERR_ARG
    f.close()
    f = Twin(hip, (0,), path=False)                                     # no uploaded path
    assert f.rollout(2, 1)[0] == RDA_ERR_ARG
    f.close()
    f = Twin(hip, (0,), duals_follow_obstacles=True)
    assert f.rollout(2, 1)[0] == RDA_ERR_UNSUPPORTED
    f.close()


def test_refused_allocations_change_nothing(hip):
    """the first call of a fleet makes every table and buffer it needs before tick 0: refused at each allocation it returns RDA_ERR_HIP, holds nothing more
    than before and has not touched the world; the call that gets through gives the logs of an undisturbed twin"""
    def live():
        n, by = C.c_longlong(0), C.c_longlong(0)
        assert hip.debug_alloc_stats(C.byref(n), C.byref(by)) == 0
        return n.value, by.value
    a, b = Twin(hip), Twin(hip)
    w0 = a.world()
    rc, n = RDA_ERR_HIP, 0
    while rc == RDA_ERR_HIP and n < 80:
        before = live()
        hip.debug_alloc_fail(n)
        try:
            rc, la = a.rollout(3, 1)
        finally:
            hip.debug_alloc_fail(-1)
        assert rc == 0 or (rc == RDA_ERR_HIP and live() == before and np.array_equal(a.world(), w0)), (n, rc)
        n += 1
    print("allocations of a fleet's first rda_fleet_rollout_lidar:", n - 1)
    assert rc == 0 and n - 1 > 30
    rc, lb = b.rollout(3, 1)
    assert rc == 0
    same_logs(la, lb, LOGS)
    a.close(); b.close()


def test_fleet_upload_scans_still_equals_upload_scan_per_member(hip):
    """the staging half of rda_fleet_upload_scans is now a function shared with the rollout: on a fresh fleet it still stages, per member, what
    rda_upload_scan stages on a solo handle - counts and slots bit for bit (scans of the lanes from numpy, at two poses)"""
    f = Twin(hip, world=False)
    solo = [solver(hip, e, scene=False)[0] for e in range(3)]
    nb, lo, hi, rmin, rmax = f.sensors
    for p in (0, 5):
        st = np.ascontiguousarray(np.array([[4.0 + 0.4 * p, 20.0 + 8.0 * e, 0.0] for e in range(3)]))
        scans = [np.ascontiguousarray(numpy_scan(st[e], SENSORS[e], lane(e)[1])["ranges"]) for e in range(3)]
        order = np.array([1, 0, 1], np.int32)
        got = np.full(3, -7, np.int32)
        assert hip.fleet_upload_scans(f.F, iptr(nb), dptr(np.concatenate(scans)), dptr(lo), dptr(hi), dptr(rmax), dptr(st), EPS, MIN_SAMPLES, iptr(order),
                                      iptr(got)) == 0
        assert hip.fleet_sync(f.F) == 0
        slots = f.slots()
        for e in range(3):
            n1 = np.zeros(1, np.int32)
            assert hip.upload_scan(solo[e]._be.handle, int(nb[e]), dptr(scans[e]), lo[e], hi[e], rmax[e], dptr(np.ascontiguousarray(st[e])), EPS, MIN_SAMPLES,
                                   int(order[e]), iptr(n1)) == 0
            assert n1[0] == got[e], (p, e)
            A, b, cone, nt = np.zeros((N, T + 1, E, 2)), np.zeros((N, T + 1, E)), np.zeros(N, np.int32), np.zeros(1, np.int32)
            assert hip.get_obstacles(solo[e]._be.handle, dptr(A), dptr(b), iptr(cone), iptr(nt)) == 0
            if got[e] > 0:
                m = N * int(nt[0]) * E
                assert nt[0] == slots[e][3] and np.array_equal(A.ravel()[:2 * m], slots[e][0]) and np.array_equal(b.ravel()[:m], slots[e][1])
                assert np.array_equal(cone, slots[e][2])
        assert got[1] > N and got[0] > 0
    f.close()


def test_python_rollout_lidar(hip):
    """Fleet.rollout(lidar=, world=, moving=True, clearance=True): the arrays of the C call on a twin fleet, the members mirrored on the host, and
    Fleet.control(scans=Fleet.raycast(...)) goes on from there"""
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    steps = 5

    def fleet():
        ms, obs, states = [], [], []
        for e in range(3):
            path, scene = lane(e)
            ms.append(MPC(car(e), [p.copy() for p in path], receding=T, sample_time=DT, iter_num=ITER, max_edge_num=E, max_obs_num=N, goal_index_threshold=MARGIN))
            obs.append(scene); states.append(path[0].copy())
        return Fleet(ms), obs, states
    fa, obs, states = fleet()
    fb, _, _ = fleet()
    out = fa.rollout([s.copy() for s in states], SPEED, steps, lidar=SENSORS, world=obs, moving=True, clearance=True)
    st = np.ascontiguousarray(np.array([s.ravel() for s in states]))
    for i, m in enumerate(fb.members):
        cur_ref_path, _ = m._piece(states[i])
        m._sync_path(cur_ref_path)
    fb.upload_worlds(obs)
    nb, lo, hi, rmin, rmax = sensor_c(SENSORS)
    cur = np.array([m.cur_index for m in fb.members], np.int32)
    want = dict(states=np.zeros((steps + 1, 3, 3)), controls=np.zeros((steps, 3, 2)), index=np.zeros((steps, 3), np.int32), arrived_at=np.zeros(3, np.int32),
                boxes=np.zeros((steps, 3), np.int32), clearance=np.zeros((steps, 3)))
    infos = (Info * (steps * 3))()
    order = np.ones(3, np.int32)
    assert hip.fleet_rollout_lidar(fb._handle, steps, dptr(st), dptr(np.full(3, SPEED)), iptr(cur), 0.1, 10, MARGIN, dptr(np.zeros((3, 2, T))), iptr(nb), dptr(lo),
                                   dptr(hi), dptr(rmin), dptr(rmax), 2.0, 6, iptr(order), 1, dptr(want["states"]), dptr(want["controls"]), iptr(want["index"]),
                                   infos, iptr(want["arrived_at"]), iptr(want["boxes"]), dptr(want["clearance"])) == 0
    assert out["boxes"].shape == (steps, 3) and out["clearance"].shape == (steps, 3) and out["states"].shape == (steps + 1, 3, 3)
    for key in want:
        assert np.array_equal(out[key], want[key]), key
    assert np.array_equal(out["iters"], np.array([i.iters for i in infos]).reshape(steps, 3))
    assert np.abs(out["controls"][:, :, 0]).min() > 0.1 and np.all(out["arrived_at"] == -1)
    for i, m in enumerate(fa.members):                                   # the members mirror the last tick
        assert np.array_equal(m.state.ravel(), out["states"][-1, i]) and m.cur_index == out["index"][-1, i]
    last = [out["states"][-1, i].reshape(3, 1) for i in range(3)]
    res = fa.control(last, SPEED, scans=fa.raycast(last, SENSORS))      # the world stands where tick `steps` finds it
    for u, info in res:
        assert u.shape == (2, 1) and np.isfinite(u).all() and info["iters"] >= 1 and not info["arrive"]
    fa.close(); fb.close()
