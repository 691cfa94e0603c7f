"""-m gpu : the fleet rollout (rda_fleet_rollout, rollout::k_rollout_advance, Fleet.rollout) - K closed-loop ticks queued on the device with one host wait -
against the host-driven loop it replaces (rda_fleet_scene_resort + rda_fleet_step_tracked per tick, tools/closed_loop_host.c closed_loop_fleet_run).
Given a state, a tick of the rollout runs the same kernels on the same data as a host-driven tick, so a twin fleet that is fed the rollout's logged states
("teacher forced") must reproduce every control, path index and iteration count bit for bit; the kinematic step between two logged states is checked
against the C expressions of the host loop; arrival, refusals, continuation and the Python surface complete the contract.
Shapes: T = 8, N = 4 slots, E = 4, iter_num = 2; 7 static polygons along each path (the nearest four change on the way); B = 3 (Ackermann, differential,
omni) on straight paths, the differential member's short enough to arrive mid-run; K = 30."""
import ctypes as C

import numpy as np
import pytest

import fleet_twin_lib as L
from fleet_twin_lib import DT, DYN, E, ITER, MARGIN, N, RDA_ERR_ARG, RDA_ERR_HIP, RDA_ERR_UNSUPPORTED, SPEED, T, FleetTwin, car, compare_ticks, info_tuple, same_logs
from fleet_twin_lib import hip          # noqa: F401  (the fixture)
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import Info, dptr, iptr

pytestmark = pytest.mark.gpu

K = 30
LENGTH = (30.0, 4.0, 30.0)             # metres of path: member 1 arrives during the run
LOGS = ("states", "controls", "index", "arrived_at")


def lane(e):
    y = 20.0 + 8.0 * e
    path = sc.line_path([4, y, 0], [4 + LENGTH[e], y, 0], 0.1)
    scene = [sc.regular_polygon(7.0 + 2.5 * j, y + (2.6 if j % 2 else -2.6), 3 + j % 2, 0.8, 0.3 * j) for j in range(7)]
    return path, scene


def moving_lane(e):
    pts, _ = lane(e)
    y = np.ascontiguousarray(pts[0], float).ravel()[1]
    return pts, [sc.regular_polygon(7.0 + 2.5 * j, y + 2.6, 4, 0.8, 0.0, velocity=(0.5, 0.0)) for j in range(7)]


def solver(hip, e, path=True, scene=True, moving=False, **kw):
    """a fresh handle of member e: its path uploaded, its raw scene resident (sorted about the start)"""
    return L.solver(hip, e, path=path, scene=scene, lane=moving_lane if moving else lane, **kw)[:3]


class Twin(FleetTwin):
    """a fleet of fresh handles (members `which`) with their raw scenes resident"""
    def __init__(self, hip, which=(0, 1, 2), svs=None):
        made = svs if svs is not None else [solver(hip, e) for e in which]
        self.make_fleet(hip, [m[0] for m in made])
        self.states = np.ascontiguousarray(np.array([m[1] for m in made]))
        self.plen = [m[2] for m in made]

    def rollout(self, k, resort, cur=None, nom_u="first", **over):
        """rda_fleet_rollout -> (rc, dict of logs); over: arguments replaced (None = a missing array)"""
        out = self.logs(k)
        a = dict(states=self.states, ref_speed=self.speed, cur_index=self.cur0 if cur is None else cur, threshold=0.1,
                 ind_range=10, goal_margin=MARGIN, nom_u=self.nom0 if isinstance(nom_u, str) else nom_u, states_log=out["states"],
                 u_log=out["controls"], index_log=out["index"], info_log=out["info"], arrived_at=out["arrived_at"])
        a.update(over)
        rc = self.hip.fleet_rollout(self.F, k, dptr(a["states"]), dptr(a["ref_speed"]), iptr(a["cur_index"]), a["threshold"], a["ind_range"],
                                    a["goal_margin"], resort, dptr(a["nom_u"]), dptr(a["states_log"]), dptr(a["u_log"]), iptr(a["index_log"]),
                                    a["info_log"], iptr(a["arrived_at"]))
        out["info"] = [info_tuple(i) for i in out["info"]]
        return rc, out

    def host_tick(self, st, cur, resort, first):
        """one host-driven tick: (re-sort,) rda_fleet_step_tracked -> controls, states, infos, min_index, end_heading"""
        st = np.ascontiguousarray(st, float)
        if resort:
            assert self.hip.fleet_scene_resort(self.F, dptr(st), 3) == 0
        return self.step_tracked(st, cur, first)

    def forced(self, logs, n, resort):
        """n host-driven ticks fed with the logged states and indices of a rollout"""
        return [self.host_tick(logs["states"][k], self.cur0 if k == 0 else logs["index"][k - 1], resort, k == 0) for k in range(n)]


@pytest.fixture(scope="module", params=[1, 0], ids=["resort", "no-resort"])
def run(hip, request):
    """ONE rollout of K ticks and its teacher-forced twin, shared by the tests below"""
    resort = request.param
    a, b = Twin(hip), Twin(hip)
    rc, logs = a.rollout(K, resort)
    assert rc == 0, rc
    ticks = b.forced(logs, K, resort)
    a.close(); b.close()
    return dict(resort=resort, logs=logs, ticks=ticks, plen=a.plen)


def test_teacher_forced_twin_bit_for_bit(run):
    """every tick of the rollout against the host-driven tick from the same logged state: first control (before the arrival: afterwards the applied control
    is zero), min_index and the executed ADMM iterations - the same kernels on the same inputs, so equality and nothing else"""
    logs = run["logs"]
    moved = compare_ticks(logs, run["ticks"], K)
    assert moved > 2 * K and np.abs(logs["controls"][:, 0, 0]).max() > 1.0        # the members drive
    if run["resort"]:
        assert logs["index"][-1, 0] > 60                                          # ... far enough for the nearest four polygons to change


def test_kinematics_follow_the_host_loop(run):
    """states_log[k+1] against the expressions of tools/closed_loop_host.c:134-136 evaluated in numpy on states_log[k], u_log[k].  Bound 1e-13: the device's
    sin / cos / tan are within a few ulp of libm's, dt |v| <= 1 here, every other operation is the same separately rounded double operation, so the true
    difference is of the order of 1e-15"""
    S, U = run["logs"]["states"], run["logs"]["controls"]
    worst = 0.0
    for i in range(S.shape[1]):
        wb = car(i).wheelbase
        for k in range(K):
            x, y, th = S[k, i]
            v, w = U[k, i]
            if DYN[i] == "acker":
                want = (x + DT * (v * np.cos(th)), y + DT * (v * np.sin(th)), th + DT * (v * np.tan(w) / wb))
            elif DYN[i] == "diff":
                want = (x + DT * (v * np.cos(th)), y + DT * (v * np.sin(th)), th + DT * w)
            else:
                want = (x + DT * (v * np.cos(w)), y + DT * (v * np.sin(w)), th)
            worst = max(worst, float(np.abs(S[k + 1, i] - np.array(want)).max()))
    print(f"max |state - host expression| = {worst:.3e}")
    assert worst <= 1e-13
    assert np.abs(DT * U[:, :, 0]).max() <= 1.0


def test_arrival(run):
    """the short-path member arrives on the first tick with min_index >= L - goal_margin: zero applied control from that tick on, standing state; the
    others do not arrive"""
    logs = run["logs"]
    arrived, idx = logs["arrived_at"], logs["index"]
    L = run["plen"][1]
    hit = np.nonzero(idx[:, 1] >= L - MARGIN)[0]
    print("arrived_at", arrived, "index of member 1", idx[:, 1])
    assert hit.size and arrived[1] == hit[0] and 3 < arrived[1] < K - 3
    k = int(arrived[1])
    assert np.all(logs["controls"][k:, 1] == 0.0) and np.abs(logs["controls"][:k, 1, 0]).min() > 0
    assert np.all(logs["states"][k:, 1] == logs["states"][k, 1])
    assert arrived[0] == -1 and arrived[2] == -1
    assert np.all(idx[:, 0] < run["plen"][0] - MARGIN) and np.all(idx[:, 2] < run["plen"][2] - MARGIN)


@pytest.mark.parametrize("which", [(0, 1, 2), (1,)], ids=["B3", "B1"])
def test_one_tick_equals_resort_and_step(hip, which):
    """K = 1 on one fleet, rda_fleet_scene_resort + rda_fleet_step_tracked on its twin: control, min_index and the whole rda_info"""
    a, b = Twin(hip, which), Twin(hip, which)
    rc, logs = a.rollout(1, 1)
    assert rc == 0, rc
    u, s, info, mi, eh = b.host_tick(b.states, b.cur0, 1, True)
    assert np.array_equal(logs["states"][0], a.states)
    assert np.array_equal(logs["controls"][0], np.stack([u[:, 0, 0], u[:, 1, 0]], axis=1))
    assert np.array_equal(logs["index"][0], mi) and logs["info"] == info
    assert np.all(logs["arrived_at"] == -1)
    last_u, last_eh = np.zeros((a.B, 2, T)), np.zeros(a.B)
    assert hip.fleet_rollout_last(a.F, dptr(last_u), dptr(last_eh)) == 0
    assert np.array_equal(last_u, u) and np.array_equal(last_eh, eh)
    a.close(); b.close()


@pytest.mark.parametrize("which", [(0, 1, 2), (2,)], ids=["B3", "B1"])
def test_host_loop_continues_after_a_rollout(hip, which):
    """10 ticks rolled out, then an ordinary host-driven tick from states_log[10]: what the twin's 11th host-driven tick gives, everything it returns"""
    a, b = Twin(hip, which), Twin(hip, which)
    rc, logs = a.rollout(10, 1)
    assert rc == 0, rc
    b.forced(logs, 10, 1)
    got = a.host_tick(logs["states"][10], logs["index"][9], 1, False)
    want = b.host_tick(logs["states"][10], logs["index"][9], 1, False)
    for x, y in zip(got, want):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    a.close(); b.close()


def test_refusals_queue_and_change_nothing(hip):
    """every refusal returns its code; the fleet that was refused then rolls out exactly like a twin that never was"""
    a, b = Twin(hip), Twin(hip)
    B = a.B
    for k in (0, -1, 4097):
        assert a.rollout(k, 1)[0] == RDA_ERR_ARG, k
    for key in ("states", "ref_speed", "cur_index", "states_log", "u_log", "index_log", "arrived_at"):
        assert a.rollout(2, 1, **{key: None})[0] == RDA_ERR_ARG, key
    assert a.rollout(2, 1, ind_range=0)[0] == RDA_ERR_ARG and a.rollout(2, 1, goal_margin=0)[0] == RDA_ERR_ARG
    for bad in (-1, a.plen[1]):
        cur = np.zeros(B, np.int32); cur[1] = bad
        assert a.rollout(2, 1, cur=cur)[0] == RDA_ERR_ARG, bad
    rc, la = a.rollout(2, 1, info_log=None)                        # (info_log may be missing)
    assert rc == 0
    rc, lb = b.rollout(2, 1)
    assert rc == 0
    lb["info"] = la["info"]
    same_logs(la, lb, LOGS)
    a.close(); b.close()
    # members that cannot be rolled out (fleets of their own)
    def refused(code, resort, then=None, **kw):
        f = Twin(hip, (0,), svs=[solver(hip, 0, **kw)])
        if then is not None:
            then(f)
        assert f.rollout(2, resort)[0] == code, kw
        return f
    refused(RDA_ERR_ARG, 0, path=False).close()                    # no uploaded path
    refused(RDA_ERR_ARG, 1, scene=False).close()                   # re-sort without a resident raw scene
    refused(RDA_ERR_ARG, 1, then=lambda f: hip.upload_scene(f.svs[0]._be.handle, 0, None, None, None, None, None, 1, None)).close()      # ... with no staged obstacle
    refused(RDA_ERR_UNSUPPORTED, 1, duals_follow_obstacles=True).close()
    refused(RDA_ERR_UNSUPPORTED, 1, moving=True).close()           # per-stage slots: the scene moves
    refused(RDA_ERR_UNSUPPORTED, 0, moving=True).close()
    # a member inside rda_tracked_begin; once its tick is closed the fleet rolls out like a twin whose member took the same tick in one call
    st = np.ascontiguousarray(lane(0)[0][0], float).ravel()[0:3].copy()
    f = refused(RDA_ERR_ARG, 1, then=lambda f: hip.tracked_begin(f.svs[0]._be.handle, dptr(st), SPEED, 0, 0.1, 10, dptr(np.zeros((2, T)))))
    u, s, info, mi, eh = np.zeros((2, T)), np.zeros((3, T + 1)), Info(), C.c_int32(0), C.c_double(0)
    assert hip.tracked_finish(f.svs[0]._be.handle, dptr(u), dptr(s), C.byref(info), None, None, C.byref(mi), C.byref(eh)) >= 0
    g = Twin(hip, (0,))
    u2, s2 = np.zeros((2, T)), np.zeros((3, T + 1))
    assert hip.step_tracked(g.svs[0]._be.handle, dptr(st), SPEED, 0, 0.1, 10, dptr(np.zeros((2, T))), dptr(u2), dptr(s2), C.byref(info), None, None,
                            C.byref(mi), C.byref(eh)) >= 0
    assert np.array_equal(u, u2)
    (rc1, l1), (rc2, l2) = f.rollout(2, 1, nom_u=None), g.rollout(2, 1, nom_u=None)
    assert rc1 == 0 and rc2 == 0
    same_logs(l1, l2, LOGS)
    f.close(); g.close()


def test_refused_allocations_change_nothing(hip):
    """the first rollout of a fleet makes every table it needs (tracking, re-sort, rollout, logs): refused at each allocation it returns RDA_ERR_HIP and holds
    nothing more than before; the call that gets through gives the logs of an undisturbed twin.  A longer rollout regrows the logs under the same rule."""
    def live():
        n, by = C.c_longlong(0), C.c_longlong(0)
        assert hip.debug_alloc_stats(C.byref(n), C.byref(by)) == 0
        return n.value, by.value
    a, b = Twin(hip), Twin(hip)
    for k in (2, 4):
        rc, n = RDA_ERR_HIP, 0
        while rc == RDA_ERR_HIP and n < 40:
            before = live()
            hip.debug_alloc_fail(n)
            try:
                rc, la = a.rollout(k, 1, nom_u="first" if k == 2 else None)
            finally:
                hip.debug_alloc_fail(-1)
            assert rc == 0 or (rc == RDA_ERR_HIP and live() == before), (k, n, rc)
            n += 1
        assert rc == 0 and n - 1 == (20 if k == 2 else 2), (k, n)
        rc, lb = b.rollout(k, 1, nom_u="first" if k == 2 else None)
        assert rc == 0
        same_logs(la, lb, LOGS)
    a.close(); b.close()


def test_python_rollout(hip):
    """Fleet.rollout after a tick of Fleet.control: the arrays of the C call (a twin fleet, called through the binding), the stated shapes, the members'
    bookkeeping, and Fleet.control goes on afterwards"""
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    steps = 6

    def fleet():
        ms, obs, states = [], [], []
        for e in range(3):
            path, scene = lane(e)
            ms.append(MPC(car(e), [p.copy() for p in path], receding=T, sample_time=DT, iter_num=ITER, max_edge_num=E, max_obs_num=N, goal_index_threshold=MARGIN))
            obs.append(scene); states.append(path[0].copy())
        f = Fleet(ms)
        res = f.control([s.copy() for s in states], SPEED, [list(o) for o in obs])
        return f, obs, [sc.kinematic_step(states[i], res[i][0], car(i), DT) for i in range(3)]
    fa, obs, states = fleet()
    fb, _, _ = fleet()
    out = fa.rollout([s.copy() for s in states], SPEED, steps)
    st = np.ascontiguousarray(np.array([s.ravel() for s in states]))
    cur = np.array([m.cur_index for m in fb.members], np.int32)
    want = dict(states=np.zeros((steps + 1, 3, 3)), controls=np.zeros((steps, 3, 2)), index=np.zeros((steps, 3), np.int32), arrived_at=np.zeros(3, np.int32))
    infos = (Info * (steps * 3))()
    assert hip.fleet_rollout(fb._handle, steps, dptr(st), dptr(np.full(3, SPEED)), iptr(cur), 0.1, 10, MARGIN, 1, None, dptr(want["states"]),
                             dptr(want["controls"]), iptr(want["index"]), infos, iptr(want["arrived_at"])) == 0
    assert out["states"].shape == (steps + 1, 3, 3) and out["controls"].shape == (steps, 3, 2)
    assert out["index"].shape == (steps, 3) and out["iters"].shape == (steps, 3) and out["arrived_at"].shape == (3,)
    for key in want:
        assert np.array_equal(out[key], want[key]), key
    assert np.array_equal(out["iters"], np.array([i.iters for i in infos]).reshape(steps, 3))
    assert np.abs(out["controls"][:, :, 0]).min() > 0.1 and np.all(out["arrived_at"] == -1)
    for i, m in enumerate(fa.members):
        assert m.cur_index == out["index"][-1, i]
        assert np.array_equal(np.asarray(m.state).ravel(), out["states"][-1, i])
        assert m._nominal_u() is None and m.cur_vel_array.shape == (2, T) and m.cur_vel_array[0, 0] == out["controls"][-1, i, 0]
    res = fa.control([out["states"][-1, i].reshape(3, 1) for i in range(3)], SPEED, [list(o) for o in obs])
    for u, info in res:
        assert u.shape == (2, 1) and np.isfinite(u).all() and info["iters"] >= 1 and not info["arrive"]
    fa.close(); fb.close()
