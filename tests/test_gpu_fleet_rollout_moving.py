"""-m gpu : the fleet rollout for scenes that move (rda_fleet_rollout_moving: scene::k_move_fleet, rollout::k_clearance_fleet; rda_fleet_clearance,
Fleet.rollout(moving=True)) against the host-driven loop it replaces - per tick the obstacles put forward on the host, rda_fleet_upload_scenes,
rda_fleet_step_tracked (tools/closed_loop_host.c closed_loop_fleet_run_moving).  The obstacle motion is compared with numpy's base + vel * (dt * k) for
equality; a twin fleet fed the logged states and the numpy-advanced geometry must reproduce every control, path index, iteration count and the staged
slots bit for bit; the clearance log is compared with scenarios.clearance.
Shapes (those of tests/test_gpu_fleet_rollout.py): T = 8, N = 4 slots, E = 4, iter_num = 2, dt = 0.1; B = 3 (Ackermann, differential, omni) on straight
lanes; 7 obstacles per member, more than N, so the staged four change on the way; K = 12, a second rollout of 5.
  member 0: polygons, all moving at 0.3 - 0.6 m/s, some across the lane
  member 1: circles and polygons, one of them at 0.005 m/s (it moves, its motion is not predicted), one standing
  member 2: a scene that does not move (nt = 1)"""
import ctypes as C

import numpy as np
import pytest

from fleet_twin_lib import (DT, E, ITER, MARGIN, N, NOBS, RDA_ERR_ARG, RDA_ERR_HIP, RDA_ERR_UNSUPPORTED, SPEED, T, FleetTwin, advanced, car, compare_ticks,
                            info_tuple, lane, same_logs, solver)
from fleet_twin_lib import hip          # noqa: F401  (the fixture)
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import Info, dptr, iptr

pytestmark = pytest.mark.gpu

K, K2 = 12, 5


class Twin(FleetTwin):
    """a fleet of fresh handles (members `which`) with their raw scenes resident"""
    def __init__(self, hip, which=(0, 1, 2), order=1, svs=None):
        self.which = which
        made = svs if svs is not None else [solver(hip, e, order) for e in which]
        self.make_fleet(hip, [m[0] for m in made])
        self.states = np.ascontiguousarray(np.array([m[1] for m in made]))
        self.plen = [m[2] for m in made]
        self.kind, self.nvert = (np.ascontiguousarray(np.concatenate([m[3][j] for m in made])) for j in (0, 1))
        self.base, self.vel = (np.ascontiguousarray(np.concatenate([m[3][j] for m in made])) for j in (2, 3))
        self.counts = np.full(self.B, NOBS, np.int32)
        self.order = np.full(self.B, order, np.int32)

    def rollout(self, k, resort, clearance=True, **over):
        """rda_fleet_rollout_moving -> (rc, dict of logs); over: arguments replaced (None = a missing array)"""
        out = self.logs(k, clearance=float if clearance else None)
        a = dict(states=self.states, ref_speed=self.speed, cur_index=self.cur0, threshold=0.1, ind_range=10, goal_margin=MARGIN, nom_u=self.nom0,
                 states_log=out["states"], u_log=out["controls"], index_log=out["index"], info_log=out["info"], arrived_at=out["arrived_at"])
        a.update(over)
        rc = self.hip.fleet_rollout_moving(self.F, k, dptr(a["states"]), dptr(a["ref_speed"]), iptr(a["cur_index"]), a["threshold"], a["ind_range"],
                                           a["goal_margin"], resort, dptr(a["nom_u"]), dptr(a["states_log"]), dptr(a["u_log"]), iptr(a["index_log"]),
                                           a["info_log"], iptr(a["arrived_at"]), dptr(out["clearance"]))
        out["info"] = [info_tuple(i) for i in out["info"]]
        return rc, out

    def geometry(self):
        """rda_debug_scene_geom of every member, concatenated like `base`"""
        out = []
        for s in self.svs:
            g, n = np.full((NOBS, E, 2), np.nan), np.zeros(1, np.int32)
            assert self.hip.debug_scene_geom(s._be.handle, dptr(g), iptr(n)) == 0 and n[0] == NOBS
            out.append(g)
        return np.concatenate(out)

    def host_tick(self, st, cur, first, geom=None, order=None, resort=False):
        """one host-driven tick: (the scenes uploaded at `geom` | re-sorted,) rda_fleet_step_tracked -> controls, states, infos, min_index, end_heading"""
        B, hip = self.B, self.hip
        st, cur = np.ascontiguousarray(st, float), np.ascontiguousarray(cur, np.int32)
        if geom is not None:
            rob = np.ascontiguousarray(st[:, 0:2])
            order = self.order if order is None else np.full(B, order, np.int32)
            assert hip.fleet_upload_scenes(self.F, iptr(self.counts), iptr(self.kind), iptr(self.nvert), dptr(np.ascontiguousarray(geom)), dptr(self.vel),
                                           dptr(rob), iptr(order)) == 0
        if resort:
            assert hip.fleet_scene_resort(self.F, dptr(st), 3) == 0
        return self.step_tracked(st, cur, first)

    def forced(self, logs, n, base, cur0, first):
        """n host-driven ticks fed with the logged states and indices of a rollout and the numpy-advanced geometry"""
        return [self.host_tick(logs["states"][k], cur0 if k == 0 else logs["index"][k - 1], first and k == 0,
                               geom=advanced(self.kind, self.nvert, base, self.vel, DT * k)[0]) for k in range(n)]


LOGS = ("states", "controls", "index", "arrived_at", "clearance")


@pytest.fixture(scope="module", params=[1, 0], ids=["resort", "staged-order"])
def run(hip, request):
    """ONE rollout of K ticks, a second one of K2, a host-driven tick behind them - and the teacher-forced twin of all of it, shared by the tests below"""
    resort = request.param
    a, b = Twin(hip, order=resort), Twin(hip, order=resort)
    out = dict(resort=resort, kind=a.kind, nvert=a.nvert, base=a.base, vel=a.vel, staged0=a.staged(0))
    rc, logs = a.rollout(K, resort)
    assert rc == 0, rc
    out.update(logs=logs, geom1=a.geometry(), slots_a=a.slots(), staged1=a.staged(0))
    rc, logs2 = a.rollout(K2, resort, states=np.ascontiguousarray(logs["states"][K]), cur_index=np.ascontiguousarray(logs["index"][K - 1]), nom_u=None)
    assert rc == 0, rc
    out.update(logs2=logs2, geom2=a.geometry(), staged2=a.staged(0))
    out["cont_a"] = a.host_tick(logs2["states"][K2], logs2["index"][K2 - 1], False, resort=True)
    out["ticks"] = b.forced(logs, K, b.base, b.cur0, True)
    out["slots_b"] = b.slots()
    base2 = advanced(b.kind, b.nvert, b.base, b.vel, DT * K)[0]
    out["ticks2"] = b.forced(logs2, K2, base2, logs["index"][K - 1], False)
    out["cont_b"] = b.host_tick(logs2["states"][K2], logs2["index"][K2 - 1], False, geom=advanced(b.kind, b.nvert, base2, b.vel, DT * K2)[0], order=1)
    a.close(); b.close()
    return out


def test_obstacles_move_by_the_rule(run):
    """after K ticks the resident geometry is base + vel * (dt * K) on every polygon vertex and circle centre, for equality; radius and padding entries are
    base's; a second rollout takes that geometry as its base"""
    kind, nvert, base, vel = run["kind"], run["nvert"], run["base"], run["vel"]
    want1, mask = advanced(kind, nvert, base, vel, DT * K)
    assert np.array_equal(run["geom1"], want1)
    assert np.array_equal(run["geom1"][~mask], base[~mask])
    assert np.abs(want1 - base).max() > 0.5 and np.any(want1[7 + 1] != base[7 + 1])       # things move - the 0.005 m/s obstacle of member 1 too
    want2, _ = advanced(kind, nvert, want1, vel, DT * K2)
    assert np.array_equal(run["geom2"], want2)
    assert np.array_equal(run["geom2"][2 * NOBS:], base[2 * NOBS:])                        # member 2 stands


def test_teacher_forced_twin_bit_for_bit(run):
    """every tick of both rollouts against rda_fleet_upload_scenes (numpy-advanced geometry, the logged position) + rda_fleet_step_tracked from the same
    logged state: first control, min_index, executed ADMM iterations; after the last tick of the first rollout the staged slots of every member"""
    logs = run["logs"]
    moved = compare_ticks(logs, run["ticks"], K) + compare_ticks(run["logs2"], run["ticks2"], K2)
    assert moved == 3 * (K + K2) and np.all(logs["arrived_at"] == -1)
    assert np.abs(logs["controls"][:, :, 0]).max() > 1.0 and np.all(logs["states"][K, :, 0] - logs["states"][0, :, 0] > 1.0)       # the members drive
    for i, (sa, sb) in enumerate(zip(run["slots_a"], run["slots_b"])):
        assert sa[3] == sb[3] == (1 if i == 2 else T + 1), i
        for x, y in zip(sa[:3], sb[:3]):
            assert np.array_equal(x, y), i
    if run["resort"]:
        print("member 0 staged", run["staged0"], "->", run["staged1"], "->", run["staged2"], " x =", logs["states"][K, 0, 0], run["logs2"]["states"][K2, 0, 0])
        assert run["staged0"] != run["staged2"]                                             # the nearest four changed on the way
    else:
        assert run["staged1"] == run["staged2"] == [0, 1, 2, 3]


def test_host_loop_continues_after_the_rollouts(run):
    """rda_fleet_scene_resort + rda_fleet_step_tracked from the last logged state on the geometry the rollouts left: what the twin's upload of that tick's
    geometry + step give, everything they return"""
    for x, y in zip(run["cont_a"], run["cont_b"]):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y


def reference_clearance(e, state, t):
    return sc.clearance(car(e), np.asarray(state, float), lane(e)[1], t=t)


def test_clearance_log(run):
    """clearance_log[k][i] against scenarios.clearance(car, states[k+1], obstacles, t = (k+1) dt).  Bound 1e-9 m, the project's bound for device geometry
    against its numpy specification: the two sides differ in the rounding of sin / cos, a 2 x 2 solve and a handful of products at <= 100 m"""
    logs, worst = run["logs"], 0.0
    assert logs["clearance"].shape == (K, 3)
    for k in range(K):
        for i in range(3):
            want = reference_clearance(i, logs["states"][k + 1, i], (k + 1) * DT)
            worst = max(worst, abs(logs["clearance"][k, i] - want))
    print(f"largest |clearance_log - scenarios.clearance| = {worst:.3e}  (values {logs['clearance'].min():.3f} .. {logs['clearance'].max():.3f})")
    assert worst <= 1e-9


def test_clearance_at_given_poses(hip):
    """rda_fleet_clearance at 20 seeded poses per member - on top of obstacles of both kinds (negative), about the lane, far away - against
    scenarios.clearance on the staged scene, 1e-9 m; no solver involved"""
    a = Twin(hip)
    rng = np.random.default_rng(sc.SEED)
    worst, lo, neg = 0.0, np.inf, set()
    for p in range(20):
        st = np.zeros((3, 3))
        for i in range(3):
            obs = lane(i)[1]
            if p < 8:                                     # on an obstacle: its centre under the robot's side
                o = obs[p % NOBS]
                c = o.center.ravel() if o.cone_type == "norm2" else o.vertex.mean(axis=1)
                th = rng.uniform(-np.pi, np.pi)
                off = np.array([-np.sin(th), np.cos(th)]) * 0.8
                st[i] = [c[0] - off[0] - 0.3 * np.cos(th), c[1] - off[1] - 0.3 * np.sin(th), th]
            elif p < 12:                                  # far from all of them
                st[i] = [rng.uniform(60, 90), rng.uniform(-40, 90), rng.uniform(-np.pi, np.pi)]
            else:
                st[i] = [rng.uniform(0, 22), 20.0 + 8.0 * i + rng.uniform(-3, 3), rng.uniform(-np.pi, np.pi)]
        got = np.full(3, np.nan)
        assert hip.fleet_clearance(a.F, dptr(st), dptr(got)) == 0
        for i in range(3):
            want = reference_clearance(i, st[i], 0.0)
            worst, lo = max(worst, abs(got[i] - want)), min(lo, want)
            if want < 0 and p < 8:
                neg.add(lane(i)[1][p % NOBS].cone_type)
    print(f"largest |rda_fleet_clearance - scenarios.clearance| = {worst:.3e}; smallest clearance {lo:.3f}; overlapped kinds {sorted(neg)}")
    assert worst <= 1e-9
    assert neg == {"norm2", "Rpositive"} and lo < -0.3
    a.close()


def test_without_a_clearance_log_the_other_logs_are_the_same(hip):
    a, b = Twin(hip), Twin(hip)
    (rc1, l1), (rc2, l2) = a.rollout(3, 1, clearance=True), b.rollout(3, 1, clearance=False)
    assert rc1 == 0 and rc2 == 0 and l2["clearance"] is None and np.all(np.isfinite(l1["clearance"]))
    same_logs(l1, l2, keys=("states", "controls", "index", "arrived_at"))
    assert np.array_equal(a.geometry(), b.geometry())
    a.close(); b.close()


def test_refusals_queue_and_change_nothing(hip):
    """every refusal returns its code and leaves the resident geometry as it was; the fleet that was refused then rolls out exactly like a twin that never was"""
    a, b = Twin(hip), Twin(hip)
    B, g0 = a.B, a.geometry()

    def refused(code, k=2, resort=1, **over):
        assert a.rollout(k, resort, **over)[0] == code, (k, resort, list(over))
        assert np.array_equal(a.geometry(), g0)
    for k in (0, -1, 4097):
        refused(RDA_ERR_ARG, k=k)
    for key in ("states", "ref_speed", "cur_index", "states_log", "u_log", "index_log", "arrived_at"):
        refused(RDA_ERR_ARG, **{key: None})
    refused(RDA_ERR_ARG, ind_range=0)
    refused(RDA_ERR_ARG, goal_margin=0)
    for bad in (-1, a.plen[1]):
        cur = np.zeros(B, np.int32); cur[1] = bad
        refused(RDA_ERR_ARG, cur_index=cur)
    refused(RDA_ERR_ARG, resort=0)                                  # staged with order = 1: the staged order cannot be rebuilt without re-sorting
    rc, la = a.rollout(2, 1, info_log=None)                         # (info_log may be missing)
    assert rc == 0
    rc, lb = b.rollout(2, 1)
    assert rc == 0
    lb["info"] = la["info"]
    same_logs(la, lb, LOGS)
    assert np.array_equal(a.geometry(), b.geometry()) and not np.array_equal(a.geometry(), g0)
    a.close(); b.close()

    # members that cannot be rolled out (fleets of their own)
    def alone(code, resort, clearance=True, then=None, **kw):
        f = Twin(hip, (0,), svs=[solver(hip, 0, **kw)])
        if then is not None:
            then(f)
        g = f.geometry() if kw.get("scene", True) and then is None else None
        assert f.rollout(2, resort, clearance=clearance)[0] == code, kw
        if g is not None:
            assert np.array_equal(f.geometry(), g)
        return f
    alone(RDA_ERR_ARG, 0, order=0, path=False).close()             # no uploaded path
    alone(RDA_ERR_ARG, 1, scene=False).close()                     # re-sort without a resident raw scene
    alone(RDA_ERR_ARG, 1, then=lambda f: hip.upload_scene(f.svs[0]._be.handle, 0, None, None, None, None, None, 1, None)).close()      # ... with no staged obstacle
    alone(RDA_ERR_UNSUPPORTED, 1, duals_follow_obstacles=True).close()
    # a circle (norm2) robot cannot be asked for a clearance log: such a member is not taken into a fleet in the first place (its LamMuZ problems need the
    # interior-point mode, which the fused fleet launches do not run), so the library's own RDA_ERR_UNSUPPORTED for it stands behind this refusal
    sv = solver(hip, 0, robot=sc.circle_robot(0.8, dynamics="diff"))[0]
    F = C.c_void_p()
    assert hip.fleet_create((C.c_void_p * 1)(sv._be.handle), 1, C.byref(F)) == RDA_ERR_UNSUPPORTED


def test_refused_allocations_change_nothing(hip):
    """the first call of a fleet makes every table it needs: refused at each allocation it returns RDA_ERR_HIP, holds nothing more than before and has not
    touched the geometry; the call that gets through gives the logs of an undisturbed twin"""
    def live():
        n, by = C.c_longlong(0), C.c_longlong(0)
        assert hip.debug_alloc_stats(C.byref(n), C.byref(by)) == 0
        return n.value, by.value
    a, b = Twin(hip), Twin(hip)
    g0 = a.geometry()
    rc, n = RDA_ERR_HIP, 0
    while rc == RDA_ERR_HIP and n < 60:
        before = live()
        hip.debug_alloc_fail(n)
        try:
            rc, la = a.rollout(3, 1)
        finally:
            hip.debug_alloc_fail(-1)
        assert rc == 0 or (rc == RDA_ERR_HIP and live() == before and np.array_equal(a.geometry(), g0)), (n, rc)
        n += 1
    print("allocations of a fleet's first rda_fleet_rollout_moving:", n - 1)
    assert rc == 0 and n - 1 > 20
    rc, lb = b.rollout(3, 1)
    assert rc == 0
    same_logs(la, lb, LOGS)
    a.close(); b.close()


def test_python_rollout_moving(hip):
    """Fleet.rollout(obstacle_lists=, moving=True, clearance=True) after a tick of Fleet.control: the arrays of the C call on a twin fleet, the caller's
    obstacle objects untouched, and Fleet.control goes on with the obstacles advanced by steps * dt"""
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    steps = 5

    def at(obs, t):
        return [[sc.Obstacle(None if o.center is None else o.center + o.velocity * t, o.radius, None if o.vertex is None else o.vertex + o.velocity * t,
                             o.cone_type, o.velocity.copy()) for o in ol] for ol in obs]

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
    obs1 = at(obs, DT)
    keep = [[(None if o.center is None else o.center.copy(), None if o.vertex is None else o.vertex.copy()) for o in ol] for ol in obs1]
    out = fa.rollout([s.copy() for s in states], SPEED, steps, obstacle_lists=obs1, moving=True, clearance=True)
    for ol, kl in zip(obs1, keep):
        for o, (c, v) in zip(ol, kl):
            assert (c is None or np.array_equal(o.center, c)) and (v is None or np.array_equal(o.vertex, v))
    st = np.ascontiguousarray(np.array([s.ravel() for s in states]))
    for i, m in enumerate(fb.members):
        m.state = states[i].copy()
    assert fb._stage_all(obs1, st)
    cur = np.array([m.cur_index for m in fb.members], np.int32)
    want = dict(states=np.zeros((steps + 1, 3, 3)), controls=np.zeros((steps, 3, 2)), index=np.zeros((steps, 3), np.int32), arrived_at=np.zeros(3, np.int32),
                clearance=np.zeros((steps, 3)))
    infos = (Info * (steps * 3))()
    assert hip.fleet_rollout_moving(fb._handle, steps, dptr(st), dptr(np.full(3, SPEED)), iptr(cur), 0.1, 10, MARGIN, 1, None, dptr(want["states"]),
                                    dptr(want["controls"]), iptr(want["index"]), infos, iptr(want["arrived_at"]), dptr(want["clearance"])) == 0
    assert out["clearance"].shape == (steps, 3) and out["states"].shape == (steps + 1, 3, 3)
    for key in want:
        assert np.array_equal(out[key], want[key]), key
    assert np.array_equal(out["iters"], np.array([i.iters for i in infos]).reshape(steps, 3))
    assert np.abs(out["controls"][:, :, 0]).min() > 0.1 and np.all(out["arrived_at"] == -1)
    assert np.array_equal(fa.clearance([out["states"][-1, i] for i in range(3)]), out["clearance"][-1])       # the same kernel on the geometry the rollout left
    res = fa.control([out["states"][-1, i].reshape(3, 1) for i in range(3)], SPEED, at(obs1, steps * DT))
    for u, info in res:
        assert u.shape == (2, 1) and np.isfinite(u).all() and info["iters"] >= 1 and not info["arrive"]
    with pytest.raises(RuntimeError):
        fa.rollout([out["states"][-1, i].reshape(3, 1) for i in range(3)], SPEED, 2)       # without moving=True a scene that moves is refused as before
    fa.close(); fb.close()
