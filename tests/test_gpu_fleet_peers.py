"""-m gpu : fleet members that avoid each other (rda_fleet_upload_scenes_peers, rda_fleet_scene_resort_peers, rda_fleet_rollout_peers,
rda_fleet_peer_clearance: scene::k_peers_fleet, rollout::k_peer_clearance_fleet; Fleet.control(peers=True), Fleet.rollout(peers=True)).
  1  the peer rows the device writes against scenarios.peer_obstacles, the own rows untouched, the row mapping
  2  a host-driven peers tick = a plain tick on the same rows (slots, controls, index, info bit for bit), also for lmz_central members; the refresh
  3  a rollout tick = a host-driven peers tick from the logged state (bit for bit), the two clearance logs, the rows the rollout leaves, a second rollout
  4  edges: a fleet of one, a member without own obstacles, R > E, a refused allocation
  5  the behaviour: three robots whose paths cross overlap when blind and keep apart with peers
Shapes (those of tests/test_gpu_fleet_rollout_moving.py): T = 8, N = 4 slots, E = 4, iter_num = 2, dt = 0.1; B = 3 (Ackermann, differential, omni; three
footprints of different size) on lanes 3 m apart, so that peers win slots; 3 own obstacles per member, one of them at 0.3 m/s."""
import ctypes as C
from math import pi

import numpy as np
import pytest

from fleet_twin_lib import DT, DYN, E, ITER, MARGIN, N, RDA_ERR_ARG, RDA_ERR_HIP, RDA_ERR_UNSUPPORTED, T, FleetTwin, advanced, compare_ticks, info_tuple, same_logs
from fleet_twin_lib import bare_fleet, refused_in_turn
from fleet_twin_lib import hip          # noqa: F401  (the fixture)
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import dptr, iptr

pytestmark = pytest.mark.gpu

K, K2 = 12, 5
NOWN = 3
SIZE = ((4.6, 1.6), (1.6, 1.0), (2.4, 1.2))             # length, width: the footprints can be told apart
SPEED = 3.0
VEL = [(0.3, 0.0), (-0.2, 0.1), (0.0, 0.0)]
TOL = 1e-9               # device geometry against its numpy specification (another maths library's sin / cos, a 2 x 2 solve, a few products at <= 100 m)


def car(e):
    return sc.rectangle_robot(length=SIZE[e][0], width=SIZE[e][1], dynamics=DYN[e], wheelbase=3.0 if DYN[e] == "acker" else 0)


def lane(e, nown=NOWN, edges=E):
    y = 20.0 + 3.0 * e
    path = sc.line_path([4, y, 0], [34, y, 0], 0.1)
    own = [sc.regular_polygon(7.0 + 3.5 * (j % 3) + 0.1 * (j // 3), y + (2.6 if j % 2 else -2.6), min(3 + j % 2, edges), 0.7, 0.3 * j, velocity=VEL[j % 3])
           for j in range(nown)]
    return path, own


class Twin(FleetTwin):
    """a fleet of fresh handles (members `which`, their paths uploaded, no scene yet) and what a caller keeps beside it"""
    def __init__(self, hip, which=(0, 1, 2), nown=None, edges=E, **kw):
        from rda_planner_amd.rda_solver import RDA_solver
        self.which, self.edges = which, edges
        nown = [NOWN] * len(which) if nown is None else nown
        svs, st, flat, self.plen = [], [], [], []
        for e, n in zip(which, nown):
            sv = RDA_solver(T, car(e), edges, N, iter_num=ITER, step_time=DT, time_print=False, **kw)
            pts, obs = lane(e, n, edges)
            P = np.ascontiguousarray(np.hstack(pts)[0:3, :].T, dtype=float)
            assert hip.upload_path(sv._be.handle, int(P.shape[0]), dptr(P)) == 0
            svs.append(sv); st.append(P[0].copy()); self.plen.append(len(pts))
            flat.append(sv.flatten_scene(list(obs)) if n else (0, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, edges, 2)), np.zeros((0, 2))))
        self.make_fleet(hip, svs, SPEED)
        self.cars = [car(e) for e in which]
        self.states = np.ascontiguousarray(np.array(st))
        self.counts = np.array(nown, np.int32)
        self.kind, self.nvert = (np.ascontiguousarray(np.concatenate([f[j] for f in flat]), np.int32) for j in (1, 2))
        self.base, self.vel = (np.ascontiguousarray(np.concatenate([f[j] for f in flat]), float) for j in (3, 4))
        self.off = np.concatenate([[0], np.cumsum(self.counts)])
        self.ctl0 = np.zeros((self.B, 2))

    def own_at(self, t, base=None):
        """the own geometry put forward by the rule of scene::k_move_fleet, base + vel * t (all own obstacles here are polygons)"""
        return advanced(self.kind, self.nvert, self.base if base is None else base, self.vel, t)[0]

    def upload_peers(self, states, controls, geom=None):
        geom = self.base if geom is None else geom
        return self.hip.fleet_upload_scenes_peers(self.F, iptr(self.counts), iptr(self.kind), iptr(self.nvert), dptr(np.ascontiguousarray(geom)), dptr(self.vel),
                                                  dptr(np.ascontiguousarray(states, float)), dptr(np.ascontiguousarray(controls, float)))

    def scene(self, i, cap=64):
        """rda_debug_scene_geom / _vel of member i -> (geom [n][E][2], vel [n][2])"""
        g, v, n, m = np.full((cap, self.edges, 2), np.nan), np.full((cap, 2), np.nan), np.zeros(1, np.int32), np.zeros(1, np.int32)
        assert self.hip.debug_scene_geom(self.svs[i]._be.handle, dptr(g), iptr(n)) == 0
        assert self.hip.debug_scene_vel(self.svs[i]._be.handle, dptr(v), iptr(m)) == 0 and n[0] == m[0]
        return g[:n[0]].copy(), v[:n[0]].copy()

    def upload_rows(self, rows, states):
        """plain rda_fleet_upload_scenes of the given per-member (geom, vel): polygons of E vertices behind the own rows' counts"""
        counts = np.array([len(g) for g, _ in rows], np.int32)
        kind = np.zeros(int(counts.sum()), np.int32)
        nvert = np.concatenate([np.concatenate([self.nvert[self.off[i]:self.off[i + 1]], np.full(len(rows[i][0]) - self.counts[i], 4, np.int32)]) for i in range(self.B)])
        geom, vel = np.ascontiguousarray(np.concatenate([g for g, _ in rows])), np.ascontiguousarray(np.concatenate([v for _, v in rows]))
        rob = np.ascontiguousarray(np.asarray(states, float)[:, 0:2])
        return self.hip.fleet_upload_scenes(self.F, iptr(counts), iptr(kind), iptr(np.ascontiguousarray(nvert, np.int32)), dptr(geom), dptr(vel), dptr(rob),
                                            iptr(np.ones(self.B, np.int32)))

    def _logs(self, k, clearance, peer):
        return self.logs(k, clearance=float if clearance else None, peer=float if peer else None)

    def rollout_peers(self, k, states=None, cur=None, nom_u="first", controls0=None, clearance=True, peer=True):
        out = self._logs(k, clearance, peer)
        states = self.states if states is None else np.ascontiguousarray(states)
        cur = self.cur0 if cur is None else np.ascontiguousarray(cur, np.int32)
        nom = self.nom0 if isinstance(nom_u, str) else nom_u
        ctl = self.ctl0 if controls0 is None else np.ascontiguousarray(controls0)
        rc = self.hip.fleet_rollout_peers(self.F, k, dptr(states), dptr(self.speed), iptr(cur), 0.1, 10, MARGIN, dptr(nom), dptr(ctl), dptr(out["states"]),
                                          dptr(out["controls"]), iptr(out["index"]), out["info"], iptr(out["arrived_at"]), dptr(out["clearance"]), dptr(out["peer"]))
        out["info"] = [info_tuple(i) for i in out["info"]]
        return rc, out

    def rollout_moving(self, k, clearance=True):
        out = self._logs(k, clearance, False)
        rc = self.hip.fleet_rollout_moving(self.F, k, dptr(self.states), dptr(self.speed), iptr(self.cur0), 0.1, 10, MARGIN, 1, dptr(self.nom0), dptr(out["states"]),
                                           dptr(out["controls"]), iptr(out["index"]), out["info"], iptr(out["arrived_at"]), dptr(out["clearance"]))
        out["info"] = [info_tuple(i) for i in out["info"]]
        return rc, out


def peer_rows(t, states, controls):
    """per member the (geom [B-1][E][2], vel [B-1][2]) scenarios.peer_obstacles asks for"""
    out = []
    for i in range(t.B):
        obs = sc.peer_obstacles(t.cars, states, controls, i)
        out.append((np.array([o.vertex.T for o in obs]).reshape(len(obs), E, 2), np.array([o.velocity.ravel() for o in obs]).reshape(len(obs), 2)))
    return out


START = np.array([[4.0, 20.0, 0.1], [5.5, 23.0, -0.2], [4.5, 26.0, 0.3]])
CTL = np.array([[1.5, 0.1], [0.8, -0.3], [1.2, 0.7]])


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_peer_rows_against_the_specification(hip):
    a = Twin(hip)
    assert a.upload_peers(START, CTL) == 0
    want = peer_rows(a, START, CTL)
    worst_g = worst_v = 0.0
    for i in range(3):
        g, v = a.scene(i)
        assert g.shape == (NOWN + 2, E, 2)
        assert np.array_equal(g[:NOWN], a.base[a.off[i]:a.off[i + 1]]) and np.array_equal(v[:NOWN], a.vel[a.off[i]:a.off[i + 1]])      # the own rows, bit for bit
        worst_g, worst_v = max(worst_g, np.abs(g[NOWN:] - want[i][0]).max()), max(worst_v, np.abs(v[NOWN:] - want[i][1]).max())
        for j in range(3):                                            # the mapping, spelled out: member j sits in row n_own + (j < i ? j : j - 1)
            if j == i:
                continue
            row = g[NOWN + (j if j < i else j - 1)]
            sides = np.linalg.norm(np.roll(row, -1, axis=0) - row, axis=1)
            assert np.allclose(sorted(sides), sorted([SIZE[j][0], SIZE[j][1]] * 2), rtol=0, atol=TOL), (i, j, sides)
            assert np.abs(row - sc.robot_vertices(a.cars[j], START[j]).T).max() <= TOL
        assert a.slots()[i][3] == T + 1
        assert any(r >= NOWN for r in a.staged(i)), (i, a.staged(i))   # a peer won a slot
    print(f"peer rows: largest |geom - spec| = {worst_g:.3e} m, |vel - spec| = {worst_v:.3e} m/s")
    assert worst_g <= TOL and worst_v <= TOL
    speed = np.linalg.norm(want[0][1], axis=1)
    assert np.all(speed > 0.5)                                        # (the velocities are not trivially zero; omni: along w, not along its heading)
    assert abs(np.arctan2(want[0][1][1, 1], want[0][1][1, 0]) - CTL[2, 1]) < 1e-12
    a.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"lmz_central": 1e-3}], ids=["enumeration", "lmz_central"])
def test_host_driven_peers_tick_equals_a_plain_tick_on_the_same_rows(hip, kw):
    a, b = Twin(hip, **kw), Twin(hip, **kw)

    def same_tick(first, states, cur):
        rows = [a.scene(i) for i in range(3)]
        assert b.upload_rows(rows, states) == 0
        for sa, sb in zip(a.slots(), b.slots()):
            assert sa[3] == sb[3] == T + 1
            for x, y in zip(sa[:3], sb[:3]):
                assert np.array_equal(x, y)
        ra, rb = a.step_tracked(states, cur, first), b.step_tracked(states, cur, first)
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        return ra
    assert a.upload_peers(START, CTL) == 0
    u, s, info, mi, eh = same_tick(True, START, a.cur0)
    assert np.abs(u[:, 0, 0]).min() > 0.05
    # the next tick through the refresh: the peer rows rewritten where the members now are, the own rows as they were
    st2 = np.array([sc.kinematic_step(START[i].reshape(3, 1), u[i, :, 0:1], a.cars[i], DT).ravel() for i in range(3)])
    ctl2 = np.ascontiguousarray(u[:, :, 0])
    assert hip.fleet_scene_resort_peers(a.F, dptr(st2), dptr(ctl2)) == 0
    hip.fleet_sync(a.F)
    want = peer_rows(a, st2, ctl2)
    for i in range(3):
        g, v = a.scene(i)
        assert np.array_equal(g[:NOWN], a.base[a.off[i]:a.off[i + 1]])
        assert np.abs(g[NOWN:] - want[i][0]).max() <= TOL and np.abs(v[NOWN:] - want[i][1]).max() <= TOL
    same_tick(False, st2, mi)
    # a plain re-sort stays legal and leaves the peer rows where they are; scenes staged otherwise end the peers state
    before = [a.scene(i) for i in range(3)]
    assert hip.fleet_scene_resort(a.F, dptr(st2), 3) == 0
    hip.fleet_sync(a.F)
    for i in range(3):
        assert all(np.array_equal(x, y) for x, y in zip(before[i], a.scene(i)))
    assert hip.fleet_scene_resort_peers(b.F, dptr(st2), dptr(ctl2)) == RDA_ERR_ARG          # b's scenes came from the plain upload
    a.close(); b.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(hip):
    """ONE peers rollout of K ticks and a second one of K2 that continues it, and the teacher-forced twin of both"""
    a, b = Twin(hip), Twin(hip)
    assert a.upload_peers(a.states, a.ctl0) == 0
    rc, logs = a.rollout_peers(K)
    assert rc == 0, rc
    out = dict(logs=logs, scenes1=[a.scene(i) for i in range(3)], cars=a.cars, base=a.base, vel=a.vel, off=a.off)
    rc, logs2 = a.rollout_peers(K2, states=logs["states"][K], cur=logs["index"][K - 1], nom_u=None, controls0=logs["controls"][K - 1])
    assert rc == 0, rc
    out.update(logs2=logs2, scenes2=[a.scene(i) for i in range(3)])

    def forced(lg, n, base, cur0, ctl0, first):
        ticks = []
        for k in range(n):
            assert b.upload_peers(lg["states"][k], ctl0 if k == 0 else lg["controls"][k - 1], geom=b.own_at(DT * k, base)) == 0
            ticks.append(b.step_tracked(lg["states"][k], cur0 if k == 0 else lg["index"][k - 1], first and k == 0))
        return ticks
    base2 = b.own_at(DT * K)                            # the second rollout's base: the geometry the first one left
    out["ticks"] = forced(logs, K, b.base, b.cur0, b.ctl0, True)
    out["ticks2"] = forced(logs2, K2, base2, logs["index"][K - 1], logs["controls"][K - 1], False)
    # the clearance against the own obstacles alone: a fleet without peer rows, rda_fleet_rollout_moving's clearance kernel at the logged states
    c = Twin(hip)
    own_clear = np.zeros((K, 3))
    for k in range(K):
        g = c.own_at(DT * (k + 1))
        assert c.upload_rows([(g[c.off[i]:c.off[i + 1]], c.vel[c.off[i]:c.off[i + 1]]) for i in range(3)], logs["states"][k + 1]) == 0
        assert hip.fleet_clearance(c.F, dptr(np.ascontiguousarray(logs["states"][k + 1])), dptr(own_clear[k])) == 0
    out.update(own_clear=own_clear, own_at=[base2, b.own_at(DT * K2, base2)])
    a.close(); b.close(); c.close()
    return out


def test_rollout_tick_equals_a_host_driven_peers_tick(run):
    """every tick of both rollouts against rda_fleet_upload_scenes_peers (the logged states, the controls of the tick before, own geometry base + vel *
    (dt * k)) + rda_fleet_step_tracked: first control, min_index, executed ADMM iterations, bit for bit"""
    logs = run["logs"]
    live = compare_ticks(logs, run["ticks"]) + compare_ticks(run["logs2"], run["ticks2"])
    assert live == 3 * (K + K2) and np.all(logs["arrived_at"] == -1)
    assert np.abs(logs["controls"][:, :, 0]).max() > 1.0 and np.all(logs["states"][K, :, 0] - logs["states"][0, :, 0] > 1.0)       # the members drive


def test_rollout_clearance_logs(run):
    """peer_clearance_log against scenarios.peer_clearance of the logged states, 1e-9 m; clearance_log = the clearance against the own obstacles alone
    (the peer rows are not counted): what the clearance kernel gives on a fleet without peer rows, for equality, and scenarios.clearance within 1e-9 m"""
    logs, cars = run["logs"], run["cars"]
    worst = max(np.abs(logs["peer"][k] - sc.peer_clearance(cars, logs["states"][k + 1])).max() for k in range(K))
    print(f"largest |peer_clearance_log - scenarios.peer_clearance| = {worst:.3e}  (values {logs['peer'].min():.3f} .. {logs['peer'].max():.3f})")
    assert worst <= TOL and np.all(np.isfinite(logs["peer"]))
    assert np.array_equal(logs["clearance"], run["own_clear"])
    worst = max(abs(logs["clearance"][k, i] - sc.clearance(cars[i], logs["states"][k + 1, i], lane(i)[1], t=(k + 1) * DT)) for k in range(K) for i in range(3))
    print(f"largest |clearance_log - scenarios.clearance(own obstacles)| = {worst:.3e}")
    assert worst <= TOL


def test_rows_a_rollout_leaves(run):
    """own rows: where tick K finds them (base + vel * (dt * K), for equality; the second rollout goes on from there); peer rows: those of tick K - 1,
    never moved"""
    for key, lg, n, own in (("scenes1", run["logs"], K, run["own_at"][0]), ("scenes2", run["logs2"], K2, run["own_at"][1])):
        last = [sc.peer_obstacles(run["cars"], lg["states"][n - 1], lg["controls"][n - 2], i) for i in range(3)]
        for i in range(3):
            g, v = run[key][i]
            assert np.array_equal(g[:NOWN], own[run["off"][i]:run["off"][i + 1]]) and np.array_equal(v[:NOWN], run["vel"][run["off"][i]:run["off"][i + 1]])
            assert max(np.abs(g[NOWN + r] - o.vertex.T).max() for r, o in enumerate(last[i])) <= TOL
            assert max(np.abs(v[NOWN + r] - o.velocity.ravel()).max() for r, o in enumerate(last[i])) <= TOL


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_a_fleet_of_one_has_no_peer_rows(hip):
    a, b = Twin(hip, (1,)), Twin(hip, (1,))
    assert a.upload_peers(a.states, a.ctl0) == 0
    assert a.scene(0)[0].shape[0] == NOWN
    rc, la = a.rollout_peers(5)
    assert rc == 0 and np.all(la["peer"] == np.inf)
    assert b.upload_rows([(b.base, b.vel)], b.states) == 0
    rc, lb = b.rollout_moving(5)
    assert rc == 0
    same_logs(la, lb, ("states", "controls", "index", "arrived_at", "clearance"))
    got = np.zeros(1)
    assert hip.fleet_peer_clearance(a.F, dptr(a.states), dptr(got)) == 0 and got[0] == np.inf
    a.close(); b.close()


def test_a_member_without_own_obstacles(hip):
    a, b = Twin(hip, nown=[NOWN, 0, NOWN]), Twin(hip, nown=[NOWN, 0, NOWN])
    assert a.upload_peers(a.states, a.ctl0) == 0 and b.upload_peers(b.states, b.ctl0) == 0
    g, v = a.scene(1)
    assert g.shape[0] == 2 and np.abs(g - peer_rows(a, a.states, a.ctl0)[1][0]).max() <= TOL and np.array_equal(v, np.zeros((2, 2)))
    rc, logs = a.rollout_peers(3)
    assert rc == 0 and np.all(logs["clearance"][:, 1] == np.inf) and np.all(np.isfinite(logs["clearance"][:, [0, 2]])) and np.all(np.isfinite(logs["peer"]))
    u, s, info, mi, eh = b.step_tracked(b.states, b.cur0, True)
    assert np.array_equal(logs["controls"][0], u[:, :, 0]) and np.array_equal(logs["index"][0], mi)
    a.close(); b.close()


def test_refusals(hip):
    a = Twin(hip, (0, 1), edges=3)                                  # rectangle robots (R = 4) and triangles: a footprint does not fit a row of E = 3
    assert a.upload_peers(a.states, a.ctl0) == RDA_ERR_UNSUPPORTED
    a.close()
    a = Twin(hip)
    assert a.rollout_peers(2)[0] == RDA_ERR_ARG                      # no peers scenes resident
    assert hip.fleet_scene_resort_peers(a.F, dptr(a.states), dptr(a.ctl0)) == RDA_ERR_ARG
    assert a.upload_peers(a.states, a.ctl0) == 0
    before = [a.scene(i) for i in range(3)]
    bad = a.counts.copy(); bad[1] = -1
    assert hip.fleet_upload_scenes_peers(a.F, iptr(bad), iptr(a.kind), iptr(a.nvert), dptr(a.base), dptr(a.vel), dptr(a.states), dptr(a.ctl0)) == RDA_ERR_ARG
    assert hip.fleet_upload_scenes_peers(a.F, iptr(a.counts), iptr(a.kind), iptr(a.nvert), dptr(a.base), None, dptr(a.states), dptr(a.ctl0)) == RDA_ERR_ARG
    assert hip.fleet_upload_scenes_peers(a.F, iptr(a.counts), iptr(a.kind), iptr(a.nvert), dptr(a.base), dptr(a.vel), dptr(a.states), None) == RDA_ERR_ARG
    assert a.rollout_peers(2, controls0=None, peer=False)[0] == 0
    lg = a._logs(2, False, False)
    assert hip.fleet_rollout_peers(a.F, 2, dptr(a.states), dptr(a.speed), iptr(a.cur0), 0.1, 10, MARGIN, None, None, dptr(lg["states"]), dptr(lg["controls"]),
                                   iptr(lg["index"]), lg["info"], iptr(lg["arrived_at"]), None, None) == RDA_ERR_ARG      # controls0 missing
    assert before[0][0].shape == a.scene(0)[0].shape
    a.close()
    f = Twin(hip, (0,), duals_follow_obstacles=True)
    assert f.upload_peers(f.states, f.ctl0) == RDA_ERR_UNSUPPORTED
    f.close()


def test_refused_allocation_leaves_the_resident_scenes(hip):
    """a peers upload that has to grow every member's scene set, refused at each of its allocations in turn: RDA_ERR_HIP, nothing more held than before,
    the members' resident scenes as they were; the call that gets through stages the larger scenes"""
    def live():
        n, by = C.c_longlong(0), C.c_longlong(0)
        assert hip.debug_alloc_stats(C.byref(n), C.byref(by)) == 0
        return n.value, by.value
    small, big = Twin(hip), Twin(hip, nown=[30, 30, 30])
    assert small.upload_peers(small.states, small.ctl0) == 0
    before = [small.scene(i) for i in range(3)]
    small.counts, small.kind, small.nvert, small.base, small.vel = big.counts, big.kind, big.nvert, big.base, big.vel      # the same fleet, larger scenes
    rc, n = RDA_ERR_HIP, 0
    while rc == RDA_ERR_HIP and n < 20:
        held = live()
        hip.debug_alloc_fail(n)
        try:
            rc = small.upload_peers(small.states, small.ctl0)
        finally:
            hip.debug_alloc_fail(-1)
        if rc == RDA_ERR_HIP:
            assert live() == held, n
            for i in range(3):
                assert all(np.array_equal(x, y) for x, y in zip(before[i], small.scene(i))), (n, i)
        n += 1
    print("allocations of a growing rda_fleet_upload_scenes_peers:", n - 1)
    assert rc == 0 and n - 1 >= 3
    assert small.scene(0)[0].shape[0] == 32 and np.array_equal(small.scene(2)[0][:30], big.base[60:90])
    small.close(); big.close()


def test_refused_allocations_of_a_first_peer_clearance_call_change_nothing(hip):
    """rda_fleet_peer_clearance on a fleet that has no peer table yet makes the table and the log: refused at each of the 8 allocations in turn it
    returns RDA_ERR_HIP and holds nothing more than before; the call that gets through returns the doubles of an undisturbed twin.  B = 3, T = 5."""
    (sa, fa), (sb, fb) = bare_fleet(hip, [car(e) for e in range(3)]), bare_fleet(hip, [car(e) for e in range(3)])
    got, want = np.full(3, np.nan), np.full(3, np.nan)
    rc, refused = refused_in_turn(hip, lambda: hip.fleet_peer_clearance(fa, dptr(START), dptr(got)))
    print("allocations of a fleet's first rda_fleet_peer_clearance:", refused)
    assert rc == 0 and refused == 8
    assert hip.fleet_peer_clearance(fb, dptr(START), dptr(want)) == 0
    assert np.array_equal(got, want) and np.all(np.isfinite(want))
    hip.fleet_destroy(fa); hip.fleet_destroy(fb)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------------------
def crossing():
    robot = sc.rectangle_robot(length=1.6, width=1.0, wheelbase=0, dynamics="diff")
    paths = [sc.line_path([4, 20, 0], [24, 20, 0], 0.1), sc.line_path([24, 20.8, pi], [4, 20.8, pi], 0.1), sc.line_path([14, 10, pi / 2], [14, 30, pi / 2], 0.1)]
    own = [[sc.regular_polygon(5 + 3 * j, 40 + 5 * e, 4, 0.5, 0.2 * j, velocity=(0.3, 0.0) if j == 0 else (0.0, 0.0)) for j in range(3)] for e in range(3)]
    return robot, paths, own


def crossing_fleet():
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    robot, paths, own = crossing()
    ms = [MPC(robot, [p.copy() for p in paths[i]], receding=T, sample_time=DT, iter_num=ITER, max_edge_num=E, max_obs_num=N, time_print=False) for i in range(3)]
    return Fleet(ms), [robot] * 3, [paths[i][0].copy() for i in range(3)], own


def test_three_crossing_robots_overlap_blind_and_keep_apart_with_peers(hip):
    """three differential robots, two head-on on lanes 0.8 m apart and one across, 2 m/s, 140 ticks.  Blind (Fleet.rollout(moving=True)) every member
    overlaps another one on the way; with peers=True the member-to-member separation stays positive - the threshold is contact itself, the CPU
    oracle's margin on this scenario is 0.63 m - and all three arrive; the Fleet.control(peers=True) loop arrives on the same ticks"""
    steps = 140
    f, cars, states, own = crossing_fleet()
    blind = f.rollout([s.copy() for s in states], 2.0, steps, obstacle_lists=own, moving=True)
    sep = np.min([f.peer_clearance(blind["states"][k]) for k in range(1, steps + 1)], axis=0)
    print("blind: minimum separation", sep, "arrived", blind["arrived_at"])
    assert np.all(sep < 0)
    assert np.abs(sep - np.min([sc.peer_clearance(cars, blind["states"][k]) for k in range(1, steps + 1)], axis=0)).max() <= TOL
    f.close()
    f, cars, states, own = crossing_fleet()
    out = f.rollout([s.copy() for s in states], 2.0, steps, obstacle_lists=own, peers=True)
    print("peers: minimum separation", out["peer_clearance"].min(axis=0), "arrived", out["arrived_at"])
    assert out["peer_clearance"].shape == (steps, 3) and "clearance" not in out
    assert np.all(out["peer_clearance"].min(axis=0) > 0)
    assert np.all(out["arrived_at"] >= 0)
    f.close()
    # the host loop it replaces: Fleet.control(peers=True) every tick, the plant and the obstacles advanced on the host
    f, cars, states, own = crossing_fleet()
    arrived = np.full(3, -1)
    for k in range(steps):
        res = f.control(states, 2.0, [[sc.Obstacle(None, None, o.vertex + o.velocity * (DT * k), o.cone_type, o.velocity) for o in ol] for ol in own], peers=True)
        for i, (u, info) in enumerate(res):
            if info["arrive"] and arrived[i] < 0:
                arrived[i] = k
        states = [sc.kinematic_step(states[i], res[i][0], cars[i], DT) for i in range(3)]
    print("host loop: arrived", arrived)
    assert np.array_equal(arrived, out["arrived_at"])
    f.close()
