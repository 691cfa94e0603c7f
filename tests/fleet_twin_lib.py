"""What the GPU tests of the fleet rollouts share: the shapes, the three lane members with their moving scenes, fresh handles of them, the numpy rule of the
obstacle motion, the comparison of a rollout's logs with host-driven ticks, and `FleetTwin`, the fleet of fresh handles every test file derives its own
twin from.  T = 8, N = 4 slots, E = 4, iter_num = 2, dt = 0.1; B = 3 (Ackermann, differential, omni) on straight lanes 8 m apart with 7 obstacles each."""
import ctypes as C
import gc

import numpy as np
import pytest

from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import Info, dptr, iptr

T, N, E, ITER, DT = 8, 4, 4, 2, 0.1
DYN = ("acker", "diff", "omni")
NOBS, SPEED, MARGIN = 7, 4.0, 3
RDA_ERR_ARG, RDA_ERR_UNSUPPORTED, RDA_ERR_HIP = -1, -2, -3
VEL0 = [(-0.5, 0.0), (-0.3, 0.0), (0.0, -0.4), (-0.4, 0.3), (0.3, -0.3), (-0.6, 0.0), (0.2, 0.4)]
VEL1 = [(0.4, 0.0), (0.005, 0.0), (0.0, -0.3), (-0.5, 0.1), (0.0, 0.0), (0.3, 0.3), (-0.2, 0.0)]


@pytest.fixture(scope="module")
def hip():
    from rda_planner_amd._lib import hip_api
    return hip_api()


def car(e):
    return sc.rectangle_robot(dynamics=DYN[e], wheelbase=3.0 if DYN[e] == "acker" else 0)


def lane(e):
    """member e's path and its obstacles where they are at tick 0 (behind, beside and ahead of the start: the nearest four change within 5 m)
      member 0: polygons, all moving at 0.3 - 0.6 m/s, some across the lane
      member 1: circles and polygons, one of them at 0.005 m/s (it moves, its motion is not predicted), one standing
      member 2: a scene that does not move (nt = 1)"""
    y = 20.0 + 8.0 * e
    path = sc.line_path([4, y, 0], [34, y, 0], 0.1)
    scene = []
    for j in range(NOBS):
        cx, cy = 1.0 + 2.5 * j, y + (2.6 if j % 2 else -2.6)
        if e == 0:
            scene.append(sc.regular_polygon(cx, cy, 3 + j % 2, 0.8, 0.3 * j, velocity=VEL0[j]))
        elif e == 1:
            scene.append(sc.circle(cx, cy, 0.6, velocity=VEL1[j]) if j % 2 == 0 else sc.regular_polygon(cx, cy, 3 + (j // 2) % 2, 0.8, 0.3 * j, velocity=VEL1[j]))
        else:
            scene.append(sc.regular_polygon(cx, cy, 3 + j % 2, 0.8, 0.3 * j))
    return path, scene


def advanced(kind, nvert, base, vel, t):
    """the rule of scene::k_move_fleet in numpy: base + vel * t on a polygon's nvert vertices and on a circle's centre; every other entry is base's"""
    full = base + vel[:, None, :] * t
    v = np.arange(base.shape[1])[None, :]
    mask = np.where(kind[:, None] == 1, v == 0, v < nvert[:, None])
    out = base.copy()
    out[mask] = full[mask]
    return out, mask


def solver(hip, e, order=1, path=True, scene=True, robot=None, lane=lane, **kw):
    """a fresh handle of member e: its path uploaded, its raw scene resident -> (solver, start state, path length, (kind, nvert, geom, vel));
    lane: e -> (path, NOBS obstacles)"""
    from rda_planner_amd.rda_solver import RDA_solver
    sv = RDA_solver(T, robot if robot is not None else car(e), E, N, iter_num=ITER, step_time=DT, time_print=False, **kw)
    pts, obs = lane(e)
    st = np.ascontiguousarray(pts[0], float).ravel()[0:3].copy()
    if path:
        P = np.ascontiguousarray(np.hstack(pts)[0:3, :].T, dtype=float)
        assert hip.upload_path(sv._be.handle, int(P.shape[0]), dptr(P)) == 0
    n, kind, nvert, geom, vel = sv.flatten_scene(list(obs))
    kind, nvert = np.ascontiguousarray(kind, np.int32), np.ascontiguousarray(nvert, np.int32)
    geom, vel = np.ascontiguousarray(geom, float), np.ascontiguousarray(vel, float)
    assert n == NOBS and geom.shape == (NOBS, E, 2)
    if scene:
        assert hip.upload_scene(sv._be.handle, int(n), iptr(kind), iptr(nvert), dptr(geom), dptr(vel), dptr(st), order, None) == 0
    return sv, st, len(pts), (kind, nvert, geom, vel)


def bare_fleet(hip, cars, t=5):
    """rda_fleet_create of fresh handles of `cars` (T = t, N = 4, E = 4): no path, no scene, none of the fleet's on-demand tables -> (solvers, fleet)"""
    from rda_planner_amd.rda_solver import RDA_solver
    svs = [RDA_solver(t, c, 4, 4, iter_num=ITER, step_time=DT, time_print=False) for c in cars]
    F = C.c_void_p()
    assert hip.fleet_create((C.c_void_p * len(svs))(*[s._be.handle for s in svs]), len(svs), C.byref(F)) == 0
    return svs, F


def refused_in_turn(hip, call, limit=40):
    """call() -> rc with its allocation 0, 1, ... refused by the host-side hook, until it is not refused: every refusal is RDA_ERR_HIP and leaves the
    live-allocation counters (rda_debug_alloc_stats) where they were -> (the last rc, the number of refusals)"""
    def live():
        n, by = C.c_longlong(0), C.c_longlong(0)
        assert hip.debug_alloc_stats(C.byref(n), C.byref(by)) == 0
        return n.value, by.value
    gc.collect()                                                           # no handle of an earlier test is released while this one counts
    for k in range(limit):
        before = live()
        hip.debug_alloc_fail(k)
        try:
            rc = call()
        finally:
            hip.debug_alloc_fail(-1)
        if rc != RDA_ERR_HIP:
            return rc, k
        assert live() == before, (k, before, live())
    return RDA_ERR_HIP, limit


def info_tuple(i):
    return (i.resi_dual, i.resi_pri, i.iters, i.su_status, i.su_ipm_iters, i.lmz_fail)


def same_logs(a, b, keys):
    """two rollouts' logs: the arrays `keys` and the whole rda_info of every tick and member, for equality"""
    for key in keys:
        assert np.array_equal(a[key], b[key]), key
    assert a["info"] == b["info"]


def compare_ticks(logs, ticks, n=None, what=("controls", "index", "iters"), arrived_too=True, start=0):
    """a rollout's logs against host-driven ticks from its logged states ((u, s, infos, min_index, end_heading[, boxes]) per tick), for equality ->
    the number of live (member, tick) pairs.  what: `controls` - the applied control of a live member is the tick's first control; `stands` - the applied
    control of a member that has arrived is zero; `index`, `iters`, `info` (the whole rda_info), `boxes` (the box counts) - of every member, or of
    the live ones only (arrived_too=False).  n: the number of ticks there must be; start: the number of the first tick in what is printed."""
    unknown = set(what) - {"controls", "stands", "index", "iters", "info", "boxes"}
    assert not unknown, unknown
    arrived = logs["arrived_at"]
    B, live = len(arrived), 0
    for k, tick in enumerate(ticks):
        u, info, mi = tick[0], tick[2], tick[3]
        for i in range(B):
            first, got = np.array([u[i, 0, 0], u[i, 1, 0]]), logs["info"][k * B + i]
            print(f"tick {start + k} member {i}: |du| = {np.abs(logs['controls'][k, i] - first).max():.3e}  index {logs['index'][k, i]} / {mi[i]}  "
                  f"info {got} / {info[i]}" + (f"  boxes {logs['boxes'][k, i]} / {tick[5][i]}" if "boxes" in what else ""))
            alive = arrived[i] < 0 or k < arrived[i]
            live += alive
            if alive and "controls" in what:
                assert np.array_equal(logs["controls"][k, i], first), (k, i)
            if not alive and "stands" in what:
                assert np.array_equal(logs["controls"][k, i], np.zeros(2)), (k, i)
            if not (alive or arrived_too):
                continue
            if "boxes" in what:
                assert logs["boxes"][k, i] == tick[5][i], (k, i)
            if "index" in what:
                assert logs["index"][k, i] == mi[i], (k, i)
            if "iters" in what:
                assert got[2] == info[i][2], (k, i)
            if "info" in what:
                assert got == info[i], (k, i)
    assert n is None or len(ticks) == n
    return int(live)


class FleetTwin:
    """a fleet of fresh handles and what a caller keeps beside it; a test file's twin adds how it stages scenes, worlds, peers or pieces, and its entry"""
    edges = E

    def make_fleet(self, hip, svs, speed=SPEED):
        """rda_fleet_create of the solvers `svs`, and the inputs of a first tick"""
        self.hip, self.svs, self.B = hip, list(svs), len(svs)
        self.arr = (C.c_void_p * self.B)(*[s._be.handle for s in self.svs])
        self.F = C.c_void_p()
        assert hip.fleet_create(self.arr, self.B, C.byref(self.F)) == 0
        self.cur0, self.nom0, self.speed = np.zeros(self.B, np.int32), np.zeros((self.B, 2, T)), np.full(self.B, speed)

    def close(self):
        self.hip.fleet_destroy(self.F)

    def logs(self, k, **more):
        """the log arrays of a rollout of k ticks, filled so that an entry the device did not write shows; more: name=dtype adds a (k, B) log,
        name=None an absent one"""
        B, n = self.B, max(k, 1)
        out = dict(states=np.zeros((max(k, 0) + 1, B, 3)), controls=np.zeros((n, B, 2)), index=np.zeros((n, B), np.int32), info=(Info * (n * B))(),
                   arrived_at=np.full(B, -7, np.int32))
        out.update({name: None if kind is None else np.full((n, B), -7, kind) for name, kind in more.items()})
        return out

    def slots(self):
        """rda_get_obstacles of every member: [(A, b, cone, nt)]"""
        out, edges = [], self.edges
        for s in self.svs:
            A, b, cone, nt = np.zeros((N, T + 1, edges, 2)), np.zeros((N, T + 1, edges)), np.zeros(N, np.int32), np.zeros(1, np.int32)
            assert self.hip.get_obstacles(s._be.handle, dptr(A), dptr(b), iptr(cone), iptr(nt)) == 0
            m = N * int(nt[0]) * edges
            out.append((A.ravel()[:2 * m].copy(), b.ravel()[:m].copy(), cone.copy(), int(nt[0])))
        return out

    def staged(self, i):
        """the scene rows member i's slots were staged from (rda_debug_slot_src), sorted"""
        src, used = (C.c_int32 * N)(), C.c_int32(0)
        assert self.hip.lib.rda_debug_slot_src(self.svs[i]._be.handle, src, C.byref(used)) == 0
        return sorted(src[:used.value])

    def step_tracked(self, st, cur, first, speed=None):
        """rda_fleet_step_tracked -> controls, states, infos, min_index, end_heading"""
        B = self.B
        st, cur = np.ascontiguousarray(st, float), np.ascontiguousarray(cur, np.int32)
        u, s, info, mi, eh = np.zeros((B, 2, T)), np.zeros((B, 3, T + 1)), (Info * B)(), np.zeros(B, np.int32), np.zeros(B)
        rc = self.hip.fleet_step_tracked(self.F, dptr(st), dptr(self.speed if speed is None else speed), iptr(cur), 0.1, 10,
                                         dptr(self.nom0) if first else None, dptr(u), dptr(s), info, None, iptr(mi), dptr(eh))
        assert rc >= 0, rc
        return u, s, [info_tuple(i) for i in info], mi, eh
