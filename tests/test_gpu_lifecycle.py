"""GPU tests of the allocation rule of librda_hip.so (rda_planner_amd/csrc/host_buf.h): handles, fleets and the pure hooks give back
everything they allocated, and a call whose allocation fails returns RDA_ERR_HIP having changed nothing - the handle or fleet then steps
bit for bit like a twin that never saw the failed call.  Allocations are refused with rda_debug_alloc_fail (before HIP is asked: the card
never runs short) and counted with rda_debug_alloc_stats.

Safety: nothing is launched on a handle or fleet after a refused call before the live counters have shown that it holds exactly the
buffers it held before (refuse_each asserts that first)."""
import ctypes as C
import types

import numpy as np
import pytest

import helpers as hp
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import Info, Opts, dptr, iptr

from fleet_twin_lib import hip          # noqa: F401  (the fixture)
from fleet_twin_lib import info_tuple

pytestmark = pytest.mark.gpu
RDA_ERR_HIP = -3


@pytest.fixture(autouse=True)
def no_gc():
    """the counters are process-wide: no solver of an earlier test may be collected (and release its buffers) in the middle of one here"""
    import gc
    gc.collect()
    gc.disable()
    yield
    gc.enable()


def live(hip):
    n, b = C.c_longlong(0), C.c_longlong(0)
    assert hip.debug_alloc_stats(C.byref(n), C.byref(b)) == 0
    return n.value, b.value


def refuse_each(hip, call, between=None, limit=40):
    """call() with its allocation n refused, n = 0, 1, ...: every refused call returns RDA_ERR_HIP and leaves the live counters as they
    were; then between() (the twins' lockstep step).  Ends with the first call that gets through; returns (n, its return code)."""
    for n in range(limit):
        before = live(hip)
        hip.debug_alloc_fail(n)
        try:
            rc = call()
        finally:
            hip.debug_alloc_fail(-1)
        if rc != RDA_ERR_HIP:
            return n, rc
        assert live(hip) == before, (n, before, live(hip))
        if between is not None:
            between()
    raise AssertionError(f"still refused after {limit} allocations")


def opts(hip, **kw):
    o = Opts()
    hip.opts_init(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def create(hip, cfg, o=None):
    h = C.c_void_p()
    o = o if o is not None else opts(hip)
    assert hip.create_opts(C.byref(cfg), C.byref(o), dptr(hp.G), dptr(hp.H), C.byref(h)) == 0
    return h


def obstacles(rng, n, E=4):
    """host-staged polygons (per_t = 0) around the nominal trajectories of hp.su_inputs"""
    A, b, cone = np.zeros((n, 1, E, 2)), np.zeros((n, 1, E)), np.zeros(n, np.int32)
    for i in range(n):
        A[i, 0], b[i, 0] = hp.random_polygon(rng, rng.uniform((-1, -3), (6, 3)), int(rng.integers(3, E + 1)), rng.uniform(0.4, 1.0), E)
    return A, b, cone


def step(hip, h, cfg, inp, obs):
    """rda_step -> everything it hands back plus the duals"""
    T = cfg.T
    u, s, info = np.zeros((2, T)), np.zeros((3, T + 1)), Info()
    A, b, cone = obs
    rc = hip.step(h, dptr(inp["nom_s"]), dptr(inp["nom_u"]), dptr(inp["ref"]), inp["vref"], len(cone), dptr(A), dptr(b), iptr(cone), 0,
                  dptr(u), dptr(s), C.byref(info))
    assert rc >= 0, rc
    return [rc, u, s, info_tuple(info)] + get_state(hip, h, cfg)


def get_state(hip, h, cfg, products=False):
    T, N, E, R = cfg.T, cfg.N, cfg.E, cfg.R
    st = [np.zeros((N, T + 1, E)), np.zeros((N, T + 1, R)), np.zeros((N, T)), np.zeros((N, T + 1, 2)), np.zeros((N, T)), np.zeros(T)]
    st += [np.zeros((N, T + 1, 2)), np.zeros((N, T + 1))] if products else [None, None]
    assert hip.get_state(h, *[dptr(x) for x in st]) == 0
    return [x for x in st if x is not None]


def same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y), (i, float(np.abs(x - y).max()))
        else:
            assert x == y, (i, x, y)


def scene_arrays(n, seed, E=4):
    obs = sc.scene_polygons(n, lo=(1, -4), hi=(12, 4), seed=seed)
    from rda_planner_amd.rda_solver import RDA_solver
    m, kind, nvert, geom, vel = RDA_solver.flatten_scene(types.SimpleNamespace(max_edge_num=E), obs)
    return (m, np.ascontiguousarray(kind, np.int32), np.ascontiguousarray(nvert, np.int32), np.ascontiguousarray(geom, float),
            np.ascontiguousarray(vel, float))


def upload_scene(hip, h, scn, xy=(0.0, 0.0)):
    m, kind, nvert, geom, vel = scn
    return hip.upload_scene(h, m, iptr(kind), iptr(nvert), dptr(geom), dptr(vel), dptr(np.array(xy, float)), 1, None)


def step_scene(hip, h, cfg, inp, scn):
    T = cfg.T
    m, kind, nvert, geom, vel = scn
    u, s, info = np.zeros((2, T)), np.zeros((3, T + 1)), Info()
    rc = hip.step_scene(h, dptr(inp["nom_s"]), dptr(inp["nom_u"]), dptr(inp["ref"]), inp["vref"], m, iptr(kind), iptr(nvert), dptr(geom),
                        dptr(vel), dptr(inp["nom_s"][0:2, 0].copy()), 1, dptr(u), dptr(s), C.byref(info))
    assert rc >= 0, rc
    return [rc, u, s, info_tuple(info)] + get_state(hip, h, cfg)


def path_array(y, L):
    path = sc.line_path([0, y, 0], [0.1 * (L - 1), y, 0], 0.1)[:L]
    return np.ascontiguousarray(np.hstack(path)[0:3, :].T, dtype=float)


def step_tracked(hip, h, cfg, state):
    T = cfg.T
    u, s, info, mi, eh = np.zeros((2, T)), np.zeros((3, T + 1)), Info(), C.c_int32(0), C.c_double(0)
    ref = np.zeros((3, T + 1))
    rc = hip.step_tracked(h, dptr(state), 3.0, 0, 0.1, 10, None, dptr(u), dptr(s), C.byref(info), None, dptr(ref), C.byref(mi), C.byref(eh))
    assert rc >= 0, rc
    return [rc, u, s, ref, info_tuple(info), mi.value, eh.value] + get_state(hip, h, cfg)


def test_handles_fleets_and_hooks_give_back_everything(hip):
    """live allocations / bytes return to their starting values after handles of several shapes and uses, a fleet of 4 that ran the tracked
    step and the scene re-sort, and 20 calls of each pure hook"""
    rng = np.random.default_rng(1)
    start = live(hip)
    for T in (10, 20, 40):
        cfg = hp.make_cfg(T=T, N=12)
        h = create(hip, cfg)
        assert live(hip)[0] > start[0]
        step(hip, h, cfg, hp.su_inputs(rng, cfg), obstacles(rng, 7))
        hip.destroy(h)
        assert live(hip) == start, T
    cfg = hp.make_cfg(T=10, N=12)
    h = create(hip, cfg, opts(hip, lmz_mode=1))                     # interior-point LamMuZ mode with its kept central points
    assert hip.lib.rda_lmz_history_doubles(h) == 80 * cfg.N * cfg.T
    step(hip, h, cfg, hp.su_inputs(rng, cfg), obstacles(rng, 7))
    hip.destroy(h)
    assert live(hip) == start
    h = create(hip, cfg, opts(hip, duals_follow=1))
    inp = hp.su_inputs(rng, cfg)
    step_scene(hip, h, cfg, inp, scene_arrays(9, 3))
    step_scene(hip, h, cfg, inp, scene_arrays(30, 4))                 # the scene buffers grow
    hip.destroy(h)
    assert live(hip) == start
    cfg9 = hp.make_cfg(T=10, N=9)
    h = create(hip, cfg9)
    assert hip.shard_config(h, 1, 2) == 0                           # padded shards (N % world != 0)
    hip.destroy(h)
    assert live(hip) == start
    h = create(hip, cfg)
    K, T = 3, cfg.T
    tr = [np.ascontiguousarray(x) for x in (np.zeros((K, 3, T + 1)), np.zeros((K, 2, T)), np.zeros((K, 3, T + 1)), np.full(K, 2.0))]
    for _ in range(2):                                              # the second upload replaces the first
        assert hip.lib.rda_upload_trace(h, K, *[dptr(x) for x in tr]) == 0
    assert hip.upload_path(h, 50, dptr(path_array(0.0, 50))) == 0
    assert hip.upload_path(h, 80, dptr(path_array(0.0, 80))) == 0
    assert upload_scene(hip, h, scene_arrays(9, 5)) == 0
    hip.destroy(h)
    assert live(hip) == start
    memb, F = fleet(hip, 4, cfg)
    run_fleet_tracked(hip, F, memb, cfg, resort=True)
    hip.fleet_destroy(F)
    for h in memb:
        hip.destroy(h)
    assert live(hip) == start
    inp = hp.lammuz_batch_inputs(rng, 64)
    su_cfg = hp.make_cfg(T=20, N=6)
    su_inp = hp.su_inputs(rng, su_cfg)
    for _ in range(20):
        hp.hip_lammuz_batch(hip, inp)
        assert live(hip) == start
        assert hp.su_solve(hip.lib.rda_su_solve, su_cfg, su_inp)[0] in (0, 1)
        assert live(hip) == start


def test_failed_create_leaves_nothing_behind(hip):
    """rda_create_opts refused at each of its allocations: RDA_ERR_HIP, *out = NULL, nothing held; the handle that is finally made steps like
    one made without refusals"""
    rng = np.random.default_rng(2)
    for kw in ({}, {"lmz_mode": 1}, {"duals_follow": 1}):
        cfg = hp.make_cfg(T=10, N=9)
        o = opts(hip, **kw)
        h = C.c_void_p()

        def call():
            h.value = 12345
            rc = hip.create_opts(C.byref(cfg), C.byref(o), dptr(hp.G), dptr(hp.H), C.byref(h))
            assert rc == 0 or not h.value, (rc, h.value)
            return rc
        n, rc = refuse_each(hip, call)
        assert rc == 0 and n >= 30, (kw, n, rc)
        twin = create(hip, cfg, o)
        inp, scn = hp.su_inputs(rng, cfg), scene_arrays(8, 9)           # (duals_follow takes scenes only)
        same(step_scene(hip, h, cfg, inp, scn), step_scene(hip, twin, cfg, inp, scn))
        hip.destroy(h)
        hip.destroy(twin)


def test_failed_trace_path_scene_uploads_keep_the_old_ones(hip):
    """a refused rda_upload_trace / rda_upload_path / rda_upload_scene leaves the handle with its old trace / path / scene: after every
    refusal the handle replays the old trace, tracks the old path and steps the old scene like its twin; the upload that goes through
    then works like the twin's"""
    rng = np.random.default_rng(3)
    cfg = hp.make_cfg(T=10, N=9)
    T = cfg.T
    a, b = create(hip, cfg), create(hip, cfg)
    obs = obstacles(rng, 6)

    def trace(K):
        inp = [hp.su_inputs(rng, cfg) for _ in range(K)]
        return [np.ascontiguousarray(np.array([x[k] for x in inp])) for k in ("nom_s", "nom_u", "ref")] + [np.full(K, 3.0)]

    def replay(h, K):
        assert hip.lib.rda_enqueue_range(h, 0, K) == 0
        out = []
        for k in range(K):
            u, s, info = np.zeros((2, T)), np.zeros((3, T + 1)), Info()
            assert hip.lib.rda_fetch_result(h, k, dptr(u), dptr(s), C.byref(info)) == 0
            out += [u, s, info_tuple(info)]
        return out + get_state(hip, h, cfg)

    for h in (a, b):
        A, bb, cone = obs
        assert hip.upload_obstacles(h, len(cone), dptr(A), dptr(bb), iptr(cone), 0) == 0
    old, new = trace(2), trace(4)
    for h in (a, b):
        assert hip.lib.rda_upload_trace(h, 2, *[dptr(x) for x in old]) == 0
    n, rc = refuse_each(hip, lambda: hip.lib.rda_upload_trace(a, 4, *[dptr(x) for x in new]), lambda: same(replay(a, 2), replay(b, 2)))
    assert rc == 0 and n == 7, (n, rc)
    assert hip.lib.rda_upload_trace(b, 4, *[dptr(x) for x in new]) == 0
    same(replay(a, 4), replay(b, 4))

    p_old, p_new = path_array(0.5, 60), path_array(0.5, 120)
    for h in (a, b):
        assert hip.upload_path(h, 60, dptr(p_old)) == 0
    state = np.array([0.3, 0.2, 0.0])
    n, rc = refuse_each(hip, lambda: hip.upload_path(a, 120, dptr(p_new)), lambda: same(step_tracked(hip, a, cfg, state), step_tracked(hip, b, cfg, state)))
    assert rc == 0 and n == 1, (n, rc)
    assert hip.upload_path(b, 120, dptr(p_new)) == 0
    same(step_tracked(hip, a, cfg, state), step_tracked(hip, b, cfg, state))

    inp = hp.su_inputs(rng, cfg)
    s_old, s_new = scene_arrays(8, 6), scene_arrays(40, 7)
    for first in (True, False):                                     # the first scene of the handles, then a larger one
        scn = s_old if first else s_new
        n, rc = refuse_each(hip, lambda: upload_scene(hip, a, scn),
                            (lambda: same(step(hip, a, cfg, inp, obs), step(hip, b, cfg, inp, obs))) if first else
                            (lambda: same(step_scene(hip, a, cfg, inp, s_old), step_scene(hip, b, cfg, inp, s_old))))
        assert rc == 0 and n == 4, (first, n, rc)
        assert upload_scene(hip, b, scn) == 0
        same(step_scene(hip, a, cfg, inp, scn), step_scene(hip, b, cfg, inp, scn))
    hip.destroy(a)
    hip.destroy(b)


def test_failed_shard_config_and_state_calls_change_nothing(hip):
    """a refused rda_shard_config keeps the single-shard geometry and terms; a refused rda_get_state / rda_set_state with products writes
    nothing (set_state allocates before it writes the duals)"""
    rng = np.random.default_rng(4)
    cfg = hp.make_cfg(T=10, N=9)
    a, b = create(hip, cfg), create(hip, cfg)
    inp, obs = hp.su_inputs(rng, cfg), obstacles(rng, 7)
    lock = lambda: same(step(hip, a, cfg, inp, obs), step(hip, b, cfg, inp, obs))      # noqa: E731
    lock()
    buf = [np.zeros_like(x) for x in get_state(hip, b, cfg, products=True)]

    def untouched():                                                # the refused get_state wrote nothing either
        assert not any(x.any() for x in buf)
        lock()
    n, rc = refuse_each(hip, lambda: hip.get_state(a, *[dptr(x) for x in buf]), untouched)
    assert rc == 0 and n == 2, (n, rc)
    same(buf, get_state(hip, b, cfg, products=True))
    st = get_state(hip, b, cfg, products=True)
    st2 = [0.5 * x for x in st]                                     # a state the handles do not have: a half-written one would show
    n, rc = refuse_each(hip, lambda: hip.set_state(a, *[dptr(x) for x in st2]), lock)
    assert rc == 0 and n == 2, (n, rc)
    assert hip.set_state(b, *[dptr(x) for x in st2]) == 0
    same(get_state(hip, a, cfg, products=True), get_state(hip, b, cfg, products=True))
    lock()

    c, d = create(hip, cfg), create(hip, cfg)
    single = hip.shard_chunk_doubles(c)
    n, rc = refuse_each(hip, lambda: hip.shard_config(c, 1, 2),
                        lambda: (assert_chunk(hip, c, d), same(step(hip, c, cfg, inp, obs), step(hip, d, cfg, inp, obs))))
    assert rc == 0 and n == 2, (n, rc)
    assert hip.shard_config(d, 1, 2) == 0
    assert hip.shard_chunk_doubles(c) < single
    assert_chunk(hip, c, d)                                         # (two shards, no communicator: compared, not stepped)
    for h in (a, b, c, d):
        hip.destroy(h)


def assert_chunk(hip, c, d):
    n = hip.shard_chunk_doubles(c)
    assert n == hip.shard_chunk_doubles(d)
    x, y = np.zeros(n), np.zeros(n)
    assert hip.shard_get_chunk(c, dptr(x)) == 0 and hip.shard_get_chunk(d, dptr(y)) == 0
    assert np.array_equal(x, y)


def fleet(hip, B, cfg, with_fleet=True):
    """B members with paths and resident scenes (tracked stepping, scene re-sort) and their fleet"""
    memb = []
    for e in range(B):
        h = create(hip, cfg)
        assert hip.upload_path(h, 120, dptr(path_array(0.6 * e, 120))) == 0
        assert upload_scene(hip, h, scene_arrays(6 + 2 * e, 20 + e), (0.0, 0.6 * e)) == 0
        memb.append(h)
    if not with_fleet:
        return memb
    arr = (C.c_void_p * B)(*memb)
    F = C.c_void_p()
    assert hip.fleet_create(arr, B, C.byref(F)) == 0
    return memb, F


def states_of(B):
    return np.ascontiguousarray(np.array([[0.2, 0.6 * e, 0.0] for e in range(B)]))


def run_fleet_tracked(hip, F, memb, cfg, resort):
    B, T = len(memb), cfg.T
    st = states_of(B)
    if resort:
        assert hip.fleet_scene_resort(F, dptr(st), 3) == 0
    u, s, info = np.zeros((B, 2, T)), np.zeros((B, 3, T + 1)), (Info * B)()
    ref, mi, eh = np.zeros((B, 3, T + 1)), np.zeros(B, np.int32), np.zeros(B)
    rc = hip.fleet_step_tracked(F, dptr(st), dptr(np.full(B, 3.0)), iptr(np.zeros(B, np.int32)), 0.1, 10, None, dptr(u), dptr(s), info,
                                dptr(ref), iptr(mi), dptr(eh))
    assert rc >= 0, rc
    return [rc, u, s, ref, mi, eh] + [info_tuple(i) for i in info]


def run_fleet_step(hip, F, memb, cfg, inp):
    B, T = len(memb), cfg.T
    u, s, info = np.zeros((B, 2, T)), np.zeros((B, 3, T + 1)), (Info * B)()
    rc = hip.fleet_step(F, dptr(inp[0]), dptr(inp[1]), dptr(inp[2]), dptr(np.full(B, 3.0)), dptr(u), dptr(s), info)
    assert rc >= 0, rc
    return [rc, u, s] + [info_tuple(i) for i in info]


def test_failed_fleet_calls_change_nothing(hip):
    """rda_fleet_create, the first rda_fleet_scene_resort and the first rda_fleet_step_tracked (their tables are made on first use)
    refused at each allocation: nothing held, and the fleet steps like a twin fleet that never saw the refusals"""
    rng = np.random.default_rng(5)
    B, cfg = 4, hp.make_cfg(T=10, N=9)
    ma, mb = fleet(hip, B, cfg, with_fleet=False), fleet(hip, B, cfg, with_fleet=False)
    Fa, Fb = C.c_void_p(), C.c_void_p()
    arr_a, arr_b = (C.c_void_p * B)(*ma), (C.c_void_p * B)(*mb)
    n, rc = refuse_each(hip, lambda: hip.fleet_create(arr_a, B, C.byref(Fa)))
    assert rc == 0 and n == 11, (n, rc)
    assert hip.fleet_create(arr_b, B, C.byref(Fb)) == 0
    inp = [np.zeros((B,) + x.shape) for x in (np.zeros((3, cfg.T + 1)), np.zeros((2, cfg.T)), np.zeros((3, cfg.T + 1)))]
    for e in range(B):
        si = hp.su_inputs(rng, cfg)
        inp[0][e], inp[1][e], inp[2][e] = si["nom_s"], si["nom_u"], si["ref"]
    inp = [np.ascontiguousarray(x) for x in inp]
    lock = lambda: same(run_fleet_step(hip, Fa, ma, cfg, inp), run_fleet_step(hip, Fb, mb, cfg, inp))     # noqa: E731
    lock()
    st = states_of(B)
    n, rc = refuse_each(hip, lambda: hip.fleet_scene_resort(Fa, dptr(st), 3), lock)
    assert rc == 0 and n == 4, (n, rc)
    assert hip.fleet_scene_resort(Fb, dptr(st), 3) == 0
    lock()

    T = cfg.T
    outs = {}

    def tracked(F, key):
        u, s, info = np.zeros((B, 2, T)), np.zeros((B, 3, T + 1)), (Info * B)()
        ref, mi, eh = np.zeros((B, 3, T + 1)), np.zeros(B, np.int32), np.zeros(B)
        rc = hip.fleet_step_tracked(F, dptr(st), dptr(np.full(B, 3.0)), iptr(np.zeros(B, np.int32)), 0.1, 10, None, dptr(u), dptr(s), info,
                                    dptr(ref), iptr(mi), dptr(eh))
        outs[key] = [rc, u, s, ref, mi, eh] + [info_tuple(i) for i in info]
        return rc
    n, rc = refuse_each(hip, lambda: tracked(Fa, "a"), lock)
    assert rc >= 0 and n == 10, (n, rc)
    assert tracked(Fb, "b") >= 0
    same(outs["a"], outs["b"])
    same(run_fleet_tracked(hip, Fa, ma, cfg, True), run_fleet_tracked(hip, Fb, mb, cfg, True))
    for F in (Fa, Fb):
        hip.fleet_destroy(F)
    for h in ma + mb:
        hip.destroy(h)


def test_failed_hook_calls_leak_nothing(hip):
    """rda_lammuz_batch and rda_su_solve_opts refused at each allocation: RDA_ERR_HIP and nothing held; the call that goes through returns
    what an undisturbed call returns"""
    rng = np.random.default_rng(6)
    inp = hp.lammuz_batch_inputs(rng, 48)
    want = hp.hip_lammuz_batch(hip, inp)
    B, E = inp["b"].shape
    R = hp.G.shape[0]
    got = [np.zeros((B, E)), np.zeros((B, R)), np.zeros(B), np.zeros((B, 4))]
    arr = {k: np.ascontiguousarray(v) for k, v in inp.items()}
    n, rc = refuse_each(hip, lambda: hip.lib.rda_lammuz_batch(B, E, R, dptr(arr["A"]), dptr(arr["b"]), iptr(arr["cone"]), dptr(arr["p"]),
                                                              dptr(arr["phi"]), dptr(hp.G), dptr(hp.H), dptr(arr["xi"]), dptr(arr["zeta"]),
                                                              dptr(arr["dbar"]), 1.0, 1e-6, 1, *[dptr(x) for x in got]))
    assert rc == 0 and n == 14, (n, rc)
    same(list(want), got)
    cfg = hp.make_cfg(T=20, N=6)
    si = hp.su_inputs(rng, cfg)
    o = opts(hip)
    want = hp.su_solve(hip.lib.rda_su_solve, cfg, si)
    res = {}

    def call():
        r = hp.su_solve(lambda *a: hip.lib.rda_su_solve_opts(a[0], C.byref(o), *a[1:]), cfg, si)
        res["r"] = r
        return r[0]
    n, rc = refuse_each(hip, call)
    assert n == 10 and rc == want[0], (n, rc)
    same(list(want), list(res["r"]))
