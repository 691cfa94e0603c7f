"""-m gpu : the landing passes of k_su after their own tail of the pass body (no step-length reduction, no complementarity sum, one barrier at the blind
start): the landing still reaches the vertex it reached before.

Small closed loops - Ackermann rectangle robot, N = 8 four-edge polygons, 12 ticks, obstacles re-sorted every tick - through the C-ABI handle MPC.control
drives (rda_create_opts / rda_step ... of librda_hip.so via ctypes), at the two sweep forms of su::solve: T = 10, the smallest horizon with the time split
(su::split_point: 10 / 20 / 25 / 30), and T = 9, one below it (the generic instantiation, one recursion over the whole horizon).

(a) the start switches (su_land_blind_from = 0: no blind landings; su_land_first = 1: no speculative ones either) take other paths to the same vertex:
    applied controls within 3e-12 of the default's, and the default run does land blind (counter 19), or the comparison says nothing about them;
(b) two recorded hard su-problems whose first landing is REFUSED (the active set is still moving after four rounds) and whose interior point then goes on to
    a later stop and is landed there.  The su hook hands no landing counters back, so the problem is put into a HANDLE: rda_set_state with lam = mu = z =
    zeta = 0, a_lam = a, b_lam = cc, xi = g, dis = d0 is exactly that su-problem (tests/su_kkt.py::su_inputs_from_state, checked bit for bit here), and
    rda_admm_begin / rda_admm_su(0) / rda_admm_finish solve it with k_su.  The handle's counters (rda_debug_su_land_n) must show at least one refusal and
    one accepted landing, the solve must spend more interior-point iterations than the same start needs to reach the FIRST landing stop (a run without
    landing whose su_tol is su_land_tol: the same stop test), status 0, and (s, u, d) equal to the oracle's at TOL_U;
(c) two identical runs of (a)'s default loop are bit-equal: controls, horizons, counters (a missing barrier shows as a run-to-run difference);
(d) a REFUSED blind landing - the one start that never formed the interior point's rows, so land_refuse() alone prepares the interior-point passes behind
    it: scenes in which the default loop has one, against the loop without blind landings.
"""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as hp
from oracle.oracle_backend import switches
from rda_planner_amd import scenarios as sc

pytestmark = pytest.mark.gpu

TICKS = 12
SEED = {9: sc.SEED + 6, 10: sc.SEED + 6}     # scenes in which the default loop lands blind (chosen on the build before the lean landing passes)
SEED_REFUSED_BLIND = sc.SEED + 5             # ... and in which one of its blind landings is refused (T = 9 and T = 10, same build)
TOL_SWITCH = 3e-12                            # the start switches of the landing, applied controls


def _scene(T, seed):
    car_t = sc.rectangle_robot(dynamics="acker")
    path = sc.line_path([4, 25, 0], [44, 25, 0], 0.1)
    clear = np.array([[p[0, 0], p[1, 0]] for p in path[::10]])
    obstacles = sc.scene_polygons(8, lo=(6, 21), hi=(22, 29), seed=seed, keep_clear=clear, clear_radius=2.2)
    kw = dict(receding=T, iter_num=4, max_edge_num=4, max_obs_num=8, ro1=200, obstacle_order=True, iter_threshold=0.2)
    return car_t, path, obstacles, kw


_RUNS = {}


def _closed_loop(T, run=0, seed=None, **opts):
    """12 ticks; (applied controls [12][2], horizons [12][2][T], ADMM counts, interior-point iterations, the 20 landing counters) - computed once per key"""
    seed = SEED[T] if seed is None else seed
    key = (T, run, seed, tuple(sorted(opts.items())))
    if key in _RUNS:
        return _RUNS[key]
    from rda_planner_amd.mpc import MPC
    from rda_planner_amd.rda_solver import hip_options
    car_t, path, obstacles, kw = _scene(T, seed)
    gpu = MPC(car_t, [p.copy() for p in path], sample_time=0.1, time_print=False, hip_opts=hip_options(**opts), **kw)
    state = path[0].copy().reshape(3, 1)
    us, hs, its, ipm = [], [], [], []
    for _ in range(TICKS):
        u, info = gpu.control(state.copy(), 4.0, list(obstacles))
        assert info["status"] == 0
        us.append(np.asarray(u, float).ravel().copy()); hs.append(gpu.cur_vel_array.copy()); its.append(info["iters"]); ipm.append(info["su_ipm_iters"])
        state = sc.kinematic_step(state, u, car_t, 0.1)
    st = (C.c_int32 * 20)()
    assert gpu.rda._be.api.lib.rda_debug_su_land_n(gpu.rda._be.handle, st, 20) == 0
    _RUNS[key] = (np.array(us), np.array(hs), its, ipm, list(st))
    return _RUNS[key]


@pytest.mark.parametrize("T", [9, 10])
def test_start_switches_of_the_landing_reach_the_same_vertex(T):
    u0, _, it0, ipm0, st0 = _closed_loop(T)
    ub, _, itb, ipmb, stb = _closed_loop(T, su_land_blind_from=0)
    uf, _, itf, ipmf, stf = _closed_loop(T, su_land_first=1)
    db, df = float(np.abs(ub - u0).max()), float(np.abs(uf - u0).max())
    print(f"T={T}: default: landings accepted {st0[0]}, refused {st0[1]}, rounds {st0[2]}, blind tried {st0[18]} accepted {st0[19]}, interior-point iterations {sum(ipm0)}; "
          f"no blind landings: |du| {db:.2e} (blind tried {stb[18]}, iterations {sum(ipmb)}); light first pass only: |du| {df:.2e} (speculative tried {stf[4]}, iterations {sum(ipmf)})")
    assert st0[19] >= 1, st0                                    # the default run lands blind
    assert stb[18] == 0 and stf[4] == 0 and stf[18] == 0, (stb, stf)      # ... and the switches switch
    assert itb == it0 and itf == it0, (it0, itb, itf)
    assert db <= TOL_SWITCH and df <= TOL_SWITCH, (db, df)


@pytest.mark.parametrize("T", [9, 10])
def test_landing_loops_repeat_bit_for_bit(T):
    a, b = _closed_loop(T), _closed_loop(T, run=1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2] == b[2] and a[3] == b[3] and a[4] == b[4], (a[2:], b[2:])


@pytest.mark.parametrize("T", [9, 10])
def test_refused_blind_landing_hands_over_to_the_interior_point(T):
    u0, _, it0, ipm0, st0 = _closed_loop(T, seed=SEED_REFUSED_BLIND)
    ub, _, itb, ipmb, stb = _closed_loop(T, seed=SEED_REFUSED_BLIND, su_land_blind_from=0)
    db = float(np.abs(ub - u0).max())
    print(f"T={T}: blind landings tried {st0[18]}, accepted {st0[19]}; landings accepted {st0[0]}, refused {st0[1]}; interior-point iterations {sum(ipm0)} "
          f"(without blind landings {sum(ipmb)}); |du| against the loop without blind landings {db:.2e}")
    assert st0[18] > st0[19], st0                               # a blind landing was refused ...
    assert stb[18] == 0 and itb == it0, (stb, it0, itb)
    assert db <= TOL_SWITCH, db                                 # ... and the interior point behind it reached the vertex all the same


def _su_problem_in_a_handle(hip, cfg, si, **opts):
    """the su-problem `si` solved by k_su through a handle; ((s, u, d), status, interior-point iterations, the 20 landing counters)"""
    from rda_planner_amd._capi import Info, dptr
    from rda_planner_amd.rda_solver import hip_options
    import su_kkt
    T, N = cfg.T, cfg.N
    o, hd = hip_options(**opts), C.c_void_p()
    assert hip.create_opts(C.byref(cfg), C.byref(o), dptr(hp.G), dptr(hp.H), C.byref(hd)) == 0
    try:
        keys = ("lam", "mu", "z", "xi", "zeta", "dis", "a_lam", "b_lam")
        st = {"lam": np.zeros((N, T + 1, cfg.E)), "mu": np.zeros((N, T + 1, cfg.R)), "z": np.zeros((N, T)), "xi": np.zeros((N, T + 1, 2)), "zeta": np.zeros((N, T)),
              "dis": np.ascontiguousarray(si["d0"], float).copy(), "a_lam": np.zeros((N, T + 1, 2)), "b_lam": np.zeros((N, T + 1))}
        st["xi"][:, 1:] = si["g"]; st["a_lam"][:, 1:] = si["a"]; st["b_lam"][:, 1:] = si["cc"]
        assert hip.set_state(hd, *[dptr(st[k]) for k in keys]) == 0
        back = {k: np.zeros_like(st[k]) for k in keys}
        assert hip.get_state(hd, *[dptr(back[k]) for k in keys]) == 0
        si2 = su_kkt.su_inputs_from_state(back, si["nom_s"], si["nom_u"], si["ref"], si["vref"], hp.G, hp.H)
        assert all(np.array_equal(si2[k], si[k]) for k in ("a", "cc", "g", "d0"))       # the handle holds the recorded problem, bit for bit
        ls = (C.c_int32 * 20)()
        assert hip.debug_su_land_n(hd, ls, 20) == 0                                      # (reading clears them)
        assert hip.admm_begin(hd, dptr(si["nom_s"]), dptr(si["nom_u"]), dptr(si["ref"]), si["vref"]) == 0
        stopped = C.c_int(0)
        assert hip.admm_su(hd, 0, C.byref(stopped)) == 0
        u, s, inf = np.zeros((2, T)), np.zeros((3, T + 1)), Info()
        assert hip.admm_finish(hd, dptr(u), dptr(s), C.byref(inf)) == 0
        assert hip.debug_su_land_n(hd, ls, 20) == 0
        assert hip.get_state(hd, *[dptr(back[k]) for k in keys]) == 0
        return (s, u, back["dis"].copy()), inf.su_status, inf.su_ipm_iters, list(ls)
    finally:
        hip.destroy(hd)


@pytest.mark.parametrize("name", ["diff_T20_N24_just_active_hinges", "omni_T15_N40_hinge_flips"])      # (T = 20: time split; T = 15: one recursion)
def test_refused_landing_goes_back_to_the_interior_point(orc, hip, name):
    from rda_planner_amd.rda_solver import hip_options
    with switches(su_land=1, **hp.COLD_SU):
        cfg, si = hp.load_su_case(os.path.join(os.path.dirname(__file__), "golden", "su_hard", name + ".npz"))
        st = (C.c_long * 8)()
        orc.lib.orc_get_su_land_stats(st)                       # (reading clears them)
        so = hp.su_solve(orc.lib.orc_su_solve, cfg, si)
        orc.lib.orc_get_su_land_stats(st)
    lt = hip_options().su_land_tol
    (s, u, d), status, ipm, ls = _su_problem_in_a_handle(hip, cfg, si, su_land=1)
    _, status1, ipm1, ls1 = _su_problem_in_a_handle(hip, cfg, si, su_land=0, su_tol=(lt[0], lt[1], lt[2]))      # the same start, run to the first landing stop only
    dd = max(float(np.abs(so[1] - s).max()), float(np.abs(so[2] - u).max()), float(np.abs(so[3] - d).max()))
    print(f"{name}: kernel landings accepted {ls[0]}, refused {ls[1]}, rounds {ls[2]}, landing passes {ls[3]}; interior-point iterations {ipm}, to the first landing stop "
          f"{ipm1} (status {status1}, landings {ls1[0] + ls1[1]}); oracle: landings tried {st[0]}, accepted {st[1]}, iterations {so[4]}; |(s, u, d)_gpu - oracle| {dd:.2e}")
    assert so[0] == 0 and st[0] == 2 and st[1] == 1, list(st)   # the recorded problem: the oracle's first landing is refused too
    assert status == 0
    assert ls[1] >= 1 and ls[0] == 1, ls                        # the kernel refused a landing and accepted one
    assert status1 == 0 and ls1[0] + ls1[1] == 0 and ipm > ipm1, (ipm, ipm1, ls1)      # ... with interior-point iterations between them
    assert dd <= hp.TOL_U, dd
