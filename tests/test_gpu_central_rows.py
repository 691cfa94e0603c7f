"""-m gpu : every row of every LamMuZ launch of driven loops in the interior-point mode (`RDA_solver(..., lmz_central=mu)`), each launch form
named by rda_lammuz_kernel, against the INDEPENDENT reference of tests/lmz_central_ref.py (a damped Newton on the log-barrier problem, certified
in extended precision) - not against the oracle, which is the same algorithm with the same stop rule.  The loop is stepped with upload_obstacles +
rda_admm_begin / su / lammuz / finish; the rows are rebuilt from the handle's state before and after each launch (rows_from_state, checked on the
oracle backend by tests/test_lmz_central_ref.py), and the fused epilogue (xi += Hm, zeta += Im - d - z, the condensed A'lam and lam'b) is checked on
the duals the kernel returned, to 4 ulp of the summed terms.

T = 6, N = 5, iter_num = 3: 30 rows per launch (not a multiple of the 16-row workgroup: shadow rows), 2 MPC steps = 6 launches = 180 reference
solves per case; launches 2 .. 6 start from kept central-path points where the form keeps them.

BOUND on the relative row deviation max |d(lam, mu, z)| / (1 + max |(lam, mu, z)|), per class (accelerated, mu*): 10 x the worst deviation of the
ORACLE from the reference on the pinned CPU grid (lmz_central_ref.ORACLE_WORST: 3.4e-9, 8.9e-9, 1.3e-8, 8.1e-7 for (1, 1e-3), (1, 1e-6), (0, 1e-3),
(0, 1e-6)).  The oracle is an independent implementation with the identical stop rule (residuals <= 1e-10, |s o z - mu* e| <= 1e-7 mu*); two
implementations may stop on different iterates inside that centring band, which is what the factor 10 covers.  Nothing here is taken from a kernel.

MEASURED on an MI355X, worst row deviation per launch form and class (each test prints its own figures):
    form                 (1, 1e-3)    (1, 1e-6)    (0, 1e-3)    (0, 1e-6)
    k_lammuz_ip          8.17e-9      1.05e-8      6.95e-9      1.23e-8          (1 872 rows; warm launches 3.15e-9, history cleared 1.08e-9)
    k_lammuz_cp_small    1.66e-9                                                 (342 rows)
    k_lammuz_cp_large    4.19e-9      3.84e-10                                   (360 rows)
    bound                3.4e-8       8.9e-8       1.3e-7       8.1e-6
No row failed (Info::lmz_fail 0 outside the non-finite slot).  Epilogue errors, in units of their 4-ulp bound: xi' <= 0.18, zeta' <= 0.13, condensed
terms <= 0.34."""
from collections import namedtuple

import numpy as np
import pytest

import helpers as hp
import lmz_central_ref as ref
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import dptr, iptr, f64
from test_lmz_central_ref import ROBOTS, check_rows, drive_rows, figures

pytestmark = pytest.mark.gpu

T, N, ITERS, DT = 6, 5, 3, 0.1
IP, CP_SMALL, CP_LARGE = "k_lammuz_ip", "k_lammuz_cp_small+k_lmz_finalize", "k_lammuz_cp_large+k_lmz_finalize"
Obs = namedtuple("Obs", "A b cone_type")          # what RDA_solver._stage reads


def _poly(V, vel=None):
    """polygon with vertices V [2][k]; with a velocity: one (A, b) per stage 0 .. T (constant-velocity prediction, as MPC.convert_inequal_polygon)"""
    if vel is None:
        A, b = sc.polygon_halfspaces(V)
        return Obs(A, b, "Rpositive")
    pairs = [sc.polygon_halfspaces(V + np.reshape(vel, (2, 1)) * (t * DT)) for t in range(T + 1)]
    return Obs([p[0] for p in pairs], [p[1] for p in pairs], "Rpositive")


def _ngon(cx, cy, k, rad, yaw, vel=None):
    ang = yaw + 2 * np.pi * np.arange(k) / k
    return _poly(np.vstack((cx + rad * np.cos(ang), cy + 0.7 * rad * np.sin(ang))), vel)


def _circle(cx, cy, r):
    return Obs(np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]), np.array([[cx], [cy], [-r]]), "norm2")


def _car(robot, dynamics="diff"):
    if robot == "rectangle":
        return sc.rectangle_robot(dynamics="acker")
    if robot == "circle":
        return sc.circle_robot(radius=0.8, dynamics=dynamics)
    G, h, _ = ROBOTS[robot]
    return sc.car(G, h.reshape(-1, 1), "Rpositive", 0, [10, 1], [10, 0.5], dynamics)


def _scene(E, moving=True, count=4):
    """`count` obstacles around the nominal trajectories of `_steps` (which start in [-2, 2]^2 and travel up to 2.4 m): a full E-gon, a triangle
    (zero-padded edge rows for E > 3), a circle, a quadrilateral that moves (per-stage slots) - near ones and far ones"""
    obs = [_ngon(3.6, 1.2, E, 1.3, 0.3), _ngon(-3.4, 2.8, 3, 1.1, 1.0), _circle(0.8, -4.2, 0.9),
           _ngon(-3.8, -3.0, min(E, 4), 1.0, 0.5, (0.6, 0.4) if moving else None), _ngon(1.0, 5.0, max(3, E - 1), 1.5, 0.1)]
    return obs[:count]


def _solver(robot, E, mu, accelerated=True, **kw):
    from rda_planner_amd.rda_solver import RDA_solver
    return RDA_solver(T, _car(robot), E, N, iter_num=ITERS, iter_threshold=1e-12, accelerated=accelerated, time_print=False, lmz_central=mu, **kw)


def _steps(solver, scenes, seed):
    """one MPC step per entry of `scenes` (an obstacle list each, staged as RDA_solver.upload_obstacles stages it: a list shorter than N is padded with
    copies of its last entry, quirk Q3), with the random nominal trajectories of helpers.su_inputs"""
    rng = np.random.default_rng(seed)
    for obstacles in scenes:
        si = hp.su_inputs(rng, solver._cfg)
        n_obs, A, b, cone, per_t = solver._stage(list(obstacles))
        yield dict(n_obs=n_obs, per_t=per_t, A=f64(A) if n_obs else None, b=f64(b) if n_obs else None, cone=cone, nom_s=si["nom_s"], nom_u=f64(si["nom_u"]),
                   ref=si["ref"], speed=4.0)


def _kernel(solver):
    return solver._be.api.lib.rda_lammuz_kernel(solver._be.handle).decode()


def _certify(solver, scenes, mu, form, seed, tag, before_call=None, skip=(), fails_per_call=0, launches=None):
    """drive `scenes`; every launch must be of `form` and report the expected failure count, every row outside `skip` must meet the reference within the
    class bound and the epilogue identities within theirs.  Prints the figures, then asserts."""
    bound = ref.gpu_bound(solver._cfg.accelerated, mu)
    worst, forms, fails = {}, set(), []

    def on_call(k, it, rows, inf, out_u):
        forms.add(_kernel(solver))
        fails.append((inf.lmz_fail, (it + 1) * fails_per_call))           # (Info::lmz_fail counts over the ADMM iterations of a step)
        assert np.isfinite(out_u).all(), (tag, k, it)
        check_rows(rows, bound, f"{tag} step {k} launch {it}", worst, skip)
    calls = drive_rows(solver, _steps(solver, scenes, seed), mu, on_call, before_call)
    print(f"\n{form} | {tag} | accelerated={solver._cfg.accelerated} mu*={mu:g} | {calls} launches, {figures(worst)}; bound {bound:.1e}")
    assert calls == (ITERS * len(scenes) if launches is None else launches) and forms == {form}, (calls, forms)
    assert all(got == want for got, want in fails), fails
    assert not worst["bad"], (len(worst["bad"]), worst["bad"][:5])
    return worst


# ---- the row-parallel kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", [1e-3, 1e-6])
def test_row_parallel_kernel_mixed_scene(mu):
    """E = 4, rectangle robot: quadrilaterals, a triangle, a circle and one moving polygon (per-stage slots), 4 obstacles in 5 slots (the padding copy
    of quirk Q3 is a row like any other)"""
    s = _solver("rectangle", 4, mu)
    w = _certify(s, [_scene(4)] * 2, mu, IP, 11, "E=4 rectangle, mixed moving scene, padded list")
    assert w["rows"] == 2 * ITERS * N * T


@pytest.mark.parametrize("robot,E,accelerated,mu,ro2", [("rectangle", 5, True, 1e-6, 1.0), ("rectangle", 7, True, 1e-3, 5.0), ("triangle", 8, False, 1e-3, 1.0),
                                                        ("triangle", 8, False, 1e-6, 1.0), ("circle", 4, True, 1e-6, 1.0)])
def test_row_parallel_kernel_shapes(robot, E, accelerated, mu, ro2):
    """E = 5 (the reference's default max_edge_num); E = 7, R = 4, accelerated: with the circle obstacle's tl all 16 lanes are variables; E = 8, R = 3, not
    accelerated; the norm2 robot cone at E = 4"""
    s = _solver(robot, E, mu, accelerated, ro2=ro2)
    _certify(s, [_scene(E, moving=False, count=5), _scene(E, count=4)], mu, IP, 12 + E, f"E={E} {robot} ro2={ro2:g}")


@pytest.mark.parametrize("cold", [False, True])
def test_row_parallel_kernel_warm_and_cold_starts_end_on_the_reference_point(hip, cold):
    """launches 2 .. 6 of a loop start from the central-path points the previous launch kept; with the history cleared before every launch
    (rda_set_lmz_history, valid = 0) all start cold.  Both meet the REFERENCE (not each other)."""
    s = _solver("rectangle", 4, 1e-3)
    n = hip.lib.rda_lmz_history_doubles(s._be.handle)
    assert n == 80 * N * T
    seen = []

    def before_call(k, it):
        valid = np.zeros(N * T, np.int32)
        assert hip.lib.rda_get_lmz_history(s._be.handle, None, iptr(valid)) == 0
        seen.append(int(valid.sum()))
        if cold:
            assert hip.lib.rda_set_lmz_history(s._be.handle, None, iptr(np.zeros(N * T, np.int32))) == 0
    _certify(s, [_scene(4, moving=False)] * 2, 1e-3, IP, 21, "E=4 rectangle, " + ("history cleared before every launch" if cold else "kept points in use"), before_call)
    assert seen[0] == 0 and all(v == N * T for v in seen[1:])          # (what each launch found: nothing before the first, every row's point afterwards)


# ---- the per-thread kernels ----------------------------------------------------------------------------------------------------------------
def test_per_thread_kernel_small(monkeypatch):
    monkeypatch.setenv("RDA_LMZ_IP_ROWS", "0")
    s = _solver("rectangle", 4, 1e-3)
    _certify(s, [_scene(4)] * 2, 1e-3, CP_SMALL, 31, "E=4 R=4, RDA_LMZ_IP_ROWS=0")


@pytest.mark.parametrize("robot,E,mu", [("rectangle", 8, 1e-3), ("octagon", 4, 1e-6)])
def test_per_thread_kernel_large(robot, E, mu):
    """the shapes that do not fit 16 lanes: E = 8, R = 4, accelerated (17 variables with a circle's tl), and R = 8 at E = 4"""
    s = _solver(robot, E, mu)
    _certify(s, [_scene(E, moving=False, count=5), _scene(E, count=4)], mu, CP_LARGE, 41 + E, f"E={E} {robot}")


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
def test_empty_obstacle_list_in_this_mode():
    """quirk Q9: no obstacle staged - finite controls, no failed row (the residuals are zero: the step stops after its first launch); then the same
    handle with obstacles again"""
    s = _solver("rectangle", 4, 1e-3)
    _certify(s, [[]], 1e-3, CP_SMALL, 51, "E=4, empty list (Q9)", launches=1)
    _certify(s, [_scene(4)], 1e-3, IP, 52, "E=4, obstacles after an empty tick")


@pytest.mark.parametrize("rows_kernel", [True, False])
def test_a_non_finite_slot_keeps_its_duals_and_the_others_meet_the_reference(monkeypatch, rows_kernel):
    """step 1: a good scene (the slot gets duals); step 2: slot 1's polygon has a NaN vertex.  Its T rows keep lam, mu, z, xi, zeta bit for bit,
    lmz_fail counts exactly them, every other row still meets the reference."""
    if not rows_kernel:
        monkeypatch.setenv("RDA_LMZ_IP_ROWS", "0")
    s = _solver("rectangle", 4, 1e-3)
    good = _scene(4, moving=False, count=5)
    _certify(s, [good], 1e-3, IP if rows_kernel else CP_SMALL, 61, "E=4, before the NaN")
    before = s.get_state()
    assert np.abs(before["lam"][1]).max() > 0 and np.abs(before["zeta"][1]).max() > 0
    A = np.array(good[1].A, float); A[0, 0] = np.nan
    broken = list(good); broken[1] = good[1]._replace(A=A)
    _certify(s, [broken], 1e-3, IP if rows_kernel else CP_SMALL, 62, "E=4, slot 1 non-finite", skip=(1,), fails_per_call=T)
    after = s.get_state()
    for key in ("lam", "mu", "z", "xi", "zeta"):
        assert np.array_equal(before[key][1], after[key][1]), key
    for key in ("lam", "xi", "zeta"):
        assert not np.array_equal(before[key][0], after[key][0]), key          # (the other slots went on)


# ---- the fleet forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,form", [(8, "k_lammuz_cp_fleet_large+k_lmz_finalize_fleet"), (5, "k_lammuz_ip_fleet")])
def test_fleet_members_are_their_certified_solo_twins(E, form):
    """the fleet launches run the solo kernels' bodies with the member in the grid: two members per shape (the solo forms of both shapes are certified
    row by row above) through `Fleet.control`, bit for bit their solo `MPC.control`, with the fleet's launch form named"""
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    car_t = sc.rectangle_robot(dynamics="acker")
    solo, memb, states, scenes = [], [], [], []
    for i in range(2):
        y = 20.0 + 6 * i
        path = sc.line_path([4, y, 0], [24, y, 0], 0.1)
        kw = dict(receding=T, iter_num=ITERS, max_edge_num=E, max_obs_num=N, lmz_central=[1e-3, 1e-6][i])
        solo.append(MPC(car_t, [p.copy() for p in path], **kw))
        memb.append(MPC(car_t, [p.copy() for p in path], **kw))
        states.append(path[0].copy().reshape(3, 1))
        scenes.append([sc.regular_polygon(9.0, y + 2.6, E, 1.2, 0.2), sc.regular_polygon(12.0, y - 2.8, 3, 1.0, 0.4), sc.circle(15.0, y + 3.0, 0.8, (0.0, -0.3))])
    fleet = Fleet(memb)
    for k in range(2):
        res = fleet.control([s.copy() for s in states], 4.0, [list(sc_) for sc_ in scenes])
        assert fleet.lammuz_kernel() == form
        for i in range(2):
            u, info = solo[i].control(states[i].copy(), 4.0, list(scenes[i]))
            uf, inf = res[i]
            assert np.array_equal(u, uf), (k, i, np.abs(u - uf).max())
            assert (info["iters"], info["resi_dual"], info["lmz_fail"]) == (inf["iters"], inf["resi_dual"], inf["lmz_fail"]) and info["lmz_fail"] == 0
            assert np.array_equal(np.hstack(info["opt_state_list"]), np.hstack(inf["opt_state_list"]))
            sa, sb = solo[i].rda.get_state(), memb[i].rda.get_state()
            assert all(np.array_equal(sa[key], sb[key]) for key in sa), (k, i)
            states[i] = sc.kinematic_step(states[i], u, car_t, 0.1)
    fleet.close()
