"""-m gpu : every row of every LamMuZ launch of driven loops in the DEFAULT mode (support enumeration, tie-breaks T1 - T3, remembered supports), each
launch form named by rda_lammuz_kernel, against the optimality certificate of tests/lmz_rows_cert.py - the KKT conditions of the documented row problem
(criterion A) or, in the slack regime, optimality for the reference's own problem with the normal in the middle of an arc located by two LPs per
direction (criterion B), and T2 - evaluated in extended precision on the duals the kernel returned.  Not against the oracle (the same enumeration by
the same hand), not against another kernel, not form against form.  The loop is stepped with upload_obstacles + rda_admm_begin / su / lammuz / finish;
the rows are rebuilt from the handle's state before and after each launch (lmz_central_ref.rows_from_state, checked on the oracle backend in the
default mode by tests/test_lmz_rows_cert.py), and the fused epilogue is checked on the returned duals to 4 ulp of the summed terms.

T = 6, N = 5, iter_num = 3, iter_threshold = 1e-12, 2 MPC steps: 30 rows per launch (not a multiple of the 16-row workgroup: shadow rows), 6
launches.  Launch 1 enumerates every row; launches 2 .. 6 run the remembered-support, one-row-away and enumeration paths, the nominal trajectory is
redrawn between the steps.  The arc of criterion B is located on at most 24 class-B rows per case (every k-th).

SCENES.  The kinds of the mixed scene of tests/test_gpu_central_rows.py (a full E-gon, a zero-padded triangle, a circle, a moving quadrilateral with
per-stage slots, 4 obstacles in 5 slots), but the E-gon and the triangle are placed relative to the step's nominal trajectory - beside the body and
diagonally ahead of it, in contact range - and the solvers run with min_sd = 0.6 (default 0.1), so that a polygon within 0.6 m of the body is a row with
an active hinge.  With the fixed scene and the default min_sd the oracle backend had no polygon row with an active hinge at all: class A was the circle.

BOUNDS: 10 x the worst figure of the numpy oracle and the C oracle's per-row solve, accelerated on and off, on the pinned CPU grid
(lmz_rows_cert.ORACLE_WORST = feas 2.7e-16, kkt 1.4e-14, H 0.95, arc 1.8e-15, z 0.8; printed and held by tests/test_lmz_rows_cert.py): feasibility 2.7e-15
absolute, scaled KKT residual 1.4e-13, |H| 9.5 eps and z 8 eps of their summed terms, arc half-widths 1.8e-14 rad.  m >= 0 of criterion B is held exactly
(both oracles: 0).  Nothing is taken from a kernel; the nearest wrong answer tried on the CPU (tests/test_lmz_rows_cert.py: the optimum of the neighbouring
problem xi + 1e-8, the delta = 0 optimum, the un-centred answer, a normal rotated by 1e-6 rad, the wrong z) lies 690 x outside its bound.

Every case asserts: the launch form by name, Info::lmz_fail, no row outside the certificate (none skipped but a slot made non-finite on purpose), no
class-A row that meets T1's trigger with a proper arc (centring quietly dropped), the epilogue identities, at least 10 rows of each class - and the
COMPOSITION of class A: at least 4 polygon rows with an active hinge on the unit circle (|a| = 1, m < 0: the nu branch of criterion A, the norm-constrained
candidates of the enumeration) and at least 1 polygon row that rests on a robot corner (two robot edges in the support).  tests/test_lmz_rows_cert.py
asserts twice these counts on the oracle backend.

MEASURED on an MI355X, worst figure per launch form (each test prints its own).  Class A is given as rows / polygon rows with duals / of them |a| = 1 and
m < 0 / on a robot corner; m_neg is 0 in every row of every case.
    form                                              class A             B      kkt        feas       H      z      arc (rows)         epilogue xi / zeta / cond.
    k_lammuz_rows (7 shapes)                          355 / 211 / 158 / 39 905    9.59e-14   5.2e-16    0.96   0.66   2.29e-15 (162)     0.20 / 0.17 / 0.19
    k_lammuz_rows, RDA_LMZ_WARM=0                      67 /  31 /  29 /  3 113    1.25e-14   4.4e-16    0.96   0.28   1.22e-15 (23)      0.16 / 0.12 / 0.15
    k_lammuz_rows, RDA_TIE_CENTRE=0                   180 / 144 /  29 / 74   0    1.18e-14   4.0e-16    -      0.29   -                  0.18 / 0.10 / 0.12
    k_lammuz_rows, after an empty tick / NaN slot     160 / 109 /  84 /  9  92    5.01e-14   4.6e-16    0.66   0.22   1.67e-15 (46)      0.16 / 0.16 / 0.13
    k_lammuz+k_lmz_finalize (E = 4 by switch)          67 /  31 /  29 /  3 113    1.25e-14   4.4e-16    0.96   0.28   1.22e-15 (23)      0.16 / 0.12 / 0.15
    k_lammuz+k_lmz_finalize (E = 8, octagon)           56 /  27 /  27 /  9 124    1.12e-13   4.4e-16    0.69   0.34   6.66e-16 (21)      0.13 / 0.14 / 0.15
    k_lammuz+k_lmz_finalize, NaN slot                  98 /  62 /  58 /  6  64    5.01e-14   4.3e-16    0.57   0.22   1.67e-15 (32)      0.13 / 0.16 / 0.13
    k_lammuz_rows_fast+k_lammuz_enum+k_lmz_finalize    67 /  31 /  29 /  3 113    1.25e-14   4.4e-16    0.96   0.28   1.22e-15 (23)      0.16 / 0.12 / 0.15
    k_lammuz_rows_dense                                67 /  31 /  29 /  3 113    1.25e-14   4.4e-16    0.96   0.28   1.22e-15 (23)      0.16 / 0.12 / 0.15
    bound                                                                         1.4e-13    2.7e-15    9.5    8      1.8e-14            1 / 1 / 1
(kkt: scaled residual; feas: absolute; H, z: eps of the summed terms; arc: radians; epilogue: units of its 4-ulp bound.)  The two largest KKT residuals,
9.59e-14 (E = 4, octagon) and 1.12e-13 (E = 8, octagon), are rows on which the oracle backend has 9.58e-14 and 1.12e-13 itself: the conditioning of the
row, not the kernel; everywhere else the kernels stay below 5.1e-14.  Rows on the work list of the split form per launch: 24, 0, 0, 16, 4, 0 - the 4 of
launch 5 are rows whose remembered support failed in a warm launch.  No launch reported a failed row outside the non-finite slot; no class-A row met T1's
trigger."""
import ctypes as C

import numpy as np
import pytest

import lmz_rows_cert as cert
import helpers as hp
from rda_planner_amd._capi import f64
from test_gpu_central_rows import T, N, ITERS, _car, _circle, _ngon
from test_lmz_central_ref import drive_rows

pytestmark = pytest.mark.gpu

ROWS, DENSE, SPLIT, WAVE = "k_lammuz_rows", "k_lammuz_rows_dense", "k_lammuz_rows_fast+k_lammuz_enum+k_lmz_finalize", "k_lammuz+k_lmz_finalize"
MIN_PER_CLASS = 10
MIN_POLYGON_UNIT, MIN_CORNER = 4, 1          # of class A: polygon rows with an active hinge and |a| = 1; polygon rows with two robot edges in the support
MIN_SD = 0.6          # the lower bound of the safety distance d-bar (default 0.1): a polygon within 0.6 m of the body is a row with an active hinge

# the shapes of the k_lammuz_rows cases: id -> (robot, E, accelerated, ro2, seed).  tests/test_lmz_rows_cert.py runs each on the oracle backend.
SHAPES = {
    "E4-rectangle": ("rectangle", 4, True, 1.0, 11),           # the mixed scene: quadrilaterals, a padded triangle, a circle, a moving polygon, 4 obstacles in 5 slots
    "E3-rectangle": ("rectangle", 3, True, 1.0, 20),
    "E5-rectangle": ("rectangle", 5, True, 1.0, 17),
    "E7-rectangle-ro2=5": ("rectangle", 7, True, 5.0, 21),
    "E8-triangle-flat": ("triangle", 8, False, 1.0, 20),
    "E4-octagon": ("octagon", 4, True, 1.0, 11),
    "E8-rectangle": ("rectangle", 8, True, 1.0, 20),           # the central-normal step needs two rounds of vertex pairs per row
    "E8-octagon": ("octagon", 8, True, 1.0, 11),               # E + R + 1 > 16: one row per wave
}


# where the two near polygons lie in the body frame of stage 3, per robot (the rectangle is 4.6 x 1.6 around (1.5, 0), the octagon 2.4 x 1.6 around the origin)
NEAR = {"rectangle": ((1.5, -2.2), (5.2, 2.1)), "triangle": ((1.5, -2.2), (5.2, 2.1)), "octagon": ((0.0, -2.0), (2.3, 1.8))}


def _scene(E, moving=True, count=4, robot="rectangle"):
    """the kinds of the mixed scene of tests/test_gpu_central_rows.py - a full E-gon, a triangle (zero-padded edge rows for E > 3), a circle, a quadrilateral
    that moves (per-stage slots), an (E - 1)-gon - as a function of the step's nominal trajectory `nom_s` [3][T + 1] (drawn at random by `_steps`): the E-gon
    lies beside the body at stage 3 and the triangle diagonally ahead of it, both within the safety distance but clear of the body, so that polygon rows
    with an active hinge and the norm constraint binding (class A, |a| = 1, m < 0) stand next to rows in the slack regime (class B); the circle sits in
    the start region, the other two far away."""
    def scene(nom_s):
        x, y, phi = nom_s[:, 3]
        c, s = np.cos(phi), np.sin(phi)
        at = lambda bx, by: (x + c * bx - s * by, y + s * bx + c * by)          # body frame of stage 3 -> world
        obs = [_ngon(*at(*NEAR[robot][0]), E, 1.0, phi + 0.3), _ngon(*at(*NEAR[robot][1]), 3, 1.0, phi + 1.0), _circle(0.6, -2.8, 0.9),
               _ngon(-3.8, -3.0, min(E, 4), 1.0, 0.5, (0.6, 0.4) if moving else None), _ngon(1.0, 5.0, max(3, E - 1), 1.5, 0.1)]
        return obs[:count]
    return scene


def _steps(solver, scenes, seed):
    """one MPC step per entry of `scenes` - an obstacle list, or a function of the step's nominal states that returns one - staged as
    RDA_solver.upload_obstacles stages it (a list shorter than N is padded with copies of its last entry, quirk Q3), with the random nominal trajectories
    of helpers.su_inputs"""
    rng = np.random.default_rng(seed)
    for obstacles in scenes:
        si = hp.su_inputs(rng, solver._cfg)
        n_obs, A, b, cone, per_t = solver._stage(list(obstacles(si["nom_s"]) if callable(obstacles) else obstacles))
        yield dict(n_obs=n_obs, per_t=per_t, A=f64(A) if n_obs else None, b=f64(b) if n_obs else None, cone=cone, nom_s=si["nom_s"], nom_u=f64(si["nom_u"]),
                   ref=si["ref"], speed=4.0)


def scenes_of(shape):
    """the two MPC steps of a shape: the mixed moving scene with a padded list twice for E = 4 rectangle, else the static scene of 5 obstacles, then the moving one of 4"""
    robot, E, *_ = SHAPES[shape]
    return [_scene(4)] * 2 if shape == "E4-rectangle" else [_scene(E, moving=False, count=5, robot=robot), _scene(E, count=4, robot=robot)]


def make_solver(shape, **kw):
    from rda_planner_amd.rda_solver import RDA_solver
    robot, E, accelerated, ro2, _ = SHAPES[shape]
    return RDA_solver(T, _car(robot), E, N, iter_num=ITERS, iter_threshold=1e-12, accelerated=accelerated, time_print=False, ro2=ro2, min_sd=MIN_SD, **kw)


def certify_loop(solver, scenes, form, seed, tag, skip=(), fails_per_call=0, launches=None, tie_centre=1, classes=True, after_call=None, arcs=cert.ARC_ROWS, corner=True):
    """drive `scenes`; every launch must be of `form` (None: a backend without launch forms) and report the expected failure count, every row outside
    `skip` must pass the certificate and the epilogue identities, and both classes must be present; the arc is located on at most `arcs` class-B rows.
    Prints the figures, then asserts."""
    worst, forms, fails = {}, set(), []

    def on_call(k, it, rows, inf, out_u):
        if form is not None:
            forms.add(solver._be.api.lib.rda_lammuz_kernel(solver._be.handle).decode())
        fails.append((inf.lmz_fail, (it + 1) * fails_per_call))           # (Info::lmz_fail counts over the ADMM iterations of a step)
        assert np.isfinite(out_u).all(), (tag, k, it)
        cert.check_rows(rows, f"{tag} step {k} launch {it}", worst, skip, tie_centre)
        if after_call is not None:
            after_call(k, it)
    calls = drive_rows(solver, _steps(solver, scenes, seed), 0.0, on_call)
    cert.check_arcs(worst, arcs)
    print(f"\n{form or 'oracle backend'} | {tag} | {calls} launches, {cert.figures(worst)}")
    assert calls == (ITERS * len(scenes) if launches is None else launches) and (form is None or forms == {form}), (calls, forms)
    assert all(got == want for got, want in fails), fails
    assert not worst.get("bad"), (len(worst["bad"]), worst["bad"][:5])
    if classes:
        assert worst.get("A", 0) >= MIN_PER_CLASS and worst.get("B", 0) >= MIN_PER_CLASS, (worst.get("A", 0), worst.get("B", 0))
        # ... and class A is not the circle's rows alone: polygon rows with an active hinge on the unit circle (the nu branch of criterion A, the
        # norm-constrained candidates of the enumeration) and rows that rest on a robot corner (`corner`: not where the slot that yields them is left out)
        assert worst.get("A_poly_unit", 0) >= MIN_POLYGON_UNIT and (not corner or worst.get("A_poly_mu2", 0) >= MIN_CORNER), (worst.get("A_poly_unit", 0), worst.get("A_poly_mu2", 0))
    return worst


def _run(shape, form, tag="", **kw):
    s = make_solver(shape)
    return certify_loop(s, scenes_of(shape), form, SHAPES[shape][4], f"{shape}{tag}", **kw)


# ---- k_lammuz_rows -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [k for k in SHAPES if k != "E8-octagon"])
def test_packed_rows_kernel(shape):
    w = _run(shape, ROWS)
    assert w["rows"] == 2 * ITERS * N * T


# ---- k_lammuz + k_lmz_finalize -------------------------------------------------------------------------------------------------------------------
def test_one_row_per_wave_kernel_by_switch(monkeypatch):
    monkeypatch.setenv("RDA_LMZ_ROWS", "0")
    _run("E4-rectangle", WAVE, ", RDA_LMZ_ROWS=0")


def test_one_row_per_wave_kernel_by_shape():
    """E = 8 with the octagon robot: E + R + 1 = 17 > 16, the packed form does not apply"""
    _run("E8-octagon", WAVE)


# ---- the dense forms ---------------------------------------------------------------------------------------------------------------------------
def test_split_form_and_its_work_list(monkeypatch):
    """k_lammuz_rows_fast + k_lammuz_enum + k_lmz_finalize; the work-list kernel must have had rows in warm launches, one of them not the first of a step"""
    monkeypatch.setenv("RDA_LMZ_DENSE_FROM", "0")
    s = make_solver("E4-rectangle")
    listed = []

    def after_call(k, it):
        rows = C.c_int(-1)
        assert s._be.api.lib.rda_debug_worklist(s._be.handle, C.byref(rows)) == 0
        listed.append(rows.value)
    certify_loop(s, scenes_of("E4-rectangle"), SPLIT, SHAPES["E4-rectangle"][4], "E4-rectangle, RDA_LMZ_DENSE_FROM=0", after_call=after_call)
    print(f"rows on the work list per launch: {listed}")
    # (launch 1 enumerates all; the first launch of step 2 lists the slots whose supports the re-upload flushed; a row on the list of ANOTHER launch is
    # one whose remembered support failed its certificate and was then enumerated)
    assert len(listed) == 2 * ITERS and all(v >= 0 for v in listed) and listed[ITERS] >= 1 and max(listed[1:ITERS] + listed[ITERS + 1:]) >= 1, listed


def test_dense_fused_form(monkeypatch):
    monkeypatch.setenv("RDA_LMZ_DENSE_FROM", "0")
    monkeypatch.setenv("RDA_LMZ_SPLIT", "0")
    _run("E4-rectangle", DENSE, ", RDA_LMZ_DENSE_FROM=0 RDA_LMZ_SPLIT=0")


# ---- switches --------------------------------------------------------------------------------------------------------------------------------
def test_every_row_enumerated_in_every_launch(monkeypatch):
    """RDA_LMZ_WARM=0: no remembered support is tried.  Held to the certificate, not to the warm run."""
    monkeypatch.setenv("RDA_LMZ_WARM", "0")
    _run("E4-rectangle", ROWS, ", RDA_LMZ_WARM=0")


def test_max_clearance_duals_without_centring(monkeypatch):
    """RDA_TIE_CENTRE=0: every row is the optimum of f_delta (criterion A), none is centred"""
    monkeypatch.setenv("RDA_TIE_CENTRE", "0")
    w = _run("E4-rectangle", ROWS, ", RDA_TIE_CENTRE=0", tie_centre=0, classes=False)
    assert w.get("B", 0) == 0 and w["A"] == w["rows"] == 2 * ITERS * N * T


# ---- edges -----------------------------------------------------------------------------------------------------------------------------------
# the one-step scenes of the edge cases (scenes, seed); tests/test_lmz_rows_cert.py runs them on the oracle backend
EDGES = {"after-empty": ([_scene(4)], 50), "before-nan": ([_scene(4, moving=False, count=5)], 66), "nan": ([_scene(4, moving=False, count=5)], 76)}


def test_empty_obstacle_list_then_obstacles_again():
    """quirk Q9: no obstacle staged - finite controls, no failed row, the step stops after its first launch; then the same handle with obstacles"""
    s = make_solver("E4-rectangle")
    certify_loop(s, [[]], WAVE, 51, "E4-rectangle, empty list (Q9)", launches=1, classes=False)
    certify_loop(s, *EDGES["after-empty"][:1], ROWS, EDGES["after-empty"][1], "E4-rectangle, obstacles after an empty tick")


def broken_scene():
    """the scene of EDGES["before-nan"] with a NaN vertex in slot 1's polygon"""
    good = EDGES["before-nan"][0][0]

    def scene(nom_s):
        obs = good(nom_s)
        A = np.array(obs[1].A, float); A[0, 0] = np.nan
        return [obs[0], obs[1]._replace(A=A)] + list(obs[2:])
    return scene


@pytest.mark.parametrize("rows_kernel", [True, False])
def test_a_non_finite_slot_keeps_its_duals_and_the_others_certify(monkeypatch, rows_kernel):
    """step 1: a good scene (the slot gets duals); step 2: slot 1's polygon has a NaN vertex.  Its T rows keep lam, mu, z, xi, zeta bit for bit,
    lmz_fail counts exactly them, every other row still passes the certificate."""
    if not rows_kernel:
        monkeypatch.setenv("RDA_LMZ_ROWS", "0")
    form = ROWS if rows_kernel else WAVE
    s = make_solver("E4-rectangle")
    good = EDGES["before-nan"][0][0]
    certify_loop(s, [good], form, EDGES["before-nan"][1], "E4-rectangle, before the NaN")
    before = s.get_state()
    assert np.abs(before["lam"][1]).max() > 0 and np.abs(before["zeta"][1]).max() > 0
    w = certify_loop(s, [broken_scene()], form, EDGES["nan"][1], "E4-rectangle, slot 1 non-finite", skip=(1,), fails_per_call=T, corner=False)
    assert w["rows"] == ITERS * (N - 1) * T
    after = s.get_state()
    for key in ("lam", "mu", "z", "xi", "zeta"):
        assert np.array_equal(before[key][1], after[key][1]), key
    for key in ("lam", "xi", "zeta"):
        assert not np.array_equal(before[key][0], after[key][0]), key          # (the other slots went on)


# ---- the fleet forms -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,form", [({"RDA_LMZ_SPLIT": "0"}, "k_lammuz_fleet_rows"), ({}, "k_lammuz_fleet_rows_fast+k_lammuz_fleet_enum+k_lmz_finalize_fleet"),
                                      ({"RDA_LMZ_ROWS": "0"}, "k_lammuz_fleet+k_lmz_finalize_fleet")], ids=["rows", "split", "wave"])
def test_fleet_members_are_their_certified_solo_twins(monkeypatch, env, form):
    """the fleet launches run the solo kernels' bodies with the member in the grid: two members through `Fleet.control`, bit for bit their solo
    `MPC.control` (forms k_lammuz_rows and k_lammuz + k_lmz_finalize, certified row by row above), with the fleet's launch form named"""
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    car_t = sc.rectangle_robot(dynamics="acker")
    E = 4
    solo, memb, states, scenes = [], [], [], []
    for i in range(2):
        y = 20.0 + 6 * i
        path = sc.line_path([4, y, 0], [24, y, 0], 0.1)
        kw = dict(receding=T, iter_num=ITERS, max_edge_num=E, max_obs_num=N)
        solo.append(MPC(car_t, [p.copy() for p in path], **kw))
        memb.append(MPC(car_t, [p.copy() for p in path], **kw))
        states.append(path[0].copy().reshape(3, 1))
        scenes.append([sc.regular_polygon(9.0, y + 2.6, E, 1.2, 0.2), sc.regular_polygon(12.0, y - 2.8, 3, 1.0, 0.4), sc.circle(15.0, y + 3.0, 0.8, (0.0, -0.3))])
    assert solo[0].rda._be.api.lib.rda_lammuz_kernel(solo[0].rda._be.handle).decode() in (ROWS, WAVE)
    fleet = Fleet(memb)
    for k in range(2):
        res = fleet.control([s.copy() for s in states], 4.0, [list(sc_) for sc_ in scenes])
        assert fleet.lammuz_kernel() == form
        for i in range(2):
            u, info = solo[i].control(states[i].copy(), 4.0, list(scenes[i]))
            assert solo[i].rda._be.api.lib.rda_lammuz_kernel(solo[i].rda._be.handle).decode() == (WAVE if env.get("RDA_LMZ_ROWS") == "0" else ROWS)
            uf, inf = res[i]
            assert np.array_equal(u, uf), (k, i, np.abs(u - uf).max())
            assert (info["iters"], info["resi_dual"], info["lmz_fail"]) == (inf["iters"], inf["resi_dual"], inf["lmz_fail"]) and info["lmz_fail"] == 0
            assert np.array_equal(np.hstack(info["opt_state_list"]), np.hstack(inf["opt_state_list"]))
            sa, sb = solo[i].rda.get_state(), memb[i].rda.get_state()
            assert all(np.array_equal(sa[key], sb[key]) for key in sa), (k, i)
            states[i] = sc.kinematic_step(states[i], u, car_t, 0.1)
    fleet.close()
