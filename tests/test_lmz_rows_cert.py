"""CPU: the optimality certificate of the default LamMuZ mode (tests/lmz_rows_cert.py) pinned on answers derived by hand, then MEASURED on the two
oracles (oracle/lammuz_np.py, orc_lammuz_one) over the pinned grid of tests/test_lmz_central_ref.py - the recorded worst figures (lmz_rows_cert.
ORACLE_WORST) are what this file prints, and 10 x them is what the GPU kernels are held to (tests/test_gpu_lmz_rows_cert.py) - then shown to REJECT
wrong answers with a margin, and last run over the harness of the GPU test on the oracle backend: the rows of every LamMuZ call rebuilt from the
handle's state in the default mode, and the very scenes of the GPU cases with their class counts."""
import ctypes as C
import os

import numpy as np
import pytest

import lmz_central_ref as ref
import lmz_rows_cert as cert
import test_gpu_lmz_rows_cert as gpu_cases
from lmz_central_ref import LD
from oracle.oracle_backend import switches
from rda_planner_amd._capi import dptr, f64
from test_lmz_central_ref import GOLD, drive_rows, grid, recorded_steps

SQ = f64([[1, 0], [0, 1], [-1, 0], [0, -1]])          # the half-space normals of an axis-parallel rectangle: x <= b0, y <= b1, -x <= b2, -y <= b3
DELTA = LD(cert.DELTA)


def _row(A, b, p, xi=(0, 0), zeta=0.0, dbar=0.5, ro2=1.0, s=0.5, circ=0, accelerated=1):
    """a row with the square robot [-s, s]^2 at p, heading 0"""
    A = f64(A)
    return ref.Row(A.shape[0], 4, A, f64(b), circ, 0, f64(p), 0.0, SQ, f64([s] * 4), f64(xi), float(zeta), float(dbar), float(ro2), accelerated, 0.0)


# ---- answers derived by hand -----------------------------------------------------------------------------------------------------------------------
def test_known_answer_no_obstacle_and_robot_inside():
    """lam = mu = 0 is the optimum of an all-padding slot (grad_mu = delta h >= 0) and of a robot whose centre lies deep inside the obstacle with xi = 0
    (q < 0 and g_m < 0: grad_lam = g_m q > 0, grad_mu = -g_m h > 0).  For an obstacle that is merely FAR AWAY it is not: -delta m rewards every gain of m, and
    the certificate must say so."""
    zero = np.zeros(4)
    pad = _row(np.zeros((4, 2)), np.zeros(4), (0.3, -0.2), zeta=1.0, dbar=0.4)
    c = cert.certify(pad, zero, zero, 0.3)
    assert c.cls == "A" and c.fig["kkt"] == 0.0, c
    assert cert.certify(pad, zero, zero, 0.6).cls is None                      # (T2: z = 1/2 max(m, 0), m = 0.6)
    assert cert.certify(pad._replace(accelerated=0), zero, zero, 0.6).cls == "A"
    inside = _row(SQ, [5, 5, 5, 5], (0, 0), dbar=0.5)
    assert cert.certify(inside, zero, zero, 0.0).cls == "A"
    far = _row(SQ, [2, 1, 0, 1], (-30.0, 0), dbar=0.5)
    c = cert.certify(far, zero, zero, 0.0)
    assert c.cls is None and c.fig["kkt"] > 1e-7, c


def test_known_answer_one_edge_contact():
    """square obstacle [0, 2] x [-1, 1], robot centre D = 0.9 in front of the middle of its edge x = 0, dbar = 0.8: the hinge is active, lam = e_3 (|a| = 1
    binds), mu = gamma on the facing robot edge with  -g_m s + ro2 (gamma - 1) = 0,  g_m = D - gamma s - dbar - delta:
    gamma = (ro2 + s (D - dbar - delta)) / (s^2 + ro2)"""
    D, s, dbar = LD(0.9), LD(0.5), LD(0.8)
    for ro2 in (1.0, 5.0):
        row = _row(SQ, [2, 1, 0, 1], (-0.9, 0), dbar=0.8, ro2=ro2)
        gam = float((LD(ro2) + s * (D - dbar - DELTA)) / (s * s + LD(ro2)))
        lam, mu = np.array([0, 0, 1.0, 0]), np.array([gam, 0, 0, 0])
        c = cert.certify(row, lam, mu, 0.0)
        assert c.cls == "A" and c.fig["kkt"] <= 1e-16, c
        assert cert.certify(row, lam, mu * (1 + 1e-9), 0.0).cls is None
        assert cert.certify(row, lam * (1 - 1e-9), mu, 0.0).cls is None


def test_known_answer_vertex_vertex_contact_on_the_unit_circle():
    """obstacle [0, 2]^2, robot centre (-d, -d), d = 0.9, dbar = 1: the corners face each other along the diagonal; by symmetry lam_3 = lam_4 = l = 1 / sqrt 2
    (|a| = 1) and mu_1 = mu_2 = g with  -g_m s + ro2 (g - l) = 0,  g_m = 2 l d - 2 g s - dbar - delta:   g = (ro2 l + s (2 l d - dbar - delta)) / (2 s^2 + ro2);
    the multiplier of |a| <= 1 is nu = -sqrt 2 g_m (d - s) > 0"""
    d, s, dbar, l = LD(0.9), LD(0.5), LD(1.0), 1 / np.sqrt(LD(2))
    row = _row(SQ, [2, 2, 0, 0], (-0.9, -0.9), dbar=1.0)
    g = float((l + s * (2 * l * d - dbar - DELTA)) / (2 * s * s + 1))
    lam, mu = np.array([0, 0, float(l), float(l)]), np.array([g, g, 0, 0])
    c = cert.certify(row, lam, mu, 0.0)
    assert c.cls == "A" and c.fig["kkt"] <= 2e-16 and c.fig["feas"] <= 2.3e-16, c
    assert cert.certify(row, lam * (1 + 1e-9), mu, 0.0).cls is None            # (|a| > 1)
    assert cert.certify(row, lam, mu + 1e-9, 0.0).cls is None


def test_known_answer_circle_inside_the_unit_disc():
    """circle of radius r = 0.6 at the origin, robot centre D = 1 to its left (overlap: D - r - s < 0), xi = (0.3, 0), dbar = 0.5: a = (-alpha, 0), lam_2 = -alpha,
    mu = 0 (grad_mu = g_m (D - r - s) >= 0 on the facing edge), and  g_m (D - r) = ro2 (xi_x - alpha),  g_m = alpha (D - r) - dbar - delta:
    alpha = (ro2 xi_x + (dbar + delta) (D - r)) / ((D - r)^2 + ro2)  in (0, 1)"""
    gap, dbar, xi = LD(1.0) - LD(0.6), LD(0.5), LD(0.3)
    row = _row([[1, 0], [0, 1], [0, 0], [0, 0]], [0, 0, -0.6, 0], (-1.0, 0), xi=(0.3, 0), dbar=0.5, circ=1)
    al = float((xi + (dbar + DELTA) * gap) / (gap * gap + 1))
    assert 0.4 < al < 0.5
    lam = np.array([-al, 0, -al, 0])
    c = cert.certify(row, lam, np.zeros(4), 0.0)
    assert c.cls == "A" and c.fig["kkt"] <= 1e-16, c
    assert cert.certify(row, lam * (1 + 1e-9), np.zeros(4), 0.0).cls is None
    assert cert.certify(row, np.array([-al, 0, -al * (1 + 1e-9), 0]), np.zeros(4), 0.0).cls is None      # (off the cone's boundary)
    assert cert.certify(row, np.array([-al, 0, -al, 1e-300]), np.zeros(4), 0.0).cls is None             # (lam_3 .. are exactly 0)


def test_known_answer_slack_regime_with_a_closed_form_arc():
    """square robot (s = 0.5) at (-3, 0) facing the square obstacle [0, 2] x [-1, 1], dbar = 0.5: lam = e_3, mu = e_1 give H = 0, m = 3 - s - dbar = 2 and the
    normal (-1, 0), which is the middle of the arc by symmetry.  For a = -(cos t, sin t), t > 0, the binding pair is the obstacle's corner (0, -1) and the
    robot's corner (s, s):  m(t) = 2.5 cos t - 1.5 sin t - 0.5, zero at  t = acos(0.5 / sqrt 8.5) - atan2(1.5, 2.5)"""
    row = _row(SQ, [2, 1, 0, 1], (-3.0, 0), dbar=0.5)
    lam, mu = np.array([0, 0, 1.0, 0]), np.array([1.0, 0, 0, 0])
    want = float(np.arccos(LD(0.5) / np.sqrt(LD(8.5))) - np.arctan2(LD(1.5), LD(2.5)))
    up, down = cert.arc(row, np.pi)
    assert abs(up - want) <= 2e-15 and abs(down - want) <= 2e-15, (up, down, want)
    c = cert.certify(row, lam, mu, 1.0)
    assert c.cls == "B" and c.fig["H"] == 0.0 and c.fig["arc"] <= 2e-15, c
    assert cert.certify(row._replace(accelerated=0), lam, mu, 2.0).cls == "B"
    assert cert.certify(row, lam, mu, 2.0).cls is None                                                  # (T2)
    m, l2, m2 = cert.lp_duals(row, np.pi)
    assert abs(m - 2.0) <= 1e-15 and np.array_equal(l2, lam) and np.array_equal(m2, mu)
    m, l2, m2 = cert.lp_duals(row, np.pi + 1e-6)                                                        # another separating normal: optimal, not the middle
    c = cert.certify(row, l2, m2, 0.5 * m)
    assert c.cls is None and "half-widths" in c.why, c
    assert cert.arc(row, 0.0) == "m < 0 at the normal"


# ---- the two oracles on the pinned grid ------------------------------------------------------------------------------------------------------------
def c_oracle(L, row, delta=cert.DELTA):
    lam, mu, zz, cmh = np.zeros(row.E), np.zeros(row.R), C.c_double(0), np.zeros(4)
    L.orc_lammuz_one(row.E, row.R, dptr(row.A), dptr(row.b), row.cone_norm2, dptr(row.p), row.phi, dptr(row.G), dptr(row.h), dptr(row.xi), row.zeta, row.dbar,
                     row.ro2, delta, row.accelerated, dptr(lam), dptr(mu), C.cast(C.byref(zz), C.POINTER(C.c_double)), dptr(cmh))
    return lam, mu, zz.value


def np_oracle(row, **kw):
    from oracle.lammuz_np import solve_lammuz
    lam, mu, z, info = solve_lammuz(row.A, row.b, bool(row.cone_norm2), row.p, row.phi, row.G, row.h, row.xi, row.zeta, row.dbar, row.ro2,
                                    accelerated=bool(row.accelerated), **kw)
    return lam, mu, z, info


def polygon_robot_grid(accelerated):
    """the rows of the pinned grid with a polygon robot (the default mode has no circle robot): E in {3, 4, 5, 6, 8} x rectangle / triangle / octagon x
    ro2 in {1, 5} x {triangle, full E-gon, between, circle} x 2 draws = 240 rows"""
    return [(label, row) for label, row in grid(accelerated, 0.0) if not row.robot_norm2]


@pytest.mark.parametrize("accelerated", [1, 0])
def test_oracle_figures_on_the_pinned_grid(orc, accelerated):
    """every row of the grid, answered by the C oracle and by the numpy oracle, passes the
    certificate; the worst figures are printed and held to the recorded ones.  The arc is located on every class-B row of E in {3, 5, 8} of the C oracle in
    the accelerated run (lam and mu of a row do not depend on `accelerated`, only z does)."""
    rows = polygon_robot_grid(accelerated)
    assert len(rows) == 240
    worst, count = {}, {"A": 0, "B": 0}
    for label, row in rows:
        answers = [("c", c_oracle(orc.lib, row))]
        lam, mu, z, info = np_oracle(row)
        answers.append(("numpy", (lam, mu, z)))
        for who, (lam, mu, z) in answers:
            c = cert.certify(row, lam, mu, z, with_arc=(who == "c" and accelerated == 1 and row.E in (3, 5, 8)))
            assert c.cls is not None, (who, label, c.why)
            assert not (c.cls == "A" and c.trigger), (who, label)            # (on this grid no arc of a triggered row is improper)
            if who == "numpy":
                assert (c.cls == "B") == info["central"], (label, c.cls)
            else:
                count[c.cls] += 1
            for key, v in c.fig.items():
                if v >= worst.get(key, (0.0, ""))[0]:
                    worst[key] = (v, f"{who} {label}")
    print(f"\noracles on the pinned grid, accelerated={accelerated}: {count['A']} class A, {count['B']} class B; worst figures: "
          + "; ".join(f"{k} {v:.3g} [{w}]" for k, (v, w) in sorted(worst.items())))
    assert count == {"A": 103, "B": 137}
    assert worst["m_neg"][0] == 0.0
    assert ("arc" in worst) == bool(accelerated)
    for key, rec in cert.ORACLE_WORST.items():
        assert key not in worst or worst[key][0] <= rec, (key, worst[key], rec)


# ---- wrong answers ---------------------------------------------------------------------------------------------------------------------------------
MOVED = 1e-12


def _moved(x, y):
    return max(np.abs(x[0] - y[0]).max(), np.abs(x[1] - y[1]).max(), abs(x[2] - y[2])) > MOVED


def test_wrong_answers_are_rejected_with_a_margin(orc):
    """five kinds of wrong answers on the accelerated grid, each certified against the ORIGINAL row.  Of the rows whose (lam, mu, z) moved by more than 1e-12
    at least 90 % must be rejected per kind, and the rejected ones lie >= 5 x outside a bound (lmz_rows_cert.margin: the figure in units of its bound)."""
    L = orc.lib
    rows = polygon_robot_grid(1)
    right = [c_oracle(L, row) for _, row in rows]
    cls = [cert.certify(row, *ans, with_arc=False).cls for (_, row), ans in zip(rows, right)]
    assert None not in cls
    kinds = {}

    def tried(kind, row, ans, wrong):
        if _moved(ans, wrong):
            kinds.setdefault(kind, []).append(cert.margin(row, *wrong))

    with switches(tie_centre=0):
        uncentred = [c_oracle(L, row) for _, row in rows]
    for k, ((label, row), ans) in enumerate(zip(rows, right)):
        tried("the optimum of the row with xi + 1e-8", row, ans, c_oracle(L, row._replace(xi=row.xi + 1e-8)))
        tried("the delta = 0 optimum", row, ans, c_oracle(L, row, delta=0.0))
        if cls[k] == "B":
            if k % 6 == 1:
                tried("the un-centred answer of a centred row", row, ans, uncentred[k])
            if k % 6 == 0:
                a = row.A.T @ ans[0]
                m, lam, mu = cert.lp_duals(row, np.arctan2(a[1], a[0]) + 1e-6)
                tried("a centred normal rotated by 1e-6 rad", row, ans, (lam, mu, 0.5 * m))
        m = float(cert._point(row, ans[0], ans[1])[-3])
        tried("z = max(m, 0) in accelerated mode", row, ans, (ans[0], ans[1], max(m, 0.0)))
    assert len(kinds) == 5
    for kind, margins in kinds.items():
        margins = np.array(margins)
        out = margins[margins > 1]
        print(f"\n{kind}: {len(margins)} rows moved, {len(out)} rejected, the nearest of them {out.min():.3g} x its bound"
              + (f"; passed: {np.sort(margins[margins <= 1])}" if len(out) < len(margins) else ""))
        assert len(margins) >= 20, (kind, len(margins))
        assert len(out) >= 0.9 * len(margins), (kind, len(out), len(margins))
        assert out.min() >= 5.0, (kind, out.min())


# ---- the harness of the GPU test, on the oracle backend in the default mode ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "c4"])
def test_rows_rebuilt_from_the_handle_state_certify_in_the_default_mode(orc, name):
    """scenes c1 (static) and c4 (moving: per-stage slots) of ref_plumbing, 3 steps, the oracle backend in its default LamMuZ mode: every rebuilt row
    passes the certificate and the epilogue identities - the rebuild (which xi, zeta, dis, state column and obstacle slot a row reads) is the one the GPU
    test relies on.  Both recorded scenes keep the robot clear of every obstacle: all their rows (660 and 1 008) are in the slack regime, class B.  Rows of
    class A are rebuilt and certified by test_scenes_of_the_gpu_cases_on_the_oracle_backend below (>= 20 per scene)."""
    from oracle.oracle_backend import oracle_backend
    from rda_planner_amd.rda_solver import RDA_solver
    from test_ref_golden import _car
    g = np.load(os.path.join(GOLD, "ref_plumbing.npz"))
    T, N, E, iter_num, ro1, dyn = (int(v) if i != 4 else float(v) for i, v in enumerate(g[f"{name}.cfg"]))
    s = RDA_solver(T, _car(dyn), E, N, iter_num=iter_num, time_print=False, ro1=ro1, _backend=oracle_backend)
    worst = {}

    def on_call(k, it, rows, inf, out_u):
        assert inf.lmz_fail == 0
        cert.check_rows(rows, f"{name} step {k} it {it}", worst)
    drive_rows(s, recorded_steps(name, 3), 0.0, on_call)
    cert.check_arcs(worst, ORACLE_ARCS)
    print(f"\n{name}, oracle backend, default mode, rows rebuilt from the handle state: {cert.figures(worst)}")
    assert not worst["bad"], worst["bad"][:5]
    assert worst["rows"] >= 100 and worst.get("A", 0) + worst.get("B", 0) == worst["rows"] and worst.get("B", 0) >= 100


MIN_PER_CLASS_ON_THE_ORACLE = 20
ORACLE_ARCS = 8          # class-B rows per loop whose arc is located here (the GPU cases: 24); the oracle's arcs are measured on the grid above


@pytest.mark.parametrize("shape", list(gpu_cases.SHAPES))
def test_scenes_of_the_gpu_cases_on_the_oracle_backend(shape):
    """the loops of tests/test_gpu_lmz_rows_cert.py on the oracle backend: every row certifies and each class has >= 20 rows (the GPU cases ask for 10)"""
    from oracle.oracle_backend import oracle_backend
    s = gpu_cases.make_solver(shape, _backend=oracle_backend)
    w = gpu_cases.certify_loop(s, gpu_cases.scenes_of(shape), None, gpu_cases.SHAPES[shape][4], shape, arcs=ORACLE_ARCS)
    assert w["A"] >= MIN_PER_CLASS_ON_THE_ORACLE and w["B"] >= MIN_PER_CLASS_ON_THE_ORACLE, (w["A"], w["B"])
    assert w["A_poly_unit"] >= 2 * gpu_cases.MIN_POLYGON_UNIT and w["A_poly_mu2"] >= 2 * gpu_cases.MIN_CORNER, (w["A_poly_unit"], w["A_poly_mu2"])


def test_edge_scenes_of_the_gpu_cases_on_the_oracle_backend():
    """the one-step scenes of the edge cases: after an empty tick; before the NaN and, on the same handle, with slot 1 non-finite"""
    from oracle.oracle_backend import oracle_backend
    T = gpu_cases.T
    s = gpu_cases.make_solver("E4-rectangle", _backend=oracle_backend)
    gpu_cases.certify_loop(s, [[]], None, 51, "empty list", launches=1, classes=False, arcs=ORACLE_ARCS)
    scenes, seed = gpu_cases.EDGES["after-empty"]
    ws = [gpu_cases.certify_loop(s, scenes, None, seed, "after an empty tick", arcs=ORACLE_ARCS)]
    s = gpu_cases.make_solver("E4-rectangle", _backend=oracle_backend)
    scenes, seed = gpu_cases.EDGES["before-nan"]
    ws.append(gpu_cases.certify_loop(s, scenes, None, seed, "before the NaN", arcs=ORACLE_ARCS))
    ws.append(gpu_cases.certify_loop(s, [gpu_cases.broken_scene()], None, gpu_cases.EDGES["nan"][1], "slot 1 non-finite", skip=(1,), fails_per_call=T, arcs=ORACLE_ARCS, corner=False))
    assert all(w["A"] >= MIN_PER_CLASS_ON_THE_ORACLE and w["B"] >= MIN_PER_CLASS_ON_THE_ORACLE for w in ws), [(w["A"], w["B"]) for w in ws]
    assert all(w["A_poly_unit"] >= 2 * gpu_cases.MIN_POLYGON_UNIT for w in ws) and all(w["A_poly_mu2"] >= 2 * gpu_cases.MIN_CORNER for w in ws[:2]), ws


def test_no_row_is_centred_with_the_tie_break_off(orc):
    """tie_centre = 0, the oracle's RDA_TIE_CENTRE=0: every row of the E = 4 scene meets criterion A"""
    from oracle.oracle_backend import oracle_backend
    with switches(tie_centre=0):
        s = gpu_cases.make_solver("E4-rectangle", _backend=oracle_backend)
        w = gpu_cases.certify_loop(s, gpu_cases.scenes_of("E4-rectangle"), None, gpu_cases.SHAPES["E4-rectangle"][4], "tie_centre = 0", tie_centre=0, classes=False)
    assert w.get("B", 0) == 0 and w["A"] == w["rows"]
