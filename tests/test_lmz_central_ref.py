"""CPU: the independent reference of the interior-point LamMuZ mode (tests/lmz_central_ref.py: a damped Newton on the log-barrier
problem, refined and certified in extended precision) pinned on hand-derived answers, then the oracle's interior-point restatement
(oracle/lmz_ipm.c) and the host instantiation of the row-parallel kernel's template (tests/emu/rip_emu.cpp) against it on one
pinned grid of rows.  No row may fail: the reference certifies every row of the grid, so a status 2 of either solver fails the
test.  Last, the harness of tests/test_gpu_central_rows.py - the rows of every LamMuZ call of a driven loop rebuilt from the
handle's state (`rows_from_state`) - is checked on the oracle backend, with the epilogue identities.

Bounds.  The oracle is held to its RECORDED worst deviation per class (accelerated, mu*) (lmz_central_ref.ORACLE_WORST; a larger
value means that the oracle or the reference changed: look, then record).  The emulation - the kernel's arithmetic - is held to
10 x that (lmz_central_ref.gpu_bound), the bound of the GPU tests: never a number taken from the kernel."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as hp
import lmz_central_ref as ref
from oracle.oracle_backend import switches
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import Info, c_double_p, c_int_p, dptr, iptr, f64
from test_ip_rows_emu import emu          # noqa: F401  (the fixture that builds tests/emu/rip_emu.cpp)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CLASSES = [(1, 1e-3), (1, 1e-6), (0, 1e-3), (0, 1e-6)]


# ---- the reference itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,w,mu", [(0.7, 1, 1e-3), (-0.4, 1, 1e-3), (0.0, 5, 1e-6), (2.0, 8, 1e-2)])
def test_known_answer_one_lp_row(c, w, mu):
    """min 1/2 x^2 - c x - mu w log x  (one LP row x >= 0 written w times):  x^2 - c x - mu w = 0,  x = (c + sqrt(c^2 + 4 mu w)) / 2"""
    prob = ref.Problem([[1.0]], [-c], [[-1.0]], [0.0], [w], [])
    x, res, step = ref.central_point(prob, mu, np.array([1.0]))
    want = (ref.LD(c) + np.sqrt(ref.LD(c) ** 2 + 4 * ref.LD(mu) * w)) / 2
    assert abs(float(x[0]) - float(want)) <= 1e-15 * max(1.0, float(want)) and res <= ref.GRAD_TOL


def test_known_answer_interval():
    """min c x - mu log x - mu log(1 - x): c x (1 - x) - mu (1 - 2x) = 0, the root in (0, 1)"""
    c, mu = 0.3, 1e-3
    prob = ref.Problem([[0.0]], [c], [[-1.0], [1.0]], [0.0, 1.0], [1, 1], [])
    x, _, _ = ref.central_point(prob, mu, np.array([0.5]))
    want = ((c + 2 * mu) - np.sqrt((c + 2 * mu) ** 2 - 4 * c * mu)) / (2 * c)      # c x^2 - (c + 2 mu) x + mu = 0
    assert abs(float(x[0]) - want) <= 1e-15


@pytest.mark.parametrize("d", [(0.0, 0.0), (0.3, -0.4), (0.9, 0.1)])
def test_known_answer_one_second_order_cone(d):
    """min c t + d'u - mu/2 log(t^2 - |u|^2), (t ; u) in Q^3, c > |d|:  c = mu t / det, d = -mu u / det  =>  det = mu^2 / (c^2 - |d|^2),
    t = c mu / (c^2 - |d|^2), u = -d mu / (c^2 - |d|^2).  (A barrier weight mu instead of mu / 2 doubles t.)"""
    c, mu, d = 1.5, 1e-3, np.array(d)
    prob = ref.Problem(np.zeros((3, 3)), np.r_[c, d], np.zeros((0, 3)), [], [], [(-np.eye(3), np.zeros(3))])
    x, res, _ = ref.central_point(prob, mu, np.array([1.0, 0.0, 0.0]))
    k = mu / (c * c - d @ d)
    assert np.abs(x.astype(float) - np.r_[c * k, -d * k]).max() <= 1e-15 and res <= ref.GRAD_TOL


def test_an_infeasible_start_or_an_unreachable_certificate_raises():
    prob = ref.Problem([[1.0]], [0.0], [[-1.0]], [0.0], [1], [])
    with pytest.raises(ref.NotCertified):
        ref.central_point(prob, 1e-3, np.array([-1.0]))


# ---- the pinned grid ------------------------------------------------------------------------------------------------------------
def _robots():
    tri = sc.polygon_halfspaces(np.array([[1.5, -1.0, -1.0], [0.0, 0.9, -0.9]]))
    ang = 2 * np.pi * np.arange(8) / 8
    octo = sc.polygon_halfspaces(np.vstack((1.2 * np.cos(ang), 0.8 * np.sin(ang))))
    return {"rectangle": (hp.G, hp.H, 0), "triangle": (f64(tri[0]), f64(tri[1]).ravel(), 0), "octagon": (f64(octo[0]), f64(octo[1]).ravel(), 0),
            "circle": (f64([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]), f64([0.0, 0.0, -0.8]), 1)}


ROBOTS = _robots()


def make_row(rng, E, robot, circ, k, accelerated, mu, ro2):
    """one row: the generator of test_ip_rows_emu._case with the edge count k of a polygon given (rows k .. E-1 zero-padded)"""
    G, h, rn2 = ROBOTS[robot]
    p = rng.uniform(-5, 5, 2)
    phi = rng.uniform(-np.pi, np.pi)
    dist = rng.choice([0.5, 1.5, 3.0, 6.0, 15.0])
    th = rng.uniform(0, 2 * np.pi)
    cen = p + dist * np.array([np.cos(th), np.sin(th)])
    if circ:
        A = np.zeros((E, 2)); A[0] = [1, 0]; A[1] = [0, 1]
        b = np.zeros(E); b[0:2] = cen; b[2] = -rng.uniform(0.3, 1.5)
    else:
        A, b = hp.random_polygon(rng, cen, k, rng.uniform(0.4, 2.0), E)
    return ref.Row(E, G.shape[0], f64(A), f64(b), int(circ), rn2, f64(p), float(phi), G, h, f64(rng.normal(0, 0.3, 2)), float(rng.normal(0, 0.5)),
                   float(rng.uniform(0.1, 1.0)), float(ro2), int(accelerated), float(mu))


def grid(accelerated, mu, edges=(3, 4, 5, 6, 8)):
    """E x robot x ro2 x {triangle (padded rows), full E-gon, something between, circle} x 2 draws"""
    out = []
    for E in edges:
        for ir, robot in enumerate(ROBOTS):
            for ro2 in (1.0, 5.0):
                rng = np.random.default_rng(1000 * E + 10 * ir + int(ro2))
                for draw in range(2):
                    for kind, k in (("tri", 3), ("full", E), ("mid", (3 + E) // 2), ("circle", 0)):
                        out.append((f"E{E} {robot} ro2={ro2:g} {kind} #{draw}", make_row(rng, E, robot, kind == "circle", k, accelerated, mu, ro2)))
    return out


def oracle_row(L, row):
    """orc_lammuz_ipm_one on a row -> (status, lam, mu, z); the caller runs it inside switches(lmz_mu=row.mu_star)"""
    lo, mo, zo, cmh, it = np.zeros(row.E), np.zeros(row.R), C.c_double(0), np.zeros(4), C.c_int(0)
    st = L.orc_lammuz_ipm_one(row.E, row.R, dptr(row.A), dptr(row.b), row.cone_norm2, row.robot_norm2, dptr(row.p), row.phi, dptr(row.G), dptr(row.h),
                              dptr(row.xi), row.zeta, row.dbar, row.ro2, row.accelerated, dptr(lo), dptr(mo), C.cast(C.byref(zo), c_double_p), dptr(cmh),
                              C.cast(C.byref(it), c_int_p))
    return st, lo, mo, zo.value


def emu_row(emu, row, state=None, warm=0):
    """rip_emu_solve on a row -> (status, lam, mu, z, iterations); `state` [80] is read when warm and written on success"""
    le, me, ze, it = np.zeros(row.E), np.zeros(row.R), C.c_double(0), C.c_int(0)
    st = emu.rip_emu_solve(row.E, row.R, dptr(row.A), dptr(row.b), row.cone_norm2, row.robot_norm2, dptr(row.p), row.phi, dptr(row.G), dptr(row.h),
                           dptr(row.xi), row.zeta, row.dbar, row.ro2, row.accelerated, row.mu_star, dptr(le), dptr(me), C.cast(C.byref(ze), c_double_p),
                           None, dptr(state) if state is not None else None, int(warm), C.cast(C.byref(it), c_int_p))
    return st, le, me, ze.value, it.value


def _fits(emu, row):
    """rip::fits of the row's shape (five ints in, an int out: the ctypes defaults)"""
    return bool(emu.rip_emu_fits(row.E, row.R, row.cone_norm2, row.robot_norm2, row.accelerated))


@pytest.mark.parametrize("accelerated,mu", CLASSES)
def test_oracle_equals_the_reference_on_the_pinned_grid(orc, accelerated, mu):
    L = orc.lib
    worst, where, res, step = 0.0, None, 0.0, 0.0
    with switches(lmz_mu=mu):
        rows = grid(accelerated, mu)
        for label, row in rows:
            want = ref.solve_row(row)                 # (raises when it cannot certify the row)
            st, lo, mo, zo = oracle_row(L, row)
            assert st == 0, (label, st)               # allowed share of failed rows: 0
            dev = ref.deviation(want, lo, mo, zo)
            if dev > worst:
                worst, where = dev, label
            res, step = max(res, want.grad_res), max(step, want.step)
    print(f"oracle vs reference, accelerated={accelerated} mu*={mu:g}: {len(rows)} rows, worst deviation {worst:.2e} at [{where}]; "
          f"reference certificate: gradient <= {res:.1e}, Newton step at the point / (1 + |x|) <= {step:.1e}")
    assert worst <= ref.ORACLE_WORST[(accelerated, mu)], (worst, where)


@pytest.mark.parametrize("accelerated,mu", CLASSES)
def test_kernel_template_equals_the_reference_on_the_pinned_grid(emu, accelerated, mu):
    """the host instantiation of the row-parallel kernel's template wherever the row fits its 16 lanes, E = 7 included, cold"""
    worst, where, n = 0.0, None, 0
    for label, row in grid(accelerated, mu, edges=(3, 4, 5, 6, 7, 8)):
        if not _fits(emu, row):
            continue
        st, le, me, ze, _ = emu_row(emu, row)
        assert st == 0, (label, st)
        dev = ref.deviation(ref.solve_row(row), le, me, ze)
        n += 1
        if dev > worst:
            worst, where = dev, label
    print(f"kernel template vs reference, accelerated={accelerated} mu*={mu:g}: {n} rows, worst deviation {worst:.2e} at [{where}]")
    assert n >= 200
    assert worst <= ref.gpu_bound(accelerated, mu), (worst, where)


@pytest.mark.parametrize("accelerated,mu", CLASSES)
def test_kernel_template_warm_starts_end_on_the_reference_point(emu, accelerated, mu):
    """the warm path (`state` / `warm`): the next solve of a slot starts from its kept point.  A near successor (the next ADMM iteration), a far
    one, and a kept point that belongs to an obstacle of ANOTHER kind (the list is re-ordered every tick: a padded triangle where an E-gon was, a
    circle where a polygon was, and back) - each must meet the reference's point of the problem that is solved, like a cold solve"""
    worst, where, n = 0.0, None, 0
    for E in (4, 5, 7):
        for robot in ("rectangle", "circle"):
            rng = np.random.default_rng(77 + E)
            kinds = (("tri", 3), ("full", E), ("circle", 0))
            for trial in range(12):
                kind, k = kinds[trial % 3]
                row = make_row(rng, E, robot, kind == "circle", k, accelerated, mu, 1.0)
                if not _fits(emu, row):
                    continue
                state = np.zeros(80)
                st, *_ = emu_row(emu, row, state, 0)
                assert st == 0, (E, robot, trial, st)
                succ = []
                for far in (1.0, 20.0):
                    succ.append((f"successor x{far:g}", row._replace(p=f64(row.p + far * rng.normal(0, 0.03, 2)), phi=row.phi + far * rng.normal(0, 0.01),
                                                                      xi=f64(row.xi + far * rng.normal(0, 0.02, 2)), zeta=row.zeta + far * rng.normal(0, 0.05))))
                okind, ok_ = kinds[(trial + 1 + trial // 3) % 3]
                other = make_row(rng, E, robot, okind == "circle", ok_, accelerated, mu, 1.0)
                succ.append((f"{kind} -> {okind}", other._replace(p=row.p, phi=row.phi, xi=row.xi, zeta=row.zeta, dbar=row.dbar)))
                for label, nxt in succ:
                    st, le, me, ze, _ = emu_row(emu, nxt, state.copy(), 1)
                    assert st == 0, (E, robot, trial, label, st)
                    dev = ref.deviation(ref.solve_row(nxt), le, me, ze)
                    n += 1
                    if dev > worst:
                        worst, where = dev, f"E{E} {robot} #{trial} {label}"
    print(f"kernel template, warm, vs reference, accelerated={accelerated} mu*={mu:g}: {n} rows, worst deviation {worst:.2e} at [{where}]")
    assert n >= 100
    assert worst <= ref.gpu_bound(accelerated, mu), (worst, where)


def test_scaling_the_half_spaces_leaves_a_and_z_unchanged():
    """(A, b) -> (diag(c) A, diag(c) b), c > 0, describes the same obstacle: lam -> lam / c, so a = A'lam, z and mu stay (a circle obstacle's three
    rows share one factor: its cone couples them).  A reference that weighted a row wrongly would not have this symmetry."""
    rng = np.random.default_rng(4)
    worst = 0.0
    for trial in range(24):
        circ = trial % 3 == 2
        E = (4, 5, 6)[trial % 3]
        row = make_row(rng, E, ("rectangle", "circle")[trial % 2], circ, 3 + trial % (E - 2), trial % 2, (1e-3, 1e-6)[(trial // 2) % 2], 1.0)
        c = np.full(E, rng.uniform(0.05, 30.0)) if circ else rng.uniform(0.05, 30.0, E)
        a0, a1 = ref.solve_row(row), ref.solve_row(row._replace(A=f64(row.A * c[:, None]), b=f64(row.b * c)))
        d = max(np.abs(row.A.T @ a0.lam - (row.A * c[:, None]).T @ a1.lam).max(), abs(a0.z - a1.z), np.abs(a0.mu - a1.mu).max(), np.abs(a0.lam - a1.lam * c).max())
        worst = max(worst, d / (1 + max(np.abs(a0.lam).max(), np.abs(a0.mu).max(), abs(a0.z))))
    print(f"scale invariance of the reference: worst relative change {worst:.1e}")
    assert worst <= 4 * ref.STEP_TOL_FLAT          # (two certified centres of the same problem, some of them not accelerated)


# ---- the harness of the GPU test, on the oracle backend -------------------------------------------------------------------------
def recorded_steps(name, steps):
    """the inputs of the first `steps` MPC steps of ref_plumbing scene `name`"""
    g = np.load(os.path.join(GOLD, "ref_plumbing.npz"))
    for k in range(steps):
        pre = f"{name}.{k}"
        yield dict(n_obs=int(g[f"{pre}.n_obs"]), per_t=int(g[f"{pre}.per_t"]), A=f64(g[f"{pre}.A"]), b=f64(g[f"{pre}.b"]),
                   cone=np.ascontiguousarray(g[f"{pre}.cone"], np.int32), nom_s=f64(g[f"{pre}.nom_s"]), nom_u=f64(g[f"{pre}.nom_u"]), ref=f64(g[f"{pre}.ref"]),
                   speed=float(g[f"{pre}.speed"]))


def drive_rows(solver, steps, mu_star, on_call, before_call=None):
    """MPC steps (dicts as `recorded_steps` yields them) through upload_obstacles + admm_begin / su / lammuz / finish, as rda_step runs them;
    on_call(k, it, rows, info, out_u) after every LamMuZ call with its rows rebuilt from the handle's state before and after it
    (lmz_central_ref.rows_from_state); before_call(k, it) just before the call.  Returns the number of LamMuZ calls."""
    api, hd = solver._be.api, solver._be.handle
    T, G, h = solver.T, f64(solver.car_tuple.G), f64(solver.car_tuple.h).ravel()
    calls = 0
    for k, sp in enumerate(steps):
        if sp["n_obs"]:
            assert api.upload_obstacles(hd, sp["n_obs"], dptr(sp["A"]), dptr(sp["b"]), iptr(sp["cone"]), sp["per_t"]) == 0
        else:
            assert api.upload_obstacles(hd, 0, None, None, None, 0) == 0
        assert api.admm_begin(hd, dptr(sp["nom_s"]), dptr(sp["nom_u"]), dptr(sp["ref"]), sp["speed"]) == 0
        out_u, out_s = np.zeros((2, T)), np.zeros((3, T + 1))
        for it in range(solver.iter_num):
            stopped = C.c_int(0)
            assert api.admm_su(hd, it, C.byref(stopped)) == 0
            if stopped.value:
                break
            if before_call is not None:
                before_call(k, it)
            st0 = solver.get_state()
            assert api.admm_lammuz(hd) == 0
            inf = Info()
            assert api.admm_finish(hd, dptr(out_u), dptr(out_s), C.byref(inf)) == 0
            rows = ref.rows_from_state(st0, solver.get_state(), out_s, sp["A"], sp["b"], sp["cone"], sp["per_t"], G, h, solver._cfg, mu_star) if sp["n_obs"] else []
            on_call(k, it, rows, inf, out_u.copy())
            calls += 1
    return calls


def check_rows(rows, bound, tag, worst, skip=()):
    """every row against the reference and its epilogue identities.  worst[...] collects the figures and worst["bad"] the rows outside a bound, for the
    caller to print and then assert empty; rows whose slot n is in `skip` are left out"""
    bad = worst.setdefault("bad", [])
    for sr in rows:
        if sr.n in skip:
            continue
        dev = ref.deviation(ref.solve_row(sr.row), sr.lam, sr.mu, sr.z)
        e_xi, b_xi, e_ze, b_ze, e_c, b_c = ref.epilogue_errors(sr)
        worst["dev"] = max(worst.get("dev", 0.0), dev)
        for key, e, b in (("xi", e_xi, b_xi), ("zeta", e_ze, b_ze), ("cond", e_c, b_c)):
            worst[key] = max(worst.get(key, 0.0), e / b if b else e)
        worst["rows"] = worst.get("rows", 0) + 1
        if not (dev <= bound and e_xi <= b_xi and e_ze <= b_ze and e_c <= b_c):
            bad.append((tag, sr.n, sr.t, f"dev {dev:.2e} / {bound:.1e}", f"xi {e_xi:.1e} / {b_xi:.1e}", f"zeta {e_ze:.1e} / {b_ze:.1e}", f"condensed {e_c:.1e} / {b_c:.1e}"))


def figures(worst):
    return (f"{worst.get('rows', 0)} rows, worst deviation {worst.get('dev', 0.0):.2e}; epilogue errors in units of their bound ({ref.EPILOGUE_ULPS} ulp of the "
            f"summed terms): xi {worst.get('xi', 0.0):.2f}, zeta {worst.get('zeta', 0.0):.2f}, condensed A'lam / lam'b {worst.get('cond', 0.0):.2f}")


@pytest.mark.parametrize("name", ["c1", "c4"])
def test_rows_rebuilt_from_the_handle_state_are_what_the_oracle_solved(orc, name):
    """oracle backend in `lmz` mode 1 (its LamMuZ step is orc_lammuz_ipm_one per row): scenes c1 (static) and c4 (moving: per-stage slots) of
    ref_plumbing, 3 steps.  Every rebuilt row's duals meet the reference within the class bound and both epilogue identities hold to rounding
    level - the rebuild (which xi, zeta, dis, state column and obstacle slot a row reads) is the one the GPU test relies on."""
    from oracle.oracle_backend import oracle_backend
    from rda_planner_amd.rda_solver import RDA_solver
    from test_ref_golden import _car
    mu = 1e-3
    g = np.load(os.path.join(GOLD, "ref_plumbing.npz"))
    T, N, E, iter_num, ro1, dyn = (int(v) if i != 4 else float(v) for i, v in enumerate(g[f"{name}.cfg"]))
    worst = {}
    with switches(lmz_mode=1, lmz_mu=mu):
        s = RDA_solver(T, _car(dyn), E, N, iter_num=iter_num, time_print=False, ro1=ro1, _backend=oracle_backend)
        bound = ref.gpu_bound(s._cfg.accelerated, mu)

        def on_call(k, it, rows, inf, out_u):
            assert inf.lmz_fail == 0
            check_rows(rows, bound, f"{name} step {k} it {it}", worst)
        drive_rows(s, recorded_steps(name, 3), mu, on_call)
    print(f"{name}, oracle backend, rows rebuilt from the handle state: {figures(worst)} (bound on the deviation {bound:.1e})")
    assert not worst["bad"], worst["bad"][:5]
    assert worst["rows"] >= 100
