"""CPU: the su-problem against an independent certified optimum (tests/su_kkt.py: KKT system of the reference's uncondensed formulation, refined
in double-double arithmetic, accepted only on its certificate).  First the reference solver itself (known answers, scipy, the problems the
UNMODIFIED reference built), then the oracle's landed cold solve on a grid, the recorded hard problems and edge generators, at TOL_U_FIXED, and
the su-problems of an oracle closed loop rebuilt from the handle's state."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import helpers as hp
import su_kkt
from oracle.oracle_backend import su_dump
from rda_planner_amd._capi import Info, dptr, iptr, f64

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DYN = ("acker", "diff", "omni")
GRID_T = (1, 2, 3, 10, 20, 25, 30, 33, 40, 64)
GRID_N = (0, 1, 24, 200)
# the landed answer of this recorded problem is 1.35e-7 from the certified optimum on the oracle (the landing's stationarity stop, tests/helpers.py)
JUST_ACTIVE_FIXTURE = "diff_T20_N24_just_active_hinges"


def check_against(cert, s, u, d, tol, what=""):
    """distance of a candidate to the certified optimum; where the optimum is nearly non-unique (m < M_SINGULAR) the objective gap and the
    distance bound of the certificate instead"""
    dist = cert.distance(s, u, d)
    if cert.unique:
        assert dist <= tol, (what, dist, cert.m)
        return dist
    gap, viol = cert.gap(u, d)
    print(f"{what}: nearly singular (m = {cert.m:.1e}): |x - x*| {dist:.1e}, f(x) - f(x*) {gap:.1e}, bound {cert.bound(u, d):.1e}, bound violation {viol:.1e}")
    assert gap <= 1e-13 * (1 + abs(cert.f_star[0])) and viol <= 1e-12, (what, gap, viol)
    return dist


# ---- the reference solver itself ---------------------------------------------------------------------------------------------------------------
def _kwcase(T, N, **kw):
    cfg = hp.make_cfg(T=T, N=N, **kw)
    nom_s = np.zeros((3, T + 1))
    si = dict(nom_s=nom_s, nom_u=np.zeros((2, T)), ref=np.zeros((3, T + 1)), vref=0.0, a=np.zeros((N, T, 2)), cc=np.zeros((N, T)),
              g=np.zeros((N, T, 2)), d0=np.ones(T))
    return cfg, si


def test_known_answer_speed_on_its_bound():
    """T = 1, N = 0, vref above max_speed, no tracking: wu (u - vref)^2 + eps_u / 2 |u|^2 is smallest at the bound; d = max_sd (no obstacle term)"""
    cfg, si = _kwcase(1, 0, ws=0.0)
    si["vref"] = 14.0
    c = su_kkt.certify(cfg, si)
    assert c.u[0, 0] == pytest.approx(10.0, abs=1e-15) and abs(c.u[1, 0]) <= 1e-15 and c.d[0] == pytest.approx(cfg.max_sd, abs=1e-15)
    assert c.nu[0] == pytest.approx(2 * cfg.wu * (14.0 - 10.0) - cfg.eps_u * 10.0, rel=1e-14)       # the speed row's multiplier: -df/du at the bound
    assert c.active_rows["speed0"] == 1 and c.active_rows["max_sd"] == 1


def test_known_answer_one_active_hinge():
    """T = 1, one obstacle row with a = 0 (Im = -cc - d): -slack_gain d + ro1 / 2 min(Im, 0)^2 is smallest at Im = -slack_gain / ro1, i.e.
    d = slack_gain / ro1 - cc, inside the distance bounds"""
    cfg, si = _kwcase(1, 1, ws=0.0)
    si["cc"][:] = -0.5
    c = su_kkt.certify(cfg, si)
    assert c.d[0] == pytest.approx(0.5 + cfg.slack_gain / cfg.ro1, abs=1e-15) and bool(c.pattern[0])
    assert c.active_rows["max_sd"] == 0 and c.active_rows["min_sd"] == 0


def _scipy_case(trial):
    rng = np.random.default_rng(100 + trial)
    cfg = hp.make_cfg(T=int(rng.integers(3, 7)), N=int(rng.integers(1, 5)), dynamics=trial % 3, accelerated=int(trial != 4),
                      ro1=[200, 300, 200, 1, 200, 300][trial])
    return cfg, hp.su_inputs(rng, cfg)


@pytest.mark.parametrize("trial", range(6))
def test_reference_solver_agrees_with_scipy(trial):
    """the cases of test_oracle_su.py::test_su_against_scipy: scipy's trust-constr on the same formulation, at scipy's own 5e-4"""
    from scipy.optimize import minimize, LinearConstraint, Bounds
    cfg, si = _scipy_case(trial)
    P = su_kkt.SuProblem(cfg, si)
    cons = [LinearConstraint(P.Ceq, P.eq.rh, P.eq.rh)]
    if P.mc:
        cons.append(LinearConstraint(P.Cin, -np.inf, P.ineq.rh))
    f = lambda y: su_kkt.objective(cfg, si, *P.unpack(y))       # noqa: E731
    y0 = np.r_[si["nom_s"].ravel(), si["nom_u"].ravel(), np.full(cfg.T, 0.5)]
    r = minimize(f, y0, method="trust-constr", constraints=cons, options={"gtol": 1e-9, "xtol": 1e-11, "maxiter": 3000})
    S, U, D = P.unpack(r.x)
    c = P.solve(start=(S, U, D))                  # seeded by scipy's answer: what certifies is the optimum whatever the seed
    assert c.distance(S, U, D) < 5e-4
    assert c.f_star[0] <= r.fun + 1e-9 * (1 + abs(r.fun))


def certified_reference_problems():
    from test_ref_golden import _su_case
    g = np.load(os.path.join(GOLD, "ref_problems.npz"))
    out = []
    for k in range(int(g["su.count"])):
        cfg, si = _su_case(g, k)
        c = su_kkt.certify(cfg, si, start=(g[f"su.{k}.s"], g[f"su.{k}.u"], g[f"su.{k}.d"]))
        out.append((cfg, si, c))
    return g, out


def test_reference_solver_on_reference_built_problems():
    """the 6 su-problems built by the reference's own construct_su_prob: the certified optimum lies within the stand-in solver's 2e-6 of the
    reference's answers - the restated formulation is the reference's"""
    g, cases = certified_reference_problems()
    for k, (cfg, si, c) in enumerate(cases):
        d = c.distance(g[f"su.{k}.s"], g[f"su.{k}.u"], g[f"su.{k}.d"])
        print(f"reference problem {k}: T={cfg.T} N={cfg.N} |x* - x_ref| {d:.1e}, m {c.m:.1e}")
        assert d < 2e-6


# ---- the oracle's landed cold solve ------------------------------------------------------------------------------------------------------------
def _oracle_vs_cert(orc, cfg, si, what, tol=hp.TOL_U_FIXED):
    st, s, u, d, it = hp.su_solve(orc.lib.orc_su_solve, cfg, si)
    landed = orc.lib.orc_get_su_landed()
    assert st == 0, what
    c = su_kkt.certify(cfg, si, start=(s, u, d))
    return check_against(c, s, u, d, tol, f"{what} (landed {landed})"), c


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("dyn", [0, 1, 2])
def test_oracle_grid_against_the_certificate(orc, dyn, acc):
    worst = 0.0
    for T in GRID_T:
        for N in GRID_N:
            rng = np.random.default_rng(1000 * dyn + 100 * acc + 7 * T + N)
            cfg = hp.make_cfg(T=T, N=N, dynamics=dyn, accelerated=acc)
            d, _ = _oracle_vs_cert(orc, cfg, hp.su_inputs(rng, cfg), f"{DYN[dyn]} acc={acc} T={T} N={N}")
            worst = max(worst, d)
    print(f"{DYN[dyn]} accelerated={acc}: worst |x_oracle - x*| over the grid {worst:.1e}")


def test_oracle_hard_fixtures_against_the_certificate(orc):
    worst = 0.0
    for path in sorted(glob.glob(os.path.join(GOLD, "su_hard", "*.npz"))):
        if os.path.basename(path) == JUST_ACTIVE_FIXTURE + ".npz":
            continue                # (its own tests below)
        cfg, si = hp.load_su_case(path)
        d, c = _oracle_vs_cert(orc, cfg, si, os.path.basename(path))
        worst = max(worst, d)
    print(f"su_hard: worst |x_oracle - x*| {worst:.1e}")


def test_just_active_fixture_within_tol_u(orc):
    """the recorded problem on which the landed oracle answer misses TOL_U_FIXED: what holds for it (the numbers: tests/helpers.py at TOL_U)"""
    cfg, si = hp.load_su_case(os.path.join(GOLD, "su_hard", JUST_ACTIVE_FIXTURE + ".npz"))
    d, c = _oracle_vs_cert(orc, cfg, si, JUST_ACTIVE_FIXTURE, tol=hp.TOL_U)
    gap, viol = c.gap(*hp.su_solve(orc.lib.orc_su_solve, cfg, si)[2:4])
    print(f"{JUST_ACTIVE_FIXTURE}: |x_oracle - x*| {d:.2e}, m {c.m:.2e}, f - f* {gap:.1e}")
    assert orc.lib.orc_get_su_landed() == 1 and c.unique and 1e-7 < d < 2e-7


@pytest.mark.xfail(strict=True, raises=AssertionError, reason=(
    "finding: the landing accepts a stationarity residual of 100 x su_tol[0] relative (oracle su_land, kernel verdict of a landing round): "
    "1.35e-7 from the certified optimum (m = 0.25) where hinge rows sit 1e-8 .. 1e-7 from their switch"))
def test_just_active_fixture_within_tol_u_fixed(orc):
    cfg, si = hp.load_su_case(os.path.join(GOLD, "su_hard", JUST_ACTIVE_FIXTURE + ".npz"))
    st, s, u, d, it = hp.su_solve(orc.lib.orc_su_solve, cfg, si)
    c = su_kkt.certify(cfg, si, start=(s, u, d))
    assert st == 0 and c.unique
    dist = c.distance(s, u, d)
    assert dist <= hp.TOL_U_FIXED, dist


def edge_case(kind, dyn, T, N, seed):
    """su-problems where landings go wrong: every speed bound saturated, rate bounds saturated, d on min_sd / max_sd, every hinge active, none"""
    rng = np.random.default_rng(seed)
    cfg = hp.make_cfg(T=T, N=N, dynamics=dyn)
    si = hp.su_inputs(rng, cfg)
    if kind == "speed_saturated":
        si["vref"] = 25.0
        cfg.max_speed[0] = 2.0
    elif kind == "rate_saturated":
        si["nom_u"][:, ::3] += np.array([[3.0], [0.6]])           # a nominal with jumps
        si["ref"][0:2] += rng.normal(0, 2.0, (2, T + 1))
        cfg.acce_bound[0], cfg.acce_bound[1] = 0.05, 0.005
    elif kind == "d_on_min_sd":
        si["cc"] += 3.0                                             # every hinge deep: d pushed down to min_sd
        cfg.slack_gain = 0.5
    elif kind == "all_hinges":
        si["cc"] = np.einsum("ntk,kt->nt", si["a"], si["nom_s"][0:2, 1:]) + rng.uniform(0.0, 0.3, (N, T))
    elif kind == "no_hinge":
        si["cc"] -= 10.0                                            # d on max_sd
    return cfg, si


EDGES = ("speed_saturated", "rate_saturated", "d_on_min_sd", "all_hinges", "no_hinge")


@pytest.mark.parametrize("kind", EDGES)
def test_oracle_edge_cases_against_the_certificate(orc, kind):
    worst, seen = 0.0, {}
    for i, (dyn, T, N) in enumerate([(0, 10, 24), (1, 20, 24), (2, 25, 24), (0, 30, 200), (1, 33, 1), (2, 40, 24)]):
        cfg, si = edge_case(kind, dyn, T, N, 500 + i)
        d, c = _oracle_vs_cert(orc, cfg, si, f"{kind} {DYN[dyn]} T={T} N={N}")
        worst = max(worst, d)
        for k, v in c.active_rows.items():
            seen[k] = seen.get(k, 0) + v
        seen["hinges"] = seen.get("hinges", 0) + int(c.pattern.sum())
    print(f"{kind}: worst |x_oracle - x*| {worst:.1e}, active rows {seen}")
    want = {"speed_saturated": "speed0", "rate_saturated": "rate0", "d_on_min_sd": "min_sd", "no_hinge": "max_sd"}
    if kind in want:
        assert seen[want[kind]] > 0, seen           # the generator really puts rows of that kind on their bounds


@pytest.mark.parametrize("dyn,T,N,i", [(0, 10, 24, 0), (2, 30, 200, 2)])      # (dyn 1, T 20, i 1: recorded as su_hard/diff_T20_N24_just_active_hinges)
def test_oracle_just_active_hinges_against_the_certificate(orc, dyn, T, N, i):
    """hinge rows that only just miss the pattern: every row outside it is moved to Im* = 1e-8 .. 1e-7 (the optimum stays where it is)"""
    rng = np.random.default_rng(700 + i)
    cfg = hp.make_cfg(T=T, N=N, dynamics=dyn)
    si = hp.su_inputs(rng, cfg)
    st, s, u, d, it = hp.su_solve(orc.lib.orc_su_solve, cfg, si)
    c = su_kkt.certify(cfg, si, start=(s, u, d))
    im = su_kkt.SuProblem(cfg, si).hinge.value(c.xh, c.xl)[0].reshape(N, T)
    near = ~c.pattern.reshape(N, T)
    si["cc"] = np.where(near, si["cc"] + im - rng.uniform(1e-8, 1e-7, (N, T)), si["cc"])
    dist, c2 = _oracle_vs_cert(orc, cfg, si, f"just active {DYN[dyn]} T={T} N={N}")
    im2 = su_kkt.SuProblem(cfg, si).hinge.value(c2.xh, c2.xl)[0]
    assert np.sum(np.abs(im2) < 1e-6) >= near.sum() // 2
    print(f"just-active hinges {DYN[dyn]} T={T} N={N}: |x_oracle - x*| {dist:.1e}")


# ---- the su-problems of a closed loop, rebuilt from the handle's state -------------------------------------------------------------------------
def drive_recorded_loop(make_solver, name, on_su, steps=None):
    """ref_plumbing scene `name` stepped through *_admm_begin / su / lammuz / finish; on_su(k, it, si_rebuilt) after every su-problem that was solved
    with the (s, u, dis) it returned.  Returns the applied controls per step."""
    g = np.load(os.path.join(GOLD, "ref_plumbing.npz"))
    T, N, E, iter_num, ro1, dyn = (int(v) if i != 4 else float(v) for i, v in enumerate(g[f"{name}.cfg"]))
    from test_ref_golden import _car
    car_t = _car(dyn)
    solver = make_solver(T, car_t, E, N, iter_num, ro1)
    api, hd = solver._be.api, solver._be.handle
    G, h = f64(car_t.G), f64(car_t.h).ravel()
    applied = []
    for k in range(int(g[f"{name}.steps"]) if steps is None else steps):
        pre = f"{name}.{k}"
        n_obs = int(g[f"{pre}.n_obs"])
        if n_obs:
            A, b, cone = f64(g[f"{pre}.A"]), f64(g[f"{pre}.b"]), np.ascontiguousarray(g[f"{pre}.cone"], np.int32)
            assert api.upload_obstacles(hd, n_obs, dptr(A), dptr(b), iptr(cone), int(g[f"{pre}.per_t"])) == 0
        else:
            assert api.upload_obstacles(hd, 0, None, None, None, 0) == 0
        nom_s, nom_u, ref, speed = f64(g[f"{pre}.nom_s"]), f64(g[f"{pre}.nom_u"]), f64(g[f"{pre}.ref"]), float(g[f"{pre}.speed"])
        assert api.admm_begin(hd, dptr(nom_s), dptr(nom_u), dptr(ref), speed) == 0
        s_prev, u_prev = nom_s, nom_u
        out_u, out_s = np.zeros((2, T)), np.zeros((3, T + 1))
        for it in range(iter_num):
            si = su_kkt.su_inputs_from_state(solver.get_state(), s_prev, u_prev, ref, speed, G, h)
            stopped = C.c_int(0)
            assert api.admm_su(hd, it, C.byref(stopped)) == 0
            if stopped.value:
                break
            assert api.admm_lammuz(hd) == 0
            inf = Info()
            assert api.admm_finish(hd, dptr(out_u), dptr(out_s), C.byref(inf)) == 0
            on_su(k, it, solver._cfg, si, out_s.copy(), out_u.copy(), solver.get_state()["dis"].copy(), inf)
            s_prev, u_prev = out_s.copy(), out_u.copy()
        applied.append(out_u[:, 0].copy())
    return np.array(applied)


def _load_dump(path, T, N):
    from rda_planner_amd._capi import Cfg
    raw = open(path, "rb").read()
    off, out, csz = 0, [], C.sizeof(Cfg)
    while off < len(raw):
        off += csz
        hd = np.frombuffer(raw, np.float64, 4, off); off += 32

        def take(n):
            nonlocal off
            a = np.frombuffer(raw, np.float64, n, off).copy(); off += 8 * n
            return a
        out.append(dict(speed=hd[2], it=int(hd[3]), nom_s=take(3 * (T + 1)), nom_u=take(2 * T), ref=take(3 * (T + 1)), a=take(2 * N * T),
                        cc=take(N * T), g=take(2 * N * T), d0=take(T)))
    return out


@pytest.mark.parametrize("name", ["c1", "c4", "ns"])
def test_rebuilt_su_problems_equal_what_the_oracle_solves(orc, tmp_path, name):
    """the harness of the GPU hot-path test: the su-problem of every ADMM iteration rebuilt from the handle's state (su_kkt.su_inputs_from_state)
    is what orc_admm_su records (oracle_backend.su_dump) bit for bit; the oracle's in-loop answers are within TOL_U_FIXED of the certified optimum"""
    from oracle.oracle_backend import oracle_backend
    from rda_planner_amd.rda_solver import RDA_solver
    dump = tmp_path / "su.bin"
    rebuilt, worst = [], [0.0]

    def make(T, car_t, E, N, iter_num, ro1):
        return RDA_solver(T, car_t, E, N, iter_num=iter_num, time_print=False, ro1=ro1, _backend=oracle_backend)

    def on_su(k, it, cfg, si, s, u, dis, inf):
        rebuilt.append((it, si))
        c = su_kkt.certify(cfg, si, start=(s, u, dis))
        worst[0] = max(worst[0], check_against(c, s, u, dis, hp.TOL_U_FIXED, f"{name} step {k} it {it}"))
    with su_dump(dump):
        drive_recorded_loop(make, name, on_su, steps=3 if name == "ns" else None)
    T, N = rebuilt[0][1]["nom_u"].shape[1], rebuilt[0][1]["a"].shape[0]
    rec = _load_dump(str(dump), T, N)
    assert len(rec) == len(rebuilt) > 0
    for (it, si), r in zip(rebuilt, rec):
        assert it == r["it"] and r["speed"] == si["vref"]
        for key in ("nom_s", "nom_u", "ref", "a", "cc", "g", "d0"):
            assert np.array_equal(si[key].ravel(), r[key]), (name, it, key, np.abs(si[key].ravel() - r[key]).max())
    print(f"{name}: {len(rec)} su-problems rebuilt bit for bit; worst |x_oracle - x*| in the loop {worst[0]:.1e}")
