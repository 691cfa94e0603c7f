"""TEST INFRASTRUCTURE: an independent reference for the interior-point LamMuZ mode (`lmz_central`).  numpy and the standard
library only; nothing of oracle/ or of the product is imported.

Every solver of the mode - oracle/lmz_ipm.c, the row-parallel kernel (csrc/lammuz_ip_device.h) and the per-thread kernels
(csrc/lammuz_cp_device.h) - claims to end on ONE point: the point of the central path of the reference's cone program of one
(obstacle slot, stage) at the barrier parameter mu*.  For a cone program  min 1/2 x'Px + q'x  s.t.  s = h - Gx in K  that point is
the unique minimiser of the log-barrier problem

    f(x)  -  mu* sum_LP w_i log s_i  -  (mu* / 2) sum_SOC log det s_k ,      det (t ; u) = t^2 - |u|^2

(its stationarity condition  Px + q + G'z = 0  with  z_i = mu* w_i / s_i  and  z_k = mu* s_k^-1  IS  s o z = mu* e with zero
residuals; w_i is the number of times an LP row is written).  This module minimises that function by a plain damped Newton
iteration - no primal-dual steps, no Nesterov-Todd scaling, no predictor-corrector, no stop rule on s o z: none of the machinery the
solvers under test share - following mu from 1 down to mu* from a strictly feasible start, and finishes with Newton steps whose
gradient, Hessian and linear-system residual are evaluated in np.longdouble.  (Where np.longdouble is not wider than double -
`WIDE` below is False - the refinement and the certificate run in double; the certificate then still holds or the row raises.)

The canonical form is the one stated in the header comments of oracle/lmz_ipm.c and csrc/lammuz_ip_device.h:

    x = [ lam (E) | mu (R) | z | th | tn | mm | (tl) | (tr) ]
    minimise  1/2 th^2 + 1/2 ro2 |M'lam + G'mu + xi|^2                  (accelerated; otherwise 1/2 Im^2 and no th)
    s.t.      z >= 0 ; th >= -Im ; th >= 0 ;  (tn ; A'lam) in Q^3 ; tn <= mm ; mm <= 1          Im = q'lam - h'mu - z + zeta - dbar
              obstacle cone  Rpositive: lam >= 0   |  norm2: (tl ; -lam_0, -lam_1) in Q^3, tl + lam_2 <= 0 written E times (w = E)
              robot cone     Rpositive: mu >= 0    |  norm2: (tr ; -mu_0 .. -mu_{R-2}) in Q^R, tr + mu_{R-1} <= 0
    q_i = A_i p - b_i ,  M_i = A_i Rot(phi) ;  the multiplier of a zero-padded edge row (A_i = 0, b_i = 0) is held at 0, and so are
    lam_3 .. lam_{E-1} of a circle obstacle (they enter nothing).

CERTIFICATE.  `solve_row` returns only what it can certify in the wide type: every slack strictly inside its cone, and the
infinity norm of the barrier gradient over the free variables <= GRAD_TOL (reached on the grid: <= 1.4e-12), and a Newton step at
the returned point (its distance to the centre, to first order) <= STEP_TOL relative (STEP_TOL_FLAT when not accelerated).  It raises
`NotCertified` otherwise: a row the reference cannot certify is an error of the test that asked for it, never a skip.

RECORDED DEVIATIONS of the oracle (`orc_lammuz_ipm_one`) from this reference, dev = max |d(lam, mu, z)| / (1 + max |(lam, mu, z)|),
worst over the pinned grid of tests/test_lmz_central_ref.py (E in {3, 4, 5, 6, 8}; rectangle, triangle, octagon and circle
robots; ro2 in {1, 5}; polygons with 3 .. E edges and circles), no oracle row failed:

    class (accelerated, mu*)      oracle worst dev      reference's own error (Newton step at its point / (1 + |x|))
    (1, 1e-3)                     3.38e-9               <= 5.9e-15
    (1, 1e-6)                     8.83e-9               <= 1.7e-12
    (0, 1e-3)                     1.23e-8               <= 6.0e-13
    (0, 1e-6)                     8.04e-7               <= 1.1e-9

The oracle is an independent implementation with the stop rule of the kernels (residuals <= 1e-10 relative, |s o z - mu* e| <=
1e-7 mu*): two implementations may stop on different iterates inside that centring band, and 10 x the oracle's worst deviation is
the bound the GPU kernels are held to per class (`gpu_bound`, tests/test_gpu_central_rows.py).  It is never derived from a kernel."""
from collections import namedtuple

import numpy as np

LD = np.longdouble
WIDE = np.finfo(LD).eps < np.finfo(np.float64).eps
GRAD_TOL = 1e-10          # certificate: |barrier gradient|_inf over the free variables, evaluated in LD
# ... and the Newton step at the returned point (the reference's own error, to first order), relative to 1 + |x|_inf.  Not accelerated, the cost
# 1/2 Im^2 is flat along z against the other terms of Im and only the barrier (curvature mu* / slack^2, 1e-8 at mu* = 1e-6) fixes the centre in that
# direction: there the rounding of the wide gradient itself (1e-16 absolute) leaves ~1e-9 relative, reached on the grid of tests/test_lmz_central_ref.py
STEP_TOL = 1e-10
STEP_TOL_FLAT = 5e-9

# worst deviation of the oracle from this reference per class (accelerated, mu*): measured by
# tests/test_lmz_central_ref.py::test_oracle_equals_the_reference_on_the_pinned_grid, rounded up (the test prints them and holds the oracle to them)
ORACLE_WORST = {(1, 1e-3): 3.4e-9, (1, 1e-6): 8.9e-9, (0, 1e-3): 1.3e-8, (0, 1e-6): 8.1e-7}


def gpu_bound(accelerated, mu_star):
    """the bound on the relative row deviation of a kernel, per class: 10 x the oracle's recorded worst"""
    return 10.0 * ORACLE_WORST[(int(bool(accelerated)), float(mu_star))]


class NotCertified(RuntimeError):
    pass


Row = namedtuple("Row", "E R A b cone_norm2 robot_norm2 p phi G h xi zeta dbar ro2 accelerated mu_star")
Central = namedtuple("Central", "lam mu z Im Hm x grad_res step")


# ---------------------------------------------------------------------------------------------------------------------------------
# the generic barrier problem:  min 1/2 x'Px + q'x  -  mu sum_i w_i log(r_i - a_i'x)  -  mu/2 sum_k log det(c_k - S_k x)
# ---------------------------------------------------------------------------------------------------------------------------------
class Problem:
    def __init__(self, P, q, lp_a, lp_r, lp_w, soc, free=None):
        n = len(q)
        self.n = n
        self.P, self.q = np.asarray(P, LD).reshape(n, n), np.asarray(q, LD)
        self.a = np.asarray(lp_a, LD).reshape(-1, n)
        self.r, self.w = np.asarray(lp_r, LD), np.asarray(lp_w, LD)
        self.soc = [(np.asarray(S, LD), np.asarray(c, LD)) for S, c in soc]
        self.free = np.ones(n, bool) if free is None else np.asarray(free, bool)
        self._cast = {}

    def _as(self, dt):
        if dt not in self._cast:
            self._cast[dt] = (self.P.astype(dt), self.q.astype(dt), self.a.astype(dt), self.r.astype(dt), self.w.astype(dt),
                              [(S.astype(dt), c.astype(dt)) for S, c in self.soc])
        return self._cast[dt]

    def barrier(self, x, mu, dt=np.float64, hessian=True):
        """(value, gradient, Hessian) of the barrier function at x, or None when a slack is not strictly inside its cone"""
        P, q, a, r, w, soc = self._as(dt)
        x, mu = x.astype(dt), dt(mu)
        Px = P @ x
        f = dt(0.5) * (x @ Px) + q @ x
        g = Px + q
        H = P.copy() if hessian else None
        if len(r):
            s = r - a @ x
            if not np.all(s > 0):
                return None
            f = f - mu * (w @ np.log(s))
            g = g + a.T @ (mu * w / s)
            if hessian:
                H += (a.T * (mu * w / (s * s))) @ a
        for S, c in soc:
            s = c - S @ x
            det = s[0] * s[0] - s[1:] @ s[1:]
            if not (s[0] > 0 and det > 0):
                return None
            f = f - dt(0.5) * mu * np.log(det)
            js = s.copy(); js[1:] = -js[1:]                      # J s ;  s^-1 = J s / det
            sinv = js / det
            g = g + mu * (S.T @ sinv)
            if hessian:                                          # Hessian of -1/2 log det in s:  2 s^-1 s^-1' - J / det
                Hs = dt(2.0) * np.outer(sinv, sinv)
                Hs[0, 0] -= dt(1.0) / det
                for i in range(1, len(s)):
                    Hs[i, i] += dt(1.0) / det
                H += mu * (S.T @ Hs @ S)
        return f, g, H


def _solve_wide(H, g):
    """H d = g for H, g in LD: the double solve, refined against the residual in LD (np.linalg has no wide solve)"""
    Hd = H.astype(float)
    d = np.linalg.solve(Hd, g.astype(float)).astype(LD)
    for _ in range(3):
        d = d + np.linalg.solve(Hd, (g - H @ d).astype(float)).astype(LD)
    return d


def central_point(prob, mu_star, x0, mu0=1.0, step_tol=STEP_TOL):
    """the minimiser of prob's barrier function at mu_star, from the strictly feasible x0; returns (x as LD, certified gradient residual, Newton step at x)"""
    fr = np.flatnonzero(prob.free)
    x = np.asarray(x0, float).copy()
    if prob.barrier(x, mu0) is None:
        raise NotCertified("the start is not strictly feasible")
    mu = max(float(mu0), float(mu_star))
    while True:
        last = mu == mu_star
        for _ in range(60):                                      # damped Newton at this mu (on the way down the centre is only needed roughly)
            f, g, H = prob.barrier(x, mu)
            dx = np.zeros(prob.n)
            dx[fr] = -np.linalg.solve(H[np.ix_(fr, fr)], g[fr])
            dec = -(g @ dx)
            if not dec > (1e-20 if last else 1e-6) * (1.0 + abs(f)):
                break
            t = 1.0
            while t >= 1e-12:
                o = prob.barrier(x + t * dx, mu, hessian=False)
                if o is not None and o[0] <= f - 1e-4 * t * dec + 1e-15 * abs(f):
                    break
                t *= 0.5
            if t < 1e-12:
                break
            x = x + t * dx
        if mu == mu_star:
            break
        mu = max(0.2 * mu, float(mu_star))
    xl = x.astype(LD)                                            # refinement: Newton steps in the wide type
    res = np.inf
    for _ in range(12):
        o = prob.barrier(xl, mu_star, LD)
        if o is None:
            raise NotCertified("a slack left its cone during the refinement")
        _, g, H = o
        r = float(np.abs(g[fr]).max())
        if not r < 0.5 * res:                                    # (the wide type's rounding level is reached)
            break
        res = r
        xl[fr] = xl[fr] - _solve_wide(H[np.ix_(fr, fr)], g[fr])
    o = prob.barrier(xl, mu_star, LD)                            # the certificate
    if o is None:
        raise NotCertified("a slack is not strictly inside its cone")
    res = float(np.abs(o[1][fr]).max())
    # the Newton step from the final point: its distance to the centre, to first order
    step = float(np.abs(_solve_wide(o[2][np.ix_(fr, fr)], o[1][fr])).max())
    if not res <= GRAD_TOL:
        raise NotCertified(f"barrier gradient {res:.2e} > {GRAD_TOL:.0e}")
    if not step <= step_tol * (1.0 + float(np.abs(xl).max())):
        raise NotCertified(f"Newton step {step:.2e} at the final point: the centre is not resolved to {step_tol:.0e} relative")
    return xl, res, step


# ---------------------------------------------------------------------------------------------------------------------------------
# one LamMuZ row
# ---------------------------------------------------------------------------------------------------------------------------------
def _geometry(row, dt=LD):
    """q [E], M [E][2] of the row in `dt`"""
    A, b, p = np.asarray(row.A, dt).reshape(row.E, 2), np.asarray(row.b, dt).ravel(), np.asarray(row.p, dt).ravel()
    c, s = np.cos(dt(row.phi)), np.sin(dt(row.phi))
    q = A @ p - b
    M = np.stack((A[:, 0] * c + A[:, 1] * s, -A[:, 0] * s + A[:, 1] * c), axis=1)
    return A, b, q, M


def build_row(row):
    """(Problem, index dict, strictly feasible start) of one row"""
    E, R, acc, circ, rn2 = row.E, row.R, bool(row.accelerated), bool(row.cone_norm2), bool(row.robot_norm2)
    A, b, q, M = _geometry(row)
    G, h, xi = np.asarray(row.G, LD).reshape(R, 2), np.asarray(row.h, LD).ravel(), np.asarray(row.xi, LD).ravel()
    names = [f"lam{i}" for i in range(E)] + [f"mu{j}" for j in range(R)] + ["z"] + (["th"] if acc else []) + ["tn", "mm"] \
        + (["tl"] if circ else []) + (["tr"] if rn2 else [])
    ix = {k: i for i, k in enumerate(names)}
    n = len(names)
    kap = LD(row.zeta) - LD(row.dbar)

    def unit(i, v=1.0):
        e = np.zeros(n, LD); e[i] = v
        return e
    cv = np.zeros(n, LD); cv[:E] = q; cv[E:E + R] = -h; cv[ix["z"]] = -1          # Im = cv'x + kap
    B = np.zeros((2, n), LD); B[:, :E] = M.T; B[:, E:E + R] = G.T                   # H = B x + xi
    ro2 = LD(row.ro2)
    P, qq = ro2 * (B.T @ B), ro2 * (B.T @ xi)
    if acc:
        P[ix["th"], ix["th"]] += 1
    else:
        P += np.outer(cv, cv); qq = qq + kap * cv
    lp = []                                                       # (a, r, w):  r - a'x > 0
    soc = []                                                      # (S, c):  c - S x in Q
    free = np.ones(n, bool)
    lp.append((unit(ix["z"], -1), 0, 1))                          # z >= 0
    if acc:
        lp.append((-unit(ix["th"]) - cv, kap, 1))                 # th + Im >= 0
        lp.append((unit(ix["th"], -1), 0, 1))                     # th >= 0
    S = np.zeros((3, n), LD); S[0, ix["tn"]] = -1; S[1:, :E] = -A.T
    soc.append((S, np.zeros(3)))                                  # (tn ; A'lam) in Q^3
    lp.append((unit(ix["tn"]) - unit(ix["mm"]), 0, 1))            # tn <= mm
    lp.append((unit(ix["mm"]), 1, 1))                             # mm <= 1
    if circ:
        S = np.zeros((3, n), LD); S[0, ix["tl"]] = -1; S[1, 0] = 1; S[2, 1] = 1
        soc.append((S, np.zeros(3)))                              # (tl ; -lam_0, -lam_1) in Q^3
        lp.append((unit(ix["tl"]) + unit(2), 0, E))               # tl + lam_2 <= 0, written E times
        free[3:E] = False
    else:
        for i in range(E):
            if np.any(A[i] != 0) or b[i] != 0:
                lp.append((unit(i, -1), 0, 1))                    # lam_i >= 0
            else:
                free[i] = False                                   # zero-padded edge row: multiplier held at 0
    if rn2:
        S = np.zeros((R, n), LD); S[0, ix["tr"]] = -1
        for j in range(R - 1):
            S[1 + j, E + j] = 1
        soc.append((S, np.zeros(R)))                              # (tr ; -mu_0 .. -mu_{R-2}) in Q^R
        lp.append((unit(ix["tr"]) + unit(E + R - 1), 0, 1))       # tr + mu_{R-1} <= 0
    else:
        for j in range(R):
            lp.append((unit(E + j, -1), 0, 1))                    # mu_j >= 0
    prob = Problem(P, qq, [a for a, _, _ in lp], [r for _, r, _ in lp], [w for _, _, w in lp], soc, free)
    # a strictly feasible start
    x = np.zeros(n)
    if circ:
        x[2], x[ix["tl"]] = -1.0, 0.5
    else:
        live = free[:E].astype(float)
        nrm = float(np.linalg.norm(np.asarray(A, float).T @ live))
        x[:E] = live * (0.25 / nrm) if nrm > 0.25 else live
    x[ix["tn"]], x[ix["mm"]] = 0.5, 0.75
    if rn2:
        x[E + R - 1], x[ix["tr"]] = -1.0, 0.5
    else:
        x[E:E + R] = 1.0
    x[ix["z"]] = 1.0
    if acc:
        x[ix["th"]] = max(-float(cv @ x.astype(LD) + kap), 0.0) + 1.0
    return prob, ix, x


def Im_terms(row, lam, mu):
    """Im(lam, mu) = q'lam - h'mu in LD, with the sum of the absolute values of its elementary products and their count
    (what a rounding-level bound on any evaluation order is made of)"""
    A, b, _, _ = _geometry(row)
    p, h = np.asarray(row.p, LD).ravel(), np.asarray(row.h, LD).ravel()
    lam, mu = np.asarray(lam, LD), np.asarray(mu, LD)
    val = lam @ (A @ p - b) - h @ mu
    mag = np.abs(lam) @ (np.abs(A[:, 0] * p[0]) + np.abs(A[:, 1] * p[1]) + np.abs(b)) + np.abs(h * mu).sum()
    return val, mag, 3 * row.E + row.R


def Hm_terms(row, lam, mu):
    """Hm(lam, mu) = M'lam + G'mu [2] in LD, likewise"""
    A, _, _, M = _geometry(row)
    G = np.asarray(row.G, LD).reshape(row.R, 2)
    lam, mu = np.asarray(lam, LD), np.asarray(mu, LD)
    c, s = np.cos(LD(row.phi)), np.sin(LD(row.phi))
    val = M.T @ lam + G.T @ mu
    al = np.abs(lam)
    mag = np.stack((al @ (np.abs(A[:, 0] * c) + np.abs(A[:, 1] * s)), al @ (np.abs(A[:, 0] * s) + np.abs(A[:, 1] * c)))) + np.abs(mu) @ np.abs(G)
    return val, mag, 2 * row.E + row.R


_cache = {}


def solve_row(row):
    """the certified central point of one row: Central(lam, mu, z, Im, Hm, x, grad_res); Im = q'lam - h'mu, Hm = M'lam + G'mu.
    Equal rows (the padding copies of a short obstacle list) are solved once."""
    key = tuple(np.asarray(v, float).tobytes() for v in row)
    if key not in _cache:
        prob, ix, x0 = build_row(row)
        xl, res, step = central_point(prob, row.mu_star, x0, step_tol=STEP_TOL if row.accelerated else STEP_TOL_FLAT)
        step /= 1.0 + float(np.abs(xl).max())
        E, R = row.E, row.R
        lam, mu, z = xl[:E], xl[E:E + R], xl[ix["z"]]
        if len(_cache) > 4096:
            _cache.clear()
        _cache[key] = Central(lam.astype(float), mu.astype(float), float(z), float(Im_terms(row, lam, mu)[0]),
                              Hm_terms(row, lam, mu)[0].astype(float), xl.astype(float), res, step)
    return _cache[key]


def deviation(ref, lam, mu, z):
    """max |d(lam, mu, z)| / (1 + max |(lam, mu, z)|) of an answer against the reference's"""
    want = np.r_[ref.lam, ref.mu, ref.z]
    got = np.r_[np.asarray(lam, float).ravel(), np.asarray(mu, float).ravel(), float(z)]
    return float(np.abs(got - want).max() / (1.0 + np.abs(want).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the rows of one LamMuZ call of a driven loop, rebuilt from the handle's state
# ---------------------------------------------------------------------------------------------------------------------------------
StateRow = namedtuple("StateRow", "n t row lam mu z xi zeta xi_new zeta_new dis a_lam b_lam")


def rows_from_state(pre_state, post_state, out_s, A, b, cone, per_t, G, h, cfg, mu_star):
    """One StateRow per (obstacle slot n, stage t) of the LamMuZ call between `pre_state` and `post_state` (dicts of *_get_state):
    xi, zeta are the ones BEFORE the call, `dis` (the d-bar of the su-problem just solved) and `out_s` (its states) the ones AFTER
    it.  A [n_obs][nt][E][2], b [n_obs][nt][E], cone [n_obs] are the staged obstacles: stage t reads slot t + 1 of a per-stage
    obstacle, else slot 0.  The duals of stage t live in column t + 1 of lam, mu, xi and in column t of z, zeta."""
    T, N, E, R = int(cfg.T), int(cfg.N), int(cfg.E), int(cfg.R)
    n_obs = len(cone)
    A, b = np.asarray(A, float).reshape(n_obs, -1, E, 2), np.asarray(b, float).reshape(n_obs, -1, E)
    G, h, out_s = np.asarray(G, float).reshape(R, 2), np.asarray(h, float).ravel(), np.asarray(out_s, float).reshape(3, T + 1)
    rows = []
    for n in range(min(n_obs, N)):
        for t in range(T):
            ti = t + 1 if per_t else 0
            row = Row(E, R, A[n, ti].copy(), b[n, ti].copy(), int(cone[n]), int(cfg.robot_norm2), out_s[0:2, t + 1].copy(), float(out_s[2, t]), G, h,
                      pre_state["xi"][n, t + 1].copy(), float(pre_state["zeta"][n, t]), float(post_state["dis"][t]), float(cfg.ro2),
                      int(cfg.accelerated), float(mu_star))
            rows.append(StateRow(n, t, row, post_state["lam"][n, t + 1].copy(), post_state["mu"][n, t + 1].copy(), float(post_state["z"][n, t]),
                                 pre_state["xi"][n, t + 1].copy(), float(pre_state["zeta"][n, t]), post_state["xi"][n, t + 1].copy(),
                                 float(post_state["zeta"][n, t]), float(post_state["dis"][t]), post_state["a_lam"][n, t + 1].copy(),
                                 float(post_state["b_lam"][n, t + 1])))
    return rows


EPS = float(np.finfo(np.float64).eps)
EPILOGUE_ULPS = 4


def _tightest(err, bound):
    """the component whose error is largest in units of its bound (an error over a zero bound first)"""
    return int(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


def epilogue_errors(sr):
    """the fused epilogue of one row, checked on the duals the solver itself returned:
        xi' = xi + Hm(lam', mu') ,   zeta' = zeta + Im(lam', mu') - dis[t] - z' ,   and the condensed terms  a_lam = A'lam' ,  b_lam = lam''b
    Returns (error of xi', its bound, error of zeta', its bound, error of the condensed terms, its bound).  The bound is a rounding-level one: EPILOGUE_ULPS eps sum |terms|, the terms being
    the elementary products of the sum (lam_i A_ik p_k, lam_i b_i, mu_j h_j | lam_i A_ik cos / sin, mu_j G_jk) and its further addends - so it holds for
    any order of evaluation (condensed A'lam and lam'b first or row by row, fused multiply-adds or not, cos / sin within an ulp), to first order and with
    the usual cancellation of rounding errors over the 10 .. 35 terms (their worst case would be (number of terms) eps sum |terms|)."""
    hm, hmag, hk = Hm_terms(sr.row, sr.lam, sr.mu)
    im, imag, ik = Im_terms(sr.row, sr.lam, sr.mu)
    d_xi = np.abs(np.asarray(sr.xi, LD) + hm - np.asarray(sr.xi_new, LD)).astype(float)
    bb_xi = EPILOGUE_ULPS * EPS * (hmag.astype(float) + np.abs(sr.xi))
    k = _tightest(d_xi, bb_xi)
    e_xi, b_xi = float(d_xi[k]), float(bb_xi[k])
    e_ze = float(abs(LD(sr.zeta) + im - LD(sr.dis) - LD(sr.z) - LD(sr.zeta_new)))
    b_ze = EPILOGUE_ULPS * EPS * float(imag + abs(sr.zeta) + abs(sr.dis) + abs(sr.z))
    A, b = np.asarray(sr.row.A, LD).reshape(sr.row.E, 2), np.asarray(sr.row.b, LD).ravel()
    lam = np.asarray(sr.lam, LD)
    d_c = np.abs(np.r_[A.T @ lam, b @ lam] - np.r_[np.asarray(sr.a_lam, LD), LD(sr.b_lam)]).astype(float)
    bb_c = EPILOGUE_ULPS * EPS * np.r_[np.abs(A).T @ np.abs(lam), np.abs(b) @ np.abs(lam)].astype(float)
    k = _tightest(d_c, bb_c)
    return e_xi, b_xi, e_ze, b_ze, float(d_c[k]), float(bb_c[k])
