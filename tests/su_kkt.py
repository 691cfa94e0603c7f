"""Independent reference solver for the su-problem, with a certificate (test infrastructure; numpy and the standard library only - nothing of
oracle/ or of the library under test).

The problem is the reference's su-problem (rda_solver.py:216-231), restated UNCONDENSED: states S 3x(T+1), controls U 2xT and safety distances
D [T] are all variables, the dynamics are equality rows.
    cost         C0 + C1 (:1011-1032): ws |w (S - ref)|^2 (w = (1, 1, 0) for omni), wu |U[0] - vref|^2, -slack_gain sum D
                 obstacle terms (:831-872): 0.5 ro1 min(Im, 0)^2 (accelerated) or 0.5 ro1 Im^2, Im = a . S[0:2, t+1] - cc - D[t];
                 0.5 ro2 |g + a (R(ph) + dR(ph) (S[2, t+1] - ph))|^2 with the rotation linearised about the nominal heading ph (:365-370)
                 the project's tie-break 0.5 eps_u |U|^2
    constraints  S[:, t+1] = A_t S[:, t] + B_t U[:, t] + C_t (:911-927), S[:, 0] = nom_s[:, 0], |U| <= max_speed,
                 |U[:, t+1] - U[:, t]| <= acce_bound (:930-938), min_sd <= D <= max_sd (:940-947)
N = 0 (no obstacle terms): D enters through -slack_gain sum D and its bounds only, D = max_sd (include/rda_hip.h, next to rda_su_solve).

Method: the active set (bound and rate rows held at equality) and the hinge pattern (Im < 0) are searched by a primal-dual active-set iteration in
float64; for a candidate set the equality-constrained KKT system is solved in float64 and refined with residuals in double-double arithmetic (~32
significant digits).  The result is accepted only on its certificate - primal feasibility <= 1e-13, inequality multipliers >= -1e-13, a consistent
hinge pattern (Im <= 1e-13 in it, >= -1e-13 outside), stationarity <= 1e-12 relative - so a wrong active set cannot certify, whatever seeded the
search.  The search itself is local: it converges from a seed near the optimum (the candidate under test, scipy's or the reference's answer, a hand
solution) and raises when it does not certify; from the nominal alone it often does not converge.
bound(x) = sqrt(2 (f(x) - f(x*)) / m) uses the curvature m on the certified face: it bounds candidates on that face (active rows at equality).
"""
import numpy as np

FEAS_TOL, MULT_TOL, HINGE_TOL, STAT_TOL = 1e-13, 1e-13, 1e-13, 1e-12
M_SINGULAR = 1e-6            # below this smallest curvature on the active face the optimum is treated as non-unique: compare objectives, not points


# ---- the reference's linearisation and cost, literally (also used by tests/test_oracle_su.py) ----------------------------------------------------
def lin(dyn, s, u, dt, L):
    phi, v, psi = s[2], u[0], u[1]
    if dyn == 2:
        phi = u[1]
        A = np.eye(3)
        B = np.array([[np.cos(phi) * dt, -v * np.sin(phi) * dt], [np.sin(phi) * dt, v * np.cos(phi) * dt], [0, 0]])
        C = np.array([phi * v * np.sin(phi) * dt, -phi * v * np.cos(phi) * dt, 0])
        return A, B, C
    A = np.array([[1, 0, -v * dt * np.sin(phi)], [0, 1, v * dt * np.cos(phi)], [0, 0, 1]])
    if dyn == 0:
        B = np.array([[np.cos(phi) * dt, 0], [np.sin(phi) * dt, 0], [np.tan(psi) * dt / L, v * dt / (L * np.cos(psi) ** 2)]])
        C = np.array([phi * v * np.sin(phi) * dt, -phi * v * np.cos(phi) * dt, -psi * v * dt / (L * np.cos(psi) ** 2)])
    else:
        B = np.array([[np.cos(phi) * dt, 0], [np.sin(phi) * dt, 0], [0, dt]])
        C = np.array([phi * v * np.sin(phi) * dt, -phi * v * np.cos(phi) * dt, 0])
    return A, B, C


def objective(cfg, si, S, U, D):
    """the reference's su cost, literally (rda_solver.py:1011-1032, 846-851, 868, 376-383), plus the eps_u tie-break"""
    T, N, dyn = cfg.T, cfg.N, cfg.dynamics
    w = np.array([1, 1, 0.0 if dyn == 2 else 1.0])[:, None]
    J = cfg.ws * np.sum(w * (S - si["ref"]) ** 2) + cfg.wu * np.sum((U[0] - si["vref"]) ** 2) - cfg.slack_gain * np.sum(D)
    J += 0.5 * cfg.eps_u * np.sum(U ** 2)
    for t in range(T):
        ph = si["nom_s"][2, t]
        Rm = np.array([[np.cos(ph), -np.sin(ph)], [np.sin(ph), np.cos(ph)]])
        dR = np.array([[-np.sin(ph), -np.cos(ph)], [np.cos(ph), -np.sin(ph)]])
        rot = Rm + dR * (S[2, t + 1] - ph)
        for n in range(N):
            Im = si["a"][n, t] @ S[0:2, t + 1] - si["cc"][n, t] - D[t]
            J += 0.5 * cfg.ro1 * (min(Im, 0) ** 2 if cfg.accelerated else Im ** 2)
            Hm = si["g"][n, t] + si["a"][n, t] @ rot
            J += 0.5 * cfg.ro2 * Hm @ Hm
    return J


# ---- double-double arithmetic (Dekker / Knuth error-free transformations; numpy arrays of (hi, lo)) ----------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _quick(a, b):
    s = a + b
    return s, b - (s - a)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_add(ah, al, bh, bl):
    s, e = _two_sum(ah, bh)
    t, f = _two_sum(al, bl)
    e = e + t
    s, e = _quick(s, e)
    return _quick(s, e + f)


def dd_mul(ah, al, bh, bl):
    p, e = _two_prod(ah, bh)
    return _quick(p, e + (ah * bl + al * bh))


def dd_sum(h, l, axis=-1):
    """pairwise sum along `axis`"""
    h, l = np.moveaxis(np.asarray(h, float), axis, -1), np.moveaxis(np.asarray(l, float), axis, -1)
    while h.shape[-1] > 1:
        if h.shape[-1] % 2:
            z = np.zeros(h.shape[:-1] + (1,))
            h, l = np.concatenate([h, z], -1), np.concatenate([l, z], -1)
        h, l = dd_add(h[..., 0::2], l[..., 0::2], h[..., 1::2], l[..., 1::2])
    if h.shape[-1] == 0:
        return np.zeros(h.shape[:-1]), np.zeros(h.shape[:-1])
    return h[..., 0], l[..., 0]


class _Rows:
    """sparse rows sum_j c[k, j] x[idx[k, j]] - r[k] (padded with c = 0), r in double-double"""

    def __init__(self, idx, c, rh, rl=None):
        k = np.asarray(c).size // max(1, len(rh)) if len(rh) else 3
        self.idx, self.c = np.asarray(idx, np.int64).reshape(len(rh), k), np.asarray(c, float).reshape(len(rh), k)
        self.rh = np.asarray(rh, float)
        self.rl = np.zeros_like(self.rh) if rl is None else np.asarray(rl, float)

    def value(self, xh, xl):
        ph, pl = dd_mul(xh[self.idx], xl[self.idx], self.c, np.zeros_like(self.c))
        vh, vl = dd_sum(ph, pl)
        return dd_add(vh, vl, -self.rh, -self.rl)

    def dense(self, n):
        M = np.zeros((len(self.rh), n))
        np.add.at(M, (np.repeat(np.arange(len(self.rh)), self.idx.shape[1]), self.idx.ravel()), self.c.ravel())
        return M


def _scatter(n, idx, th, tl):
    """dd sum of the contributions th + tl [k, j] into the variables idx [k, j]"""
    idx, th, tl = idx.ravel(), th.ravel(), tl.ravel()
    nz = (th != 0) | (tl != 0)
    idx, th, tl = idx[nz], th[nz], tl[nz]
    order = np.argsort(idx, kind="stable")
    idx, th, tl = idx[order], th[order], tl[order]
    cnt = np.bincount(idx, minlength=n)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    pos = np.arange(len(idx)) - start[idx]
    W = max(1, int(cnt.max()) if len(cnt) else 1)
    Ph, Pl = np.zeros((n, W)), np.zeros((n, W))
    Ph[idx, pos], Pl[idx, pos] = th, tl
    return dd_sum(Ph, Pl)


class SuProblem:
    """the su-problem of (cfg, si) - si in the form of helpers.su_inputs / helpers.load_su_case"""

    def __init__(self, cfg, si):
        T, N, dyn = int(cfg.T), int(cfg.N), int(cfg.dynamics)
        self.cfg, self.T, self.N, self.acc = cfg, T, N, bool(cfg.accelerated)
        nom_s, nom_u = np.asarray(si["nom_s"], float).reshape(3, T + 1), np.asarray(si["nom_u"], float).reshape(2, T)
        ref = np.asarray(si["ref"], float).reshape(3, T + 1)
        a, cc, g = (np.asarray(si["a"], float).reshape(N, T, 2), np.asarray(si["cc"], float).reshape(N, T), np.asarray(si["g"], float).reshape(N, T, 2))
        self.nom_u = nom_u
        self.nS = 3 * (T + 1)
        self.n = n = self.nS + 3 * T
        S = lambda r, t: r * (T + 1) + t            # noqa: E731
        Ui = lambda i, t: self.nS + i * T + t       # noqa: E731
        Di = lambda t: self.nS + 2 * T + t          # noqa: E731
        self.Ui, self.Di = Ui, Di
        # quadratic cost rows: f = sum_k 0.5 w_k (row_k)^2 + q . x
        idx, c, rh, rl, w = [], [], [], [], []

        def row(ii, cf, r, wt, r_lo=0.0):
            ii, cf = list(ii) + [0] * (3 - len(ii)), list(cf) + [0.0] * (3 - len(cf))
            idx.append(ii); c.append(cf); rh.append(r); rl.append(r_lo); w.append(wt)
        wr = [1.0, 1.0, 0.0 if dyn == 2 else 1.0]
        for r in range(3):
            if wr[r]:
                for t in range(T + 1):
                    row([S(r, t)], [1.0], ref[r, t], 2 * cfg.ws * wr[r])
        for t in range(T):
            row([Ui(0, t)], [1.0], float(si["vref"]), 2 * cfg.wu)
            for i in range(2):
                row([Ui(i, t)], [1.0], 0.0, cfg.eps_u)
        # rotation rows, vectorised over (n, t, j): g_j + k0_j + k1_j (S2 - ph) = k1_j S2 - (k1_j ph - g_j - k0_j), the constant in double-double
        ph = nom_s[2, :T]
        cs, sn = np.cos(ph), np.sin(ph)
        k0 = np.stack([a[..., 0] * cs + a[..., 1] * sn, -a[..., 0] * sn + a[..., 1] * cs], -1)          # a @ R(ph)
        k1 = np.stack([-a[..., 0] * sn + a[..., 1] * cs, -a[..., 0] * cs - a[..., 1] * sn], -1)         # a @ dR(ph)
        ph3 = np.broadcast_to(ph[None, :, None], k1.shape)
        r_h, r_l = _two_prod(k1, ph3)
        r_h, r_l = dd_add(r_h, r_l, -g, np.zeros_like(g))
        r_h, r_l = dd_add(r_h, r_l, -k0, np.zeros_like(k0))
        col = np.broadcast_to(np.array([S(2, t + 1) for t in range(T)], np.int64)[None, :, None], k1.shape)
        K = k1.size
        idx_r = np.zeros((K, 3), np.int64); idx_r[:, 0] = col.ravel()
        c_r = np.zeros((K, 3)); c_r[:, 0] = k1.ravel()
        idx = np.vstack([np.array(idx, np.int64).reshape(-1, 3), idx_r]); c = np.vstack([np.array(c, float).reshape(-1, 3), c_r])
        rh = np.r_[rh, r_h.ravel()]; rl = np.r_[rl, r_l.ravel()]; w = np.r_[w, np.full(K, float(cfg.ro2))]
        self.cost = _Rows(idx, c, rh, rl)
        self.w = np.array(w)
        self.q = np.zeros(n)
        self.q[[Di(t) for t in range(T)]] = -cfg.slack_gain
        # hinge rows Im = a . S[0:2, t+1] - D[t] - cc
        tt = np.tile(np.arange(T), N)
        hi = np.stack([S(0, tt + 1), S(1, tt + 1), Di(tt)], -1).reshape(N * T, 3)
        hc = np.concatenate([a.reshape(N * T, 2), -np.ones((N * T, 1))], 1)
        self.hinge = _Rows(hi, hc, cc.reshape(N * T))
        # equality rows
        ei, ec, er = [], [], []
        for r in range(3):
            ei.append([S(r, 0)] + [0] * 5); ec.append([1.0] + [0.0] * 5); er.append(nom_s[r, 0])
        for t in range(T):
            A, B, Cc = lin(dyn, nom_s[:, t], nom_u[:, t], cfg.dt, cfg.L)
            for r in range(3):
                ei.append([S(r, t + 1), S(0, t), S(1, t), S(2, t), Ui(0, t), Ui(1, t)])
                ec.append([1.0, -A[r, 0], -A[r, 1], -A[r, 2], -B[r, 0], -B[r, 1]]); er.append(Cc[r])
        self.eq = _Rows(ei, ec, er)
        # inequality rows C x <= e: speed, rate, distance
        ii, ic, ie, self.kind = [], [], [], []
        ms, ab = [float(cfg.max_speed[0]), float(cfg.max_speed[1])], [float(cfg.acce_bound[0]), float(cfg.acce_bound[1])]
        for t in range(T):
            for i in range(2):
                for sg in (1.0, -1.0):
                    ii.append([Ui(i, t), 0]); ic.append([sg, 0.0]); ie.append(ms[i]); self.kind.append(f"speed{i}")
        for t in range(T - 1):
            for i in range(2):
                for sg in (1.0, -1.0):
                    ii.append([Ui(i, t + 1), Ui(i, t)]); ic.append([sg, -sg]); ie.append(ab[i]); self.kind.append(f"rate{i}")
        for t in range(T):
            ii.append([Di(t), 0]); ic.append([1.0, 0.0]); ie.append(float(cfg.max_sd)); self.kind.append("max_sd")
            ii.append([Di(t), 0]); ic.append([-1.0, 0.0]); ie.append(-float(cfg.min_sd)); self.kind.append("min_sd")
        self.ineq = _Rows(ii, ic, ie) if ie else _Rows(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))
        self.mc = len(ie)
        self.Ceq, self.Cin = self.eq.dense(n), self.ineq.dense(n)
        # float64 Hessians: without hinge terms, and one column block per hinge row
        H0 = np.zeros((n, n))
        ci, cv = self.cost.idx, self.cost.c * np.sqrt(self.w)[:, None]
        np.add.at(H0, (np.repeat(ci, 3, axis=1).ravel(), np.tile(ci, (1, 3)).ravel()), (cv[:, :, None] * cv[:, None, :]).reshape(-1))
        self.H0 = H0

    # ---- pieces in double-double -------------------------------------------------------------------------------------------------------------------
    def _grad(self, xh, xl, pat):
        """gradient of the cost with hinge pattern `pat`, dd"""
        vh, vl = self.cost.value(xh, xl)
        vh, vl = dd_mul(vh, vl, self.w, np.zeros_like(self.w))
        th, tl = dd_mul(np.repeat(vh[:, None], 3, 1), np.repeat(vl[:, None], 3, 1), self.cost.c, np.zeros_like(self.cost.c))
        idx = [self.cost.idx]; TH = [th]; TL = [tl]
        if self.N:
            on = pat.astype(float) * self.cfg.ro1
            ih, il = dd_mul(*self.hinge.value(xh, xl), on, np.zeros_like(on))
            th, tl = dd_mul(np.repeat(ih[:, None], 3, 1), np.repeat(il[:, None], 3, 1), self.hinge.c, np.zeros_like(self.hinge.c))
            idx.append(self.hinge.idx); TH.append(th); TL.append(tl)
        idx.append(np.arange(self.n)[:, None]); TH.append(self.q[:, None]); TL.append(np.zeros((self.n, 1)))
        gi = np.concatenate([i.reshape(-1) for i in idx])
        return _scatter(self.n, gi, np.concatenate([t.reshape(-1) for t in TH]), np.concatenate([t.reshape(-1) for t in TL]))

    def _ct_mult(self, rows, mh, ml):
        th, tl = dd_mul(np.repeat(mh[:, None], rows.idx.shape[1], 1), np.repeat(ml[:, None], rows.idx.shape[1], 1), rows.c, np.zeros_like(rows.c))
        return _scatter(self.n, rows.idx.reshape(-1), th.reshape(-1), tl.reshape(-1))

    def f_dd(self, xh, xl=None):
        """objective (hinge terms by their true sign), dd"""
        xl = np.zeros_like(xh) if xl is None else xl
        vh, vl = self.cost.value(xh, xl)
        sh, sl = dd_mul(vh, vl, vh, vl)
        sh, sl = dd_mul(sh, sl, 0.5 * self.w, np.zeros_like(self.w))
        parts_h, parts_l = [sh], [sl]
        if self.N:
            ih, il = self.hinge.value(xh, xl)
            on = np.ones_like(ih) if not self.acc else (ih < 0).astype(float)
            hh, hl = dd_mul(ih, il, ih, il)
            hh, hl = dd_mul(hh, hl, 0.5 * self.cfg.ro1 * on, np.zeros_like(on))
            parts_h.append(hh); parts_l.append(hl)
        qh, ql = dd_mul(xh, xl, self.q, np.zeros_like(self.q))
        parts_h.append(qh); parts_l.append(ql)
        return dd_sum(np.concatenate(parts_h), np.concatenate(parts_l))

    def unpack(self, x):
        T = self.T
        return x[:self.nS].reshape(3, T + 1), x[self.nS:self.nS + 2 * T].reshape(2, T), x[self.nS + 2 * T:]

    def rollout_dd(self, U, D):
        """the feasible point of the controls U and distances D: states rolled out through the dynamics in dd"""
        T = self.T
        xh = np.r_[np.zeros(self.nS), np.asarray(U, float).ravel(), np.asarray(D, float).ravel()]
        xl = np.zeros(self.n)
        for r in range(3):
            xh[r * (T + 1)] = self.eq.rh[r]
        for t in range(T):
            for r in range(3):
                k = 3 + 3 * t + r
                ph, pl = dd_mul(xh[self.eq.idx[k, 1:]], xl[self.eq.idx[k, 1:]], -self.eq.c[k, 1:], np.zeros(5))
                vh, vl = dd_sum(ph, pl)
                vh, vl = dd_add(vh, vl, self.eq.rh[k], self.eq.rl[k])
                xh[r * (T + 1) + t + 1], xl[r * (T + 1) + t + 1] = vh, vl
        return xh, xl

    # ---- the KKT solve for one (active set, hinge pattern) ----------------------------------------------------------------------------------------
    def _hessian(self, pat):
        H = self.H0.copy()
        if self.N and pat.any():
            ci, cv = self.hinge.idx[pat], self.hinge.c[pat] * np.sqrt(self.cfg.ro1)
            np.add.at(H, (np.repeat(ci, 3, axis=1).ravel(), np.tile(ci, (1, 3)).ravel()), (cv[:, :, None] * cv[:, None, :]).reshape(-1))
        return H

    def _kkt(self, act, pat, refine=3):
        n, me = self.n, len(self.eq.rh)
        ia = np.flatnonzero(act)
        H = self._hessian(pat)
        Ca = self.Cin[ia]
        m = me + len(ia)
        K = np.zeros((n + m, n + m))
        K[:n, :n] = H
        K[:n, n:n + me] = self.Ceq.T; K[n:n + me, :n] = self.Ceq
        K[:n, n + me:] = Ca.T; K[n + me:, :n] = Ca
        try:
            lu = np.linalg.inv(K)
        except np.linalg.LinAlgError:
            return None
        zh, zl = np.zeros(n + m), np.zeros(n + m)
        for _ in range(refine + 1):
            r = self._residual(zh, zl, ia, pat)
            dz = -(lu @ r[0])
            dz = dz - lu @ (K @ dz + r[0])          # one float64 correction of the correction
            zh, zl = dd_add(zh, zl, dz, np.zeros_like(dz))
        return zh, zl, ia, H

    def _residual(self, zh, zl, ia, pat):
        n, me = self.n, len(self.eq.rh)
        xh, xl = zh[:n], zl[:n]
        gh, gl = self._grad(xh, xl, pat)
        sh, sl = dd_add(gh, gl, *self._ct_mult(self.eq, zh[n:n + me], zl[n:n + me]))
        if len(ia):
            sub = _Rows(self.ineq.idx[ia], self.ineq.c[ia], self.ineq.rh[ia])
            sh, sl = dd_add(sh, sl, *self._ct_mult(sub, zh[n + me:], zl[n + me:]))
            ah, al = sub.value(xh, xl)
        else:
            ah, al = np.zeros(0), np.zeros(0)
        eh, el = self.eq.value(xh, xl)
        rh = np.r_[sh, eh, ah]
        return rh + np.r_[sl, el, al], gh

    def _pin_free_distances(self, act, pat):
        """a stage without a hinge term in the pattern has D[t] in the cost through -slack_gain D[t] only (no curvature): it sits on a bound"""
        T = self.T
        on = pat.reshape(self.N, T).any(axis=0) if self.N else np.zeros(T, bool)
        base = 4 * T + 4 * (T - 1)
        for t in np.flatnonzero(~on):
            if not (act[base + 2 * t] or act[base + 2 * t + 1]):
                act[base + 2 * t + (0 if self.cfg.slack_gain >= 0 else 1)] = True

    def _independent(self, act):
        Q = np.linalg.qr(self.Ceq.T)[0]
        for i in np.flatnonzero(act):
            v = self.Cin[i] - Q @ (Q.T @ self.Cin[i])
            if np.linalg.norm(v) < 1e-9:
                act[i] = False
            else:
                Q = np.column_stack([Q, v / np.linalg.norm(v)])

    # ---- search + certificate ----------------------------------------------------------------------------------------------------------------------
    def solve(self, start=None, max_rounds=60):
        """certified optimum; start: (s, u, d) whose near-active rows / hinge pattern seed the search (default: the nominal).  A seed that is only
        approximately optimal is read at several widths: rows within 1e-9, 1e-5, 1e-3 of their bounds"""
        err = None
        for width in ((1e-9, 1e-5, 1e-3) if start is not None else (1e-9,)):
            try:
                return self._solve(start, max_rounds, width)
            except RuntimeError as e:
                err = e
        raise err

    def _solve(self, start, max_rounds, width):
        """certified optimum.  start: optional (s, u, d) whose active set / hinge pattern seeds the search (the default seed is the nominal)"""
        T, N = self.T, self.N
        if start is None:
            ms = np.array([float(self.cfg.max_speed[0]), float(self.cfg.max_speed[1])])[:, None]
            x0 = self.rollout_dd(np.clip(self.nom_u, -ms, ms), np.full(T, float(self.cfg.max_sd)))[0]
        else:
            s, u, d = start
            x0 = np.r_[np.asarray(s, float).ravel(), np.asarray(u, float).ravel(), np.asarray(d, float).ravel()]
        pat = (self.hinge.value(x0, np.zeros(self.n))[0] < (0 if width < 1e-6 else width)) if self.acc else np.ones(N * T, bool)
        cx = self.Cin @ x0 - self.ineq.rh if self.mc else np.zeros(0)
        act = cx > -width
        seen, why = set(), ""
        for rnd in range(max_rounds):
            key = (act.tobytes(), pat.tobytes())
            single = key in seen or None in seen  # the set has been here before: move only the worst offender from now on
            seen.add(key)
            self._pin_free_distances(act, pat)
            out = self._kkt(act, pat)
            if out is None:                       # rows moved in together that are linearly dependent: keep an independent subset
                self._independent(act)
                out = self._kkt(act, pat)
            if out is None:
                why = "singular KKT matrix"
                break
            zh, zl, ia, H = out
            n, me = self.n, len(self.eq.rh)
            xh, xl = zh[:n], zl[:n]
            nu = np.zeros(self.mc); nu[ia] = zh[n + me:]
            cx = self.ineq.value(xh, xl)[0] if self.mc else np.zeros(0)
            im = self.hinge.value(xh, xl)[0] if N else np.zeros(0)
            r, gh = self._residual(zh, zl, ia, pat)
            stat = np.abs(r[:n]).max() / (1 + np.abs(gh).max())
            feas = max(np.abs(r[n:]).max(initial=0), cx[~act].max(initial=-1))
            viol_in = np.where(~act, cx, -np.inf)             # rows to move in
            viol_out = np.where(act, -nu, -np.inf)            # rows to move out
            hin = np.where(~pat, -im, -np.inf) if self.acc else np.full(N * T, -np.inf)      # pattern rows to add (Im < 0 outside)
            hout = np.where(pat, im, -np.inf) if self.acc else np.full(N * T, -np.inf)       # ... to drop (Im > 0 inside)
            ok = (feas <= FEAS_TOL and viol_out.max(initial=-1) <= MULT_TOL and hin.max(initial=-1) <= HINGE_TOL and hout.max(initial=-1) <= HINGE_TOL
                  and stat <= STAT_TOL)
            if ok:
                return Certificate(self, xh, xl, zh[n:n + me], nu, act.copy(), pat.copy(), H, rnd + 1)
            cand = [(viol_in.max(initial=-np.inf), 0), (viol_out.max(initial=-np.inf), 1), (hin.max(initial=-np.inf), 2), (hout.max(initial=-np.inf), 3)]
            if single:
                v, k = max(cand)
                if v <= 0:
                    why = f"no row to move (stationarity {stat:.1e}, feasibility {feas:.1e})"
                    break
                arr = [viol_in, viol_out, hin, hout][k]
                j = int(np.argmax(arr))
                if k < 2:
                    act[j] = not act[j]
                else:
                    pat[j] = not pat[j]
            else:
                act = (act & (nu > -MULT_TOL)) | (~act & (cx > FEAS_TOL))
                if self.acc:
                    pat = np.where(pat, im <= HINGE_TOL, im < -HINGE_TOL)
                if (act.tobytes(), pat.tobytes()) == key:
                    seen.add(None)
        raise RuntimeError(f"su_kkt: no certified optimum ({why or 'round limit'}; T={T} N={N})")


class Certificate:
    """a certified optimum: x* (s, u, d) with multipliers, active set, hinge pattern, the smallest curvature m on the active face and f(x*)"""

    def __init__(self, P, xh, xl, lam, nu, act, pat, H, rounds):
        self.P, self.xh, self.xl, self.lam, self.nu, self.active, self.pattern, self.rounds = P, xh, xl, lam, nu, act, pat, rounds
        self.s, self.u, self.d = (v.copy() for v in P.unpack(xh))
        fh, fl = P.f_dd(xh, xl)
        self.f_star = (float(fh), float(fl))
        # reduced Hessian on the null space of the equality rows and the active rows
        C = np.vstack([P.Ceq, P.Cin[act]])
        _, sv, Vt = np.linalg.svd(C)
        rank = int((sv > 1e-12 * sv.max()).sum())
        Z = Vt[rank:].T
        self.m = float(np.linalg.eigvalsh(Z.T @ H @ Z).min()) if Z.shape[1] else np.inf
        # slack_gain = 0: a stage without hinge terms in the pattern has d free between its bounds (pinned on max_sd by the search): not unique
        free_d = P.cfg.slack_gain == 0 and (not P.N or not pat.reshape(P.N, P.T).any(axis=0).all())
        self.unique = self.m > M_SINGULAR and not free_d
        self.active_rows = {k: int(sum(1 for i in np.flatnonzero(act) if P.kind[i] == k)) for k in sorted(set(P.kind))}

    def distance(self, s, u, d):
        """max-norm distance of a candidate to x* in s, u and d"""
        return max(float(np.abs(np.asarray(s).reshape(self.s.shape) - self.s).max()), float(np.abs(np.asarray(u).reshape(self.u.shape) - self.u).max()),
                   float(np.abs(np.asarray(d).ravel() - self.d).max()) if self.d.size else 0.0)

    def gap(self, u, d):
        """f(x) - f(x*) in dd, x = the candidate's controls and distances with the states rolled out exactly; and the candidate's bound violation"""
        xh, xl = self.P.rollout_dd(u, d)
        fh, fl = self.P.f_dd(xh, xl)
        gh, gl = dd_add(fh, fl, -self.f_star[0], -self.f_star[1])
        viol = float((self.P.Cin @ xh - self.P.ineq.rh).max(initial=0))
        return float(gh) + float(gl), max(viol, 0.0)

    def bound(self, u, d):
        """||x - x*|| <= sqrt(2 (f(x) - f(x*)) / m) for a feasible candidate on the certified face"""
        g, _ = self.gap(u, d)
        return float(np.sqrt(2 * max(g, 0.0) / self.m)) if self.m > 0 else np.inf


def certify(cfg, si, start=None):
    """certified optimum of the su-problem (cfg, si); start: optional (s, u, d) that seeds the active-set search - any point will do, the
    candidate under test included: a wrong seed does not certify, it raises"""
    return SuProblem(cfg, si).solve(start=start)


def su_inputs_from_state(st, nom_s, nom_u, ref, speed, G, h, d0=None):
    """the su-problem an ADMM iteration solves, rebuilt from a handle's state (rda_get_state / orc_get_state) - the formula of
    oracle/ref_harness.py::su_inputs_from_reference: a = a_lam[:, 1:], cc = b_lam[:, 1:] + mu[:, 1:] h + z - zeta, g = mu[:, 1:] G + xi[:, 1:];
    (nom_s, nom_u) the (s, u) of the previous ADMM iteration (of the step's nominal for the first), d0 = dis.  Sums in the order the solvers form them."""
    mu, R = st["mu"][:, 1:], len(h)
    muh = np.zeros(mu.shape[:2])
    g = st["xi"][:, 1:].copy()
    for j in range(R):
        muh = muh + mu[..., j] * h[j]
        g[..., 0] = g[..., 0] + mu[..., j] * G[j, 0]
        g[..., 1] = g[..., 1] + mu[..., j] * G[j, 1]
    cc = st["b_lam"][:, 1:] + ((muh + st["z"]) - st["zeta"])
    T = st["dis"].shape[0]
    return dict(nom_s=np.ascontiguousarray(nom_s, float).reshape(3, T + 1), nom_u=np.ascontiguousarray(nom_u, float).reshape(2, T),
                ref=np.ascontiguousarray(ref, float).reshape(3, T + 1), vref=float(speed), a=np.ascontiguousarray(st["a_lam"][:, 1:]),
                cc=np.ascontiguousarray(cc), g=np.ascontiguousarray(g), d0=np.ascontiguousarray(st["dis"] if d0 is None else d0, float))
