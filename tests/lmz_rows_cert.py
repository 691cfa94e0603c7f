"""TEST INFRASTRUCTURE: an optimality certificate for ONE row of the default LamMuZ mode (support enumeration, tie-breaks T1 - T3, remembered
supports), evaluated on the duals (lam, mu, z) a solver returned.  numpy, scipy and the standard library only; nothing of oracle/ or of the product is
imported, and of tests/lmz_central_ref.py only the `Row` / `StateRow` tuples, the geometry helpers and the epilogue identities - not its solver.  There is
no solver here at all: no enumeration of supports, no closed forms of a candidate, none of the tie-break code.  A point is judged, never computed.

THE PROBLEM of a row (header of csrc/lammuz_device.h, docstring of oracle/lammuz_np.py), z eliminated:

    f_delta(lam, mu) = 1/2 neg(m)^2 - delta m + 1/2 ro2 |H|^2 ,    m = lam'q - mu'h + zeta - dbar ,    H = M'lam + G'mu + xi ,    delta = 1e-6
    over  lam in K_obs ,  |A'lam| <= 1 ,  mu >= 0 ;      q = A p - b ,  M = A Rot(phi) ,  a = A'lam

K_obs of a polygon is lam >= 0 with the multiplier of a zero-padded edge row (A_i = 0, b_i = 0) held at exactly 0; of a circle it is
lam = (a, lam_2 <= -|a|, 0 ..) and the optimum has lam_2 = -|a| (its cost gradient g_m r is negative).  f_delta is convex, so a feasible point is optimal
iff it satisfies the KKT conditions, and those are checked on the returned point alone, in np.longdouble.  With g_m = min(m, 0) - delta,
grad_lam = g_m q + ro2 M H and grad_mu = -g_m h + ro2 G H, a row PASSES when it meets criterion A or criterion B, and T2.

CRITERION A - the optimum of f_delta.  Feasible: lam_i >= 0 (polygon) or lam_2 = -|a| (circle), padded multipliers exactly 0, |a| <= 1, mu_j >= 0
(figure `feas`: the largest violation, absolute).  Stationary (figure `kkt`: the largest of the residuals below, divided by 1 + |g_m| max(|q|, |h|)):
    mu:       grad_mu >= 0 ,  grad_mu o mu = 0
    polygon:  a nu >= 0 with  sigma = grad_lam + nu A a^ >= 0 ,  sigma o lam = 0 ,  nu (1 - |a|) = 0 ;  nu is the least-squares fit of sigma = 0 on
              the support {lam_i > 0}, clipped at 0 (a^ = a / |a|; nu = 0 where a = 0)
    circle:   the reduced gradient r = grad_lam[:2] - grad_lam[2] a^ of a -> f(a, -|a|) has no tangential part; its radial part is <= 0 and vanishes
              unless |a| = 1 (radial (1 - |a|) = 0); at a = 0, where the reduced cost has a kink, |grad_lam[:2]| <= -grad_lam[2]

CRITERION B - the slack regime, tie-break T1.  The point is optimal for the reference's own problem (delta = 0): feasible as above, m >= 0 (figure
`m_neg`) and H = 0 (figure `H`), both in units of eps x the sum of the absolute values of their elementary products and addends, and |a| = 1 (within
the bound of `feas`).  And its normal is the MIDDLE of the arc of separating directions, located independently: for a unit a(theta) let m(theta) be the largest
lam'q - mu'h + zeta - dbar over the duals that support it with H = 0 - two small LPs (scipy.optimize.linprog): over lam >= 0 with A'lam = a, and over
mu >= 0 with G'mu = -Rot(phi)'a - xi; a circle obstacle contributes the closed form a'(p - c) - r instead of the first.  The ends of the arc are the
first sign changes of m(theta) on either side of the returned direction (a scan in steps of pi / 12, then a bracketing root finder); the two
half-widths must agree (figure `arc`, radians).  No vertex enumeration, none of central_normal's vertex-pair formulas.

T2, both criteria: z = 1/2 max(m, 0) accelerated, max(m, 0) otherwise, m evaluated in longdouble on the returned (lam, mu) (figure `z`, in units of
eps x the summed terms of m).

COVERAGE CONDITIONS (not tolerances; tests/test_lmz_rows_cert.py and tests/test_gpu_lmz_rows_cert.py assert them):
  - every row of a launch without failed rows passes A or B; only a slot that was made non-finite on purpose is left out;
  - centring is not quietly dropped: a row that passes only A although it meets the documented trigger of T1 (m > 0, |H|^2 < 1e-8, |a|^2 >= 1 - 1e-9,
    tie_centre = 1) must be a row whose LP arc around its own normal is IMPROPER - m(theta) < 0 at that normal, or no finite end within pi on one side;
  - both classes are present in every case that can have both;
  - the epilogue identities (lmz_central_ref.epilogue_errors: xi', zeta', condensed A'lam and lam'b, 4 ulp) hold on the returned duals.

BOUNDS.  ORACLE_WORST below is the worst value of each figure over the answers of the numpy oracle (oracle/lammuz_np.py) and of the C oracle's per-row
solve (orc_lammuz_one) on the pinned grid of tests/test_lmz_rows_cert.py, as that test prints them, rounded up.  A kernel is held to 10 x that
(`bound`; the convention of lmz_central_ref.gpu_bound: measured on the oracle, never on a kernel; the factor covers another order of evaluation and
fused multiply-adds).  Each bound stays >= 5 x below the smallest figure of the wrong answers of the same test (the optimum of a neighbouring problem,
the delta = 0 optimum, the un-centred answer, a normal rotated by 1e-6 rad, the wrong z)."""
from collections import namedtuple

import numpy as np
from scipy.optimize import brentq, linprog

import lmz_central_ref as ref
from lmz_central_ref import LD, EPS

DELTA = 1e-6
TRIGGER_H2, TRIGGER_A2 = 1e-8, 1.0 - 1e-9          # the documented trigger of tie-break T1 (with m > 0)
SCAN = np.pi / 12                                   # the scan step of the arc search
LP_OPTIONS = {"presolve": False}                    # (two-row LPs: the presolve costs more than it saves)
ARC_ROWS = 24                                       # centred rows per case whose arc is located

# worst figures of the two oracles on the pinned grid (tests/test_lmz_rows_cert.py::test_oracle_figures_on_the_pinned_grid prints them), rounded up
ORACLE_WORST = {"feas": 2.7e-16, "kkt": 1.4e-14, "H": 0.95, "arc": 1.8e-15, "z": 0.8}


def bound(key):
    """the bound of a kernel's figure: 10 x the oracles' recorded worst; m >= 0 of criterion B is held exactly (both oracles: 0)"""
    return 0.0 if key == "m_neg" else 10.0 * ORACLE_WORST[key]


Cert = namedtuple("Cert", "cls why fig trigger")      # cls "A" | "B" | None ;  fig: the figures that were evaluated ;  trigger: the row meets T1's trigger


def _point(row, lam, mu):
    A, b, q, M = ref._geometry(row)
    G, h, xi = np.asarray(row.G, LD).reshape(row.R, 2), np.asarray(row.h, LD).ravel(), np.asarray(row.xi, LD).ravel()
    lam, mu = np.asarray(lam, LD).ravel(), np.asarray(mu, LD).ravel()
    m = lam @ q - mu @ h + LD(row.zeta) - LD(row.dbar)
    H = M.T @ lam + G.T @ mu + xi
    return A, b, q, M, G, h, xi, lam, mu, m, H, A.T @ lam


def live_rows(row):
    """the edge rows of a polygon that are no zero padding"""
    A, b = np.asarray(row.A, float).reshape(row.E, 2), np.asarray(row.b, float).ravel()
    return np.array([bool(np.any(A[i] != 0) or b[i] != 0) for i in range(row.E)])


def feasibility(row, lam, mu):
    """(largest violation of the cone, norm and sign constraints, padded multipliers exactly zero, |a|)"""
    *_, lam, mu, m, H, a = _point(row, lam, mu)
    na = np.sqrt(a @ a)
    v = [max(na - 1, LD(0)), max((-mu).max(), LD(0))]
    if row.cone_norm2:
        v.append(abs(lam[2] + np.sqrt(lam[0] * lam[0] + lam[1] * lam[1])))
        exact = bool(np.all(lam[3:] == 0))
    else:
        live = live_rows(row)
        v.append(max((-lam).max(), LD(0)))
        exact = bool(np.all(lam[~live] == 0))
    return float(max(v)), exact, float(na)


def criterion_a(row, lam, mu, delta=DELTA):
    """the scaled KKT residual of (lam, mu) for f_delta (the figure `kkt`)"""
    A, b, q, M, G, h, xi, lam, mu, m, H, a = _point(row, lam, mu)
    gm = min(m, LD(0)) - LD(delta)
    ro2 = LD(row.ro2)
    gl, gu = gm * q + ro2 * (M @ H), -gm * h + ro2 * (G @ H)
    scale = 1 + abs(gm) * max(np.abs(q).max(), np.abs(h).max())
    na = np.sqrt(a @ a)
    res = [max((-gu).max(), LD(0)), np.abs(gu * mu).max()]
    gap = max(1 - na, LD(0))
    if row.cone_norm2:
        if na > 0:
            ah = a / na
            r = gl[:2] - gl[2] * ah
            rad, tan = r @ ah, -r[0] * ah[1] + r[1] * ah[0]
            res += [abs(tan), max(rad, LD(0)), abs(rad) * gap]
        else:
            res.append(max(np.sqrt(gl[:2] @ gl[:2]) + gl[2], LD(0)))
    else:
        live = live_rows(row)
        nu = LD(0)
        c = np.zeros(row.E, LD)
        if na > 0:
            c = A @ (a / na)
            sup = lam > 0
            if sup.any() and (c[sup] @ c[sup]) > 0:
                nu = max(-(gl[sup] @ c[sup]) / (c[sup] @ c[sup]), LD(0))
        sig = gl + nu * c
        res += [max((-sig[live]).max(), LD(0)) if live.any() else LD(0), np.abs(sig * lam).max(), nu * gap]
    return float(max(res) / scale)


def slack_figures(row, lam, mu):
    """criterion B without the arc: (m_neg, H) in units of eps x their summed terms"""
    *_, lam, mu, m, H, a = _point(row, lam, mu)
    _, imag, _ = ref.Im_terms(row, lam, mu)
    _, hmag, _ = ref.Hm_terms(row, lam, mu)
    m_neg = float(max(-m, LD(0)) / (EPS * (imag + abs(LD(row.zeta)) + abs(LD(row.dbar)))))
    den = EPS * (hmag + np.abs(np.asarray(row.xi, LD).ravel()))
    Hrel = float(max(abs(H[k]) / den[k] if den[k] > 0 else (np.inf if H[k] != 0 else 0.0) for k in range(2)))      # (a component without terms is exactly 0)
    return m_neg, Hrel


def t2_error(row, lam, mu, z):
    """|z - T2(m)| in units of eps x the summed terms of m"""
    *_, m, H, a = _point(row, lam, mu)
    _, imag, _ = ref.Im_terms(row, lam, mu)
    want = (LD(0.5) if row.accelerated else LD(1)) * max(m, LD(0))
    return float(abs(LD(z) - want) / (EPS * (imag + abs(LD(row.zeta)) + abs(LD(row.dbar)))))


def trigger(row, lam, mu):
    """the documented trigger of tie-break T1 at this point"""
    *_, m, H, a = _point(row, lam, mu)
    return bool(m > 0 and H @ H < TRIGGER_H2 and a @ a >= TRIGGER_A2)


# ---- the arc of separating directions, by two LPs per direction -------------------------------------------------------------------------------
def lp_duals(row, th):
    """(m, lam, mu): the duals that support the unit normal a(th) with H = 0 and the largest m, or (-inf, None, None) when there are none"""
    A, b = np.asarray(row.A, float).reshape(row.E, 2), np.asarray(row.b, float).ravel()
    G, h, xi, p = np.asarray(row.G, float).reshape(row.R, 2), np.asarray(row.h, float).ravel(), np.asarray(row.xi, float).ravel(), np.asarray(row.p, float).ravel()
    a = np.array([np.cos(th), np.sin(th)])
    c, s = np.cos(row.phi), np.sin(row.phi)
    lam = np.zeros(row.E)
    if row.cone_norm2:
        lam[0], lam[1], lam[2] = a[0], a[1], -1.0
        mo = a @ (p - b[:2]) + b[2]                                   # a'(p - c) - r
    else:
        live = live_rows(row)
        q = A @ p - b
        r = linprog(-q[live], A_eq=A[live].T, b_eq=a, bounds=(0, None), method="highs", options=LP_OPTIONS)
        if r.status != 0:
            return -np.inf, None, None
        lam[live] = r.x
        mo = -r.fun
    g = -np.array([c * a[0] + s * a[1], -s * a[0] + c * a[1]]) - xi    # G'mu = -Rot(phi)'a - xi
    r = linprog(h, A_eq=G.T, b_eq=g, bounds=(0, None), method="highs", options=LP_OPTIONS)
    if r.status != 0:
        return -np.inf, None, None
    return float(mo - r.fun + row.zeta - row.dbar), lam, np.asarray(r.x, float)


def arc(row, th):
    """the half-widths (up, down) of the arc {m(theta) >= 0} around th, or a string saying why the arc is improper"""
    f = lambda t: lp_duals(row, t)[0]
    if not f(th) >= 0:
        return "m < 0 at the normal"
    out = []
    for sg in (1.0, -1.0):
        lo = 0.0
        for k in range(1, 13):
            hi = k * SCAN
            if f(th + sg * hi) < 0:
                if out and lo < out[0] - 1e-6 and out[0] + 1e-6 < hi and f(th + sg * (out[0] - 1e-6)) >= 0 and f(th + sg * (out[0] + 1e-6)) < 0:
                    lo, hi = out[0] - 1e-6, out[0] + 1e-6          # (the other side's end lies in this bracket too: start the root finder there)
                out.append(brentq(lambda t: f(th + sg * t), lo, hi, xtol=1e-15, rtol=8.9e-16))
                break
            lo = hi
        else:
            return "no finite end within pi"
    return tuple(out)


def arc_error(row, lam):
    """|up - down| of the arc around the direction of a = A'lam (the figure `arc`), or the reason why there is none"""
    a = np.asarray(row.A, float).reshape(row.E, 2).T @ np.asarray(lam, float).ravel()
    w = arc(row, float(np.arctan2(a[1], a[0])))
    return w if isinstance(w, str) else abs(w[0] - w[1])


# ---- the verdict on one row ------------------------------------------------------------------------------------------------------------------------
def _judge(row, lam, mu, z, with_arc, tie_centre, delta):
    """(figures, trigger, excess under criterion A, excess under criterion B, reasons).  An excess is the largest figure of the criterion in units of its
    bound, T2 and feasibility included; inf for a violated condition that is no figure, and for criterion B when A already holds (A is tried first)."""
    fig, why, inf = {}, [], float("inf")
    lam, mu = np.asarray(lam, float).ravel(), np.asarray(mu, float).ravel()
    if not (np.isfinite(lam).all() and np.isfinite(mu).all() and np.isfinite(z)):
        return fig, False, inf, inf, ["non-finite duals"]
    fig["feas"], exact, na = feasibility(row, lam, mu)
    fig["z"] = t2_error(row, lam, mu, z)
    trig = trigger(row, lam, mu)
    common = max(fig["feas"] / bound("feas"), fig["z"] / bound("z")) if exact else inf
    if not exact:
        why.append("a padded multiplier is not exactly 0")
    if not fig["feas"] <= bound("feas"):
        why.append(f"infeasible by {fig['feas']:.2e}")
    if not fig["z"] <= bound("z"):
        why.append(f"T2: z off by {fig['z']:.2f} eps of the summed terms")
    fig["kkt"] = criterion_a(row, lam, mu, delta)
    ex_a = max(common, fig["kkt"] / bound("kkt"))
    if ex_a <= 1:
        w = arc_error(row, lam) if trig and tie_centre else ""
        if isinstance(w, str):
            return fig, trig, ex_a, inf, why
        ex_a = inf
        why.append(f"A: T1's trigger is met and the arc around the normal is proper (half-widths differ by {w:.2e}): not centred")
    elif not fig["kkt"] <= bound("kkt"):
        why.append(f"A: KKT residual {fig['kkt']:.2e}")
    fig["m_neg"], fig["H"] = slack_figures(row, lam, mu)
    ex_b = max(common, 0.0 if fig["m_neg"] == 0 else float("inf"), fig["H"] / bound("H"), abs(na - 1.0) / bound("feas"))
    if not fig["m_neg"] <= bound("m_neg"):
        why.append(f"B: m < 0 by {fig['m_neg']:.3g} eps of its terms")
    if not fig["H"] <= bound("H"):
        why.append(f"B: |H| is {fig['H']:.3g} eps of its terms")
    if not abs(na - 1.0) <= bound("feas"):
        why.append(f"B: |a| - 1 = {na - 1.0:.2e}")
    if ex_b <= 1 and with_arc:
        w = arc_error(row, lam)
        if isinstance(w, str):
            ex_b = inf
            why.append(f"B: improper arc ({w})")
        else:
            fig["arc"] = w
            ex_b = max(ex_b, w / bound("arc"))
            if not w <= bound("arc"):
                why.append(f"B: the half-widths of the arc differ by {w:.2e}")
    return fig, trig, ex_a, ex_b, why


def certify(row, lam, mu, z, with_arc=True, tie_centre=1, delta=DELTA):
    """Cert of the answer (lam, mu, z) to `row`.  cls is "A" or "B" when the row passes (criterion A is tried first), None with `why` otherwise.  The arc of
    a class-B row is located only `with_arc`; the LP arc of a class-A row that meets T1's trigger is always looked at."""
    fig, trig, ex_a, ex_b, why = _judge(row, lam, mu, z, with_arc, tie_centre, delta)
    if ex_a <= 1:
        return Cert("A", "", fig, trig)
    if ex_b <= 1:
        fig.pop("kkt")                                     # (not a figure of this class)
        return Cert("B", "", fig, trig)
    return Cert(None, "; ".join(why), fig, trig)


def margin(row, lam, mu, z, tie_centre=1):
    """how far outside the certificate an answer lies: its excess under criterion A or under criterion B (arc included), the smaller of the two.
    certify() passes a row iff this is <= 1; the tests of wrong answers measure their distance to the bounds with it."""
    _, _, ex_a, ex_b, _ = _judge(row, lam, mu, z, True, tie_centre, DELTA)
    return min(ex_a, ex_b)


# ---- the rows of a driven loop (lmz_central_ref.StateRow, rebuilt from the handle's state) ----------------------------------------------------------
def check_rows(rows, tag, worst, skip=(), tie_centre=1):
    """every StateRow outside the slots `skip` against the certificate (class-B rows without their arc: `check_arcs` afterwards) and the epilogue
    identities.  worst[...] collects the figures per class, the class counts, worst["bad"] the rows that fail and worst["centred"] the class-B rows."""
    bad, cen = worst.setdefault("bad", []), worst.setdefault("centred", [])
    for sr in rows:
        if sr.n in skip:
            continue
        c = certify(sr.row, sr.lam, sr.mu, sr.z, with_arc=False, tie_centre=tie_centre)
        e_xi, b_xi, e_ze, b_ze, e_c, b_c = ref.epilogue_errors(sr)
        for key, e, b in (("xi", e_xi, b_xi), ("zeta", e_ze, b_ze), ("cond", e_c, b_c)):
            worst[key] = max(worst.get(key, 0.0), e / b if b else e)
        worst["rows"] = worst.get("rows", 0) + 1
        if c.cls is None:
            bad.append((tag, sr.n, sr.t, c.why))
            continue
        worst[c.cls] = worst.get(c.cls, 0) + 1
        for key, v in c.fig.items():
            worst[(c.cls, key)] = max(worst.get((c.cls, key), 0.0), v)
        if c.cls == "B":
            cen.append((tag, sr))
        elif c.trigger and tie_centre:
            worst["triggered"] = worst.get("triggered", 0) + 1          # (at T1's trigger with an improper arc: rightly not centred)
        if c.cls == "A" and not sr.row.cone_norm2 and np.any(sr.lam != 0):      # the composition of class A: polygon rows with duals, ...
            *_, m, _, a = _point(sr.row, sr.lam, sr.mu)
            worst["A_poly"] = worst.get("A_poly", 0) + 1
            if m < 0 and a @ a >= TRIGGER_A2:                                      # ... of them hinge-active with the norm constraint binding, ...
                worst["A_poly_unit"] = worst.get("A_poly_unit", 0) + 1
            if np.count_nonzero(sr.mu) == 2:                                       # ... and with two robot edges in the support (a robot corner)
                worst["A_poly_mu2"] = worst.get("A_poly_mu2", 0) + 1
        if not (e_xi <= b_xi and e_ze <= b_ze and e_c <= b_c):
            bad.append((tag, sr.n, sr.t, f"epilogue: xi {e_xi:.1e} / {b_xi:.1e}, zeta {e_ze:.1e} / {b_ze:.1e}, condensed {e_c:.1e} / {b_c:.1e}"))


def check_arcs(worst, most=ARC_ROWS):
    """the arc of every k-th class-B row that check_rows collected, at most `most` of them"""
    cen = worst.get("centred", [])
    k = max(1, -(-len(cen) // most))
    for tag, sr in cen[::k]:
        w = arc_error(sr.row, sr.lam)
        worst["arcs"] = worst.get("arcs", 0) + 1
        if isinstance(w, str):
            worst["bad"].append((tag, sr.n, sr.t, f"B: improper arc ({w})"))
            continue
        worst[("B", "arc")] = max(worst.get(("B", "arc"), 0.0), w)
        if not w <= bound("arc"):
            worst["bad"].append((tag, sr.n, sr.t, f"B: the half-widths of the arc differ by {w:.2e}"))


def figures(worst):
    g = lambda *k: worst.get(k if len(k) > 1 else k[0], 0)
    return (f"{g('rows')} rows: {g('A')} class A ({g('A_poly')} polygon rows with duals, {g('A_poly_unit')} of them |a| = 1 and m < 0, {g('A_poly_mu2')} on a robot corner; {g('triggered')} at T1's trigger; kkt {g('A', 'kkt'):.2e}, feas {g('A', 'feas'):.1e}, z {g('A', 'z'):.2f}), {g('B')} class B (H {g('B', 'H'):.2f}, "
            f"m_neg {g('B', 'm_neg'):.2f}, feas {g('B', 'feas'):.1e}, z {g('B', 'z'):.2f}, arc {g('B', 'arc'):.2e} on {g('arcs')} rows); epilogue in units of its "
            f"{ref.EPILOGUE_ULPS}-ulp bound: xi {g('xi'):.2f}, zeta {g('zeta'):.2f}, condensed {g('cond'):.2f}")
