"""shared generators / thin wrappers for the tests"""
import ctypes as C

import numpy as np

from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import Cfg, dptr, iptr

# ---- THE stated fp64 tolerance of the closed-loop parity, asserted by every HIP-vs-oracle closed-loop test -----------------------------
# applied control |u_gpu - u_oracle| in the solver's own coordinates (speed [m/s]; steering angle / yaw rate / velocity heading [rad]),
# per MPC step from the same state, on steps whose ADMM iteration counts agree.
# Round 6: both sides LAND the su solve on its vertex (rda_opts::su_land / oracle su_land, default on): the interior point only has to get close
# enough for the active set to be read off, the vertex is then computed exactly and verified on the true objective - the answer no longer depends
# on the interior-point path (cold / warm / easy / hard starts, speculative landings: tests/test_gpu_land.py 7e-15 .. 9e-11 per su-problem).
# Largest value seen against the COLD oracle in 35 360 soak steps at the final kernels of round 6 (tools/soak.py --cold: default seeds 0 / 77, --large, --circles,
# --exotic --robots, --tight, --lmz-central 1e-3; profiles/r06_soak_final_*.txt): 1.3e-8 (interior-point LamMuZ mode; default mode 6.8e-9); 100 k steps over the round's
# builds: 3.1e-8; the fixed scenes of the BASELINE sizes <= 3e-11.  Asserted with a factor 30 of margin on the seeds of the tests.
# THE EXCEPTION (found by the long soaks of the round's last hours, 213 k more steps: DESIGN.md 2): a solve whose landings are ALL refused returns its fallback, the
# interior point at su_tol - TOL_U_IP below is what holds for it.  Seen on 4 of 64 000 `--exotic` soak steps (0 of 230 000 others): 4.8e-6 .. 1.2e-4 in the steering angle
# of an Ackermann robot at |v| <= 0.13 m/s, a direction the su-problem is nearly singular in; <= 3.9e-7 in what the robot does with the control (yaw rate).
# Since the last commit of the round that fallback runs 1e-3 x tighter than su_tol (SU_LAND_FALLBACK, both sides): the same 64 000 steps again: max 4.6e-7, no step outside TOL_U.
# Against the independent certified optimum (tests/su_kkt.py, tests/test_su_kkt_ref.py): the landed cold oracle is within 4e-10 of x* on a 240-problem grid and the
# recorded hard problems - but 1.35e-7 on tests/golden/su_hard/diff_T20_N24_just_active_hinges.npz (m = 0.25, f - f* = 1.7e-13): hinge rows 1e-8 .. 1e-7 from their switch,
# and a landing that is accepted at a stationarity residual of 100 x su_tol[0] relative.  Inside TOL_U, outside TOL_U_FIXED (pinned as a strict xfail there).
TOL_U = 1e-6
# ... and the bound asserted on the FIXED scenes of tests/test_gpu_baseline_sizes.py (BASELINE sizes) and the reference's dynamic_obs scene
TOL_U_FIXED = 1e-7
# The interior-point-only mode (su_land = 0 on both sides: the `no_landing` fixture - tests whose subject is the interior-point iteration itself) keeps
# the statement of rounds 3-5.  Why 5e-4 and not rounding level there: both sides stop their su interior point at a 1e-9 relative KKT residual and a
# 1e-11 (1 + |grad|) complementarity.  Where an inequality row is WEAKLY active (multiplier lam* ~ 1e-4: a rate or speed bound the solution just
# touches) the central-path point at complementarity mu lies mu / lam* from the solution, so two solves that stop at different mu - they walk
# different paths: cold / warm / easy starts - differ by up to a few 1e-5 per su-problem (tests/test_oracle_su.py::
# test_stop_tolerance_vs_weakly_active_rows: <= 5e-5 on the recorded worst cases, where a solve at the reference solver's ECOS-class 1e-8 tolerances
# is 2e-4 ... 3e-3 away), and the ADMM iterations of a step carry that through the LamMuZ problems.  Largest value seen in 38 400 + 12 800 + 9 600
# soak steps of rounds 3-5: 2.3e-4.
TOL_U_IP = 5e-4
TOL_U_FLIP = 5e-2          # steps on which the two sides stop one ADMM iteration apart (a residual within solver tolerance of iter_threshold)
MAX_FLIPS_PER_1000 = 5
# the COLD oracle, the independent checker (every su-problem of a step starts cold): `with switches(**hp.COLD_SU):`
COLD_SU = dict(su_warm=(0.0, 0.0), su_warm_cap=0)

ROBOT = sc.rectangle_robot()
G = np.ascontiguousarray(ROBOT.G, float)
H = np.ascontiguousarray(np.asarray(ROBOT.h, float).ravel())


def make_cfg(T=10, N=5, E=4, R=4, dynamics=0, accelerated=1, iter_num=2, ro1=200.0, ro2=1.0, ws=1.0, wu=1.0,
             slack_gain=8.0, max_sd=1.0, min_sd=0.1, iter_threshold=0.2, dt=0.1, L=3.0):
    c = Cfg()
    c.T, c.N, c.E, c.R = T, N, E, R
    c.dynamics, c.accelerated, c.iter_num, c.robot_norm2 = dynamics, accelerated, iter_num, 0
    c.dt, c.L = dt, L
    c.max_speed[0], c.max_speed[1] = 10.0, 1.0
    c.acce_bound[0], c.acce_bound[1] = 1.0, 0.05
    c.iter_threshold, c.ws, c.wu = iter_threshold, ws, wu
    c.slack_gain, c.max_sd, c.min_sd, c.ro1, c.ro2 = slack_gain, max_sd, min_sd, ro1, ro2
    c.delta, c.eps_u = 1e-6, 1e-8
    return c


def random_polygon(rng, centre, k, rad, E):
    # k distinct angles in CCW order, every gap in (0.35, pi): a valid (non-empty, convex) polygon -
    # the precondition under which basic dual solutions exist (an empty {x: Ax<=b} makes the dual LP unbounded)
    while True:
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        gaps = np.diff(np.r_[ang, ang[0] + 2 * np.pi])
        if gaps.min() > 0.35 and gaps.max() < np.pi - 0.05:
            break
    V = np.vstack((centre[0] + rad * np.cos(ang), centre[1] + rad * np.sin(ang)))
    A, b = sc.polygon_halfspaces(V)
    Ap = np.zeros((E, 2))
    bp = np.zeros(E)
    Ap[:k] = A
    bp[:k] = b.ravel()
    return Ap, bp


def lammuz_batch_inputs(rng, B, E=4, circles=0.25, near=True):
    """B random (obstacle, stage) sub-problems around random robot poses"""
    A = np.zeros((B, E, 2))
    b = np.zeros((B, E))
    cone = np.zeros(B, np.int32)
    p = rng.uniform(-5, 5, (B, 2))
    phi = rng.uniform(-np.pi, np.pi, B)
    xi = np.zeros((B, 2))
    zeta = np.zeros(B)
    dbar = rng.uniform(0.1, 1.0, B)
    for i in range(B):
        dist = rng.choice([0.5, 1.5, 3.0, 6.0, 15.0] if near else [6.0, 15.0, 30.0])
        th = rng.uniform(0, 2 * np.pi)
        cen = p[i] + dist * np.array([np.cos(th), np.sin(th)])
        if rng.random() < circles and E >= 3:
            A[i, 0] = [1, 0]
            A[i, 1] = [0, 1]
            b[i, 0:3] = [cen[0], cen[1], -rng.uniform(0.3, 1.5)]
            cone[i] = 1
        else:
            k = int(rng.integers(3, E + 1))
            A[i], b[i] = random_polygon(rng, cen, k, rng.uniform(0.5, 2.0), E)
        xi[i] = rng.normal(0, rng.choice([0, 0.05, 0.5]), 2)
        zeta[i] = rng.normal(0, rng.choice([0, 0.3, 2.0]))
    return dict(A=A, b=b, cone=cone, p=p, phi=phi, xi=xi, zeta=zeta, dbar=dbar)


def oracle_lammuz_batch(orc, inp, ro2=1.0, delta=1e-6, accelerated=1, G=G, h=H):
    B, E = inp["b"].shape
    R = G.shape[0]
    lam = np.zeros((B, E))
    mu = np.zeros((B, R))
    z = np.zeros(B)
    cmh = np.zeros((B, 4))
    for i in range(B):
        zz = C.c_double(0)
        orc.lib.orc_lammuz_one(E, R, dptr(np.ascontiguousarray(inp["A"][i])), dptr(np.ascontiguousarray(inp["b"][i])),
                               int(inp["cone"][i]), dptr(np.ascontiguousarray(inp["p"][i])), float(inp["phi"][i]),
                               dptr(G), dptr(h), dptr(np.ascontiguousarray(inp["xi"][i])), float(inp["zeta"][i]),
                               float(inp["dbar"][i]), ro2, delta, accelerated, dptr(lam[i]), dptr(mu[i]),
                               C.cast(C.byref(zz), C.POINTER(C.c_double)), dptr(cmh[i]))
        z[i] = zz.value
    return lam, mu, z, cmh


def hip_lammuz_batch(hip, inp, ro2=1.0, delta=1e-6, accelerated=1, G=G, h=H):
    B, E = inp["b"].shape
    R = G.shape[0]
    lam = np.zeros((B, E))
    mu = np.zeros((B, R))
    z = np.zeros(B)
    cmh = np.zeros((B, 4))
    arr = {k: np.ascontiguousarray(v) for k, v in inp.items()}
    rc = hip.lib.rda_lammuz_batch(B, E, R, dptr(arr["A"]), dptr(arr["b"]), iptr(arr["cone"]), dptr(arr["p"]), dptr(arr["phi"]),
                                  dptr(G), dptr(h), dptr(arr["xi"]), dptr(arr["zeta"]), dptr(arr["dbar"]), ro2, delta,
                                  accelerated, dptr(lam), dptr(mu), dptr(z), dptr(cmh))
    assert rc == 0, rc
    return lam, mu, z, cmh


def su_inputs(rng, cfg):
    """random su-problem around a rolled-out nominal, with some hinges active"""
    T, N, dyn = cfg.T, cfg.N, cfg.dynamics
    nom_u = np.vstack([rng.uniform(1, 4, T), rng.uniform(-0.3, 0.3, T)])
    nom_s = np.zeros((3, T + 1))
    nom_s[:, 0] = [rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-3, 3)]
    for t in range(T):
        phi, v, psi = nom_s[2, t], nom_u[0, t], nom_u[1, t]
        if dyn == 0:
            ds = np.array([v * np.cos(phi), v * np.sin(phi), v * np.tan(psi) / cfg.L])
        elif dyn == 1:
            ds = np.array([v * np.cos(phi), v * np.sin(phi), psi])
        else:
            ds = np.array([v * np.cos(psi), v * np.sin(psi), 0.0])
        nom_s[:, t + 1] = nom_s[:, t] + cfg.dt * ds
    ref = nom_s + rng.normal(0, 0.3, (3, T + 1))
    a = rng.normal(0, 0.5, (N, T, 2))
    a /= np.maximum(1, np.linalg.norm(a, axis=2, keepdims=True))
    cc = np.einsum("ntk,kt->nt", a, nom_s[0:2, 1:]) - rng.uniform(-0.5, 1.5, (N, T))
    g = rng.normal(0, 0.3, (N, T, 2))
    return dict(nom_s=np.ascontiguousarray(nom_s), nom_u=np.ascontiguousarray(nom_u), ref=np.ascontiguousarray(ref),
                vref=4.0, a=np.ascontiguousarray(a), cc=np.ascontiguousarray(cc), g=np.ascontiguousarray(g), d0=np.ones(T))


def su_solve(fn, cfg, inp):
    T = cfg.T
    s = np.zeros((3, T + 1))
    u = np.zeros((2, T))
    d = np.zeros(T)
    it = C.c_int(0)
    st = fn(C.byref(cfg), dptr(inp["nom_s"]), dptr(inp["nom_u"]), dptr(inp["ref"]), inp["vref"], dptr(inp["a"]),
            dptr(inp["cc"]), dptr(inp["g"]), dptr(inp["d0"]), dptr(s), dptr(u), dptr(d), C.byref(it))
    return st, s, u, d, it.value


def load_su_case(path):
    """(cfg, inputs) of a recorded su-problem (tests/golden/su_hard/*.npz, written by the soak run)"""
    d = np.load(path)
    dyn = {"acker": 0, "diff": 1, "omni": 2}[str(d["dyn"])]
    cfg = make_cfg(T=int(d["T"]), N=int(d["N"]), dynamics=dyn, ro1=float(d["ro1"]))
    inp = dict(nom_s=np.ascontiguousarray(d["nom_s"], float).reshape(3, -1), nom_u=np.ascontiguousarray(d["nom_u"], float),
               ref=np.ascontiguousarray(d["ref"], float), vref=float(d["speed"]), a=np.ascontiguousarray(d["a"]),
               cc=np.ascontiguousarray(d["cc"]), g=np.ascontiguousarray(d["g"]), d0=np.ascontiguousarray(d["d0"], float).ravel())
    return cfg, inp
