"""-m gpu : the HIP su solve against the independent certified optimum of tests/su_kkt.py.

  a. the cold hook rda_su_solve (default options) on the grid and the recorded hard problems of tests/test_su_kkt_ref.py, compiled (10, 20, 25, 30)
     and generic horizons
  b. the hot path: recorded closed loops driven through rda_admm_begin / su / lammuz / finish (checked against rda_step), every su-problem rebuilt
     from the handle's state (su_kkt.su_inputs_from_state) and certified; the kernel's (s, u, dis) per landing path (rda_debug_su_land_n)
  c. status against truth: with su_accept = 0 a cold landed solve whose answer is within TOL_U of the optimum reports status 0
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import helpers as hp
import su_kkt
from rda_planner_amd._capi import Info, dptr, iptr, f64
from test_su_kkt_ref import DYN, GOLD, GRID_N, GRID_T, JUST_ACTIVE_FIXTURE, check_against, drive_recorded_loop

pytestmark = pytest.mark.gpu


def _hook_cases():
    for dyn in range(3):
        for acc in (0, 1):
            for T in GRID_T:
                for N in GRID_N:
                    rng = np.random.default_rng(1000 * dyn + 100 * acc + 7 * T + N)
                    cfg = hp.make_cfg(T=T, N=N, dynamics=dyn, accelerated=acc)
                    yield f"{DYN[dyn]} acc={acc} T={T} N={N}", cfg, hp.su_inputs(rng, cfg)
    for path in sorted(glob.glob(os.path.join(GOLD, "su_hard", "*.npz"))):
        cfg, si = hp.load_su_case(path)
        yield os.path.basename(path), cfg, si


def test_cold_hook_against_the_certificate(hip):
    worst = {"grid": 0.0, "su_hard": 0.0}
    for what, cfg, si in _hook_cases():
        if cfg.N == 0:          # (the hook refuses a problem without obstacle terms: include/rda_hip.h)
            assert hp.su_solve(hip.lib.rda_su_solve, cfg, si)[0] == -2, what
            continue
        st, s, u, d, it = hp.su_solve(hip.lib.rda_su_solve, cfg, si)
        assert st == 0, what
        c = su_kkt.certify(cfg, si, start=(s, u, d))
        key = "su_hard" if what.endswith(".npz") else "grid"
        if what == JUST_ACTIVE_FIXTURE + ".npz":
            print(f"{what}: |x_gpu - x*| {c.distance(s, u, d):.2e} (the landing's stationarity stop, tests/helpers.py)")
            assert c.distance(s, u, d) <= hp.TOL_U
            continue
        worst[key] = max(worst[key], check_against(c, s, u, d, hp.TOL_U_FIXED, what))
    print(f"cold hook: worst |x_gpu - x*| grid {worst['grid']:.2e}, su_hard {worst['su_hard']:.2e}")


def _land_counters(solver):
    out = (C.c_int32 * 6)()
    assert solver._be.api.lib.rda_debug_su_land_n(solver._be.handle, out, 6) == 0
    return list(out)


@pytest.mark.parametrize("name", ["c1", "pad", "c2", "c4", "ns"])
def test_hot_path_against_the_certificate(name):
    from rda_planner_amd.rda_solver import RDA_solver
    solvers = []

    def make(T, car_t, E, N, iter_num, ro1):
        s = RDA_solver(T, car_t, E, N, iter_num=iter_num, time_print=False, ro1=ro1)
        solvers.append(s)
        _land_counters(s)
        return s
    worst = {"landed": 0.0, "speculative": 0.0, "fallback": 0.0}
    count = {k: 0 for k in worst}
    spec_total = [0]

    def on_su(k, it, cfg, si, s, u, dis, inf):
        lc = _land_counters(solvers[0])
        path = "fallback" if lc[0] == 0 else ("speculative" if lc[5] > 0 else "landed")
        spec_total[0] += lc[5]
        c = su_kkt.certify(cfg, si, start=(s, u, dis))
        tol = hp.TOL_U if path == "fallback" else hp.TOL_U_FIXED
        worst[path] = max(worst[path], check_against(c, s, u, dis, tol, f"{name} step {k} it {it} ({path})"))
        count[path] += 1
    steps = None
    applied = drive_recorded_loop(make, name, on_su, steps=steps)
    # what the instrumented loop computes is what the hot path computes: the same steps driven plainly through the same pieces (one finish per step) and
    # through rda_step agree with it to TOL_U_FIXED.  (Not bit for bit: the finish per iteration that reads (s, u) back also records whether the ADMM has
    # converged - the key of the hard warm start of the next su-problem - so the interior point may start differently; the landed vertex is the same.)
    g = np.load(os.path.join(GOLD, "ref_plumbing.npz"))
    T, N, E, iter_num, ro1, dyn = (int(v) if i != 4 else float(v) for i, v in enumerate(g[f"{name}.cfg"]))
    from test_ref_golden import _car
    plain, stepped = (RDA_solver(T, _car(dyn), E, N, iter_num=iter_num, time_print=False, ro1=ro1) for _ in range(2))
    for k in range(len(applied)):
        pre = f"{name}.{k}"
        n_obs = int(g[f"{pre}.n_obs"])
        A, b, cone = (f64(g[f"{pre}.A"]), f64(g[f"{pre}.b"]), np.ascontiguousarray(g[f"{pre}.cone"], np.int32)) if n_obs else (None, None, None)
        per_t = int(g[f"{pre}.per_t"]) if n_obs else 0
        args = (dptr(f64(g[f"{pre}.nom_s"])), dptr(f64(g[f"{pre}.nom_u"])), dptr(f64(g[f"{pre}.ref"])), float(g[f"{pre}.speed"]))
        obs = (n_obs, dptr(A) if n_obs else None, dptr(b) if n_obs else None, iptr(cone) if n_obs else None, per_t)
        api, hd = plain._be.api, plain._be.handle
        assert api.upload_obstacles(hd, *obs) == 0 and api.admm_begin(hd, *args) == 0
        for it in range(iter_num):
            stopped = C.c_int(0)
            assert api.admm_su(hd, it, C.byref(stopped)) == 0
            if stopped.value:
                break
            assert api.admm_lammuz(hd) == 0
        u1, s1, inf = np.zeros((2, T)), np.zeros((3, T + 1)), Info()
        assert api.admm_finish(hd, dptr(u1), dptr(s1), C.byref(inf)) == 0
        assert np.abs(u1[:, 0] - applied[k]).max() <= hp.TOL_U_FIXED, (name, k, np.abs(u1[:, 0] - applied[k]).max())
        u2, s2 = np.zeros((2, T)), np.zeros((3, T + 1))
        assert stepped._be.api.step(stepped._be.handle, *args, *obs, dptr(u2), dptr(s2), C.byref(Info())) >= 0
        assert np.abs(u2[:, 0] - applied[k]).max() <= hp.TOL_U_FIXED, (name, k, np.abs(u2[:, 0] - applied[k]).max())
    print(f"{name}: worst |x_gpu - x*| per path " + ", ".join(f"{p} {worst[p]:.2e} ({count[p]} solves)" for p in worst)
          + f"; speculative landings accepted {spec_total[0]}")
    if name in ("c4", "ns"):
        assert spec_total[0] > 0            # the speculative path went through the check


def test_status_against_truth(hip):
    """with su_accept = 0 and su_land = 1, a cold solve whose answer is within TOL_U of the certified optimum returns status 0"""
    from rda_planner_amd.rda_solver import hip_options
    o = hip_options(su_accept=0, su_land=1)
    fn = lambda *a: hip.lib.rda_su_solve_opts(a[0], C.byref(o), *a[1:])       # noqa: E731
    nonzero = []
    for what, cfg, si in _hook_cases():
        if cfg.N == 0:
            continue
        st, s, u, d, it = hp.su_solve(fn, cfg, si)
        try:
            c = su_kkt.certify(cfg, si, start=(s, u, d))
        except RuntimeError:
            assert st != 0, what         # an answer that is not near the optimum cannot seed the certificate: it must not claim success
            continue
        if c.distance(s, u, d) <= hp.TOL_U and st != 0:
            nonzero.append((what, st, c.distance(s, u, d)))
    print(f"status vs truth: {len(nonzero)} solves within TOL_U with status != 0")
    assert not nonzero, nonzero
