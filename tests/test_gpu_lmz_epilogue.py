"""GPU: the epilogue of the packed-rows LamMuZ kernels (k_lammuz_rows: the row's sums and the residual reduction run on the row's lanes)
against the one-sub-problem-per-wave form (RDA_LMZ_ROWS=0: k_lammuz, whose epilogue in lammuz_body is one lane's sequential loop over the E
obstacle rows and the R robot rows).  Both forms call the same device functions for the solve, and the packed epilogue forms every sum from
the same operands in the same order with the same fused multiply-adds, so everything a tick leaves behind must agree BIT FOR BIT: lam, mu,
z, xi, zeta, the condensed terms (a_lam, b_lam of get_state), the residuals of the info and the applied controls.  No tolerance anywhere.

Two ticks of three ADMM iterations, re-sorted between the ticks (obstacle_order=True, the state moves), T = 3.  N in {1, 7, 9}: a block of
GS = 8 slots with one live row, one with a dead slot, and a second block with one live row.  E in {3, 4, 8} with the rectangle robot
(R = 4; E = 8 fills 13 of a row's 16 lanes).  The scenes hold a full polygon, a padded one (a null row; at E = 3 a triangle is already full),
a circle and a polygon with a NaN vertex (the failed-row path: it keeps its duals, residual inf); N = 1 takes one of the four kinds per E.
One fleet of two members against its solo twins runs the fleet launch forms of the same body."""
import os

import numpy as np
import pytest

from rda_planner_amd import scenarios as sc

pytestmark = pytest.mark.gpu

T, ITERS, TICKS = 3, 3, 2
STATE_KEYS = ("lam", "mu", "z", "xi", "zeta", "a_lam", "b_lam")


def _scene(N, E):
    """N obstacles beside the path y = 25: kinds in turn (full polygon, padded polygon, circle, NaN polygon), the first kind chosen by E so that
    the one-obstacle scenes cover three kinds between them"""
    kinds = ["full", "padded", "circle", "nan"]
    first = {3: 0, 4: 1, 8: 2}[E]
    rng = np.random.default_rng(100 * N + E)
    out = []
    for i in range(N):
        kind = kinds[(first + i) % 4]
        cx, cy = 7.0 + 1.9 * i, 25.0 + (3.1 if i % 2 else -3.0) + rng.uniform(-0.3, 0.3)
        if kind == "circle":
            out.append(sc.circle(cx, cy, 0.7))
            continue
        k = max(3, E - 1) if kind == "padded" else E
        o = sc.regular_polygon(cx, cy, k, 0.9, rng.uniform(-np.pi, np.pi))
        if kind == "nan":
            v = o.vertex.copy(); v[0, 0] = np.nan
            o = o._replace(vertex=v)
        out.append(o)
    return out


def _run(N, E, rows):
    from rda_planner_amd.mpc import MPC
    old = os.environ.get("RDA_LMZ_ROWS")
    os.environ["RDA_LMZ_ROWS"] = rows
    try:
        car_t = sc.rectangle_robot(dynamics="acker")
        path = sc.line_path([4, 25, 0], [30, 25, 0], 0.1)
        mpc = MPC(car_t, [p.copy() for p in path], receding=T, iter_num=ITERS, max_edge_num=E, max_obs_num=N, obstacle_order=True, time_print=False)
        kernel = None
        state = path[0].copy().reshape(3, 1)
        scene, ticks = _scene(N, E), []
        for k in range(TICKS):
            u, info = mpc.control(state.copy(), 4.0, list(scene))
            kernel = mpc.rda._be.api.lib.rda_lammuz_kernel(mpc.rda._be.handle).decode()
            st = mpc.rda.get_state()
            ticks.append((u.copy(), (info["iters"], info["resi_dual"], info["resi_pri"], info["lmz_fail"]), {key: st[key].copy() for key in STATE_KEYS}))
            state = np.array([[4.0 + 2.5 * (k + 1)], [25.0 + 0.4 * (k + 1)], [0.05 * (k + 1)]])      # far enough to change the order of the slots
        return kernel, ticks
    finally:
        os.environ.pop("RDA_LMZ_ROWS", None) if old is None else os.environ.__setitem__("RDA_LMZ_ROWS", old)


@pytest.mark.parametrize("E", [3, 4, 8])
@pytest.mark.parametrize("N", [1, 7, 9])
def test_packed_epilogue_equals_the_sequential_one(N, E):
    kr, rows = _run(N, E, "1")
    kw, wave = _run(N, E, "0")
    assert kr.startswith("k_lammuz_rows") and kw.startswith("k_lammuz") and not kw.startswith("k_lammuz_rows"), (kr, kw)
    has_nan = any(o.vertex is not None and np.isnan(o.vertex).any() for o in _scene(N, E))
    for k, ((ur, ir, sr), (uw, iw, sw)) in enumerate(zip(rows, wave)):
        print(f"N={N} E={E} tick {k}: iters {ir[0]} resi_dual {ir[1]:.3e} resi_pri {ir[2]:.3e} lmz_fail {ir[3]}  max|du| {np.abs(ur - uw).max():.1e}")
        assert ir == iw, (k, ir, iw)
        assert np.array_equal(ur, uw), (k, np.abs(ur - uw).max())
        for key in STATE_KEYS:
            assert np.array_equal(sr[key], sw[key], equal_nan=True), (k, key, np.abs(sr[key] - sw[key]).max())
        assert np.isfinite(ur).all()
        assert (ir[3] > 0 and ir[1] == np.inf) if has_nan else ir[3] == 0, (k, ir)
    # the ticks did something: duals moved, and the second tick is not the first again
    assert any(np.abs(rows[-1][2][key]).max() > 0 for key in ("mu", "xi")) or has_nan
    assert not np.array_equal(rows[0][0], rows[1][0])


def test_fleet_of_two_equals_its_solo_twins():
    """the fleet launch forms of the packed body (member in the grid) against two solo handles, two ticks, state and all"""
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    car_t = sc.rectangle_robot(dynamics="acker")
    E, N = 4, 7
    solo, memb, states, scenes = [], [], [], []
    for i in range(2):
        y = 20.0 + 9 * i
        path = sc.line_path([4, y, 0], [30, y, 0], 0.1)
        kw = dict(receding=T, iter_num=ITERS, max_edge_num=E, max_obs_num=N, obstacle_order=True, time_print=False)
        solo.append(MPC(car_t, [p.copy() for p in path], **kw))
        memb.append(MPC(car_t, [p.copy() for p in path], **kw))
        states.append(path[0].copy().reshape(3, 1))
        scenes.append([o if o.vertex is None else o._replace(vertex=o.vertex + np.array([[0.0], [y - 25.0]])) for o in _scene(N, E)[:3]]
                      + [sc.circle(9.0 + i, y + 3.0, 0.8)])
    fleet = Fleet(memb)
    try:
        for k in range(TICKS):
            res = fleet.control([s.copy() for s in states], 4.0, [list(s) for s in scenes])
            assert fleet.lammuz_kernel().startswith("k_lammuz_fleet_rows"), fleet.lammuz_kernel()
            for i in range(2):
                u, info = solo[i].control(states[i].copy(), 4.0, list(scenes[i]))
                uf, inf = res[i]
                assert np.array_equal(u, uf), (k, i, np.abs(u - uf).max())
                assert (info["iters"], info["resi_dual"], info["resi_pri"], info["lmz_fail"]) == (inf["iters"], inf["resi_dual"], inf["resi_pri"], inf["lmz_fail"])
                sa, sb = solo[i].rda.get_state(), memb[i].rda.get_state()
                for key in STATE_KEYS:
                    assert np.array_equal(sa[key], sb[key], equal_nan=True), (k, i, key)
                states[i] = sc.kinematic_step(states[i], u, car_t, 0.1)
    finally:
        fleet.close()
