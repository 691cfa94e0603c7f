"""-m gpu : fleets whose members run the interior-point LamMuZ mode (`MPC(..., lmz_central=mu)`, rda_opts::lmz_mode = 1).  The fleet launches
(`k_lammuz_ip_fleet`, `k_lammuz_cp_fleet_*` + `k_lmz_finalize_fleet`) run the solo kernels' bodies with the member in the grid, and the launch form is
chosen PER MEMBER by the rule of a solo handle - so every member is bit for bit its solo twin, whatever its neighbours stage: controls, states, iteration
counts, residuals, failure counts, the dual state and the kept central-path points.  `rda_fleet_lammuz_kernel` proves which kernels ran."""
import ctypes as C

import numpy as np
import pytest

import helpers as hp
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import Info, dptr, iptr

from fleet_twin_lib import hip          # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

RDA_ERR_UNSUPPORTED = -2
ROWS, CP_SMALL, CP_LARGE, FIN = "k_lammuz_ip_fleet", "k_lammuz_cp_fleet_small", "k_lammuz_cp_fleet_large", "k_lmz_finalize_fleet"


def _fleet(hip, memb):
    B = len(memb)
    arr = (C.c_void_p * B)(*[m._be.handle for m in memb])
    F = C.c_void_p()
    assert hip.fleet_create(arr, B, C.byref(F)) == 0
    return F


def _kernel(hip, F):
    return hip.fleet_lammuz_kernel(F).decode()


def _history(hip, s):
    n = hip.lib.rda_lmz_history_doubles(s._be.handle)
    pts, valid = np.zeros(max(n, 1)), np.zeros(max(n // 80, 1), np.int32)
    if n > 0:
        assert hip.lib.rda_get_lmz_history(s._be.handle, dptr(pts), iptr(valid)) == 0
    return n, pts, valid


def _twins(B, T, N, E, mus, thresholds, counts, iter_num=3):
    """B (solo, member) pairs in the interior-point mode and the host-staged obstacle list of each: member i stages counts[i] obstacles (fewer than
    N: padded with copies of the last, quirk Q3), one of them a circle.  Member 0's obstacles are far from every nominal trajectory (its residuals are
    tiny: with thresholds[0] it stops early), the others' are among them."""
    from rda_planner_amd.rda_solver import RDA_solver
    from rda_planner_amd.mpc import MPC
    solo, memb, staged = [], [], []
    for i in range(B):
        dyn = ["acker", "diff", "omni"][i % 3]
        car_t = sc.rectangle_robot(dynamics=dyn, wheelbase=3.0 if dyn == "acker" else 0)
        kw = dict(iter_num=iter_num, time_print=False, ro1=[200.0, 100.0, 300.0][i % 3], slack_gain=8.0 + i, iter_threshold=thresholds[i],
                  lmz_central=mus[i])
        solo.append(RDA_solver(T, car_t, E, N, **kw))
        memb.append(RDA_solver(T, car_t, E, N, **kw))
        lo, hi = ((40, 40), (48, 48)) if i == 0 else ((-2, -4), (7, 4))
        obstacles = sc.scene_polygons(counts[i] - 1, lo=lo, hi=hi, seed=21 + i) + [sc.circle(0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.7)]
        conv = MPC.__new__(MPC); conv.receding = T; conv.dt = 0.1; conv.state = np.zeros((3, 1))
        staged.append(MPC.convert_rda_obstacle(conv, obstacles, np.zeros((3, 1)), True))
        assert sum(o.cone_type == "norm2" for o in staged[i]) == 1 and len(staged[i]) == counts[i] < N
    return solo, memb, staged


def _inputs(rng, B, T, N, K):
    noms, nomu, refs = np.zeros((K, B, 3, T + 1)), np.zeros((K, B, 2, T)), np.zeros((K, B, 3, T + 1))
    for k in range(K):
        for i in range(B):
            si = hp.su_inputs(rng, hp.make_cfg(T=T, N=N, dynamics=i % 3))
            noms[k, i], nomu[k, i], refs[k, i] = si["nom_s"], si["nom_u"].reshape(2, T), si["ref"]
    return noms, nomu, refs


def _step_both(hip, F, solo, memb, lists, noms, nomu, refs, speed, k):
    """step k: every twin by rda_step, the members by ONE rda_fleet_step, on copies of lists[i]; asserts that they agree bit for bit and returns
    the members' (iters, lmz_fail)"""
    B, T = len(solo), solo[0].T
    want = []
    for i in range(B):
        want.append(solo[i].iterative_solve(noms[k, i], nomu[k, i], [refs[k, i][:, j:j + 1] for j in range(T + 1)], speed[i], list(lists[i])))
        memb[i].upload_obstacles(list(lists[i]))
    ou, os_, infos = np.zeros((B, 2, T)), np.zeros((B, 3, T + 1)), (Info * B)()
    assert hip.fleet_step(F, dptr(noms[k]), dptr(nomu[k]), dptr(refs[k]), dptr(speed), dptr(ou), dptr(os_), infos) == 0
    for i in range(B):
        u, info = want[i]
        assert np.array_equal(ou[i], u), (k, i, np.abs(ou[i] - u).max())
        assert np.array_equal(os_[i], np.hstack(info["opt_state_list"])), (k, i)
        got = (infos[i].iters, infos[i].su_status, infos[i].resi_dual, infos[i].resi_pri, infos[i].lmz_fail)
        assert got == (info["iters"], info["status"], info["resi_dual"], info["resi_pri"], info["lmz_fail"]), (k, i, got)
    return [(infos[i].iters, infos[i].lmz_fail) for i in range(B)]


def _same_state_and_history(hip, solo, memb):
    for i, (a, b) in enumerate(zip(solo, memb)):
        sa, sb = a.get_state(), b.get_state()
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (i, key)
        (na, pa, va), (nb, pb, vb) = _history(hip, a), _history(hip, b)
        assert na == nb and np.array_equal(va, vb) and np.array_equal(pa, pb), (i, na, nb)


MUS, THRESHOLDS = (1e-3, 1e-3, 1e-6), (5.0, 0.2, 1e-12)


@pytest.mark.parametrize("N", [5, 9])
def test_fleet_step_equals_member_steps_in_the_interior_point_mode(hip, N):
    """B = 3, E = R = 4, T = 6, iter_num = 3, lmz_mu 1e-3 / 1e-3 / 1e-6, different obstacle counts below N (Q3 padding copies), one circle each.
    N = 5: one 8-slot block with dead rows; N = 9: two blocks and the fillers of the packed grid.  Four steps: from the second on the kept
    central-path points are in use.  One member stops early while another runs all iterations (the stop flag is per member inside one launch)."""
    B, T, K = 3, 6, 4
    solo, memb, staged = _twins(B, T, N, 4, MUS, THRESHOLDS, [N - 1, N - 2, 3])
    noms, nomu, refs = _inputs(np.random.default_rng(15 + N), B, T, N, K)
    speed = np.linspace(2.0, 5.0, B)
    F = _fleet(hip, memb)
    mixed_stop = False
    for k in range(K):
        its = [it for it, fail in _step_both(hip, F, solo, memb, staged, noms, nomu, refs, speed, k)]
        assert _kernel(hip, F) == ROWS, k                       # (every member has staged obstacles)
        mixed_stop = mixed_stop or (min(its) < 3 and max(its) == 3)
    assert mixed_stop
    _same_state_and_history(hip, solo, memb)
    n, _, valid = _history(hip, memb[1])
    assert n == 80 * N * T and valid.any()                      # the central-path points were kept (and compared above)
    assert _kernel(hip, F) == ROWS
    hip.fleet_destroy(F)


def test_launch_form_is_chosen_per_member(hip):
    """the same fleet with member 1's obstacle list EMPTY on ticks 2 - 3 (quirk Q9: that member runs the per-thread kernel and the finalize, the
    others stay on the row-parallel kernel): every member bit for bit its twin on every tick, both forms named while they run"""
    B, T, N, K = 3, 6, 5, 5
    solo, memb, staged = _twins(B, T, N, 4, MUS, THRESHOLDS, [N - 1, N - 2, 3])
    noms, nomu, refs = _inputs(np.random.default_rng(33), B, T, N, K)
    speed = np.linspace(2.0, 5.0, B)
    F = _fleet(hip, memb)
    for k in range(K):
        lists = [staged[i] if not (i == 1 and k in (2, 3)) else [] for i in range(B)]
        _step_both(hip, F, solo, memb, lists, noms, nomu, refs, speed, k)
        assert _kernel(hip, F) == ("+".join((ROWS, CP_SMALL, FIN)) if k in (2, 3) else ROWS), k      # (the members as this tick staged them)
    _same_state_and_history(hip, solo, memb)
    hip.fleet_destroy(F)


def test_shapes_beyond_sixteen_variables_run_the_per_thread_kernel(hip):
    """E = 8, R = 4: E + R + 6 > 16, the row-parallel kernel does not take the shape - every member runs the per-thread kernel (T = 4, N = 3, B = 2,
    two steps: that kernel is slow)"""
    B, T, N, K = 2, 4, 3, 2
    solo, memb, staged = _twins(B, T, N, 8, (1e-3, 1e-6), (0.2, 1e-12), [2, 2])
    noms, nomu, refs = _inputs(np.random.default_rng(34), B, T, N, K)
    speed = np.array([3.0, 4.0])
    F = _fleet(hip, memb)
    for k in range(K):
        _step_both(hip, F, solo, memb, staged, noms, nomu, refs, speed, k)
        assert _kernel(hip, F) == CP_LARGE + "+" + FIN
    _same_state_and_history(hip, solo, memb)
    hip.fleet_destroy(F)


def test_a_failed_sub_problem_stays_with_its_member(hip):
    """one member's obstacle gets a non-finite half-space (a NaN vertex): its rows keep their duals and are counted in lmz_fail exactly as its
    twin's are; the other members do not notice"""
    B, T, N, K = 3, 6, 5, 3
    solo, memb, staged = _twins(B, T, N, 4, MUS, THRESHOLDS, [N - 1, N - 2, 3])
    bad = next(j for j, o in enumerate(staged[1]) if o.cone_type == "Rpositive")
    A = np.array(staged[1][bad].A, float); A[0, 0] = np.nan
    broken = list(staged[1]); broken[bad] = broken[bad]._replace(A=A)
    noms, nomu, refs = _inputs(np.random.default_rng(35), B, T, N, K)
    speed = np.linspace(2.0, 5.0, B)
    F = _fleet(hip, memb)
    for k in range(K):
        lists = [staged[0], broken if k >= 1 else staged[1], staged[2]]
        res = _step_both(hip, F, solo, memb, lists, noms, nomu, refs, speed, k)
        fails = [fail for it, fail in res]
        assert fails[0] == 0 and fails[2] == 0 and (fails[1] > 0) == (k >= 1), (k, fails)
    _same_state_and_history(hip, solo, memb)
    hip.fleet_destroy(F)


def test_fleet_control_equals_member_control_with_lmz_central():
    """`Fleet.control` over 4 closed loops with `lmz_central` (1e-3 and 1e-6; acker / diff / omni; static and moving scenes; one member converting
    its obstacles on the host), 25 ticks == four `MPC.control` loops, bit for bit"""
    from rda_planner_amd.mpc import MPC
    from rda_planner_amd.fleet import Fleet
    B = 4
    solo, memb, cars, scenes, states = [], [], [], [], []
    for i in range(B):
        dyn = ["acker", "diff", "omni"][i % 3]
        car_t = sc.rectangle_robot(dynamics=dyn, wheelbase=3.0 if dyn == "acker" else 0)
        y = 20.0 + 3 * i
        path = sc.line_path([4, y, 0], [24 + 2 * i, y, 0], 0.1)
        clear = np.array([[p[0, 0], p[1, 0]] for p in path[::10]])
        scene = sc.scene_polygons([7, 4][i % 2], lo=(6, y - 8), hi=(28, y + 8), seed=60 + i, keep_clear=clear, clear_radius=3.0, moving=(i % 2 == 0))
        scene.append(sc.circle(15.0, y + 4.0, 0.8, (0.0, -0.2)))
        kw = dict(receding=8, iter_num=3, max_edge_num=4, max_obs_num=6, device_obstacles=(i != 2), lmz_central=[1e-3, 1e-6][i % 2])
        solo.append(MPC(car_t, [p.copy() for p in path], **kw))
        memb.append(MPC(car_t, [p.copy() for p in path], **kw))
        cars.append(car_t); scenes.append(scene)
        st = path[0].copy().reshape(3, 1)
        if dyn == "omni":
            st[2, 0] = 0.0
        states.append(st)
    fleet = Fleet(memb)
    for k in range(25):
        cur = [[o if not o.velocity.any() else (o._replace(vertex=o.vertex + o.velocity * (0.1 * k)) if o.cone_type == "Rpositive"
                                                else o._replace(center=o.center + o.velocity * (0.1 * k))) for o in scenes[i]] for i in range(B)]
        res = fleet.control([s.copy() for s in states], [3.0 + 0.2 * i for i in range(B)], [list(c) for c in cur])
        assert fleet.lammuz_kernel() == ROWS
        for i in range(B):
            u, info = solo[i].control(states[i].copy(), 3.0 + 0.2 * i, list(cur[i]))
            uf, inf = res[i]
            assert np.array_equal(u, uf), (k, i, np.abs(u - uf).max())
            assert info["iters"] == inf["iters"] and info["arrive"] == inf["arrive"] and info["resi_dual"] == inf["resi_dual"]
            assert np.array_equal(np.hstack(info["opt_state_list"]), np.hstack(inf["opt_state_list"]))
            states[i] = sc.kinematic_step(states[i], u, cars[i], 0.1)
    assert np.linalg.norm(states[0][0:2, 0] - np.array([4.0, 20.0])) > 3.0          # the loops moved
    fleet.close()


def test_fleet_control_with_scans_equals_member_control_with_scan_with_lmz_central():
    """`Fleet.control(scans=)` (rda_fleet_upload_scans: the box counts choose every member's LamMuZ form) over three robots with their own lidar worlds -
    those of tests/test_gpu_fleet_lidar.py - in the robust mode == three `MPC.control(scan=)` loops, bit for bit"""
    import test_gpu_fleet_lidar as fl
    from rda_planner_amd.fleet import Fleet
    envs = [fl._track_world(k) for k in range(3)]
    memb, solo = [fl._mpc(lmz_central=1e-3) for _ in envs], [fl._mpc(lmz_central=1e-3) for _ in envs]
    fleet = Fleet(memb)
    for tick in range(5):
        states = [e.robot.state.copy() for e in envs]
        scans_t = [e.get_lidar_scan() for e in envs]
        res = fleet.control([s.copy() for s in states], 4, scans=scans_t)
        assert ROWS in fleet.lammuz_kernel()                    # (some member saw a box)
        for i, env in enumerate(envs):
            u, info = solo[i].control(states[i].copy(), 4, scan=scans_t[i])
            uf, inf = res[i]
            assert np.array_equal(u, uf), (tick, i, u.ravel(), uf.ravel())
            assert all(np.array_equal(x, y) for x, y in zip(info["opt_state_list"], inf["opt_state_list"])), (tick, i)
            assert info["iters"] == inf["iters"] and info["resi_dual"] == inf["resi_dual"] and info["lmz_fail"] == inf["lmz_fail"], (tick, i)
            env.step(u)
    fleet.close()


def test_robust_mode_reaches_the_goal_as_one_fleet_rollout():
    """The point of it: the corridor (C2) from the 16 perturbed starts of test_gpu_central's
    test_robust_mode_reaches_the_goal_from_perturbed_starts as ONE 16-member fleet rollout in the robust mode (`lmz_central=1e-3`) with the device
    clearance log.  Success = arrived, and the clearance up to arrival stayed positive.  The bound is the one asserted for the same scene, mode and
    starts run one by one (13 of 16: a rate, these closed loops are chaotic)."""
    from rda_planner_amd.mpc import MPC
    from rda_planner_amd.fleet import Fleet
    rng = np.random.default_rng(11)
    starts = [(0.0, 0.0, 0.0)] + [(rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.08, 0.08)) for _ in range(15)]
    car_a = sc.rectangle_robot(dynamics="acker")
    path = sc.line_path([0, 20, 0], [60, 20, 0], 0.1)
    obs = sc.scene_corridor(n_extra=0)
    memb = [MPC(car_a, [p.copy() for p in path], sample_time=0.1, max_edge_num=4, max_obs_num=6, lmz_central=1e-3) for _ in starts]
    states = [np.array([[0.0 + dx], [20.0 + dy], [0.0 + dth]]) for dx, dy, dth in starts]
    fleet = Fleet(memb)
    out = fleet.rollout(states, 4, steps=300, obstacle_lists=[list(obs) for _ in starts], moving=True, clearance=True)
    assert fleet.lammuz_kernel() == ROWS
    ok = 0
    for i in range(len(starts)):
        at = int(out["arrived_at"][i])
        ok += int(at >= 0 and out["clearance"][:at + 1, i].min() > 0.0)
    print(f"robust mode (central path at mu = 1e-3), corridor as one 16-member fleet rollout: {ok} / 16")
    fleet.close()
    assert ok >= 13, ok


def test_mixed_modes_are_refused(hip):
    """all members or none in the interior-point mode: a mix is RDA_ERR_UNSUPPORTED, and the Python constructor says why"""
    from rda_planner_amd.rda_solver import RDA_solver
    from rda_planner_amd.mpc import MPC
    from rda_planner_amd.fleet import Fleet
    car_t = sc.rectangle_robot()
    a = RDA_solver(6, car_t, 4, 5, iter_num=2, time_print=False, lmz_central=1e-3)
    b = RDA_solver(6, car_t, 4, 5, iter_num=2, time_print=False)
    for pair in ((a, b), (b, a)):
        arr = (C.c_void_p * 2)(pair[0]._be.handle, pair[1]._be.handle)
        F = C.c_void_p()
        assert hip.fleet_create(arr, 2, C.byref(F)) == RDA_ERR_UNSUPPORTED
    msg = hip.lib.rda_strerror(RDA_ERR_UNSUPPORTED).decode()
    assert "norm2 robot" in msg and "mixed" in msg and "interior-point mode in a fleet" not in msg
    path = sc.line_path([4, 20, 0], [24, 20, 0], 0.1)
    kw = dict(receding=6, iter_num=2, max_edge_num=4, max_obs_num=5)
    with pytest.raises(RuntimeError, match="all members or none use lmz_central"):
        Fleet([MPC(car_t, [p.copy() for p in path], lmz_central=1e-3, **kw), MPC(car_t, [p.copy() for p in path], **kw)])
