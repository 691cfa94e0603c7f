"""-m gpu : parity of the HIP kernels against the CPU oracle through the C-ABI (include/rda_hip.h).

Tolerances (all fp64):
  * LamMuZ unique quantities (cost, m, H) and z .................. 1e-10
  * LamMuZ (lam, mu) where the minimiser is not an exact tie ...... 1e-9
  * su-problem s, u, d ............................................ 1e-6  (both sides stop their interior
    point method at the same 1e-9 / 1e-10 / 1e-11 residual thresholds; dense Cholesky vs Riccati rounding can
    shift the stop by one iteration, worth <= 2e-7 on the weakly convex ro1 = 1 case, ~1e-11 typically)
  * closed loop (state re-synchronised to the oracle every step) .. 1e-6 on the applied control
"""
import ctypes as C
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import pytest

import helpers as hp
from oracle.oracle_backend import switches
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import Info, dptr, iptr

pytestmark = pytest.mark.gpu


def _cmp_lammuz(o, h):
    lo, mo, zo, co = o
    lh, mh, zh, ch = h
    assert np.abs(co - ch).max() < 1e-10
    assert np.abs(zo - zh).max() < 1e-10
    d = np.maximum(np.abs(lo - lh).max(axis=1), np.abs(mo - mh).max(axis=1))
    tie = d > 1e-9
    # an exact tie between two basic solutions may be broken differently: identical cost to the last bits
    assert tie.mean() < 0.01 and np.abs(co[tie, 0] - ch[tie, 0]).max(initial=0) < 1e-13
    return int(tie.sum())


@pytest.mark.parametrize("seed,B,E,circles", [(0, 2000, 4, 0.25), (1, 1500, 5, 0.0), (2, 1000, 8, 0.1), (3, 777, 3, 0.5)])
def test_lammuz_batch_random(orc, hip, seed, B, E, circles):
    rng = np.random.default_rng(seed)
    inp = hp.lammuz_batch_inputs(rng, B, E=E, circles=circles)
    _cmp_lammuz(hp.oracle_lammuz_batch(orc, inp), hp.hip_lammuz_batch(hip, inp))


def test_lammuz_modes_and_parameters(orc, hip):
    rng = np.random.default_rng(5)
    inp = hp.lammuz_batch_inputs(rng, 600)
    for ro2, delta, acc in ((1.0, 1e-6, 0), (5.0, 1e-6, 1), (0.3, 1e-3, 1)):
        _cmp_lammuz(hp.oracle_lammuz_batch(orc, inp, ro2=ro2, delta=delta, accelerated=acc),
                    hp.hip_lammuz_batch(hip, inp, ro2=ro2, delta=delta, accelerated=acc))


def test_lammuz_edge_cases(orc, hip):
    rng = np.random.default_rng(9)
    inp = hp.lammuz_batch_inputs(rng, 9, circles=0.0)          # ragged batch (not a multiple of 4 waves)
    inp["A"][0] = 0; inp["b"][0] = 0                           # padding-only obstacle
    inp["A"][1], inp["b"][1] = hp.random_polygon(rng, inp["p"][1], 4, 8.0, 4)   # robot inside the obstacle
    inp["xi"][2] = [3.0, -2.0]; inp["zeta"][3] = -50.0; inp["zeta"][4] = 50.0
    o = hp.oracle_lammuz_batch(orc, inp)
    h = hp.hip_lammuz_batch(hip, inp)
    _cmp_lammuz(o, h)
    assert np.all(h[0][0] == 0) and np.isfinite(h[3]).all()
    one = {k: v[:1] for k, v in inp.items()}                   # B = 1
    _cmp_lammuz(hp.oracle_lammuz_batch(orc, one), hp.hip_lammuz_batch(hip, one))


def test_lammuz_golden(hip):
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "lammuz_golden.json")))
    inp = {k: np.array(v) for k, v in gold["inputs"].items()}
    inp["cone"] = inp["cone"].astype(np.int32)
    lam, mu, z, cmh = hp.hip_lammuz_batch(hip, inp)
    assert np.abs(cmh - np.array(gold["cmh"])).max() < 1e-10 and np.abs(z - np.array(gold["z"])).max() < 1e-10
    ok = np.array(gold["unique"], bool)
    assert np.abs(lam - np.array(gold["lam"]))[ok].max() < 1e-8 and np.abs(mu - np.array(gold["mu"]))[ok].max() < 1e-8


def test_lammuz_full_size_properties(hip):
    """BASELINE full size (N*T = 40 000 sub-problems): size-independent properties instead of the oracle -
    feasibility, permutation invariance over the batch, and idempotence of a second identical launch"""
    rng = np.random.default_rng(4)
    inp = hp.lammuz_batch_inputs(rng, 40000, circles=0.0)
    lam, mu, z, cmh = hp.hip_lammuz_batch(hip, inp)
    a = np.einsum("bek,be->bk", inp["A"], lam)
    assert (lam >= 0).all() and (mu >= 0).all() and (z >= 0).all() and (np.linalg.norm(a, axis=1) <= 1 + 1e-9).all()
    perm = rng.permutation(40000)
    l2, m2, z2, c2 = hp.hip_lammuz_batch(hip, {k: v[perm] for k, v in inp.items()})
    assert np.array_equal(l2, lam[perm]) and np.array_equal(m2, mu[perm]) and np.array_equal(c2, cmh[perm])
    l3, m3, z3, c3 = hp.hip_lammuz_batch(hip, inp)
    assert np.array_equal(l3, lam) and np.array_equal(c3, cmh)


@pytest.mark.parametrize("T,N,dyn,acc,ro1", [(5, 3, 0, 1, 200), (10, 5, 1, 0, 300), (20, 20, 2, 1, 200), (30, 50, 0, 1, 1.0),
                                             (10, 200, 1, 1, 200), (20, 200, 0, 1, 300), (20, 2000, 0, 1, 200), (64, 7, 1, 1, 200),
                                             (25, 40, 0, 1, 200)])
def test_su_solve(orc, hip, T, N, dyn, acc, ro1):
    rng = np.random.default_rng(T * 1000 + N)
    cfg = hp.make_cfg(T=T, N=N, dynamics=dyn, accelerated=acc, ro1=ro1)
    si = hp.su_inputs(rng, cfg)
    so = hp.su_solve(orc.lib.orc_su_solve, cfg, si)
    sh = hp.su_solve(hip.lib.rda_su_solve, cfg, si)
    assert so[0] == 0 and sh[0] == 0
    assert abs(so[4] - sh[4]) <= 1                            # same interior-point iteration count (+-1 at the threshold)
    for k in (1, 2, 3):
        assert np.abs(so[k] - sh[k]).max() < 1e-6


def _pair(kw, car_t, path, oracle_backend):
    from rda_planner_amd.mpc import MPC
    return (MPC(car_t, [p.copy() for p in path], sample_time=0.1, _backend=oracle_backend, **kw),
            MPC(car_t, [p.copy() for p in path], sample_time=0.1, **kw))


@pytest.mark.parametrize("dyn", ["acker", "diff", "omni"])
def test_closed_loop_polygons(dyn):
    """C2/C3-style scene (static boxes), all three kinematics, iter_num=3: identical controls, residuals,
    iteration counts and dual state step after step"""
    from oracle.oracle_backend import oracle_backend
    car_t = sc.rectangle_robot(dynamics=dyn, wheelbase=3.0 if dyn == "acker" else 0)
    path = sc.line_path([4, 25, 0], [40, 25, 0], 0.1)
    clear = np.array([[p[0, 0], p[1, 0]] for p in path[::10]])
    obstacles = sc.scene_boxes(20, (8, 14), (40, 36), keep_clear=clear, clear_radius=3.5)
    kw = dict(receding=12, iter_num=3, max_edge_num=4, max_obs_num=20)
    cpu, gpu = _pair(kw, car_t, path, oracle_backend)
    state = path[0].copy().reshape(3, 1)
    if dyn == "omni":
        state[2, 0] = 0.0
    for i in range(40):
        uc, ic = cpu.control(state.copy(), 4.0, list(obstacles))
        ug, ig = gpu.control(state.copy(), 4.0, list(obstacles))
        assert ic["iters"] == ig["iters"], i
        assert np.abs(uc - ug).max() < 1e-6, (i, np.abs(uc - ug).max())
        assert abs(ic["resi_dual"] - ig["resi_dual"]) < 1e-6 * (1 + ic["resi_dual"]) and abs(ic["resi_pri"] - ig["resi_pri"]) < 1e-6
        sc_, sg_ = cpu.rda.get_state(), gpu.rda.get_state()
        for k in sc_:
            assert np.abs(sc_[k] - sg_[k]).max() < 1e-5, (i, k)
        gpu.rda.set_state(sc_)                                # re-synchronise: isolate the per-step error
        gpu.cur_vel_array = cpu.cur_vel_array.copy()
        state = sc.kinematic_step(state, uc, car_t, 0.1)


def test_closed_loop_dynamic_obstacles_and_quirks():
    """C4-style: moving polygons (per-stage A, b lists), fewer obstacles than slots (padding Q3), distance
    re-sorting every step (Q5), then an empty obstacle list (Q9) and reset() (Q6)"""
    from oracle.oracle_backend import oracle_backend
    car_t = sc.rectangle_robot(dynamics="acker")
    path = sc.line_path([4, 25, 0], [40, 25, 0], 0.1)
    clear = np.array([[p[0, 0], p[1, 0]] for p in path[::10]])
    obstacles = sc.scene_polygons(9, lo=(8, 14), hi=(40, 36), moving=True, keep_clear=clear, clear_radius=4.0)
    kw = dict(receding=10, iter_num=2, max_edge_num=4, max_obs_num=12, ro1=300)
    cpu, gpu = _pair(kw, car_t, path, oracle_backend)
    state = path[0].copy().reshape(3, 1)
    for i in range(12):
        lst = list(obstacles) if i != 6 else []
        uc, ic = cpu.control(state.copy(), 4.0, list(lst))
        ug, ig = gpu.control(state.copy(), 4.0, list(lst))
        assert ic["iters"] == ig["iters"] and np.abs(uc - ug).max() < 1e-6, i
        if i == 8:
            cpu.reset(); gpu.reset()
        sc_, sg_ = cpu.rda.get_state(), gpu.rda.get_state()
        for k in sc_:
            assert np.abs(sc_[k] - sg_[k]).max() < 1e-5, (i, k)
        state = sc.kinematic_step(state, uc, car_t, 0.1)


def test_closed_loop_path_track_golden_and_no_collision():
    """BASELINE C1 on the GPU: the committed golden controls, then the whole run to the goal"""
    from rda_planner_amd.mpc import MPC
    car_d = sc.rectangle_robot(wheelbase=0, dynamics="diff")
    ref = sc.path_track_ref()
    obs = sc.scene_path_track()
    mpc = MPC(car_d, [r.copy() for r in ref], receding=10, sample_time=0.1, iter_num=2, obstacle_order=True, ro1=300,
              max_edge_num=4, max_obs_num=11, slack_gain=8)
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "path_track_diff_golden.json")))
    state = np.array([[10.0], [42.0], [1.57]])      # robot state of path_track_diff.yaml:13
    minc, arrived = np.inf, False
    for i in range(500):
        u, info = mpc.control(state, 4, list(obs))
        if i < 40:
            assert np.abs(u.ravel() - np.array(gold["u"][i])).max() < 1e-5, i
        state = sc.kinematic_step(state, u, car_d, 0.1)
        minc = min(minc, sc.clearance(car_d, state, obs))
        if info["arrive"]:
            arrived = True
            break
    assert arrived and minc > 0.05


def test_device_resident_replay_equals_host_steps(hip):
    """rda_upload_trace / rda_enqueue_step (what bench.py times) == rda_step called step by step"""
    from rda_planner_amd.rda_solver import RDA_solver
    rng = np.random.default_rng(3)
    car_t = sc.rectangle_robot()
    T, N, K = 10, 16, 6
    obstacles = sc.scene_polygons(N, lo=(5, -8), hi=(25, 8), seed=7)
    a = RDA_solver(T, car_t, 4, N, iter_num=3, time_print=False)
    b = RDA_solver(T, car_t, 4, N, iter_num=3, time_print=False)
    from rda_planner_amd.mpc import MPC
    conv = MPC.__new__(MPC); conv.receding = T; conv.dt = 0.1; conv.state = np.zeros((3, 1))
    rl = MPC.convert_rda_obstacle(conv, obstacles, np.zeros((3, 1)), False)
    n, A, bb, cone, per_t = a._stage(list(rl))
    noms, nomu, refs = [], [], []
    for k in range(K):
        cfg = hp.make_cfg(T=T, N=N)
        si = hp.su_inputs(rng, cfg)
        noms.append(si["nom_s"]); nomu.append(si["nom_u"]); refs.append(si["ref"])
    noms, nomu, refs = map(lambda x: np.ascontiguousarray(np.array(x)), (noms, nomu, refs))
    speed = np.full(K, 4.0)
    outs = []
    for k in range(K):
        u, info = a.iterative_solve(noms[k], nomu[k], [refs[k][:, i:i + 1] for i in range(T + 1)], 4.0, list(rl))
        outs.append((u, info["iters"], info["resi_dual"]))
    h = b._be.handle
    assert hip.lib.rda_upload_obstacles(h, n, dptr(A), dptr(bb), iptr(cone), per_t) == 0
    assert hip.lib.rda_upload_trace(h, K, dptr(noms), dptr(nomu), dptr(refs), dptr(speed)) == 0
    for k in range(K):
        assert hip.lib.rda_enqueue_step(h, k) == 0
    assert hip.lib.rda_sync(h) == 0
    for k in range(K):
        u = np.zeros((2, T)); s = np.zeros((3, T + 1)); info = Info()
        assert hip.lib.rda_fetch_result(h, k, dptr(u), dptr(s), C.byref(info)) == 0
        assert np.array_equal(u, outs[k][0]) and info.iters == outs[k][1] and info.resi_dual == outs[k][2]


def test_error_codes(hip):
    from rda_planner_amd._capi import Cfg
    cfg = hp.make_cfg(T=10, N=4, E=9)
    hnd = C.c_void_p()
    assert hip.create(C.byref(cfg), dptr(hp.G), dptr(hp.H), C.byref(hnd)) == -2      # RDA_ERR_UNSUPPORTED (E above the compiled limit)
    cfg = hp.make_cfg(T=200, N=4)
    assert hip.create(C.byref(cfg), dptr(hp.G), dptr(hp.H), C.byref(hnd)) == -2
    assert hip.lib.rda_enqueue_step(None, 0) == -1                                    # RDA_ERR_ARG
    assert b"unsupported" in hip.lib.rda_strerror(-2)


@pytest.mark.parametrize("world,n_obs,su_pre", [(2, 6, 1), (2, 5, 1), (3, 7, 1), (2, 6, 0), (8, 200, 1), (4, 2001, 1)])
def test_obstacle_shards_emulated_ranks_one_gpu(hip, world, n_obs, su_pre):
    """N>1 path of the HIP library on one device: `world` handles act as the ranks of an obstacle shard, the per-iteration
    all-gather is emulated on the host (rda_shard_get_chunk / set_chunks).  All ranks must agree bit for bit with each
    other, and with the un-sharded solve up to the summation order of the su-problem's obstacle reductions.  Uneven shards
    (N % world != 0): ceil(N / world) slots per rank, the padding slots must be invisible.
    su_pre = 0: the raw-term su set-up reads g = G'mu + xi, which is local to the owning rank - rda_shard_config forces
    the reduced form for world > 1, so a handle created with su_pre = 0 must give the same answers.  And: rda_reset / rda_set_state on
    a sharded handle that has stepped are refused (the remote slots' local terms cannot be rebuilt on this rank)."""
    from rda_planner_amd.rda_solver import RDA_solver, hip_options
    from rda_planner_amd.sharded import ShardedRDA
    from test_sharded_gloo import _problem
    import ctypes
    car_t, T, N, rl, steps = _problem(n_obs, 8 if n_obs <= 50 else 20)       # (the last two: BASELINE sizes, 25 / 501 slots per rank, uneven at 2001)
    single = RDA_solver(T, car_t, 4, N, iter_num=3, time_print=False)
    ranks = [RDA_solver(T, car_t, 4, N, iter_num=3, time_print=False, hip_opts=hip_options(su_pre=su_pre)) for _ in range(world)]
    sh = [ShardedRDA(ranks[r], r, world, lambda c: c) for r in range(world)]
    api = hip
    for nom_s, nom_u, ref in steps:
        us, infos = [], []
        # drive the ranks iteration by iteration (what `world` processes would do concurrently)
        for r in range(world):
            s = ranks[r]
            n_obs_, A, b, cone, per_t = s._stage(list(rl))
            assert api.upload_obstacles(sh[r].h, n_obs_, dptr(A), dptr(b), iptr(cone), per_t) == 0
            refa = np.ascontiguousarray(np.hstack(ref)[0:3, :])
            assert api.admm_begin(sh[r].h, dptr(np.ascontiguousarray(nom_s)), dptr(np.ascontiguousarray(nom_u)), dptr(refa), 4.0) == 0
        for it in range(3):
            stop = [ctypes.c_int(0) for _ in range(world)]
            for r in range(world):
                assert api.admm_su(sh[r].h, it, ctypes.byref(stop[r])) == 0
            assert len({s_.value for s_ in stop}) == 1
            if stop[0].value:
                break
            chunks = []
            for r in range(world):
                assert api.admm_lammuz(sh[r].h) == 0
                c = np.zeros(sh[r].chunk)
                assert api.shard_get_chunk(sh[r].h, dptr(c)) == 0
                chunks.append(c)
            everyone = np.concatenate(chunks)
            for r in range(world):
                assert api.shard_set_chunks(sh[r].h, dptr(everyone)) == 0
        for r in range(world):
            u = np.zeros((2, T)); so = np.zeros((3, T + 1)); info = Info()
            assert api.admm_finish(sh[r].h, dptr(u), dptr(so), C.byref(info)) == 0
            us.append(u); infos.append((info.iters, info.resi_dual, info.resi_pri))
        assert all(np.array_equal(us[0], u) for u in us) and all(infos[0] == i for i in infos)
        u1, i1 = single.iterative_solve(nom_s, nom_u, ref, 4.0, list(rl))
        assert i1["iters"] == infos[0][0]
        assert np.abs(u1 - us[0]).max() < 1e-8 and abs(i1["resi_dual"] - infos[0][1]) < 1e-9
    # the duals of every obstacle live on exactly one rank and equal the un-sharded ones
    st1 = single.get_state()
    nloc = -(-N // world)
    for r in range(world):
        st = ranks[r].get_state()
        lo, hi = r * nloc, min((r + 1) * nloc, N)
        for k in ("lam", "mu", "z", "xi", "zeta"):
            assert np.abs(st[k][lo:hi] - st1[k][lo:hi]).max(initial=0) < 1e-7, (r, k)
    assert api.lib.rda_reset(sh[0].h) == -2                  # RDA_ERR_UNSUPPORTED: sharded and stepped
    assert single.reset() is None                             # (an unsharded handle resets as before)


def test_obstacle_shards_rccl_two_gpus():
    """the in-library ncclAllGather path; needs two visible GPUs (skipped on the single-GPU test box)"""
    import subprocess
    import sys
    from rda_planner_amd._lib import hip_api
    if hip_api().lib.rda_device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29611", os.path.join(root, "tools", "rccl_shard_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RCCL_SHARD_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_rccl_path_with_a_one_rank_communicator():
    """what a 1-GPU box can run of the in-library RCCL path: librccl is loaded, ncclGetUniqueId / ncclCommInitRank build a
    one-rank communicator and every ADMM iteration queues the in-place ncclAllGather of the condensed terms on the handle's
    stream (a one-rank gather moves nothing, but symbol resolution, argument types, stream ordering and tear-down are the real
    thing).  Results must EQUAL the plain handle's, also through the device-resident replay (rda_enqueue_step)."""
    from rda_planner_amd.rda_solver import RDA_solver
    from rda_planner_amd.sharded import enable_rccl
    from test_sharded_gloo import _problem
    car_t, T, N, rl, steps = _problem()
    plain = RDA_solver(T, car_t, 4, N, iter_num=3, time_print=False)
    comm = RDA_solver(T, car_t, 4, N, iter_num=3, time_print=False)
    enable_rccl(comm, 0, 1, lambda raw: raw)
    for nom_s, nom_u, ref in steps:
        u0, i0 = plain.iterative_solve(nom_s, nom_u, ref, 4.0, list(rl))
        u1, i1 = comm.iterative_solve(nom_s, nom_u, ref, 4.0, list(rl))
        assert np.array_equal(u0, u1) and i0["iters"] == i1["iters"] and i0["resi_dual"] == i1["resi_dual"]
    s0, s1 = plain.get_state(), comm.get_state()
    for k in s0:
        assert np.array_equal(s0[k], s1[k]), k


def test_rccl_path_in_a_process_that_also_has_torch():
    """what every multi-GPU run looks like (bench.py --gpus N, tools/rccl_shard_check.py): torch - which brings its OWN librccl.so.1 and
    HIP runtime - is imported first, librda_hip.so is loaded into the same process afterwards (it binds to the HIP runtime that is
    already there).  The library must then use the RCCL the process already has: a second copy of librccl next to torch's fails in
    ncclCommInitRank (measured).  One-rank communicator, every step == the plain handle.  Own process: the import order matters.
    (The opposite order - librda_hip.so first, torch second - is not supported by TORCH: it then finds no GPU; INTEGRATION.md.)"""
    import subprocess
    import sys
    code = f"""
import sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import numpy as np
import torch; torch.cuda.init(); x = torch.zeros(4, device='cuda')
from rda_planner_amd.rda_solver import RDA_solver
from rda_planner_amd.sharded import enable_rccl
from test_sharded_gloo import _problem
car_t, T, N, rl, steps = _problem()
plain = RDA_solver(T, car_t, 4, N, iter_num=3, time_print=False)
comm = RDA_solver(T, car_t, 4, N, iter_num=3, time_print=False)
enable_rccl(comm, 0, 1, lambda raw: raw)
for nom_s, nom_u, ref in steps:
    u0, i0 = plain.iterative_solve(nom_s, nom_u, ref, 4.0, list(rl))
    u1, i1 = comm.iterative_solve(nom_s, nom_u, ref, 4.0, list(rl))
    assert np.array_equal(u0, u1) and i0['iters'] == i1['iters']
assert comm._be.api.lib.rda_shard_comm_count(comm._be.handle) == 1
print('RCCL_WITH_TORCH_OK')
"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert "RCCL_WITH_TORCH_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_full_size_step_properties():
    """BASELINE scaling point T=20, N=2000 (40 000 sub-problems per ADMM iteration), where the oracle is too slow to
    be the checker for many steps: size-independent properties of one solver step instead.
      * slot permutation: the su-problem sums over obstacles, the LamMuZ problems are per obstacle -> permuting the
        obstacle slots leaves the control unchanged (up to the summation order of the hinge sums)
      * padding (quirk Q3, rda_solver.py:488-490): n < N obstacles == the same list padded with copies of the last one
      * zero obstacles: pure tracking step, dual side skipped (:625)
      * one step against the oracle (5 ADMM iterations' worth of work, ~seconds on the CPU)"""
    from oracle.oracle_backend import oracle_backend
    from rda_planner_amd.mpc import MPC
    car_t = sc.rectangle_robot()
    path = sc.line_path([5, 25, 0], [45, 25, 0], 0.1)
    clear = np.array([[p[0, 0], p[1, 0]] for p in path[::10]])
    obstacles = sc.scene_polygons(2000, lo=(5, 5), hi=(60, 45), keep_clear=clear, clear_radius=2.5)
    kw = dict(receding=20, iter_num=3, max_edge_num=4, max_obs_num=2000, obstacle_order=False, time_print=False)
    state = path[0].copy().reshape(3, 1)

    def first_controls(obs, steps=3, backend=None, **over):
        extra = {"_backend": backend} if backend is not None else {}
        mpc = MPC(car_t, [p.copy() for p in path], **dict(kw, **over), **extra)
        st, us = state.copy(), []
        for _ in range(steps):
            u, info = mpc.control(st, 4.0, list(obs))
            assert info["status"] == 0 and 1 <= info["iters"] <= 3
            us.append(u.ravel().copy())
            st = sc.kinematic_step(st, u, car_t, 0.1)
        return np.array(us), mpc

    base, mpc0 = first_controls(obstacles)
    perm = np.random.default_rng(3).permutation(2000)
    shuf, _ = first_controls([obstacles[i] for i in perm])
    assert np.abs(base - shuf).max() < 1e-7, np.abs(base - shuf).max()
    short = obstacles[:1500]
    padded, _ = first_controls(short + [short[-1]] * 500)
    auto, _ = first_controls(short)
    assert np.array_equal(padded, auto)
    free, _ = first_controls([])
    assert np.isfinite(free).all() and np.abs(free - base).max() > 0          # the obstacles do act on the control
    lam = mpc0.rda.get_state()["lam"]
    assert (lam >= 0).all() and np.isfinite(lam).all()
    ref, _ = first_controls(obstacles, steps=1, backend=oracle_backend)
    assert np.abs(ref[0] - base[0]).max() < 1e-6, np.abs(ref[0] - base[0]).max()


def test_warm_started_lammuz_equals_enumeration(monkeypatch):
    """k_lammuz accepts the previous support only with an optimality certificate of the full convex problem, so the
    closed loop with the warm start (default) and with plain enumeration (RDA_LMZ_WARM=0) must coincide"""
    from rda_planner_amd.mpc import MPC
    car_t = sc.rectangle_robot()
    path = sc.line_path([5, 25, 0], [45, 25, 0], 0.1)
    clear = np.array([[p[0, 0], p[1, 0]] for p in path[::10]])
    obstacles = sc.scene_polygons(150, lo=(5, 12), hi=(50, 38), keep_clear=clear, clear_radius=2.2) + \
        [sc.circle(20.0, 28.5, 0.8), sc.circle(30.0, 21.5, 0.6, velocity=(0.2, 0.3))]
    runs = []
    for warm in ("1", "0"):
        monkeypatch.setenv("RDA_LMZ_WARM", warm)
        mpc = MPC(car_t, [p.copy() for p in path], receding=15, iter_num=4, max_edge_num=4, max_obs_num=152, time_print=False)
        state = path[0].copy().reshape(3, 1)
        us, its = [], []
        for k in range(60):
            u, info = mpc.control(state, 4.0, list(obstacles))
            us.append(u.ravel().copy()); its.append(info["iters"])
            state = sc.kinematic_step(state, u, car_t, 0.1)
        runs.append((np.array(us), its, mpc.rda.get_state()))
    (ua, ia, sa), (ub, ib, sb) = runs
    assert ia == ib
    # the two runs feed the su-problem duals that differ by rounding (1e-13) wherever the certificate accepted a point the
    # enumeration reaches through another candidate; the su-problem is solved to a tolerance (and, in ADMM iterations >= 1,
    # from the previous multipliers), so its solutions then differ at the level of that tolerance, not of the rounding
    assert np.abs(ua - ub).max() < 5e-6, np.abs(ua - ub).max()
    for k in ("lam", "mu", "z"):
        assert np.abs(sa[k] - sb[k]).max() < 5e-5, (k, np.abs(sa[k] - sb[k]).max())


@pytest.mark.parametrize("name", ["omni_T15_N13", "diff_T10_N13", "omni_T10_N33_restart", "omni_T25_N26_stagnating_dual", "acker_T15_N45_rate_rows_cycle",
                                  "omni_T15_N40_hinge_flips"])
def test_su_hard_instances_from_the_soak_run(orc, hip, name, no_landing):
    """two su-problems on which an earlier kernel left the oracle's iteration path (the hinge screening was only verified
    at convergence and the late fallback restarted from a badly centred point): 44 and 10 interior-point iterations in
    the oracle, the kernel must follow.  The third one used to cycle (100 iterations, then the restart from a more central
    point) until the fraction to the boundary became adaptive; on the fourth the dual residual stagnates at 1e-7 relative
    while the complementarity falls to 1e-17 (the second termination clause accepts it at 1e-12); on the fifth two rate rows traded
    places for ever until cold attempts that pass 25 iterations kept every pair at lam w >= 1e-5 mu, on the sixth a hinge term switched
    on and off for ever until such attempts smooth the hinge terms over 0.1 sqrt(mu) (round 3)"""
    cfg, inp = hp.load_su_case(os.path.join(os.path.dirname(__file__), "golden", "su_hard", name + ".npz"))
    so = hp.su_solve(orc.lib.orc_su_solve, cfg, inp)
    sh = hp.su_solve(no_landing, cfg, inp)                 # (the interior-point paths are compared: landing off on both sides)
    assert so[0] == 0 and sh[0] == 0
    assert abs(so[4] - sh[4]) <= 1, (so[4], sh[4])
    for k in (1, 2, 3):
        assert np.abs(so[k] - sh[k]).max() < 1e-6


def test_su_end_game_noise_instance_converges_in_the_kernel(orc, hip, no_landing):
    """the one su-problem of 32 000 round-4 soak steps on which a side failed - the ORACLE (its dual residual grows from 8e-10 to 3e-5 as mu
    falls below 1e-9, Cholesky breakdown; tests/test_oracle_su.py::test_end_game_lost_in_rounding_returns_the_near_converged_iterate).
    The kernel's cold solve converges (16 iterations); the iterate the checker's safety net returns is of the looser class (mu = 2e-9
    instead of 1e-11: 1e-4 from the kernel's point, see test_stop_tolerance_vs_weakly_active_rows) - within the stated tolerance of the interior-point-only mode, TOL_U_IP."""
    cfg, inp = hp.load_su_case(os.path.join(os.path.dirname(__file__), "golden", "su_hard", "omni_T25_N20_end_game_noise.npz"))
    so = hp.su_solve(orc.lib.orc_su_solve, cfg, inp)
    sh = hp.su_solve(no_landing, cfg, inp)
    assert so[0] == 0 and sh[0] == 0 and sh[4] <= 20, (so[0], sh[0], sh[4])
    d = max(float(np.abs(so[k] - sh[k]).max()) for k in (1, 2, 3))
    print(f"|(s, u, d)_gpu - oracle's accepted iterate| {d:.2e} ({sh[4]} interior-point iterations)")
    assert d <= hp.TOL_U_IP


@pytest.mark.parametrize("name", ["omni_T15_N30_weakly_active_a", "omni_T15_N13_weakly_active_b", "acker_T15_N27_weakly_active_c"])
def test_su_weakly_active_instances_from_the_round4_soak(orc, hip, name):
    """the su-problems behind the largest GPU-vs-oracle control differences of the round-4 soak (weakly active inequality rows, see
    tests/test_oracle_su.py::test_stop_tolerance_vs_weakly_active_rows): the kernel's cold solve against the oracle solved to 1e-12 / 1e-15
    - within 5e-5, a tenth of the stated closed-loop tolerance of the interior-point-only mode (rounds 4-5).  Round 6: the kernel's solve is LANDED (default):
    it ends on the vertex the tight oracle converges to (8e-9 .. 1e-9: what that interior point is still short of it)"""
    import ctypes as C
    cfg, inp = hp.load_su_case(os.path.join(os.path.dirname(__file__), "golden", "su_hard", name + ".npz"))
    with switches(su_tol=(1e-12, 1e-12, 1e-15)):
        so = hp.su_solve(orc.lib.orc_su_solve, cfg, inp)
    sh = hp.su_solve(hip.lib.rda_su_solve, cfg, inp)
    assert so[0] == 0 and sh[0] == 0
    d = max(float(np.abs(so[k] - sh[k]).max()) for k in (1, 2, 3))
    print(f"{name}: |(s, u, d)_gpu - tight oracle| {d:.2e} ({sh[4]} interior-point iterations, tight oracle {so[4]})")
    assert d <= 5e-8 < hp.TOL_U


def test_closed_loop_corridor_example():
    """BASELINE config C2, the reference's corridor example with its default MPC parameters: the GPU path follows the
    oracle step by step (state re-synchronised every step) AND, run on its own, slaloms through to the goal"""
    from oracle.oracle_backend import oracle_backend
    from rda_planner_amd.mpc import MPC
    car_a = sc.rectangle_robot(dynamics="acker")
    path = sc.line_path([0, 20, 0], [60, 20, 0], 0.1)
    obs = sc.scene_corridor(n_extra=0)
    kw = dict(max_edge_num=4, max_obs_num=6)
    cpu, gpu = _pair(kw, car_a, path, oracle_backend)
    state = np.array([[0.0], [20.0], [0.0]])
    for i in range(120):
        uc, ic = cpu.control(state.copy(), 4.0, list(obs))
        ug, ig = gpu.control(state.copy(), 4.0, list(obs))
        assert ic["iters"] == ig["iters"], i
        # close quarters: the steering is weakly determined next to the boxes, both interior-point solves stop at a
        # 1e-9 relative residual -> a few 1e-6 on the control
        assert np.abs(uc - ug).max() < 1e-5, (i, np.abs(uc - ug).max())
        gpu.rda.set_state(cpu.rda.get_state())
        gpu.cur_vel_array = cpu.cur_vel_array.copy()
        state = sc.kinematic_step(state, uc, car_a, 0.1)
    solo = MPC(car_a, [p.copy() for p in path], sample_time=0.1, **kw)
    state = np.array([[0.0], [20.0], [0.0]])
    minc = np.inf
    for i in range(260):
        u, info = solo.control(state, 4.0, list(obs))
        state = sc.kinematic_step(state, u, car_a, 0.1)
        minc = min(minc, sc.clearance(car_a, state, obs))
        if info["arrive"]:
            break
    assert info["arrive"] and minc > 0.2, (info["arrive"], minc)


def test_closed_loop_dynamic_obs_example(orc):
    """The reference's own dynamic scene (example/dynamic_obs/dynamic_obs.yaml:24-32 through the headless world: 7 moving CIRCLES - norm2 obstacle cone,
    per-stage (A, b) lists) with the keywords of dynamic_obs.py:22 (T = 10, iter_num = 2, max_obs_num = 6, min_sd = 0.5, wu = 0.2, max_acce = [10, 1],
    reference speed 6, re-sorted every tick): the GPU path against the COLD oracle (every su-problem from the cold start, like ECOS in the reference)
    step by step at TOL_U_FIXED - state re-synchronised every step - and, run on its own, to the goal without touching anything."""
    from oracle.oracle_backend import oracle_backend
    from rda_planner_amd.mpc import MPC
    import rda_planner_amd.world as irsim
    yaml_path = os.path.join(os.path.dirname(__file__), "golden", "world_dynamic_obs.yaml")
    kw = dict(receding=10, process_num=5, iter_num=2, max_edge_num=4, max_obs_num=6, min_sd=0.5, wu=0.2, obstacle_order=True, time_print=False)
    path = sc.path_track_ref()

    def car_of(env):
        ri = env.get_robot_info()
        return sc.car(ri.G, ri.h, ri.cone_type, ri.wheelbase, [10, 1], [10, 1.0], "acker")
    with switches(**hp.COLD_SU):
        env = irsim.make(yaml_path)
        car_t = car_of(env)
        cpu = MPC(car_t, [p.copy() for p in path], sample_time=0.1, _backend=oracle_backend, **kw)
        gpu = MPC(car_t, [p.copy() for p in path], sample_time=0.1, **kw)
        worst, same, steps = 0.0, 0, 150
        for i in range(steps):
            obs = env.get_obstacle_info_list()
            assert sum(o.cone_type == "norm2" for o in obs) == 7
            uc, ic = cpu.control(env.robot.state.copy(), 6, list(obs))
            ug, ig = gpu.control(env.robot.state.copy(), 6, list(obs))
            assert ic["status"] == 0 and ig["status"] == 0, (i, ic["status"], ig["status"])
            if ic["iters"] == ig["iters"]:
                same += 1
                worst = max(worst, float(np.abs(uc - ug).max()), float(np.abs(cpu.cur_vel_array - gpu.cur_vel_array).max()))
            else:
                assert np.abs(uc - ug).max() <= hp.TOL_U_FLIP, (i, float(np.abs(uc - ug).max()))
            gpu.rda.set_state(cpu.rda.get_state())
            gpu.cur_vel_array = cpu.cur_vel_array.copy()
            gpu._dev_u = None
            env.step(uc)
            if env.done() or ic["arrive"]:
                break
        print(f"dynamic_obs example vs cold oracle: {i + 1} steps, max |du| over the horizon {worst:.2e}, same ADMM iteration count on {same}")
        assert worst <= hp.TOL_U_FIXED and same >= 0.95 * (i + 1), (worst, same, i + 1)
    env = irsim.make(yaml_path)
    solo = MPC(car_of(env), [p.copy() for p in path], sample_time=0.1, **kw)
    minc = np.inf
    for i in range(500):
        u, info = solo.control(env.robot.state, 6, env.get_obstacle_info_list())
        env.step(u)
        minc = min(minc, env.clearance())
        if env.done() or info["arrive"]:
            break
    print(f"dynamic_obs example, GPU path on its own: {i + 1} steps, arrive={info['arrive']}, collided={env.collided}, min clearance {minc:.2f} m")
    assert info["arrive"] and not env.collided and minc > 0.1, (info["arrive"], env.collided, minc)


def test_closed_loop_lidar_example():
    """BASELINE config C3 (example/lidar_nav/lidar_path_track.py): boxes clustered from each lidar scan, max_obs_num=4 - the set of
    obstacles, their order and their number change from tick to tick.  The GPU path follows the oracle step by step (state
    re-synchronised every step) and, run on its own, reaches the goal without touching anything"""
    from oracle.oracle_backend import oracle_backend
    from rda_planner_amd.mpc import MPC
    from rda_planner_amd.lidar import scan_box
    import rda_planner_amd.world as irsim
    yaml_path = os.path.join(os.path.dirname(__file__), "golden", "world_lidar_track.yaml")
    env = irsim.make(yaml_path)
    ri = env.get_robot_info()
    car_t = sc.car(ri.G, ri.h, ri.cone_type, ri.wheelbase, [10, 1], [10, 0.5], "acker")
    kw = dict(receding=10, iter_num=2, max_edge_num=4, max_obs_num=4, obstacle_order=True, wu=1.0, slack_gain=13)
    cpu, gpu = _pair(kw, car_t, sc.path_track_ref(), oracle_backend)
    for i in range(150):
        obs = scan_box(env.robot.state, env.get_lidar_scan())
        uc, ic = cpu.control(env.robot.state.copy(), 4.0, list(obs))
        ug, ig = gpu.control(env.robot.state.copy(), 4.0, list(obs))
        assert ic["iters"] == ig["iters"] and cpu.cur_index == gpu.cur_index, i
        assert np.abs(uc - ug).max() < 1e-6, (i, np.abs(uc - ug).max())
        gpu.rda.set_state(cpu.rda.get_state())
        gpu.cur_vel_array = cpu.cur_vel_array.copy()
        env.step(uc)
    # run on its own the loop is chaotic in this scene (tests/test_host_api.py::test_lidar_example_reaches_the_goal_from_most_starts):
    # the rate of starts that reach the goal is asserted, not one trajectory
    from test_host_api import LIDAR_STARTS, lidar_closed_loop
    runs = [lidar_closed_loop(s) for s in LIDAR_STARTS]
    assert sum(a and not c and mc > 0.0 for a, c, mc, _ in runs) >= 3, runs


@pytest.mark.parametrize("E,dyn,moving", [(4, "acker", False), (3, "diff", True), (6, "omni", False), (8, "acker", True)])
def test_packed_rows_kernel_equals_one_per_wave_kernel(monkeypatch, E, dyn, moving):
    """k_lammuz_rows (four sub-problems per wavefront, default when E+R+1 <= 16) and k_lammuz (one per wavefront,
    RDA_LMZ_ROWS=0) run the same device functions: closed loops over polygons with 3..E edges, circles, padded and truncated
    obstacle lists must agree BIT FOR BIT - controls, iteration counts, residuals and the dual state.  E=8 exercises two
    rounds of (vertex, vertex) pairs per row in the central-normal step, N*T not a multiple of 16 the shadow rows."""
    from rda_planner_amd.mpc import MPC
    car_t = sc.rectangle_robot(dynamics=dyn, wheelbase=3.0 if dyn == "acker" else 0)
    path = sc.line_path([5, 25, 0], [35, 25, 0], 0.1)
    clear = np.array([[p[0, 0], p[1, 0]] for p in path[::10]])
    rng = np.random.default_rng(E)
    obstacles = []
    while len(obstacles) < 37:
        c = rng.uniform((6, 14), (40, 36))
        if np.min(np.linalg.norm(clear - c, axis=1)) < 2.4:
            continue
        k = int(rng.integers(3, E + 1))
        vel = rng.uniform(-0.5, 0.5, 2) if (moving and rng.random() < 0.5) else (0.0, 0.0)
        obstacles.append(sc.regular_polygon(c[0], c[1], k, rng.uniform(0.4, 1.0), rng.uniform(-np.pi, np.pi), vel))
    obstacles += [sc.circle(18.0, 28.6, 0.7), sc.circle(27.0, 21.2, 0.5, velocity=(0.1, 0.2))]
    runs = []
    for rows in ("1", "0"):
        monkeypatch.setenv("RDA_LMZ_ROWS", rows)
        mpc = MPC(car_t, [p.copy() for p in path], receding=11, iter_num=3, max_edge_num=E, max_obs_num=41, time_print=False)
        state = path[0].copy().reshape(3, 1)
        if dyn == "omni":
            state[2, 0] = 0.0
        us, meta = [], []
        for k in range(45):
            cur = [o if not o.velocity.any() else (o._replace(vertex=o.vertex + o.velocity * (0.1 * k)) if o.cone_type == "Rpositive"
                                                   else o._replace(center=o.center + o.velocity * (0.1 * k))) for o in obstacles]
            shown = cur if k % 7 else cur[:20]                      # now and then fewer obstacles than slots (padding, Q3)
            u, info = mpc.control(state, 4.0, list(shown))
            us.append(u.ravel().copy()); meta.append((info["iters"], info["resi_dual"], info["resi_pri"], info["su_ipm_iters"]))
            state = sc.kinematic_step(state, u, car_t, 0.1)
        runs.append((np.array(us), meta, mpc.rda.get_state()))
    (ua, ma, sa), (ub, mb, sb) = runs
    assert ma == mb
    assert np.array_equal(ua, ub), np.abs(ua - ub).max()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k


def test_failure_semantics_degenerate_obstacles_gpu_equals_oracle():
    """NaN / zero-area / non-convex / zero-radius obstacles through the default HIP path (device-side conversion, packed rows)
    and through the one-sub-problem-per-wave kernel: the NaN slot keeps its duals, residual inf, no early stop, counted in
    info['lmz_fail']; everything else as the oracle computes it"""
    from oracle.oracle_backend import oracle_backend
    from test_host_api import _run_degenerate
    want, mc, _ = _run_degenerate({"_backend": oracle_backend})
    for env in ({}, {"RDA_LMZ_ROWS": "0"}, {"device_obstacles": False}):
        kw = {k: v for k, v in env.items() if not k.startswith("RDA_")}
        old = {k: os.environ.get(k) for k in env if k.startswith("RDA_")}
        os.environ.update({k: v for k, v in env.items() if k.startswith("RDA_")})
        try:
            got, mg, printed = _run_degenerate(kw)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        assert "Update Lam Mu Fail" in printed
        for (uc, ic), (ug, ig) in zip(want, got):
            assert ig["lmz_fail"] == ic["lmz_fail"] == 24 and ig["resi_dual"] == np.inf and ig["iters"] == ic["iters"] == 3
            assert np.abs(uc - ug).max() < 1e-6 and abs(ic["resi_pri"] - ig["resi_pri"]) < 1e-6
        sc_, sg_ = mc.rda.get_state(), mg.rda.get_state()
        for k in sc_:
            assert np.isfinite(sg_[k]).all() and np.abs(sc_[k] - sg_[k]).max() < 1e-5, (env, k)


def test_bench_shard_mode_two_ranks_oversubscribed():
    """`bench.py --gpus 2 --mode shard` launched the way the driver launches it, on however many GPUs the box has: with one
    GPU the two ranks share it and exchange their shard chunks over gloo (plumbing of the N > 1 strong-scaling path, uneven
    shards included); with two or more the in-library RCCL all-gather runs"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29633", os.path.join(root, "bench.py"), "--gpus", "2", "--mode", "shard", "--steps", "6", "--warmup", "2",
                          "--n-obs", "21", "--horizon", "10"], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, out.stdout[-1500:] + out.stderr[-3000:]
    d = json.loads(lines[-1])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    err = d.get("max_du_vs_unsharded_closed_loop", d.get("device_resident_replay", {}).get("max_du_vs_python_closed_loop"))
    assert err is not None and err < 1e-8, d


def test_time_print_surface_of_the_reference(capsys):
    """rda_solver.py:587-601 with time_print=True: one 'iteration i time:' line per EXECUTED ADMM iteration (here: the GPU time
    of that iteration's su + LamMuZ kernels), 'iteration early stop: i' when the residual test ended the loop, the total"""
    from rda_planner_amd.rda_solver import RDA_solver
    from test_sharded_gloo import _problem
    car_t, T, N, rl, steps = _problem()
    solver = RDA_solver(T, car_t, 4, N, iter_num=4, time_print=True)
    for nom_s, nom_u, ref in steps:
        capsys.readouterr()
        u, info = solver.iterative_solve(nom_s, nom_u, ref, 4.0, list(rl))
        out = capsys.readouterr().out
        lines = [ln for ln in out.splitlines() if ln.startswith("iteration ") and " time: " in ln and not ln.startswith("iteration time")]
        assert len(lines) == info["iters"], out
        assert [int(ln.split()[1]) for ln in lines] == list(range(info["iters"]))
        assert all(0 < float(ln.split()[-1]) < 0.1 for ln in lines)
        assert "iteration time:" in out
        stopped = info["resi_dual"] < 0.2 and info["resi_pri"] < 0.2
        assert (f"iteration early stop: {info['iters'] - 1}" in out) == stopped
