#!/usr/bin/env python
"""
bench.py - MPC steps/s of the MI355X-native RDA ADMM inner solver (BASELINE.json metric).

    python bench.py --gpus 1 --steps K --warmup W                # plain run: the headline loop and its line, nothing else
    python bench.py --gpus 1 --steps K --warmup W --full         # + every other leg, check, size and roofline described below
    python bench.py ... --dump-outputs DIR                        # + what the last timed step handed back, as DIR/<name>.npy (float64)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W
    python bench.py --only-headline --steps 200 --warmup 10       # the headline loop + its timing pass (what tools/profile_round.sh profiles)

A plain run sets up the workload, runs W warm-up and then EXACTLY K timed steps of the headline closed loop, writes the outputs of the last
timed step when --dump-outputs is given, and prints the line (metric, value, unit, higher_is_better, dtype, ms_per_step = wall time of the
K steps / K, ...).  Everything below that is not the headline figure itself - the recorded Python closed loops and the comparison with them,
the second window, the other legs, `sizes`, rooflines, cpu_baseline, the obstacle-shard leg - runs with --full only.

One "step" = one RDA_solver.iterative_solve (reference rda_solver.py:573-610): up to iter_num
ADMM iterations with early stop.  Workload (north-star point of BASELINE.json / SURVEY.md 8d):
Ackermann rectangle robot, T=20, N_obs=200 static polygons, E=4, synthetic seeded scene.

Protocol: closed loop in the reference's DEFAULT semantics (obstacle_order=True: the obstacle list re-sorted about the
robot on every tick, mpc.py:205-206), W warm-up steps, then EXACTLY K steps, each one a pair of C-ABI calls that takes the robot state
and returns the control with ONE host synchronisation at its end (`rda_tracked_begin` + `rda_scene_resort` + `rda_tracked_finish`:
MPC.pre_process, the re-sort / re-staging of the resident scene, the ADMM loop and the D2H of the control on the device; the host applies
the control to the kinematic model and calls again).  The caller of those K steps is C (tools/closed_loop_host.c, loaded here): C-ABI
calls and the kinematic model only, no interpreter objects between two steps.  The raw obstacle scene is resident in HBM when the timed
region starts.  `value` = K / wall time of those K steps (max over ranks); `median_ms_per_step` is the median of the K per-step wall
times; `second_window` = max(K, 50) more steps of the same loop right behind them (the metric's own protocol, SURVEY.md 8d: the median
of >= 50 timed steps); `residuals` = where the ADMM of the timed steps ends against iter_threshold.  Reported beside it, never as `value`:
  * `fixed_slot_binding`    - obstacle_order=False (slots bound once, `rda_step_tracked`: the protocol of rounds 2-3);
  * `su_hard_warm_off`      - the headline loop without the start rule that is default since round 5 (opt-out leg);
  * `lammuz_interior_point_closed_loops` - the robust LamMuZ mode (lmz_central = 1e-3) and a circle robot, in the headline protocol AND
                              with a fixed binding;
  * `pcie_inclusive`        - the raw scene (vertices, velocities) handed over from host memory on every tick;
  * `device_resident_replay`- the recorded step inputs replayed back-to-back with no per-step synchronisation;
  * the same closed loop through the Python `MPC.control` API with host / device obstacle staging; multi-ego legs; `sizes`.
A Python closed loop first records the W+K step inputs; every other leg must reproduce its controls.

N > 1: one process per GPU, independent ego replicas (BASELINE config "batched multi-ego":
scenario batch sharded, no data-path collective) - weak scaling, value = sum over ranks.

The pieces live in benchlib/ (workload, closed_loop, roofline, cpu_baseline, legs); this file is the entry point and the assembly of
the ONE JSON line.
"""
import os
os.environ.setdefault("OMP_PROC_BIND", "close")   # cpu_baseline leg: keep the oracle's OpenMP threads on neighbouring cores (read when libgomp loads)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # the multi-ego leg runs one HIP stream per ego; the default 4 hardware queues serialise them
import argparse
import json
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from benchlib import closed_loop, compact, cpu_baseline, legs, roofline       # noqa: E402
from benchlib.context import Ctx, stats                              # noqa: E402
from benchlib.workload import build_workload, record_trace           # noqa: E402,F401  (tools/ import them from here)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)     # 200 timed MPC steps = 80 m of driving
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n-obs", type=int, default=200)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--full", action="store_true", help="every leg, check, size, roofline and baseline besides the headline loop (a plain run "
                    "times the headline loop and prints its line, nothing else)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps write what the last one handed back (applied "
                    "control, robot state, residuals, solver duals) as DIR/<name>.npy, float64, <= 64 MB in all")
    ap.add_argument("--only-headline", action="store_true", help="the headline closed loop (+ its hipEvent timing pass) and nothing else: no recorded "
                    "traces, no comparison, no other leg - every kernel launch of the process belongs to the loop `value` comes from (profiles)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--moving", action="store_true", help="moving obstacles: per-stage (A, b) over the horizon (dynamic_obs config)")
    ap.add_argument("--egos", type=int, default=16, help="extra leg: this many independent egos concurrently on one GPU (0/1 = skip)")
    ap.add_argument("--fleet-egos", type=int, default=64, help="extra leg: this many egos stepped as one fleet (batched launches; 0/1 = skip)")
    ap.add_argument("--no-ip-legs", action="store_true", help="skip the interior-point LamMuZ closed loops (extra keys)")
    ap.add_argument("--duals-follow-leg", action="store_true", help="extra leg: the headline loop with the opt-in duals_follow (NOT reference semantics)")
    ap.add_argument("--no-shard-leg", action="store_true", help="N > 1, replica mode: skip the extra obstacle-shard leg (one ego, N_obs = --shard-n-obs)")
    ap.add_argument("--force-shard-leg", action="store_true", help="run the obstacle-shard leg on ONE GPU with a one-rank communicator (plumbing check)")
    ap.add_argument("--shard-n-obs", type=int, default=2000)
    ap.add_argument("--shard-leg-timeout", type=float, default=120.0)
    ap.add_argument("--no-sizes", action="store_true", help="skip the `sizes` legs (N=20, N=2000, C4, C5 shape: one short sub-run of this script each)")
    ap.add_argument("--sizes-budget-s", type=float, default=120.0, help="wall-clock budget of the `sizes` legs; a leg that would start after it is skipped (and says so)")
    ap.add_argument("--size-leg", action="store_true", help="(internal) reduced set of legs: what one entry of `sizes` needs")
    ap.add_argument("--cpu-threads", type=int, default=0, help="cpu_baseline with this one thread count instead of the sweep")
    ap.add_argument("--mode", choices=["replicas", "shard"], default="replicas",
                    help="N>1: independent ego replicas (default, no collective) or ONE ego whose obstacles are sharded over the ranks "
                         "with an RCCL all-gather per ADMM iteration (strong scaling, --n-obs = total obstacles)")
    args = ap.parse_args()
    if args.size_leg:                                   # one entry of `sizes`: the closed loops, the timed replay, one cpu_baseline sample
        args.egos, args.no_ip_legs, args.no_sizes, args.full = 0, True, True, True
    if args.dump_outputs and args.mode == "shard" and args.gpus > 1:
        ap.error("--dump-outputs: the obstacle-shard mode has no headline closed loop to take the outputs from")
    return args


def setup(args):
    """process group, C-ABI, workload"""
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist, oversub, ndev, dev_index, tdev = None, False, 1, 0, "cpu"
    if args.force_shard_leg:
        import torch                               # torch (its HIP runtime, its RCCL) must be in the process BEFORE librda_hip.so is loaded
        torch.cuda.init()
    if world > 1:
        import torch
        import torch.distributed as dist
        ndev = torch.cuda.device_count()
        oversub = ndev < world                     # fewer GPUs than ranks (plumbing test on a 1-GPU box): gloo + shared device
        dev_index = local_rank % max(ndev, 1)
        torch.cuda.set_device(dev_index)
        if oversub:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        tdev = "cpu" if oversub else "cuda"
    from rda_planner_amd._lib import hip_api
    api = hip_api()
    api.lib.rda_set_device(dev_index if world > 1 else local_rank)
    K, W = args.steps, args.warmup
    shard = args.mode == "shard" and world > 1
    car_t, path, obstacles, kw = build_workload(seed_offset=0 if shard else rank, n_obs=args.n_obs, T=args.horizon, n_steps=K + W, moving=args.moving)
    ctx = Ctx(args=args, api=api, rank=rank, world=world, dist=dist, tdev=tdev, shard=shard, oversub=oversub, ndev=ndev,
              car_t=car_t, path=path, obstacles=obstacles, kw=kw, kw_rec=dict(kw, obstacle_order=False), T=kw["receding"], N=kw["max_obs_num"],
              K=K, W=W, path_length=max(40.0, 0.4 * (K + W) + 12.0))

    def make_sharded(solver):
        """obstacle shards + in-library ncclAllGather; the 128-byte unique id travels over torch.distributed"""
        if not shard or oversub:            # ranks sharing one GPU cannot form an RCCL communicator: host-driven exchange (legs.oversubscribed_shard_run)
            return
        import torch
        from rda_planner_amd.sharded import enable_rccl

        def bcast(buf):
            t = torch.zeros(128, dtype=torch.uint8, device="cuda")
            if rank == 0:
                t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).clone().cuda()
            dist.broadcast(t, 0)
            return bytes(t.cpu().numpy().tobytes())
        enable_rccl(solver, rank, world, bcast)
    ctx.make_sharded = make_sharded
    return ctx


PROTOCOL_STATIC = ("closed loop through the C-ABI, caller in C (tools/closed_loop_host.c), the reference's default obstacle_order=True: per step "
                   "rda_tracked_begin(state) + rda_scene_resort(state) + rda_tracked_finish -> control (the resident scene is re-sorted about the robot "
                   "and the nearest max_obs_num re-staged by k_keys / k_rank / k_build / k_prepare INSIDE the timed region, mpc.py:205-206), one host "
                   "sync per step, host applies the control to the kinematic model; raw scene resident in HBM")
PROTOCOL_MOVING = ("closed loop through the C-ABI, caller in C (tools/closed_loop_host.c), obstacles advance every tick and are re-sorted "
                   "(obstacle_order=True): rda_tracked_begin + rda_upload_scene_async(order=1) + rda_tracked_finish per step")


def rooflines(ctx, kt, lm_kernel, n_exec):
    """the two solver kernels of a loop: (dominant, secondary, r_su, r_lm)"""
    kw, T, N = ctx.kw, ctx.T, ctx.N
    E, R = kw["max_edge_num"], 4
    n_loc = -(-N // ctx.world) if ctx.shard else N
    su_name = f"k_su<{T}>" if T in (10, 20, 25, 30) else "k_su<0>"
    J = -(-n_loc // 8)
    r_lm = roofline.roof(lm_kernel, kt["k_lammuz"], roofline.unit_bytes(E, R) * n_loc * T, n_exec)
    r_su = roofline.roof(su_name, kt["k_su"], roofline.su_bytes(T, n_loc, ctx.world if ctx.shard else 1), n_exec)
    r_su["includes"] = f"k_su_tracked<{T}> (first solve of every tick) and {su_name} launches of the timed closed loop"
    # latency roof of the su kernel: ONE workgroup (4 waves) on one CU walks a dependent chain; what bounds it is the length of
    # that chain, not bytes - stated next to the HBM fraction so the fraction is not read as a bandwidth problem
    r_su["cus_occupied"] = 1
    r_lm["cus_occupied"] = min(256, (T * J * 128 + 255) // 256) if "rows" in lm_kernel or "k_lammuz_ip" in lm_kernel else min(256, (n_loc * T + 63) // 64)
    if ctx.world == 1:
        roofline.attach_traffic(ROOT, r_su, r_lm, N, T, ctx.args.moving, lm_kernel)
        roofline.attach_issue(ROOT, r_su, r_lm, N, T, ctx.args.moving)
    dominant, secondary = (r_su, r_lm) if r_su["total_ms"] >= r_lm["total_ms"] else (r_lm, r_su)
    return dominant, secondary


def base_line(ctx, value, ms_step, protocol):
    args, kw, T, N, world = ctx.args, ctx.kw, ctx.T, ctx.N, ctx.world
    kind_word = "moving" if args.moving else "static"
    return {
        "metric": f"MPC steps/sec (ADMM early stop or iter_num cap: see residuals), T={T}, N_obs={N}", "value": round(value, 3), "unit": "steps/s",
        "n_gpus": world, "steps": ctx.K, "warmup": ctx.W, "ms_per_step": round(ms_step, 5),
        "higher_is_better": True, "scaling": "strong" if ctx.shard else "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"north-star: acker rectangle robot, T={T}, N_obs={N} {kind_word} seeded polygons, E={kw['max_edge_num']}, iter_num={kw['iter_num']}, iter_threshold=0.2, ro1={kw['ro1']}",
                   "parallelism": "single GPU" if world == 1 else (f"one ego, obstacles sharded {world}-way, RCCL all-gather per ADMM iteration" if ctx.shard else f"{world} independent ego replicas (no collective)"),
                   "protocol": protocol, "env_switches": {k: v for k, v in os.environ.items() if k.startswith("RDA_")}},
    }


DUMP_BYTES = 64 << 20


def dump_outputs(d, outputs):
    """outputs of the last timed step -> d/<name>.npy (float64).  Should they pass DUMP_BYTES (huge scenes), every array is cut to the same
    fixed, seeded sample of obstacle slots (its first axis)."""
    os.makedirs(d, exist_ok=True)
    total = sum(a.nbytes for a in outputs.values())
    if total > DUMP_BYTES:
        per_slot = sum(a.nbytes // a.shape[0] for a in outputs.values() if a.ndim > 1)
        n_slots = max(a.shape[0] for a in outputs.values() if a.ndim > 1)
        keep = np.sort(np.random.default_rng(0).choice(n_slots, min(n_slots, (DUMP_BYTES - 4096) // max(per_slot, 1)), replace=False))
        outputs = {k: (a[keep] if a.ndim > 1 and a.shape[0] == n_slots else a) for k, a in outputs.items()}
        outputs["sampled_slots"] = keep.astype(np.float64)
    for name, a in outputs.items():
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(a, np.float64))


def print_line(out):
    """the one stdout line of a plain run (no detail file is written)"""
    line = json.loads(compact.line(out))
    line.pop("detail", None)
    print(json.dumps(line, separators=(",", ":")), flush=True)


def plain(ctx):
    """a plain run: warm-up, the K timed steps of the headline loop, its outputs (--dump-outputs) and the line - no recorded Python closed loop,
    no comparison, no second window, no timing pass, no other leg (--full)"""
    args, K = ctx.args, ctx.K
    hd = closed_loop.run(ctx, per_tick_scene=bool(args.moving), ordered=True, compare=False, second_window=False, outputs=bool(args.dump_outputs))
    if ctx.rank != 0:
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, hd.outputs)
    out = base_line(ctx, K * ctx.world / hd.elapsed, hd.elapsed / K * 1e3, PROTOCOL_MOVING if args.moving else PROTOCOL_STATIC)
    out["median_ms_per_step"] = round(float(np.median(hd.times) * 1e3), 5)
    out["mean_admm_iters"] = round(float(np.mean(hd.iters)), 3)
    out["residuals"] = closed_loop.residual_summary(hd.info, 0.2)
    if hd.elapsed_per_rank:
        out["per_rank_steps_per_s"] = [round(K / e, 3) for e in hd.elapsed_per_rank]
    print_line(out)


def headline_only(ctx):
    """--only-headline: the loop `value` comes from, its hipEvent timing pass, nothing else"""
    args, K = ctx.args, ctx.K
    hd = closed_loop.run(ctx, per_tick_scene=bool(args.moving), ordered=True, compare=False, outputs=bool(args.dump_outputs))
    tm = closed_loop.run(ctx, per_tick_scene=bool(args.moving), ordered=True, timing=True, compare=False)
    if ctx.rank != 0:
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, hd.outputs)
    out = base_line(ctx, K * ctx.world / hd.elapsed, hd.elapsed / K * 1e3, PROTOCOL_MOVING if args.moving else PROTOCOL_STATIC)
    out["median_ms_per_step"] = round(float(np.median(hd.times) * 1e3), 5)
    out["mean_admm_iters"] = round(float(np.mean(hd.iters)), 3)
    out["residuals"] = closed_loop.residual_summary(hd.info, 0.2)
    out["second_window"] = hd.second_window
    out["roofline"], out["roofline_secondary"] = rooflines(ctx, tm.kernel_ms, tm.lmz_kernel, int(np.sum(tm.iters)))
    out["only_headline"] = True
    compact.emit(out, "bench_detail_only_headline.json")


def main():
    args = parse_args()
    ctx = setup(args)
    rank, world, dist, shard, K, W, T, N, kw = ctx.rank, ctx.world, ctx.dist, ctx.shard, ctx.K, ctx.W, ctx.T, ctx.N, ctx.kw
    if (args.only_headline or not args.full) and not shard:
        (headline_only if args.only_headline else plain)(ctx)
        if dist is not None:
            dist.destroy_process_group()
        return
    # obstacle slots must not be re-sorted between recording and replay: record with the distance
    # order of the first step frozen (static scene), i.e. obstacle_order only affects slot binding
    ctx.trace, ctx.staged, mpc_rec = record_trace(ctx.car_t, ctx.path, ctx.obstacles, ctx.kw_rec, W + K, post_init=ctx.make_sharded)
    cl_dev = cl_trk = None
    if rank == 0 and not shard:
        if not args.size_leg:
            cl_dev = legs.python_api_closed_loop(ctx, False)
            cl_trk = legs.python_api_closed_loop(ctx, True)
        # the reference's default: obstacle_order=True, the list re-sorted by distance on EVERY tick (mpc.py:205-206).  That closed loop
        # through the Python API with host-side staging: the controls the ordered C-ABI legs must reproduce, and the staged slots of
        # every step for the cpu_baseline leg (the oracle is timed on the SAME ordered workload)
        ctx.trace_o, _, _ = record_trace(ctx.car_t, ctx.path, ctx.obstacles, kw, W + K, stage_every_step=True, moving=args.moving)
        if not args.moving:
            ctx.u_ord = np.array([u.ravel() for u in ctx.trace_o["u"]])
    if shard and ctx.oversub:
        legs.oversubscribed_shard_run(ctx, mpc_rec)
        dist.destroy_process_group()
        return

    moving = bool(args.moving)
    one = rank == 0 and world == 1
    head = fixed = follow = early = hard_off = pydrv = pcie = None
    if not shard:
        # HEADLINE = the reference's default semantics: obstacle_order=True, the scene re-sorted about the robot on every tick
        head = closed_loop.run(ctx, per_tick_scene=moving, ordered=True, outputs=bool(args.dump_outputs))
        if rank == 0 and args.dump_outputs:
            dump_outputs(args.dump_outputs, head.outputs)
        if one:
            # the protocol of rounds 2-3: slots bound once (obstacle_order=False), no conversion kernel inside the timed region
            lp = closed_loop.run(ctx, per_tick_scene=moving)
            fixed = stats(K, lp.elapsed, lp.times, lp.iters, max_du_vs_python_closed_loop=lp.du if not moving else None, second_window=lp.second_window,
                          residuals=closed_loop.residual_summary(lp.info, 0.2),
                          what="obstacle_order=False: slots bound once at staging, rda_step_tracked per step (the headline protocol of rounds 2-3; the reference's default re-sorts every tick)")
        from rda_planner_amd.rda_solver import hip_options as _ho
        if one:
            # opt-OUT leg: the headline loop without rda_opts::su_hard_warm (default since round 5) - the start rule of round 4
            try:
                lp = closed_loop.run(ctx, per_tick_scene=moving, ordered=True, compare=False, hip_opts=_ho(su_hard_warm=(0.0, 0.0)))
                hard_off = stats(K, lp.elapsed, lp.times, lp.iters, residuals=closed_loop.residual_summary(lp.info, 0.2),
                                 what="the headline protocol with su_hard_warm = (0, 0): the warm attempts of the unconverged steps start like in round 4 - "
                                      "same su-problems, same tolerance, more interior-point iterations")
            except (AssertionError, RuntimeError) as e:          # the headline must not depend on an opt-out leg
                hard_off = {"error": str(e)[:200]}
        if one and args.duals_follow_leg:
            # NOT the reference's semantics (opt-in, rda_opts::duals_follow): the duals move WITH their obstacles through the re-binding (quirk Q5)
            try:
                lp = closed_loop.run(ctx, per_tick_scene=moving, ordered=True, compare=False, duals_follow_obstacles=True)
                follow = stats(K, lp.elapsed, lp.times, lp.iters, second_window=lp.second_window,
                               what="the headline protocol with duals_follow_obstacles=True: an extension, NOT reference semantics - never `value`")
            except (AssertionError, RuntimeError) as e:
                follow = {"error": str(e)[:200]}
        if one and not args.size_leg:
            # opt-in rda_opts::su_tol_early: the su-problems before the last ADMM iteration of a step at the reference solver's own class of
            # tolerance (ECOS defaults, 1e-8) instead of the 1000 x tighter su_tol the parity tolerance is stated against
            try:
                lp = closed_loop.run(ctx, per_tick_scene=moving, ordered=True, compare=False, hip_opts=_ho(su_tol_early=(1e-6, 1e-7, 1e-8)))
                early = stats(K, lp.elapsed, lp.times, lp.iters, residuals=closed_loop.residual_summary(lp.info, 0.2),
                              what="the headline protocol with su_tol_early = (1e-6, 1e-7, 1e-8): opt-in, the stated parity tolerance does not hold with it - never `value`")
            except (AssertionError, RuntimeError) as e:
                early = {"error": str(e)[:200]}
            lp = closed_loop.run(ctx, per_tick_scene=moving, driver="python", ordered=True)
            pydrv = stats(K, lp.elapsed, lp.times, lp.iters, max_du_vs_python_closed_loop=lp.du if not moving else None,
                          what="the headline loop with the caller written in Python (ctypes calls + numpy kinematics between two steps)")
        if one and not moving:
            lp = closed_loop.run(ctx, per_tick_scene=True, ordered=True)
            pcie = stats(K, lp.elapsed, lp.times, lp.iters, max_du_vs_python_closed_loop=lp.du,
                         what="raw scene (vertices, velocities) handed over from host memory AND re-sorted every tick: rda_tracked_begin + rda_upload_scene_async(order=1) + rda_tracked_finish")

    # per-launch GPU times of the HEADLINE loop (ordered): one more pass of the same closed loop with hipEvents around every launch
    head_t = None
    if head is not None and one:
        head_t = closed_loop.run(ctx, per_tick_scene=moving, ordered=True, timing=True, compare=False)

    # ---- the other sizes the metric names (sub-processes), BEFORE this process runs its fleet legs: a sub-process started after the 64-ego fleet legs
    #      prints 8 - 15 % less on every size (n20 4.08 k against 4.68 k, C4 684 against 769, the C5 fleet 31.8 k against 34.7 k ego-steps/s; the multi-ego
    #      and interior-point legs have no such effect, a garbage collection changes nothing, an idle process holding handles neither:
    #      tools/experiments/sizes_parent_probe.sh, idle_context_probe.sh, round 6) - seconds of all 256 CUs busy leave the device in a slower state for a
    #      while.  Every size leg is a measurement of its own configuration: it runs on the device as the headline found it.
    sizes_res = None
    if one and not shard and not args.no_sizes and (N, T, moving) == (200, 20, False):
        sizes_res = legs.sizes(args.sizes_budget_s, os.path.abspath(__file__))

    # ---- interior-point LamMuZ mode (row-parallel kernel k_lammuz_ip): the robust setting lmz_central = 1e-3 on the headline scene, and a
    #      CIRCLE robot (norm2 robot cone, rda_solver.py:1034-1039: always this mode) - in the headline protocol (re-sorted every tick:
    #      VERDICT r04 #5) and with a fixed binding.  The reference solves EVERY LamMuZ problem with an interior point (rda_solver.py:768,800).
    ip_legs = None
    if one and not moving and not args.no_ip_legs:
        ip_legs = {}
        try:
            from rda_planner_amd import scenarios as sc_
            circ = sc_.circle_robot(radius=0.8, dynamics="diff")
            for name, kws in (("rectangle_robot_lmz_central_1e-3", dict(lmz_central=1e-3)), ("circle_robot_norm2_cone", dict(car=circ))):
                ent = {}
                for proto, ordered in (("resorted_every_tick", True), ("fixed_slot_binding", False)):
                    lp = closed_loop.run(ctx, per_tick_scene=False, compare=False, ordered=ordered, **kws)
                    ent[proto] = stats(K, lp.elapsed, lp.times, lp.iters, residuals=closed_loop.residual_summary(lp.info, 0.2), second_window=lp.second_window)
                ip_legs[name] = ent
        except (AssertionError, RuntimeError) as e:          # (a robot that reaches the goal inside the timed region, ...)
            ip_legs["error"] = str(e)

    rp = legs.replay_legs(ctx)
    mean_iters = float(np.mean(rp["iters"]))
    multi = legs.multi_ego(ctx) if one and args.egos > 1 else None
    fleet = legs.fleet(ctx) if one and args.fleet_egos > 1 and getattr(ctx.api, "has_fleet", False) else None

    want_shard_leg = (world > 1 and not shard and not ctx.oversub and not args.no_shard_leg) or (world == 1 and args.force_shard_leg)
    if rank != 0:
        if want_shard_leg:
            wd = threading.Timer(args.shard_leg_timeout, lambda: os._exit(0))
            wd.daemon = True; wd.start()
            try:
                legs.shard_leg(ctx)
            except Exception:
                pass
            wd.cancel()
        if dist is not None:
            dist.destroy_process_group()
        return

    # the rooflines of the line: the launches of the HEADLINE loop (re-sorted every tick) when there is one, else of the replay
    n_exec_replay = int(np.sum(rp["iters"]))
    rd, rs = rooflines(ctx, rp["kt"], rp["lmz_kernel"], n_exec_replay)
    replay_roofs = {"k_su": rd if rd["kernel"].startswith("k_su") else rs, "k_lammuz": rs if rd["kernel"].startswith("k_su") else rd,
                    "what": "device-resident replay of the recorded closed loop with obstacle_order=False (slots bound once)"}
    if head_t is not None:
        dominant, secondary = rooflines(ctx, head_t.kernel_ms, head_t.lmz_kernel, int(np.sum(head_t.iters)))
    else:
        dominant, secondary = rd, rs

    replay = {"steps_per_s": round(K * (1 if shard else world) / rp["elapsed"], 3), "ms_per_step": round(rp["elapsed"] / K * 1e3, 5),
              "instrumented_ms_per_step": round(rp["elapsed_instrumented"] / K * 1e3, 5), "max_du_vs_python_closed_loop": rp["replay_err"],
              "what": "recorded step inputs replayed back-to-back on the device, no per-step host synchronisation",
              "synchronised_per_step": rp["sync_replay"]}
    if head is not None:
        value, ms_step, protocol = K * world / head.elapsed, head.elapsed / K * 1e3, (PROTOCOL_MOVING if moving else PROTOCOL_STATIC)
    else:                   # obstacle shards: the RCCL path is driven by the replay (every rank enqueues the same steps)
        value, ms_step, protocol = replay["steps_per_s"], replay["ms_per_step"], replay["what"]
    out = base_line(ctx, value, ms_step, protocol)
    out.update({
        "median_ms_per_step": round(float(np.median(head.times) * 1e3), 5) if head else None,
        "max_du_vs_python_closed_loop": head.du if head and not moving else None,
        "mean_admm_iters": round(float(np.mean(head.iters)) if head else mean_iters, 3),
        "residuals": closed_loop.residual_summary(head.info, 0.2) if head else None,
        "second_window": head.second_window if head else None,
        "fixed_slot_binding": fixed,
        "su_hard_warm_off": hard_off,
        "su_tol_early": early,
        "duals_follow_obstacles": follow,
        "pcie_inclusive": pcie,
        "python_caller_closed_loop": pydrv,
        "device_resident_replay": replay,
        "python_api_closed_loop": {"host_obstacle_staging_steps_per_s": round(1.0 / ctx.trace["closed_loop_s_per_step"], 2),
                                   "device_obstacles": cl_dev, "device_obstacles_and_tracking": cl_trk},
        "multi_ego_one_gpu": multi,
        "multi_ego_fleet": fleet,
        "lammuz_interior_point_closed_loops": ip_legs,
        "roofline": dominant, "roofline_secondary": secondary,
        "roofline_fixed_slot_binding_replay": {k: ({kk: v[kk] for kk in ("kernel", "avg_launch_us", "launches", "skipped_launches", "frac", "achieved")} if isinstance(v, dict) else v)
                                               for k, v in replay_roofs.items()},
        "parity": {"stated_tolerance_applied_control": 1e-6, "asserted_on_the_baseline_sizes": 1e-7,
                   "where": "tests/helpers.py TOL_U / TOL_U_FIXED (round 6: the su solve is landed on its vertex on both sides; soaks against the cold oracle at the last "
                            "commit: 213 k steps, largest difference 3.3e-7 - and FOUR steps (of 64 k in the exotic flavour; NONE - max 4.6e-7 - with the tighter fallback stop of the last commit) at 4.8e-6 .. 1.2e-4 in the steering angle of an Ackermann robot "
                            "at |v| <= 0.13 m/s, <= 3.9e-7 in its yaw rate: a refused landing, whose fallback is the interior point, in a nearly singular direction); asserted by tests/test_gpu_soak.py (random scenes) and "
                            "tests/test_gpu_baseline_sizes.py; DESIGN.md 2"},
    })
    if head is not None and head.elapsed_per_rank:
        out["per_rank_steps_per_s"] = [round(K / e, 3) for e in head.elapsed_per_rank]
    if not args.no_cpu_baseline and world == 1:
        out["cpu_baseline"] = cpu_baseline.run(ctx)
    if sizes_res is not None:
        out["sizes"], out["sizes_wall_s"] = sizes_res
    if want_shard_leg:
        def give_up():
            out["obstacle_shard_leg"] = {"error": f"no result within {args.shard_leg_timeout:.0f} s (collective did not complete)"}
            compact.emit(out)
            os._exit(0)
        wd = threading.Timer(args.shard_leg_timeout, give_up)
        wd.daemon = True; wd.start()
        try:
            out["obstacle_shard_leg"] = legs.shard_leg(ctx)
        except Exception as e:                               # the headline line must not depend on this leg
            out["obstacle_shard_leg"] = {"error": repr(e)}
        wd.cancel()
    compact.emit(out, None if args.size_leg else "bench_detail.json", detail_to_stdout=args.size_leg)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
