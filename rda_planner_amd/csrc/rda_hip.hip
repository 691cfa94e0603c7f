// librda_hip.so - MI355X (gfx950) implementation of the C-ABI in include/rda_hip.h.
//
// Per ADMM iteration two launches on the handle's stream, no host synchronisation in between:
//   k_su      <<<1, 256>>>      su-problem (interior point + Riccati), relinearisation point update,
//                               residual reduction / early-stop flag of the previous iteration
//   k_lammuz_rows <<<N*T/16, 256>>>  one (obstacle, stage) LamMuZ sub-problem per 16-lane row of a wavefront (k_lammuz
//                               <<<N*T/4, 256>>>: one per wavefront, for E+R+1 > 16), fused with
//                               the lam'A / lam'b products, the xi / zeta updates and the residual
//                               partials (reference rda_solver.py:529-542, 639-690, 781-793)
// Dense grids (more than 256 workgroups per ego, fleets) run the LamMuZ step as two launches: k_lammuz_rows_fast (the common path
// only, three waves per SIMD) and k_lammuz_enum (the rows whose warm candidate failed its certificate).
// In front of them, optional: scene::k_* (the caller's obstacle conversion / ordering) and the caller's pre_process, which
// shares a launch with the first su-problem of the tick (k_su_tracked: two workgroups); rda_fleet_* launches the same bodies
// once for B egos.  The launch that ends a step (the su launch that detects the early stop, else k_finish) writes the result
// slot into pinned host memory and publishes a sequence word the host polls.
// All solver state (duals, products, nominal trajectory, staged obstacles) stays resident in HBM
// between iterations and between MPC steps, exactly like the reference keeps it in CVXPY Parameter
// values (quirks Q4-Q6 come for free).
#include <hip/hip_runtime.h>
#include <cfloat>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <chrono>
#include <memory>
#include <dlfcn.h>
#include "../../include/rda_hip.h"
#include "host_buf.h"
#include "lmz_plan.h"
#include "lammuz_device.h"
#include "lammuz_cp_device.h"
#include "lammuz_ip_device.h"
#include "su_device.h"
#include "scene_device.h"
#include "lidar_device.h"
#include "track_device.h"
#include "rollout_device.h"

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, "librda_hip: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); return RDA_ERR_HIP; } } while (0)

struct Ctrl {
    int stop, iters, su_status, ipm_iters, st_tmp, it_tmp;
    int su_last;             // interior-point iterations of the last su-solve of this handle (99 = none / it did not converge): picks the next start
                             // (a history per ADMM iteration index was measured: no gain on dynamic_obs, and it leaves the oracle's mirrored path)
    int lmz_fail;            // sub-problems of this step that kept their previous duals (non-finite input or result), rda_solver.py:791-793
    double resi_dual, resi_pri;
    int finished;                 // the result slot of this step has been written (by the launch that ended the step)
    int su_probe;                 // consecutive su-solves in the hard regime (see su_body)
    int hint_par;                 // which of the two Dev::hint buffers the LamMuZ launch of this iteration WRITES (flipped by every executed su launch)
    int wl_count;                 // entries of Dev::wl written by the common-path LamMuZ kernel of this iteration (reset by k_su)
    int wlc_count;                // ... and its CIRCLE rows, which fill Dev::wl from the back (round 6: the work-list kernel serves them four per wave, remembered case first)
    int resi_iter;                // ADMM iterations of this step whose residuals are in resi_dual / resi_pri (k_su / k_finish)
    int pose_ok;                  // Dev::pose and the near masks of Dev::coef describe the same terms (a LamMuZ launch / k_lmz_finalize made them)
    int prev_unconv;              // the previous step ended with a residual above iter_threshold (all iter_num iterations, no early stop): picks the warm start (su_hard_warm)
    int su_hardlike;              // the last su-solve started far from its solution (relative dual residual of its first iterate > su::HARD_RD0): the other key of su_hard_warm
    double rd0_tmp;               // ... that residual, written by the solve
    int land_easy;                // consecutive su-solves of this handle that needed no interior-point iteration and ONE landing round: the next warm su-problem of the same step starts with a blind landing (su_body): solver history
    double land_rho_prev;         // penalty scale of the last landing (what a blind landing uses)
    int blind_ok;                 // blind landings are tried while this is >= 0: +1 per accepted one (capped at 4), -6 after a refused one, +1 per opportunity skipped (N = 2000: 7 of 37 accepted, north star 54 of 62): solver history
    int land_hard;                // > 0: one of the last four su-solves' landings took three or more rounds (many rows / hinge terms still undecided at the 1e-3-class stop: moving obstacles): the next solve's interior point runs to 1e-2 x su_land_tol before it is landed (C4: 2.7 -> rounds per solve, +4 % steps/s; north star: 1.1 - 1.3 rounds, unaffected): solver history
    int spec_credit;              // su_land_first = 2: speculative landings are tried while this is >= 0 (+3 per accepted one, capped at 6; -2 per refused one; +1 per eligible solve that had to skip): solver history
    int land_stat[su::LAND_STATS];  // su_land: landings accepted, refused, rounds, passes spent on landings, speculative landings (rda_debug_su_land, rda_debug_su_land_n)
    unsigned long long ref_seq;   // tick number whose reference is complete (k_su_tracked: written by the sampling workgroup)
#ifdef RDA_LMZ_STATS
    unsigned lmz_stat[8];    // debug build only: [0] executed launches, [1] rows that needed the enumeration, [2+k] waves with k such rows
#endif
};

constexpr int NCOEF = 9;      // per-(slot, stage) term arrays: NGATH of them travel with the shard chunk (Dev::coef), the rest stay local (Dev::coefL)
constexpr int NGATH = 3;      // ax, ay, cb: what the su hinge reads per term
constexpr int NBS = su::NBS;  // doubles per (stage, GS-slot block) partial; one more 8-byte word per block carries the near mask
constexpr int GS = su::GS;    // slots per block partial = rows of a packed LamMuZ workgroup (2 waves x 4 rows of 16 lanes)
static_assert(GS == lmzplan::GS, "lmz_plan.h sizes its grids for another block partial");
struct Dev;
__host__ __device__ inline double *coef_arr(const Dev &d, int r, int k);

struct Dev {
    rda_cfg c;
    int nt;                  // time slots of the staged obstacles (T+1 or 1)
    int warm;                // k_lammuz tries the previous support first (RDA_LMZ_WARM=0 disables)
    int rows;                // four sub-problems per wave (k_lammuz_rows) when E+R+1 <= 16 (RDA_LMZ_ROWS=0 disables)
    unsigned char muc[40]; int nmv;   // robot support candidates that survive the vertex test (host, rda_create)
    double rv[28][2]; int nrv;        // robot vertices of the surviving pairs (list order)
    double *su_lam_keep;               // inequality multipliers of the last converged su-solve [10*T] (interior-point warm start)
    int su_warm_first;                 // the first su-problem of a step starts from the previous step's multipliers, shifted by one stage
    int su_warm_cap;                   // iterations granted to the warm start before the cold one takes over
    double su_tol[3];                  // interior-point stop of the su-problem (rda_opts::su_tol)
    double su_tol_early[3];            // ... of the ADMM iterations before the last one of a step (rda_opts::su_tol_early; 0 = su_tol)
    int su_light;                        // su_device Cfg::light_check
    int su_split;                        // su_device Args::split (time split of the Newton system)
    int su_accept;                       // su_device Args::accept (safety net: the best near-converged iterate)
    int su_first_attempt;                // su_device Args::first_attempt (test switch)
    int su_land; double su_land_tol[3], su_land_rho;  // su_device Args::land (rda_opts::su_land)
    int su_land_first;                   // su_device Args::land_first (rda_opts::su_land_first)
    int su_land_blind_from;              // blind landings after this many easy solves in a row (0: never)
    int *wl; int wl_cap;                 // [wl_cap >= N*T] work list: sub-problems whose warm candidate failed its certificate (split LamMuZ launch): polygon rows from the front, circle rows from the back
    int *sc_bad;                         // non-convex counter of the staged raw scene (null: obstacles were staged as (A, b) slots)
    int su_easy_nopred;
    int su_pre;                        // the su set-up reads the block sums / near masks of the LamMuZ launch (0: it evaluates every term itself)
    int su_cold_probe;
    int su_cold_from;                  // a solve that follows one with more interior-point iterations than this starts cold (0 = never)
    double su_easy[5]; int su_easy_max;  // wfl, mu0, clip, tau, sigma of the start used while the su-solves are EASY (the last one took <= su_easy_max
                                       // interior-point iterations; max = 0 disables)
    double su_warm_clip;               // start of a warm attempt: relative margin inside the boxes (cold 0.01)
    double su_warm_tau, su_warm_sig;   // end game of the warm attempt (floors; cold solves: 0.995, 1e-3)
    double su_warm_wfl, su_warm_mu0;   // interior-point start of the su-problems of ADMM iterations >= 1 ("0,0" = cold)
    double su_hard_wfl, su_hard_mu0;   // ... of the steps that follow an UNCONVERGED step (rda_opts::su_hard_warm; mu0 = 0: the rule is off)
    int lmz_mode;            // 0: support enumeration + tie-breaks T1-T3 (default), 1: interior point, central path at lmz_mu (norm2 robots: always)
    int ip_rows;             // mode 1 and the row-parallel kernel takes this shape (and rda_opts::lmz_ip_rows): with staged obstacles the launch form is k_lammuz_ip, else the
                             // per-thread kernel + k_lmz_finalize (lmzplan::member_ip_rows: the host's plans and the fleet kernels decide per member from this record)
    double lmz_mu;           // barrier parameter of the returned central-path point (mode 1)
    int centre;              // tie-break T1: central separating normal in the slack regime
    int obstacle_num;        // 0 or N
    double *G, *h;
    double *A, *b; int *cone;                 // [N][nt][E][2], [N][nt][E], [N]
    // per (slot, time slot) candidate list and vertices of the staged obstacle (pose independent): k_prepare, at upload
    unsigned char *oc_lamc; double *oc_vtx; int *oc_cnt;      // [N*nt][oc_ls], [N*nt][oc_vs], [N*nt][2] = (npv, nlv)
    int oc_ls, oc_vs;        // strides of the two tables: 1 + E + E (E-1)/2 candidates (rounded up to 4), E (E-1) vertex coordinates - NOT the 40 / 56 of E = 8 (round 6: with moving
                             // obstacles the tables are per (slot, STAGE): 496 B a row against 96 B of half-spaces; E = 4: 128 B)
    // Remembered supports (candidate index of the last max-clearance optimum, -1 = none) - a pure cache: whatever it holds is only the
    // first candidate of a row, which is accepted on its certificate alone.  Two buffers of hint_len ints, [T][hint_stride] each: a
    // LamMuZ launch reads the one the previous executed launch wrote and writes the other (Ctrl::hint_par, flipped by the su launch of
    // the iteration), so that the FIRST launch of a tick can read stage t+1 of the previous tick - the horizon has moved on by one
    // stage, that support belongs to this pose - without racing against the row that rewrites it.  Key of a row: the SOURCE obstacle
    // of its slot when the scene was staged by the device pipeline (slot_src = its rank table: a re-sorted scene re-binds most slots
    // every tick, the supports stay with their obstacles), else the slot itself (host-staged slots, padding copies).
    int *hint; int hint_len, hint_stride, src_cap;
    const int *slot_src; int src_used;        // slot -> index in the caller's raw scene, valid for slots < src_used (null: host-staged)
    // Dual state, STAGE-MAJOR: lam [T+1][N][E], mu [T+1][N][R], xi [T+1][N][2], z / zeta [T][N] - a LamMuZ workgroup owns GS consecutive
    // slots of one stage, so what it reads and writes are whole lines (the accessors rda_get_state / rda_set_state speak the
    // reference's [N][T+1][.] shapes)
    double *lam, *mu, *z, *xi, *zeta, *dis;
    // Condensed su terms + residual partials per obstacle shard (P = 1 on a single GPU), arrays [T][Nloc] indexed t*Nloc + nl:
    //   k = 0 ax, 1 ay (a = A'lam), 8 cb = lam'b + mu'h + z - zeta (the offset of the su hinge)      -> the shard CHUNK, coef[r*chunk + ..]
    //   k = 2 lam'b, 3 mu'h + z - zeta, 4 / 5 G'mu + xi, 6 dual residual, 7 |Hm|^2                    -> local only, coefL[r*lchunk + ..]
    //   bsum : coef[r*chunk + NGATH*T*Nloc + ((t*J + j)*NBS + q)]   sums over the slots GS j .. GS j + GS-1 of stage t (su::row_term; [6], [7])
    //   bmask: the 8-byte words behind bsum, [t*J + j]: bit r = slot GS j + r is NEAR (su hinge screening) at the pose table's position
    // chunk r (what the su-problem reads: three arrays + the reduced sums and masks) is produced by rank r's LamMuZ launch and replicated
    // by one all-gather per ADMM iteration; the local arrays serve the state accessors, failed rows and k_lmz_finalize of the own rank.
    double *coef, *coefL; int P, rank, Nloc, J; size_t chunk, lchunk;
    int Nlive;                                // obstacle slots of THIS rank's shard that exist (< Nloc on the last ranks when N % P != 0)
    double *s, *u;                            // nominal (para_s, para_u)
    double *pose;                             // [T][4] px, py (column t+1), cos, sin (heading of column t) of Dev::s: written by every su launch,
                                              // read by the LamMuZ rows (no trigonometry per row) and by the next su set-up
    double *ref, *ref_speed;                  // current step reference (device)
    Ctrl *ctrl;
    long long *su_prof;                       // optional phase cycle counters of the su-solves of this handle (RDA_SU_PROF), else null
    // interior-point LamMuZ mode, row-parallel kernel: the central-path point (x | s diag | z diag | s general | z general, 5 x 16 doubles)
    // every (stage, slot) ended on and whether it is valid - the start of that sub-problem's next solve (solver history, like su_lam_keep)
    double *ipw; int *ipf;                    // [T][N][5][16], [T][N]; null: always the cold start
};

__host__ __device__ inline double *coef_arr(const Dev &d, int r, int k)
{
    const size_t tn = (size_t)d.c.T * d.Nloc;
    if (k < 2) return d.coef + (size_t)r * d.chunk + (size_t)k * tn;
    if (k == 8) return d.coef + (size_t)r * d.chunk + 2 * tn;
    return d.coefL + (size_t)r * d.lchunk + (size_t)(k - 2) * tn;
}
__host__ __device__ inline double *bsum_arr(const Dev &d, int r) { return d.coef + (size_t)r * d.chunk + (size_t)NGATH * d.c.T * d.Nloc; }
__host__ __device__ inline unsigned long long *bmask_arr(const Dev &d, int r) { return (unsigned long long *)(bsum_arr(d, r) + (size_t)NBS * d.c.T * d.J); }
__host__ __device__ inline size_t chunk_doubles(int T, int Nloc) { const size_t J = (Nloc + GS - 1) / GS; return (size_t)NGATH * T * Nloc + (size_t)(NBS + 1) * T * J; }
__host__ __device__ inline size_t lchunk_doubles(int T, int Nloc) { return (size_t)(NCOEF - NGATH) * T * Nloc; }
// row index of (slot n, dual column tt) / (slot n, stage t) in the stage-major dual arrays
__host__ __device__ inline size_t drow(const Dev &d, int n, int tt) { return (size_t)tt * d.c.N + n; }

// ------------------------------------------------------------------------------------------------
// resi_dual (mean over the slots of the squared dual change, rda_solver.py:735-737) and resi_pri (|stack(Hm)|, :688) from the block
// partials of every shard.  ONE wave (the first 64 threads of the calling workgroup), lane l sums the partials l, l+64, ... in that
// order, then a wave reduction: the values do not depend on the kernel (or workgroup size) that takes the verdict, and they are
// identical on every rank.  All threads of the workgroup call.
struct ResPre { double a[16], b[16]; };       // first batch of shard 0's residual partials, requested ahead (su_body: with everything else the launch reads)
__device__ __forceinline__ void residual_prefetch(const Dev &d, int tid, ResPre &p)
{
    const double *bs = bsum_arr(d, 0);
    const int nb = d.J * d.c.T;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int i = tid + 64 * k; const int ii = (tid < 64 && i < nb) ? i : 0; p.a[k] = bs[(size_t)ii * NBS + 3]; p.b[k] = bs[(size_t)ii * NBS + 4]; }      // (unconditional loads: see reduce_residuals)
}
// `iters`: the value of Ctrl::iters (the caller has it).  `bc` (LDS, 2 doubles, optional): the verdict reaches the other threads through it - (rd, rp) are
// returned to every thread - instead of a store to the control block and a trip back.
// (pre by reference + a flag, never a selected pointer: its members stay registers)
__device__ __forceinline__ void reduce_residuals(const Dev &d, int tid, int iters, const ResPre &pre, const bool have_pre, double *bc, double &out_rd, double &out_rp)
{
    const int T = d.c.T, N = d.c.N;
    if (tid < 64) {
        double rd = 0, rp = 0;
        if (d.obstacle_num != 0)
            for (int r = 0; r < d.P; ++r) {
                const double *bs = bsum_arr(d, r);
                const int nb = d.J * T;
                for (int base = 0; base < nb; base += 64 * 16) {        // sixteen independent loads in flight per lane and quantity,
                    double a[16], b[16];                                 // accumulated in the order of the plain loop
                    if (have_pre && r == 0 && base == 0) {
#pragma unroll
                        for (int k = 0; k < 16; ++k) { a[k] = pre.a[k]; b[k] = pre.b[k]; }
                    } else {
                        // (entries beyond nb are read from entry 0 and not added below.  `in ? load : 0` became sixteen conditional loads with a wait each - found in the ISA, round 6)
#pragma unroll
                        for (int k = 0; k < 16; ++k) { const int i = base + tid + 64 * k; const int ii = i < nb ? i : 0; a[k] = bs[(size_t)ii * NBS + 3]; b[k] = bs[(size_t)ii * NBS + 4]; }
                    }
#pragma unroll
                    for (int k = 0; k < 16; ++k) if (base + tid + 64 * k < nb) { rd += a[k]; rp += b[k]; }
                }
            }
        rd = su::wave_allreduce(rd, false);
        rp = su::wave_allreduce(rp, false);
        if (tid == 0) {
            d.ctrl->resi_dual = rd / N; d.ctrl->resi_pri = sqrt(rp); d.ctrl->resi_iter = iters;
            if (bc) { bc[0] = rd / N; bc[1] = sqrt(rp); }
        }
    }
    __syncthreads();
    if (bc) { out_rd = bc[0]; out_rp = bc[1]; }
}

extern __shared__ __attribute__((aligned(16))) double smem_su[];

// The kernel arguments of the one-workgroup launches (Dev by value: 1.3 KB = 21 lines of the scalar cache) are read by s_load where the code needs them - a
// dependent chain of scalar-cache misses through the launch's prologue (~25 s_load / s_waitcnt pairs in k_su<20>, round 6).  One load per line up front, all
// in flight together: the later ones hit.
template <int BYTES> __device__ __forceinline__ void warm_kernargs()
{
    const int __attribute__((address_space(4))) *kp = (const int __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    int acc = 0;
#pragma unroll
    for (int o = 0; o < BYTES; o += 64) acc |= kp[o / 4];
    asm volatile("" :: "s"(acc));
}

// Where a step's result goes: the device slot [u | s | info | track out] (one contiguous block starting at out_u), and optionally
// `mirror` (pinned host memory): the same block written straight into the caller-visible host buffer and published with a
// sequence number (system-scope release) - the host polls that word instead of queueing a device-to-host copy and waiting for
// the stream (fetch_result).
struct Fin { double *out_u = nullptr, *out_s = nullptr; rda_info *info = nullptr; double *mirror = nullptr; unsigned long long seq = 0; int slot = 0;   // slot: out_u is the handle's contiguous result slot (Fin{}: no result hand-over)
             // obstacle shards: the su launch that takes the early-stop verdict itself publishes it (2 vseq + stop) in pinned host memory
             // BEFORE it starts its solve - the host polls that word and queues the next LamMuZ launch + all-gather (or stops queueing)
             // while the su-problem is still being solved: no stream synchronisation inside a step
             unsigned long long *verdict = nullptr; unsigned long long vseq = 0; };

// all threads of the calling workgroup (any size); the residuals in d.ctrl are final
__device__ __forceinline__ void publish_result(const Dev &d, const Fin &f)
{
    const int tid = threadIdx.x, nth = blockDim.x, T = d.c.T;
    for (int i = tid; i < 2 * T; i += nth) f.out_u[i] = d.u[i];
    for (int i = tid; i < 3 * (T + 1); i += nth) f.out_s[i] = d.s[i];
    if (tid == 0) {
        f.info->resi_dual = d.ctrl->resi_dual; f.info->resi_pri = d.ctrl->resi_pri;
        f.info->iters = d.ctrl->iters; f.info->su_status = d.ctrl->su_status; f.info->su_ipm_iters = d.ctrl->ipm_iters;
        f.info->lmz_fail = d.ctrl->lmz_fail;
        d.ctrl->prev_unconv = !(d.ctrl->resi_dual < d.c.iter_threshold && d.ctrl->resi_pri < d.c.iter_threshold);
    }
    // polygons of the staged scene that failed the reference's convexity test (mpc.py:476-549 prints a warning per polygon)
    if (f.slot && tid == 1) *(long long *)(f.out_u + 2 * T + 3 * (T + 1) + 6) = d.sc_bad ? (long long)*d.sc_bad : 0ll;
    if (!f.mirror) return;
    __syncthreads();
    const int n = 2 * T + 3 * (T + 1) + 7;                   // out_u, out_s, info (4 doubles), the track::Out (2), the non-convex count
    for (int i = tid; i < n; i += nth) f.mirror[i] = f.out_u[i];
    __threadfence_system();
    __syncthreads();
    if (tid == 0) __hip_atomic_store((unsigned long long *)(f.mirror + n), f.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int TT, typename RefWait = su::NoRefWait>
__device__ __forceinline__ void su_body(const Dev &d, int it, const double *in_s, const double *in_u,
                                        const double *ref, const double *ref_speed,
                                        const unsigned long long *ref_flag = nullptr, unsigned long long ref_seq = 0,
                                        const Fin *fin = nullptr, RefWait ref_wait = RefWait())
{
#ifdef SU_TRACE
    const long long t_entry_ = clock64();
#endif
    const int tid = threadIdx.x;
    // ---- (round 6) ONE trip to memory for everything this launch reads before its first Newton step.  The prologue used to be a chain of dependent
    //      trips (~1.5 us each: what the previous launch wrote sits in HBM / another XCD's L2): control block (stop?) -> residual partials -> their verdict
    //      back through the control block -> solver history for the start rule -> the solve's own inputs.  Now: the part of su::Args that follows from the
    //      kernel arguments alone is filled first, the solve's inputs (su::prefetch), a copy of the control block and the first batch of the residual
    //      partials are requested together, and the bookkeeping below works on the copy (thread 0 stores what changes; nothing is read back).
    su::Args a;
    a.c.T = d.c.T; a.c.N = d.c.N; a.c.dynamics = d.c.dynamics; a.c.accelerated = d.c.accelerated;
    a.c.dt = d.c.dt; a.c.L = d.c.L; a.c.umax0 = d.c.max_speed[0]; a.c.umax1 = d.c.max_speed[1];
    a.c.ab0 = d.c.acce_bound[0]; a.c.ab1 = d.c.acce_bound[1]; a.c.ws = d.c.ws; a.c.wu = d.c.wu;
    a.c.slack_gain = d.c.slack_gain; a.c.max_sd = d.c.max_sd; a.c.min_sd = d.c.min_sd; a.c.ro1 = d.c.ro1; a.c.ro2 = d.c.ro2;
    a.c.eps_u = d.c.eps_u; a.c.tol_rd = d.su_tol[0]; a.c.tol_rp = d.su_tol[1]; a.c.tol_mu = d.su_tol[2]; a.c.light_check = d.su_light;
    if (it < d.c.iter_num - 1 && d.su_tol_early[0] > 0) { a.c.tol_rd = d.su_tol_early[0]; a.c.tol_rp = d.su_tol_early[1]; a.c.tol_mu = d.su_tol_early[2]; }
    a.in_s = it == 0 ? in_s : d.s; a.in_u = it == 0 ? in_u : d.u;
    a.ref = ref; a.ref_speed = ref_speed; a.ref_flag = ref_flag; a.ref_seq = ref_seq;
    a.ax = coef_arr(d, 0, 0); a.ay = coef_arr(d, 0, 1); a.cb = coef_arr(d, 0, 8); a.gx = coef_arr(d, 0, 4); a.gy = coef_arr(d, 0, 5);
    a.P = d.P; a.Nloc = d.Nloc; a.chunk = d.chunk;
    // the reduced form of the terms (block sums, near masks at the pose table's positions): no pass over the N terms in the set-up
    if (d.su_pre) { a.bsum = bsum_arr(d, 0); a.bmask = bmask_arr(d, 0); a.J = d.J; a.pose = d.pose; }
    // iterations >= 1 are linearised about the previous solution, whose pose table the previous su launch wrote
    if (it > 0) { a.pose = d.pose; a.pose_lin = 1; }
    a.pose_out = d.pose;
    a.d_in = d.dis; a.out_s = d.s; a.out_u = d.u; a.out_d = d.dis;
    a.lam_keep = d.su_lam_keep;
    if (it == 0 && d.su_warm_mu0 > 0 && d.su_warm_first) a.warm_shift = 1;
    su::Pre pre;
    su::prefetch<TT>(a, pre);
    Ctrl cl = *d.ctrl;
    ResPre rpre;
    const bool res_pre = it > 0 && d.obstacle_num != 0;
    if (res_pre) residual_prefetch(d, tid, rpre);
#ifdef SU_TRACE
    long long t_mark_[4] = {0, 0, 0, 0};
    t_mark_[0] = clock64();                  // every load of the prologue has been requested
#endif
    if (it == 0) {                      // first su-problem of a step: the step's bookkeeping starts here (no separate launch)
        if (tid == 0) {
            d.ctrl->stop = 0; d.ctrl->iters = 0; d.ctrl->su_status = 0; d.ctrl->ipm_iters = 0; d.ctrl->lmz_fail = 0;
            d.ctrl->resi_dual = 0; d.ctrl->resi_pri = 0; d.ctrl->finished = 0; d.ctrl->resi_iter = 0;
        }
        cl.stop = 0; cl.iters = 0; cl.su_status = 0; cl.ipm_iters = 0; cl.lmz_fail = 0; cl.resi_dual = 0; cl.resi_pri = 0; cl.finished = 0; cl.resi_iter = 0;
    } else if (cl.stop) {
        if (fin && fin->verdict && tid == 0) __hip_atomic_store(fin->verdict, 2 * fin->vseq + 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
#ifdef SU_TRACE
    t_mark_[1] = clock64();                  // the copy of the control block has arrived (stop flag tested)
#endif
    // The early stop of rda_solver.py:594 after iteration it-1: the residual partials of the LamMuZ launch are reduced and the verdict taken here
    // (a tail of the LamMuZ launch that did it instead - rda_opts::lmz_tail, rounds 2-5 - measured 2-4 % slower: tools/experiments/lmz_tail.patch).
    if (it > 0) {
        double rd = cl.resi_dual, rp = cl.resi_pri;
        if (cl.resi_iter != it) reduce_residuals(d, tid, cl.iters, rpre, res_pre, smem_su, rd, rp);          // (k_finish of a host-driven caller may have reduced them already)
        const bool stop_now = rd < d.c.iter_threshold && rp < d.c.iter_threshold;   // rda_solver.py:594
        if (fin && fin->verdict && tid == 0) __hip_atomic_store(fin->verdict, 2 * fin->vseq + (stop_now ? 1ull : 0ull), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (stop_now) {
            __syncthreads();
            if (tid == 0) d.ctrl->stop = 1;
            // The step ends here (rda_solver.py:594-596): hand the result over now - the launches still queued behind this one return
            // at once and k_finish finds the slot written.
            if (fin && fin->out_u) {
                publish_result(d, *fin);
                if (tid == 0) d.ctrl->finished = 1;
            }
            return;
        }
        __syncthreads();                // (the broadcast slot of the verdict is LDS of the solve)
    }
#ifdef SU_TRACE
    t_mark_[2] = clock64();                  // residuals reduced, verdict taken
#endif
    if (tid == 0) { d.ctrl->wl_count = 0; d.ctrl->wlc_count = 0; d.ctrl->hint_par = cl.hint_par ^ 1; }     // the LamMuZ launches of this iteration start with an empty work list and write the other support buffer
    if (d.su_pre) a.pose_ok = cl.pose_ok;
    a.status = &d.ctrl->st_tmp; a.ipm_iters = &d.ctrl->it_tmp; a.rd0 = &d.ctrl->rd0_tmp; a.prof = d.su_prof; a.split = d.su_split; a.accept = d.su_accept; a.first_attempt = d.su_first_attempt;
    su::Result res; res.rd0 = cl.rd0_tmp;
    a.land = d.su_land; a.land_tol[0] = d.su_land_tol[0]; a.land_tol[1] = d.su_land_tol[1]; a.land_tol[2] = d.su_land_tol[2]; a.land_stat = d.ctrl->land_stat; a.land_rho = d.su_land_rho;
    // warm start of iterations >= 1 from the multipliers of the previous su-solve of THIS step (only if that one converged)
    if (it > 0 && d.su_warm_mu0 > 0 && !((cl.su_status >> (it - 1)) & 1)) { a.warm_wfl = d.su_warm_wfl; a.warm_mu0 = d.su_warm_mu0; a.warm_cap = d.su_warm_cap; }
    if (it == 0 && d.su_warm_mu0 > 0 && d.su_warm_first) { a.warm_wfl = d.su_warm_wfl; a.warm_mu0 = d.su_warm_mu0; a.warm_cap = d.su_warm_cap; }
    a.warm_tau = d.su_warm_tau; a.warm_sig = d.su_warm_sig; a.warm_clip = d.su_warm_clip;
    // While consecutive su-problems are close (static scenes: the previous solve needed one or two iterations) the warm attempt starts
    // 1e-6 from the previous solution's active bounds with its multipliers and takes near-full steps: ONE iteration + the
    // convergence pass.  After a solve that needed more (moving obstacles, a changed active set) the moderate start above is used.
    // (su_last / su_probe / su_lam_keep are solver history of the handle: rda_reset clears them, rda_get/set_su_history carry them.)
    bool hard = false;
    if (a.warm_mu0 > 0 && d.su_easy_max > 0 && cl.su_last <= d.su_easy_max) {
        a.warm_wfl = d.su_easy[0]; a.warm_mu0 = d.su_easy[1]; a.warm_clip = d.su_easy[2]; a.warm_tau = d.su_easy[3]; a.warm_sig = d.su_easy[4];
        a.warm_nopred = d.su_easy_nopred;
    } else if (a.warm_mu0 > 0 && d.su_hard_mu0 > 0 && cl.prev_unconv && cl.su_hardlike && cl.su_last < 99) {
        // The ADMM of the previous step did not converge (a caller that re-sorts its obstacles every tick, quirk Q5; many moving obstacles)
        // AND consecutive su-problems really are far apart: the last solve's first iterate - the previous solution with its multipliers - had a
        // relative dual residual above su::HARD_RD0.  A warm attempt then does best from a point WELL inside the boxes (slack floor 1) with
        // the previous multipliers and next to no barrier (mu0 1e-3; the rows of d: su::HARD_DMU) - and it beats the cold start, so that rule is
        // skipped.  Oracle (same rule), interior-point iterations per su-solve: re-sorted north star 7.6 -> 5.7, N = 2000 8.1 -> 6.3, C4
        // re-sorted 14.2 -> 12.7, converged / easy loops unchanged.  (Round 4 keyed on the last solve's iteration count: a hard-started solve
        // costs >= 3 iterations whatever the problem, so `> 2` locked the easy start out - iter_num = 1: 1.0 -> 3.0 iterations per solve -
        // and `> 3` left most of the gain: 7.6 -> 6.2.)
        a.warm_wfl = d.su_hard_wfl; a.warm_mu0 = d.su_hard_mu0; a.hard_dmu = su::HARD_DMU; hard = true;
    }
    // Hard regime (many moving obstacles: consecutive su-problems are far apart): a warm attempt then needs MORE iterations than a cold
    // start.  While the last solve needed more than su_cold_from iterations the solve starts cold; every su_cold_probe-th such solve tries the
    // warm start again, so that the handle finds its way back when the scene calms down.
    // landing first: the warm-started su-problems
    a.land_level0 = (a.land && cl.land_hard > 0) ? 1 : 0;
    a.land_rho_prev = cl.land_rho_prev;
    const bool lf_eligible = a.warm_mu0 > 0 && a.land;       // (every warm attempt: ADMM iterations >= 1, and the first su-problem of a tick - the previous tick's solution shifted by one stage)
    if (lf_eligible) a.land_first = d.su_land_first == 2 ? (cl.spec_credit >= 0 ? 2 : 1) : d.su_land_first;
    const bool blind_opportunity = lf_eligible && d.su_land_first == 2 && it > 0 && cl.land_easy >= d.su_land_blind_from && d.su_land_blind_from > 0 && cl.land_rho_prev > 0;
    if (blind_opportunity && cl.blind_ok >= 0) a.land_blind = 1;
    if (!hard && a.warm_mu0 > 0 && d.su_cold_from > 0 && cl.su_last > d.su_cold_from && cl.su_last < 99 && cl.su_probe % d.su_cold_probe != d.su_cold_probe - 1) a.warm_mu0 = 0;
#ifdef SU_TRACE
    a.t_entry = t_entry_; t_mark_[3] = clock64();
    for (int k = 0; k < 4; ++k) a.t_mark[k] = t_mark_[k];
#endif
    su::solve<TT>(a, smem_su, pre, true, res, ref_wait);
    if (tid == 0) {                     // (from the verdict the solve left in registers and the copy of the control block: stores only)
        const int su_last = res.status == 0 ? res.iters : 99;
        d.ctrl->iters = it + 1;
        if (res.status != 0) d.ctrl->su_status = cl.su_status | (1 << it);
        d.ctrl->ipm_iters = cl.ipm_iters + res.iters;
        d.ctrl->su_last = su_last;
        d.ctrl->su_hardlike = res.rd0 > su::HARD_RD0;
        d.ctrl->su_probe = (d.su_cold_from > 0 && su_last > d.su_cold_from && su_last < 99) ? cl.su_probe + 1 : 0;
        d.ctrl->pose_ok = 0;          // the pose table has moved on; the LamMuZ launch that follows makes the masks that go with it
        if (a.land) {
            const bool easy1 = res.status == 0 && res.iters == 0 && res.rounds_all == 1;
            d.ctrl->land_easy = easy1 ? (cl.land_easy < 8 ? cl.land_easy + 1 : 8) : 0;
            if (res.land_rho > 0) d.ctrl->land_rho_prev = res.land_rho;
            if (blind_opportunity) d.ctrl->blind_ok = res.blind == 1 ? (cl.blind_ok < 4 ? cl.blind_ok + 1 : 4) : (res.blind == 2 ? -6 : (cl.blind_ok < 0 ? cl.blind_ok + 1 : cl.blind_ok));
        }
        if (a.land && res.status == 0) {
            // sticky: a landing of three or more rounds sends the next FOUR solves to the later stop (a good landing at the later stop says nothing about the
            // earlier one: with a one-solve memory C4 alternated between the two levels)
            int lh = cl.land_hard;
            if (res.land_rounds >= 3) lh = 4; else if (lh > 0) lh -= 1;
            d.ctrl->land_hard = lh;
        }
        if (lf_eligible && d.su_land_first == 2) {
            // speculative landings pay where consecutive su-problems keep their active set (static scenes: 50 - 65 % accepted) and cost two landing rounds where
            // they do not (C4, moving obstacles: none accepted): a handle that keeps failing tries every third eligible solve only; at one success in two the credit grows
            int cr = cl.spec_credit;
            if (res.spec == 1) cr = cr + 3 > 6 ? 6 : cr + 3; else if (res.spec == 2) cr -= 2; else if (cr < 0) cr += 1;
            d.ctrl->spec_credit = cr;
        }
    }
}

template <int TT> __global__ __launch_bounds__(su::NT) void k_su(Dev d, int it, const double *in_s, const double *in_u, Fin fin)
{
    warm_kernargs<sizeof(Dev) + 2 * sizeof(void *) + sizeof(int) + sizeof(Fin)>();
    su_body<TT>(d, it, in_s, in_u, d.ref, d.ref_speed, nullptr, 0, &fin);
}

// final bookkeeping of a step that ran all its iterations: residuals of the last one, result slot
__device__ __forceinline__ void finish_body(const Dev &d, const Fin &f)
{
    if (d.ctrl->finished) return;                   // (uniform) the launch that ended the step already handed the result over
    if (!d.ctrl->stop && d.ctrl->resi_iter != d.ctrl->iters) { ResPre none; double rd, rp; reduce_residuals(d, threadIdx.x, d.ctrl->iters, none, false, nullptr, rd, rp); }
    __syncthreads();
    publish_result(d, f);
}

__global__ __launch_bounds__(su::NT) void k_finish(Dev d, Fin f) { finish_body(d, f); }

__device__ __forceinline__ void begin_body(const Dev &d)
{
    if (threadIdx.x == 0) {
        d.ctrl->stop = 0; d.ctrl->iters = 0; d.ctrl->su_status = 0; d.ctrl->ipm_iters = 0; d.ctrl->lmz_fail = 0;
        d.ctrl->resi_dual = 0; d.ctrl->resi_pri = 0; d.ctrl->finished = 0; d.ctrl->wl_count = 0; d.ctrl->wlc_count = 0; d.ctrl->resi_iter = 0;
    }
}

__global__ void k_begin(Dev d) { begin_body(d); }

// ------------------------------------------------------------------------------------------------
// K1: one wavefront per (obstacle n, stage t); 4 wavefronts per workgroup.
// candidate list + vertices of every staged obstacle slot (one wave per (slot, time slot)); runs once per upload
__device__ __forceinline__ void prepare_body(const Dev &d, lmz::WaveLDS *wl)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, E = d.c.E;
    const int w = blockIdx.x * 4 + wv;
    if (w >= d.c.N * d.nt) return;
    const int n = w / d.nt;
    lmz::WaveLDS &W = wl[wv];
    if (lane < 2 * E) W.A[lane >> 1][lane & 1] = d.A[(size_t)w * E * 2 + lane];
    if (lane < E) W.b[lane] = d.b[(size_t)w * E + lane];
    lmz::wave_sync();
    lmz::build_lists(W, E, d.cone[n], lane);
    lmz::wave_sync();
    if (lane < d.oc_ls) d.oc_lamc[(size_t)w * d.oc_ls + lane] = W.lamc[lane];
    if (lane < d.oc_vs) d.oc_vtx[(size_t)w * d.oc_vs + lane] = (&W.vtx[0][0])[lane];
    if (lane == 0) { d.oc_cnt[2 * w] = W.npv; d.oc_cnt[2 * w + 1] = W.nlv; }
}
__global__ __launch_bounds__(256) void k_prepare(Dev d) { __shared__ lmz::WaveLDS wl[4]; prepare_body(d, wl); }
__global__ __launch_bounds__(256) void k_prepare_fleet(const Dev *devs)
{
    __shared__ lmz::WaveLDS wl[4];
    if (!devs[blockIdx.y].obstacle_num) return;      // (uniform) a member without staged obstacles has no slots to list (rda_fleet_upload_scans: zero boxes)
    prepare_body(devs[blockIdx.y], wl);
}

// Unit w of a rank's LamMuZ grid -> (stage t, local slot nl): the SLOT runs fastest and a stage is padded to GS J units, so a
// workgroup of the packed kernels (GS = 8 rows: 2 waves x 4 rows) owns the slots GS j .. GS j + GS-1 of ONE stage: with the stage-major
// dual arrays and the [T][Nloc] condensed-term arrays everything it reads and writes are whole 64-byte half lines, and its rows reduce
// to one block partial.  (Two-wave workgroups: the north-star grid T J = 500 of them is ONE round on 256 CUs at one wave per SIMD.)
__device__ __forceinline__ void unit_of(const Dev &d, int w, int &t, int &nl) { const int S = GS * d.J; t = w / S; nl = w - t * S; }
// Launch index of a packed workgroup -> its block (stage t, GS-slot group j), or t = -1 for a filler.  Workgroups are handed to the
// 8 XCDs round robin (block b runs on XCD b % 8 - observed, used for speed only), and each XCD has its own L2.  The T workgroups that
// share the staged data of the same obstacles (half-spaces, candidate lists, vertices: ~0.5 KB per slot, read once per STAGE) should
// meet in ONE L2, and every XCD must get the same number of workgroups (the north-star grid is exactly one round of the chip): the
// blocks are numbered group-major (u = j T + t) and cut into 8 equal contiguous ranges, one per XCD - a group's stages land on one
// XCD (two for the few groups a cut goes through), neighbouring groups (which share the 128-byte lines of the [T][N] arrays) too.
//   b = 8 q + x ;  u = x per + q ,  per = ceil(T J / 8) ;  j = u / T ,  t = u % T
__device__ __forceinline__ void block_of(const Dev &d, int b, int &t, int &j)
{
    const int T = d.c.T, W = T * d.J, per = (W + 7) / 8, x = b & 7, q = b >> 3, u = x * per + q;
    j = u / T; t = u - j * T;
    if (u >= W) t = -1;
}

// What one solved (or failed) row hands to the su-problem and to the residuals, as stored in the coef arrays
struct RowOut { double ax, ay, bl, c3, c4, c5, res, hh; };
__device__ __forceinline__ void store_row(const Dev &d, int k, const RowOut &o)
{
    coef_arr(d, d.rank, 0)[k] = o.ax; coef_arr(d, d.rank, 1)[k] = o.ay; coef_arr(d, d.rank, 2)[k] = o.bl;   // rda_solver.py:541-542
    coef_arr(d, d.rank, 3)[k] = o.c3; coef_arr(d, d.rank, 4)[k] = o.c4; coef_arr(d, d.rank, 5)[k] = o.c5;
    coef_arr(d, d.rank, 6)[k] = o.res; coef_arr(d, d.rank, 7)[k] = o.hh; coef_arr(d, d.rank, 8)[k] = o.bl + o.c3;
}
// a row that cannot be solved (non-finite data or result): previous lam, mu, z, xi, zeta stay; the stage drops out of the su hinge
// (a = 0, offset and g as they were); its residual is inf (rda_solver.py:781-793)
__device__ __forceinline__ RowOut failed_row(const Dev &d, int k)
{
    RowOut o; o.ax = 0; o.ay = 0; o.bl = 0; o.c3 = coef_arr(d, d.rank, 3)[k]; o.c4 = coef_arr(d, d.rank, 4)[k]; o.c5 = coef_arr(d, d.rank, 5)[k];
    o.res = INFINITY; o.hh = 0;
    return o;
}

// GS row records [GS][6] = (|a|^2, g.a, g x a, dual residual, |Hm|^2, near) in LDS -> the block partial of (stage t, block j): threads
// q = 0..4 sum one quantity over the rows IN ROW ORDER (dead rows hold zeros), thread 5 packs the near mask.  Stored write-through
// (sc1: 8-byte agent-scope stores), as round 2's tail of the launch read them without a release fence (tools/experiments/lmz_tail.patch); kept: the next su launch reads them from L2 either way.
__device__ __forceinline__ void block_partial(const Dev &d, int t, int j, const double (*rowv)[6], int q)
{
    const size_t bi = (size_t)t * d.J + j;
    if (q < NBS) {
        double acc = 0;
        for (int r = 0; r < GS; ++r) acc += rowv[r][q];
        __hip_atomic_store(bsum_arr(d, d.rank) + bi * NBS + q, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (q == NBS) {
        unsigned long long m = 0;
        for (int r = 0; r < GS; ++r) m |= rowv[r][5] != 0.0 ? 1ull << r : 0ull;
        __hip_atomic_store(bmask_arr(d, d.rank) + bi, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ __forceinline__ void row_record(double *rv, const Dev &d, const RowOut &o, double px, double py)
{
    const su::RowTerm q = su::row_term(o.ax, o.ay, o.c4, o.c5, o.bl + o.c3, px, py, d.c.max_sd, true);
    rv[0] = q.aa; rv[1] = q.ga; rv[2] = q.gxa; rv[3] = o.res; rv[4] = o.hh; rv[5] = (!d.c.accelerated || q.near) ? 1.0 : 0.0;
}

// K1, one (slot, stage) sub-problem per wavefront; 4 wavefronts per workgroup (shapes with E+R+1 > 16, RDA_LMZ_ROWS=0, and the
// no-obstacle case).  Writes the per-row terms only: k_lmz_finalize forms the block partials and runs the tail behind it.
__device__ __forceinline__ size_t hint_key(const Dev &d, int n, int t)
{
    int key = n;
    if (d.slot_src && n < d.src_used) { const int src = d.slot_src[n]; if (src >= 0 && src < d.src_cap) key = d.c.N + src; }
    return (size_t)t * d.hint_stride + key;
}
// `first` = first LamMuZ launch of a tick: the support remembered for stage t+1 of the previous tick
__device__ __forceinline__ int hint_read(const Dev &d, int par, int n, int t, bool first)
{
    return d.hint[(size_t)(par ^ 1) * d.hint_len + hint_key(d, n, first && t + 1 < d.c.T ? t + 1 : t)];
}
__device__ __forceinline__ void hint_write(const Dev &d, int par, int n, int t, int v) { d.hint[(size_t)par * d.hint_len + hint_key(d, n, t)] = v; }
// ... with the slot's source already at hand (`src` = slot_src[n], or -1 where hint_key would not read it): the same key without the trip to memory for it
__device__ __forceinline__ void hint_write_src(const Dev &d, int par, int n, int t, int src, int v)
{
    const int key = (src >= 0 && src < d.src_cap) ? d.c.N + src : n;
    d.hint[(size_t)par * d.hint_len + (size_t)t * d.hint_stride + key] = v;
}

__device__ __forceinline__ void lammuz_body(const Dev &d, const int block, const int it)
{
#pragma clang fp contract(on)          // see lammuz_device.h: results independent of the kernel the body is compiled into
    __shared__ lmz::WaveLDS wl[4];
    __shared__ lmz::RobotLDS rb;
    const int T = d.c.T, N = d.c.N, E = d.c.E, R = d.c.R;
    if (d.ctrl->stop) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (d.obstacle_num == 0) {
        // quirk Q9 (rda_solver.py:564-568): only slot N-1 loses its lam'A / lam'b products
        if (block == 0 && d.rank == (N - 1) / d.Nloc)
            for (int t = threadIdx.x; t < T; t += 256) {
                int i = t * d.Nloc + (N - 1) % d.Nloc;
                coef_arr(d, d.rank, 0)[i] = 0; coef_arr(d, d.rank, 1)[i] = 0; coef_arr(d, d.rank, 2)[i] = 0;
                coef_arr(d, d.rank, 8)[i] = coef_arr(d, d.rank, 3)[i];
            }
        return;
    }
    if (threadIdx.x < 2 * R) rb.G[threadIdx.x >> 1][threadIdx.x & 1] = d.G[threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x < 64 + R) rb.h[threadIdx.x - 64] = d.h[threadIdx.x - 64];
    if (threadIdx.x >= 128 && threadIdx.x < 128 + 40) rb.muc[threadIdx.x - 128] = d.muc[threadIdx.x - 128];
    if (threadIdx.x >= 192 && threadIdx.x < 192 + 56) (&rb.rv[0][0])[threadIdx.x - 192] = (&d.rv[0][0])[threadIdx.x - 192];
    if (threadIdx.x == 255) { rb.nmv = d.nmv; rb.nrv = d.nrv; }
    const int w = block * 4 + wv;
    int t, nl; unit_of(d, w, t, nl);
    const bool live = t < T && nl < d.Nlive;
    if (!live) { t = 0; nl = 0; }
    const int n = d.rank * d.Nloc + nl;                        // this rank's obstacle shard [rank*Nloc, (rank+1)*Nloc)
    lmz::WaveLDS &W = wl[wv];
    const size_t ao = ((size_t)n * d.nt + (d.nt > 1 ? t + 1 : 0)) * E;
    if (lane < 2 * E) W.A[lane >> 1][lane & 1] = d.A[ao * 2 + lane];
    if (lane < E) W.b[lane] = d.b[ao + lane];
    __syncthreads();
    if (!live) return;
    lmz::Params P;
    P.E = E; P.R = R; P.norm2 = d.cone[n];
    const double *ps = d.pose + 4 * t;                        // position of column t+1, heading of column t (quirk Q1)
    P.px = ps[0]; P.py = ps[1]; P.cs = ps[2]; P.sn = ps[3];
    const size_t o = drow(d, n, t + 1), zi = drow(d, n, t);
    P.xi0 = d.xi[2 * o]; P.xi1 = d.xi[2 * o + 1];
    const double zeta = d.zeta[zi], dbar = d.dis[t];
    P.kappa0 = zeta - dbar; P.ro2 = d.c.ro2; P.delta = d.c.delta;
    lmz::Sol best;
    // previous value of this lane's dual entry: warm start of the support + the dual residual below
    double prev = 0.0;
    if (lane < E) prev = d.lam[o * E + lane];
    else if (lane < E + R) prev = d.mu[o * R + lane - E];
    // A sub-problem whose data are not finite cannot be solved: like a LamMuZ solve of the reference that does not end OPTIMAL
    // (rda_solver.py:781-793) it keeps its previous duals and its residual is inf (no early stop).  The solver below is run on
    // harmless stand-in data instead (its loops then see no NaN) and its answer is dropped.
    bool bad = !isfinite(P.px + P.py + P.cs + P.sn + P.xi0 + P.xi1 + P.kappa0);
    if (lane < 2 * E) bad = bad || !isfinite(W.A[lane >> 1][lane & 1]);
    if (lane < E) bad = bad || !isfinite(W.b[lane]);
    bad = __ballot(bad) != 0;
    if (bad) {
        if (lane < 2 * E) W.A[lane >> 1][lane & 1] = 0;
        if (lane < E) W.b[lane] = 0;
        P.px = P.py = P.sn = P.xi0 = P.xi1 = P.kappa0 = 0; P.cs = 1;
        lmz::wave_sync();
    }
    lmz::pose_products(W, P, lane);
    {   // candidate list and vertices of this slot from the upload-time cache
        const size_t oc = (size_t)n * d.nt + (d.nt > 1 ? t + 1 : 0);
        if (lane < d.oc_ls) W.lamc[lane] = d.oc_lamc[oc * d.oc_ls + lane];
        if (lane < d.oc_vs) (&W.vtx[0][0])[lane] = d.oc_vtx[oc * d.oc_vs + lane];
        if (lane == 0) { W.npv = d.oc_cnt[2 * oc]; W.nlv = d.oc_cnt[2 * oc + 1]; }
    }
    lmz::wave_sync();
    const int hpar = d.ctrl->hint_par & 1;
    if (!d.warm || !lmz::solve_wave_warm<64>(W, rb, P, lane, hint_read(d, hpar, n, t, it == 0), best)) lmz::solve_wave(W, rb, P, lane, best);
    if (lane == 0) hint_write(d, hpar, n, t, best.id >> 1);
    if (d.centre) lmz::central_normal_wave<64>(W, rb, P, lane, best);
    bad = bad || !(isfinite(best.cost) && isfinite(best.m) && isfinite(best.H0) && isfinite(best.H1));
    const int k = t * d.Nloc + nl;
    if (bad) {
        if (lane == 0) {
            store_row(d, k, failed_row(d, k));
            hint_write(d, hpar, n, t, -1);
            atomicAdd(&d.ctrl->lmz_fail, 1);
        }
        return;
    }
    // ---- fused dual / residual updates (every lane holds the winner) ----------------------------
    const double znew = (d.c.accelerated ? 0.5 : 1.0) * (best.m > 0 ? best.m : 0.0);     // tie-break T2
    double res = 0;
    if (lane < E) {
        double v = lmz::lam_of(best, P.norm2, lane);
        res = (v - prev) * (v - prev); d.lam[o * E + lane] = v;
    } else if (lane < E + R) {
        int j = lane - E;
        double v = lmz::mu_of(best, j);
        res = (v - prev) * (v - prev); d.mu[o * R + j] = v;
    } else if (lane == E + R) {
        double old = d.z[zi];
        res = (znew - old) * (znew - old); d.z[zi] = znew;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) res += __shfl_xor(res, off, 64);
    if (lane == 0) {
        double ax = 0, ay = 0, bl = 0, mh = 0, gx = 0, gy = 0;
        for (int i = 0; i < E; ++i) {
            double v = lmz::lam_of(best, P.norm2, i);
            ax += v * W.A[i][0]; ay += v * W.A[i][1]; bl += v * W.b[i];
        }
        for (int j = 0; j < R; ++j) {
            double v = lmz::mu_of(best, j);
            mh += v * rb.h[j]; gx += v * rb.G[j][0]; gy += v * rb.G[j][1];
        }
        const double hx = gx + P.cs * ax + P.sn * ay, hy = gy - P.sn * ax + P.cs * ay;      // Hm, :682
        const double xin0 = P.xi0 + hx, xin1 = P.xi1 + hy;                                  // :683
        d.xi[2 * o] = xin0; d.xi[2 * o + 1] = xin1;
        const double im = ax * P.px + ay * P.py - bl - mh;                                  // :659
        const double zetan = zeta + im - dbar - znew;                                       // :666
        d.zeta[zi] = zetan;
        RowOut ro; ro.ax = ax; ro.ay = ay; ro.bl = bl; ro.c3 = mh + znew - zetan; ro.c4 = gx + xin0; ro.c5 = gy + xin1;
        ro.res = res; ro.hh = hx * hx + hy * hy;
        store_row(d, k, ro);
    }
}

__global__ __launch_bounds__(256) void k_lammuz(Dev d, int it) { lammuz_body(d, blockIdx.x, it); }

// K1, packed: FOUR sub-problems per wavefront, one per 16-lane DPP row (16 per workgroup).  The warm-started path - one
// candidate on two lanes, the optimality certificate on E+R lanes, the central-normal step on (vertex, vertex) pairs, the
// dual updates on E+R+1 lanes - never used more than a quarter of a wave, and the kernel is bound by instruction issue
// (DESIGN.md section 5): the rows run it side by side.  Only a row whose certificate fails needs the 64-lane enumeration;
// those rows are served one after the other by the whole wave.  Same device functions, same arithmetic, same results as
// lammuz_body.  Requires E + R + 1 <= 16 (else the one-per-wave body is launched).
// MODE 0: everything in one kernel (single ego, latency), INCLUDING the block partial of the workgroup's GS slots.  Dense grids are served by
//         three launches instead:
// MODE 1: the common path only - three waves per SIMD, no spills; a row whose warm candidate fails its certificate goes on the
//         handle's work list (Dev::wl) and writes nothing;
// MODE 2: the rows on the work list, ONE per wave (row 0 of the wave; rows 1-3 idle) and pass, straight to the enumeration, then
//         the very same 16-lane code as modes 0 / 1 - so the results do not depend on which launch solved a row;
//         then k_lmz_finalize: block partials from the stored terms (same function, same order as mode 0) and the tail.
#ifdef RDA_LMZ_CLK
__device__ unsigned long long *g_lmz_clk = nullptr;
constexpr int LMZ_CLK_WORDS = 32;                  // per wave: [0..7] sections, [8..14] counts / totals / wall clock, [16..31] sub-marks (tools/lmz_wave_clocks.py)
__device__ int *g_lmz_faillog = nullptr;          // [0] count, then (old hint, new support id, circle?) triples of the rows whose certificate failed
#endif
template <int MODE = 0, bool CW = false> __device__ __forceinline__ void lammuz_body_rows(const Dev &d, const int block, const int nblocks, const int it, const Fin &fin)
{
#pragma clang fp contract(on)          // see lammuz_device.h
    constexpr int WPB = GS / 4;        // waves per workgroup (4 rows each)
    // The single-ego latency form (k_lammuz_rows, one wave per SIMD: the launch is one wave's dependent chain) runs the tail of the row on the row's lanes and
    // takes three trips to memory off the chain (hint_par inside the batch, the robot tables, the slot's source for the hint write): DESIGN.md 3.1.  The forms
    // that share their SIMD (dense, common path, work list, fleet) keep the one-lane tail: the lane-parallel one costs them 6 - 14 more spilled registers, and
    // they are bound by issue, not by latency.
    constexpr bool LANES = CW;
    __shared__ lmz::WaveLDS wl[GS];
    __shared__ lmz::RobotLDS rb;
    __shared__ double rowv[MODE == 0 ? GS : 1][6];
    const int T = d.c.T, E = d.c.E, R = d.c.R;
#ifdef RDA_LMZ_CLK
    // debug build only (tools/lmz_wave_clocks.py): clock64 ticks per section of a wave, in the wave's own LMZ_CLK_WORDS-word slot of g_lmz_clk
    long long clk_prev = clock64(); const long long clk_in = clk_prev; bool clk_enum = false; const unsigned long long clk_wall_in = (unsigned long long)wall_clock64();
    unsigned long long *const clk_slot = g_lmz_clk ? g_lmz_clk + LMZ_CLK_WORDS * (size_t)(block * (GS / 4) + (threadIdx.x >> 6)) : nullptr;
    long long clk_sub = clk_prev;      // LMZ_SUB(k): ticks since the previous mark of either kind, into word 16 + k - the sub-marks split a section, its rest is what follows the last one
#define LMZ_CLK(k) do { if (MODE == 0) { const long long now_ = clock64(); if (clk_slot && (threadIdx.x & 63) == 0) clk_slot[k] += (unsigned long long)(now_ - clk_prev); clk_prev = now_; clk_sub = now_; } } while (0)
#define LMZ_SUB(k) do { if (MODE == 0) { const long long now_ = clock64(); if (clk_slot && (threadIdx.x & 63) == 0) clk_slot[16 + (k)] += (unsigned long long)(now_ - clk_sub); clk_sub = now_; } } while (0)
#else
#define LMZ_CLK(k) do { } while (0)
#define LMZ_SUB(k) do { } while (0)
#endif
    int tb = 0, jb = 0;                                        // (modes 0, 1) the workgroup's block: stage and GS-slot group
    if (MODE != 2) { block_of(d, block, tb, jb); if (tb < 0) return; }      // a filler of the XCD-aware launch order
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, row = lane >> 4, gl = lane & 15;
    // MODE 0 (one ego, one wave per SIMD: the launch IS the dependent chain of one wave, and six of its links were trips to the L2 -
    // stop flag, half-spaces, pose / duals, support cache, slot -> obstacle, remembered support): everything a row reads is requested
    // here, in two batches, before the first of them is waited for.  The throughput forms (modes 1, 2) keep their loads where the
    // values are used: there the registers are worth more than the latency (three waves per SIMD hide it).
    struct Early { double px, py, cs, sn, xi0, xi1, zeta, dbar, prev, vtx[4], A, b, G, h, zold, rv; int cone, src, hpar, hint, npv, nlv; unsigned char lamc[3], muc; } ey;
    if (MODE == 0) {
        const int nl0 = jb * GS + wv * 4 + row, nl = nl0 < d.Nlive ? nl0 : 0, n = d.rank * d.Nloc + nl;
        ey.src = (d.slot_src && n < d.src_used) ? d.slot_src[n] : -1;
        ey.hpar = d.ctrl->hint_par & 1;
        // the robot's candidate tables sit in the kernel arguments and are indexed per thread: a trip to memory of their own, which stood between the batch
        // below and the barrier (load, wait, LDS store).  One element per thread (56 <= the workgroup), requested here with the first loads of the launch
        static_assert(64 * WPB >= 56, "one element of the robot tables per thread");
        if (LANES) { ey.muc = d.muc[(int)threadIdx.x < 40 ? threadIdx.x : 0]; ey.rv = (&d.rv[0][0])[(int)threadIdx.x < 56 ? threadIdx.x : 0]; }
    }
    if (LANES) {
        // hint_par was requested above, yet it is only used by the batch below, and the compiler moved its load there: issued in the middle of the batch and waited
        // for at once (the address of the remembered support needs it) - a whole trip to the L2 inside the issue of the batch.  Pinned: it arrives with the stop flag,
        // a word of the same line
        int stop = d.ctrl->stop;
        asm volatile("" : "+v"(ey.hpar), "+v"(stop));
        ey.hpar = __builtin_amdgcn_readfirstlane(ey.hpar);      // (both are the same for every lane: scalar again behind the pin)
        if (__builtin_amdgcn_readfirstlane(stop)) return;
    } else
    if (d.ctrl->stop) return;                                 // (not merged into the batch below: launches behind the stop flag are on the next tick's way and must stay short - measured)
    if (MODE == 2 && block * WPB >= d.ctrl->wl_count + (d.ctrl->wlc_count + 3) / 4) return;  // work-list form: nothing for this workgroup (the list is short or empty since round 3: no trip for the robot data)
    LMZ_CLK(0);
    if (MODE == 0) {
        const int t = tb, nl0 = jb * GS + wv * 4 + row, nl = nl0 < d.Nlive ? nl0 : 0, n = d.rank * d.Nloc + nl;
        const double *ps = d.pose + 4 * t;
        const size_t o = drow(d, n, t + 1), zi = drow(d, n, t), oc = (size_t)n * d.nt + (d.nt > 1 ? t + 1 : 0);
        ey.px = ps[0]; ey.py = ps[1]; ey.cs = ps[2]; ey.sn = ps[3];
        ey.xi0 = d.xi[2 * o]; ey.xi1 = d.xi[2 * o + 1]; ey.zeta = d.zeta[zi]; ey.dbar = d.dis[t]; ey.cone = d.cone[n];
        ey.zold = d.z[zi];                // (the previous z of the row's residual: it was fetched where it is used, a trip to memory inside the update phase)
        // (ONE unconditional load through a selected address: as `gl < E ? lam : (gl < E + R ? mu : 0)` the two loads shared their destination register and the
        // second one waited - vmcnt(0), in the middle of the batch - for the first; lanes beyond E + R read lam[0] and are zeroed where `prev` is used.  Round 6)
        ey.prev = *(gl < E ? &d.lam[o * E + gl] : (gl < E + R ? &d.mu[o * R + gl - E] : &d.lam[o * E]));
        // half-spaces of the row and the robot's (G, h): they used to be fetched one after the other behind this batch - load, vmcnt(0), LDS store, four times
        // (G, h, A, b): four dependent trips to the L2 in a launch that IS one wave's dependent chain
        {
            const size_t ao = ((size_t)n * d.nt + (d.nt > 1 ? t + 1 : 0)) * E;
            ey.A = d.A[ao * 2 + (gl < 2 * E ? gl : 0)]; ey.b = d.b[ao + (gl < E ? gl : 0)];
            ey.G = d.G[(int)threadIdx.x < 2 * R ? threadIdx.x : 0]; ey.h = d.h[(int)threadIdx.x < R ? threadIdx.x : 0];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) ey.lamc[k] = gl + 16 * k < d.oc_ls ? d.oc_lamc[oc * d.oc_ls + gl + 16 * k] : (unsigned char)0;      // (wave-uniform bounds for k >= 1 at E <= 5: whole loads drop out)
#pragma unroll
        for (int k = 0; k < 4; ++k) ey.vtx[k] = gl + 16 * k < d.oc_vs ? d.oc_vtx[oc * d.oc_vs + gl + 16 * k] : 0.0;
        ey.npv = d.oc_cnt[2 * oc]; ey.nlv = d.oc_cnt[2 * oc + 1];
        {   // the remembered support (hint_read with the slot's source already at hand)
            const int key = (ey.src >= 0 && ey.src < d.src_cap) ? d.c.N + ey.src : n, tr = (it == 0 && t + 1 < T) ? t + 1 : t;
            ey.hint = d.hint[(size_t)(ey.hpar ^ 1) * d.hint_len + (size_t)tr * d.hint_stride + key];
        }
    }
    LMZ_SUB(0);
    if (MODE == 0) {                                          // (2 R <= 16 < the workgroup: one element per thread, from the batch above)
        if ((int)threadIdx.x < 2 * R) rb.G[threadIdx.x >> 1][threadIdx.x & 1] = ey.G;
        if ((int)threadIdx.x < R) rb.h[threadIdx.x] = ey.h;
    } else {
        for (int i = threadIdx.x; i < 2 * R; i += 64 * WPB) rb.G[i >> 1][i & 1] = d.G[i];
        for (int i = threadIdx.x; i < R; i += 64 * WPB) rb.h[i] = d.h[i];
    }
    if (LANES) {
        if ((int)threadIdx.x < 40) rb.muc[threadIdx.x] = ey.muc;
        if ((int)threadIdx.x < 56) (&rb.rv[0][0])[threadIdx.x] = ey.rv;
    } else {
        for (int i = threadIdx.x; i < 40; i += 64 * WPB) rb.muc[i] = d.muc[i];
        for (int i = threadIdx.x; i < 56; i += 64 * WPB) (&rb.rv[0][0])[i] = (&d.rv[0][0])[i];
    }
    if (threadIdx.x == 0) { rb.nmv = d.nmv; rb.nrv = d.nrv; }
    LMZ_SUB(1);
    // Work-list form: the list has two ends.  Polygon rows (from the front, Ctrl::wl_count) take a wave each: they go straight to the 64-lane enumeration.
    // Circle rows (from the back, Ctrl::wlc_count) take a 16-lane row each, FOUR per wave: their remembered case runs side by side like in the single-ego
    // form, and only a row whose certificate fails is enumerated by its wave (round 6).  A wave slot = one polygon row or one group of four circle rows.
    const int cntP = MODE == 2 ? d.ctrl->wl_count : 1, cntC = MODE == 2 ? d.ctrl->wlc_count : 0;
    const int cnt = cntP + (cntC + 3) / 4;
    for (int base = MODE == 2 ? block * WPB : 0; base < cnt; base += MODE == 2 ? nblocks * WPB : 1) {       // modes 0, 1: one pass
    if (MODE == 2) __syncthreads();                            // the slabs of the previous pass are free again
    const bool entry = MODE == 2 && base + wv < cnt;            // (wave-uniform) this wave has a work-list slot in this pass
    // a row past the end (a dead slot of the padded stage, an idle row of mode 2) shadows an existing unit and writes nothing
    int t, nl;
    bool live2 = false;
    if (MODE == 2) {
        const int sl = entry ? base + wv : base;               // (a wave without a slot shadows the first slot of the pass)
        int widx;
        if (sl < cntP) { widx = sl; live2 = entry && row == 0; }
        else { const int c0 = 4 * (sl - cntP), ci = c0 + row; live2 = entry && ci < cntC; widx = d.wl_cap - 1 - (live2 ? ci : c0); }
        unit_of(d, d.wl[widx], t, nl);
    } else { t = tb; nl = jb * GS + wv * 4 + row; }
    const bool live = MODE == 2 ? live2 : nl < d.Nlive;
    if (!live) nl = 0;
    const int n = d.rank * d.Nloc + nl;
    lmz::WaveLDS &W = wl[wv * 4 + row];
    const size_t ao = ((size_t)n * d.nt + (d.nt > 1 ? t + 1 : 0)) * E;
    if (MODE == 0) {
        if (gl < 2 * E) W.A[gl >> 1][gl & 1] = ey.A;
        if (gl < E) W.b[gl] = ey.b;
    } else {
        if (gl < 2 * E) W.A[gl >> 1][gl & 1] = d.A[ao * 2 + gl];
        if (gl < E) W.b[gl] = d.b[ao + gl];
    }
    LMZ_SUB(2);
    __syncthreads();
    LMZ_CLK(1);
    lmz::Params P;
    P.E = E; P.R = R; P.norm2 = MODE == 0 ? ey.cone : d.cone[n];
    const double *ps = d.pose + 4 * t;                        // position of column t+1, cos / sin of the heading of column t (quirk Q1)
    if (MODE == 0) { P.px = ey.px; P.py = ey.py; P.cs = ey.cs; P.sn = ey.sn; }
    else { P.px = ps[0]; P.py = ps[1]; P.cs = ps[2]; P.sn = ps[3]; }
    const size_t o = drow(d, n, t + 1), zi = drow(d, n, t);
    if (MODE == 0) { P.xi0 = ey.xi0; P.xi1 = ey.xi1; } else { P.xi0 = d.xi[2 * o]; P.xi1 = d.xi[2 * o + 1]; }
    const double zeta = MODE == 0 ? ey.zeta : d.zeta[zi], dbar = MODE == 0 ? ey.dbar : d.dis[t];
    P.kappa0 = zeta - dbar; P.ro2 = d.c.ro2; P.delta = d.c.delta;
    lmz::Sol best;
    double prev = 0.0;
    if (MODE == 0) prev = gl < E + R ? ey.prev : 0.0;
    else if (gl < E) prev = d.lam[o * E + gl];
    else if (gl < E + R) prev = d.mu[o * R + gl - E];
    // non-finite data: see lammuz_body (the row solves harmless stand-in data, keeps its previous duals, residual inf)
    const double px0 = P.px, py0 = P.py;                       // (the pose as read: a failed row overwrites it with stand-ins)
    bool bad = !isfinite(P.px + P.py + P.cs + P.sn + P.xi0 + P.xi1 + P.kappa0);
    if (gl < 2 * E) bad = bad || !isfinite(W.A[gl >> 1][gl & 1]);
    if (gl < E) bad = bad || !isfinite(W.b[gl]);
    bad = ((__ballot(bad) >> (16 * row)) & 0xffffull) != 0;
    if (bad) {
        if (gl < 2 * E) W.A[gl >> 1][gl & 1] = 0;
        if (gl < E) W.b[gl] = 0;
        P.px = P.py = P.sn = P.xi0 = P.xi1 = P.kappa0 = 0; P.cs = 1;
    }
    lmz::wave_sync();
    lmz::pose_products(W, P, gl);
    {
        const size_t oc = (size_t)n * d.nt + (d.nt > 1 ? t + 1 : 0);
        if (MODE == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) if (gl + 16 * k < d.oc_ls) W.lamc[gl + 16 * k] = ey.lamc[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) if (gl + 16 * k < d.oc_vs) (&W.vtx[0][0])[gl + 16 * k] = ey.vtx[k];
            if (gl == 0) { W.npv = ey.npv; W.nlv = ey.nlv; }
        } else {
            for (int i = gl; i < d.oc_ls; i += 16) W.lamc[i] = d.oc_lamc[oc * d.oc_ls + i];
            for (int i = gl; i < d.oc_vs; i += 16) (&W.vtx[0][0])[i] = d.oc_vtx[oc * d.oc_vs + i];
            if (gl == 0) { W.npv = d.oc_cnt[2 * oc]; W.nlv = d.oc_cnt[2 * oc + 1]; }
        }
    }
    lmz::wave_sync();
    LMZ_CLK(2);
    const int hpar = MODE == 0 ? ey.hpar : (d.ctrl->hint_par & 1);
    // (work-list form: only a CIRCLE row reads its remembered support - round 6, see below)
    const int hint_in = MODE == 0 ? ey.hint : (MODE != 2 ? hint_read(d, hpar, n, t, it == 0) : ((P.norm2 && live) ? hint_read(d, hpar, n, t, it == 0) : -1));
    bool ok = MODE != 2 && d.warm && lmz::solve_wave_warm<16>(W, rb, P, lane, hint_in, best);
    // CW (the single-ego kernel only, see lmz::warm_circle): the remembered case of a circle obstacle's row, four rows of the wave side by side
    if (CW && MODE == 0 && d.warm && P.norm2 && live && !bad) ok = lmz::warm_circle<16>(W, rb, P, lane, hint_in, best);
    // ... and in the WORK-LIST form (round 6): the common-path kernel of the dense launch forms and the fleet cannot afford the circle cases inline (registers:
    // lmz::warm_circle's header), so it defers every circle row - and the work-list kernel used to enumerate each of them, on every ADMM iteration (64 lanes, the
    // interior candidate a Newton iteration: ~31 k cycles a row).  This kernel has the registers (one wave per SIMD): the remembered case first, the enumeration
    // only when its certificate fails - the same routine as the single-ego form, so a circle row's answer no longer depends on the launch form.
    if (MODE == 2 && d.warm && P.norm2 && live && !bad) ok = lmz::warm_circle<16>(W, rb, P, lane, hint_in, best);
    LMZ_CLK(3);
    if (MODE != 2 && !live && !ok) {                           // a dead row never asks for the enumeration; nothing of `best` is used
        best.cost = 0; best.id = 0; best.m = -1; best.H0 = best.H1 = 0; best.i1 = best.i2 = best.j1 = best.j2 = -1;
        best.l1 = best.l2 = best.g1 = best.g2 = 0;
        ok = true;
    }
    unsigned long long need = __ballot(!ok);                   // rows that need the enumeration (wave-uniform from here)
    if (MODE == 2) {
        need = __ballot(live && !ok);                            // the polygon row of the slot, or the circle rows whose remembered case was not accepted
        if (!live) {                                            // idle rows: nothing of `best` is used below
            best.cost = 0; best.id = 0; best.m = -1; best.H0 = best.H1 = 0; best.i1 = best.i2 = best.j1 = best.j2 = -1;
            best.l1 = best.l2 = best.g1 = best.g2 = 0;
        }
    }
#ifdef RDA_LMZ_STATS
    if (lane == 0) {
        const int nf = __popcll(need) >> 4;
        if (block == 0 && wv == 0) atomicAdd(&d.ctrl->lmz_stat[0], 1u);
        atomicAdd(&d.ctrl->lmz_stat[1], (unsigned)nf); atomicAdd(&d.ctrl->lmz_stat[2 + nf], 1u);
    }
#endif
    bool defer = false;
    if (MODE == 1) {
        defer = ((need >> (16 * row)) & 1) != 0 && !bad;
        if ((need >> (16 * row)) & 1) {     // nothing of `best` is used below (deferred, or a non-finite row): a harmless value
            best.cost = 0; best.id = 0; best.m = -1; best.H0 = best.H1 = 0; best.i1 = best.i2 = best.j1 = best.j2 = -1;
            best.l1 = best.l2 = best.g1 = best.g2 = 0;
        }
        if (defer && gl == 0 && live) {
            if (P.norm2) d.wl[d.wl_cap - 1 - atomicAdd(&d.ctrl->wlc_count, 1)] = t * GS * d.J + nl;      // circle rows: from the back (see the work-list form)
            else d.wl[atomicAdd(&d.ctrl->wl_count, 1)] = t * GS * d.J + nl;
        }
        need = 0;
    }
    if (MODE == 0) {
        // The rows of the WORKGROUP whose certificate failed are shared out over its waves: the launch time of a small grid is its
        // slowest wave, and that was a wave with two failing rows (2 - 3 % of the rows fail; ~13 us common path + ~6 us per
        // enumeration served one after the other) - with the list in LDS a workgroup's two waves take one each.  A row's result
        // does not depend on which wave enumerated it (same function on the same slab).
        struct Prm { int norm2; double px, py, cs, sn, xi0, xi1, kappa0; };
        __shared__ int nfail; __shared__ unsigned char flist[GS]; __shared__ Prm prm[GS]; __shared__ lmz::Sol sol[GS];
        if (threadIdx.x == 0) nfail = 0;
        __syncthreads();
        const bool mine = ((need >> (16 * row)) & 1) != 0;
        if (mine && gl == 0) {
            const int rid = wv * 4 + row; flist[atomicAdd(&nfail, 1)] = (unsigned char)rid;
            Prm &q = prm[rid]; q.norm2 = P.norm2; q.px = P.px; q.py = P.py; q.cs = P.cs; q.sn = P.sn; q.xi0 = P.xi0; q.xi1 = P.xi1; q.kappa0 = P.kappa0;
        }
        __syncthreads();
        const int nf = nfail;
        for (int i = wv; i < nf; i += WPB) {
            const int rid = flist[i];
            lmz::Params Pg;
            { const Prm &q = prm[rid]; Pg.E = E; Pg.R = R; Pg.norm2 = q.norm2; Pg.px = q.px; Pg.py = q.py; Pg.cs = q.cs; Pg.sn = q.sn; Pg.xi0 = q.xi0; Pg.xi1 = q.xi1;
              Pg.kappa0 = q.kappa0; Pg.ro2 = P.ro2; Pg.delta = P.delta; }
            lmz::Sol bg;
            lmz::solve_wave(wl[rid], rb, Pg, lane, bg);
            if (lane == 0) sol[rid] = bg;
        }
        __syncthreads();
        if (mine) best = sol[wv * 4 + row];
        need = 0;
#ifdef RDA_LMZ_CLK
        clk_enum = nf > 0;
        if (mine && gl == 0 && live && g_lmz_faillog) {
            const int k = atomicAdd(&g_lmz_faillog[0], 1);
            if (k < 200000) { g_lmz_faillog[1 + 3 * k] = hint_in; g_lmz_faillog[2 + 3 * k] = best.id >> 1; g_lmz_faillog[3 + 3 * k] = P.norm2; }
        }
#endif
    }
    LMZ_CLK(4);
    while (need) {
        const int g = (__ffsll((long long)need) - 1) >> 4;
        need &= ~(0xffffull << (16 * g));
        lmz::Params Pg;
        const int src = 16 * g;
        Pg.E = E; Pg.R = R; Pg.norm2 = __shfl(P.norm2, src, 64);
        Pg.px = __shfl(P.px, src, 64); Pg.py = __shfl(P.py, src, 64); Pg.cs = __shfl(P.cs, src, 64); Pg.sn = __shfl(P.sn, src, 64);
        Pg.xi0 = __shfl(P.xi0, src, 64); Pg.xi1 = __shfl(P.xi1, src, 64); Pg.kappa0 = __shfl(P.kappa0, src, 64);
        Pg.ro2 = P.ro2; Pg.delta = P.delta;
        lmz::Sol bg;
        lmz::solve_wave(wl[wv * 4 + g], rb, Pg, lane, bg);
        if (row == g) best = bg;
    }
    if (gl == 0 && live && !defer) {      // (single-ego form: hint_key's read of the slot's source was a trip to memory in front of the central normal)
        if (LANES) hint_write_src(d, hpar, n, t, ey.src, best.id >> 1); else hint_write(d, hpar, n, t, best.id >> 1);
    }
    LMZ_SUB(3);
#ifdef RDA_LMZ_CLK
    {
        long long cn[5]; for (int q = 0; q < 5; ++q) cn[q] = 0;
        if (d.centre) lmz::central_normal_wave<16, LANES>(W, rb, P, lane, best, cn);
        // (a row that leaves early has no later stamps: a stamp counts for the wave only when its first lane took it)
        if (MODE == 0 && clk_slot && (threadIdx.x & 63) == 0) { long long pv = clk_sub; for (int q = 0; q < 5; ++q) if (cn[q]) { clk_slot[20 + q] += (unsigned long long)(cn[q] - pv); pv = cn[q]; } }
    }
#else
    if (d.centre) lmz::central_normal_wave<16, LANES>(W, rb, P, lane, best);
#endif
    LMZ_CLK(5);
    bad = bad || !(isfinite(best.cost) && isfinite(best.m) && isfinite(best.H0) && isfinite(best.H1));      // uniform over the row
    // ---- fused dual / residual updates (every lane of the row holds the row's winner) ----------------
    const double znew = (d.c.accelerated ? 0.5 : 1.0) * (best.m > 0 ? best.m : 0.0);     // tie-break T2
    double res = 0;
    const bool wr = live && !bad && !defer;
    if (LANES) {
        // one selected value through one selected address: as three branches the stores fetched their three base pointers one after the other
        const bool isl = gl < E, ism = !isl && gl < E + R, isz = gl == E + R;
        const double vlam = lmz::lam_of(best, P.norm2, gl), vmu = lmz::mu_of(best, gl - E);
        const double v = isl ? vlam : (ism ? vmu : znew), old = isz ? ey.zold : prev;
        res = (isl || ism || isz) ? (v - old) * (v - old) : 0.0;
        double *const p = isl ? &d.lam[o * E + gl] : (ism ? &d.mu[o * R + gl - E] : &d.z[zi]);
        if (wr && gl <= E + R) *p = v;
    } else
    if (gl < E) {
        double v = lmz::lam_of(best, P.norm2, gl);
        res = (v - prev) * (v - prev); if (wr) d.lam[o * E + gl] = v;
    } else if (gl < E + R) {
        int j = gl - E;
        double v = lmz::mu_of(best, j);
        res = (v - prev) * (v - prev); if (wr) d.mu[o * R + j] = v;
    } else if (gl == E + R) {
        const double old = MODE == 0 ? ey.zold : d.z[zi];
        res = (znew - old) * (znew - old); if (wr) d.z[zi] = znew;
    }
    LMZ_SUB(9);
    // the row's dual residual: the xor butterfly (8, 4, 2, 1) on DPP row operations instead of four dependent LDS-crossbar permutes.  A rotation by 8 IS xor 8;
    // behind it the partial sums have period 8 along the row, so the rotation by 4 hands every lane the value of lane ^ 4; xor 2 and xor 1 are quad
    // permutations.  Every lane adds the same two operands as before.
    if (LANES) {
        res += lmz::dpp_mov0_f64<0x128>(res);      // row_ror:8
        res += lmz::dpp_mov0_f64<0x124>(res);      // row_ror:4
        res += lmz::dpp_mov0_f64<0x4E>(res);       // quad_perm [2, 3, 0, 1]
        res += lmz::dpp_mov0_f64<0xB1>(res);       // quad_perm [1, 0, 3, 2]
    } else {
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) res += __shfl_xor(res, off, 16);
    }
    LMZ_SUB(10);
    // The row's six sums a = A'lam (2), b'lam, h'mu, G'mu (2) on the row's lanes.  They were one lane's loops over the E and the R rows, an LDS read and the
    // lam_of / mu_of selects per trip in front of three dependent fused multiply-adds, while the other lanes of the row waited.  Now lane gl holds the
    // operands of element E-1-gl of the lam sums and of element R-1-gl of the mu sums, and the partial sums travel DOWN the row (row_shl:1: a lane reads
    // its upper neighbour): lane E-1 adds element 0 to the +0 of lane E, lane E-2 element 1 to that, ... and after E steps lane 0 holds
    // fma(v[E-1], c[E-1], ... fma(v[0], c[0], +0)) - the operands, the order and the contraction of the loop.  Lanes beyond the sum hold v = c = +0 and
    // stay +0 (lane 15 reads +0 from beyond the row), a lane that has its final value recomputes it, so max(E, R) steps serve both families.
    double ax = 0, ay = 0, bl = 0, mh = 0, gx = 0, gy = 0;
    if (LANES) {
        const bool le = gl < E, lr = gl < R;
        const int ie = le ? E - 1 - gl : 0, je = lr ? R - 1 - gl : 0;
        // (the six operands are read whatever the lane, from a clamped index, and zeroed by a select: as `le ? W.A[ie][0] : 0.0` each read was a branch of its own)
        const double a0r = W.A[ie][0], a1r = W.A[ie][1], bbr = W.b[ie], hhr = rb.h[je], g0r = rb.G[je][0], g1r = rb.G[je][1];
        const double vl = le ? lmz::lam_of(best, P.norm2, ie) : 0.0, vm = lr ? lmz::mu_of(best, je) : 0.0;
        const double a0 = le ? a0r : 0.0, a1 = le ? a1r : 0.0, bb = le ? bbr : 0.0, hh = lr ? hhr : 0.0, g0 = lr ? g0r : 0.0, g1 = lr ? g1r : 0.0;
        const int ns = E > R ? E : R;
        for (int s = 0; s < ns; ++s) {
            ax = vl * a0 + lmz::dpp_mov0_f64<0x101>(ax); ay = vl * a1 + lmz::dpp_mov0_f64<0x101>(ay); bl = vl * bb + lmz::dpp_mov0_f64<0x101>(bl);
            mh = vm * hh + lmz::dpp_mov0_f64<0x101>(mh); gx = vm * g0 + lmz::dpp_mov0_f64<0x101>(gx); gy = vm * g1 + lmz::dpp_mov0_f64<0x101>(gy);
        }
        LMZ_SUB(11);
    }
    if (gl == 0) {
        const int k = t * d.Nloc + nl;
        RowOut ro;
        bool have = false;
        if (live && bad) {
            ro = failed_row(d, k); have = true;
            store_row(d, k, ro);
            if (LANES) hint_write_src(d, hpar, n, t, ey.src, -1); else hint_write(d, hpar, n, t, -1);
            atomicAdd(&d.ctrl->lmz_fail, 1);
        } else if (wr) {
            if (!LANES) {                 // one lane's loops over the E and the R rows
                for (int i = 0; i < E; ++i) {
                    double v = lmz::lam_of(best, P.norm2, i);
                    ax += v * W.A[i][0]; ay += v * W.A[i][1]; bl += v * W.b[i];
                }
                for (int j = 0; j < R; ++j) {
                    double v = lmz::mu_of(best, j);
                    mh += v * rb.h[j]; gx += v * rb.G[j][0]; gy += v * rb.G[j][1];
                }
                LMZ_SUB(11);
            }
            const double hx = gx + P.cs * ax + P.sn * ay, hy = gy - P.sn * ax + P.cs * ay;      // Hm, :682
            const double xin0 = P.xi0 + hx, xin1 = P.xi1 + hy;                                  // :683
            d.xi[2 * o] = xin0; d.xi[2 * o + 1] = xin1;
            const double im = ax * P.px + ay * P.py - bl - mh;                                  // :659
            const double zetan = zeta + im - dbar - znew;                                       // :666
            d.zeta[zi] = zetan;
            ro.ax = ax; ro.ay = ay; ro.bl = bl; ro.c3 = mh + znew - zetan; ro.c4 = gx + xin0; ro.c5 = gy + xin1;
            ro.res = res; ro.hh = hx * hx + hy * hy; have = true;
            store_row(d, k, ro);
            LMZ_SUB(12);
        }
        if (MODE == 0) {                  // this row's record for the block partial (a dead slot: zeros)
            double *rv = rowv[wv * 4 + row];
            if (have) row_record(rv, d, ro, px0, py0);
            else { rv[0] = rv[1] = rv[2] = rv[3] = rv[4] = rv[5] = 0.0; }
        }
    }
    LMZ_CLK(6);
    if (MODE == 0) {
        __syncthreads();
        LMZ_SUB(13);
        block_partial(d, tb, jb, rowv, threadIdx.x);
        if (block == 0 && threadIdx.x == 0) d.ctrl->pose_ok = 1;
    }
    LMZ_CLK(7);
#ifdef RDA_LMZ_CLK
    if (MODE == 0 && clk_slot && (threadIdx.x & 63) == 0) {
        const unsigned long long tot = (unsigned long long)(clock64() - clk_in);
        clk_slot[8] += 1; clk_slot[9] += tot; if (tot > clk_slot[10]) clk_slot[10] = tot;
        clk_slot[13] = clk_wall_in; clk_slot[14] = (unsigned long long)wall_clock64();      // (last launch) start / end on the device-wide 100 MHz clock
        if (clk_enum) { clk_slot[11] += 1; clk_slot[12] += tot; }
    }
#endif
    }
#undef LMZ_CLK
#undef LMZ_SUB
}

// two builds: all registers and one wave per SIMD (no spills: the shorter critical path a single ego wants), or two
// waves per SIMD with a few spilled registers (more sub-problems in flight: what a full chip wants)
__global__ __launch_bounds__(64 * GS / 4) void k_lammuz_rows(Dev d, int it, Fin fin) { warm_kernargs<sizeof(Dev) + sizeof(int) + sizeof(Fin)>(); lammuz_body_rows<0, true>(d, blockIdx.x, gridDim.x, it, fin); }
__global__ __launch_bounds__(64 * GS / 4, 2) void k_lammuz_rows_dense(Dev d, int it, Fin fin) { lammuz_body_rows<0>(d, blockIdx.x, gridDim.x, it, fin); }
__global__ __launch_bounds__(64 * GS / 4, 3) void k_lammuz_rows_fast(Dev d, int it) { lammuz_body_rows<1>(d, blockIdx.x, gridDim.x, it, Fin{}); }
// (measured: the common path with four waves per SIMD and 31 spilled registers is 9 % slower.  Round 4, same-box A/B (tools/experiments/ab_so.sh): the common
// path at TWO waves per SIMD - no scratch spills - is 9 % slower at N = 2000 and 20 % slower for the 64-ego C5 fleet than at three waves with its 53 spilled
// registers, so it stays at three; the work list at ONE wave per SIMD (no spills; round 2-3: two waves, 91 spilled registers) is +1 % / +-0 %: kept)
__global__ __launch_bounds__(64 * GS / 4, 1) void k_lammuz_enum(Dev d, int it) { lammuz_body_rows<2>(d, blockIdx.x, gridDim.x, it, Fin{}); }

// Block partials from the STORED terms - the same row_term, the same row order as mode 0 of the packed kernel forms them in flight - and
// the tail of the step.  Runs behind every LamMuZ form that leaves its rows to more than one workgroup or launch (split launch, one
// sub-problem per wave, the per-thread interior-point kernel), after the no-obstacle launch (quirk Q9 edits terms) and whenever the
// host rewrites terms (rda_set_state, rda_reset, rda_shard_config).  One GS-slot block per GS threads, 256 / GS blocks per workgroup;
// it < 0: no tail.
constexpr int FPB = lmzplan::FPB;         // block partials per workgroup of k_lmz_finalize
__device__ __forceinline__ void finalize_body(const Dev &d, const int block, const int nblocks, const int it, const Fin &fin)
{
#pragma clang fp contract(on)
    __shared__ double rowv[FPB][GS][6];
    if (it >= 0 && d.ctrl->stop) return;
    const int T = d.c.T, g = threadIdx.x / GS, row = threadIdx.x % GS;
    const int B = block * FPB + g, t = B / d.J, j = B - t * d.J, nl = GS * j + row;
    double *rv = rowv[g][row];
    if (B < T * d.J && nl < d.Nlive) {
        const int k = t * d.Nloc + nl;
        RowOut ro; ro.ax = coef_arr(d, d.rank, 0)[k]; ro.ay = coef_arr(d, d.rank, 1)[k]; ro.bl = coef_arr(d, d.rank, 2)[k];
        ro.c3 = coef_arr(d, d.rank, 3)[k]; ro.c4 = coef_arr(d, d.rank, 4)[k]; ro.c5 = coef_arr(d, d.rank, 5)[k];
        ro.res = coef_arr(d, d.rank, 6)[k]; ro.hh = coef_arr(d, d.rank, 7)[k];
        row_record(rv, d, ro, d.pose[4 * t], d.pose[4 * t + 1]);
    } else { rv[0] = rv[1] = rv[2] = rv[3] = rv[4] = rv[5] = 0.0; }
    __syncthreads();
    if (B < T * d.J) block_partial(d, t, j, rowv[g], row);
    if (block == 0 && threadIdx.x == 0) d.ctrl->pose_ok = 1;
}
__global__ __launch_bounds__(256) void k_lmz_finalize(Dev d, int it, Fin fin) { finalize_body(d, blockIdx.x, gridDim.x, it, fin); }

// K1, interior-point variant (lammuz_cp_device.h): one (obstacle, stage) sub-problem per thread, same fused dual / residual
// updates as lammuz_body.  A solve that does not end on the central path keeps the previous duals of its stage and makes the
// residual inf (rda_solver.py:781-793); unlike non-finite data (where everything of the stage is left alone) the xi / zeta
// updates then run with the kept duals, as the reference's do.
template <int NX, int MX> __device__ __forceinline__ void lammuz_cp_body(const Dev &d, const int block)
{
    const int T = d.c.T, E = d.c.E, R = d.c.R;
    if (d.ctrl->stop) return;
    const int w = block * blockDim.x + threadIdx.x;
    if (d.obstacle_num == 0) {          // quirk Q9, as in lammuz_body
        if (w < T && d.rank == (d.c.N - 1) / d.Nloc) {
            const int i = w * d.Nloc + (d.c.N - 1) % d.Nloc;
            coef_arr(d, d.rank, 0)[i] = 0; coef_arr(d, d.rank, 1)[i] = 0; coef_arr(d, d.rank, 2)[i] = 0;
            coef_arr(d, d.rank, 8)[i] = coef_arr(d, d.rank, 3)[i];
        }
        return;
    }
    if (w >= d.Nlive * T) return;
    const int nl = w % d.Nlive, t = w / d.Nlive, n = d.rank * d.Nloc + nl;
    const size_t ao = ((size_t)n * d.nt + (d.nt > 1 ? t + 1 : 0)) * E, o = drow(d, n, t + 1), zi = drow(d, n, t);
    const int k = t * d.Nloc + nl;
    double A[16], b[8];
    for (int i = 0; i < 2 * E; ++i) A[i] = d.A[ao * 2 + i];
    for (int i = 0; i < E; ++i) b[i] = d.b[ao + i];
    cpq::Problem p;
    p.E = E; p.R = R; p.cone_norm2 = d.cone[n]; p.robot_norm2 = d.c.robot_norm2; p.accelerated = d.c.accelerated;
    p.A = A; p.b = b; p.G = d.G; p.h = d.h;
    const double *ps = d.pose + 4 * t;                        // position of column t+1, heading of column t (quirk Q1)
    p.px = ps[0]; p.py = ps[1]; p.cs = ps[2]; p.sn = ps[3];
    p.xi0 = d.xi[2 * o]; p.xi1 = d.xi[2 * o + 1];
    const double zeta = d.zeta[zi], dbar = d.dis[t];
    p.kappa0 = zeta - dbar; p.ro2 = d.c.ro2; p.mu_target = d.lmz_mu;
    bool finite_in = isfinite(p.px + p.py + p.cs + p.sn + p.xi0 + p.xi1 + p.kappa0);
    for (int i = 0; i < 2 * E; ++i) finite_in = finite_in && isfinite(A[i]);
    for (int i = 0; i < E; ++i) finite_in = finite_in && isfinite(b[i]);
    if (!finite_in) {
        store_row(d, k, failed_row(d, k));
        atomicAdd(&d.ctrl->lmz_fail, 1);
        return;
    }
    cpq::Result rs;
    {
        cpq::Solver<NX, MX> sv;
        sv.run(p, rs);
    }
    const bool fail = rs.status != 0;
    double res = 0, lam[8], mu[8], znew;
    for (int i = 0; i < E; ++i) { const double old = d.lam[o * E + i]; lam[i] = fail ? old : rs.lam[i]; res += (lam[i] - old) * (lam[i] - old); }
    for (int j = 0; j < R; ++j) { const double old = d.mu[o * R + j]; mu[j] = fail ? old : rs.mu[j]; res += (mu[j] - old) * (mu[j] - old); }
    { const double old = d.z[zi]; znew = fail ? old : rs.z; res += (znew - old) * (znew - old); }
    if (!fail) {
        for (int i = 0; i < E; ++i) d.lam[o * E + i] = lam[i];
        for (int j = 0; j < R; ++j) d.mu[o * R + j] = mu[j];
        d.z[zi] = znew;
    } else atomicAdd(&d.ctrl->lmz_fail, 1);
    double ax = 0, ay = 0, bl = 0, mh = 0, gx = 0, gy = 0;
    for (int i = 0; i < E; ++i) { ax += lam[i] * A[2 * i]; ay += lam[i] * A[2 * i + 1]; bl += lam[i] * b[i]; }
    for (int j = 0; j < R; ++j) { mh += mu[j] * d.h[j]; gx += mu[j] * d.G[2 * j]; gy += mu[j] * d.G[2 * j + 1]; }
    const double hx = gx + p.cs * ax + p.sn * ay, hy = gy - p.sn * ax + p.cs * ay;      // Hm, :682
    const double xin0 = p.xi0 + hx, xin1 = p.xi1 + hy;                                  // :683
    d.xi[2 * o] = xin0; d.xi[2 * o + 1] = xin1;
    const double im = ax * p.px + ay * p.py - bl - mh;                                  // :659
    const double zetan = zeta + im - dbar - znew;                                       // :666
    d.zeta[zi] = zetan;
    RowOut ro; ro.ax = ax; ro.ay = ay; ro.bl = bl; ro.c3 = mh + znew - zetan; ro.c4 = gx + xin0; ro.c5 = gy + xin1;
    ro.res = fail ? INFINITY : res; ro.hh = hx * hx + hy * hy;
    store_row(d, k, ro);
}
__global__ __launch_bounds__(64) void k_lammuz_cp_small(Dev d) { lammuz_cp_body<16, 24>(d, blockIdx.x); }      // E, R <= 4
__global__ __launch_bounds__(64) void k_lammuz_cp_large(Dev d) { lammuz_cp_body<24, 36>(d, blockIdx.x); }      // E, R <= 8

// K1, interior-point variant, ROW-PARALLEL (lammuz_ip_device.h): one sub-problem per 16-lane row, lane i = variable i of the cone
// program, GS rows per workgroup in the launch order and with the epilogue of the packed enumeration kernel - duals, condensed terms,
// block partial, tail of the step all in this ONE launch.  A solve that does not reach the central path keeps the previous duals of
// its stage and makes the residual inf (rda_solver.py:781-793); unlike non-finite data (where everything of the stage is left alone)
// the xi / zeta updates then run with the kept duals, as the reference's do.
__device__ __forceinline__ void lammuz_ip_body(const Dev &d, const int block, const int it, const Fin &fin)
{
    constexpr int WPB = GS / 4;
    __shared__ lmz::WaveLDS wl[GS];
    __shared__ lmz::RobotLDS rb;
    __shared__ double rowv[GS][6];
    typedef rip::DevLanes L;
    const int E = d.c.E, R = d.c.R;
    if (d.ctrl->stop) return;
    int t, jb; block_of(d, block, t, jb);
    if (t < 0) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, row = lane >> 4, gl = lane & 15;
    for (int i = threadIdx.x; i < 2 * R; i += 64 * WPB) rb.G[i >> 1][i & 1] = d.G[i];
    for (int i = threadIdx.x; i < R; i += 64 * WPB) rb.h[i] = d.h[i];
    int nl = jb * GS + wv * 4 + row;
    const bool live = nl < d.Nlive;
    if (!live) nl = 0;
    const int n = d.rank * d.Nloc + nl;
    lmz::WaveLDS &W = wl[wv * 4 + row];
    const size_t ao = ((size_t)n * d.nt + (d.nt > 1 ? t + 1 : 0)) * E;
    if (gl < 2 * E) W.A[gl >> 1][gl & 1] = d.A[ao * 2 + gl];
    if (gl < E) W.b[gl] = d.b[ao + gl];
    __syncthreads();
    rip::Problem p;
    p.E = E; p.R = R; p.cone_norm2 = d.cone[n]; p.robot_norm2 = d.c.robot_norm2; p.accelerated = d.c.accelerated;
    p.A = &W.A[0][0]; p.b = W.b; p.G = &rb.G[0][0]; p.h = rb.h;
    const double *ps = d.pose + 4 * t;                        // position of column t+1, cos / sin of the heading of column t (quirk Q1)
    p.px = ps[0]; p.py = ps[1]; p.cs = ps[2]; p.sn = ps[3];
    const size_t o = drow(d, n, t + 1), zi = drow(d, n, t);
    p.xi0 = d.xi[2 * o]; p.xi1 = d.xi[2 * o + 1];
    const double zeta = d.zeta[zi], dbar = d.dis[t];
    p.kappa0 = zeta - dbar; p.ro2 = d.c.ro2; p.mu_target = d.lmz_mu;
    double prev = 0.0;                                        // this lane's dual entry before the solve: lam | mu | z
    if (gl < E) prev = d.lam[o * E + gl];
    else if (gl < E + R) prev = d.mu[o * R + gl - E];
    else if (gl == E + R) prev = d.z[zi];
    bool bad = !isfinite(p.px + p.py + p.cs + p.sn + p.xi0 + p.xi1 + p.kappa0);
    if (gl < 2 * E) bad = bad || !isfinite(W.A[gl >> 1][gl & 1]);
    if (gl < E) bad = bad || !isfinite(W.b[gl]);
    bad = ((__ballot(bad) >> (16 * row)) & 0xffffull) != 0;                      // uniform over the row
    int status = 2;
    double v = prev;
    double *const wst = d.ipw ? d.ipw + (zi * 5) * 16 : nullptr;      // this sub-problem's kept central-path point
    if (!bad) {
        rip::Solver<L> sv;
        sv.build(p);
        const bool warm = wst && d.ipf[zi] != 0;                      // (uniform over the row)
        if (warm) sv.load(wst[gl], wst[16 + gl], wst[32 + gl], wst[48 + gl], wst[64 + gl]);
        status = sv.run(p.mu_target, warm);
        if (wst && live) {
            if (status == 0) { wst[gl] = sv.x; wst[16 + gl] = sv.s.d; wst[32 + gl] = sv.z.d; wst[48 + gl] = sv.s.g; wst[64 + gl] = sv.z.g; }
            if (gl == 0) d.ipf[zi] = status == 0 ? 1 : 0;
        }
        if (status == 0) {
            v = sv.x;
            if (gl < E) { if (!p.cone_norm2 && v < 0) v = 0; }
            else if (gl < E + R) { if (!p.robot_norm2 && v < 0) v = 0; }
            else if (gl == E + R) { if (!(v > 0)) v = 0; }
            const bool fin_ok = gl > E + R || isfinite(v);
            if (((__ballot(!fin_ok) >> (16 * row)) & 0xffffull) != 0) status = 2;
        }
    }
    const bool fail = status != 0;                             // (row-uniform) previous duals kept
    if (fail) v = prev;
    const double dv = gl <= E + R ? v - prev : 0.0;
    const double res = L::rsum(dv * dv);
    const bool wr = live && !bad;
    if (wr && !fail) {
        if (gl < E) d.lam[o * E + gl] = v;
        else if (gl < E + R) d.mu[o * R + gl - E] = v;
        else if (gl == E + R) d.z[zi] = v;
    }
    // lam'A, lam'b, mu'h, G'mu with the duals in force (new, or kept): row reductions of the lanes' products
    const double la = gl < E ? v : 0.0, ma = (gl >= E && gl < E + R) ? v : 0.0;
    const int ie = gl < E ? gl : 0, jr = (gl >= E && gl < E + R) ? gl - E : 0;
    const double ax = L::rsum(la * W.A[ie][0]), ay = L::rsum(la * W.A[ie][1]), bl = L::rsum(la * W.b[ie]);
    const double mh = L::rsum(ma * rb.h[jr]), gx = L::rsum(ma * rb.G[jr][0]), gy = L::rsum(ma * rb.G[jr][1]);
    const double znew = L::bc<0>(__shfl(v, (lane & 48) + E + R, 64));           // lane E+R of the row
    if (gl == 0) {
        const int k = t * d.Nloc + nl;
        RowOut ro;
        bool have = false;
        if (live && bad) {
            ro = failed_row(d, k); have = true;
            store_row(d, k, ro);
            atomicAdd(&d.ctrl->lmz_fail, 1);
        } else if (wr) {
            const double hx = gx + p.cs * ax + p.sn * ay, hy = gy - p.sn * ax + p.cs * ay;      // Hm, :682
            const double xin0 = p.xi0 + hx, xin1 = p.xi1 + hy;                                  // :683
            d.xi[2 * o] = xin0; d.xi[2 * o + 1] = xin1;
            const double im = ax * p.px + ay * p.py - bl - mh;                                  // :659
            const double zetan = zeta + im - dbar - znew;                                       // :666
            d.zeta[zi] = zetan;
            ro.ax = ax; ro.ay = ay; ro.bl = bl; ro.c3 = mh + znew - zetan; ro.c4 = gx + xin0; ro.c5 = gy + xin1;
            ro.res = fail ? INFINITY : res; ro.hh = hx * hx + hy * hy; have = true;
            store_row(d, k, ro);
            if (fail) atomicAdd(&d.ctrl->lmz_fail, 1);
        }
        double *rv = rowv[wv * 4 + row];
        if (have) row_record(rv, d, ro, p.px, p.py);
        else { rv[0] = rv[1] = rv[2] = rv[3] = rv[4] = rv[5] = 0.0; }
    }
    __syncthreads();
    block_partial(d, t, jb, rowv, threadIdx.x);
    if (block == 0 && threadIdx.x == 0) d.ctrl->pose_ok = 1;
}
__global__ __launch_bounds__(64 * GS / 4) void k_lammuz_ip(Dev d, int it, Fin fin) { lammuz_ip_body(d, blockIdx.x, it, fin); }

struct RobotCands { unsigned char muc[40]; int nmv; double rv[28][2]; int nrv; int centre; };

// pure-function batch hook (rda_lammuz_batch)
__global__ __launch_bounds__(256) void k_lammuz_batch(int B, int E, int R, const double *A, const double *b, const int *cone,
                                                      const double *p, const double *phi, const double *G, const double *h,
                                                      const double *xi, const double *zeta, const double *dbar, double ro2,
                                                      double delta, int accelerated, double *lam, double *mu, double *z, double *cmh, long long *prof, RobotCands rc)
{
    __shared__ lmz::WaveLDS wl[4];
    __shared__ lmz::RobotLDS rb;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long t_begin = prof ? clock64() : 0;
    if (threadIdx.x < 2 * R) rb.G[threadIdx.x >> 1][threadIdx.x & 1] = G[threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x < 64 + R) rb.h[threadIdx.x - 64] = h[threadIdx.x - 64];
    if (threadIdx.x >= 128 && threadIdx.x < 128 + 40) rb.muc[threadIdx.x - 128] = rc.muc[threadIdx.x - 128];
    if (threadIdx.x >= 192 && threadIdx.x < 192 + 56) (&rb.rv[0][0])[threadIdx.x - 192] = (&rc.rv[0][0])[threadIdx.x - 192];
    if (threadIdx.x == 255) { rb.nmv = rc.nmv; rb.nrv = rc.nrv; }
    const int w = blockIdx.x * 4 + wv;
    const bool live = w < B;
    const int k = live ? w : 0;
    lmz::WaveLDS &W = wl[wv];
    if (lane < 2 * E) W.A[lane >> 1][lane & 1] = A[(size_t)k * E * 2 + lane];
    if (lane < E) W.b[lane] = b[(size_t)k * E + lane];
    __syncthreads();
    if (!live) return;
    lmz::Params P;
    P.E = E; P.R = R; P.norm2 = cone[k]; P.px = p[2 * k]; P.py = p[2 * k + 1];
    P.cs = cos(phi[k]); P.sn = sin(phi[k]); P.xi0 = xi[2 * k]; P.xi1 = xi[2 * k + 1];
    P.kappa0 = zeta[k] - dbar[k]; P.ro2 = ro2; P.delta = delta;
    P.prof = (prof && w == 0) ? prof : nullptr;               // wave 0 of the batch reports its phase cycles
    if (P.prof && lane == 0) prof[0] += clock64() - t_begin;
    lmz::Sol best;
    lmz::prepare_wave(W, P, lane);
    lmz::solve_wave(W, rb, P, lane, best);
    if (rc.centre) lmz::central_normal_wave<64>(W, rb, P, lane, best);
    if (P.prof && lane == 0) prof[7] += clock64() - t_begin;
    if (lane < E) lam[(size_t)k * E + lane] = lmz::lam_of(best, P.norm2, lane);
    else if (lane < E + R) mu[(size_t)k * R + lane - E] = lmz::mu_of(best, lane - E);
    else if (lane == E + R) {
        z[k] = (accelerated ? 0.5 : 1.0) * (best.m > 0 ? best.m : 0.0);
        cmh[4 * k] = best.cost; cmh[4 * k + 1] = best.m; cmh[4 * k + 2] = best.H0; cmh[4 * k + 3] = best.H1;
    }
}

// standalone su-solve hook
template <int TT> __global__ __launch_bounds__(su::NT) void k_su_hook(su::Args a) { su::Pre pre; su::Result res; su::solve<TT>(a, smem_su, pre, false, res); }

// horizons with a compile-time specialisation of the su kernel (BASELINE configs C1, north star, C5, C4); any other T runs the generic one
#define RDA_SU_DISPATCH(T, CALL) do { switch (T) { case 10: { constexpr int TT = 10; CALL; } break; case 20: { constexpr int TT = 20; CALL; } break; \
                                                    case 25: { constexpr int TT = 25; CALL; } break; case 30: { constexpr int TT = 30; CALL; } break; \
                                                    default: { constexpr int TT = 0; CALL; } break; } } while (0)

template <int TT> __global__ __launch_bounds__(su::NT) void k_su_tracked(Dev d, track::In in, double *path, int L, const double *nom_u, double *step,
                                                                          track::Out *out, unsigned long long seq);

// [N][T+1][2] / [N][T+1] <-> [T][N] transposes for the state accessors
__global__ void k_products_get(Dev d, double *a_lam, double *b_lam)
{
    const int T = d.c.T, N = d.c.N;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N * (T + 1); i += gridDim.x * blockDim.x) {
        int n = i / (T + 1), tt = i % (T + 1);
        double ax = 0, ay = 0, bl = 0;
        if (tt >= 1) { int r = n / d.Nloc, k = (tt - 1) * d.Nloc + (n - r * d.Nloc); ax = coef_arr(d, r, 0)[k]; ay = coef_arr(d, r, 1)[k]; bl = coef_arr(d, r, 2)[k]; }
        a_lam[2 * i] = ax; a_lam[2 * i + 1] = ay; b_lam[i] = bl;
    }
}
// rebuild every condensed term from the dual state (after rda_set_state); k_lmz_finalize then rebuilds the block partials
__global__ void k_products_set(Dev d, const double *a_lam, const double *b_lam)
{
    const int T = d.c.T, N = d.c.N, R = d.c.R;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N * T; i += gridDim.x * blockDim.x) {
        int n = i / T, t = i % T, r = n / d.Nloc, k = t * d.Nloc + (n - r * d.Nloc);
        const size_t o = drow(d, n, t + 1), zi = drow(d, n, t), oh = (size_t)n * (T + 1) + t + 1;     // oh: the caller's [N][T+1] layout
        if (a_lam) { coef_arr(d, r, 0)[k] = a_lam[2 * oh]; coef_arr(d, r, 1)[k] = a_lam[2 * oh + 1]; }
        if (b_lam) coef_arr(d, r, 2)[k] = b_lam[oh];
        double mh = 0, gx = 0, gy = 0;
        for (int j = 0; j < R; ++j) { double v = d.mu[o * R + j]; mh += v * d.h[j]; gx += v * d.G[2 * j]; gy += v * d.G[2 * j + 1]; }
        coef_arr(d, r, 3)[k] = mh + d.z[zi] - d.zeta[zi];
        coef_arr(d, r, 4)[k] = gx + d.xi[2 * o]; coef_arr(d, r, 5)[k] = gy + d.xi[2 * o + 1];
        coef_arr(d, r, 8)[k] = coef_arr(d, r, 2)[k] + coef_arr(d, r, 3)[k];
        coef_arr(d, r, 6)[k] = 0; coef_arr(d, r, 7)[k] = 0;
    }
}
// reset() of the reference (rda_solver.py:1060-1068) clears the lam'A / lam'b products only - the duals stay (quirk Q6)
__global__ void k_reset(Dev d)
{
    const int T = d.c.T;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d.P * d.Nloc * T; i += gridDim.x * blockDim.x) {     // incl. padding slots (zero anyway)
        int r = i / (d.Nloc * T), k = i % (d.Nloc * T);
        coef_arr(d, r, 0)[k] = 0; coef_arr(d, r, 1)[k] = 0; coef_arr(d, r, 2)[k] = 0;
        coef_arr(d, r, 8)[k] = coef_arr(d, r, 3)[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { d.ctrl->su_last = 99; d.ctrl->su_probe = 0; d.ctrl->prev_unconv = 0; d.ctrl->su_hardlike = 0; d.ctrl->spec_credit = 0; d.ctrl->land_hard = 0; d.ctrl->land_easy = 0; d.ctrl->land_rho_prev = 0; d.ctrl->blind_ok = 0; }      // solver history of the handle
    if (blockIdx.x == 0) for (int i = threadIdx.x; i < su::NC * T; i += blockDim.x) d.su_lam_keep[i] = 0;
    if (d.ipf) for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d.c.N * T; i += gridDim.x * blockDim.x) d.ipf[i] = 0;
}
// the same rebuild for every shard of a handle (the host rewrote terms: all P chunks are local copies)
__global__ __launch_bounds__(256) void k_lmz_finalize_all(Dev d)
{
    Dev q = d; q.rank = blockIdx.y; q.Nlive = d.c.N - q.rank * d.Nloc; if (q.Nlive > d.Nloc) q.Nlive = d.Nloc; if (q.Nlive < 0) q.Nlive = 0;
    finalize_body(q, blockIdx.x, gridDim.x, -1, Fin{});
}

// ---- rda_opts::duals_follow: the dual state moves with its obstacle when the device pipeline re-binds the slots ----------------------
// One workgroup per slot s.  map[s] = the slot that held, at the previous staging, the raw-scene entry slot s holds now (-1: it was in
// no slot -> initial duals, zeros).  Padding slots (s >= used: copies of the last obstacle, quirk Q3) keep their own state for as long
// as they stay padding slots.  The rows (stage, slot) of lam | mu | xi (T+1 stages) and z | zeta (T stages) of a slot that changes hands
// are gathered through the map into `tmp` (same layouts, one after the other) and written back by a second launch: the state never
// aliases itself.
__global__ __launch_bounds__(64) void k_follow_gather(Dev d, const int *now, int used, const int *prev, int prev_used, int *map, double *tmp)
{
    const int T = d.c.T, N = d.c.N, E = d.c.E, R = d.c.R, sl = blockIdx.x, lane = threadIdx.x;
    int m = -1;
    if (sl < used) {
        const int want = now[sl];
        for (int j = lane; j < prev_used; j += 64) if (prev[j] == want) m = j;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(m, off, 64); m = o > m ? o : m; }
    } else m = sl >= prev_used ? sl : -1;
    if (lane == 0) map[sl] = m;
    if (m == sl) return;                                      // the slot kept its obstacle
    const size_t rows = (size_t)(T + 1) * N;
    double *tl = tmp, *tm = tl + rows * E, *tx = tm + rows * R, *tz = tx + rows * 2, *tzt = tz + (size_t)T * N;
    for (int t = lane; t <= T; t += 64) {
        const size_t i = (size_t)t * N + sl, o = (size_t)t * N + (m >= 0 ? m : 0);
        for (int e = 0; e < E; ++e) tl[i * E + e] = m >= 0 ? d.lam[o * E + e] : 0.0;
        for (int j = 0; j < R; ++j) tm[i * R + j] = m >= 0 ? d.mu[o * R + j] : 0.0;
        tx[2 * i] = m >= 0 ? d.xi[2 * o] : 0.0; tx[2 * i + 1] = m >= 0 ? d.xi[2 * o + 1] : 0.0;
        if (t < T) { tz[i] = m >= 0 ? d.z[o] : 0.0; tzt[i] = m >= 0 ? d.zeta[o] : 0.0; }
    }
}
// map == nullptr: the first staging of a handle, only the binding is recorded
__global__ __launch_bounds__(64) void k_follow_back(Dev d, const int *map, const double *tmp, const int *now, int used, int *prev)
{
    const int T = d.c.T, N = d.c.N, E = d.c.E, R = d.c.R, sl = blockIdx.x, lane = threadIdx.x;
    if (lane == 0 && sl < used) prev[sl] = now[sl];
    if (!map || map[sl] == sl) return;
    const size_t rows = (size_t)(T + 1) * N;
    const double *tl = tmp, *tm = tl + rows * E, *tx = tm + rows * R, *tz = tx + rows * 2, *tzt = tz + (size_t)T * N;
    for (int t = lane; t <= T; t += 64) {
        const size_t i = (size_t)t * N + sl;
        for (int e = 0; e < E; ++e) d.lam[i * E + e] = tl[i * E + e];
        for (int j = 0; j < R; ++j) d.mu[i * R + j] = tm[i * R + j];
        d.xi[2 * i] = tx[2 * i]; d.xi[2 * i + 1] = tx[2 * i + 1];
        if (t < T) {
            d.z[i] = tz[i]; d.zeta[i] = tzt[i];
            if (d.ipf) d.ipf[i] = 0;                              // interior-point mode: the kept central point belonged to another obstacle (cold start)
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The two blocks every tick passes through: offsets and sizes in doubles, functions of the horizon T.  Host code takes them from here.
// Three device places spell the same layouts out and keep their own text (the code of the su kernels follows how their source is
// cut into functions): publish_result (result block), k_track and k_su_tracked (step block).  Whoever changes a block visits those three.
constexpr size_t traj_s(size_t T) { return 3 * (T + 1); }      // a state trajectory [3][T+1]
constexpr size_t traj_u(size_t T) { return 2 * T; }            // a control trajectory [2][T]
// Step block  nom_s [3(T+1)] | nom_u [2T] | ref [3(T+1)] | speed [1]:  rda_handle::step (its four parts on the device: step_views), and one per member in
// the fleet's `in`
constexpr size_t step_u(size_t T) { return traj_s(T); }
constexpr size_t step_ref(size_t T) { return step_u(T) + traj_u(T); }
constexpr size_t step_speed(size_t T) { return step_ref(T) + traj_s(T); }     // (= the block without its speed: what a tracked tick reads back)
constexpr size_t step_doubles(size_t T) { return step_speed(T) + 1; }
// Result block  u [2T] | s [3(T+1)] | rda_info | track::Out | non-convex count (long long) | sequence word:  rda_handle::res (ResultBlock: the parts
// are computed from these offsets, nowhere stored), identical on the device and in pinned memory.  The zero-copy form publishes the sequence word behind the mirrored block; the D2H form copies the block without it.
constexpr size_t res_s(size_t T) { return traj_u(T); }
constexpr size_t res_info(size_t T) { return res_s(T) + traj_s(T); }          // (= u | s alone: a member's block of the fleet's h_out / d_out)
constexpr size_t res_track(size_t T) { return res_info(T) + sizeof(rda_info) / sizeof(double); }
constexpr size_t res_nonconvex(size_t T) { return res_track(T) + sizeof(track::Out) / sizeof(double); }
constexpr size_t res_seq(size_t T) { return res_nonconvex(T) + 1; }
constexpr size_t res_copied_doubles(size_t T) { return res_seq(T); }
constexpr size_t res_doubles(size_t T) { return res_seq(T) + 1; }
static_assert(sizeof(rda_info) % sizeof(double) == 0 && sizeof(track::Out) % sizeof(double) == 0, "info and track output are whole doubles of the result block");
static_assert(res_doubles(1) == 2 * 1 + 3 * (1 + 1) + 8 && res_doubles(RDA_TMAX) == 2 * RDA_TMAX + 3 * (RDA_TMAX + 1) + 8, "the result block keeps its size (publish_result)");
static_assert(step_doubles(1) == 2 * 3 * (1 + 1) + 2 * 1 + 1 && step_doubles(RDA_TMAX) == 2 * 3 * (RDA_TMAX + 1) + 2 * RDA_TMAX + 1, "the step block keeps its size (k_track, k_su_tracked)");
static_assert(9 * su::NT >= track::LDS_DOUBLES, "TrackedRefWait runs track::run in the su solve's `part` scratch");

// The table sets of a handle, each a struct held by value.  Those that rda_create_opts makes hold views into rda_handle::mem; those made on first use and
// regrown on demand own their Group: a call builds the new set beside the old one and moves it in (H->x = std::move(built)); H->x = {} releases one.
struct StageBufs { double *A = nullptr, *b = nullptr; int *cone = nullptr; };     // pinned, N slots: the host-staged obstacles on their way to Dev::A, b, cone
struct ResultBlock {                      // the step path's result block on the device and its pinned mirror, which k_finish writes (see there) or a D2H copy
    hbuf::Pair<double> blk; size_t T = 0; unsigned long long seq = 0;
    double *out_u() const { return blk.d; }
    double *out_s() const { return blk.d + res_s(T); }
    rda_info *info() const { return (rda_info *)(blk.d + res_info(T)); }
    track::Out *track() const { return (track::Out *)(blk.d + res_track(T)); }
    const rda_info *h_info() const { return (const rda_info *)(blk.h + res_info(T)); }
    const track::Out *h_track() const { return (const track::Out *)(blk.h + res_track(T)); }
};
struct TraceSet {                         // rda_upload_trace: K steps' inputs and where their results go
    hbuf::Group g; int K = 0; double *s = nullptr, *u = nullptr, *ref = nullptr, *speed = nullptr, *out_u = nullptr, *out_s = nullptr; rda_info *info = nullptr;
    int alloc(size_t k, size_t ns, size_t nu)
    {
        K = (int)k;
        return (g.dev(&s, k * ns) | g.dev(&u, k * nu) | g.dev(&ref, k * ns) | g.dev(&speed, k) |
                g.dev(&out_u, k * nu) | g.dev(&out_s, k * ns) | g.dev(&info, k)) ? RDA_ERR_HIP : RDA_OK;
    }
};
struct PathSet { hbuf::Group g; double *d = nullptr; int len = 0; };     // device-side pre_process (rda_upload_path / rda_step_tracked): the path [len][3]
// the gear pieces of a path (rda_upload_path_pieces / rda_fleet_rollout_gears), apart from `path`: all P pieces in one buffer [off[P]][3], the first waypoint
// of every piece off [P+1] and its gear [P] on the device, the tables' host copies beside them
struct PieceSet {
    hbuf::Group g; double *buf = nullptr, *gear = nullptr; int *off = nullptr; int P = 0; std::vector<int> h_off; std::vector<double> h_gear;
    int alloc(int p, size_t total) { P = p; return (g.dev(&buf, 3 * total) | g.dev(&off, (size_t)p + 1) | g.dev(&gear, (size_t)p)) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return buf != nullptr; }
};
// The raw scene block, identical on the host (pinned) and on the device:  geom [n][E][2] | vel [n][2] | robot [2] | nonconvex counter (int, padded to 8
// bytes) | kind [n] | nvert [n].  Offsets in doubles, size in bytes.
struct SceneLayout { size_t vel, robot, nonconvex, ints, bytes; };
static SceneLayout scene_layout(size_t n, size_t E)
{
    SceneLayout l;
    l.vel = n * E * 2; l.robot = l.vel + n * 2; l.nonconvex = l.robot + 2; l.ints = l.nonconvex + 1; l.bytes = l.ints * sizeof(double) + 2 * n * sizeof(int);
    return l;
}
// device-side obstacle pipeline (rda_upload_scene): the raw scene and the kernels' scratch for up to `cap` obstacles | the pinned staging block (ONE H2D copy
// per upload).  Grown on demand, each on its own.
struct SceneDev {
    hbuf::Group g; double *blk = nullptr, *key = nullptr; int *sel = nullptr; int cap = 0;
    int alloc(int n, size_t E)
    {
        cap = n;
        return (g.dev(&blk, scene_layout((size_t)n, E).bytes / sizeof(double) + 1) | g.dev(&sel, (size_t)n) | g.dev(&key, (size_t)n)) ? RDA_ERR_HIP : RDA_OK;
    }
    bool have() const { return blk != nullptr; }
};
struct SceneHost {
    hbuf::Group g; char *blk = nullptr; size_t bytes = 0;
    int alloc(size_t n) { bytes = n; return g.pin(&blk, n) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return blk != nullptr; }
};
struct SceneSet {                         // args, n: the resident raw scene as the conversion kernels were last given it (n = 0: none)
    SceneDev dev; SceneHost host; scene::Args args; int n = 0;
    const void *peers_of = nullptr;       // the fleet whose rda_fleet_upload_scenes_peers staged it (its last B - 1 rows are peer rows), null: any other staging
};
// device-side lidar front end (rda_scan_boxes / rda_upload_scan), made by the first scan: the boxes of the last scan on the device; pinned, read / written by
// the kernel itself: the ranges, the two counters, and the host's copy of labels and boxes
struct LidarSet {
    hbuf::Group g; double *d_boxes = nullptr, *h_ranges = nullptr, *h_boxes = nullptr; int *h_count = nullptr, *h_labels = nullptr;
    int alloc()
    {
        return (g.dev(&d_boxes, (size_t)lidar::MAXB * 8) | g.pin(&h_ranges, (size_t)lidar::MAXB) | g.pin(&h_count, 2) | g.pin(&h_labels, (size_t)lidar::MAXB) |
                g.pin(&h_boxes, (size_t)lidar::MAXB * 8)) ? RDA_ERR_HIP : RDA_OK;
    }
    bool have() const { return d_boxes != nullptr; }
};
// rda_opts::duals_follow: slot -> raw-scene entry of the staging the dual state is arranged by (prev_used = -1: none yet), the map and the gathered rows
struct FollowSet { int *prev_sel = nullptr, *map = nullptr; double *tmp = nullptr; int prev_used = -1; };
struct ShardLink {                        // obstacle-shard exchange (RCCL, resolved lazily with dlopen so that single-GPU use has no rccl dependency)
    void *lib = nullptr, *comm = nullptr;
    int (*allgather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*comm_destroy)(void *) = nullptr;
    hbuf::Group g; unsigned long long *verdict = nullptr, vseq = 0;     // pinned early-stop verdict word of the su launches (made with the communicator)
};
struct OpenTick {                         // a tick opened by rda_tracked_begin and not yet closed by rda_tracked_finish
    int pending = 0, pending_scene = 0; const double *in_u = nullptr;
    int stages = 0, has_event = 0;        // see rda_tracked_begin
    int scene_on_s2 = 0;                  // in-tick scene staging runs beside the first su-problem (stream2, ev_tick, ev_scene)
};

// ------------------------------------------------------------------------------------------------
// A handle owns its device / pinned buffers through `mem`, `terms` and the table sets above (Dev holds views into the first two), its events and its
// streams: deleting a handle releases everything, the streams first (each is synchronised before it is destroyed).
struct rda_handle {
    Dev d;
    rda_opts opts;                        // sanitised (opts_sanitised): what the host code reads its switches from
    size_t su_lds = 0, su_trk_lds = 0; unsigned long long trk_seq = 0;
    char lmz_name[lmzplan::NAME_CAP] = "";      // what rda_lammuz_kernel last returned
    int admm_it = 0;         // host-driven ADMM pieces (rda_admm_*): the iteration rda_admm_su was last called with
    int stepped = 0;         // a step has been queued on this handle (sharded handles: rda_reset / rda_set_state are refused from then on)
    double scan_split = 0.0; // rda_set_scan_split: lidar::Args::split_tol of this handle's scans (0: one box per cluster)
    int timing = 0; size_t ev_used[4] = {0, 0, 0, 0};     // events in use of ev[]: 0 LamMuZ launches, 1 su launches, 2 shard all-gathers, 3 lidar scans (second stream)
    std::vector<double> rob_G, rob_h;     // the robot's G x <= h as handed to rda_create (host copy: the clearance's robot vertices are solved from it)
    hbuf::Group mem;                      // what lives as long as the handle: the Dev arrays (but coef / coefL) and the four sets below
    hbuf::Group terms;                    // Dev::coef, coefL (rda_shard_config replaces them)
    StageBufs stage; hbuf::Pair<double> step; ResultBlock res; FollowSet fol;      // step: the step block (step_doubles), pinned and on the device
    TraceSet trace; PathSet path; PieceSet pieces; SceneSet sc; LidarSet li; ShardLink shard; OpenTick tick;
    std::vector<hbuf::Event> ev[4];
    hbuf::Event ev_tick, ev_scene;
    hbuf::Stream stream, stream2;         // (last: destroyed first)
};

extern "C" const char *rda_strerror(int code)
{
    switch (code) {
        case RDA_OK: return "ok";
        case RDA_ERR_ARG: return "invalid argument";
        case RDA_ERR_UNSUPPORTED: return "unsupported configuration (E/R/T above the compiled limits, non-canonical circle obstacle, a norm2 robot or mixed LamMuZ modes in a fleet)";
        case RDA_ERR_HIP: return "HIP runtime error";
        case RDA_ERR_NODEVICE: return "no HIP device";
        default: return code > 0 ? "soft status" : "unknown error";
    }
}
extern "C" int rda_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
extern "C" int rda_set_device(int dev) { HIPCHK(hipSetDevice(dev)); return RDA_OK; }

// Solver options: the library defaults.  No environment is read here or anywhere else in the library
extern "C" void rda_opts_init(rda_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->lmz_mode = 0; o->tie_centre = 1; o->lmz_mu = 1e-6;
    o->su_tol[0] = 1e-9; o->su_tol[1] = 1e-10; o->su_tol[2] = 1e-11; o->su_tol_early[0] = o->su_tol_early[1] = o->su_tol_early[2] = 0; o->su_hard_warm[0] = 1.0; o->su_hard_warm[1] = 1e-3;
    o->lmz_warm = 1; o->lmz_rows = 1; o->lmz_dense_from = 256; o->lmz_split = 1; o->lmz_ip_rows = 1; o->lmz_ip_warm = 1;
    o->su_pre = 1; o->su_light = 1; o->su_warm_first = 1; o->su_warm_cap = 30; o->su_easy_max = 2; o->su_easy_nopred = 1;
    o->su_cold_from = 7; o->su_cold_probe = 8; o->zero_copy = 1; o->early_finish = 1; o->fuse_track = 1; o->su_prof = 0; o->su_split = 1; o->duals_follow = 0; o->su_accept = 1; o->su_first_attempt = 0;
    o->su_land_blind_from = 1; o->su_land_first = 2; o->su_land = 1; o->su_land_tol[0] = 1e-3; o->su_land_tol[1] = 1e-4; o->su_land_tol[2] = 1e-5; o->su_land_rho = 1e4;
    o->su_warm[0] = 1e-3; o->su_warm[1] = 1e-3; o->su_warm_endgame[0] = 0.9999; o->su_warm_endgame[1] = 1e-5; o->su_warm_clip = 0.01;
    // easy start = the previous solution ITSELF: slack floor, barrier parameter and clip margin below the stop tolerances (1e-12 against
    // mu <= 1e-11 (1 + |grad|), |r_p| <= 1e-10), so that the stop test can accept the start when the new su-problem's optimality
    // conditions already hold there (a converging ADMM in a static scene: 57 % of the north-star solves) - zero Newton steps
    { const double ez[5] = {1e-12, 1e-12, 1e-12, 0.999999, 1e-7}; for (int i = 0; i < 5; ++i) o->su_easy[i] = ez[i]; }
    // (A library call has no process-global configuration: the RDA_* switches of the A/B tools and
    // tests are applied by the Python host package - rda_planner_amd.rda_solver.hip_options - to the struct it hands to rda_create_opts.)
}
// The options as the solver uses them (null: the defaults): entries outside their range clamped or replaced by the values of rda_opts_init.
// su_tol falls back per entry, su_land_tol and su_tol_early (to 0 = off) all three together; su_hard_warm[0] <= 0 switches that rule off.
static rda_opts opts_sanitised(const rda_opts *opts)
{
    rda_opts def; rda_opts_init(&def);
    if (!opts) return def;
    rda_opts o = *opts;
    if (!(o.lmz_mu > 0)) o.lmz_mu = def.lmz_mu;
    for (int i = 0; i < 3; ++i) if (!(o.su_tol[i] > 0)) o.su_tol[i] = def.su_tol[i];
    if (!(o.su_tol_early[0] > 0 && o.su_tol_early[1] > 0 && o.su_tol_early[2] > 0)) for (int i = 0; i < 3; ++i) o.su_tol_early[i] = def.su_tol_early[i];
    if (!(o.su_land_tol[0] > 0 && o.su_land_tol[1] > 0 && o.su_land_tol[2] > 0)) for (int i = 0; i < 3; ++i) o.su_land_tol[i] = def.su_land_tol[i];
    if (!(o.su_land_rho > 0)) o.su_land_rho = def.su_land_rho;
    if (!(o.su_hard_warm[0] > 0)) o.su_hard_warm[1] = 0.0;
    if (o.su_cold_probe < 1) o.su_cold_probe = 1;
    o.su_land_first = o.su_land_first < 0 ? 0 : (o.su_land_first > 2 ? 2 : o.su_land_first);
    o.su_land = o.su_land ? 1 : 0;
    return o;
}

// mu support candidates of a polygon robot: pairs whose intersection is a vertex of the robot, then the non-null rows, then
// the empty support (same rule and order as the lam lists built per wave in lmz::solve_wave)
static int robot_candidates(int R, const double *G, const double *h, unsigned char *out, double (*rv)[2], int *nrv)
{
    int n = 0, p = 0;
    for (int j1 = 0; j1 < R; ++j1) for (int j2 = j1 + 1; j2 < R; ++j2, ++p) {
        const double a00 = G[2 * j1], a01 = G[2 * j1 + 1], a10 = G[2 * j2], a11 = G[2 * j2 + 1];
        const double det = a00 * a11 - a01 * a10;
        if (det == 0 || !(det * det > 1e-24 * (a00 * a00 + a01 * a01) * (a10 * a10 + a11 * a11))) continue;
        const double wx = h[j1] * a11 - a01 * h[j2], wy = a00 * h[j2] - h[j1] * a10, sg = det > 0 ? 1.0 : -1.0, ad = fabs(det);
        bool ok = true;
        for (int k = 0; k < R; ++k) {
            const double viol = sg * (G[2 * k] * wx + G[2 * k + 1] * wy - h[k] * det);
            if (viol > 1e-9 * (ad + fabs(h[k]) * ad + fabs(G[2 * k] * wx) + fabs(G[2 * k + 1] * wy))) ok = false;
        }
        if (ok) { rv[n][0] = wx / det; rv[n][1] = wy / det; out[n++] = (unsigned char)(1 + R + p); }
    }
    *nrv = n;
    for (int j = 0; j < R; ++j) if (G[2 * j] != 0 || G[2 * j + 1] != 0) out[n++] = (unsigned char)(1 + j);
    out[n++] = 0;
    return n;
}

static int terms_rebuild(rda_handle *H);

extern "C" int rda_create_opts(const rda_cfg *cfg, const rda_opts *opts, const double *G, const double *h, rda_handle **out)
{
    if (!cfg || !G || !h || !out) return RDA_ERR_ARG;
    if (cfg->robot_norm2 && cfg->R < 2) return RDA_ERR_UNSUPPORTED;
    if (cfg->E < 1 || cfg->E > RDA_EMAX || cfg->R < 1 || cfg->R > RDA_RMAX || cfg->T < 1 || cfg->T > RDA_TMAX || cfg->N < 1) return RDA_ERR_UNSUPPORTED;
    if (cfg->E + cfg->R + 1 > 64) return RDA_ERR_UNSUPPORTED;
    if (rda_device_count() < 1) return RDA_ERR_NODEVICE;
    *out = nullptr;
    std::unique_ptr<rda_handle> owner(new rda_handle());     // a failure on the way drops the handle and with it what was built
    rda_handle *H = owner.get();
    memset(&H->d, 0, sizeof(Dev));
    H->d.c = *cfg; H->d.nt = 1; H->d.obstacle_num = 0;
    const rda_opts &o = H->opts = opts_sanitised(opts);
    H->d.warm = o.lmz_warm;
    H->d.rows = (cfg->E + cfg->R + 1 <= 16) && o.lmz_rows != 0;
    H->d.nmv = robot_candidates(cfg->R, G, h, H->d.muc, H->d.rv, &H->d.nrv);
    H->rob_G.assign(G, G + 2 * cfg->R); H->rob_h.assign(h, h + cfg->R);
    H->d.centre = o.tie_centre ? 1 : 0;
    H->d.lmz_mode = (o.lmz_mode || cfg->robot_norm2) ? 1 : 0; H->d.lmz_mu = o.lmz_mu;      // the enumeration has no norm2-robot candidates
    H->d.su_warm_wfl = o.su_warm[0]; H->d.su_warm_mu0 = o.su_warm[1]; H->d.su_warm_cap = o.su_warm_cap; H->d.su_warm_first = o.su_warm_first;
    H->d.su_hard_wfl = o.su_hard_warm[0]; H->d.su_hard_mu0 = o.su_hard_warm[1];
    H->d.su_warm_tau = o.su_warm_endgame[0]; H->d.su_warm_sig = o.su_warm_endgame[1]; H->d.su_warm_clip = o.su_warm_clip;
    for (int i = 0; i < 5; ++i) H->d.su_easy[i] = o.su_easy[i];
    H->d.su_easy_max = o.su_easy_max; H->d.su_easy_nopred = o.su_easy_nopred;
    H->d.su_pre = o.su_pre;
    H->d.su_cold_from = o.su_cold_from; H->d.su_cold_probe = o.su_cold_probe;
    H->d.su_light = o.su_light; H->d.su_split = o.su_split; H->d.su_accept = o.su_accept; H->d.su_first_attempt = o.su_first_attempt;
    H->d.su_land_first = o.su_land_first; H->d.su_land_blind_from = o.su_land_blind_from;
    H->d.su_land = o.su_land; H->d.su_land_rho = o.su_land_rho;
    for (int i = 0; i < 3; ++i) { H->d.su_tol[i] = o.su_tol[i]; H->d.su_tol_early[i] = o.su_tol_early[i]; H->d.su_land_tol[i] = o.su_land_tol[i]; }
    const size_t T = cfg->T, N = cfg->N, E = cfg->E, R = cfg->R;
    HIPCHK(hipStreamCreate(H->stream.out()));
    HIPCHK(hipStreamCreate(H->stream2.out()));
    HIPCHK(hipEventCreateWithFlags(H->ev_tick.out(), hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(H->ev_scene.out(), hipEventDisableTiming));
    Dev &d = H->d;
    hbuf::Group &m = H->mem;
    int rc = 0;
    rc |= m.dev(&d.G, 2 * R); rc |= m.dev(&d.h, R);
    rc |= m.dev(&d.A, N * (T + 1) * E * 2); rc |= m.dev(&d.b, N * (T + 1) * E); rc |= m.dev(&d.cone, N);
    rc |= m.dev(&d.wl, (N + GS) * T); d.wl_cap = (int)((N + GS) * T); d.src_cap = (int)(4 * N + 256); d.hint_stride = (int)N + d.src_cap; d.hint_len = d.hint_stride * (int)T; d.slot_src = nullptr; d.src_used = 0;
    rc |= m.dev(&d.hint, 2 * (size_t)d.hint_len); d.oc_ls = (1 + (int)E + (int)E * ((int)E - 1) / 2 + 3) & ~3; d.oc_vs = (int)E * ((int)E - 1) > 2 ? (int)E * ((int)E - 1) : 2;
    rc |= m.dev(&d.oc_lamc, N * (T + 1) * d.oc_ls); rc |= m.dev(&d.oc_vtx, N * (T + 1) * d.oc_vs); rc |= m.dev(&d.oc_cnt, N * (T + 1) * 2);
    rc |= m.dev(&d.lam, N * (T + 1) * E); rc |= m.dev(&d.mu, N * (T + 1) * R); rc |= m.dev(&d.z, N * T);
    rc |= m.dev(&d.xi, N * (T + 1) * 2); rc |= m.dev(&d.zeta, N * T); rc |= m.dev(&d.dis, T);
    d.P = 1; d.rank = 0; d.Nloc = (int)N; d.Nlive = (int)N; d.J = (int)((N + GS - 1) / GS); d.chunk = chunk_doubles((int)T, (int)N); d.lchunk = lchunk_doubles((int)T, (int)N);
    rc |= H->terms.dev(&d.coef, d.chunk); rc |= H->terms.dev(&d.coefL, d.lchunk);
    rc |= m.dev(&d.s, traj_s(T)); rc |= m.dev(&d.u, traj_u(T)); rc |= m.dev(&d.pose, 4 * T);
    rc |= m.dev(&d.ctrl, 1);
    rc |= m.dev(&d.su_lam_keep, 10 * T);
    if (H->opts.duals_follow) {
        rc |= m.dev(&H->fol.prev_sel, N); rc |= m.dev(&H->fol.map, N);
        rc |= m.dev(&H->fol.tmp, N * (T + 1) * (E + R + 2) + 2 * N * T);
    }
#if defined(SU_TRACE)
    if (o.su_prof) rc |= m.dev(&d.su_prof, su::PROF_WORDS);                   // 16 + the per-wave event trace of the LAST su launch (tools/su_trace.py)
#elif defined(SU_PROF) || defined(SU_FINE)
    if (o.su_prof) rc |= m.dev(&d.su_prof, 16);
#else
    if (o.su_prof) return RDA_ERR_UNSUPPORTED;     // phase counters: profiling builds only (-DSU_PROF / -DSU_FINE, tools/su_phase_profile.py)
#endif
    rc |= m.dev(&H->step.d, step_doubles(T)); rc |= m.dev(&H->res.blk.d, res_doubles(T));
    rc |= m.pin(&H->stage.A, N * (T + 1) * E * 2); rc |= m.pin(&H->stage.b, N * (T + 1) * E); rc |= m.pin(&H->stage.cone, N);
    rc |= m.pin(&H->step.h, step_doubles(T)); rc |= m.pin(&H->res.blk.h, res_doubles(T));
    H->step.n = step_doubles(T); H->res.blk.n = res_doubles(T); H->res.T = T;      // (the two pairs filled in by hand: the allocations keep their order)
    d.ip_rows = (d.lmz_mode && o.lmz_ip_rows && rip::fits(cfg->E, cfg->R, cfg->E >= 3, cfg->robot_norm2, cfg->accelerated)) ? 1 : 0;
    if (d.ip_rows && o.lmz_ip_warm) { rc |= m.dev(&d.ipw, N * T * 80); rc |= m.dev(&d.ipf, N * T); }
    if (rc) return RDA_ERR_HIP;
    { const int hard = 99; HIPCHK(hipMemcpy(&d.ctrl->su_last, &hard, sizeof(int), hipMemcpyHostToDevice)); }     // no su history yet
    HIPCHK(hipMemcpy(d.G, G, 2 * R * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.h, h, R * sizeof(double), hipMemcpyHostToDevice));
    std::vector<double> ones(T, 1.0);                                       // para_dis init, rda_solver.py:119
    HIPCHK(hipMemcpy(d.dis, ones.data(), T * sizeof(double), hipMemcpyHostToDevice));
    std::vector<int> cn(N, 1);                                              // para_cone init, rda_solver.py:158
    HIPCHK(hipMemcpy(d.cone, cn.data(), N * sizeof(int), hipMemcpyHostToDevice));
    H->su_lds = su::lds_bytes((int)T);
    RDA_SU_DISPATCH((int)T, HIPCHK(hipFuncSetAttribute((const void *)k_su<TT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)H->su_lds)));
    HIPCHK(hipFuncSetAttribute((const void *)k_finish, hipFuncAttributeMaxDynamicSharedMemorySize, (int)H->su_lds));
    H->su_trk_lds = H->su_lds > track::LDS_DOUBLES * sizeof(double) ? H->su_lds : track::LDS_DOUBLES * sizeof(double);
    RDA_SU_DISPATCH((int)T, HIPCHK(hipFuncSetAttribute((const void *)k_su_tracked<TT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)H->su_trk_lds)));
    // the terms of a fresh handle are all zero: their block partials (zero sums, every slot NEAR: a = 0 puts the hinge at -d < 0)
    if (int rcf = terms_rebuild(H)) return rcf;
    HIPCHK(hipStreamSynchronize(H->stream));
    *out = owner.release();
    return RDA_OK;
}
extern "C" int rda_create(const rda_cfg *cfg, const double *G, const double *h, rda_handle **out) { return rda_create_opts(cfg, nullptr, G, h, out); }

extern "C" void rda_destroy(rda_handle *H)
{
    if (!H) return;
    (void)hipStreamSynchronize(H->stream);         // nothing is released while a launch or a collective may still use it
    (void)hipStreamSynchronize(H->stream2);
    if (H->shard.comm && H->shard.comm_destroy) H->shard.comm_destroy(H->shard.comm);  // (before the streams go: not a destructor's work)
    delete H;
}

extern "C" int rda_set_adjust(rda_handle *H, double slack_gain, double max_sd, double min_sd, double ro1, double ro2)
{
    if (!H) return RDA_ERR_ARG;
    H->d.c.slack_gain = slack_gain; H->d.c.max_sd = max_sd; H->d.c.min_sd = min_sd; H->d.c.ro1 = ro1; H->d.c.ro2 = ro2;
    return RDA_OK;
}

// block partials (sums, near masks) of every local chunk from the stored terms: after the host rewrote terms
static int terms_rebuild(rda_handle *H)
{
    const Dev &d = H->d;
    const int nb = (d.c.T * d.J + FPB - 1) / FPB;
    hipLaunchKernelGGL(k_lmz_finalize_all, dim3(nb, d.P), dim3(256), 0, H->stream, d);
    HIPCHK(hipGetLastError());
    return RDA_OK;
}

// Obstacle shards: the local term arrays (hinge offsets, G'mu + xi) of the OTHER ranks' slots are never populated on this rank, so the
// terms of remote slots cannot be rebuilt here once the ranks have stepped - a reset / state rewrite would leave every rank with a
// different su-problem (and different early-stop verdicts: the next all-gather would hang).  Refused from the first step on.
static inline bool shard_frozen(const rda_handle *H) { return H->d.P > 1 && H->stepped; }
extern "C" int rda_reset(rda_handle *H)
{
    if (!H) return RDA_ERR_ARG;
    if (shard_frozen(H)) return RDA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_reset, dim3(64), dim3(256), 0, H->stream, H->d);
    HIPCHK(hipGetLastError());
    int rc = terms_rebuild(H);
    if (rc != RDA_OK) return rc;
    HIPCHK(hipStreamSynchronize(H->stream));
    return RDA_OK;
}

extern "C" int rda_get_su_history_n(rda_handle *H, int32_t *hist, int n_hist, double *lam_keep)
{
    if (!H || n_hist < 0) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(H->stream));
    if (hist && n_hist > 0) {
        Ctrl c;
        HIPCHK(hipMemcpy(&c, H->d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost));
        const int32_t all[RDA_SU_HISTORY_INTS] = { c.su_last, c.su_probe, c.prev_unconv, c.su_hardlike, c.spec_credit, c.land_hard, c.land_easy, c.blind_ok };
        for (int i = 0; i < n_hist; ++i) hist[i] = i < RDA_SU_HISTORY_INTS ? all[i] : 0;      // (entries a later version may add read as 0 here)
    }
    if (lam_keep) HIPCHK(hipMemcpy(lam_keep, H->d.su_lam_keep, (size_t)su::NC * H->d.c.T * sizeof(double), hipMemcpyDeviceToHost));
    return RDA_OK;
}
extern "C" int rda_set_su_history_n(rda_handle *H, const int32_t *hist, int n_hist, const double *lam_keep)
{
    if (!H || n_hist < 0) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(H->stream));
    if (hist) {
        int *dst[RDA_SU_HISTORY_INTS] = { &H->d.ctrl->su_last, &H->d.ctrl->su_probe, &H->d.ctrl->prev_unconv, &H->d.ctrl->su_hardlike, &H->d.ctrl->spec_credit, &H->d.ctrl->land_hard, &H->d.ctrl->land_easy, &H->d.ctrl->blind_ok };
        for (int i = 0; i < n_hist && i < RDA_SU_HISTORY_INTS; ++i) HIPCHK(hipMemcpy(dst[i], &hist[i], sizeof(int), hipMemcpyHostToDevice));   // entries the caller does not have keep their value
    }
    if (lam_keep) HIPCHK(hipMemcpy(H->d.su_lam_keep, lam_keep, (size_t)su::NC * H->d.c.T * sizeof(double), hipMemcpyHostToDevice));
    return RDA_OK;
}
// the forms without a count: RDA_SU_HISTORY_INTS (= 8 since round 6; round 5: 4, round 4: 2) entries - a caller built against an older header must use the _n forms
extern "C" int rda_get_su_history(rda_handle *H, int32_t *hist, double *lam_keep) { return rda_get_su_history_n(H, hist, RDA_SU_HISTORY_INTS, lam_keep); }
extern "C" int rda_set_su_history(rda_handle *H, const int32_t *hist, const double *lam_keep) { return rda_set_su_history_n(H, hist, RDA_SU_HISTORY_INTS, lam_keep); }
extern "C" int rda_lmz_history_doubles(rda_handle *H) { return !H ? RDA_ERR_ARG : (H->d.ipw ? 80 * H->d.c.N * H->d.c.T : 0); }
extern "C" int rda_get_lmz_history(rda_handle *H, double *points, int32_t *valid)
{
    if (!H) return RDA_ERR_ARG;
    if (!H->d.ipw) return RDA_ERR_UNSUPPORTED;
    HIPCHK(hipStreamSynchronize(H->stream));
    const size_t nt = (size_t)H->d.c.N * H->d.c.T;
    if (points) HIPCHK(hipMemcpy(points, H->d.ipw, nt * 80 * sizeof(double), hipMemcpyDeviceToHost));
    if (valid) HIPCHK(hipMemcpy(valid, H->d.ipf, nt * sizeof(int), hipMemcpyDeviceToHost));
    return RDA_OK;
}
extern "C" int rda_set_lmz_history(rda_handle *H, const double *points, const int32_t *valid)
{
    if (!H) return RDA_ERR_ARG;
    if (!H->d.ipw) return RDA_ERR_UNSUPPORTED;
    HIPCHK(hipStreamSynchronize(H->stream));
    const size_t nt = (size_t)H->d.c.N * H->d.c.T;
    if (points) HIPCHK(hipMemcpy(H->d.ipw, points, nt * 80 * sizeof(double), hipMemcpyHostToDevice));
    if (valid) HIPCHK(hipMemcpy(H->d.ipf, valid, nt * sizeof(int), hipMemcpyHostToDevice));
    return RDA_OK;
}
extern "C" int rda_debug_su_prof(rda_handle *H, long long *out16)
{
    if (!H || !out16) return RDA_ERR_ARG;
    if (!H->d.su_prof) return RDA_ERR_UNSUPPORTED;
    HIPCHK(hipStreamSynchronize(H->stream));
    HIPCHK(hipMemcpy(out16, H->d.su_prof, 16 * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(H->d.su_prof, 0, 16 * sizeof(long long)));
    return RDA_OK;
}

extern "C" int rda_debug_su_land_n(rda_handle *H, int32_t *out, int n)
{
    if (!H || !out || n < 1 || n > su::LAND_STATS) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(H->stream));
    HIPCHK(hipMemcpy(out, H->d.ctrl->land_stat, n * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(H->d.ctrl->land_stat, 0, su::LAND_STATS * sizeof(int)));
    return RDA_OK;
}
extern "C" int rda_debug_su_land(rda_handle *H, int32_t *out4) { return rda_debug_su_land_n(H, out4, 4); }      // the first four, as before the counters grew

// debug, -DSU_TRACE builds only: (event id, clock64) pairs of the four waves of the LAST su launch of this handle, [4][cap][2]; *n_out = events per wave
extern "C" int rda_debug_su_trace(rda_handle *H, long long *out, int cap, int *n_out)
{
    if (!H || !out || !n_out || cap < 1) return RDA_ERR_ARG;
#if defined(SU_TRACE)
    if (!H->d.su_prof) return RDA_ERR_UNSUPPORTED;
    HIPCHK(hipStreamSynchronize(H->stream));
    std::vector<long long> buf(2 * 4 * su::TRACE_CAP);
    HIPCHK(hipMemcpy(buf.data(), H->d.su_prof + 16, buf.size() * sizeof(long long), hipMemcpyDeviceToHost));
    const int n = cap < su::TRACE_CAP ? cap : su::TRACE_CAP;
    for (int w = 0; w < 4; ++w)
        for (int e = 0; e < n; ++e) { out[(w * cap + e) * 2] = buf[(w * su::TRACE_CAP + e) * 2]; out[(w * cap + e) * 2 + 1] = buf[(w * su::TRACE_CAP + e) * 2 + 1]; }
    *n_out = n;
    return RDA_OK;
#else
    (void)H;
    return RDA_ERR_UNSUPPORTED;
#endif
}

// debug: rows the common-path LamMuZ kernel of the LAST executed iteration put on the work list (split launch form only)
// debug / test hook: forget every remembered support (both buffers -> "none").  The supports are a cache - every answer is accepted on its
// optimality certificate alone - so a loop must return the same bits with or without them (tests/test_gpu_supports.py).
extern "C" int rda_debug_flush_supports(rda_handle *H)
{
    if (!H) return RDA_ERR_ARG;
    HIPCHK(hipMemsetAsync(H->d.hint, 0xff, 2 * (size_t)H->d.hint_len * sizeof(int), H->stream));
    HIPCHK(hipStreamSynchronize(H->stream));
    return RDA_OK;
}
extern "C" int rda_debug_slot_src(rda_handle *H, int32_t *src, int32_t *used)
{
    if (!H || !src || !used) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(H->stream));
    if (H->tick.scene_on_s2) HIPCHK(hipStreamSynchronize(H->stream2));
    *used = H->d.slot_src ? H->d.src_used : 0;
    if (*used > 0) HIPCHK(hipMemcpy(src, H->d.slot_src, (size_t)*used * sizeof(int), hipMemcpyDeviceToHost));
    return RDA_OK;
}
extern "C" int rda_debug_worklist(rda_handle *H, int *rows)
{
    if (!H || !rows) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(H->stream));
    HIPCHK(hipMemcpy(rows, &H->d.ctrl->wl_count, sizeof(int), hipMemcpyDeviceToHost));
    return RDA_OK;
}
// debug / test hooks of the rule that a failed call changes nothing and leaks nothing (host_buf.h): refuse the allocation with index n among
// those this thread requests from now on (n < 0: none), and what the library holds now
extern "C" int rda_debug_alloc_fail(int n) { hbuf::refuse_in = n; return RDA_OK; }
extern "C" int rda_debug_alloc_stats(long long *live_allocs, long long *live_bytes)
{
    if (live_allocs) *live_allocs = hbuf::live_allocs;
    if (live_bytes) *live_bytes = hbuf::live_bytes;
    return RDA_OK;
}

// assign_obstacle_parameter (rda_solver.py:483-526): pad / truncate into N slots, then upload
static int obstacles_stage(rda_handle *H, int n_obs, const double *A, const double *b, const int32_t *cone, int per_t, bool sync)
{
    if (!H) return RDA_ERR_ARG;
    Dev &d = H->d;
    const size_t T = d.c.T, N = d.c.N, E = d.c.E;
    if (n_obs <= 0) { d.obstacle_num = 0; return RDA_OK; }       // nothing written: stale A, b stay
    if (!A || !b || !cone) return RDA_ERR_ARG;
    if (H->opts.duals_follow) return RDA_ERR_UNSUPPORTED;        // duals_follow: host-staged slots carry no obstacle identity
    d.sc_bad = nullptr;
    H->sc.n = 0;                                                 // the slots no longer come from the resident raw scene: rda_scene_resort must not rebuild them from it
    const size_t nt = per_t ? T + 1 : 1;
    for (size_t n = 0; n < N; ++n) {
        size_t src = n < (size_t)n_obs ? n : (size_t)n_obs - 1;   // quirk Q3: duplicate the last obstacle
        memcpy(&H->stage.A[n * nt * E * 2], &A[src * nt * E * 2], nt * E * 2 * sizeof(double));
        memcpy(&H->stage.b[n * nt * E], &b[src * nt * E], nt * E * sizeof(double));
        H->stage.cone[n] = cone[src];
        if (cone[src] == 1) {         // canonical circle only (mpc.py:440-458)
            for (size_t t = 0; t < nt; ++t) {
                const double *At = &H->stage.A[(n * nt + t) * E * 2];
                if (E < 3 || At[0] != 1 || At[1] != 0 || At[2] != 0 || At[3] != 1 || At[4] != 0 || At[5] != 0) return RDA_ERR_UNSUPPORTED;
            }
        }
    }
    HIPCHK(hipMemcpyAsync(d.A, H->stage.A, N * nt * E * 2 * sizeof(double), hipMemcpyHostToDevice, H->stream));
    HIPCHK(hipMemcpyAsync(d.b, H->stage.b, N * nt * E * sizeof(double), hipMemcpyHostToDevice, H->stream));
    HIPCHK(hipMemcpyAsync(d.cone, H->stage.cone, N * sizeof(int), hipMemcpyHostToDevice, H->stream));
    d.nt = (int)nt; d.obstacle_num = (int)N;
    d.slot_src = nullptr; d.src_used = 0;                    // host-staged slots: the remembered supports are keyed by slot
    hipLaunchKernelGGL(k_prepare, dim3((unsigned)((N * nt + 3) / 4)), dim3(256), 0, H->stream, d);
    if (sync) HIPCHK(hipStreamSynchronize(H->stream));      // staging buffers are reused by the next call
    return RDA_OK;
}

extern "C" int rda_upload_obstacles(rda_handle *H, int n_obs, const double *A, const double *b, const int32_t *cone, int per_t)
{
    return obstacles_stage(H, n_obs, A, b, cone, per_t, true);
}

// ---- device-side obstacle pipeline -----------------------------------------------------------------------------
// the grown scene set, built beside the old one (alloc) and moved in (commit) only when all of it exists - rda_fleet_upload_scans allocates for every member
// before it commits for any.  A part that stays empty has nothing to grow.
struct SceneGrow { SceneDev dev; SceneHost host; };
static int scene_grow_alloc(const rda_handle *H, int n, SceneGrow &g)
{
    const size_t E = H->d.c.E, need = scene_layout((size_t)n, E).bytes;
    int rc = 0;
    if (n > H->sc.dev.cap) rc |= g.dev.alloc(n + n / 2 + 16, E);
    if (need > H->sc.host.bytes) rc |= g.host.alloc(need * 2);
    return rc ? RDA_ERR_HIP : RDA_OK;
}
static void scene_grow_commit(rda_handle *H, SceneGrow &g)
{
    if (g.dev.have()) { H->sc.dev = std::move(g.dev); H->sc.n = 0; }      // (the resident raw scene went with the old block)
    if (g.host.have()) H->sc.host = std::move(g.host);
}
static int scene_reserve(rda_handle *H, int n)
{
    SceneGrow g;
    if (scene_grow_alloc(H, n, g) != RDA_OK) return RDA_ERR_HIP;
    scene_grow_commit(H, g);
    return RDA_OK;
}
// the conversion kernels' arguments for a raw scene of n obstacles in the handle's (reserved) device block, its slots built for nt stages
static scene::Args scene_args(const rda_handle *H, int n, int nt, int order)
{
    const Dev &d = H->d;
    const SceneLayout l = scene_layout((size_t)n, (size_t)d.c.E);
    double *db = H->sc.dev.blk;
    scene::Args a;
    a.n = n; a.N = d.c.N; a.E = d.c.E; a.T = d.c.T; a.nt = nt; a.order = order; a.dt = d.c.dt;
    a.kind = (int *)(db + l.ints); a.nvert = (int *)(db + l.ints) + n; a.geom = db; a.vel = db + l.vel; a.robot = db + l.robot;
    a.key = H->sc.dev.key; a.sel = H->sc.dev.sel; a.A = d.A; a.b = d.b; a.cone = d.cone; a.nonconvex = (int *)(db + l.nonconvex);
    a.rx = 0; a.ry = 0; a.robot_val = 0;
    return a;
}
// The host-side record that the handle's slots now come from the raw scene `a`.  store: `a` is also the resident raw scene from now on (rda_scene_resort
// runs the kernels on modified arguments and keeps what is stored).
static void scene_bind(rda_handle *H, const scene::Args &a, bool store)
{
    Dev &d = H->d;
    if (store) { H->sc.args = a; H->sc.n = a.n; H->sc.peers_of = nullptr; }
    d.nt = a.nt; d.obstacle_num = a.N; d.sc_bad = a.nonconvex;
    d.slot_src = H->sc.dev.sel; d.src_used = a.n < a.N ? a.n : a.N;  // the remembered supports follow the obstacles through the re-binding (Dev::hint)
}

// the binding and the conversion kernels on a raw scene that is in device memory: distance keys, stable rank, half-space slots, candidate lists
static void scene_kernels(rda_handle *H, const scene::Args &a, hipStream_t st, bool store)
{
    Dev &d = H->d;
    const int n = a.n, N = a.N;
    scene_bind(H, a, store);
    hipLaunchKernelGGL(scene::k_keys, dim3((n + 255) / 256), dim3(256), 0, st, a);
    hipLaunchKernelGGL(scene::k_rank, dim3((n + 15) / 16), dim3(256), 0, st, a);
    hipLaunchKernelGGL(scene::k_build, dim3((N * a.nt + 255) / 256), dim3(256), 0, st, a);
    if (H->opts.duals_follow) {
        // rda_opts::duals_follow: the dual state is re-arranged from the previous binding to this one.  Nothing of a tick's head reads
        // lam, mu, xi, z, zeta (the su-problem reads the condensed terms, which the first LamMuZ launch of the tick rewrites for every
        // slot): inside a tick this runs on the second stream beside the first su-problem like the rest of the staging.
        const int used = d.src_used;
        const bool have = H->fol.prev_used >= 0;
        if (have) hipLaunchKernelGGL(k_follow_gather, dim3(N), dim3(64), 0, st, d, (const int *)H->sc.dev.sel, used, (const int *)H->fol.prev_sel, H->fol.prev_used, H->fol.map, H->fol.tmp);
        hipLaunchKernelGGL(k_follow_back, dim3(N), dim3(64), 0, st, d, have ? (const int *)H->fol.map : (const int *)nullptr, (const double *)H->fol.tmp,
                           (const int *)H->sc.dev.sel, used, H->fol.prev_sel);
        H->fol.prev_used = used;
    }
    hipLaunchKernelGGL(k_prepare, dim3((unsigned)((N * a.nt + 3) / 4)), dim3(256), 0, st, d);
}

static int scene_stage(rda_handle *H, int n, const int32_t *kind, const int32_t *nvert, const double *geom,
                       const double *vel, const double *robot_xy, int order, int32_t *n_nonconvex, bool sync, hipStream_t st = nullptr)
{
    if (!H) return RDA_ERR_ARG;
    if (!st) st = H->stream;
    Dev &d = H->d;
    if (n_nonconvex) *n_nonconvex = 0;
    if (n <= 0) { d.obstacle_num = 0; return RDA_OK; }           // nothing written: stale A, b stay (rda_solver.py:485)
    if (!kind || !nvert || !geom || !vel || (order && !robot_xy)) return RDA_ERR_ARG;
    const int E = d.c.E, T = d.c.T;
    bool any_moving = false;
    for (int i = 0; i < n; ++i) {
        if (kind[i] == 1) { if (E < 3) return RDA_ERR_UNSUPPORTED; }
        else if (kind[i] != 0 || nvert[i] < 0 || nvert[i] > E) return RDA_ERR_ARG;
        any_moving = any_moving || sqrt(vel[2 * i] * vel[2 * i] + vel[2 * i + 1] * vel[2 * i + 1]) > 0.01;
    }
    if (int rc = scene_reserve(H, n)) return rc;
    // one pinned staging block -> its device mirror, one copy
    const SceneLayout l = scene_layout((size_t)n, (size_t)E);
    double *hb = (double *)H->sc.host.blk;
    memcpy(hb, geom, l.vel * sizeof(double));
    memcpy(hb + l.vel, vel, (size_t)n * 2 * sizeof(double));
    hb[l.robot] = robot_xy ? robot_xy[0] : 0; hb[l.robot + 1] = robot_xy ? robot_xy[1] : 0;
    hb[l.nonconvex] = 0.0;                                                 // all-zero bits: the int counter starts at 0
    memcpy((int *)(hb + l.ints), kind, (size_t)n * sizeof(int));
    memcpy((int *)(hb + l.ints) + n, nvert, (size_t)n * sizeof(int));
    HIPCHK(hipMemcpyAsync(H->sc.dev.blk, hb, l.bytes, hipMemcpyHostToDevice, st));
    const scene::Args a = scene_args(H, n, any_moving ? T + 1 : 1, order);
    scene_kernels(H, a, st, true);
    HIPCHK(hipGetLastError());
    if (n_nonconvex) {
        HIPCHK(hipMemcpyAsync(H->sc.host.blk, a.nonconvex, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *n_nonconvex = *(int *)H->sc.host.blk;
    } else if (sync) {
        HIPCHK(hipStreamSynchronize(st));                  // the staging block is reused by the next call
    }
    return RDA_OK;
}

extern "C" int rda_last_nonconvex(rda_handle *H)
{
    if (!H) return RDA_ERR_ARG;
    return (int)*(const long long *)(H->res.blk.h + res_nonconvex(H->d.c.T));
}

extern "C" int rda_upload_scene(rda_handle *H, int n, const int32_t *kind, const int32_t *nvert, const double *geom,
                                const double *vel, const double *robot_xy, int order, int32_t *n_nonconvex)
{
    return scene_stage(H, n, kind, nvert, geom, vel, robot_xy, order, n_nonconvex, true);
}

// test hook: the staged obstacle slots as the solver sees them
extern "C" int rda_get_obstacles(rda_handle *H, double *A, double *b, int32_t *cone, int32_t *nt)
{
    if (!H || !A || !b || !cone || !nt) return RDA_ERR_ARG;
    const Dev &d = H->d;
    const size_t N = d.c.N, E = d.c.E;
    HIPCHK(hipStreamSynchronize(H->stream));
    HIPCHK(hipMemcpy(A, d.A, N * d.nt * E * 2 * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(b, d.b, N * d.nt * E * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cone, d.cone, N * sizeof(int), hipMemcpyDeviceToHost));
    *nt = d.nt;
    return RDA_OK;
}
// test hook: the resident raw geometry [n][E][2] as it stands (rda_fleet_rollout_moving advances it on the device); *n = 0: no resident raw scene
extern "C" int rda_debug_scene_geom(rda_handle *H, double *geom, int32_t *n)
{
    if (!H || !geom || !n) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(H->stream));
    if (H->tick.scene_on_s2) HIPCHK(hipStreamSynchronize(H->stream2));
    *n = H->sc.n > 0 ? H->sc.n : 0;
    if (*n > 0) HIPCHK(hipMemcpy(geom, H->sc.args.geom, (size_t)*n * H->d.c.E * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return RDA_OK;
}

// ... and its velocities [n][2] (rda_fleet_upload_scenes_peers: the peer rows' are written on the device)
extern "C" int rda_debug_scene_vel(rda_handle *H, double *vel, int32_t *n)
{
    if (!H || !vel || !n) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(H->stream));
    if (H->tick.scene_on_s2) HIPCHK(hipStreamSynchronize(H->stream2));
    *n = H->sc.n > 0 ? H->sc.n : 0;
    if (*n > 0) HIPCHK(hipMemcpy(vel, H->sc.args.vel, (size_t)*n * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return RDA_OK;
}

static hipEvent_t next_event(rda_handle *H, int which)
{
    if (H->ev_used[which] == H->ev[which].size()) { hbuf::Event e; (void)hipEventCreate(e.out()); H->ev[which].push_back(std::move(e)); }
    return H->ev[which][H->ev_used[which]++];
}
// the event pair around a timed launch (rda_timing_*): one recorded where the guard is made, one where it goes; nothing with the timing off
struct TimedLaunch {
    rda_handle *H; int which; hipStream_t st;
    TimedLaunch(rda_handle *h, int w, hipStream_t s) : H(h->timing ? h : nullptr), which(w), st(s) { if (H) (void)hipEventRecord(next_event(H, which), st); }
    ~TimedLaunch() { if (H) (void)hipEventRecord(next_event(H, which), st); }
    TimedLaunch(const TimedLaunch &) = delete;          // (a copy would record a third event)
    TimedLaunch &operator=(const TimedLaunch &) = delete;
};

// K1 launches of ADMM iteration `it`.  Which kernels, in which order and on what grid is lmzplan::solo's decision (lmz_plan.h) from the handle's shape
// and staged obstacles: launch_lammuz executes that plan, rda_lammuz_kernel names it (bench.py labels its per-launch times with the name).
static lmzplan::Member lmz_member(const rda_handle *H, const Dev &d)
{
    return { d.c.T, d.Nlive, d.J, d.c.E, d.c.R, d.nt, d.obstacle_num, d.rows, d.lmz_mode, d.ip_rows, H->opts.lmz_dense_from, H->opts.lmz_split };
}
extern "C" const char *rda_lammuz_kernel(rda_handle *H)
{
    if (!H) return "";
    lmzplan::name(lmzplan::solo(lmz_member(H, H->d)), false, H->lmz_name, sizeof H->lmz_name);
    return H->lmz_name;
}
static void launch_lammuz(rda_handle *H, const Dev &d, int it, const Fin &fin)
{
    if (d.Nlive == 0) return;                    // a shard without obstacles (N < P)
    const lmzplan::Plan p = lmzplan::solo(lmz_member(H, d));
    for (int i = 0; i < p.n; ++i) {
        const dim3 grid(p.l[i].grid), block(p.l[i].block);
        // one case per kernel id: the kernel of that name (checked against the table that rda_lammuz_kernel reports from) with its argument list
#define LMZ_SOLO(ID, KERNEL, ...) case lmzplan::ID: static_assert(lmzplan::same(lmzplan::NAMES[lmzplan::ID].solo, #KERNEL), #KERNEL); \
                                  hipLaunchKernelGGL(KERNEL, grid, block, 0, H->stream, __VA_ARGS__); break;
        switch (p.l[i].kernel) {
            LMZ_SOLO(ROWS, k_lammuz_rows, d, it, fin)
            LMZ_SOLO(ROWS_DENSE, k_lammuz_rows_dense, d, it, fin)
            LMZ_SOLO(ROWS_FAST, k_lammuz_rows_fast, d, it)
            LMZ_SOLO(ENUM, k_lammuz_enum, d, it)
            LMZ_SOLO(WAVE, k_lammuz, d, it)
            LMZ_SOLO(IP, k_lammuz_ip, d, it, fin)               // (the row-parallel interior-point kernel)
            LMZ_SOLO(CP_SMALL, k_lammuz_cp_small, d)
            LMZ_SOLO(CP_LARGE, k_lammuz_cp_large, d)
            LMZ_SOLO(FINALIZE, k_lmz_finalize, d, it, fin)
        }
#undef LMZ_SOLO
    }
}

// The ADMM loop of one MPC step (rda_solver.py:588-596) is queued without host synchronisation, in two parts.  The HEAD (the first su-problem,
// which also resets the step's control block) reads the nominal trajectory and the condensed terms of the PREVIOUS step (quirk Q4) but nothing of
// the staged obstacles, so a caller may stage this tick's obstacles on the stream between head and tail while the first su-problem is being
// solved (rda_tracked_begin/_finish).  launch_su: one su-problem, ADMM iteration `it`.
static void launch_su(rda_handle *H, const Dev &d, int it, const double *in_s, const double *in_u, const Fin &fin = Fin{})
{
    const int T = d.c.T;
    TimedLaunch timed(H, 1, H->stream);
    RDA_SU_DISPATCH(T, hipLaunchKernelGGL(k_su<TT>, dim3(1), dim3(su::NT), H->su_lds, H->stream, d, it, in_s, in_u, fin));
}
// Hand-over of a step's result slot to the pinned result block res.blk.h.  Zero-copy form: the launch that ends the step (the su launch that
// detects the early stop, else k_finish) writes the block itself and the host polls the sequence word behind it.  Everything the
// step queued before that launch has completed by then; what is still queued behind it are launches that return at once.
// After 20 ms without the word - or with the timing events on, or RDA_ZERO_COPY=0 - the stream is synchronised the ordinary
// way, which also surfaces a device fault.
static Fin make_fin(rda_handle *H, double *out_u, double *out_s, rda_info *info)
{
    const bool zc = H->opts.zero_copy && !H->timing && out_u == H->res.out_u();
    if (zc) H->res.seq += 1;
    return Fin{ out_u, out_s, info, zc ? H->res.blk.h : nullptr, H->res.seq, out_u == H->res.out_u() ? 1 : 0 };
}
static int launch_finish(rda_handle *H, const Dev &d, const Fin &fin)
{
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(su::NT), H->su_lds, H->stream, d, fin);
    HIPCHK(hipGetLastError());
    return RDA_OK;
}
static inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#endif
}
// spins on a pinned word that a kernel publishes until (word >> shift) == want (acquire), for at most `ms` milliseconds
static bool poll_word(volatile unsigned long long *w, int shift, unsigned long long want, int ms)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 0;; ++spin) {
        if ((*w >> shift) == want) { __atomic_thread_fence(__ATOMIC_ACQUIRE); return true; }
        cpu_relax();
        if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(ms)) return false;
    }
}
static int fetch_result(rda_handle *H)
{
    const size_t T = H->d.c.T;
    if (H->opts.zero_copy && !H->timing) {
        volatile unsigned long long *flag = (volatile unsigned long long *)(H->res.blk.h + res_seq(T));
        if (poll_word(flag, 0, H->res.seq, 20)) return RDA_OK;
        // 20 ms without the word (a healthy step takes a fraction of a millisecond): synchronise the ordinary way.  A device fault -
        // in this step, or in the launches that were still queued behind the hand-over of the PREVIOUS step (the zero-copy hand-over
        // returns before they have drained) - never publishes the word and surfaces here as the stream's error.
        HIPCHK(hipStreamSynchronize(H->stream));
        if (*flag == H->res.seq) return RDA_OK;
        return RDA_ERR_HIP;
    }
    // D2H form: the result block without the sequence word behind it (that word belongs to the zero-copy protocol)
    HIPCHK(hipMemcpyAsync(H->res.blk.h, H->res.out_u(), res_copied_doubles(T) * sizeof(double), hipMemcpyDeviceToHost, H->stream));
    HIPCHK(hipStreamSynchronize(H->stream));
    return RDA_OK;
}
// a finished step out of a pinned result block (blk: u | s) and its info; null = not wanted
static void result_out(const double *blk, const rda_info *blk_info, size_t T, double *out_u, double *out_s, rda_info *info)
{
    if (out_u) memcpy(out_u, blk, traj_u(T) * sizeof(double));
    if (out_s) memcpy(out_s, blk + res_s(T), traj_s(T) * sizeof(double));
    if (info) *info = *blk_info;
}
struct StepViews { double *s, *u, *ref, *speed; };            // the four parts of the step block on the device
static inline StepViews step_views(const rda_handle *H)
{
    const size_t T = H->d.c.T;
    double *const b = H->step.d;
    return { b, b + step_u(T), b + step_ref(T), b + step_speed(T) };
}
// fills the pinned step block and queues its copy to the device
static int step_block_upload(rda_handle *H, const double *nom_s, const double *nom_u, const double *ref_s, double ref_speed)
{
    const size_t T = H->d.c.T;
    memcpy(H->step.h, nom_s, traj_s(T) * sizeof(double));
    memcpy(H->step.h + step_u(T), nom_u, traj_u(T) * sizeof(double));
    memcpy(H->step.h + step_ref(T), ref_s, traj_s(T) * sizeof(double));
    H->step.h[step_speed(T)] = ref_speed;
    HIPCHK(H->step.push(H->stream));
    return RDA_OK;
}
static int enqueue_admm_head(rda_handle *H, const double *in_s, const double *in_u, const double *ref, const double *speed)
{
    Dev d = H->d;
    H->stepped = 1;
    d.ref = const_cast<double *>(ref); d.ref_speed = const_cast<double *>(speed);
    launch_su(H, d, 0, in_s, in_u);                    // resets the step's control block itself (su_body, it == 0)
    HIPCHK(hipGetLastError());
    return RDA_OK;
}
static int enqueue_admm_tail(rda_handle *H, const double *in_s, const double *in_u, const double *ref, const double *speed,
                             double *out_u, double *out_s, rda_info *info)
{
    Dev d = H->d;                                     // taken AFTER the obstacles of this tick were staged (nt, obstacle_num)
    d.ref = const_cast<double *>(ref); d.ref_speed = const_cast<double *>(speed);
    const Fin fin = make_fin(H, out_u, out_s, info);  // the su launch that detects the early stop hands the result over itself
    for (int it = 0; it < d.c.iter_num; ++it) {
        if (it > 0) {
            Fin f = H->opts.early_finish ? fin : Fin{};
            if (H->shard.comm) { f.verdict = H->shard.verdict; f.vseq = ++H->shard.vseq; }
            launch_su(H, d, it, in_s, in_u, f);
        }
        if (it > 0 && H->shard.comm) {
            // The early stop (rda_solver.py:594) is a device flag and kernels queued behind it return at once - a collective cannot, so
            // with a communicator no all-gather may be queued for an iteration that does not run.  The su launch publishes its verdict
            // in pinned host memory as soon as it has reduced the residuals (before its solve; every rank takes the same verdict: the
            // su-problems are bitwise identical); the host polls that word - no copy, no stream synchronisation - and goes on queueing
            // (or stops) while the su-problem is being solved.
            volatile unsigned long long *vw = H->shard.verdict;
            if (!poll_word(vw, 1, H->shard.vseq, 50)) { HIPCHK(hipStreamSynchronize(H->stream)); if ((*vw >> 1) != H->shard.vseq) return RDA_ERR_HIP; }
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            if (*vw & 1ull) break;
        }
        { TimedLaunch timed(H, 0, H->stream); launch_lammuz(H, d, it, H->opts.early_finish ? fin : Fin{}); }
        if (H->shard.comm) {  // one exchange per ADMM iteration: every rank's chunk to every rank (in place)
            int nrc;
            { TimedLaunch timed(H, 2, H->stream); nrc = H->shard.allgather(d.coef + (size_t)d.rank * d.chunk, d.coef, d.chunk, /*ncclDouble*/ 8, H->shard.comm, H->stream); }
            if (nrc != 0) { fprintf(stderr, "librda_hip: ncclAllGather failed (%d)\n", nrc); return RDA_ERR_HIP; }
        }
    }
    return launch_finish(H, d, fin);
}
static int enqueue_admm(rda_handle *H, const double *in_s, const double *in_u, const double *ref, const double *speed,
                        double *out_u, double *out_s, rda_info *info)
{
    int rc = enqueue_admm_head(H, in_s, in_u, ref, speed);
    if (rc != RDA_OK) return rc;
    return enqueue_admm_tail(H, in_s, in_u, ref, speed, out_u, out_s, info);
}

// nominal / reference in, ADMM loop, control / state / info out (host buffers, synchronous).  `stage` queues this tick's
// obstacles (pinned staging block -> H2D -> conversion kernels) WITHOUT waiting: the one synchronisation of the step is
// the one at its end, which also makes the staging blocks reusable by the next call.
template <typename Stage>
static int step_common(rda_handle *H, const double *nom_s, const double *nom_u, const double *ref_s, double ref_speed,
                       double *out_u, double *out_s, rda_info *info, Stage stage)
{
    if (H->tick.pending) return RDA_ERR_ARG;
    int rc = stage();
    if (rc != RDA_OK) { (void)hipStreamSynchronize(H->stream); return rc; }
    const size_t T = H->d.c.T;
    rc = step_block_upload(H, nom_s, nom_u, ref_s, ref_speed);
    if (rc != RDA_OK) return rc;
    const StepViews v = step_views(H);
    rc = enqueue_admm(H, v.s, v.u, v.ref, v.speed, H->res.out_u(), H->res.out_s(), H->res.info());
    if (rc != RDA_OK) return rc;
    rc = fetch_result(H);
    if (rc != RDA_OK) return rc;
    result_out(H->res.blk.h, H->res.h_info(), T, out_u, out_s, info);
    return RDA_OK;
}

extern "C" int rda_step(rda_handle *H, const double *nom_s, const double *nom_u, const double *ref_s,
                        double ref_speed, int n_obs, const double *A, const double *b, const int32_t *cone,
                        int per_t, double *out_u, double *out_s, rda_info *info)
{
    if (!H || !nom_s || !nom_u || !ref_s || !out_u || !out_s) return RDA_ERR_ARG;
    return step_common(H, nom_s, nom_u, ref_s, ref_speed, out_u, out_s, info,
                       [&]() { return obstacles_stage(H, n_obs, A, b, cone, per_t, false); });
}

extern "C" int rda_step_scene(rda_handle *H, const double *nom_s, const double *nom_u, const double *ref_s, double ref_speed,
                              int n, const int32_t *kind, const int32_t *nvert, const double *geom, const double *vel,
                              const double *robot_xy, int order, double *out_u, double *out_s, rda_info *info)
{
    if (!H || !nom_s || !nom_u || !ref_s || !out_u || !out_s) return RDA_ERR_ARG;
    return step_common(H, nom_s, nom_u, ref_s, ref_speed, out_u, out_s, info,
                       [&]() { return scene_stage(H, n, kind, nvert, geom, vel, robot_xy, order, nullptr, false); });
}

// ---- device-side pre_process --------------------------------------------------------------------
__global__ void k_track(Dev d, track::In in, double *path, int L, const double *nom_u, double *step, track::Out *out)
{
    __shared__ double win[track::LDS_DOUBLES];
    const int T = d.c.T, ns = 3 * (T + 1), nu = 2 * T;
    track::Ego e;
    e.path = path; e.L = L; e.nom_u = nom_u; e.nom_s = step; e.ref = step + ns + nu; e.speed = step + 2 * ns + nu;
    e.T = T; e.dynamics = d.c.dynamics; e.dt = d.c.dt; e.wheelbase = d.c.L;
    track::run(e, in, *out, win, threadIdx.x);
}

// k_track and the first su-problem of the step as ONE launch of two workgroups.  Workgroup 0: wave 0 rolls the nominal out (the
// only part of pre_process the su set-up needs), then the su-problem starts; workgroup 1 samples the reference from the path
// meanwhile (closest_point, inter_point: 20 dependent searches, ~12 us) and publishes it under the tick number; the solve picks it
// up after its set-up (su::Args::ref_flag).  Same arithmetic as k_track followed by k_su<TT>(it = 0).
// HIP does not promise that the two workgroups run concurrently (CU masking, a saturated GPU, a debugger): the wait is BOUNDED, and on
// expiry workgroup 0 samples the reference itself (the same track::run part, the same values - should workgroup 1 still run later it
// rewrites them identically).
struct TrackedRefWait {
    track::Ego e; track::In in; track::Out *out; const unsigned long long *flag; unsigned long long seq;
    __device__ __forceinline__ void operator()(double *scratch) const
    {
        int *okw = reinterpret_cast<int *>(scratch);
        if (threadIdx.x == 0) {
            int ok = 0;
            for (int spin = 0; spin < 40000; ++spin) {            // ~ 20 ms at the slowest; a normal wait is 10 - 30 us
                if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == seq) { ok = 1; break; }
                __builtin_amdgcn_s_sleep(8);
            }
            *okw = ok;
        }
        __syncthreads();
        const int ok = *(volatile int *)okw;
        __syncthreads();
        if (!ok) {
            if (threadIdx.x < 64) track::run(e, in, *out, scratch, threadIdx.x, 2);
            __syncthreads();
        }
        if (threadIdx.x == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __syncthreads();
    }
};
template <int TT> __global__ __launch_bounds__(su::NT) void k_su_tracked(Dev d, track::In in, double *path, int L, const double *nom_u, double *step,
                                                                          track::Out *out, unsigned long long seq)
{
    warm_kernargs<sizeof(Dev) + sizeof(track::In) + 5 * sizeof(void *)>();
    const int T = d.c.T, ns = 3 * (T + 1), nu = 2 * T;
    track::Ego e;
    e.path = path; e.L = L; e.nom_u = nom_u; e.nom_s = step; e.ref = step + ns + nu; e.speed = step + 2 * ns + nu;
    e.T = T; e.dynamics = d.c.dynamics; e.dt = d.c.dt; e.wheelbase = d.c.L;
    if (blockIdx.x == 1) {
        if (threadIdx.x < 64) {
            track::run(e, in, *out, smem_su, threadIdx.x, 2);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (threadIdx.x == 0) __hip_atomic_store(&d.ctrl->ref_seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    if (threadIdx.x < 64) track::run(e, in, *out, smem_su, threadIdx.x, 1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    su_body<TT>(d, 0, step, nom_u, d.ref, d.ref_speed, &d.ctrl->ref_seq, seq, nullptr, TrackedRefWait{ e, in, out, &d.ctrl->ref_seq, seq });
}

extern "C" int rda_upload_path(rda_handle *H, int L, const double *path)
{
    if (!H || L < 1 || !path) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(H->stream));
    PathSet t;                                          // a longer path goes to a new buffer that replaces the old one once it holds the path
    const bool grow = L > H->path.len || !H->path.d;
    if (grow && t.g.dev(&t.d, (size_t)3 * L)) return RDA_ERR_HIP;
    HIPCHK(hipMemcpy(grow ? t.d : H->path.d, path, (size_t)3 * L * sizeof(double), hipMemcpyHostToDevice));
    if (grow) H->path = std::move(t);
    H->path.len = L;
    return RDA_OK;
}

// All gear pieces of a path (MPC.curve_list) resident at once, for rda_fleet_rollout_gears: `path` holds the P pieces one behind the other.  `H->path` and
// what reads it are not involved.  The new set is built beside the old one and replaces it once it holds everything.
extern "C" int rda_upload_path_pieces(rda_handle *H, int P, const int32_t *len, const double *gear, const double *path)
{
    if (!H || P < 1 || !len || !gear || !path) return RDA_ERR_ARG;
    PieceSet t;
    t.h_off.assign((size_t)P + 1, 0); t.h_gear.assign(gear, gear + P);
    for (int p = 0; p < P; ++p) {
        if (len[p] < 1 || len[p] > INT_MAX / 3 - t.h_off[p]) return RDA_ERR_ARG;
        t.h_off[p + 1] = t.h_off[p] + len[p];
    }
    HIPCHK(hipStreamSynchronize(H->stream));
    if (t.alloc(P, (size_t)t.h_off[P])) return RDA_ERR_HIP;
    HIPCHK(hipMemcpy(t.buf, path, (size_t)3 * t.h_off[P] * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.off, t.h_off.data(), ((size_t)P + 1) * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.gear, t.h_gear.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice));
    H->pieces = std::move(t);
    return RDA_OK;
}

extern "C" int rda_tracked_begin(rda_handle *H, const double *state, double ref_speed, int cur_index, double threshold, int ind_range,
                                 const double *nom_u)
{
    if (!H || !state || H->tick.pending) return RDA_ERR_ARG;
    if (!H->path.d || cur_index < 0 || cur_index >= H->path.len || ind_range < 1) return RDA_ERR_ARG;
    const size_t T = H->d.c.T;
    const StepViews v = step_views(H);
    const double *in_u = H->d.u;                       // the controls of the last solve are still resident
    if (nom_u) {
        memcpy(H->step.h + step_u(T), nom_u, traj_u(T) * sizeof(double));
        HIPCHK(hipMemcpyAsync(v.u, H->step.h + step_u(T), traj_u(T) * sizeof(double), hipMemcpyHostToDevice, H->stream));
        in_u = v.u;
    }
    track::In in; in.sx = state[0]; in.sy = state[1]; in.sth = state[2]; in.speed = ref_speed; in.threshold = threshold;
    in.cur_index = cur_index; in.ind_range = ind_range;
    // everything queued before this tick: an in-tick scene staging (rda_upload_scene_async) starts behind this event, beside the first
    // su-problem.  Recorded only for callers that stage inside their ticks (learned from the previous tick); a first in-tick staging
    // without it orders itself behind the head of the tick instead.
    H->tick.has_event = 0;
    if (H->tick.stages) { HIPCHK(hipEventRecord(H->ev_tick, H->stream)); H->tick.has_event = 1; }
    H->tick.stages = 0;
    if (H->opts.fuse_track) {
        Dev d = H->d;
        d.ref = v.ref; d.ref_speed = v.speed;
        H->trk_seq += 1;
        {
            TimedLaunch timed(H, 1, H->stream);
            RDA_SU_DISPATCH((int)T, hipLaunchKernelGGL(k_su_tracked<TT>, dim3(2), dim3(su::NT), H->su_trk_lds, H->stream, d, in, H->path.d, H->path.len,
                                                       in_u, v.s, H->res.track(), H->trk_seq));
        }
        HIPCHK(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_track, dim3(1), dim3(64), 0, H->stream, H->d, in, H->path.d, H->path.len, in_u, v.s, H->res.track());
        if (int rc = enqueue_admm_head(H, v.s, in_u, v.ref, v.speed)) return rc;
    }
    H->tick.pending = 1; H->tick.in_u = in_u;
    return RDA_OK;
}

// asynchronous scene work (stage(stream) -> rc; `live`: it queued something), outside or inside a tick
template <typename Stage> static int scene_async(rda_handle *H, bool live, Stage stage)
{
    // one pinned staging block per handle: a second upload before the caller's synchronising call (rda_tracked_finish,
    // rda_sync, a fleet step) has to wait for the first one to have been copied
    if (H->tick.pending_scene) { HIPCHK(hipStreamSynchronize(H->stream)); HIPCHK(hipStreamSynchronize(H->stream2)); H->tick.pending_scene = 0; H->tick.scene_on_s2 = 0; }
    if (!H->tick.pending) {
        int rc = stage(H->stream);
        if (rc == RDA_OK && live) H->tick.pending_scene = 1;
        return rc;
    }
    // inside a tick: the copy and the conversion kernels touch only the obstacle slots, which nothing of the head (k_track,
    // the first su-problem) reads - they run on the second stream BESIDE the first su-problem; rda_tracked_finish joins
    if (!H->tick.has_event) { HIPCHK(hipEventRecord(H->ev_tick, H->stream)); H->tick.has_event = 1; }
    H->tick.stages = 1;
    HIPCHK(hipStreamWaitEvent(H->stream2, H->ev_tick, 0));
    int rc = stage(H->stream2);
    if (rc == RDA_OK && live) { HIPCHK(hipEventRecord(H->ev_scene, H->stream2)); H->tick.pending_scene = 1; H->tick.scene_on_s2 = 1; }
    return rc;
}

extern "C" int rda_upload_scene_async(rda_handle *H, int n, const int32_t *kind, const int32_t *nvert, const double *geom,
                                      const double *vel, const double *robot_xy, int order)
{
    if (!H) return RDA_ERR_ARG;
    return scene_async(H, n > 0, [&](hipStream_t st) -> int { return scene_stage(H, n, kind, nvert, geom, vel, robot_xy, order, nullptr, false, st); });
}

// The reference re-sorts the obstacle list by distance on EVERY tick (mpc.py:205-206, obstacle_order=True) before the first max_obs_num
// are staged.  For a scene that is already resident (rda_upload_scene*) this re-ranks it about a new robot position and rebuilds the
// slots - the same three kernels, the position travels in the kernel arguments: no host-to-device copy.  Asynchronous like
// rda_upload_scene_async (inside a tick it runs beside the first su-problem).  Obstacles with a velocity are predicted from the
// geometry that was uploaded, i.e. a scene that MOVES between ticks has to be uploaded again instead.
extern "C" int rda_scene_resort(rda_handle *H, const double *robot_xy)
{
    if (!H || !robot_xy) return RDA_ERR_ARG;
    if (H->sc.n <= 0 || H->d.obstacle_num == 0) return RDA_ERR_ARG;              // no resident raw scene
    return scene_async(H, true, [&](hipStream_t st) -> int {
        scene::Args a = H->sc.args;
        a.order = 1; a.robot_val = 1; a.rx = robot_xy[0]; a.ry = robot_xy[1];
        HIPCHK(hipMemsetAsync(a.nonconvex, 0, sizeof(int), st));
        scene_kernels(H, a, st, false);
        HIPCHK(hipGetLastError());
        return (int)RDA_OK;
    });
}

// ---- lidar front end on the device (lidar_device.h) ------------------------------------------------------------------------------
static int lidar_reserve(rda_handle *H)
{
    if (H->li.have()) return RDA_OK;
    LidarSet t;
    if (t.alloc()) return RDA_ERR_HIP;
    HIPCHK(hipFuncSetAttribute((const void *)lidar::k_scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lidar::LDS_BYTES));
    H->li = std::move(t);
    return RDA_OK;
}

// One scan through lidar::k_scan, and the wait for it.  The kernel runs on the SECOND stream and touches nothing but the lidar buffers, so inside a
// tick the wait is for this kernel alone, not for the first su-problem.  The boxes stay in li.d_boxes; to_host: labels and boxes also in li.h_labels, li.h_boxes.
static int scan_run(rda_handle *H, int n_beams, const double *ranges, double angle_min, double angle_max, double range_max,
                    const double *state, double eps, int min_samples, bool to_host, int *n_boxes)
{
    if (!H || n_beams < 0 || !ranges || !state || !(eps > 0) || min_samples < 1) return RDA_ERR_ARG;
    if (n_beams > lidar::MAXB || H->d.c.E < 4) return RDA_ERR_UNSUPPORTED;
    // a staging that is still queued may be reading the boxes of the previous scan
    if (H->tick.pending_scene) { HIPCHK(hipStreamSynchronize(H->stream)); HIPCHK(hipStreamSynchronize(H->stream2)); }
    if (int rc = lidar_reserve(H)) return rc;
    memcpy(H->li.h_ranges, ranges, (size_t)n_beams * sizeof(double));
    H->li.h_count[0] = 0; H->li.h_count[1] = 0;
    lidar::Args a;
    a.n_beams = n_beams; a.ranges = H->li.h_ranges; a.angle_min = angle_min; a.angle_max = angle_max; a.range_max = range_max;
    a.sx = state[0]; a.sy = state[1]; a.sth = state[2]; a.eps = eps; a.min_samples = min_samples;
    a.boxes = H->li.d_boxes; a.count = H->li.h_count;
    a.labels_h = to_host ? H->li.h_labels : nullptr; a.boxes_h = to_host ? H->li.h_boxes : nullptr; a.split_tol = H->scan_split;
    { TimedLaunch timed(H, 3, H->stream2); hipLaunchKernelGGL(lidar::k_scan, dim3(1), dim3(lidar::NT), lidar::LDS_BYTES, H->stream2, a); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(H->stream2));
    *n_boxes = H->li.h_count[0];
    return RDA_OK;
}

// The split stage of the scan kernels (lidar::split_stage): 0 = off, the default; the value stays until it is set again.  The handle's value is read by
// rda_scan_boxes and rda_upload_scan, the fleet's by every fleet call that scans - the members' own values are not read there.
static bool scan_split_ok(double tol) { return tol >= 0 && tol <= DBL_MAX; }      // (a NaN fails both)
extern "C" int rda_set_scan_split(rda_handle *H, double tol)
{
    if (!H || !scan_split_ok(tol)) return RDA_ERR_ARG;
    H->scan_split = tol;
    return RDA_OK;
}

extern "C" int rda_scan_boxes(rda_handle *H, int n_beams, const double *ranges, double angle_min, double angle_max, double range_max,
                              const double *state, double eps, int min_samples, int32_t *n_boxes, double *boxes, int cap, int32_t *labels)
{
    if (!n_boxes || cap < 0 || (cap > 0 && !boxes)) return RDA_ERR_ARG;
    int n = 0;
    if (int rc = scan_run(H, n_beams, ranges, angle_min, angle_max, range_max, state, eps, min_samples, true, &n)) return rc;
    *n_boxes = n;
    if (boxes) memcpy(boxes, H->li.h_boxes, (size_t)(n < cap ? n : cap) * 8 * sizeof(double));
    if (labels) memcpy(labels, H->li.h_labels, (size_t)n_beams * sizeof(int32_t));
    return RDA_OK;
}

// the boxes of the last scan as the handle's raw scene (what scene_stage does with a host scene, from device memory) and the conversion kernels
static int scan_stage(rda_handle *H, int n, const double *state, int order, hipStream_t st)
{
    Dev &d = H->d;
    if (n <= 0) { d.obstacle_num = 0; return RDA_OK; }           // nothing written: stale A, b stay (rda_solver.py:485)
    if (int rc = scene_reserve(H, n)) return rc;
    const scene::Args a = scene_args(H, n, 1, order);                  // (boxes: 4-vertex polygons without velocity)
    hipLaunchKernelGGL(lidar::k_scene_fill, dim3((n + 255) / 256), dim3(256), 0, st, (const double *)H->li.d_boxes, n, a.E, const_cast<double *>(a.geom),
                       const_cast<double *>(a.vel), const_cast<double *>(a.robot), a.nonconvex, const_cast<int *>(a.kind), const_cast<int *>(a.nvert), state[0], state[1]);
    scene_kernels(H, a, st, true);
    HIPCHK(hipGetLastError());
    return RDA_OK;
}

extern "C" int rda_upload_scan(rda_handle *H, int n_beams, const double *ranges, double angle_min, double angle_max, double range_max,
                               const double *state, double eps, int min_samples, int order, int32_t *n_boxes)
{
    if (!H) return RDA_ERR_ARG;
    const bool fresh = !H->li.have();
    int n = 0;
    int rc = scan_run(H, n_beams, ranges, angle_min, angle_max, range_max, state, eps, min_samples, false, &n);
    if (rc != RDA_OK) return rc;
    rc = scene_async(H, n > 0, [&](hipStream_t st) -> int { return scan_stage(H, n, state, order, st); });
    if (rc != RDA_OK) { if (fresh) H->li = {}; return rc; }       // a failed call leaves what the handle holds as it was
    if (n_boxes) *n_boxes = n;
    return RDA_OK;
}

extern "C" int rda_tracked_finish(rda_handle *H, double *out_u, double *out_s, rda_info *info,
                                  double *nom_s_out, double *ref_out, int32_t *min_index, double *end_heading)
{
    if (!H || !H->tick.pending) return RDA_ERR_ARG;
    const size_t T = H->d.c.T;
    const double *in_u = H->tick.in_u;
    if (H->tick.scene_on_s2) HIPCHK(hipStreamWaitEvent(H->stream, H->ev_scene, 0));
    H->tick.pending = 0; H->tick.pending_scene = 0; H->tick.scene_on_s2 = 0;
    const StepViews v = step_views(H);
    int rc = enqueue_admm_tail(H, v.s, in_u, v.ref, v.speed, H->res.out_u(), H->res.out_s(), H->res.info());
    if (rc != RDA_OK) { (void)hipStreamSynchronize(H->stream); return rc; }
    if (nom_s_out || ref_out) {
        HIPCHK(H->step.pull(H->stream, step_speed(T)));
        HIPCHK(hipStreamSynchronize(H->stream));
    }
    rc = fetch_result(H);
    if (rc != RDA_OK) return rc;
    result_out(H->res.blk.h, H->res.h_info(), T, out_u, out_s, info);
    if (nom_s_out) memcpy(nom_s_out, H->step.h, traj_s(T) * sizeof(double));
    if (ref_out) memcpy(ref_out, H->step.h + step_ref(T), traj_s(T) * sizeof(double));
    if (min_index) *min_index = H->res.h_track()->min_index;
    if (end_heading) *end_heading = H->res.h_track()->end_heading;
    return RDA_OK;
}

extern "C" int rda_step_tracked(rda_handle *H, const double *state, double ref_speed, int cur_index, double threshold, int ind_range,
                                const double *nom_u, double *out_u, double *out_s, rda_info *info,
                                double *nom_s_out, double *ref_out, int32_t *min_index, double *end_heading)
{
    if (!H || !state || !out_u || !out_s) return RDA_ERR_ARG;
    int rc = rda_tracked_begin(H, state, ref_speed, cur_index, threshold, ind_range, nom_u);
    if (rc != RDA_OK) return rc;
    return rda_tracked_finish(H, out_u, out_s, info, nom_s_out, ref_out, min_index, end_heading);
}

extern "C" int rda_upload_trace(rda_handle *H, int K, const double *nom_s, const double *nom_u, const double *ref_s, const double *ref_speed)
{
    if (!H || K < 1 || !nom_s || !nom_u || !ref_s || !ref_speed) return RDA_ERR_ARG;
    const size_t ns = traj_s(H->d.c.T), nu = traj_u(H->d.c.T);
    TraceSet t;                                         // the new trace replaces the old one once it is complete: a failed upload keeps the old
    if (t.alloc((size_t)K, ns, nu)) return RDA_ERR_HIP;
    HIPCHK(hipMemcpy(t.s, nom_s, K * ns * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.u, nom_u, K * nu * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.ref, ref_s, K * ns * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.speed, ref_speed, K * sizeof(double), hipMemcpyHostToDevice));
    H->trace = std::move(t);
    return RDA_OK;
}

extern "C" int rda_enqueue_step(rda_handle *H, int k)
{
    if (!H || k < 0 || k >= H->trace.K) return RDA_ERR_ARG;
    const size_t ns = traj_s(H->d.c.T), nu = traj_u(H->d.c.T);
    return enqueue_admm(H, H->trace.s + k * ns, H->trace.u + k * nu, H->trace.ref + k * ns, H->trace.speed + k,
                        H->trace.out_u + k * nu, H->trace.out_s + k * ns, H->trace.info + k);
}

// steps k0 .. k1-1 of the uploaded trace, queued back to back (one host call instead of k1-k0)
extern "C" int rda_enqueue_range(rda_handle *H, int k0, int k1)
{
    if (!H || k0 < 0 || k1 > H->trace.K || k0 > k1) return RDA_ERR_ARG;
    for (int k = k0; k < k1; ++k) { int rc = rda_enqueue_step(H, k); if (rc != RDA_OK) return rc; }
    return RDA_OK;
}

#ifdef RDA_LMZ_CLK
extern "C" int rda_debug_lmz_clk(rda_handle *H, unsigned long long *out, int max_waves)     // out[max_waves][LMZ_CLK_WORDS]; reads and clears
{
    static unsigned long long *buf = nullptr; static int cap = 0;
    static hbuf::Group &keep = *new hbuf::Group;      // the armed buffers live as long as the process (the device globals point into them)
    HIPCHK(hipStreamSynchronize(H->stream));
    if (!buf) {
        hbuf::Group g; unsigned long long *b;
        if (g.dev(&b, (size_t)max_waves * LMZ_CLK_WORDS)) return RDA_ERR_HIP;
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_lmz_clk), &b, sizeof(b)));
        keep.d.push_back(std::move(g.d[0])); buf = b; cap = max_waves;
        return RDA_OK;
    }
    if (max_waves < 0) {          // the fail log instead: out = int[1 + 3 * 200000]; first call arms it
        static int *flog = nullptr;
        if (!flog) {
            hbuf::Group g; int *f;
            if (g.dev(&f, 1 + 3 * 200000)) return RDA_ERR_HIP;
            HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_lmz_faillog), &f, sizeof(f)));
            keep.d.push_back(std::move(g.d[0])); flog = f;
            return RDA_OK;
        }
        HIPCHK(hipMemcpy(out, flog, (1 + 3 * 200000) * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemset(flog, 0, sizeof(int)));
        return RDA_OK;
    }
    if (max_waves > cap) return RDA_ERR_ARG;
    HIPCHK(hipMemcpy(out, buf, (size_t)max_waves * LMZ_CLK_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(buf, 0, (size_t)cap * LMZ_CLK_WORDS * sizeof(unsigned long long)));
    return RDA_OK;
}
#endif
#ifdef RDA_LMZ_STATS
extern "C" int rda_debug_lmz_stats(rda_handle *H, unsigned *out)
{
    HIPCHK(hipStreamSynchronize(H->stream));
    HIPCHK(hipMemcpy(out, (char *)H->d.ctrl + offsetof(Ctrl, lmz_stat), 8 * sizeof(unsigned), hipMemcpyDeviceToHost));
    return RDA_OK;
}
#endif
extern "C" int rda_sync(rda_handle *H) { if (!H) return RDA_ERR_ARG; HIPCHK(hipStreamSynchronize(H->stream)); H->tick.pending_scene = 0; return RDA_OK; }

extern "C" int rda_fetch_result(rda_handle *H, int k, double *out_u, double *out_s, rda_info *info)
{
    if (!H || k < 0 || k >= H->trace.K) return RDA_ERR_ARG;
    const size_t ns = traj_s(H->d.c.T), nu = traj_u(H->d.c.T);
    HIPCHK(hipStreamSynchronize(H->stream));
    if (out_u) HIPCHK(hipMemcpy(out_u, H->trace.out_u + k * nu, nu * sizeof(double), hipMemcpyDeviceToHost));
    if (out_s) HIPCHK(hipMemcpy(out_s, H->trace.out_s + k * ns, ns * sizeof(double), hipMemcpyDeviceToHost));
    if (info) HIPCHK(hipMemcpy(info, H->trace.info + k, sizeof(rda_info), hipMemcpyDeviceToHost));
    return RDA_OK;
}

extern "C" int rda_timing_reset(rda_handle *H, int enable)
{
    if (!H) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(H->stream));
    HIPCHK(hipStreamSynchronize(H->stream2));
    H->timing = enable; H->ev_used[0] = H->ev_used[1] = H->ev_used[2] = H->ev_used[3] = 0;
    return RDA_OK;
}
extern "C" int rda_timing_read(rda_handle *H, int which, double *total_ms, int *launches)
{
    if (!H || which < 0 || which > 3) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(which == 3 ? H->stream2 : H->stream));
    double tot = 0; int n = 0;
    for (size_t i = 0; i + 1 < H->ev_used[which]; i += 2) {
        float ms = 0; HIPCHK(hipEventElapsedTime(&ms, H->ev[which][i], H->ev[which][i + 1]));
        tot += ms; ++n;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = n;
    return RDA_OK;
}

extern "C" int rda_timing_launches(rda_handle *H, int which, double *ms_out, int cap, int *launches)
{
    if (!H || which < 0 || which > 3 || (cap > 0 && !ms_out)) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(which == 3 ? H->stream2 : H->stream));
    int n = 0;
    for (size_t i = 0; i + 1 < H->ev_used[which]; i += 2, ++n) {
        if (n >= cap) continue;
        float ms = 0; HIPCHK(hipEventElapsedTime(&ms, H->ev[which][i], H->ev[which][i + 1]));
        ms_out[n] = ms;
    }
    if (launches) *launches = n;
    return RDA_OK;
}

// The dual state lives stage-major on the device ([T+1][N][.], [T][N]); the accessors speak the reference's shapes ([N][T+1][.],
// [N][T]): transposed on the host (test / checkpoint path, not the hot path)
static void tr_to_host(const std::vector<double> &dev, double *host, size_t N, size_t TT, size_t W)
{
    for (size_t n = 0; n < N; ++n) for (size_t t = 0; t < TT; ++t) memcpy(host + (n * TT + t) * W, dev.data() + (t * N + n) * W, W * sizeof(double));
}
static void tr_to_dev(const double *host, std::vector<double> &dev, size_t N, size_t TT, size_t W)
{
    for (size_t n = 0; n < N; ++n) for (size_t t = 0; t < TT; ++t) memcpy(dev.data() + (t * N + n) * W, host + (n * TT + t) * W, W * sizeof(double));
}
extern "C" int rda_get_state(rda_handle *H, double *lam, double *mu, double *z, double *xi, double *zeta,
                             double *dis, double *a_lam, double *b_lam)
{
    if (!H) return RDA_ERR_ARG;
    Dev &d = H->d; const size_t T = d.c.T, N = d.c.N, E = d.c.E, R = d.c.R;
    hbuf::Group g;                                      // the product temporaries, allocated before anything is written
    double *ta = nullptr, *tb = nullptr;
    if ((a_lam || b_lam) && (g.dev(&ta, N * (T + 1) * 2) || g.dev(&tb, N * (T + 1)))) return RDA_ERR_HIP;
    HIPCHK(hipStreamSynchronize(H->stream));
    std::vector<double> tmp;
    auto get = [&](const double *dev, double *host, size_t TT, size_t W) -> int {
        tmp.resize(N * TT * W);
        HIPCHK(hipMemcpy(tmp.data(), dev, N * TT * W * sizeof(double), hipMemcpyDeviceToHost));
        tr_to_host(tmp, host, N, TT, W);
        return RDA_OK;
    };
    if (lam && get(d.lam, lam, T + 1, E)) return RDA_ERR_HIP;
    if (mu && get(d.mu, mu, T + 1, R)) return RDA_ERR_HIP;
    if (z && get(d.z, z, T, 1)) return RDA_ERR_HIP;
    if (xi && get(d.xi, xi, T + 1, 2)) return RDA_ERR_HIP;
    if (zeta && get(d.zeta, zeta, T, 1)) return RDA_ERR_HIP;
    if (dis) HIPCHK(hipMemcpy(dis, d.dis, T * sizeof(double), hipMemcpyDeviceToHost));
    if (a_lam || b_lam) {
        hipLaunchKernelGGL(k_products_get, dim3(64), dim3(256), 0, H->stream, d, ta, tb);
        HIPCHK(hipStreamSynchronize(H->stream));
        if (a_lam) HIPCHK(hipMemcpy(a_lam, ta, N * (T + 1) * 2 * sizeof(double), hipMemcpyDeviceToHost));
        if (b_lam) HIPCHK(hipMemcpy(b_lam, tb, N * (T + 1) * sizeof(double), hipMemcpyDeviceToHost));
    }
    return RDA_OK;
}

extern "C" int rda_set_state(rda_handle *H, const double *lam, const double *mu, const double *z,
                             const double *xi, const double *zeta, const double *dis,
                             const double *a_lam, const double *b_lam)
{
    if (!H) return RDA_ERR_ARG;
    if (shard_frozen(H)) return RDA_ERR_UNSUPPORTED;
    Dev &d = H->d; const size_t T = d.c.T, N = d.c.N, E = d.c.E, R = d.c.R;
    hbuf::Group g;                                      // the product temporaries, allocated before anything is written
    double *ta = nullptr, *tb = nullptr;
    if ((a_lam && g.dev(&ta, N * (T + 1) * 2)) || (b_lam && g.dev(&tb, N * (T + 1)))) return RDA_ERR_HIP;
    HIPCHK(hipStreamSynchronize(H->stream));
    std::vector<double> tmp;
    auto put = [&](const double *host, double *dev, size_t TT, size_t W) -> int {
        tmp.resize(N * TT * W);
        tr_to_dev(host, tmp, N, TT, W);
        HIPCHK(hipMemcpy(dev, tmp.data(), N * TT * W * sizeof(double), hipMemcpyHostToDevice));
        return RDA_OK;
    };
    if (lam && put(lam, d.lam, T + 1, E)) return RDA_ERR_HIP;
    if (mu && put(mu, d.mu, T + 1, R)) return RDA_ERR_HIP;
    if (z && put(z, d.z, T, 1)) return RDA_ERR_HIP;
    if (xi && put(xi, d.xi, T + 1, 2)) return RDA_ERR_HIP;
    if (zeta && put(zeta, d.zeta, T, 1)) return RDA_ERR_HIP;
    if (dis) HIPCHK(hipMemcpy(d.dis, dis, T * sizeof(double), hipMemcpyHostToDevice));
    if (a_lam) HIPCHK(hipMemcpy(ta, a_lam, N * (T + 1) * 2 * sizeof(double), hipMemcpyHostToDevice));
    if (b_lam) HIPCHK(hipMemcpy(tb, b_lam, N * (T + 1) * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_products_set, dim3(64), dim3(256), 0, H->stream, d, ta, tb);
    int rc = terms_rebuild(H);                          // block sums / near masks of the rewritten terms
    HIPCHK(hipStreamSynchronize(H->stream));            // (before the temporaries go)
    return rc;
}


// ---- obstacle sharding ------------------------------------------------------------------------------
// shard slots past the last obstacle (N % P != 0): terms the su-problem must not see.  a = g = 0 and the offset `ee` so low that
// the hinge margin a'p - (blam + ee) - d is astronomically positive: never active, screened out, no rotation term, no residual.
__global__ void k_dead_slots(Dev d)
{
    const int T = d.c.T;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d.P * d.Nloc * T; i += gridDim.x * blockDim.x) {
        const int r = i / (d.Nloc * T), k = i % (d.Nloc * T), nl = k % d.Nloc;
        if (r * d.Nloc + nl >= d.c.N) { coef_arr(d, r, 3)[k] = -1e30; coef_arr(d, r, 8)[k] = -1e30; }      // (their block partials: zero sums, bit clear)
    }
}
extern "C" int rda_shard_config(rda_handle *H, int rank, int world)
{
    if (!H || world < 1 || rank < 0 || rank >= world) return RDA_ERR_ARG;
    if (H->d.c.N % world != 0 && !H->d.c.accelerated) return RDA_ERR_UNSUPPORTED;    // padded shards rely on the hinge of the accelerated cost
    if (world > 1 && H->opts.duals_follow) return RDA_ERR_UNSUPPORTED;               // duals_follow moves rows between slots = between ranks
    HIPCHK(hipStreamSynchronize(H->stream));
    Dev &d = H->d;
    const int Nloc = (d.c.N + world - 1) / world, first = rank * Nloc;
    const size_t chunk = chunk_doubles(d.c.T, Nloc), lchunk = lchunk_doubles(d.c.T, Nloc);
    hbuf::Group g;                                      // the new term arrays (zeroed) replace the old ones, and the geometry changes, only once both exist
    double *coef, *coefL;
    if (g.dev(&coef, chunk * world) || g.dev(&coefL, lchunk * world)) return RDA_ERR_HIP;
    H->terms = std::move(g); d.coef = coef; d.coefL = coefL;
    // su_pre = 0 (the su set-up evaluates every term itself) reads g = G'mu + xi of every slot, which lives in the LOCAL chunk and is
    // never gathered: with more than one rank the reduced form (block sums / near masks, part of the gathered chunk) is the only one
    if (world > 1) d.su_pre = 1;
    d.P = world; d.rank = rank; d.Nloc = Nloc; d.J = (Nloc + GS - 1) / GS; d.chunk = chunk; d.lchunk = lchunk;
    d.Nlive = first >= d.c.N ? 0 : (d.c.N - first < Nloc ? d.c.N - first : Nloc);
    if (d.Nloc * world != d.c.N) hipLaunchKernelGGL(k_dead_slots, dim3(64), dim3(256), 0, H->stream, d);
    int rc = terms_rebuild(H);                          // (the duals of a handle that is re-sharded are NOT re-condensed: shard before the first step)
    if (rc != RDA_OK) return rc;
    HIPCHK(hipStreamSynchronize(H->stream));
    return RDA_OK;
}
static void *rccl_sym(rda_handle *H, const char *name);
// ranks of the handle's communicator as RCCL counts them (ncclCommCount); 0 without a communicator
extern "C" int rda_shard_comm_count(rda_handle *H)
{
    if (!H) return RDA_ERR_ARG;
    if (!H->shard.comm) return 0;
    typedef int (*fn)(void *, int *);
    fn f = (fn)rccl_sym(H, "ncclCommCount");
    int n = 0;
    if (!f || f(H->shard.comm, &n) != 0) return RDA_ERR_HIP;
    return n;
}
extern "C" int rda_shard_chunk_doubles(rda_handle *H) { return H ? (int)H->d.chunk : RDA_ERR_ARG; }
extern "C" int rda_shard_get_chunk(rda_handle *H, double *host)
{
    if (!H || !host) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(H->stream));
    HIPCHK(hipMemcpy(host, H->d.coef + (size_t)H->d.rank * H->d.chunk, H->d.chunk * sizeof(double), hipMemcpyDeviceToHost));
    return RDA_OK;
}
extern "C" int rda_shard_set_chunks(rda_handle *H, const double *host_all)
{
    if (!H || !host_all) return RDA_ERR_ARG;
    HIPCHK(hipStreamSynchronize(H->stream));
    HIPCHK(hipMemcpy(H->d.coef, host_all, H->d.chunk * H->d.P * sizeof(double), hipMemcpyHostToDevice));
    return RDA_OK;
}
static void *rccl_sym(rda_handle *H, const char *name)
{
    if (!H->shard.lib) {
        // The RCCL the process ALREADY has, if any: a host that imported torch brought its own librccl.so.1 (and HIP runtime) with it,
        // and a second copy next to it breaks - default-visibility symbols of the second resolve into the first (measured:
        // ncclCommInitRank of /opt/rocm's copy fails with ncclUnhandledCudaError once torch's is mapped).  RTLD_NOLOAD matches by SONAME.
        H->shard.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!H->shard.lib) H->shard.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!H->shard.lib) H->shard.lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!H->shard.lib) H->shard.lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    }
    return H->shard.lib ? dlsym(H->shard.lib, name) : nullptr;
}
extern "C" int rda_shard_unique_id(rda_handle *H, void *out128)
{
    if (!H || !out128) return RDA_ERR_ARG;
    typedef int (*fn)(void *);
    fn f = (fn)rccl_sym(H, "ncclGetUniqueId");
    if (!f) return RDA_ERR_UNSUPPORTED;
    return f(out128) == 0 ? RDA_OK : RDA_ERR_HIP;
}
extern "C" int rda_shard_comm_init(rda_handle *H, const void *uid128)
{
    if (!H || !uid128 || H->d.P < 1) return RDA_ERR_ARG;     // a one-rank communicator is legal (plumbing check on a 1-GPU box)
    struct uid_t { char b[128]; } uid;
    memcpy(&uid, uid128, 128);
    typedef int (*init_fn)(void **, int, uid_t, int);
    init_fn f = (init_fn)rccl_sym(H, "ncclCommInitRank");
    H->shard.allgather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))rccl_sym(H, "ncclAllGather");
    H->shard.comm_destroy = (int (*)(void *))rccl_sym(H, "ncclCommDestroy");
    if (!f || !H->shard.allgather) return RDA_ERR_UNSUPPORTED;
    hbuf::Group g;                                      // the verdict word (zero) exists before the communicator does
    unsigned long long *verdict = H->shard.verdict;
    if (!verdict && g.pin(&verdict, 1)) return RDA_ERR_HIP;
    int rc = f(&H->shard.comm, H->d.P, uid, H->d.rank);
    if (rc != 0) { fprintf(stderr, "librda_hip: ncclCommInitRank failed (%d)\n", rc); H->shard.comm = nullptr; return RDA_ERR_HIP; }
    if (!H->shard.verdict) { H->shard.g = std::move(g); H->shard.verdict = verdict; }
    return RDA_OK;
}

// ---- host-driven ADMM iteration (exchange done by the caller: tests, gloo, MPI ...) -----------------------
extern "C" int rda_admm_begin(rda_handle *H, const double *nom_s, const double *nom_u, const double *ref_s, double ref_speed)
{
    if (!H || !nom_s || !nom_u || !ref_s) return RDA_ERR_ARG;
    H->stepped = 1;
    HIPCHK(hipStreamSynchronize(H->stream));
    { int rc = step_block_upload(H, nom_s, nom_u, ref_s, ref_speed); if (rc != RDA_OK) return rc; }
    hipLaunchKernelGGL(k_begin, dim3(1), dim3(64), 0, H->stream, H->d);
    HIPCHK(hipGetLastError());
    return RDA_OK;
}
extern "C" int rda_admm_su(rda_handle *H, int it, int *stopped)
{
    if (!H || it < 0) return RDA_ERR_ARG;
    const size_t T = H->d.c.T;
    H->admm_it = it;
    Dev d = H->d;
    const StepViews v = step_views(H);
    d.ref = v.ref; d.ref_speed = v.speed;
    RDA_SU_DISPATCH((int)T, hipLaunchKernelGGL(k_su<TT>, dim3(1), dim3(su::NT), H->su_lds, H->stream, d, it, v.s, v.u, Fin{}));
    HIPCHK(hipGetLastError());
    if (stopped) {
        Ctrl c;
        HIPCHK(hipMemcpyAsync(&c, d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, H->stream));
        HIPCHK(hipStreamSynchronize(H->stream));
        *stopped = c.stop;
    }
    return RDA_OK;
}
extern "C" int rda_admm_lammuz(rda_handle *H)
{
    if (!H) return RDA_ERR_ARG;
    Dev d = H->d;
    launch_lammuz(H, d, H->admm_it, Fin{});
    HIPCHK(hipGetLastError());
    return RDA_OK;
}
extern "C" int rda_admm_finish(rda_handle *H, double *out_u, double *out_s, rda_info *info)
{
    if (!H || !out_u || !out_s) return RDA_ERR_ARG;
    Dev d = H->d;
    { int rc = launch_finish(H, d, make_fin(H, H->res.out_u(), H->res.out_s(), H->res.info())); if (rc != RDA_OK) return rc; }
    { int rc = fetch_result(H); if (rc != RDA_OK) return rc; }
    result_out(H->res.blk.h, H->res.h_info(), H->d.c.T, out_u, out_s, info);
    return RDA_OK;
}

// ------------------------------------------------------------------------------------------------
// Fleet: B independent egos (BASELINE config C5) advanced by ONE set of launches per ADMM iteration.  Every member keeps
// its own handle (state, obstacles, trace) - the fleet only holds a device array of their `Dev` records and a table of
// per-ego input / output locations.  The grid gets an ego dimension: k_su runs B workgroups (one CU each) side by side,
// k_lammuz B * N*T/4 workgroups, so the launch fills the 256 CUs that a single ego cannot.
struct EgoIO {            // base pointers, indexed by the step number k inside the kernels
    const double *s, *u, *ref, *speed; double *out_u, *out_s; rda_info *info;
};


template <int TT> __global__ __launch_bounds__(su::NT) void k_su_fleet(const Dev *devs, const EgoIO *io, int it, int k)
{
    const Dev &d = devs[blockIdx.x];
    const EgoIO e = io[blockIdx.x];
    const size_t ns = 3 * (d.c.T + 1), nu = 2 * d.c.T;
    su_body<TT>(d, it, e.s + k * ns, e.u + k * nu, e.ref + k * ns, e.speed + k);
}

// Enumeration mode: the fleet uses the packed kernels only when every member can - a member without obstacles (Q9) or of a shape the packed body does
// not take puts the whole fleet on the one-per-wave kernel (lmzplan::fleet; the forms agree bit for bit).  Member d's result locations of step k:
__device__ __forceinline__ Fin fleet_fin(const Dev &d, const EgoIO &e, int k)
{
    const size_t ns = 3 * (d.c.T + 1), nu = 2 * d.c.T;
    return Fin{ e.out_u + k * nu, e.out_s + k * ns, e.info + k, nullptr, 0, 0 };
}
__global__ __launch_bounds__(256) void k_lammuz_fleet(const Dev *devs, int it) { lammuz_body(devs[blockIdx.y], blockIdx.x, it); }
__global__ __launch_bounds__(64 * GS / 4, 2) void k_lammuz_fleet_rows(const Dev *devs, const EgoIO *io, int it, int k)
{
    lammuz_body_rows<0>(devs[blockIdx.y], blockIdx.x, gridDim.x, it, fleet_fin(devs[blockIdx.y], io[blockIdx.y], k));
}
#ifndef LMZ_FLEET_FAST_OCC
#define LMZ_FLEET_FAST_OCC 3
#endif
__global__ __launch_bounds__(64 * GS / 4, LMZ_FLEET_FAST_OCC) void k_lammuz_fleet_rows_fast(const Dev *devs, int it) { lammuz_body_rows<1>(devs[blockIdx.y], blockIdx.x, gridDim.x, it, Fin{}); }
__global__ __launch_bounds__(64 * GS / 4, 1) void k_lammuz_fleet_enum(const Dev *devs, int it) { lammuz_body_rows<2>(devs[blockIdx.y], blockIdx.x, gridDim.x, it, Fin{}); }
// Interior-point mode: the launch form is chosen PER MEMBER by the rule of a solo handle (lmzplan::member_ip_rows) - the row-parallel kernel for a member whose
// shape it takes (Dev::ip_rows) and that has staged obstacles, else the per-thread kernel (with its quirk-Q9 branch) + k_lmz_finalize_fleet.  The two kernels agree
// only to ~4e-6, so a fleet-wide choice would make a member's result depend on its neighbours.  A kernel of one form returns at once for the members of the other; the
// host launches only the forms some member needs (lmzplan::fleet).
using lmzplan::member_ip_rows;
#ifndef LMZ_FLEET_IP_OCC
#define LMZ_FLEET_IP_OCC 1
#endif
__global__ __launch_bounds__(64 * GS / 4, LMZ_FLEET_IP_OCC) void k_lammuz_ip_fleet(const Dev *devs, int it)
{
    const Dev &d = devs[blockIdx.y];
    if (!member_ip_rows(d)) return;
    lammuz_ip_body(d, blockIdx.x, it, Fin{});
}
__global__ __launch_bounds__(64) void k_lammuz_cp_fleet_small(const Dev *devs)      // E, R <= 4
{
    const Dev &d = devs[blockIdx.y];
    if (member_ip_rows(d)) return;
    lammuz_cp_body<16, 24>(d, blockIdx.x);
}
__global__ __launch_bounds__(64) void k_lammuz_cp_fleet_large(const Dev *devs)      // E, R <= 8
{
    const Dev &d = devs[blockIdx.y];
    if (member_ip_rows(d)) return;
    lammuz_cp_body<24, 36>(d, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_lmz_finalize_fleet(const Dev *devs, const EgoIO *io, int it, int k)
{
    if (member_ip_rows(devs[blockIdx.y])) return;      // (the row-parallel interior-point kernel made this member's block partials: the solo path launches no k_lmz_finalize behind it)
    finalize_body(devs[blockIdx.y], blockIdx.x, gridDim.x, it, fleet_fin(devs[blockIdx.y], io[blockIdx.y], k));
}

__global__ __launch_bounds__(su::NT) void k_finish_fleet(const Dev *devs, const EgoIO *io, int k)
{
    const Dev &d = devs[blockIdx.x];
    const EgoIO e = io[blockIdx.x];
    finish_body(d, fleet_fin(d, e, k));
}

// The table sets a fleet makes on first use.  Each owns its allocations (g: zeroed, counted) beside the views into them - a device array with its pinned
// mirror (hbuf::Pair) or a plain pointer where only one side exists - and is built beside the fleet (alloc: all or RDA_ERR_HIP).  The call that needs a set
// moves it in (FleetReserve) only when it can no longer be refused: a refused allocation leaves the fleet as it was.  have(): allocated; size(): the
// elements of a set that is regrown when a call needs more.
struct FleetTrack {                       // tracked stepping (device-side pre_process): rda_fleet_step_tracked, the rollouts
    hbuf::Group g; hbuf::Pair<track::In> in; hbuf::Pair<track::Out> out; hbuf::Pair<double *> paths; hbuf::Pair<int> lens; hbuf::Pair<EgoIO> io;
    int alloc(size_t B) { return (in.alloc(g, B) | out.alloc(g, B) | paths.alloc(g, B) | lens.alloc(g, B) | io.alloc(g, B)) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return in.d != nullptr; }
};
struct FleetResort {                      // rda_fleet_scene_resort, the rollouts: the members' scene arguments, their robots' positions [B][2]
    hbuf::Group g; hbuf::Pair<scene::Args> sc; hbuf::Pair<double> rob;
    int alloc(size_t B) { return (sc.alloc(g, B) | rob.alloc(g, 2 * B)) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return sc.d != nullptr; }
};
// fleet lidar (rda_fleet_scan_boxes / rda_fleet_upload_scans): per member the scan kernel's arguments, the fill kernel's and the conversion kernels'; the
// boxes of the last scans [B][MAXB][4][2] on the device; pinned, read / written by the kernel itself: the concatenated ranges [B * MAXB], the counters [B][2]
struct FleetLidar {
    hbuf::Group g; hbuf::Pair<lidar::Args> args; hbuf::Pair<lidar::Fill> fill; hbuf::Pair<scene::Args> sc;
    double *d_boxes = nullptr, *h_ranges = nullptr; int *h_count = nullptr;
    int alloc(size_t B)
    {
        return (args.alloc(g, B) | fill.alloc(g, B) | sc.alloc(g, B) | g.dev(&d_boxes, B * lidar::MAXB * 8) | g.pin(&h_ranges, B * lidar::MAXB) |
                g.pin(&h_count, 2 * B)) ? RDA_ERR_HIP : RDA_OK;
    }
    bool have() const { return d_boxes != nullptr; }
};
struct FleetLidarHost {                   // for rda_fleet_scan_boxes alone: the host's copy of labels and boxes (pinned, written by the kernel)
    hbuf::Group g; double *h_boxes = nullptr; int *h_labels = nullptr;
    int alloc(size_t B) { return (g.pin(&h_boxes, B * lidar::MAXB * 8) | g.pin(&h_labels, B * lidar::MAXB)) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return h_boxes != nullptr; }
};
// Tracked fleet lidar (rda_fleet_upload_scans_tracked, rda_fleet_rollout_lidar_tracked, rda_fleet_track_boxes): lidar::k_track_boxes_fleet's member table and
// every member's resident table of tracks, double-buffered - buffer `par` holds the tracks as the last tracked tick left them, the kernel writes the other
// one and the host switches when the tick goes through.  Per buffer and member: the count, per track its length, its history [MAX_TRACKS][8][2] and the
// velocity its box got; vel [B][MAXB][2]: every box's velocity of the last launch, what the fill kernel reads.  Device memory comes zeroed: no tracks.
struct FleetTracks {
    hbuf::Group g; hbuf::Pair<lidar::Track> tab;
    int *cnt = nullptr, *len = nullptr, *h_cnt = nullptr, *h_len = nullptr; double *hist = nullptr, *tvel = nullptr, *vel = nullptr, *h_hist = nullptr, *h_tvel = nullptr;
    int par = 0;
    int alloc(size_t B)
    {
        const size_t M = lidar::MAX_TRACKS;
        return (tab.alloc(g, B) | g.dev(&cnt, 2 * B) | g.dev(&len, 2 * B * M) | g.dev(&hist, 2 * B * M * lidar::TRK_HIST * 2) | g.dev(&tvel, 2 * B * M * 2) |
                g.dev(&vel, B * lidar::MAXB * 2) | g.pin(&h_cnt, B) | g.pin(&h_len, B * M) | g.pin(&h_hist, B * M * lidar::TRK_HIST * 2) |
                g.pin(&h_tvel, B * M * 2)) ? RDA_ERR_HIP : RDA_OK;
    }
    bool have() const { return cnt != nullptr; }
};
// the rollouts: the advance kernel's member table, the io tables of tick 0 | of the later ticks [2][B] (results in the fleet's `out` whatever the members'
// zero_copy says)
struct FleetRollTables {
    hbuf::Group g; hbuf::Pair<rollout::Member> m; hbuf::Pair<EgoIO> io;
    int alloc(size_t B) { return (m.alloc(g, B) | io.alloc(g, 2 * B)) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return m.d != nullptr; }
};
struct RollLayout { size_t states, u, endh, last, info, index, arrived, bytes; };      // byte offsets of the log block's parts (rollout::Logs; last [B][res_info]: the last tick's u | s)
static RollLayout roll_layout(size_t K, size_t B, size_t T)
{
    RollLayout l;
    l.states = 0; l.u = l.states + (K + 1) * B * 3 * sizeof(double); l.endh = l.u + K * B * 2 * sizeof(double); l.last = l.endh + B * sizeof(double);
    l.info = l.last + B * res_info(T) * sizeof(double);
    l.index = l.info + K * B * sizeof(rda_info); l.arrived = l.index + K * B * sizeof(int); l.bytes = l.arrived + B * sizeof(int);
    return l;
}
struct FleetRollLog {                     // the rollouts' log block of `cap` ticks (roll_layout), regrown for a longer rollout
    hbuf::Group g; hbuf::Pair<char> log; int cap = 0;
    int alloc(int K, size_t B, size_t T) { cap = K; return log.alloc(g, roll_layout((size_t)K, B, T).bytes) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return log.d != nullptr; }
    size_t size() const { return (size_t)cap; }
};
// rda_fleet_rollout_moving, rda_fleet_clearance: per member the move kernel's and the clearance kernel's arguments, the members' scene arguments as they
// stand (resort = 0: slots rebuilt in the staged order), the states of rda_fleet_clearance [B][3]
struct FleetMove {
    hbuf::Group g; hbuf::Pair<scene::Move> mv; hbuf::Pair<rollout::Clear> cl; hbuf::Pair<scene::Args> sc; hbuf::Pair<double> st;
    int alloc(size_t B) { return (mv.alloc(g, B) | cl.alloc(g, B) | sc.alloc(g, B) | st.alloc(g, 3 * B)) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return mv.d != nullptr; }
};
struct FleetSnapshot {                    // rda_fleet_rollout_moving: the snapshot of all members' raw geometry (cap doubles), regrown when a call needs more
    hbuf::Group g; double *d = nullptr; size_t cap = 0;
    int alloc(size_t n) { cap = n; return g.dev(&d, n) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return d != nullptr; }
    size_t size() const { return cap; }
};
struct FleetDoubles {                     // v.n doubles, regrown when a call needs more: the clearance log [K][B] | the ranges of the last ray cast
    hbuf::Group g; hbuf::Pair<double> v;
    int alloc(size_t n) { return v.alloc(g, n) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return v.d != nullptr; }
    size_t size() const { return v.n; }
};
// members as each other's obstacles (rda_fleet_*_peers, rda_fleet_peer_clearance): the peer table, the states [B][3] and the controls [B][2] of a host-driven
// refresh or of a rollout's tick 0
struct FleetPeers {
    hbuf::Group g; hbuf::Pair<scene::Peer> tab; hbuf::Pair<double> st, ctl;
    int alloc(size_t B) { return (tab.alloc(g, B) | st.alloc(g, 3 * B) | ctl.alloc(g, 2 * B)) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return tab.d != nullptr; }
};
// peers predicted along their plans (rda_fleet_*_peers_plan): the plans [B][3][T+1] and their validity [B] of a host-driven call or of a rollout's tick 0
struct FleetPlan {
    hbuf::Group g; hbuf::Pair<double> plan; hbuf::Pair<int> valid;
    int alloc(size_t B, size_t T) { return (plan.alloc(g, B * traj_s(T)) | valid.alloc(g, B)) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return plan.d != nullptr; }
};
// the gear rollout (rda_fleet_rollout_gears): per member the record of its resident pieces; the tables the tracker and the advance kernel share - the piece in
// force and what k_track_fleet reads as the member's path and length [B] (the rollout's own: trk.paths / lens keep the rda_upload_path paths)
struct FleetGears {
    hbuf::Group g; hbuf::Pair<rollout::Gears> rec; hbuf::Pair<int> piece, lens; hbuf::Pair<double *> paths;
    int alloc(size_t B) { return (rec.alloc(g, B) | piece.alloc(g, B) | lens.alloc(g, B) | paths.alloc(g, B)) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return rec.d != nullptr; }
};
struct FleetInts {                        // v.n ints, regrown when a call needs more: the piece log [K][B]
    hbuf::Group g; hbuf::Pair<int> v;
    int alloc(size_t n) { return v.alloc(g, n) ? RDA_ERR_HIP : RDA_OK; }
    bool have() const { return v.d != nullptr; }
    size_t size() const { return v.n; }
};
// The members' resident WORLDS (rda_fleet_upload_worlds): what the simulated sensor sees (lidar::k_raycast_fleet), apart from the raw scenes that a lidar
// tick overwrites with boxes.  Member-major geometry [total][e][2], its snapshot of the same size (rda_fleet_rollout_lidar, moving), velocities, kinds,
// vertex counts; off[i]: member i's first obstacle.  Per member the ray caster's, the move kernel's and the clearance kernel's arguments and the poses of
// rda_fleet_raycast [B][3].
struct FleetWorld {
    hbuf::Group g; double *geom = nullptr, *base = nullptr, *vel = nullptr; int *kind = nullptr, *nvert = nullptr; int e = 0; size_t total = 0;
    std::vector<int> counts; std::vector<size_t> off;
    hbuf::Pair<lidar::Ray> ray; hbuf::Pair<scene::Move> mv; hbuf::Pair<rollout::Clear> cl; hbuf::Pair<double> st;
    int alloc(size_t B, const int32_t *member_counts, int we)
    {
        e = we; counts.assign(member_counts, member_counts + B); off.assign(B, 0);
        for (size_t i = 1; i < B; ++i) off[i] = off[i - 1] + (size_t)counts[i - 1];
        total = off[B - 1] + (size_t)counts[B - 1];
        const size_t nt = total ? total : 1;              // (an all-empty fleet still gets buffers to point at)
        return (g.dev(&geom, nt * e * 2) | g.dev(&base, nt * e * 2) | g.dev(&vel, nt * 2) | g.dev(&kind, nt) | g.dev(&nvert, nt) |
                ray.alloc(g, B) | mv.alloc(g, B) | cl.alloc(g, B) | st.alloc(g, 3 * B)) ? RDA_ERR_HIP : RDA_OK;
    }
    bool have() const { return geom != nullptr; }
};

// the on-demand sets a fleet holds - and a FleetReserve, one empty set of each, builds beside it
struct FleetSets {
    FleetTrack trk; FleetResort res;
    FleetLidar li; FleetLidarHost li_host; FleetTracks tk;
    FleetRollTables ro; FleetRollLog ro_log;
    FleetMove mov; FleetSnapshot snap; FleetDoubles cl_log;      // cl_log: the clearance log
    FleetWorld world; FleetDoubles rays;                          // rays: the ranges of the last ray cast
    FleetPeers pe; FleetDoubles pc_log;                           // pc_log: the peer clearance log
    FleetPlan pl;
    FleetGears gr; FleetInts gr_log; FleetDoubles gr_endh;        // gr_endh: the pieces' end headings
    template <typename Fn> static void each(Fn f)                 // f(&FleetSets::set) for every set
    {
        f(&FleetSets::trk); f(&FleetSets::res); f(&FleetSets::li); f(&FleetSets::li_host); f(&FleetSets::tk); f(&FleetSets::ro); f(&FleetSets::ro_log);
        f(&FleetSets::mov); f(&FleetSets::snap); f(&FleetSets::cl_log); f(&FleetSets::world); f(&FleetSets::rays); f(&FleetSets::pe); f(&FleetSets::pc_log);
        f(&FleetSets::pl); f(&FleetSets::gr); f(&FleetSets::gr_log); f(&FleetSets::gr_endh);
    }
};
struct rda_fleet : FleetSets {            // (owns its buffers, event and stream like rda_handle; the sets outlive the stream)
    int B;
    std::vector<rda_handle *> egos;
    hbuf::Group mem;                      // what rda_fleet_create makes:
    hbuf::Pair<Dev> devs;                 // the members' records
    EgoIO *h_io, *d_io_step, *d_io_trace;
    hbuf::Pair<double> in;                // step path, per ego: a step block (step_doubles)
    hbuf::Pair<double> out;               // per ego: u | s, the head of a result block (res_info doubles)
    hbuf::Pair<rda_info> info;
    int T, iter_num, J;
    char lmz_name[lmzplan::NAME_CAP] = "";    // what rda_fleet_lammuz_kernel last returned
    size_t su_lds;
    int rob_pending;                      // a copy out of res.rob.h may be queued
    double scan_split = 0.0;              // rda_fleet_set_scan_split: lidar::Args::split_tol of every member's scan in the fleet's calls
    int roll_K;                           // the ticks of the rollout whose logs are on the host
    std::vector<int> n_own;               // every member's own obstacles as the last peers upload staged them
    int gear_total;                       // the pieces of all members of the gear rollout whose logs are on the host (0: none)
    hbuf::Event ev;
    hbuf::Stream stream;                  // (last: destroyed first)
};

// The wait for the fleet's stream: nothing is queued behind it, so no copy out of res.rob.h either.  consumed: the call was a step or a rollout - the
// members' staged scenes have been consumed.
static hipError_t fleet_wait(rda_fleet *F, bool consumed = false)
{
    const hipError_t e = hipStreamSynchronize(F->stream);
    if (e != hipSuccess) return e;
    F->rob_pending = 0;
    if (consumed) for (rda_handle *H : F->egos) H->tick.pending_scene = 0;
    return e;
}
// The refresh of a pinned mirror, in its two halves; get(i): record i as it should be now.  mirror_differs: does any record differ from the mirror?
// mirror_upload: the mirror rewritten and pushed.  Between the two comes fleet_wait (an earlier copy out of the mirror may still be queued): fleet_table for
// one table; where one wait covers several tables the caller asks about all of them first.
template <typename T, typename Get> static bool mirror_differs(const hbuf::Pair<T> &p, Get get)
{
    for (size_t i = 0; i < p.n; ++i) { const T &r = get(i); if (memcmp(&r, &p.h[i], sizeof(T)) != 0) return true; }
    return false;
}
template <typename T, typename Get> static hipError_t mirror_upload(const hbuf::Pair<T> &p, Get get, hipStream_t stream)
{
    for (size_t i = 0; i < p.n; ++i) { const T &r = get(i); memcpy((void *)&p.h[i], &r, sizeof(T)); }
    return p.push(stream);
}
template <typename T> static auto records(const std::vector<T> &v) { return [&v](size_t i) -> const T & { return v[i]; }; }
static auto member_devs(const rda_fleet *F) { return [F](size_t i) -> const Dev & { return F->egos[i]->d; }; }
static auto member_paths(const rda_fleet *F) { return [F](size_t i) { return F->egos[i]->path.d; }; }
static auto member_lens(const rda_fleet *F) { return [F](size_t i) { return F->egos[i]->path.len; }; }
// one table: uploaded when it differs from what the device holds
template <typename T, typename Get> static int fleet_table(rda_fleet *F, const hbuf::Pair<T> &p, Get get)
{
    if (!mirror_differs(p, get)) return RDA_OK;
    HIPCHK(fleet_wait(F));
    HIPCHK(mirror_upload(p, get, F->stream));
    return RDA_OK;
}

// What a call builds beside the fleet before it changes anything: one empty set of each kind.  need / grow / fresh allocate what the fleet lacks (alloc's
// arguments follow the set) and remember a refusal.  adopt, once the call has asked for everything: RDA_ERR_HIP after a refusal - what was built goes with
// the call, the fleet is as it was - else the sets move in.  It is the only place where a set of the fleet is assigned.
struct FleetReserve {
    rda_fleet *F; FleetSets s; int refused = 0;
    explicit FleetReserve(rda_fleet *fleet) : F(fleet) {}
    template <typename S, typename... A> void need(S FleetSets::*m, A... a) { if (!(F->*m).have()) refused |= (s.*m).alloc(a...); }                 // this set
    template <typename S, typename... A> void grow(S FleetSets::*m, size_t n, A... a) { if (n > (F->*m).size()) refused |= (s.*m).alloc(a...); }    // ... of at least n elements
    template <typename S, typename... A> void fresh(S FleetSets::*m, A... a) { refused |= (s.*m).alloc(a...); }                                     // a new one in its place
    void need_lidar(bool host_copy)                     // the lidar block (the first one raises the scan kernels' LDS limit) and, host_copy, the host's copies
    {
        need(&FleetSets::li, (size_t)F->B);
        if (s.li.have() && (hipFuncSetAttribute((const void *)lidar::k_scan_fleet, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lidar::LDS_BYTES) != hipSuccess ||
                            hipFuncSetAttribute((const void *)lidar::k_scan_fleet_at, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lidar::LDS_BYTES) != hipSuccess))
            refused = 1;
        if (host_copy) need(&FleetSets::li_host, (size_t)F->B);
    }
    // what every rollout reserves before its first tick: the tracker's tables, the rollout tables, a log block of K ticks and (clearance) a clearance log
    void need_rollout(int K, bool clearance)
    {
        const size_t B = F->B;
        need(&FleetSets::trk, B); need(&FleetSets::ro, B); grow(&FleetSets::ro_log, (size_t)K, K, B, (size_t)F->T);
        if (clearance) grow(&FleetSets::cl_log, (size_t)K * B, (size_t)K * B);
    }
    int bad() const { return refused ? RDA_ERR_HIP : RDA_OK; }
    // the set a call that runs before it adopts works on: the fleet's, or the one built here
    template <typename S> S &now(S FleetSets::*m) { return (s.*m).have() ? s.*m : F->*m; }
    // Whatever was built moves in.  The wait comes first where a set the fleet holds is replaced - the old block may be in flight, and it is freed here - and
    // where the caller goes on to rewrite pinned tables unconditionally (rewrites); a first-use set needs none.
    int adopt(bool rewrites = false)
    {
        if (refused) return RDA_ERR_HIP;
        bool wait = rewrites;
        FleetSets::each([&](auto m) { if ((s.*m).have() && (F->*m).have()) wait = true; });
        if (wait) HIPCHK(fleet_wait(F));
        FleetSets::each([&](auto m) { if ((s.*m).have()) F->*m = std::move(s.*m); });
        return RDA_OK;
    }
};

// Member i's locations on the step path: its step block in `in` (in_u: nominal controls that live elsewhere, else null), its u | s block
// under out_base, its info under info_base
static EgoIO fleet_member_io(const rda_fleet *F, size_t i, const double *in_u, double *out_base, rda_info *info_base)
{
    const size_t T = F->T;
    EgoIO e;
    e.s = F->in.d + i * step_doubles(T); e.u = in_u ? in_u : e.s + step_u(T); e.ref = e.s + step_ref(T); e.speed = e.s + step_speed(T);
    e.out_u = out_base + i * res_info(T); e.out_s = e.out_u + res_s(T); e.info = info_base + i;
    return e;
}
// member i's finished step out of the fleet's pinned blocks, into the per-ego arrays of rda_step, concatenated
static void fleet_result_out(const rda_fleet *F, size_t i, double *out_u, double *out_s, rda_info *info)
{
    const size_t T = F->T;
    result_out(F->out.h + i * res_info(T), F->info.h + i, T, out_u + i * traj_u(T), out_s + i * traj_s(T), info ? info + i : nullptr);
}

extern "C" void rda_fleet_destroy(rda_fleet *F)
{
    if (!F) return;
    (void)hipStreamSynchronize(F->stream);
    delete F;
}

extern "C" int rda_fleet_create(rda_handle *const *egos, int B, rda_fleet **out)
{
    if (!egos || B < 1 || !out) return RDA_ERR_ARG;
    for (int i = 0; i < B; ++i) {
        if (!egos[i]) return RDA_ERR_ARG;
        const rda_cfg &a = egos[0]->d.c, &b = egos[i]->d.c;
        // one grid for all members: the problem SHAPE must agree (weights, bounds, kinematics and robots may differ)
        if (a.T != b.T || a.N != b.N || a.E != b.E || a.R != b.R || a.iter_num != b.iter_num) return RDA_ERR_UNSUPPORTED;
        if (egos[i]->shard.comm || egos[i]->d.P != 1) return RDA_ERR_UNSUPPORTED;  // egos are replicas, obstacle shards are not
        if (b.robot_norm2) return RDA_ERR_UNSUPPORTED;                             // (no enumeration candidates, no clearance form: out of scope)
        if ((egos[i]->d.lmz_mode != 0) != (egos[0]->d.lmz_mode != 0)) return RDA_ERR_UNSUPPORTED;      // one LamMuZ mode per fleet (lmz_mu may differ)
    }
    std::unique_ptr<rda_fleet> owner(new rda_fleet());     // a failure on the way drops the fleet and with it what was built
    rda_fleet *F = owner.get();
    F->B = B; F->egos.assign(egos, egos + B);
    const rda_cfg &c = egos[0]->d.c;
    F->T = c.T; F->iter_num = c.iter_num; F->J = (c.N + GS - 1) / GS; F->su_lds = egos[0]->su_lds;
    HIPCHK(hipStreamCreate(F->stream.out()));
    HIPCHK(hipEventCreateWithFlags(F->ev.out(), hipEventDisableTiming));
    const size_t T = c.T, nin = step_doubles(T), nout = res_info(T);
    hbuf::Group &m = F->mem;
    if (F->devs.alloc(m, (size_t)B) | F->in.alloc(m, B * nin) | F->out.alloc(m, B * nout) | F->info.alloc(m, (size_t)B) |
        m.dev(&F->d_io_step, (size_t)B) | m.dev(&F->d_io_trace, (size_t)B) | m.pin(&F->h_io, (size_t)B)) return RDA_ERR_HIP;
    for (int i = 0; i < B; ++i) F->h_io[i] = fleet_member_io(F, i, nullptr, F->out.d, F->info.d);
    HIPCHK(hipMemcpy(F->d_io_step, F->h_io, B * sizeof(EgoIO), hipMemcpyHostToDevice));
    RDA_SU_DISPATCH((int)T, HIPCHK(hipFuncSetAttribute((const void *)k_su_fleet<TT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)F->su_lds)));
    HIPCHK(hipFuncSetAttribute((const void *)k_finish_fleet, hipFuncAttributeMaxDynamicSharedMemorySize, (int)F->su_lds));
    *out = owner.release();
    return RDA_OK;
}

// the LamMuZ launches of an ADMM iteration that the members allow together, as they stand now (their host records: what the next upload of F->devs
// carries, and what the last one carried wherever a step is enqueued)
static lmzplan::Plan fleet_lmz_plan(const rda_fleet *F)
{
    return lmzplan::fleet(F->B, [F](int i) { return lmz_member(F->egos[i], F->egos[i]->d); });
}
// the LamMuZ launches of the next tick as the members stand now (kernel names joined by '+')
extern "C" const char *rda_fleet_lammuz_kernel(rda_fleet *F)
{
    if (!F) return "";
    lmzplan::name(fleet_lmz_plan(F), true, F->lmz_name, sizeof F->lmz_name);
    return F->lmz_name;
}

// members' records (obstacle count, staged pointers, weights may have changed since the last call) -> device; the fleet
// stream then waits for whatever the members still have in flight on their own streams (obstacle uploads)
static int fleet_refresh(rda_fleet *F)
{
    for (int i = 0; i < F->B; ++i) {
        // the fleet's stream must run behind whatever a member still has queued on its OWN stream (an upload, a solo step).  An idle member stream needs no
        // edge: the event record + wait pair per member cost ~8 us of host time each, twice per fleet tick (re-sort + step) = 1 ms of a 4.2 ms tick of the
        // 64-ego closed loop with the GPU idle meanwhile (rocprofv3 kernel trace cut into ticks, tools/experiments/fleet_tick_trace.sh, round 6)
        const hipError_t q = hipStreamQuery(F->egos[i]->stream);
        if (q == hipSuccess) continue;
        if (q != hipErrorNotReady) { fprintf(stderr, "librda_hip: hipStreamQuery failed: %s (%s:%d)\n", hipGetErrorString(q), __FILE__, __LINE__); return RDA_ERR_HIP; }
        (void)hipGetLastError();                            // ("not ready" is an answer, not an error to be found by a later hipGetLastError)
        HIPCHK(hipEventRecord(F->ev, F->egos[i]->stream));
        HIPCHK(hipStreamWaitEvent(F->stream, F->ev, 0));
    }
    return fleet_table(F, F->devs, member_devs(F));
}

static int fleet_enqueue(rda_fleet *F, const EgoIO *io, int k)
{
    const int B = F->B;
    const Dev *devs = F->devs.d;
    const lmzplan::Plan p = fleet_lmz_plan(F);
    for (int it = 0; it < F->iter_num; ++it) {          // iteration 0 resets every member's control block (su_body)
        RDA_SU_DISPATCH(F->T, hipLaunchKernelGGL(k_su_fleet<TT>, dim3(B), dim3(su::NT), F->su_lds, F->stream, devs, io, it, k));
        for (int i = 0; i < p.n; ++i) {
            const dim3 grid(p.l[i].grid, B), block(p.l[i].block);
            // one case per kernel id, as in launch_lammuz: the fleet kernel of that name with its argument list
#define LMZ_FLEET(ID, KERNEL, ...) case lmzplan::ID: static_assert(lmzplan::same(lmzplan::NAMES[lmzplan::ID].fleet, #KERNEL), #KERNEL); \
                                   hipLaunchKernelGGL(KERNEL, grid, block, 0, F->stream, __VA_ARGS__); break;
            switch (p.l[i].kernel) {
                LMZ_FLEET(ROWS, k_lammuz_fleet_rows, devs, io, it, k)
                LMZ_FLEET(ROWS_FAST, k_lammuz_fleet_rows_fast, devs, it)
                LMZ_FLEET(ENUM, k_lammuz_fleet_enum, devs, it)
                LMZ_FLEET(WAVE, k_lammuz_fleet, devs, it)
                LMZ_FLEET(IP, k_lammuz_ip_fleet, devs, it)
                LMZ_FLEET(CP_SMALL, k_lammuz_cp_fleet_small, devs)
                LMZ_FLEET(CP_LARGE, k_lammuz_cp_fleet_large, devs)
                LMZ_FLEET(FINALIZE, k_lmz_finalize_fleet, devs, io, it, k)
                case lmzplan::ROWS_DENSE: break;                       // (no fleet kernel: lmzplan::fleet plans none)
            }
#undef LMZ_FLEET
        }
    }
    hipLaunchKernelGGL(k_finish_fleet, dim3(B), dim3(su::NT), F->su_lds, F->stream, devs, io, k);
    HIPCHK(hipGetLastError());
    return RDA_OK;
}

// one synchronous MPC step of every member: inputs / outputs are the per-ego arrays of rda_step, concatenated
extern "C" int rda_fleet_step(rda_fleet *F, const double *nom_s, const double *nom_u, const double *ref_s, const double *ref_speed,
                              double *out_u, double *out_s, rda_info *info)
{
    if (!F || !nom_s || !nom_u || !ref_s || !ref_speed || !out_u || !out_s) return RDA_ERR_ARG;
    const size_t T = F->T, ns = traj_s(T), nu = traj_u(T), nin = step_doubles(T), B = F->B;
    for (size_t i = 0; i < B; ++i) {
        double *q = F->in.h + i * nin;
        memcpy(q, nom_s + i * ns, ns * sizeof(double)); memcpy(q + step_u(T), nom_u + i * nu, nu * sizeof(double));
        memcpy(q + step_ref(T), ref_s + i * ns, ns * sizeof(double)); q[step_speed(T)] = ref_speed[i];
    }
    int rc = fleet_refresh(F);
    if (rc != RDA_OK) return rc;
    HIPCHK(F->in.push(F->stream));
    rc = fleet_enqueue(F, F->d_io_step, 0);
    if (rc != RDA_OK) return rc;
    HIPCHK(F->out.pull(F->stream, F->out.n));
    HIPCHK(F->info.pull(F->stream, B));
    HIPCHK(fleet_wait(F, true));
    for (size_t i = 0; i < B; ++i) fleet_result_out(F, i, out_u, out_s, info);
    return RDA_OK;
}

// device-side pre_process of every member (one wave per ego), then the fleet step on what it wrote
__global__ void k_track_fleet(const Dev *devs, const EgoIO *io, const track::In *ins, double *const *paths, const int *lens,
                              track::Out *outs, int B)
{
    __shared__ double win[track::LDS_DOUBLES];
    const int b = blockIdx.x;
    if (b >= B) return;
    const Dev &d = devs[b];
    track::Ego e;
    e.path = paths[b]; e.L = lens[b]; e.nom_u = io[b].u; e.nom_s = const_cast<double *>(io[b].s); e.ref = const_cast<double *>(io[b].ref);
    e.speed = const_cast<double *>(io[b].speed);
    e.T = d.c.T; e.dynamics = d.c.dynamics; e.dt = d.c.dt; e.wheelbase = d.c.L;
    track::run(e, ins[b], outs[b], win, threadIdx.x);
}

// What the entries ask of the members.  An entry whose rules interleave per member (member 0's second rule in front of member 1's first) spells them out.
// no member is inside a tick of its own (else RDA_ERR_ARG)
static bool fleet_members_idle(const rda_fleet *F) { for (const rda_handle *H : F->egos) if (H->tick.pending) return false; return true; }
// some member has rda_opts::duals_follow (RDA_ERR_UNSUPPORTED: k_follow_* are per member)
static bool fleet_duals_follow(const rda_fleet *F) { for (const rda_handle *H : F->egos) if (H->opts.duals_follow) return true; return false; }
// a polygon robot whose consecutive rows intersect: what the clearance kernel, the peer table and a footprint take (else RDA_ERR_UNSUPPORTED)
static bool member_clearance_ok(const rda_handle *H)
{
    if (H->d.c.robot_norm2) return false;
    const int R = H->d.c.R;
    const double *G = H->rob_G.data();
    for (int k = 0; k < R; ++k) { const int j = (k + R - 1) % R; if (G[2 * j] * G[2 * k + 1] - G[2 * j + 1] * G[2 * k] == 0) return false; }
    return true;
}
static bool fleet_clearance_ok(const rda_fleet *F) { for (const rda_handle *H : F->egos) if (!member_clearance_ok(H)) return false; return true; }
// rda_fleet_clearance, rda_fleet_peer_clearance: member by member, idle and then a robot the kernel takes
static int fleet_check_clearance_call(const rda_fleet *F)
{
    for (const rda_handle *H : F->egos) {
        if (H->tick.pending) return RDA_ERR_ARG;
        if (!member_clearance_ok(H)) return RDA_ERR_UNSUPPORTED;
    }
    return RDA_OK;
}

// every member's raw scene in one call (member i owns counts[i] consecutive entries of the arrays): staged on the members'
// streams without waiting - the next fleet step orders itself behind them (fleet_refresh) and ends with a synchronisation
extern "C" int rda_fleet_upload_scenes(rda_fleet *F, const int32_t *counts, const int32_t *kind, const int32_t *nvert, const double *geom,
                                       const double *vel, const double *robot_xy, const int32_t *order)
{
    if (!F || !counts || !robot_xy || !order) return RDA_ERR_ARG;
    size_t off = 0;
    for (int i = 0; i < F->B; ++i) {
        rda_handle *H = F->egos[i];
        const size_t E = H->d.c.E;
        const int n = counts[i];
        if (n < 0) return RDA_ERR_ARG;
        int rc = rda_upload_scene_async(H, n, kind ? kind + off : nullptr, nvert ? nvert + off : nullptr, geom ? geom + off * E * 2 : nullptr,
                                        vel ? vel + off * 2 : nullptr, robot_xy + 2 * i, order[i]);
        if (rc != RDA_OK) return rc;
        off += (size_t)n;
    }
    return RDA_OK;
}

// rda_scene_resort for every member in ONE launch set (round 6): the members' resident raw scenes (rda_upload_scene*, static obstacles) re-ranked about
// states[i * stride + 0..1] and their slots rebuilt on the fleet's stream; the next fleet step runs behind it.  Same device code per member as
// rda_scene_resort: bit-identical slots.  Members with rda_opts::duals_follow, without a resident scene, or inside a tick: RDA_ERR_UNSUPPORTED / _ARG.
static scene::Args fleet_resort_args(const rda_handle *H) { scene::Args a = H->sc.args; a.order = 1; a.robot_val = 0; a.rx = 0; a.ry = 0; return a; }      // (the position: from res.rob)
// the members' scene arguments (uploaded when they changed) and their robots' positions -> res.sc, res.rob; nmax, wmax: what sizes the launches
static int fleet_resort_positions(rda_fleet *F, const double *states, int stride, int &nmax, int &wmax)
{
    const size_t B = F->B;
    const auto args = [F](size_t i) { return fleet_resort_args(F->egos[i]); };
    for (size_t i = 0; i < B; ++i) {
        const scene::Args &a = F->egos[i]->sc.args;
        nmax = a.n > nmax ? a.n : nmax; wmax = a.N * a.nt > wmax ? a.N * a.nt : wmax;
    }
    const bool changed = mirror_differs(F->res.sc, args);
    if (changed || F->rob_pending) HIPCHK(fleet_wait(F));
    if (changed) HIPCHK(mirror_upload(F->res.sc, args, F->stream));
    for (size_t i = 0; i < B; ++i) { F->res.rob.h[2 * i] = states[i * stride]; F->res.rob.h[2 * i + 1] = states[i * stride + 1]; }
    HIPCHK(F->res.rob.push(F->stream));
    F->rob_pending = 1;
    return RDA_OK;
}
// the four launches of a re-sort: the members' scene arguments `sc` re-ranked about the positions `rob` (null: every member's arguments as they stand)
// plan (scenes of the peers upload, B >= 2): scene::k_build_plan_fleet in k_build_fleet's place - peers predicted along their plans
static void fleet_resort_launch(rda_fleet *F, const scene::Args *sc, const double *rob, int nmax, int wmax, const scene::Plan *plan = nullptr)
{
    const unsigned B = (unsigned)F->B;
    hipLaunchKernelGGL(scene::k_keys_fleet, dim3((nmax + 255) / 256, B), dim3(256), 0, F->stream, sc, rob);
    hipLaunchKernelGGL(scene::k_rank_fleet, dim3((nmax + 15) / 16, B), dim3(256), 0, F->stream, sc, rob);
    if (plan && B > 1)
        hipLaunchKernelGGL(scene::k_build_plan_fleet, dim3((wmax + 255) / 256, B), dim3(256), 0, F->stream, sc, rob, (const scene::Peer *)F->pe.tab.d, *plan, (int)B);
    else
        hipLaunchKernelGGL(scene::k_build_fleet, dim3((wmax + 255) / 256, B), dim3(256), 0, F->stream, sc, rob);
    hipLaunchKernelGGL(k_prepare_fleet, dim3((unsigned)((wmax + 3) / 4), B), dim3(256), 0, F->stream, (const Dev *)F->devs.d);
}
extern "C" int rda_fleet_scene_resort(rda_fleet *F, const double *states, int stride)
{
    if (!F || !states || stride < 2) return RDA_ERR_ARG;
    for (rda_handle *H : F->egos) {
        if (H->sc.n <= 0 || H->d.obstacle_num == 0 || H->tick.pending) return RDA_ERR_ARG;
        if (H->opts.duals_follow) return RDA_ERR_UNSUPPORTED;
    }
    FleetReserve rsv(F);
    rsv.need(&FleetSets::res, (size_t)F->B);
    int rc = rsv.adopt();
    if (rc == RDA_OK) rc = fleet_refresh(F);
    if (rc != RDA_OK) return rc;
    int nmax = 0, wmax = 0;
    rc = fleet_resort_positions(F, states, stride, nmax, wmax);
    if (rc != RDA_OK) return rc;
    fleet_resort_launch(F, F->res.sc.d, F->res.rob.d, nmax, wmax);
    HIPCHK(hipGetLastError());
    return RDA_OK;
}

// ---- fleet lidar (lidar::k_scan_fleet): every member's range scan in one launch --------------------------------------------------------------------
// rda_set_scan_split for the fleet's scans (fleet_scan_run, fleet_rollout_lidar)
extern "C" int rda_fleet_set_scan_split(rda_fleet *F, double tol)
{
    if (!F || !scan_split_ok(tol)) return RDA_ERR_ARG;
    F->scan_split = tol;
    return RDA_OK;
}

// the argument rules of scan_run, for every member
static int fleet_scan_check(const rda_fleet *F, const int32_t *n_beams, const double *ranges, const double *angle_min, const double *angle_max,
                            const double *range_max, const double *states, double eps, int min_samples)
{
    if (!F || !n_beams || !ranges || !angle_min || !angle_max || !range_max || !states || !(eps > 0) || min_samples < 1) return RDA_ERR_ARG;
    for (int i = 0; i < F->B; ++i) if (n_beams[i] < 0) return RDA_ERR_ARG;
    for (int i = 0; i < F->B; ++i) if (n_beams[i] > lidar::MAXB || F->egos[i]->d.c.E < 4) return RDA_ERR_UNSUPPORTED;
    return RDA_OK;
}

// All members' scans through ONE lidar::k_scan_fleet launch on the fleet's stream (a workgroup and so a compute unit per member), and the ONE wait for
// it: the counters are then in li.h_count [B][2], the boxes in li.d_boxes; to_host: labels (at the member's beam offset) and boxes also in li_host.
struct TrackArgs { double gate; int window; };      // tracked mode: lidar::k_track_boxes_fleet's association gate [m] and history length
static int track_check(const TrackArgs &t) { return (t.gate > 0 && t.window >= 1 && t.window <= lidar::TRK_HIST) ? RDA_OK : RDA_ERR_ARG; }
// the tracker's member table -> device: member i's boxes and box count where the scan kernels leave them (li.d_boxes, li.h_count), its part of both buffers
// of tk, its sample time.  The pinned mirror is rewritten only when it differs, which it does on the first tracked call and after the lidar block was
// made anew.  li, tk: the fleet's, or (rda_fleet_upload_scans_tracked, whose scan runs before the call can no longer be refused) its reservation's.
static int fleet_track_table(rda_fleet *F, const FleetLidar &li, const FleetTracks &tk)
{
    const size_t B = F->B, M = lidar::MAX_TRACKS;
    std::vector<lidar::Track> tv(B);
    for (size_t i = 0; i < B; ++i) {
        lidar::Track &t = tv[i];
        memset((void *)&t, 0, sizeof(t));
        t.boxes = li.d_boxes + i * lidar::MAXB * 8; t.count = li.h_count + 2 * i;
        for (size_t p = 0; p < 2; ++p) {
            t.cnt[p] = tk.cnt + p * B + i; t.len[p] = tk.len + (p * B + i) * M; t.hist[p] = tk.hist + (p * B + i) * M * lidar::TRK_HIST * 2;
            t.tvel[p] = tk.tvel + (p * B + i) * M * 2;
        }
        t.vel = tk.vel + i * lidar::MAXB * 2; t.dt = F->egos[i]->d.c.dt;
    }
    return fleet_table(F, tk.tab, records(tv));
}
// one launch for the fleet, behind the scan kernel that wrote the counts; the caller switches tk.par once the tick goes through
static void fleet_track_launch(rda_fleet *F, const FleetTracks &tk, const TrackArgs &t)
{
    hipLaunchKernelGGL(lidar::k_track_boxes_fleet, dim3((unsigned)F->B), dim3(lidar::TRK_NT), 0, F->stream, (const lidar::Track *)tk.tab.d, tk.par, t.gate,
                       t.window);
}

// li (and track: tk): as for fleet_track_table
static int fleet_scan_run(rda_fleet *F, FleetLidar &li, const int32_t *n_beams, const double *ranges, const double *angle_min, const double *angle_max,
                          const double *range_max, const double *states, double eps, int min_samples, bool to_host, const TrackArgs *track = nullptr,
                          const FleetTracks *tk = nullptr)
{
    const size_t B = F->B;
    size_t off = 0;
    for (size_t i = 0; i < B; ++i) {
        lidar::Args &a = li.args.h[i];
        a.n_beams = n_beams[i]; a.ranges = li.h_ranges + off; a.angle_min = angle_min[i]; a.angle_max = angle_max[i]; a.range_max = range_max[i];
        a.sx = states[3 * i]; a.sy = states[3 * i + 1]; a.sth = states[3 * i + 2]; a.eps = eps; a.min_samples = min_samples;
        a.boxes = li.d_boxes + i * lidar::MAXB * 8; a.count = li.h_count + 2 * i;
        a.labels_h = to_host ? F->li_host.h_labels + off : nullptr; a.boxes_h = to_host ? F->li_host.h_boxes + i * lidar::MAXB * 8 : nullptr;
        a.split_tol = F->scan_split;
        li.h_count[2 * i] = 0; li.h_count[2 * i + 1] = 0;
        off += (size_t)n_beams[i];
    }
    memcpy(li.h_ranges, ranges, off * sizeof(double));                  // one pinned copy of all ranges (off <= B * MAXB)
    HIPCHK(li.args.push(F->stream));
    hipLaunchKernelGGL(lidar::k_scan_fleet, dim3((unsigned)B), dim3(lidar::NT), lidar::LDS_BYTES, F->stream, (const lidar::Args *)li.args.d);
    if (track) fleet_track_launch(F, *tk, *track);                      // (in front of the wait: the tick gains a launch, no wait)
    HIPCHK(hipGetLastError());
    HIPCHK(fleet_wait(F));
    return RDA_OK;
}

extern "C" int rda_fleet_scan_boxes(rda_fleet *F, const int32_t *n_beams, const double *ranges, const double *angle_min, const double *angle_max,
                                    const double *range_max, const double *states, double eps, int min_samples, int32_t *n_boxes, double *boxes, int cap,
                                    int32_t *labels)
{
    if (!n_boxes || cap < 0 || (cap > 0 && !boxes)) return RDA_ERR_ARG;
    int rc = fleet_scan_check(F, n_beams, ranges, angle_min, angle_max, range_max, states, eps, min_samples);
    if (rc != RDA_OK) return rc;
    FleetReserve rsv(F);
    rsv.need_lidar(true);
    rc = rsv.adopt();
    if (rc == RDA_OK) rc = fleet_scan_run(F, F->li, n_beams, ranges, angle_min, angle_max, range_max, states, eps, min_samples, true);
    if (rc != RDA_OK) return rc;
    size_t off = 0;
    for (size_t i = 0; i < (size_t)F->B; ++i) {
        const int n = F->li.h_count[2 * i];
        n_boxes[i] = n;
        if (boxes) memcpy(boxes + i * (size_t)cap * 8, F->li_host.h_boxes + i * lidar::MAXB * 8, (size_t)(n < cap ? n : cap) * 8 * sizeof(double));
        if (labels) memcpy(labels + off, F->li_host.h_labels + off, (size_t)n_beams[i] * sizeof(int32_t));
        off += (size_t)n_beams[i];
    }
    return RDA_OK;
}

// The staging half of rda_fleet_upload_scans, shared with rda_fleet_rollout_lidar: the B box counts are in li.h_count, the boxes in li.d_boxes and the
// fleet's stream is idle.  Every member's boxes -> raw scene -> slots -> candidate lists by FIVE launches whatever B is (blockIdx.y = the member); the
// zero-box rule, the members' records and the LamMuZ launch form follow the counts.  grow: every member's larger raw scene where it needs one, allocated
// by the caller (nothing of any member has changed when an allocation is refused).  The robot positions: states [B][3] on the host, or (pose_dev) [B][3]
// in device memory - rda_fleet_rollout_lidar, where only the device knows them.  Host-side member state ends as scan_stage / scene_kernels leave it.
// tracked: the boxes carry the velocities lidar::k_track_boxes_fleet left in tk.vel and every member with boxes gets slots for T + 1 stages - the host does
// not see the velocities (as with the peers modes); scene::build_body's 0.01 m/s rule decides per box whether it is predicted.
static int fleet_scan_stage(rda_fleet *F, std::vector<SceneGrow> &grow, const double *states, const double *pose_dev, const int32_t *order, bool tracked = false)
{
    const size_t B = F->B;
    FleetLidar &li = F->li;
    int nmax = 0, wmax = 0;
    for (size_t i = 0; i < B; ++i) {
        rda_handle *H = F->egos[i];
        Dev &d = H->d;
        const int n = li.h_count[2 * i];
        lidar::Fill &f = li.fill.h[i];
        if (n <= 0) {                                   // nothing written: stale A, b stay (rda_solver.py:485)
            d.obstacle_num = 0;
            memset((void *)&li.sc.h[i], 0, sizeof(scene::Args)); memset((void *)&f, 0, sizeof(f));
            continue;
        }
        scene_grow_commit(H, grow[i]);
        const scene::Args a = scene_args(H, n, tracked ? d.c.T + 1 : 1, order[i] ? 1 : 0);
        f.boxes = li.d_boxes + i * lidar::MAXB * 8; f.n = n; f.E = a.E; f.vel_in = tracked ? F->tk.vel + i * lidar::MAXB * 2 : nullptr;
        f.geom = const_cast<double *>(a.geom); f.vel = const_cast<double *>(a.vel); f.robot = const_cast<double *>(a.robot);
        f.nonconvex = a.nonconvex; f.kind = const_cast<int *>(a.kind); f.nvert = const_cast<int *>(a.nvert);
        f.rx = states ? states[3 * i] : 0.0; f.ry = states ? states[3 * i + 1] : 0.0; f.rob = pose_dev ? pose_dev + 3 * i : nullptr;
        memcpy((void *)&li.sc.h[i], &a, sizeof(a));
        scene_bind(H, a, true);                         // (no per-member kernels: the launches below take every member)
        nmax = n > nmax ? n : nmax; wmax = a.N * a.nt > wmax ? a.N * a.nt : wmax;
    }
    // the members' records as they are now (the stream is idle: nothing reads the pinned mirrors)
    HIPCHK(mirror_upload(F->devs, member_devs(F), F->stream));
    if (nmax > 0) {
        HIPCHK(li.fill.push(F->stream));
        HIPCHK(li.sc.push(F->stream));
        hipLaunchKernelGGL(lidar::k_scene_fill_fleet, dim3((nmax + 255) / 256, (unsigned)B), dim3(256), 0, F->stream, (const lidar::Fill *)li.fill.d);
        fleet_resort_launch(F, li.sc.d, nullptr, nmax, wmax);                             // every member's own order and robot position
        HIPCHK(hipGetLastError());
    }
    return RDA_OK;
}

// rda_upload_scan for every member: one scan launch, one wait for the B counts, then the staging above, all on the fleet's stream.
// track: the tracked form - the tracker's launch behind the scan's, the table switched once nothing can refuse the tick any more
static int fleet_upload_scans(rda_fleet *F, const int32_t *n_beams, const double *ranges, const double *angle_min, const double *angle_max,
                              const double *range_max, const double *states, double eps, int min_samples, const int32_t *order, int32_t *n_boxes,
                              const TrackArgs *track)
{
    if (!order) return RDA_ERR_ARG;
    int rc = fleet_scan_check(F, n_beams, ranges, angle_min, angle_max, range_max, states, eps, min_samples);
    if (rc == RDA_OK && track) rc = track_check(*track);
    if (rc != RDA_OK) return rc;
    const size_t B = F->B;
    if (!fleet_members_idle(F)) return RDA_ERR_ARG;
    if (fleet_duals_follow(F)) return RDA_ERR_UNSUPPORTED;
    // The scan runs on the blocks of the reservation where the fleet has none yet: how many boxes it finds decides what else the call allocates, so the
    // call can still be refused behind it (the blocks then go with the call; the tracks: not switched)
    FleetReserve rsv(F);
    if (track) rsv.need(&FleetSets::tk, B);
    rsv.need_lidar(false);
    rc = rsv.bad();
    FleetLidar &li = rsv.now(&FleetSets::li);
    const FleetTracks &tk = rsv.now(&FleetSets::tk);
    if (rc == RDA_OK) rc = fleet_refresh(F);            // behind whatever the members still have queued
    if (rc == RDA_OK && track) rc = fleet_track_table(F, li, tk);
    if (rc == RDA_OK) rc = fleet_scan_run(F, li, n_beams, ranges, angle_min, angle_max, range_max, states, eps, min_samples, false, track, &tk);
    // larger raw scenes where a member needs one: allocated for all members before anything of any member changes
    std::vector<SceneGrow> grow(B);
    for (size_t i = 0; i < B && rc == RDA_OK; ++i) if (li.h_count[2 * i] > 0) rc = scene_grow_alloc(F->egos[i], li.h_count[2 * i], grow[i]);
    if (rc == RDA_OK) rc = rsv.adopt();                 // (first-use sets: no wait)
    if (rc != RDA_OK) return rc;
    if (track) F->tk.par ^= 1;
    rc = fleet_scan_stage(F, grow, states, nullptr, order, track != nullptr);
    if (rc != RDA_OK) return rc;
    if (n_boxes) for (size_t i = 0; i < B; ++i) n_boxes[i] = F->li.h_count[2 * i];
    return RDA_OK;
}
extern "C" int rda_fleet_upload_scans(rda_fleet *F, const int32_t *n_beams, const double *ranges, const double *angle_min, const double *angle_max,
                                      const double *range_max, const double *states, double eps, int min_samples, const int32_t *order, int32_t *n_boxes)
{
    return fleet_upload_scans(F, n_beams, ranges, angle_min, angle_max, range_max, states, eps, min_samples, order, n_boxes, nullptr);
}
extern "C" int rda_fleet_upload_scans_tracked(rda_fleet *F, const int32_t *n_beams, const double *ranges, const double *angle_min, const double *angle_max,
                                              const double *range_max, const double *states, double eps, int min_samples, const int32_t *order,
                                              int32_t *n_boxes, double gate, int window)
{
    const TrackArgs t{ gate, window };
    return fleet_upload_scans(F, n_beams, ranges, angle_min, angle_max, range_max, states, eps, min_samples, order, n_boxes, &t);
}

// The tracker alone, on boxes the caller supplies: n [B] counts (at most 4096 each and at most cap), boxes [B][cap][4][2]; vel_out [B][cap][2] (may be
// null).  The table advances by one tick; nothing is staged.  The boxes take the place of the last scan's in the fleet's lidar block.
extern "C" int rda_fleet_track_boxes(rda_fleet *F, const int32_t *n, const double *boxes, int cap, double gate, int window, double *vel_out)
{
    if (!F || !n || cap < 0 || (cap > 0 && !boxes)) return RDA_ERR_ARG;
    const TrackArgs t{ gate, window };
    if (track_check(t)) return RDA_ERR_ARG;
    const size_t B = F->B;
    for (size_t i = 0; i < B; ++i) if (n[i] < 0 || n[i] > cap) return RDA_ERR_ARG;
    for (size_t i = 0; i < B; ++i) if (n[i] > lidar::MAXB) return RDA_ERR_UNSUPPORTED;
    FleetReserve rsv(F);
    rsv.need(&FleetSets::tk, B);
    rsv.need_lidar(false);
    int rc = rsv.adopt();
    if (rc != RDA_OK) return rc;
    HIPCHK(fleet_wait(F));                              // (a staging that is still queued may be reading the boxes of the last scan)
    rc = fleet_track_table(F, F->li, F->tk);
    if (rc != RDA_OK) return rc;
    for (size_t i = 0; i < B; ++i) {
        F->li.h_count[2 * i] = n[i]; F->li.h_count[2 * i + 1] = 0;
        if (n[i] > 0) HIPCHK(hipMemcpyAsync(F->li.d_boxes + i * lidar::MAXB * 8, boxes + i * (size_t)cap * 8, (size_t)n[i] * 8 * sizeof(double), hipMemcpyHostToDevice, F->stream));
    }
    fleet_track_launch(F, F->tk, t);
    HIPCHK(hipGetLastError());
    std::vector<double> v;
    if (vel_out) {
        v.resize(B * lidar::MAXB * 2);
        HIPCHK(hipMemcpyAsync(v.data(), F->tk.vel, v.size() * sizeof(double), hipMemcpyDeviceToHost, F->stream));
    }
    HIPCHK(fleet_wait(F));
    F->tk.par ^= 1;
    if (vel_out) for (size_t i = 0; i < B; ++i) memcpy(vel_out + i * (size_t)cap * 2, v.data() + i * lidar::MAXB * 2, (size_t)n[i] * 2 * sizeof(double));
    return RDA_OK;
}

// the table as the last tracked call left it: n [B] tracks per member (may exceed cap: the first cap are written), per track its position centres
// [B][cap][2], the velocity its box got vel [B][cap][2] and the entries of its history age [B][cap] (each may be null).  No tracked call yet: no tracks.
extern "C" int rda_fleet_box_tracks(rda_fleet *F, int cap, int32_t *n, double *centres, double *vel, int32_t *age)
{
    if (!F || !n || cap < 0) return RDA_ERR_ARG;
    const size_t B = F->B, M = lidar::MAX_TRACKS;
    FleetTracks &tk = F->tk;
    if (!tk.have()) { for (size_t i = 0; i < B; ++i) n[i] = 0; return RDA_OK; }
    const size_t p = (size_t)tk.par;
    HIPCHK(hipMemcpyAsync(tk.h_cnt, tk.cnt + p * B, B * sizeof(int), hipMemcpyDeviceToHost, F->stream));
    HIPCHK(hipMemcpyAsync(tk.h_len, tk.len + p * B * M, B * M * sizeof(int), hipMemcpyDeviceToHost, F->stream));
    HIPCHK(hipMemcpyAsync(tk.h_hist, tk.hist + p * B * M * lidar::TRK_HIST * 2, B * M * lidar::TRK_HIST * 2 * sizeof(double), hipMemcpyDeviceToHost, F->stream));
    HIPCHK(hipMemcpyAsync(tk.h_tvel, tk.tvel + p * B * M * 2, B * M * 2 * sizeof(double), hipMemcpyDeviceToHost, F->stream));
    HIPCHK(fleet_wait(F));
    for (size_t i = 0; i < B; ++i) {
        int c = tk.h_cnt[i]; c = c < 0 ? 0 : (c > (int)M ? (int)M : c);
        n[i] = c;
        for (int k = 0; k < c && k < cap; ++k) {
            int l = tk.h_len[i * M + k]; l = l < 1 ? 1 : (l > lidar::TRK_HIST ? lidar::TRK_HIST : l);
            const size_t o = i * (size_t)cap + k;
            if (centres) { const double *h = tk.h_hist + ((i * M + k) * lidar::TRK_HIST + (l - 1)) * 2; centres[2 * o] = h[0]; centres[2 * o + 1] = h[1]; }
            if (vel) { vel[2 * o] = tk.h_tvel[(i * M + k) * 2]; vel[2 * o + 1] = tk.h_tvel[(i * M + k) * 2 + 1]; }
            if (age) age[o] = l;
        }
    }
    return RDA_OK;
}

// the members which [count] (NULL: all) lose their tracks: their boxes of the next tracked tick start new ones
extern "C" int rda_fleet_reset_tracks(rda_fleet *F, const int32_t *which, int count)
{
    if (!F || (which && count < 0)) return RDA_ERR_ARG;
    const size_t B = F->B;
    if (which) for (int k = 0; k < count; ++k) if (which[k] < 0 || (size_t)which[k] >= B) return RDA_ERR_ARG;
    FleetTracks &tk = F->tk;
    if (!tk.have()) return RDA_OK;
    int *cur = tk.cnt + (size_t)tk.par * B;
    if (!which) HIPCHK(hipMemsetAsync(cur, 0, B * sizeof(int), F->stream));
    else for (int k = 0; k < count; ++k) HIPCHK(hipMemsetAsync(cur + which[k], 0, sizeof(int), F->stream));
    return RDA_OK;
}

// One tick's tracker inputs, for rda_fleet_step_tracked and the rollouts' tick 0: the nominal controls (null: they are resident) into the members' step
// blocks, every member's track::In -> device
static int fleet_track_inputs(rda_fleet *F, const double *states, const double *ref_speed, const int32_t *cur_index, double threshold, int ind_range,
                              const double *nom_u)
{
    const size_t T = F->T, nu = traj_u(T), nin = step_doubles(T), B = F->B;
    if (nom_u) {
        for (size_t i = 0; i < B; ++i) memcpy(F->in.h + i * nin + step_u(T), nom_u + i * nu, nu * sizeof(double));
        HIPCHK(hipMemcpy2DAsync(F->in.d + step_u(T), nin * sizeof(double), F->in.h + step_u(T), nin * sizeof(double), nu * sizeof(double), B,
                                hipMemcpyHostToDevice, F->stream));
    }
    for (size_t i = 0; i < B; ++i) {
        track::In &in = F->trk.in.h[i];
        in.sx = states[3 * i]; in.sy = states[3 * i + 1]; in.sth = states[3 * i + 2]; in.speed = ref_speed[i]; in.threshold = threshold;
        in.cur_index = cur_index[i]; in.ind_range = ind_range;
    }
    HIPCHK(F->trk.in.push(F->stream));
    return RDA_OK;
}

extern "C" int rda_fleet_step_tracked(rda_fleet *F, const double *states, const double *ref_speed, const int32_t *cur_index,
                                      double threshold, int ind_range, const double *nom_u,
                                      double *out_u, double *out_s, rda_info *info, double *ref_out, int32_t *min_index, double *end_heading)
{
    if (!F || !states || !ref_speed || !cur_index || !out_u || !out_s || ind_range < 1) return RDA_ERR_ARG;
    const size_t T = F->T, ns = traj_s(T), nin = step_doubles(T), B = F->B;
    FleetReserve rsv(F);
    rsv.need(&FleetSets::trk, B);
    int rc = rsv.adopt();
    if (rc != RDA_OK) return rc;
    // the result of the tick is written where the host reads it (round 6): k_finish_fleet and k_track_fleet store straight into the pinned blocks (write-only,
    // fire-and-forget stores over the link, complete at the end of their kernels) instead of three device-to-host copies queued behind the last launch
    // (~10 us each on the tick's critical path).  rda_opts::zero_copy = 0 on any member keeps the copies.
    bool zc = true;
    for (size_t i = 0; i < B; ++i) if (!F->egos[i]->opts.zero_copy) zc = false;
    double *const out_base = zc ? F->out.h : F->out.d;
    rda_info *const info_base = zc ? F->info.h : F->info.d;
    FleetTrack &trk = F->trk;
    for (size_t i = 0; i < B; ++i) {
        const rda_handle *H = F->egos[i];
        if (!H->path.d || cur_index[i] < 0 || cur_index[i] >= H->path.len) return RDA_ERR_ARG;
    }
    const auto io = [&](size_t i) { return fleet_member_io(F, i, nom_u ? nullptr : F->egos[i]->d.u, out_base, info_base); };
    const bool tables = mirror_differs(trk.io, io) || mirror_differs(trk.paths, member_paths(F)) || mirror_differs(trk.lens, member_lens(F));
    rc = fleet_refresh(F);
    if (rc != RDA_OK) return rc;
    if (tables) {
        HIPCHK(fleet_wait(F));
        HIPCHK(mirror_upload(trk.io, io, F->stream));
        HIPCHK(mirror_upload(trk.paths, member_paths(F), F->stream));
        HIPCHK(mirror_upload(trk.lens, member_lens(F), F->stream));
    }
    rc = fleet_track_inputs(F, states, ref_speed, cur_index, threshold, ind_range, nom_u);
    if (rc != RDA_OK) return rc;
    hipLaunchKernelGGL(k_track_fleet, dim3((unsigned)B), dim3(64), 0, F->stream, F->devs.d, trk.io.d, trk.in.d, trk.paths.d, trk.lens.d,
                       zc ? trk.out.h : trk.out.d, (int)B);
    rc = fleet_enqueue(F, trk.io.d, 0);
    if (rc != RDA_OK) return rc;
    if (!zc) {
        HIPCHK(F->out.pull(F->stream, F->out.n));
        HIPCHK(F->info.pull(F->stream, B));
        HIPCHK(trk.out.pull(F->stream, B));
    }
    if (ref_out) HIPCHK(F->in.pull(F->stream, F->in.n));
    HIPCHK(fleet_wait(F, true));
    for (size_t i = 0; i < B; ++i) {
        fleet_result_out(F, i, out_u, out_s, info);
        if (ref_out) memcpy(ref_out + i * ns, F->in.h + i * nin + step_ref(T), ns * sizeof(double));
        if (min_index) min_index[i] = trk.out.h[i].min_index;
        if (end_heading) end_heading[i] = trk.out.h[i].end_heading;
    }
    return RDA_OK;
}

// ---- rda_fleet_rollout: K closed-loop ticks queued back to back, ONE host wait ---------------------------------------------------------------------
// Per tick the launches of the host loop (closed_loop_fleet_run: re-sort, k_track_fleet, the ADMM launches) and rollout::k_rollout_advance, which does on
// the device what that loop's host does between two ticks and writes the next tick's inputs where these kernels read them.
// What the entries (rda_fleet_rollout, _moving, _lidar, _peers*, _gears) take alike; clearance_log: null for the static entry
struct RollArgs {
    int K; const double *states, *ref_speed; const int32_t *cur_index; double threshold; int ind_range, goal_margin; const double *nom_u;
    double *states_log, *u_log; int32_t *index_log; rda_info *info_log; int32_t *arrived_at; double *clearance_log;
    bool peers = false; const double *controls0 = nullptr; double *peer_clearance_log = nullptr;     // rda_fleet_rollout_peers
    bool plan = false; const double *plans0 = nullptr; const int32_t *plan_valid0 = nullptr;          // rda_fleet_rollout_peers_plan (with peers)
    bool gears = false; const int32_t *piece0 = nullptr; int32_t *piece_log = nullptr;                // rda_fleet_rollout_gears: ref_speed unsigned, cur_index within piece0
    // the head every entry fills (a constructor: an entry that leaves one of them out does not compile)
    RollArgs(int K, const double *states, const double *ref_speed, const int32_t *cur_index, double threshold, int ind_range, int goal_margin, const double *nom_u,
             double *states_log, double *u_log, int32_t *index_log, rda_info *info_log, int32_t *arrived_at, double *clearance_log)
        : K(K), states(states), ref_speed(ref_speed), cur_index(cur_index), threshold(threshold), ind_range(ind_range), goal_margin(goal_margin), nom_u(nom_u),
          states_log(states_log), u_log(u_log), index_log(index_log), info_log(info_log), arrived_at(arrived_at), clearance_log(clearance_log) {}
};
// the argument rules every entry has: of the arrays and counts, and (roll_check_members) of the members' paths
static int roll_check_args(const rda_fleet *F, const RollArgs &a)
{
    if (!F || a.K < 1 || a.K > 4096 || !a.states || !a.ref_speed || !a.cur_index || !a.states_log || !a.u_log || !a.index_log || !a.arrived_at) return RDA_ERR_ARG;
    return a.ind_range < 1 || a.goal_margin < 1 ? RDA_ERR_ARG : RDA_OK;
}
static int roll_check_members(const rda_fleet *F, const int32_t *cur_index)
{
    for (int i = 0; i < F->B; ++i) {
        const rda_handle *H = F->egos[i];
        if (!H->path.d || cur_index[i] < 0 || cur_index[i] >= H->path.len || H->tick.pending) return RDA_ERR_ARG;
    }
    return RDA_OK;
}
// ... of their resident pieces: the gear rollout does not read the members' rda_upload_path paths
static int roll_check_pieces(const rda_fleet *F, const RollArgs &a)
{
    if (!a.piece0 || !a.piece_log) return RDA_ERR_ARG;
    for (int i = 0; i < F->B; ++i) {
        const PieceSet &ps = F->egos[i]->pieces;
        if (!ps.have() || a.piece0[i] < 0 || a.piece0[i] >= ps.P || F->egos[i]->tick.pending) return RDA_ERR_ARG;
        if (a.cur_index[i] < 0 || a.cur_index[i] >= ps.h_off[a.piece0[i] + 1] - ps.h_off[a.piece0[i]]) return RDA_ERR_ARG;
    }
    return RDA_OK;
}

// One member's move and clearance records for the geometry [n][E][2] it is given - its resident raw scene, or its world (geom null: none; base: the
// geometry's snapshot).  Robot vertices of the clearance: body-frame intersections of consecutive rows of G x <= h (scenarios.robot_vertices: vertex i
// from rows i - 1 and i); 0 vertices for a norm2 robot.
static void member_move_clear(const rda_handle *H, double *geom, double *base, const double *vel, const int *kind, const int *nvert, int n, int E,
                              scene::Move &m, rollout::Clear &c)
{
    memset((void *)&m, 0, sizeof(m)); memset((void *)&c, 0, sizeof(c));
    const int R = H->d.c.R;
    c.R = H->d.c.robot_norm2 ? 0 : R;
    for (int k = 0; k < c.R; ++k) {
        const int j = (k + R - 1) % R;
        const double *G = H->rob_G.data(), *h = H->rob_h.data();
        const double det = G[2 * j] * G[2 * k + 1] - G[2 * j + 1] * G[2 * k];
        c.rv[k][0] = (h[j] * G[2 * k + 1] - G[2 * j + 1] * h[k]) / det;
        c.rv[k][1] = (G[2 * j] * h[k] - h[j] * G[2 * k]) / det;
    }
    c.E = E;
    if (!geom) return;
    m.geom = geom; m.base = base; m.vel = vel; m.kind = kind; m.nvert = nvert; m.n = n; m.E = E; m.dt = H->d.c.dt;
    c.geom = geom; c.kind = kind; c.nvert = nvert; c.n = n;
}
// The moving entry's per-member tables as the members' raw scenes stand now.  mv_total: doubles of all members' raw geometry; gmax: the largest n * E.
struct MoveView { std::vector<scene::Move> mv; std::vector<rollout::Clear> cl; std::vector<scene::Args> sc; std::vector<size_t> off; size_t mv_total = 0; int gmax = 0, nmax = 0, wmax = 0; };
static bool member_raw_scene(const rda_handle *H) { return H->sc.n > 0 && H->d.obstacle_num != 0; }
// a member whose resident raw scene is the one this fleet's last peers upload staged: n_own own obstacles and B - 1 peer rows
static bool member_peers_scene(const rda_fleet *F, size_t i)
{
    const rda_handle *H = F->egos[i];
    return H->sc.peers_of == F && member_raw_scene(H) && F->n_own.size() == (size_t)F->B && H->sc.n == F->n_own[i] + F->B - 1;
}
// own: the move and clearance records end at the members' own obstacles (scenes of the peers upload: the peer rows are neither moved nor counted)
static void fleet_move_view(const rda_fleet *F, MoveView &v, bool own = false)
{
    const size_t B = F->B;
    v.mv.resize(B); v.cl.resize(B); v.sc.resize(B); v.off.assign(B, 0);
    for (size_t i = 0; i < B; ++i) {
        const rda_handle *H = F->egos[i];
        const bool raw = member_raw_scene(H);
        scene::Args &a = v.sc[i];
        memset((void *)&a, 0, sizeof(a));
        if (raw) a = H->sc.args;
        const int nm = own && raw ? F->n_own[i] : a.n;
        member_move_clear(H, raw ? const_cast<double *>(a.geom) : nullptr, nullptr, a.vel, a.kind, a.nvert, nm, H->d.c.E, v.mv[i], v.cl[i]);      // (Move::base is set by the rollout)
        if (!raw) continue;
        v.off[i] = v.mv_total;                                                    // (its place in the snapshot buffer)
        v.mv_total += (size_t)nm * a.E * 2;
        v.gmax = nm * a.E > v.gmax ? nm * a.E : v.gmax;
        v.nmax = a.n > v.nmax ? a.n : v.nmax; v.wmax = a.N * a.nt > v.wmax ? a.N * a.nt : v.wmax;
    }
}
// The peer table as the members stand now: every member's footprint and kinematics, and its tail where its scene came from the peers upload
static void fleet_peer_view(const rda_fleet *F, std::vector<scene::Peer> &v)
{
    const size_t B = F->B;
    v.resize(B);
    for (size_t i = 0; i < B; ++i) {
        const rda_handle *H = F->egos[i];
        scene::Peer &p = v[i];
        scene::Move m; rollout::Clear c;
        memset((void *)&p, 0, sizeof(p));
        member_move_clear(H, nullptr, nullptr, nullptr, nullptr, nullptr, 0, H->d.c.E, m, c);
        p.E = H->d.c.E; p.R = c.R; p.dynamics = H->d.c.dynamics;
        memcpy(p.rv, c.rv, sizeof(p.rv));
        if (!member_peers_scene(F, i)) continue;
        p.n_own = F->n_own[i];
        p.geom = const_cast<double *>(H->sc.args.geom) + (size_t)p.n_own * p.E * 2;
        p.vel = const_cast<double *>(H->sc.args.vel) + (size_t)p.n_own * 2;
    }
}
// scene::k_peers_fleet from states [B][3] and controls [B][2] in device memory; a fleet of one has no peer rows (and a grid of zero blocks is a launch error)
static void fleet_peers_launch(rda_fleet *F, const double *states, const double *controls)
{
    const int B = F->B, E = F->egos[0]->d.c.E;
    if (B < 2) return;
    hipLaunchKernelGGL(scene::k_peers_fleet, dim3((unsigned)(((B - 1) * E + 255) / 256), (unsigned)B), dim3(256), 0, F->stream, (const scene::Peer *)F->pe.tab.d,
                       states, controls, B);
}
static_assert(sizeof(((scene::Peer *)nullptr)->rv) == sizeof(((rollout::Clear *)nullptr)->rv), "the peer table takes the clearance record's robot vertices");
// the peer table as the members stand now -> device, when it differs from what the device holds
static int fleet_peer_table(rda_fleet *F)
{
    std::vector<scene::Peer> pv;
    fleet_peer_view(F, pv);
    return fleet_table(F, F->pe.tab, records(pv));
}
// the peers' inputs of a host-driven refresh or of a rollout's tick 0 -> device: states [B][3], controls [B][2] and (plans non-null) the plans with
// their validity
static int fleet_peers_inputs(rda_fleet *F, const double *states, const double *controls, const double *plans, const int32_t *plan_valid)
{
    HIPCHK(F->pe.st.upload(states, F->stream)); HIPCHK(F->pe.ctl.upload(controls, F->stream));
    if (plans) { HIPCHK(F->pl.plan.upload(plans, F->stream)); HIPCHK(F->pl.valid.upload(plan_valid, F->stream)); }
    return RDA_OK;
}
// every member's separation from the nearest other member at states [B][3] in device memory -> out [B]
static void fleet_peer_clearance_launch(rda_fleet *F, const double *states, double *out)
{
    hipLaunchKernelGGL(rollout::k_peer_clearance_fleet, dim3((unsigned)F->B), dim3(64), 0, F->stream, (const scene::Peer *)F->pe.tab.d, states, out, F->B);
}

// What every rollout entry does around its ticks.
// The advance kernel's member table and the io tables of tick 0 | of the later ticks as the members stand now; true: they, or the members' paths, differ
// from what the device holds.
struct RollView { std::vector<rollout::Member> wm; std::vector<EgoIO> wio; };
static bool fleet_roll_view(const rda_fleet *F, bool have_nom_u, RollView &v)
{
    const size_t B = F->B, T = F->T;
    v.wm.resize(B); v.wio.resize(2 * B);
    for (size_t i = 0; i < B; ++i) {
        const rda_handle *H = F->egos[i];
        v.wio[i] = fleet_member_io(F, i, have_nom_u ? nullptr : H->d.u, F->out.d, F->info.d);      // tick 0
        v.wio[B + i] = fleet_member_io(F, i, H->d.u, F->out.d, F->info.d);                         // later ticks: the resident controls
        rollout::Member &m = v.wm[i];
        memset((void *)&m, 0, sizeof(m));
        m.out_u = v.wio[i].out_u; m.info = v.wio[i].info; m.T = (int)T; m.L = H->path.len; m.dynamics = H->d.c.dynamics; m.dt = H->d.c.dt; m.wheelbase = H->d.c.L;
    }
    return mirror_differs(F->trk.paths, member_paths(F)) || mirror_differs(F->trk.lens, member_lens(F)) || mirror_differs(F->ro.m, records(v.wm)) ||
           mirror_differs(F->ro.io, records(v.wio));
}
// ... uploaded (the fleet's stream is idle: nothing reads the pinned mirrors)
static int fleet_roll_upload(rda_fleet *F, const RollView &v)
{
    HIPCHK(mirror_upload(F->ro.m, records(v.wm), F->stream));
    HIPCHK(mirror_upload(F->ro.io, records(v.wio), F->stream));
    HIPCHK(mirror_upload(F->trk.paths, member_paths(F), F->stream));
    HIPCHK(mirror_upload(F->trk.lens, member_lens(F), F->stream));
    return RDA_OK;
}
// tick 0's nominal controls and tracker inputs, as rda_fleet_step_tracked uploads them; lg: the device logs of this rollout, arrived_at reset to -1
static int fleet_roll_inputs(rda_fleet *F, const RollLayout &lay, const RollArgs &a, rollout::Logs &lg)
{
    std::vector<double> signed_speed;                                           // gears: the single product gear * ref_speed of every member's first piece
    if (a.gears) for (int i = 0; i < F->B; ++i) signed_speed.push_back(F->egos[i]->pieces.h_gear[a.piece0[i]] * a.ref_speed[i]);
    int rc = fleet_track_inputs(F, a.states, a.gears ? signed_speed.data() : a.ref_speed, a.cur_index, a.threshold, a.ind_range, a.nom_u);
    if (rc != RDA_OK) return rc;
    char *log = F->ro_log.log.d;
    lg.states = (double *)(log + lay.states); lg.u = (double *)(log + lay.u); lg.end_heading = (double *)(log + lay.endh);
    lg.info = (rda_info *)(log + lay.info); lg.index = (int *)(log + lay.index); lg.arrived_at = (int *)(log + lay.arrived);
    HIPCHK(hipMemsetAsync(lg.arrived_at, 0xff, F->B * sizeof(int), F->stream));  // -1: not arrived
    return RDA_OK;
}
// The tail of tick k, behind whatever the entry's head did to the members' slots: k_track_fleet, the ADMM launches, k_rollout_advance (rob: where it leaves
// the robots' positions for the next re-sort, or null), then (mv: the raw scenes' or the world's move table, null: nothing moves) scene::k_move_fleet over
// `gmove` and (cl: their clearance table, null: no clearance log) k_clearance_fleet of state k + 1 against the geometry of tick k + 1.
static int fleet_roll_tail(rda_fleet *F, int k, const rollout::Logs &lg, int goal_margin, double *rob, const scene::Move *mv, dim3 gmove,
                           const rollout::Clear *cl, const rollout::GearTab *gt = nullptr)
{
    const size_t B = F->B;
    FleetTrack &trk = F->trk;
    const EgoIO *io = F->ro.io.d + (k == 0 ? 0 : B);
    // gt: a gear rollout - the tracker reads the piece in force from the rollout's tables, which the gear form of the advance kernel rewrites at a switch
    hipLaunchKernelGGL(k_track_fleet, dim3((unsigned)B), dim3(64), 0, F->stream, F->devs.d, io, trk.in.d, gt ? gt->paths : trk.paths.d,
                       gt ? (const int *)gt->lens : trk.lens.d, trk.out.d, (int)B);
    int rc = fleet_enqueue(F, io, 0);
    if (rc != RDA_OK) return rc;
    if (gt)
        hipLaunchKernelGGL(rollout::k_rollout_advance_gears, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, F->stream, (const rollout::Member *)F->ro.m.d,
                           (const track::Out *)trk.out.d, trk.in.d, rob, lg, k, goal_margin, (int)B, *gt);
    else
        hipLaunchKernelGGL(rollout::k_rollout_advance, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, F->stream, (const rollout::Member *)F->ro.m.d,
                           (const track::Out *)trk.out.d, trk.in.d, rob, lg, k, goal_margin, (int)B);
    if (mv) hipLaunchKernelGGL(scene::k_move_fleet, gmove, dim3(256), 0, F->stream, mv, k + 1);      // where tick k + 1 finds them
    if (cl)
        hipLaunchKernelGGL(rollout::k_clearance_fleet, dim3((unsigned)B), dim3(rollout::CLEAR_NT), 0, F->stream, cl,
                           (const double *)(lg.states + (size_t)(k + 1) * B * 3), F->cl_log.v.d + (size_t)k * B, (int)B);
    return RDA_OK;
}
// the logs to the host behind the last tick, the wait for them, and out to the caller's arrays
static int fleet_roll_fetch(rda_fleet *F, const RollLayout &lay, const RollArgs &a)
{
    const size_t T = F->T, B = F->B, K = a.K;
    const char *log = F->ro_log.log.h;
    if (a.clearance_log) HIPCHK(F->cl_log.v.pull(F->stream, K * B));
    const bool peer_log = a.peer_clearance_log && B > 1;                        // (a fleet of one: +inf, nothing was launched)
    if (peer_log) HIPCHK(F->pc_log.v.pull(F->stream, K * B));
    size_t gear_total = 0;
    if (a.gears) {                                                              // the piece log, every member's piece now and the pieces' end headings (Q12)
        for (const rda_handle *Hm : F->egos) gear_total += (size_t)Hm->pieces.P;
        hipLaunchKernelGGL(rollout::k_gear_headings, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, F->stream, (const rollout::Gears *)F->gr.rec.d, F->gr_endh.v.d, (int)B);
        HIPCHK(hipGetLastError());
        HIPCHK(F->gr_log.v.pull(F->stream, K * B)); HIPCHK(F->gr.piece.pull(F->stream, B)); HIPCHK(F->gr_endh.v.pull(F->stream, gear_total));
    }
    HIPCHK(hipMemcpyAsync(F->ro_log.log.d + lay.last, F->out.d, B * res_info(T) * sizeof(double), hipMemcpyDeviceToDevice, F->stream));      // the last tick's full controls and planned states, beside the logs
    HIPCHK(F->ro_log.log.pull(F->stream, lay.bytes));
    HIPCHK(fleet_wait(F, true));
    F->roll_K = a.K; F->gear_total = (int)gear_total;
    if (a.gears) memcpy(a.piece_log, F->gr_log.v.h, K * B * sizeof(int32_t));
    memcpy(a.states_log, a.states, B * 3 * sizeof(double));                     // row 0: the input
    memcpy(a.states_log + B * 3, log + lay.states + B * 3 * sizeof(double), K * B * 3 * sizeof(double));
    memcpy(a.u_log, log + lay.u, K * B * 2 * sizeof(double));
    memcpy(a.index_log, log + lay.index, K * B * sizeof(int32_t));
    if (a.info_log) memcpy(a.info_log, log + lay.info, K * B * sizeof(rda_info));
    memcpy(a.arrived_at, log + lay.arrived, B * sizeof(int32_t));
    if (a.clearance_log) memcpy(a.clearance_log, F->cl_log.v.h, K * B * sizeof(double));
    if (peer_log) memcpy(a.peer_clearance_log, F->pc_log.v.h, K * B * sizeof(double));
    else if (a.peer_clearance_log) for (size_t k = 0; k < K; ++k) a.peer_clearance_log[k] = INFINITY;
    return RDA_OK;
}

// scene::k_move_fleet's grid for members of at most gmax = n * E doubles of geometry and (mv: the move table, null: nothing moves) the snapshot over it -
// `base`: the geometry as the call finds it
static dim3 fleet_move_grid(rda_fleet *F, int gmax, const scene::Move *mv)
{
    const dim3 gmove((unsigned)((gmax + 255) / 256), (unsigned)F->B);
    if (mv) hipLaunchKernelGGL(scene::k_snapshot_fleet, gmove, dim3(256), 0, F->stream, mv);
    return gmove;
}
// rda_fleet_rollout (moving = false: exactly the static entry), rda_fleet_rollout_moving and (a.peers: resort and moving set) rda_fleet_rollout_peers share
// this body
static int fleet_rollout_scenes(rda_fleet *F, const RollArgs &a, int resort, bool moving)
{
    int rc = roll_check_args(F, a);
    if (rc == RDA_OK) rc = a.gears ? roll_check_pieces(F, a) : roll_check_members(F, a.cur_index);
    if (rc != RDA_OK) return rc;
    const size_t T = F->T, B = F->B;
    size_t gear_total = 0;
    if (a.gears) for (const rda_handle *H : F->egos) gear_total += (size_t)H->pieces.P;
    if (a.peers) {
        if (!a.controls0 || (a.plan && (!a.plans0 || !a.plan_valid0))) return RDA_ERR_ARG;
        for (size_t i = 0; i < B; ++i) if (!member_peers_scene(F, i)) return RDA_ERR_ARG;      // the scenes of rda_fleet_upload_scenes_peers, nothing staged since
    }
    for (const rda_handle *H : F->egos) if (resort && (H->sc.n <= 0 || H->d.obstacle_num == 0)) return RDA_ERR_ARG;
    if (fleet_duals_follow(F)) return RDA_ERR_UNSUPPORTED;
    for (const rda_handle *H : F->egos) if (!moving && H->d.obstacle_num != 0 && H->d.nt > 1) return RDA_ERR_UNSUPPORTED;  // a scene that moves has to be uploaded again every tick
    MoveView mvw;
    if (moving) {
        for (const rda_handle *H : F->egos) {
            if (!resort && member_raw_scene(H) && H->sc.args.order != 0) return RDA_ERR_ARG;          // slots rebuilt in the staged order: only meaningful for order = 0
            if (H->d.obstacle_num != 0 && H->d.nt > 1 && H->sc.n <= 0) return RDA_ERR_UNSUPPORTED;    // host-staged per-stage slots: no raw scene to move
            if (a.clearance_log && !member_clearance_ok(H)) return RDA_ERR_UNSUPPORTED;
        }
        fleet_move_view(F, mvw, a.peers);
    }
    const bool peer_log = a.peers && a.peer_clearance_log && B > 1;
    const size_t KB = (size_t)a.K * B;
    FleetReserve rsv(F);
    rsv.need_rollout(a.K, a.clearance_log != nullptr);
    if (a.gears) { rsv.need(&FleetSets::gr, B); rsv.grow(&FleetSets::gr_log, KB, KB); rsv.grow(&FleetSets::gr_endh, gear_total, gear_total); }
    if (peer_log) rsv.grow(&FleetSets::pc_log, KB, KB);
    if (a.plan) rsv.need(&FleetSets::pl, B, T);
    if (resort) rsv.need(&FleetSets::res, B);
    if (moving) { rsv.need(&FleetSets::mov, B); rsv.grow(&FleetSets::snap, mvw.mv_total, mvw.mv_total); }
    rc = rsv.adopt();
    if (rc != RDA_OK) return rc;
    F->roll_K = 0; F->gear_total = 0;                                           // (until this rollout's logs are on the host)
    rc = fleet_refresh(F);
    if (rc != RDA_OK) return rc;
    // one-time table refreshes (the only other waits of a rollout): the tables are compared with what the device holds and uploaded when they differ
    RollView rv;
    bool tables = fleet_roll_view(F, a.nom_u != nullptr, rv);
    if (moving) {
        for (size_t i = 0; i < B; ++i) if (mvw.mv[i].n > 0) mvw.mv[i].base = F->snap.d + mvw.off[i];
        if (mirror_differs(F->mov.mv, records(mvw.mv)) || mirror_differs(F->mov.cl, records(mvw.cl)) || mirror_differs(F->mov.sc, records(mvw.sc))) tables = true;
    }
    std::vector<scene::Peer> pv;
    if (a.peers) { fleet_peer_view(F, pv); if (mirror_differs(F->pe.tab, records(pv))) tables = true; }
    if (tables) {
        HIPCHK(fleet_wait(F));
        if (a.peers) HIPCHK(mirror_upload(F->pe.tab, records(pv), F->stream));
        if (moving) {
            HIPCHK(mirror_upload(F->mov.mv, records(mvw.mv), F->stream));
            HIPCHK(mirror_upload(F->mov.cl, records(mvw.cl), F->stream));
            HIPCHK(mirror_upload(F->mov.sc, records(mvw.sc), F->stream));
        }
        rc = fleet_roll_upload(F, rv);
        if (rc != RDA_OK) return rc;
    }
    // tick 0's inputs, as rda_fleet_scene_resort and rda_fleet_step_tracked upload them
    int nmax = 0, wmax = 0;
    if (resort) { rc = fleet_resort_positions(F, a.states, 3, nmax, wmax); if (rc != RDA_OK) return rc; }
    if (a.peers) {                                                              // (behind fleet_resort_positions: no copy out of the pinned mirrors is queued)
        rc = fleet_peers_inputs(F, a.states, a.controls0, a.plan ? a.plans0 : nullptr, a.plan_valid0);
        if (rc != RDA_OK) return rc;
    }
    const RollLayout lay = roll_layout((size_t)a.K, B, T);
    rollout::Logs lg;
    rc = fleet_roll_inputs(F, lay, a, lg);
    if (rc != RDA_OK) return rc;
    // gears: the members' piece records and tick 0's tables (the device rewrites them, so they travel on every call; nothing queued reads the mirrors)
    rollout::GearTab gt;
    if (a.gears) {
        int hbase = 0;
        for (size_t i = 0; i < B; ++i) {
            const PieceSet &ps = F->egos[i]->pieces;
            const int p = a.piece0[i];
            F->gr.rec.h[i] = rollout::Gears{ ps.buf, ps.off, ps.gear, ps.P, hbase, a.ref_speed[i] };
            F->gr.piece.h[i] = p; F->gr.paths.h[i] = ps.buf + 3 * (size_t)ps.h_off[p]; F->gr.lens.h[i] = ps.h_off[p + 1] - ps.h_off[p];
            hbase += ps.P;
        }
        HIPCHK(F->gr.rec.push(F->stream)); HIPCHK(F->gr.piece.push(F->stream)); HIPCHK(F->gr.paths.push(F->stream)); HIPCHK(F->gr.lens.push(F->stream));
        gt = rollout::GearTab{ F->gr.rec.d, F->gr.piece.d, F->gr.paths.d, F->gr.lens.d, F->gr_log.v.d };
    }
    const bool moves = moving && mvw.gmax > 0;
    const dim3 gmove = fleet_move_grid(F, mvw.gmax, moves ? F->mov.mv.d : nullptr);
    for (int k = 0; k < a.K; ++k) {
        // the peer rows of tick k: the members' states at its start and the controls applied one tick earlier (tick 0: the caller's, then the device logs)
        if (a.peers) fleet_peers_launch(F, k == 0 ? F->pe.st.d : lg.states + (size_t)k * B * 3, k == 0 ? F->pe.ctl.d : lg.u + (size_t)(k - 1) * B * 2);
        // the plans of tick k: the caller's (tick 0), then what the members' solves of tick k - 1 left in the fleet's result block; valid while not arrived
        const scene::Plan pk = k == 0 ? scene::Plan{ F->pe.st.d, F->pl.plan.d, traj_s(T), F->pl.valid.d, nullptr }
                                      : scene::Plan{ lg.states + (size_t)k * B * 3, F->out.d + res_s(T), res_info(T), nullptr, lg.arrived_at };
        if (resort) fleet_resort_launch(F, F->res.sc.d, F->res.rob.d, nmax, wmax, a.plan ? &pk : nullptr);      // about res.rob: the caller's positions (tick 0), then the advance kernel's
        else if (moves) fleet_resort_launch(F, F->mov.sc.d, nullptr, mvw.nmax, mvw.wmax);     // a scene that moved: its slots rebuilt in the staged order
        rc = fleet_roll_tail(F, k, lg, a.goal_margin, resort ? F->res.rob.d : nullptr, moves ? F->mov.mv.d : nullptr, gmove,
                             a.clearance_log ? F->mov.cl.d : nullptr, a.gears ? &gt : nullptr);
        if (rc != RDA_OK) return rc;
        if (peer_log) fleet_peer_clearance_launch(F, lg.states + (size_t)(k + 1) * B * 3, F->pc_log.v.d + (size_t)k * B);
    }
    HIPCHK(hipGetLastError());
    return fleet_roll_fetch(F, lay, a);                                         // the rollout's one wait
}
extern "C" int rda_fleet_rollout(rda_fleet *F, int K, const double *states, const double *ref_speed, const int32_t *cur_index, double threshold,
                                 int ind_range, int goal_margin, int resort, const double *nom_u, double *states_log, double *u_log, int32_t *index_log,
                                 rda_info *info_log, int32_t *arrived_at)
{
    return fleet_rollout_scenes(F, RollArgs{ K, states, ref_speed, cur_index, threshold, ind_range, goal_margin, nom_u, states_log, u_log, index_log, info_log,
                                             arrived_at, nullptr }, resort, false);
}
// The rollout for scenes that move: behind every tick's advance kernel scene::k_move_fleet puts every member's raw geometry where the next tick finds it
// (base + vel * (dt * k), base = the geometry the call found), the tick's re-sort launches rebuild the per-stage slots from it, and (clearance_log)
// rollout::k_clearance_fleet logs every member's clearance after the tick.
extern "C" int rda_fleet_rollout_moving(rda_fleet *F, int K, const double *states, const double *ref_speed, const int32_t *cur_index, double threshold,
                                        int ind_range, int goal_margin, int resort, const double *nom_u, double *states_log, double *u_log,
                                        int32_t *index_log, rda_info *info_log, int32_t *arrived_at, double *clearance_log)
{
    return fleet_rollout_scenes(F, RollArgs{ K, states, ref_speed, cur_index, threshold, ind_range, goal_margin, nom_u, states_log, u_log, index_log, info_log,
                                             arrived_at, clearance_log }, resort, true);
}
// The rollouts above for members whose paths have gear pieces (rda_upload_path_pieces): MPC._piece / _end / _sync_path of a reverse path on the device.
// moving = 0: rda_fleet_rollout, else rda_fleet_rollout_moving; the same body, its tracker reading the rollout's own path tables.
extern "C" int rda_fleet_rollout_gears(rda_fleet *F, int K, const double *states, const double *ref_speed, const int32_t *piece0, const int32_t *cur_index,
                                       double threshold, int ind_range, int goal_margin, int resort, int moving, const double *nom_u, double *states_log,
                                       double *u_log, int32_t *index_log, rda_info *info_log, int32_t *arrived_at, int32_t *piece_log, double *clearance_log)
{
    if (!moving && clearance_log) return RDA_ERR_ARG;                          // (the clearance log belongs to the moving form)
    RollArgs a{ K, states, ref_speed, cur_index, threshold, ind_range, goal_margin, nom_u, states_log, u_log, index_log, info_log, arrived_at, clearance_log };
    a.gears = true; a.piece0 = piece0; a.piece_log = piece_log;
    return fleet_rollout_scenes(F, a, resort, moving != 0);
}
// of the last rda_fleet_rollout_gears: every member's piece after its last tick, and the heading the last waypoint of every piece has now (quirk Q12),
// member-major.  Either may be null.  No device work.
extern "C" int rda_fleet_rollout_last_pieces(rda_fleet *F, int32_t *piece, double *end_headings)
{
    if (!F || F->roll_K < 1 || F->gear_total < 1) return RDA_ERR_ARG;
    if (piece) memcpy(piece, F->gr.piece.h, (size_t)F->B * sizeof(int32_t));
    if (end_headings) memcpy(end_headings, F->gr_endh.v.h, (size_t)F->gear_total * sizeof(double));
    return RDA_OK;
}
// every member's clearance at states [B][3] against its resident raw scene as it stands: the rollout's kernel, one launch, one wait
extern "C" int rda_fleet_clearance(rda_fleet *F, const double *states, double *clearance)
{
    if (!F || !states || !clearance) return RDA_ERR_ARG;
    const size_t B = F->B;
    int rc = fleet_check_clearance_call(F);
    if (rc != RDA_OK) return rc;
    FleetReserve rsv(F);
    rsv.need(&FleetSets::mov, B);
    rsv.grow(&FleetSets::cl_log, B, B);
    rc = rsv.adopt();
    if (rc == RDA_OK) rc = fleet_refresh(F);            // behind whatever the members still have queued
    if (rc != RDA_OK) return rc;
    MoveView v;
    fleet_move_view(F, v);
    rc = fleet_table(F, F->mov.cl, records(v.cl));
    if (rc != RDA_OK) return rc;
    HIPCHK(F->mov.st.upload(states, F->stream));
    hipLaunchKernelGGL(rollout::k_clearance_fleet, dim3((unsigned)B), dim3(rollout::CLEAR_NT), 0, F->stream, (const rollout::Clear *)F->mov.cl.d,
                       (const double *)F->mov.st.d, F->cl_log.v.d, (int)B);
    HIPCHK(hipGetLastError());
    HIPCHK(F->cl_log.v.pull(F->stream, B));
    HIPCHK(fleet_wait(F));
    memcpy(clearance, F->cl_log.v.h, B * sizeof(double));
    return RDA_OK;
}
// ---- members as each other's obstacles (scene::k_peers_fleet, rollout::k_peer_clearance_fleet) ---------------------------------------------------------
// The refresh of the peer rows from the caller's states and controls and the four re-sort launches behind it, on the fleet's stream
// plans (null: the constant-velocity mode): with plan_valid into the fleet's staging buffers, and scene::k_build_plan_fleet builds the slots
static int fleet_peers_resort(rda_fleet *F, const double *states, const double *controls, const double *plans, const int32_t *plan_valid)
{
    int nmax = 0, wmax = 0;
    int rc = fleet_resort_positions(F, states, 3, nmax, wmax);                  // (waits for an earlier copy out of the pinned mirrors)
    if (rc == RDA_OK) rc = fleet_peers_inputs(F, states, controls, plans, plan_valid);
    if (rc != RDA_OK) return rc;
    fleet_peers_launch(F, F->pe.st.d, F->pe.ctl.d);
    const scene::Plan pk{ F->pe.st.d, F->pl.plan.d, traj_s((size_t)F->T), F->pl.valid.d, nullptr };
    fleet_resort_launch(F, F->res.sc.d, F->res.rob.d, nmax, wmax, plans ? &pk : nullptr);
    HIPCHK(hipGetLastError());
    return RDA_OK;
}
// rda_fleet_upload_scenes with B - 1 peer rows behind every member's own obstacles.  Everything the call needs is allocated before anything of the fleet or
// of a member changes; the staging runs on the fleet's stream and the call returns when it is done.
// plan: the _plan entry (plans and plan_valid required)
static int fleet_upload_scenes_peers(rda_fleet *F, const int32_t *counts, const int32_t *kind, const int32_t *nvert, const double *geom, const double *vel,
                                     const double *states, const double *controls, bool plan, const double *plans, const int32_t *plan_valid)
{
    if (!F || !counts || !states || !controls || (plan && (!plans || !plan_valid))) return RDA_ERR_ARG;
    const size_t B = F->B;
    const int E = F->egos[0]->d.c.E, R = F->egos[0]->d.c.R, T = F->T;
    size_t total = 0;
    for (size_t i = 0; i < B; ++i) { if (counts[i] < 0) return RDA_ERR_ARG; total += (size_t)counts[i]; }
    if (total && (!kind || !nvert || !geom || !vel)) return RDA_ERR_ARG;
    if (!fleet_members_idle(F)) return RDA_ERR_ARG;
    if (!fleet_clearance_ok(F) || R > E || fleet_duals_follow(F)) return RDA_ERR_UNSUPPORTED;         // (a footprint is a polygon row of R <= E vertices)
    for (size_t e = 0; e < total; ++e) {                                        // scene_stage's rules
        if (kind[e] == 1) { if (E < 3) return RDA_ERR_UNSUPPORTED; }
        else if (kind[e] != 0 || nvert[e] < 0 || nvert[e] > E) return RDA_ERR_ARG;
    }
    if (B == 1 && counts[0] == 0) { F->egos[0]->d.obstacle_num = 0; return RDA_OK; }      // nothing written: stale A, b stay (rda_upload_scene with n = 0)
    FleetReserve rsv(F);
    std::vector<SceneGrow> grow(B);
    rsv.need(&FleetSets::pe, B);
    if (plan) rsv.need(&FleetSets::pl, B, (size_t)T);
    rsv.need(&FleetSets::res, B);
    for (size_t i = 0; i < B; ++i) rsv.refused |= scene_grow_alloc(F->egos[i], counts[i] + (int)B - 1, grow[i]);
    int rc = rsv.bad();
    if (rc == RDA_OK) rc = fleet_refresh(F);            // behind whatever the members still have queued ...
    if (rc == RDA_OK) rc = rsv.adopt(true);             // ... and done: the members' pinned staging blocks are free
    if (rc != RDA_OK) return rc;
    F->n_own.assign(counts, counts + B);
    size_t off = 0;
    for (size_t i = 0; i < B; ++i) {
        rda_handle *H = F->egos[i];
        const size_t own = (size_t)counts[i], n = own + B - 1;
        H->tick.pending_scene = 0;
        scene_grow_commit(H, grow[i]);
        // one pinned staging block -> its device mirror, one copy: the own rows as given; the peer rows as polygons of R vertices, zeroed until k_peers_fleet
        const SceneLayout l = scene_layout(n, (size_t)E);
        double *hb = (double *)H->sc.host.blk;
        memset(hb, 0, l.bytes);
        if (own) {
            memcpy(hb, geom + off * E * 2, own * E * 2 * sizeof(double));
            memcpy(hb + l.vel, vel + off * 2, own * 2 * sizeof(double));
            memcpy((int *)(hb + l.ints), kind + off, own * sizeof(int));
            memcpy((int *)(hb + l.ints) + n, nvert + off, own * sizeof(int));
        }
        hb[l.robot] = states[3 * i]; hb[l.robot + 1] = states[3 * i + 1];
        for (size_t r = own; r < n; ++r) ((int *)(hb + l.ints))[n + r] = R;
        HIPCHK(hipMemcpyAsync(H->sc.dev.blk, hb, l.bytes, hipMemcpyHostToDevice, F->stream));
        // per-stage slots always: the peer rows' velocities are known on the device only
        scene_bind(H, scene_args(H, (int)n, T + 1, 1), true);
        H->sc.peers_of = F;
        off += own;
    }
    std::vector<scene::Peer> pv;
    fleet_peer_view(F, pv);
    HIPCHK(mirror_upload(F->pe.tab, records(pv), F->stream));
    HIPCHK(mirror_upload(F->devs, member_devs(F), F->stream));
    rc = fleet_peers_resort(F, states, controls, plan ? plans : nullptr, plan_valid);
    if (rc != RDA_OK) return rc;
    HIPCHK(fleet_wait(F));                              // the staging blocks are reused by the next call; the members' own calls see the scene
    return RDA_OK;
}
extern "C" int rda_fleet_upload_scenes_peers(rda_fleet *F, const int32_t *counts, const int32_t *kind, const int32_t *nvert, const double *geom,
                                             const double *vel, const double *states, const double *controls)
{
    return fleet_upload_scenes_peers(F, counts, kind, nvert, geom, vel, states, controls, false, nullptr, nullptr);
}
extern "C" int rda_fleet_upload_scenes_peers_plan(rda_fleet *F, const int32_t *counts, const int32_t *kind, const int32_t *nvert, const double *geom,
                                                  const double *vel, const double *states, const double *controls, const double *plans,
                                                  const int32_t *plan_valid)
{
    return fleet_upload_scenes_peers(F, counts, kind, nvert, geom, vel, states, controls, true, plans, plan_valid);
}
// rda_fleet_scene_resort for scenes of the peers upload: the peer rows refreshed from states and controls, then the re-sort
static int fleet_scene_resort_peers(rda_fleet *F, const double *states, const double *controls, bool plan, const double *plans, const int32_t *plan_valid)
{
    if (!F || !states || !controls || (plan && (!plans || !plan_valid))) return RDA_ERR_ARG;
    for (size_t i = 0; i < (size_t)F->B; ++i) {
        if (!member_peers_scene(F, i) || F->egos[i]->tick.pending) return RDA_ERR_ARG;
        if (F->egos[i]->opts.duals_follow) return RDA_ERR_UNSUPPORTED;
    }
    FleetReserve rsv(F);
    if (plan) rsv.need(&FleetSets::pl, (size_t)F->B, (size_t)F->T);
    int rc = rsv.adopt();
    if (rc == RDA_OK) rc = fleet_refresh(F);
    if (rc == RDA_OK) rc = fleet_peer_table(F);
    if (rc != RDA_OK) return rc;
    return fleet_peers_resort(F, states, controls, plan ? plans : nullptr, plan_valid);
}
extern "C" int rda_fleet_scene_resort_peers(rda_fleet *F, const double *states, const double *controls)
{
    return fleet_scene_resort_peers(F, states, controls, false, nullptr, nullptr);
}
// ... with the peers predicted along their plans
extern "C" int rda_fleet_scene_resort_peers_plan(rda_fleet *F, const double *states, const double *controls, const double *plans, const int32_t *plan_valid)
{
    return fleet_scene_resort_peers(F, states, controls, true, plans, plan_valid);
}
// The rollout of a fleet whose members see each other: per tick the peer rows, the re-sort, the tick's tail on the own rows, the peer clearance
extern "C" int rda_fleet_rollout_peers(rda_fleet *F, int K, const double *states, const double *ref_speed, const int32_t *cur_index, double threshold,
                                       int ind_range, int goal_margin, const double *nom_u, const double *controls0, double *states_log, double *u_log,
                                       int32_t *index_log, rda_info *info_log, int32_t *arrived_at, double *clearance_log, double *peer_clearance_log)
{
    RollArgs a{ K, states, ref_speed, cur_index, threshold, ind_range, goal_margin, nom_u, states_log, u_log, index_log, info_log, arrived_at, clearance_log };
    a.peers = true; a.controls0 = controls0; a.peer_clearance_log = peer_clearance_log;
    return fleet_rollout_scenes(F, a, 1, true);
}
// ... with the peers predicted along their plans: tick 0 from plans0 / plan_valid0, tick k >= 1 from the states the members' solves of tick k - 1 planned
extern "C" int rda_fleet_rollout_peers_plan(rda_fleet *F, int K, const double *states, const double *ref_speed, const int32_t *cur_index, double threshold,
                                            int ind_range, int goal_margin, const double *nom_u, const double *controls0, double *states_log, double *u_log,
                                            int32_t *index_log, rda_info *info_log, int32_t *arrived_at, double *clearance_log, double *peer_clearance_log,
                                            const double *plans0, const int32_t *plan_valid0)
{
    RollArgs a{ K, states, ref_speed, cur_index, threshold, ind_range, goal_margin, nom_u, states_log, u_log, index_log, info_log, arrived_at, clearance_log };
    a.peers = true; a.controls0 = controls0; a.peer_clearance_log = peer_clearance_log;
    a.plan = true; a.plans0 = plans0; a.plan_valid0 = plan_valid0;
    return fleet_rollout_scenes(F, a, 1, true);
}
// every member's separation from the nearest other member at states [B][3]: the rollout's kernel, one launch, one wait
extern "C" int rda_fleet_peer_clearance(rda_fleet *F, const double *states, double *out)
{
    if (!F || !states || !out) return RDA_ERR_ARG;
    const size_t B = F->B;
    int rc = fleet_check_clearance_call(F);
    if (rc != RDA_OK) return rc;
    if (B == 1) { out[0] = INFINITY; return RDA_OK; }  // no peer, no launch
    FleetReserve rsv(F);
    rsv.need(&FleetSets::pe, B);
    rsv.grow(&FleetSets::pc_log, B, B);
    rc = rsv.adopt(F->rob_pending != 0);                // (pe.st below: the states of a re-sort that is still queued)
    if (rc == RDA_OK) rc = fleet_peer_table(F);
    if (rc != RDA_OK) return rc;
    HIPCHK(F->pe.st.upload(states, F->stream));
    fleet_peer_clearance_launch(F, F->pe.st.d, F->pc_log.v.d);
    HIPCHK(hipGetLastError());
    HIPCHK(F->pc_log.v.pull(F->stream, B));
    HIPCHK(fleet_wait(F));
    memcpy(out, F->pc_log.v.h, B * sizeof(double));
    return RDA_OK;
}
// ---- the members' worlds and the simulated sensor (lidar::k_raycast_fleet) -----------------------------------------------------------------------------
// Every member's world in one call, in the layout of rda_fleet_upload_scenes with its own vertex stride `we`.  Built beside the old world and moved in
// once everything is on the device: a refused call leaves the old world as it was.
extern "C" int rda_fleet_upload_worlds(rda_fleet *F, const int32_t *counts, int we, const int32_t *kind, const int32_t *nvert, const double *geom,
                                       const double *vel)
{
    if (!F || !counts || we < 3 || we > RDA_EMAX) return RDA_ERR_ARG;
    const size_t B = F->B;
    size_t total = 0;
    for (size_t i = 0; i < B; ++i) { if (counts[i] < 0) return RDA_ERR_ARG; total += (size_t)counts[i]; }
    if (total > 0 && (!kind || !nvert || !geom)) return RDA_ERR_ARG;
    for (size_t j = 0; j < total; ++j) {
        if (kind[j] == 0) { if (nvert[j] < 3 || nvert[j] > we) return RDA_ERR_ARG; }
        else if (kind[j] != 1) return RDA_ERR_ARG;
    }
    FleetReserve rsv(F);
    rsv.fresh(&FleetSets::world, B, counts, we);
    if (rsv.bad()) return RDA_ERR_HIP;
    FleetWorld &w = rsv.s.world;
    if (total > 0) {
        HIPCHK(hipMemcpy(w.geom, geom, total * we * 2 * sizeof(double), hipMemcpyHostToDevice));
        if (vel) HIPCHK(hipMemcpy(w.vel, vel, total * 2 * sizeof(double), hipMemcpyHostToDevice));   // (NULL: the zeros of the allocation - a standing world)
        HIPCHK(hipMemcpy(w.kind, kind, total * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(w.nvert, nvert, total * sizeof(int), hipMemcpyHostToDevice));
    }
    return rsv.adopt();                                   // (waits where there is an old world: a ray cast of it may still be queued)
}

// test hook: the resident worlds' geometry as it stands, member-major [total][we][2]
extern "C" int rda_debug_fleet_world(rda_fleet *F, double *geom, int32_t *n_total, int32_t *we)
{
    if (!F || !n_total) return RDA_ERR_ARG;
    const FleetWorld &w = F->world;
    *n_total = (int32_t)w.total;
    if (we) *we = w.e;
    if (w.total == 0 || !geom) return RDA_OK;
    HIPCHK(fleet_wait(F));
    HIPCHK(hipMemcpy(geom, w.geom, w.total * w.e * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return RDA_OK;
}

// the argument rules of the sensor arrays (rda_fleet_raycast, rda_fleet_rollout_lidar); total: the beams of all members
static int fleet_ray_check(const rda_fleet *F, const int32_t *n_beams, const double *angle_min, const double *angle_max, const double *range_min,
                           const double *range_max, size_t &total)
{
    if (!F || !n_beams || !angle_min || !angle_max || !range_min || !range_max || !F->world.have()) return RDA_ERR_ARG;
    total = 0;
    for (int i = 0; i < F->B; ++i) { if (n_beams[i] < 0) return RDA_ERR_ARG; total += (size_t)n_beams[i]; }
    for (int i = 0; i < F->B; ++i) if (n_beams[i] > lidar::MAXB) return RDA_ERR_UNSUPPORTED;
    return RDA_OK;
}
// the ray caster's member table for these sensors (member i's ranges at its beam offset in rays.v.d) -> device; returns the longest scan
static int fleet_ray_table(rda_fleet *F, const int32_t *n_beams, const double *angle_min, const double *angle_max, const double *range_min,
                           const double *range_max, int &maxb)
{
    const size_t B = F->B;
    FleetWorld &w = F->world;
    size_t off = 0;
    maxb = 0;
    for (size_t i = 0; i < B; ++i) {
        lidar::Ray &r = w.ray.h[i];
        memset((void *)&r, 0, sizeof(r));
        r.geom = w.geom + w.off[i] * w.e * 2; r.kind = w.kind + w.off[i]; r.nvert = w.nvert + w.off[i];
        r.n = w.counts[i]; r.E = w.e; r.n_beams = n_beams[i];
        r.angle_min = angle_min[i]; r.angle_max = angle_max[i]; r.range_min = range_min[i]; r.range_max = range_max[i];
        r.ranges = F->rays.v.d + off;
        off += (size_t)n_beams[i];
        maxb = n_beams[i] > maxb ? n_beams[i] : maxb;
    }
    HIPCHK(w.ray.push(F->stream));
    return RDA_OK;
}
// see: the form that also casts against the other members' footprints at `poses` (the peer table is on the device); a fleet of one has no peer to see
static void fleet_ray_launch(rda_fleet *F, const double *poses, int maxb, bool see = false)
{
    if (maxb <= 0) return;
    const dim3 grid((unsigned)((maxb + lidar::RAY_NT - 1) / lidar::RAY_NT), (unsigned)F->B);
    if (see && F->B > 1)
        hipLaunchKernelGGL(lidar::k_raycast_fleet_peers, grid, dim3(lidar::RAY_NT), 0, F->stream, (const lidar::Ray *)F->world.ray.d,
                           (const scene::Peer *)F->pe.tab.d, poses, F->B);
    else
        hipLaunchKernelGGL(lidar::k_raycast_fleet, grid, dim3(lidar::RAY_NT), 0, F->stream, (const lidar::Ray *)F->world.ray.d, poses);
}

// the resident worlds as they stand (see: and the other members at `states`), ray-cast from states [B][3]: one launch, one wait
static int fleet_raycast(rda_fleet *F, const int32_t *n_beams, const double *angle_min, const double *angle_max, const double *range_min,
                         const double *range_max, const double *states, double *ranges, bool see)
{
    size_t total = 0;
    int rc = fleet_ray_check(F, n_beams, angle_min, angle_max, range_min, range_max, total);
    if (rc != RDA_OK) return rc;
    if (!states || (total > 0 && !ranges)) return RDA_ERR_ARG;
    if (see && !fleet_clearance_ok(F)) return RDA_ERR_UNSUPPORTED;               // (a footprint needs the vertices of a polygon robot)
    FleetReserve rsv(F);
    rsv.grow(&FleetSets::rays, total, total);
    if (see) rsv.need(&FleetSets::pe, (size_t)F->B);
    rc = rsv.adopt();
    if (rc == RDA_OK && see) rc = fleet_peer_table(F);
    int maxb = 0;
    if (rc == RDA_OK) rc = fleet_ray_table(F, n_beams, angle_min, angle_max, range_min, range_max, maxb);
    if (rc != RDA_OK) return rc;
    HIPCHK(F->world.st.upload(states, F->stream));
    fleet_ray_launch(F, F->world.st.d, maxb, see);
    HIPCHK(hipGetLastError());
    if (total > 0) HIPCHK(F->rays.v.pull(F->stream, total));
    HIPCHK(fleet_wait(F));
    if (total > 0) memcpy(ranges, F->rays.v.h, total * sizeof(double));
    return RDA_OK;
}
extern "C" int rda_fleet_raycast(rda_fleet *F, const int32_t *n_beams, const double *angle_min, const double *angle_max, const double *range_min,
                                 const double *range_max, const double *states, double *ranges)
{
    return fleet_raycast(F, n_beams, angle_min, angle_max, range_min, range_max, states, ranges, false);
}
// ... with every member seeing the others' footprints at `states` too (lidar::k_raycast_fleet_peers); B = 1: rda_fleet_raycast
extern "C" int rda_fleet_raycast_peers(rda_fleet *F, const int32_t *n_beams, const double *angle_min, const double *angle_max, const double *range_min,
                                       const double *range_max, const double *states, double *ranges)
{
    return fleet_raycast(F, n_beams, angle_min, angle_max, range_min, range_max, states, ranges, true);
}

// ---- rda_fleet_rollout_lidar: the closed loop around the simulated sensor -------------------------------------------------------------------------------
// Per tick, on the fleet's stream: k_raycast_fleet from the pose the advance kernel left (row k of the device state log; row 0: the caller's) into
// rays.v.d, k_scan_fleet_at on those ranges at that pose, the ONE wait for the B box counts (they choose the LamMuZ launch form, apply the zero-box rule
// and size the staging launches - fleet_scan_stage), then the tick's tail as in fleet_rollout_scenes (fleet_roll_tail): k_track_fleet, the ADMM launches
// and k_rollout_advance, and behind them (moving) scene::k_move_fleet on the WORLD and (clearance_log) k_clearance_fleet against the world.  Everything is
// allocated before tick 0.
// see (rda_fleet_rollout_lidar_peers): the same ticks with k_raycast_fleet_peers in the ray caster's place - row k of the state log holds the poses of ALL
// members, arrived ones where they stand - and (a.peer_clearance_log) k_peer_clearance_fleet of state k + 1 behind the tail.
struct LidarArgs {
    const int32_t *n_beams; const double *angle_min, *angle_max, *range_min, *range_max; double eps; int min_samples; const int32_t *order; int moving;
    int32_t *nbox_log;
};
// track (rda_fleet_rollout_lidar_tracked): lidar::k_track_boxes_fleet behind every tick's scan kernel, in front of the wait, and the tracked staging.
static int fleet_rollout_lidar(rda_fleet *F, const RollArgs &a, const LidarArgs &s, bool see, const TrackArgs *track = nullptr)
{
    int rc = roll_check_args(F, a);
    if (rc != RDA_OK) return rc;
    if (!s.order || !(s.eps > 0) || s.min_samples < 1 || (track && track_check(*track))) return RDA_ERR_ARG;
    size_t total = 0;
    rc = fleet_ray_check(F, s.n_beams, s.angle_min, s.angle_max, s.range_min, s.range_max, total);
    if (rc == RDA_OK) rc = roll_check_members(F, a.cur_index);
    if (rc != RDA_OK) return rc;
    const size_t T = F->T, B = F->B;
    const int K = a.K;
    if (fleet_duals_follow(F) || F->egos[0]->d.c.E < 4) return RDA_ERR_UNSUPPORTED;      // (a box has four vertices)
    if ((a.clearance_log || see) && !fleet_clearance_ok(F)) return RDA_ERR_UNSUPPORTED;
    const bool peer_log = see && a.peer_clearance_log && B > 1;
    // a raw scene for the most boxes a member's beams can give, beside the members as the sets are beside the fleet | per tick: nothing to grow
    FleetReserve rsv(F);
    std::vector<SceneGrow> grow(B), none(B);
    rsv.need_rollout(K, a.clearance_log != nullptr);
    if (track) rsv.need(&FleetSets::tk, B);
    rsv.grow(&FleetSets::rays, total, total);
    if (see) rsv.need(&FleetSets::pe, B);
    if (peer_log) rsv.grow(&FleetSets::pc_log, (size_t)K * B, (size_t)K * B);
    for (size_t i = 0; i < B; ++i) if (s.n_beams[i] > 0) rsv.refused |= scene_grow_alloc(F->egos[i], s.n_beams[i], grow[i]);
    rsv.need_lidar(false);
    rc = rsv.bad();
    if (rc == RDA_OK) rc = fleet_refresh(F);                                    // behind whatever the members still have queued
    if (rc == RDA_OK) rc = rsv.adopt(true);                                     // (the lidar ticks rewrite the pinned tables whatever they hold)
    if (rc != RDA_OK) return rc;
    F->roll_K = 0; F->gear_total = 0;                                           // (until this rollout's logs are on the host)
    for (size_t i = 0; i < B; ++i) scene_grow_commit(F->egos[i], grow[i]);
    if (track) { rc = fleet_track_table(F, F->li, F->tk); if (rc != RDA_OK) return rc; }
    RollView rv;
    if (fleet_roll_view(F, a.nom_u != nullptr, rv)) { rc = fleet_roll_upload(F, rv); if (rc != RDA_OK) return rc; }
    if (see) { rc = fleet_peer_table(F); if (rc != RDA_OK) return rc; }
    const RollLayout lay = roll_layout((size_t)K, B, T);
    rollout::Logs lg;
    rc = fleet_roll_inputs(F, lay, a, lg);
    if (rc != RDA_OK) return rc;
    // the sensor, scan, move and clearance tables; tick 0's poses into row 0 of the device state log
    FleetLidar &li = F->li;
    FleetWorld &w = F->world;
    int maxb = 0, gmax = 0;
    rc = fleet_ray_table(F, s.n_beams, s.angle_min, s.angle_max, s.range_min, s.range_max, maxb);
    if (rc != RDA_OK) return rc;
    memcpy(w.st.h, a.states, 3 * B * sizeof(double));
    HIPCHK(hipMemcpyAsync(lg.states, w.st.h, 3 * B * sizeof(double), hipMemcpyHostToDevice, F->stream));
    {
        size_t off = 0;
        for (size_t i = 0; i < B; ++i) {
            lidar::Args &sa = li.args.h[i];
            memset((void *)&sa, 0, sizeof(sa));
            sa.n_beams = s.n_beams[i]; sa.ranges = F->rays.v.d + off; sa.angle_min = s.angle_min[i]; sa.angle_max = s.angle_max[i]; sa.range_max = s.range_max[i];
            sa.eps = s.eps; sa.min_samples = s.min_samples; sa.split_tol = F->scan_split;      // (the pose: k_scan_fleet_at's second argument)
            sa.boxes = li.d_boxes + i * lidar::MAXB * 8; sa.count = li.h_count + 2 * i;
            off += (size_t)s.n_beams[i];
            const size_t at = w.off[i];
            member_move_clear(F->egos[i], w.geom + at * w.e * 2, w.base + at * w.e * 2, w.vel + at * 2, w.kind + at, w.nvert + at, w.counts[i], w.e,
                              w.mv.h[i], w.cl.h[i]);
            gmax = w.counts[i] * w.e > gmax ? w.counts[i] * w.e : gmax;
        }
    }
    HIPCHK(li.args.push(F->stream));
    HIPCHK(w.mv.push(F->stream));
    HIPCHK(w.cl.push(F->stream));
    const bool moves = s.moving && gmax > 0;
    const dim3 gmove = fleet_move_grid(F, gmax, moves ? w.mv.d : nullptr);
    for (int k = 0; k < K; ++k) {
        const double *pose = lg.states + (size_t)k * B * 3;                     // where the advance kernel of tick k - 1 wrote the states
        for (size_t i = 0; i < B; ++i) { li.h_count[2 * i] = 0; li.h_count[2 * i + 1] = 0; }
        fleet_ray_launch(F, pose, maxb, see);
        hipLaunchKernelGGL(lidar::k_scan_fleet_at, dim3((unsigned)B), dim3(lidar::NT), lidar::LDS_BYTES, F->stream, (const lidar::Args *)li.args.d, pose);
        if (track) { fleet_track_launch(F, F->tk, *track); F->tk.par ^= 1; }
        HIPCHK(hipGetLastError());
        HIPCHK(fleet_wait(F));                                                  // the tick's one wait: the B box counts
        if (s.nbox_log) for (size_t i = 0; i < B; ++i) s.nbox_log[(size_t)k * B + i] = li.h_count[2 * i];
        rc = fleet_scan_stage(F, none, nullptr, pose, s.order, track != nullptr);
        if (rc == RDA_OK) rc = fleet_roll_tail(F, k, lg, a.goal_margin, nullptr, moves ? w.mv.d : nullptr, gmove, a.clearance_log ? w.cl.d : nullptr);
        if (rc != RDA_OK) return rc;
        if (peer_log) fleet_peer_clearance_launch(F, lg.states + (size_t)(k + 1) * B * 3, F->pc_log.v.d + (size_t)k * B);
    }
    HIPCHK(hipGetLastError());
    return fleet_roll_fetch(F, lay, a);
}
extern "C" int rda_fleet_rollout_lidar(rda_fleet *F, int K, const double *states, const double *ref_speed, const int32_t *cur_index, double threshold,
                                       int ind_range, int goal_margin, const double *nom_u, const int32_t *n_beams, const double *angle_min,
                                       const double *angle_max, const double *range_min, const double *range_max, double eps, int min_samples,
                                       const int32_t *order, int moving, double *states_log, double *u_log, int32_t *index_log, rda_info *info_log,
                                       int32_t *arrived_at, int32_t *nbox_log, double *clearance_log)
{
    const RollArgs a{ K, states, ref_speed, cur_index, threshold, ind_range, goal_margin, nom_u, states_log, u_log, index_log, info_log, arrived_at, clearance_log };
    return fleet_rollout_lidar(F, a, LidarArgs{ n_beams, angle_min, angle_max, range_min, range_max, eps, min_samples, order, moving, nbox_log }, false);
}
extern "C" int rda_fleet_rollout_lidar_peers(rda_fleet *F, int K, const double *states, const double *ref_speed, const int32_t *cur_index, double threshold,
                                             int ind_range, int goal_margin, const double *nom_u, const int32_t *n_beams, const double *angle_min,
                                             const double *angle_max, const double *range_min, const double *range_max, double eps, int min_samples,
                                             const int32_t *order, int moving, double *states_log, double *u_log, int32_t *index_log, rda_info *info_log,
                                             int32_t *arrived_at, int32_t *nbox_log, double *clearance_log, double *peer_clearance_log)
{
    RollArgs a{ K, states, ref_speed, cur_index, threshold, ind_range, goal_margin, nom_u, states_log, u_log, index_log, info_log, arrived_at, clearance_log };
    a.peer_clearance_log = peer_clearance_log;
    return fleet_rollout_lidar(F, a, LidarArgs{ n_beams, angle_min, angle_max, range_min, range_max, eps, min_samples, order, moving, nbox_log }, true);
}

extern "C" int rda_fleet_rollout_lidar_tracked(rda_fleet *F, int K, const double *states, const double *ref_speed, const int32_t *cur_index, double threshold,
                                               int ind_range, int goal_margin, const double *nom_u, const int32_t *n_beams, const double *angle_min,
                                               const double *angle_max, const double *range_min, const double *range_max, double eps, int min_samples,
                                               const int32_t *order, int moving, double *states_log, double *u_log, int32_t *index_log, rda_info *info_log,
                                               int32_t *arrived_at, int32_t *nbox_log, double *clearance_log, double *peer_clearance_log, int see, double gate,
                                               int window)
{
    RollArgs a{ K, states, ref_speed, cur_index, threshold, ind_range, goal_margin, nom_u, states_log, u_log, index_log, info_log, arrived_at, clearance_log };
    if (see) a.peer_clearance_log = peer_clearance_log;
    const TrackArgs t{ gate, window };
    return fleet_rollout_lidar(F, a, LidarArgs{ n_beams, angle_min, angle_max, range_min, range_max, eps, min_samples, order, moving, nbox_log }, see != 0, &t);
}

// What a caller that mirrors the members needs besides the logs, of the last tick of the last rollout: every member's full controls (the nominal controls
// of its next tick) and track::Out::end_heading (quirk Q12: what the heading of its path's last waypoint is now).  Either may be null.
extern "C" int rda_fleet_rollout_last(rda_fleet *F, double *out_u, double *end_heading)
{
    if (!F || F->roll_K < 1) return RDA_ERR_ARG;
    const RollLayout lay = roll_layout((size_t)F->roll_K, (size_t)F->B, (size_t)F->T);
    const size_t T = F->T;
    const double *last = (const double *)(F->ro_log.log.h + lay.last);
    if (out_u) for (size_t i = 0; i < (size_t)F->B; ++i) memcpy(out_u + i * traj_u(T), last + i * res_info(T), traj_u(T) * sizeof(double));
    if (end_heading) memcpy(end_heading, F->ro_log.log.h + lay.endh, (size_t)F->B * sizeof(double));
    return RDA_OK;
}
// ... and every member's planned states out_s [B][3][T+1] of that tick: plans0 of a rda_fleet_rollout_peers_plan or of a host-driven plan tick that continues
extern "C" int rda_fleet_rollout_last_plan(rda_fleet *F, double *out_s)
{
    if (!F || F->roll_K < 1 || !out_s) return RDA_ERR_ARG;
    const size_t T = F->T;
    const double *last = (const double *)(F->ro_log.log.h + roll_layout((size_t)F->roll_K, (size_t)F->B, T).last);
    for (size_t i = 0; i < (size_t)F->B; ++i) memcpy(out_s + i * traj_s(T), last + i * res_info(T) + res_s(T), traj_s(T) * sizeof(double));
    return RDA_OK;
}

// steps k0 .. k1-1 of every member's uploaded trace (rda_upload_trace), no host synchronisation; results are read with
// rda_fetch_result on the members after rda_fleet_sync
extern "C" int rda_fleet_enqueue_range(rda_fleet *F, int k0, int k1)
{
    if (!F || k0 < 0 || k0 > k1) return RDA_ERR_ARG;
    for (int i = 0; i < F->B; ++i) {
        rda_handle *H = F->egos[i];
        if (k1 > H->trace.K) return RDA_ERR_ARG;
        EgoIO &e = F->h_io[i];
        e.s = H->trace.s; e.u = H->trace.u; e.ref = H->trace.ref; e.speed = H->trace.speed;
        e.out_u = H->trace.out_u; e.out_s = H->trace.out_s; e.info = H->trace.info;
    }
    int rc = fleet_refresh(F);
    if (rc != RDA_OK) return rc;
    HIPCHK(hipMemcpyAsync(F->d_io_trace, F->h_io, F->B * sizeof(EgoIO), hipMemcpyHostToDevice, F->stream));
    for (int k = k0; k < k1; ++k) { rc = fleet_enqueue(F, F->d_io_trace, k); if (rc != RDA_OK) return rc; }
    return RDA_OK;
}

extern "C" int rda_fleet_sync(rda_fleet *F) { if (!F) return RDA_ERR_ARG; HIPCHK(fleet_wait(F)); return RDA_OK; }
extern "C" int rda_fleet_size(rda_fleet *F) { return F ? F->B : RDA_ERR_ARG; }

// ---- pure-function hooks ------------------------------------------------------------------------
extern "C" int rda_lammuz_batch(int B, int E, int R, const double *A, const double *b, const int32_t *cone,
                                const double *p, const double *phi, const double *G, const double *h,
                                const double *xi, const double *zeta, const double *dbar, double ro2, double delta,
                                int accelerated, double *lam, double *mu, double *z, double *cmh)
{
    if (B < 1 || E < 1 || E > RDA_EMAX || R < 1 || R > RDA_RMAX || E + R + 1 > 64) return RDA_ERR_UNSUPPORTED;
    if (rda_device_count() < 1) return RDA_ERR_NODEVICE;
    double *dA, *db, *dp, *dphi, *dG, *dh, *dxi, *dzeta, *ddbar, *dlam, *dmu, *dz, *dcmh; int *dcone;
    struct Cp { double **dst; const double *src; size_t n; };
    const size_t sB = (size_t)B;
    Cp ins[] = { {&dA, A, sB * E * 2}, {&db, b, sB * E}, {&dp, p, sB * 2}, {&dphi, phi, sB}, {&dG, G, (size_t)R * 2}, {&dh, h, (size_t)R},
                 {&dxi, xi, sB * 2}, {&dzeta, zeta, sB}, {&ddbar, dbar, sB} };
    hbuf::Group g;                                      // every buffer of the call, released on every way out
    for (auto &c : ins) { if (g.dev(c.dst, c.n)) return RDA_ERR_HIP; HIPCHK(hipMemcpy(*c.dst, c.src, c.n * 8, hipMemcpyHostToDevice)); }
    if (g.dev(&dcone, sB)) return RDA_ERR_HIP;
    HIPCHK(hipMemcpy(dcone, cone, sB * 4, hipMemcpyHostToDevice));
    if (g.dev(&dlam, sB * E) || g.dev(&dmu, sB * R) || g.dev(&dz, sB) || g.dev(&dcmh, sB * 4)) return RDA_ERR_HIP;
    rda_opts od; rda_opts_init(&od);                   // tie-break T1 of the defaults
    RobotCands rcands; rcands.nmv = robot_candidates(R, G, h, rcands.muc, rcands.rv, &rcands.nrv); rcands.centre = od.tie_centre ? 1 : 0;
    long long *dprof = nullptr;
#ifdef RDA_LMZ_PROF     // debug build only: phase cycles of sub-problem 0 on stderr
    if (g.dev(&dprof, 8)) return RDA_ERR_HIP;
#endif
    hipLaunchKernelGGL(k_lammuz_batch, dim3((B + 3) / 4), dim3(256), 0, 0, B, E, R, dA, db, dcone, dp, dphi, dG, dh, dxi, dzeta, ddbar,
                       ro2, delta, accelerated, dlam, dmu, dz, dcmh, dprof, rcands);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    if (dprof) {
        long long hp[8]; HIPCHK(hipMemcpy(hp, dprof, sizeof(hp), hipMemcpyDeviceToHost));
        fprintf(stderr, "lammuz prof (ticks, sub-problem 0): setup=%lld p1.it0=%lld p1.it1=%lld p2.it0=%lld p2.it1=%lld argmin1=%lld argmin2=%lld total=%lld\n",
                hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6], hp[7]);
    }
    HIPCHK(hipMemcpy(lam, dlam, sB * E * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(mu, dmu, sB * R * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(z, dz, sB * 8, hipMemcpyDeviceToHost));
    if (cmh) HIPCHK(hipMemcpy(cmh, dcmh, sB * 4 * 8, hipMemcpyDeviceToHost));
    return RDA_OK;
}

extern "C" int rda_su_solve_opts(const rda_cfg *cfg, const rda_opts *opts, const double *nom_s, const double *nom_u, const double *ref_s,
                            double ref_speed, const double *a, const double *cc, const double *g,
                            const double *d0, double *s, double *u, double *dd, int32_t *ipm_iters)
{
    if (!cfg || cfg->T < 1 || cfg->T > RDA_TMAX || cfg->N < 1) return RDA_ERR_UNSUPPORTED;
    if (rda_device_count() < 1) return RDA_ERR_NODEVICE;
    const size_t T = cfg->T, N = cfg->N, ns = traj_s(T), nu = traj_u(T);
    std::vector<double> soa(6 * T * N, 0.0);
    for (size_t n = 0; n < N; ++n) for (size_t t = 0; t < T; ++t) {
        size_t k = t * N + n;
        soa[0 * T * N + k] = a[(n * T + t) * 2]; soa[1 * T * N + k] = a[(n * T + t) * 2 + 1];
        soa[2 * T * N + k] = cc[n * T + t];
        soa[4 * T * N + k] = g[(n * T + t) * 2]; soa[5 * T * N + k] = g[(n * T + t) * 2 + 1];
    }
    double *dsoa, *dns, *dnu, *dref, *dspeed, *dd0, *dos, *dou, *dod; int *dst;
    hbuf::Group gb;                                     // every buffer of the call, released on every way out
    if (gb.dev(&dsoa, soa.size())) return RDA_ERR_HIP; HIPCHK(hipMemcpy(dsoa, soa.data(), soa.size() * 8, hipMemcpyHostToDevice));
    if (gb.dev(&dns, ns)) return RDA_ERR_HIP; HIPCHK(hipMemcpy(dns, nom_s, ns * 8, hipMemcpyHostToDevice));
    if (gb.dev(&dnu, nu)) return RDA_ERR_HIP; HIPCHK(hipMemcpy(dnu, nom_u, nu * 8, hipMemcpyHostToDevice));
    if (gb.dev(&dref, ns)) return RDA_ERR_HIP; HIPCHK(hipMemcpy(dref, ref_s, ns * 8, hipMemcpyHostToDevice));
    if (gb.dev(&dspeed, 1)) return RDA_ERR_HIP; HIPCHK(hipMemcpy(dspeed, &ref_speed, 8, hipMemcpyHostToDevice));
    if (gb.dev(&dd0, T)) return RDA_ERR_HIP;
    if (d0) HIPCHK(hipMemcpy(dd0, d0, T * 8, hipMemcpyHostToDevice));
    if (gb.dev(&dos, ns) || gb.dev(&dou, nu) || gb.dev(&dod, T) || gb.dev(&dst, 2)) return RDA_ERR_HIP;
    su::Args ar;
    ar.c.T = cfg->T; ar.c.N = cfg->N; ar.c.dynamics = cfg->dynamics; ar.c.accelerated = cfg->accelerated;
    ar.c.dt = cfg->dt; ar.c.L = cfg->L; ar.c.umax0 = cfg->max_speed[0]; ar.c.umax1 = cfg->max_speed[1];
    ar.c.ab0 = cfg->acce_bound[0]; ar.c.ab1 = cfg->acce_bound[1]; ar.c.ws = cfg->ws; ar.c.wu = cfg->wu;
    ar.c.slack_gain = cfg->slack_gain; ar.c.max_sd = cfg->max_sd; ar.c.min_sd = cfg->min_sd; ar.c.ro1 = cfg->ro1; ar.c.ro2 = cfg->ro2;
    const rda_opts od = opts_sanitised(opts);          // the stop tolerances / switches: the caller's, else the defaults
    ar.c.eps_u = cfg->eps_u; ar.c.tol_rd = od.su_tol[0]; ar.c.tol_rp = od.su_tol[1]; ar.c.tol_mu = od.su_tol[2];
    ar.split = od.su_split; ar.accept = od.su_accept; ar.first_attempt = od.su_first_attempt;
    ar.land = od.su_land; ar.land_rho = od.su_land_rho;
    for (int i = 0; i < 3; ++i) ar.land_tol[i] = od.su_land_tol[i];
    ar.in_s = dns; ar.in_u = dnu; ar.ref = dref; ar.ref_speed = dspeed;
    ar.ax = dsoa; ar.ay = dsoa + T * N; ar.cb = dsoa + 2 * T * N; ar.gx = dsoa + 4 * T * N; ar.gy = dsoa + 5 * T * N;
    ar.P = 1; ar.Nloc = (int)N; ar.chunk = 0;
    ar.d_in = d0 ? dd0 : nullptr; ar.out_s = dos; ar.out_u = dou; ar.out_d = dod; ar.status = dst; ar.ipm_iters = dst + 1;
    long long *dprof = nullptr;
    if (od.su_prof && gb.dev(&dprof, su::PROF_WORDS)) return RDA_ERR_HIP;
    ar.prof = dprof;
    double *ddbg = nullptr;
    if (od.su_prof > 1 && gb.dev(&ddbg, 400)) return RDA_ERR_HIP;
    ar.dbg = ddbg;
    const size_t lds = su::lds_bytes((int)T);
    RDA_SU_DISPATCH((int)T, HIPCHK(hipFuncSetAttribute((const void *)k_su_hook<TT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)));
    RDA_SU_DISPATCH((int)T, hipLaunchKernelGGL(k_su_hook<TT>, dim3(1), dim3(su::NT), lds, 0, ar));
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    int st[2];
    HIPCHK(hipMemcpy(st, dst, sizeof(st), hipMemcpyDeviceToHost));
    if (ddbg) {
        double hd[400]; HIPCHK(hipMemcpy(hd, ddbg, sizeof(hd), hipMemcpyDeviceToHost));
        for (int i = 0; i < 100 && (i == 0 || hd[4 * i + 3] != 0); ++i)
            fprintf(stderr, "it %d rdn %.3e rpn %.3e mu %.3e sc %.3e\n", i, hd[4 * i], hd[4 * i + 1], hd[4 * i + 2], hd[4 * i + 3]);
    }
    if (dprof) {
        long long hp[16]; HIPCHK(hipMemcpy(hp, dprof, sizeof(hp), hipMemcpyDeviceToHost));
        fprintf(stderr, "su prof (cycles) iters=%d:", st[1]); for (int i = 0; i < 16; ++i) fprintf(stderr, " [%d]=%lld", i, hp[i]); fprintf(stderr, "\n");
    }
    HIPCHK(hipMemcpy(s, dos, ns * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(u, dou, nu * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(dd, dod, T * 8, hipMemcpyDeviceToHost));
    if (ipm_iters) *ipm_iters = st[1];
    return st[0] == 0 ? 0 : 1;
}
extern "C" int rda_su_solve(const rda_cfg *cfg, const double *nom_s, const double *nom_u, const double *ref_s,
                            double ref_speed, const double *a, const double *cc, const double *g,
                            const double *d0, double *s, double *u, double *dd, int32_t *ipm_iters)
{
    return rda_su_solve_opts(cfg, nullptr, nom_s, nom_u, ref_s, ref_speed, a, cc, g, d0, s, u, dd, ipm_iters);
}
