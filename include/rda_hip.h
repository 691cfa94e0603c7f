/*
 * rda_hip.h - C-ABI of librda_hip.so, the MI355X-native RDA ADMM inner solver.
 *
 * Drop-in boundary: these entry points are what a ctypes / cffi binding inside
 * the reference's RDA_planner/rda_solver.py would call instead of CVXPY + pathos.  Plain
 * pointers and sizes only; every array is C-contiguous float64 (int32 for cone codes); host
 * pointers unless the name says `dev`.  The library owns all device memory and keeps no
 * caller pointer past a call.  Return value: 0 ok, >0 soft status, <0 hard error
 * (rda_strerror).  One HIP stream per handle; a handle is not thread-safe, distinct handles
 * are independent; no global state: everything that configures a solver travels in rda_cfg (the
 * reference's constructor arguments) and rda_opts (solver options that are not reference arguments),
 * both copied into the handle at creation.  The library reads NO environment variable (since round 5): the RDA_* switches of the
 * A/B tools are applied by the Python host package (rda_planner_amd.rda_solver.hip_options) to the rda_opts it hands over.
 *
 * reference interface replaced                       | entry point
 * ---------------------------------------------------+-------------------------------------
 * RDA_solver.__init__            rda_solver.py:18-61 | rda_create / rda_create_opts
 * assign_adjust_parameter        rda_solver.py:426   | rda_set_adjust
 * reset                          rda_solver.py:1060  | rda_reset
 * iterative_solve                rda_solver.py:573   | rda_step (host buffers in/out)
 * assign_obstacle_parameter      rda_solver.py:483   | rda_upload_obstacles
 * MPC.convert_rda_obstacle + sort mpc.py:189-218,440 | rda_upload_scene / rda_step_scene (caller-side obstacle pipeline on device)
 * rda_solver loop body           rda_solver.py:612   | rda_enqueue_step (device-resident inputs)
 * solve_parallel (pure function) rda_solver.py:743   | rda_lammuz_batch
 * su_prob_solve                  rda_solver.py:692   | rda_su_solve
 * para_*.value getters/setters   rda_solver.py:129   | rda_get_state / rda_set_state
 */
#ifndef RDA_HIP_H
#define RDA_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RDA_EMAX 8     /* max_edge_num supported by the kernels */
#define RDA_RMAX 8     /* robot half-spaces supported           */
#define RDA_TMAX 64    /* receding horizon supported            */

typedef struct rda_cfg {
    int32_t T;            /* receding                      rda_solver.py:34  */
    int32_t N;            /* max_obs_num                   rda_solver.py:38  */
    int32_t E;            /* max_edge_num                  rda_solver.py:39  */
    int32_t R;            /* car_tuple.G.shape[0]          rda_solver.py:99  */
    int32_t dynamics;     /* 0 acker, 1 diff, 2 omni       rda_solver.py:446 */
    int32_t accelerated;  /*                               rda_solver.py:47  */
    int32_t iter_num;     /*                               rda_solver.py:42  */
    int32_t robot_norm2;  /* car_tuple.cone_type=='norm2' (rda_solver.py:1034-1039): solved by the interior-point LamMuZ kernel */
    double dt, L;
    double max_speed[2];  /* rda_solver.py:37 */
    double acce_bound[2]; /* max_acce*dt, rda_solver.py:44 */
    double iter_threshold;
    double ws, wu;                                /* rda_solver.py:218-219 */
    double slack_gain, max_sd, min_sd, ro1, ro2;  /* rda_solver.py:196-201 */
    double delta;         /* tie-break T1 (clearance reward), 1e-6 */
    double eps_u;         /* tie-break for an undetermined steering column, 1e-8 */
} rda_cfg;

typedef struct rda_info {
    double resi_dual, resi_pri;   /* rda_solver.py:607-608 */
    int32_t iters;                /* ADMM iterations executed (early stop, :594) */
    int32_t su_status;            /* bit i: su-solve of iteration i not converged -> nominal kept (:699) */
    int32_t su_ipm_iters;         /* interior-point iterations, summed */
    int32_t lmz_fail;             /* (obstacle, stage) sub-problems that kept their previous duals - non-finite data or result; their
                                     residual is inf, which blocks the early stop like a non-OPTIMAL solve does (:781-793, :816-826) */
} rda_info;

typedef struct rda_handle rda_handle;

enum { RDA_OK = 0, RDA_ERR_ARG = -1, RDA_ERR_UNSUPPORTED = -2, RDA_ERR_HIP = -3, RDA_ERR_NODEVICE = -4 };

/* Solver options that are NOT arguments of the reference's constructor.  rda_opts_init fills the defaults below - and nothing else: the
 * library reads no environment variable (round 5; the RDA_* names in the right-hand column are switches of the Python host package,
 * rda_planner_amd.rda_solver.hip_options, which applies them to the struct it hands over).  A caller changes what it wants and hands the
 * struct to rda_create_opts, which copies it.  The first block is what a user may want to choose; the rest are the A/B switches of the kernels' restructurings -
 * every one of them changes where / when work is done, never the result (tests/test_gpu_switches.py). */
typedef struct rda_opts {
    int32_t lmz_mode;        /* 0 (default) support enumeration with the tie-breaks T1-T3 of DESIGN.md 2; 1 interior point ending on the
                                central path of the reference's own cone program at barrier parameter lmz_mu (interior duals like the
                                reference's solver returns, any combination of cones).  A norm2 robot always uses 1.     RDA_LMZ_MODE */
    int32_t tie_centre;      /* tie-break T1 in the slack regime: 1 (default) duals of the central separating normal, 0 max clearance.  RDA_TIE_CENTRE */
    double  lmz_mu;          /* 1e-6                                                                                      RDA_LMZ_MU */
    double  su_tol[3];       /* interior-point stop of the su-problem: |r_dual|_inf <= [0] (1+|grad|_inf), |r_prim|_inf <= [1], mean
                                complementarity <= [2] (1+|grad|_inf); 1e-9, 1e-10, 1e-11                                  RDA_SU_TOL */
    double  su_tol_early[3]; /* [0, 0, 0 = off] opt-in: the su-problems of the ADMM iterations BEFORE the last one of a step (it < iter_num - 1)
                                stop at these instead of su_tol.  The reference's own solver stops at ECOS defaults (1e-8 class) in EVERY
                                iteration; su_tol is 1000 x tighter because the parity tolerance is stated against it.  "1e-6,1e-7,1e-8":
                                two interior-point iterations fewer per su-problem.  A step that stops early returns the control of an
                                su-problem solved to THIS tolerance (some 1e-3 from the exact one where an inequality is weakly active,
                                tests/test_oracle_su.py), so the stated tolerance TOL_U does not hold with it.            RDA_SU_TOL_EARLY */
    double  su_hard_warm[2]; /* [1, 1e-3; 0, 0 = off] slack floor / barrier parameter of the warm attempts of a step that follows an UNCONVERGED step
                                (its ADMM used all iter_num iterations with a residual above iter_threshold) while consecutive su-problems are far
                                apart (the last solve's first iterate - the previous solution with its multipliers - had a relative dual residual
                                above 1e-2): a point well inside the boxes with the previous multipliers, a barrier of their own for the rows of the
                                safety distance; the cold-start rule is skipped there.  Same su-problems, same stop tolerance, another start: the
                                reference's default protocol (obstacle list re-sorted every tick, quirk Q5) needs 25 % fewer interior-point
                                iterations, converged loops are untouched.  Default since round 5 (it has been through the parity suite and the
                                soak; both keys are part of rda_get_su_history).                                          RDA_SU_HARD_WARM */
    /* ---- A/B switches (defaults in brackets) ---- */
    int32_t lmz_warm;        /* [1] try the remembered support first, then the supports one row away from it, before a row is
                                enumerated; every answer is accepted on its optimality certificate alone.  The supports are a cache of
                                the handle (not part of rda_get_state): they follow the source obstacle of a slot through the
                                re-binding of a re-sorted scene (rda_upload_scene*) and the horizon through the tick.  Circle obstacles
                                (norm2 cone) have one since round 5 in the single-ego launch form; in the dense forms and in a
                                fleet their rows are enumerated as before                                                RDA_LMZ_WARM */
    int32_t lmz_rows;        /* [1] four sub-problems per wave when E+R+1 <= 16                                        RDA_LMZ_ROWS */
    int32_t lmz_dense_from;  /* [256] grid size (CUs at one wave per SIMD) above which the split form of the LamMuZ launch is used; x 7/4 for moving scenes  RDA_LMZ_DENSE_FROM */
    int32_t lmz_split;       /* [1] dense grids: common-path kernel + work-list kernel + finalize                      RDA_LMZ_SPLIT */
    int32_t lmz_ip_rows;     /* [1] interior-point mode: the row-parallel kernel (16 lanes per sub-problem) when the shape allows
                                (0: one sub-problem per thread)                                                         RDA_LMZ_IP_ROWS */
    int32_t lmz_ip_warm;     /* [1] interior-point mode, row-parallel kernel: every sub-problem starts from the central-path point its last
                                solve ended on (same end point, 2 - 4 instead of ~9 iterations; solver history: rda_get_lmz_history) RDA_LMZ_IP_WARM */
    int32_t su_pre;          /* [1] the su set-up reads the block sums / near masks the LamMuZ launch wrote (0: evaluates every term) RDA_SU_PRE */
    int32_t su_light;        /* [1] convergence pass without the factorisation when the last step predicts convergence  RDA_SU_LIGHT */
    int32_t su_warm_first;   /* [1] the first su-problem of a step starts from the previous step's multipliers          RDA_SU_WARM_FIRST */
    int32_t su_warm_cap;     /* [30] iterations granted to a warm attempt                                               RDA_SU_WARM (3rd) */
    int32_t su_easy_max;     /* [2] easy mode while the last su-solve needed <= this many iterations (0 = never)        RDA_SU_EASY (6th) */
    int32_t su_easy_nopred;  /* [1] first iteration of an easy attempt without the predictor                            RDA_SU_EASY_NOPRED */
    int32_t su_cold_from;    /* [7] cold start after a solve with more iterations than this (0 = never) ...              RDA_SU_COLD_FROM */
    int32_t su_cold_probe;   /* [8] ... every this-many-th such solve tries the warm start                              RDA_SU_COLD_FROM (2nd) */
    int32_t zero_copy;       /* [1] result slot written into pinned host memory by the kernel, host polls a sequence word  RDA_ZERO_COPY */
    int32_t early_finish;    /* [1] the launch that detects the early stop hands the result over (0: k_finish does)      RDA_EARLY_FINISH */
    int32_t fuse_track;      /* [1] k_su_tracked (tracking beside su-problem 0; 0: k_track then k_su)                   RDA_FUSE_TRACK */
    int32_t su_prof;         /* [0] phase cycle counters of the su-solves (rda_debug_su_prof): PROFILING builds of the library only (-DSU_PROF /
                                -DSU_FINE, tools/su_phase_profile.py) - the product build refuses 1 with RDA_ERR_UNSUPPORTED   RDA_SU_PROF */
    int32_t su_split;        /* [1] su Newton system of the horizons 10, 20, 25, 30 cut in two halves that two waves factorise and sweep at
                                the same time, joined by a 5 x 5 interface system (same linear system, same answers up to rounding; 0: one
                                recursion over the whole horizon)                                                          RDA_SU_SPLIT */
    int32_t duals_follow;    /* [0] NOT reference semantics (opt-in).  The reference keeps lam, mu, z, xi, zeta per obstacle SLOT while its
                                default caller re-sorts the obstacle list on every tick (mpc.py:205-206), so after a re-sort most slots
                                continue from another obstacle's duals and the ADMM does not reach iter_threshold within iter_num (SURVEY
                                quirk Q5).  1: when the device pipeline re-binds the slots (rda_upload_scene*, rda_scene_resort) the dual
                                state moves WITH its obstacle - slot s takes the duals of the slot that held the same entry of the caller's
                                raw scene at the previous staging, an obstacle that was in no slot starts from the initial duals (zeros).
                                Obstacle i of the raw scene must denote the same obstacle from call to call.  The first su-problem of a
                                tick reads the terms of the previous tick's slots (as always).  Needs slots staged by the device pipeline
                                (rda_upload_obstacles / rda_step: RDA_ERR_UNSUPPORTED) and an unsharded handle.  rda_get_state /
                                rda_set_state speak the CURRENT slot order (rda_debug_slot_src tells which obstacle a slot holds); the
                                kept central points of the interior-point LamMuZ mode are dropped for a re-bound slot.  RDA_DUALS_FOLLOW */
    int32_t su_accept;       /* [1] safety net of the su interior point: the best iterate that is primal feasible to su_tol[1], dual feasible to
                                10 x su_tol[0] and complementary to 1000 x su_tol[2] (the class the reference's solver stops at) is remembered; a
                                solve whose every attempt then loses its end game in rounding (dual residual growing while the complementarity
                                falls below 1e-15, factorisation breaking down: one oracle solve in 32 000 soak steps) returns it instead of
                                'no update' (rda_solver.py:696-700).  Same rule as the oracle's orc_set_su_accept.  0: off; 2: test switch - every solve
                                hands back its remembered iterate (the path is otherwise never taken)                     RDA_SU_ACCEPT */
    int32_t su_first_attempt; /* [0] test switch: 1 = every su-solve starts with its LAST-RESORT attempt (plain long-step path following: no
                                predictor, fixed centring, lam w >= 1e-2 mu; normally reached only when the warm and the cold attempt have both
                                failed - csrc/su_device.h SU_SAFE_*).  Same solution, more iterations.                    (no env switch) */
    double  su_warm[2];      /* [1e-3, 1e-3] slack floor / barrier parameter of a warm start ("0,0" = always cold)      RDA_SU_WARM */
    double  su_warm_endgame[2]; /* [0.9999, 1e-5] floors of the fraction to the boundary / centering parameter, warm attempts  RDA_SU_WARM_ENDGAME */
    double  su_warm_clip;    /* [0.01]                                                                                  RDA_SU_WARM_CLIP */
    double  su_easy[5];      /* [1e-12, 1e-12, 1e-12, 0.999999, 1e-7] wfl, mu0, clip, tau, sigma of the easy start: the first three lie
                                BELOW the stop tolerances, i.e. the easy start is the previous solution itself and the stop test may
                                accept it without a Newton step when the new problem's optimality conditions hold there  RDA_SU_EASY */
    int32_t su_land;         /* [1] LANDING of the su interior point (round 6; oracle mirror orc_set_su_land): 1 = the interior point runs to
                                su_land_tol only - close enough for the active set to be read off (lam > w) - and the vertex it approaches is
                                computed exactly: active rows as equalities, the others dropped, the equality-constrained quadratic model solved
                                with the same factorisation and sweeps (two steps of the method of multipliers = the two passes of an iteration),
                                verified on the true objective, rows moved in / out by their signs for at most 4 rounds; refused -> the iterate
                                is restored and the iteration goes on; once every landing of an attempt has been refused it stops at 1e-3 x su_tol (SU_LAND_FALLBACK).  The answer no longer depends on WHERE on
                                the central path the iteration stopped (the reason for the stated tolerance of rounds 3-5, 5e-4: a row that is only just
                                active keeps the slack mu / lam*): kernel and cold oracle agree to 1e-9 with it (tests/test_gpu_land.py).
                                Costs one factorisation + a verification pass per solve, saves the last interior-point iteration.  RDA_SU_LAND */
    double  su_land_tol[3];  /* [1e-3, 1e-4, 1e-5] first stop of the interior point when it is landed; a refused landing is tried again at 1e-2^k x
                                these values (k = 1, 2, ... while they lie above su_tol), then the iteration stops at SU_LAND_FALLBACK x su_tol RDA_SU_LAND_TOL */
    double  su_land_rho;     /* [1e4] penalty of the landing's active rows, relative to the largest entry of the stage Hessians  RDA_SU_LAND_RHO */
    int32_t su_land_first;   /* [2] landing FIRST, for the warm-started su-problems (ADMM iterations >= 1: from the previous solution of the step and its multipliers; the first
                                one of a tick: from the previous tick's solution, shifted by one stage).
                                1: the first pass of the warm attempt is a light one (measures only - the start usually meets the landing's stop as it stands and the
                                factorisation of that pass was thrown away by the landing round anyway); results are bit-identical to 0.  2: ... and when the start
                                does not meet the stop the landing is tried all the same, from the start, active set = the rows whose kept multiplier exceeds the
                                slack, at most two rounds (a warm-started active-set method; accepted only on the verified optimality conditions of the true
                                problem, so the answer is the same vertex: differences at rounding level); refused: the interior point takes over.  RDA_SU_LAND_FIRST */
    int32_t su_land_blind_from; /* [1] with su_land_first = 2: after this many su-solves in a row that needed no interior-point iteration and one landing round, the next warm
                                su-problem of the same step starts WITH its landing round - no measuring pass in front of it (one round; refused: the interior
                                point takes over).  0 = never.                                                                  RDA_SU_LAND_BLIND_FROM */
} rda_opts;
void rda_opts_init(rda_opts *o);

int  rda_create(const rda_cfg *cfg, const double *G /*R*2*/, const double *h /*R*/, rda_handle **out);   /* = rda_create_opts(cfg, NULL, ...) */
int  rda_create_opts(const rda_cfg *cfg, const rda_opts *opts /* NULL: rda_opts_init */, const double *G, const double *h, rda_handle **out);
void rda_destroy(rda_handle *h);
int  rda_set_adjust(rda_handle *h, double slack_gain, double max_sd, double min_sd, double ro1, double ro2);
/* reset() of the reference (rda_solver.py:1060-1068): clears the lam'A / lam'b products, NOT the duals (quirk Q6); also clears the
 * handle's solver history (rda_get_su_history) */
int  rda_reset(rda_handle *h);
const char *rda_strerror(int code);
int  rda_device_count(void);
int  rda_set_device(int dev);     /* device used by handles created afterwards (one process per GPU).  HIP's current device belongs to the calling HOST THREAD
                                   * (default 0): a thread that drives handles or fleets created on device `dev` calls this once first.  The library keeps
                                   * no state outside its handles and fleets but the two debug counters of rda_debug_alloc_fail (per thread) and
                                   * rda_debug_alloc_stats (process-wide, atomic): distinct handles / fleets may be driven by distinct threads concurrently
                                   * (one thread at a time per handle or fleet) */

/* One MPC step, host buffers: nom_s 3x(T+1), nom_u 2xT, ref_s 3x(T+1) row-major;
 * obstacles A [n_obs][per_t? T+1 : 1][E][2], b [n_obs][per_t? T+1 : 1][E], cone [n_obs] (0 Rpositive, 1 norm2);
 * n_obs < N pads by duplicating the last obstacle, n_obs > N uses the first N, n_obs == 0 skips the
 * dual side (rda_solver.py:483-526,625).  out_u 2xT, out_s 3x(T+1). */
int  rda_step(rda_handle *h, const double *nom_s, const double *nom_u, const double *ref_s,
              double ref_speed, int n_obs, const double *A, const double *b, const int32_t *cone,
              int per_t, double *out_u, double *out_s, rda_info *info);

/* Caller-side obstacle pipeline on the device.  Replaces, per MPC tick: MPC.convert_rda_obstacle,
 * rda_obs_distance and the distance sort (mpc.py:189-218), convert_inequal_circle / convert_inequal_polygon with
 * the constant-velocity prediction `+ velocity * (t * dt)` (mpc.py:440-472), gen_inequal_global / is_convex_and_ordered
 * (mpc.py:476-549), and RDA_solver.assign_obstacle_parameter (rda_solver.py:483-526: first max_obs_num by distance,
 * padding with the last one, zeroed spare rows, per-t replication).  The solver's obstacle slots come out bit-identical
 * to what the Python caller stages.
 *   kind [n]      0 = polygon (cone 'Rpositive'), 1 = circle (cone 'norm2')
 *   nvert [n]     polygon vertex count, <= E (ignored for circles)
 *   geom [n][E][2] polygon: vertices in the caller's order (CW input is reversed like the reference does);
 *                  circle: geom[i][0] = centre, geom[i][1][0] = radius
 *   vel [n][2]    obstacle velocity; |vel| > 0.01 makes the obstacle time-varying over the horizon
 *   robot_xy [2]  robot position for the ordering (order != 0: nearest first, stable; order == 0: caller's order)
 *   n_nonconvex   (optional) number of staged polygons that fail the reference's convexity test (it prints a warning)
 * n == 0 leaves the slots untouched and skips the dual side, like rda_step. */
int  rda_upload_scene(rda_handle *h, int n, const int32_t *kind, const int32_t *nvert, const double *geom,
                      const double *vel, const double *robot_xy, int order, int32_t *n_nonconvex);
/* rda_step with the obstacle conversion done on the device */
int  rda_step_scene(rda_handle *h, const double *nom_s, const double *nom_u, const double *ref_s, double ref_speed,
                    int n, const int32_t *kind, const int32_t *nvert, const double *geom, const double *vel,
                    const double *robot_xy, int order, double *out_u, double *out_s, rda_info *info);
/* test hook: staged slots A [N][nt][E][2], b [N][nt][E], cone [N]; *nt = 1 or T+1 (buffers sized for T+1) */
int  rda_get_obstacles(rda_handle *h, double *A, double *b, int32_t *cone, int32_t *nt);
/* test hook: the resident raw geometry [n][E][2] of the device pipeline as it stands (rda_fleet_rollout_moving advances it on the device); *n = 0: none */
int  rda_debug_scene_geom(rda_handle *h, double *geom /*n*E*2*/, int32_t *n);
/* ... and its velocities [n][2] (the peer rows of rda_fleet_upload_scenes_peers are written on the device) */
int  rda_debug_scene_vel(rda_handle *h, double *vel /*n*2*/, int32_t *n);

/* Device-resident pipeline (what bench.py times): obstacles and a trace of K step inputs are
 * uploaded once; rda_enqueue_step queues the whole ADMM loop of step k on the handle's stream
 * without any host synchronisation; results land in device slot k and are fetched afterwards. */
int  rda_upload_obstacles(rda_handle *h, int n_obs, const double *A, const double *b, const int32_t *cone, int per_t);
int  rda_upload_trace(rda_handle *h, int K, const double *nom_s /*K*3*(T+1)*/, const double *nom_u /*K*2*T*/,
                      const double *ref_s /*K*3*(T+1)*/, const double *ref_speed /*K*/);
int  rda_enqueue_step(rda_handle *h, int k);
int  rda_enqueue_range(rda_handle *h, int k0, int k1);      /* steps k0 .. k1-1, one host call */
int  rda_sync(rda_handle *h);
int  rda_fetch_result(rda_handle *h, int k, double *out_u, double *out_s, rda_info *info);
/* elapsed GPU time (ms, hipEvent) of the launches named `which` (0 = LamMuZ, 1 = su, 2 = the shard all-gather) over the
 * steps enqueued since the last rda_timing_reset, and the number of launches */
int  rda_timing_reset(rda_handle *h, int enable);
int  rda_timing_read(rda_handle *h, int which, double *total_ms, int *launches);
/* the same per launch, in launch order: ms_out[i] for i < min(cap, *launches).  The early stop of rda_solver.py:594 is a
 * device flag, so launches queued behind it return at once; a caller that knows the executed ADMM iterations (rda_info.iters)
 * separates the two populations with this (bench.py: roofline per EXECUTED launch) */
int  rda_timing_launches(rda_handle *h, int which, double *ms_out, int cap, int *launches);
/* the LamMuZ launches of an ADMM iteration as the library plans them for this handle's shape and staged obstacles (kernel names joined by '+').
 * The string lives in the handle: valid until the next call on the same handle ("" for a null handle) */
const char *rda_lammuz_kernel(rda_handle *h);

/* ---- caller-side nominal roll-out + reference sampling on the device ------------------------------
 * What MPC.pre_process (mpc.py:251-291) with closest_point / inter_point / range_cir_seg / wraptopi and the three
 * motion_predict_model_* (mpc.py:293-433) computes per tick, as a device kernel in front of the ADMM loop: the caller
 * hands over the robot state, the signed reference speed and its path index instead of the 3x(T+1) nominal states
 * and reference.  rda_upload_path stores the polyline (L waypoints x, y, heading; row-major [L][3]).  The last
 * waypoint's heading is rewritten by a tick that reaches the end of the path exactly like the reference rewrites it
 * in place (quirk Q12); `end_heading` returns it so a host mirror of the path can follow.
 * nom_u: the nominal controls [2][T] (MPC.cur_vel_array), or NULL = the controls of the previous solve, which are
 * still resident (what cur_vel_array holds unless the caller replaced it).  min_index = the new MPC.cur_index.
 * nom_s_out / ref_out (may be NULL) return the 3x(T+1) nominal states / reference the solver was given. */
/* Number of polygons of the scene the LAST completed step ran on that fail the reference's convexity test (mpc.py:476-549 prints
 * "Warning: The polygon constructed by vertex is not convex" for each); 0 when the obstacles were staged as (A, b) slots.  Travels
 * with the step's result, costs no synchronisation (rda_upload_scene's n_nonconvex is the synchronous form). */
int  rda_last_nonconvex(rda_handle *h);
int  rda_upload_path(rda_handle *h, int L, const double *path /*L*3*/);
/* All gear pieces of a path at once (MPC.split_path / curve_list of an enable_reverse path), for rda_fleet_rollout_gears: P pieces of len[p] waypoints and
 * gear[p] = +1 / -1, `path` the pieces one behind the other, row-major [sum len][3].  They live in a buffer of their own, owned by the handle: rda_upload_path's
 * path and everything that reads it are not touched.  A plain path is one piece with gear +1.  The last waypoint's heading of EVERY piece is rewritten by the
 * ticks that reach its end (quirk Q12).  RDA_ERR_ARG: P < 1, a len < 1, a missing array.  A new upload replaces the old pieces once it holds everything: a
 * refused allocation (RDA_ERR_HIP) leaves them in place. */
int  rda_upload_path_pieces(rda_handle *h, int P, const int32_t *len /*P*/, const double *gear /*P*/, const double *path /*sum(len)*3*/);
int  rda_step_tracked(rda_handle *h, const double *state /*3*/, double ref_speed, int cur_index, double threshold, int ind_range,
                      const double *nom_u, double *out_u, double *out_s, rda_info *info,
                      double *nom_s_out, double *ref_out, int32_t *min_index, double *end_heading);
/* The same tick in two halves, so that the caller's per-tick obstacle work overlaps the first su-problem.  The first
 * su-problem of a step reads the nominal trajectory and the lam'A / lam'b products of the PREVIOUS step (the reference never
 * refreshes them before rda_solver.py:591 - SURVEY quirk Q4) and nothing of the obstacles staged for this tick, so
 *   rda_tracked_begin        queues k_track, the step reset and su-problem 0 and returns at once;
 *   rda_upload_scene_async   (optional) stages this tick's raw scene like rda_upload_scene, without waiting; also usable on
 *                            its own when the caller's next call on the handle synchronises (rda_sync, a step, a fleet
 *                            step) - a second upload before that waits for the first one;
 *                            rda_upload_obstacles / rda_upload_scene may be used instead (they synchronise);
 *   rda_tracked_finish       queues the rest of the ADMM loop, waits, returns what rda_step_tracked returns.
 * Results are bit-identical to rda_upload_scene + rda_step_tracked (same kernels, same order of dependent work).
 * Between begin and finish only the upload calls may be used on the handle. */
int  rda_tracked_begin(rda_handle *h, const double *state /*3*/, double ref_speed, int cur_index, double threshold, int ind_range,
                       const double *nom_u);
int  rda_upload_scene_async(rda_handle *h, int n, const int32_t *kind, const int32_t *nvert, const double *geom,
                            const double *vel, const double *robot_xy, int order);
int  rda_tracked_finish(rda_handle *h, double *out_u, double *out_s, rda_info *info,
                        double *nom_s_out, double *ref_out, int32_t *min_index, double *end_heading);
/* The reference re-sorts the caller's obstacle list by distance to the robot on EVERY tick (MPC.convert_rda_obstacle with
 * obstacle_order=True, its default: mpc.py:205-206) and stages the first max_obs_num.  For a raw scene that is already resident
 * (rda_upload_scene / rda_upload_scene_async) rda_scene_resort re-ranks it about robot_xy and rebuilds the obstacle slots with the same
 * kernels (k_keys / k_rank / k_build / k_prepare): the position travels in the kernel arguments, nothing is copied.  Asynchronous like
 * rda_upload_scene_async and usable between rda_tracked_begin and rda_tracked_finish.  Slots come out bit-identical to uploading the
 * same scene again with order = 1.  A scene whose obstacles MOVE between ticks has to be uploaded again instead (the prediction over
 * the horizon starts from the uploaded geometry).  RDA_ERR_ARG without a resident raw scene. */
int  rda_scene_resort(rda_handle *h, const double *robot_xy /*2*/);

/* ---- lidar front end on the device -----------------------------------------------------------------
 * What the reference's lidar example does per tick in host Python before MPC.control (`scan_box`,
 * example/lidar_nav/lidar_path_track.py:20-60): range scan -> hit points in the sensor frame -> DBSCAN(eps, min_samples) ->
 * one minimum-area rectangle per cluster -> 4-vertex 'Rpositive' obstacles in the world frame.  One kernel of one workgroup,
 * the points in LDS; the semantics are those of rda_planner_amd/lidar.py stage by stage:
 *   beam i has the angle angle_min + i (angle_max - angle_min) / (n_beams - 1), the last one exactly angle_max; it is a hit
 *   iff range < range_max - 0.01 (a NaN range is a miss); hits keep the beam order;
 *   DBSCAN labels as scikit-learn gives them (core: >= min_samples points within eps, itself included; clusters numbered by
 *   their smallest core point; a border point joins the lowest-numbered cluster in reach; noise -1);
 *   the rectangle has a side on an edge of the cluster's convex hull (least area, the first such edge among equals), an
 *   extent below 1 cm is widened to it; corners counter-clockwise; state = sensor pose (x, y, heading) in the world frame.
 * Fewer than 4 hits give no box.  n_beams <= 4096 and a handle with E >= 4, else RDA_ERR_UNSUPPORTED; eps <= 0,
 * min_samples < 1, n_beams < 0 or a missing array: RDA_ERR_ARG.
 * scan -> boxes, returned to the host (the drop-in for the reference's scan_box; also the test hook).
 * boxes [cap][4][2] world frame, CCW; labels [n_beams]: -2 miss, -1 noise, >= 0 cluster (either may be NULL).
 * *n_boxes = clusters found (may exceed cap: the first cap are written). */
int  rda_scan_boxes(rda_handle *h, int n_beams, const double *ranges, double angle_min, double angle_max, double range_max,
                    const double *state /*3*/, double eps, int min_samples,
                    int32_t *n_boxes, double *boxes, int cap, int32_t *labels);
/* the same scan staged as the handle's obstacles: equivalent to rda_upload_scene(order) of those boxes with robot_xy = state[0..1],
 * but the boxes go device to device into the resident raw scene (rda_scene_resort works on it afterwards); only the 4-byte box
 * count is read back (it sizes the scene launches and decides the n == 0 rule: slots untouched, dual side skipped).  The scan
 * kernel runs on the handle's second stream: between rda_tracked_begin and rda_tracked_finish the wait for the count is not a
 * wait for the first su-problem, and the conversion kernels run beside it like those of rda_upload_scene_async.  Outside a
 * tick the staging is asynchronous like rda_upload_scene_async.  With rda_timing_reset(h, 1) the scan kernels are timed as
 * launches `which` = 3 of rda_timing_read / rda_timing_launches. */
int  rda_upload_scan(rda_handle *h, int n_beams, const double *ranges, double angle_min, double angle_max, double range_max,
                     const double *state /*3*/, double eps, int min_samples, int order, int32_t *n_boxes /* may be NULL */);

/* ---- Fleet: B independent egos advanced together (BASELINE config C5, "batched multi-ego") -------------------
 * The reference plans one robot per RDA_solver object (rda_solver.py:54-109) and a multi-robot user loops over
 * objects.  Here the members stay ordinary handles (own state, obstacles, trace, accessors); the fleet launches
 * their ADMM iterations as ONE grid with an ego dimension, which is what fills the 256 CUs.  Members must agree on
 * T, N, E, R and iter_num (weights, bounds, kinematics, robot polygons and obstacles may differ), must live on the
 * current device and must not be obstacle shards.  Results are identical to stepping every member with rda_step /
 * rda_enqueue_step.  Between rda_fleet_enqueue_range and rda_fleet_sync the members must not be used.
 * LamMuZ mode: ALL members or NONE run the interior-point mode (rda_opts::lmz_mode = 1; lmz_mu may differ per member) - a mix is
 * RDA_ERR_UNSUPPORTED.  Every fleet entry (step, tracked step, trace replay, the three rollouts) serves such a fleet; the launch form
 * is chosen per member by the rule of a solo handle (the row-parallel kernel where the shape allows it and obstacles are staged, else
 * the per-thread kernel), the kept central-path points stay in the members (rda_get / rda_set_lmz_history between fleet ticks).
 * A member with a norm2 (circle) robot is refused with RDA_ERR_UNSUPPORTED: out of scope (the clearance log has no circle-robot form). */
typedef struct rda_fleet rda_fleet;
int  rda_fleet_create(rda_handle *const *egos, int B, rda_fleet **out);   /* does not take ownership of the members */
void rda_fleet_destroy(rda_fleet *f);
int  rda_fleet_size(rda_fleet *f);
/* the fleet counterpart of rda_lammuz_kernel: the LamMuZ launches the next fleet tick issues per ADMM iteration as the members stand now
 * (kernel names joined by '+').  Enumeration fleets: "k_lammuz_fleet_rows_fast+k_lammuz_fleet_enum+k_lmz_finalize_fleet", "k_lammuz_fleet_rows" or
 * "k_lammuz_fleet+k_lmz_finalize_fleet".  Interior-point fleets: "k_lammuz_ip_fleet" when every member runs the row-parallel form,
 * "k_lammuz_cp_fleet_small|large+k_lmz_finalize_fleet" when none does, all three names when both forms have members.
 * The string lives in the fleet: valid until the next call on the same fleet ("" for a null fleet). */
const char *rda_fleet_lammuz_kernel(rda_fleet *f);
/* one synchronous MPC step of every member with the obstacles each member has staged (rda_upload_obstacles /
 * rda_upload_scene): per-ego arrays of rda_step, concatenated ego-major */
int  rda_fleet_step(rda_fleet *f, const double *nom_s /*B*3*(T+1)*/, const double *nom_u /*B*2*T*/,
                    const double *ref_s /*B*3*(T+1)*/, const double *ref_speed /*B*/,
                    double *out_u /*B*2*T*/, double *out_s /*B*3*(T+1)*/, rda_info *info /*B, may be NULL*/);
/* rda_upload_scene_async for every member in one call: member i owns counts[i] consecutive entries of kind / nvert / geom /
 * vel, robot_xy [B][2], order [B].  No waiting: the next fleet step orders itself behind the staging and synchronises. */
int  rda_fleet_upload_scenes(rda_fleet *f, const int32_t *counts /*B*/, const int32_t *kind, const int32_t *nvert, const double *geom,
                             const double *vel, const double *robot_xy /*B*2*/, const int32_t *order /*B*/);
/* rda_step_tracked for every member (paths uploaded with rda_upload_path on the members); per-ego arrays ego-major,
 * nom_u NULL = every member's resident controls */
int  rda_fleet_step_tracked(rda_fleet *f, const double *states /*B*3*/, const double *ref_speed /*B*/, const int32_t *cur_index /*B*/,
                            double threshold, int ind_range, const double *nom_u /*B*2*T or NULL*/,
                            double *out_u, double *out_s, rda_info *info, double *ref_out /*B*3*(T+1) or NULL*/,
                            int32_t *min_index /*B*/, double *end_heading /*B*/);
/* rda_scene_resort for every member in ONE launch set: the members' resident raw scenes (rda_upload_scene*, obstacles that do not move between ticks) re-ranked
 * about states[i * stride + 0..1] (stride >= 2: the caller's [B][3] state array serves) and their slots rebuilt on the fleet's stream; the next fleet step runs
 * behind it.  Replaces one MPC.convert_rda_obstacle + distance sort per robot and tick (mpc.py:189-218, obstacle_order=True).  Slots bit-identical to
 * rda_scene_resort on each member.  Until the next fleet step has returned the members must not be used on their own. */
int  rda_fleet_scene_resort(rda_fleet *f, const double *states, int stride);
/* Fleet lidar: rda_scan_boxes / rda_upload_scan for every member in ONE scan launch (a workgroup, and so a compute unit, per member; the reference's
 * scan_box runs once per robot and tick, example/lidar_nav/lidar_path_track.py:20-60).  Per-member arrays are member-major; `ranges` is the
 * concatenation of the members' scans (member i owns n_beams[i] consecutive entries, counts may differ, 0 = no scan: no box); states [B][3] are the
 * sensor poses.  Same device code per member as the solo calls: counts, boxes, labels and staged slots are bit-identical to theirs.  Argument rules
 * of the solo calls, for every member: a missing array, eps <= 0, min_samples < 1 or a negative beam count: RDA_ERR_ARG; a member with more than
 * 4096 beams, E < 4, or (upload) a member with rda_opts::duals_follow: RDA_ERR_UNSUPPORTED - nothing is staged for any member then.  A refused
 * allocation: RDA_ERR_HIP, fleet and members as they were.
 * scans -> boxes, returned to the host: n_boxes [B] = clusters found per member (may exceed cap: the first cap are written), boxes [B][cap][4][2]
 * world frame, CCW; labels at the member's offset in `ranges`: -2 miss, -1 noise, >= 0 cluster (boxes with cap = 0, and labels, may be NULL). */
int  rda_fleet_scan_boxes(rda_fleet *f, const int32_t *n_beams /*B*/, const double *ranges, const double *angle_min /*B*/,
                          const double *angle_max /*B*/, const double *range_max /*B*/, const double *states /*B*3*/,
                          double eps, int min_samples, int32_t *n_boxes /*B*/, double *boxes /*B*cap*4*2 or NULL*/, int cap,
                          int32_t *labels /*sum of n_beams, or NULL*/);
/* the same scans staged as every member's obstacles, each exactly as rda_upload_scan(order[i]) stages it on the member (resident raw scene for a later
 * rda_fleet_scene_resort / rda_scene_resort; zero boxes: obstacle count 0, slots untouched, dual side skipped): one pinned copy of all ranges, one scan
 * launch, ONE wait for the B box counts, then boxes -> raw scenes -> slots -> candidate lists of all members by five launches whatever B is.  Everything
 * runs on the fleet's stream, behind whatever the members still have queued; the next fleet step runs behind it.  As with rda_fleet_scene_resort: until
 * rda_fleet_sync or the next fleet step has returned the members must not be used on their own (a member inside rda_tracked_begin: RDA_ERR_ARG). */
int  rda_fleet_upload_scans(rda_fleet *f, const int32_t *n_beams, const double *ranges, const double *angle_min,
                            const double *angle_max, const double *range_max, const double *states /*B*3*/,
                            double eps, int min_samples, const int32_t *order /*B*/, int32_t *n_boxes /*B or NULL*/);
/* Fleet rollout: K closed-loop ticks of every member queued back to back on the fleet's stream, ONE host wait - the loop a caller otherwise runs around
 * rda_fleet_scene_resort + rda_fleet_step_tracked (tools/closed_loop_host.c closed_loop_fleet_run), with the host's part between two ticks done by a
 * kernel: the member's first control is applied to its kinematic model (its own dynamics, dt, wheelbase; the expressions of that C loop, separately
 * rounded), the new state and min_index become the next tick's tracker input and (resort != 0) re-sort position.  Arrival as in MPC.control
 * (mpc.py:166-187): on the first tick k with min_index >= path length - goal_margin, arrived_at[i] = k and the applied control is zero on that tick and on
 * every later one (the member keeps being stepped from its standing state: its solver state is then only good for rda_reset).
 * states [B][3], ref_speed [B] (signed), cur_index [B], threshold, ind_range, nom_u: tick 0's inputs as in rda_fleet_step_tracked (nom_u NULL = the resident
 * controls; later ticks always use them).  Logs, member-major per tick: states_log [K+1][B][3] (row 0 = states, row k+1 = after tick k), u_log [K][B][2] the
 * applied controls, index_log [K][B] min_index, info_log [K][B] (may be NULL), arrived_at [B] (-1 = not arrived).  During a rollout the results stay in device
 * memory whatever rda_opts::zero_copy says; given a state, a tick computes bit for bit what rda_fleet_scene_resort + rda_fleet_step_tracked compute.
 * RDA_ERR_ARG: K < 1, K > 4096, a missing array, ind_range < 1, goal_margin < 1, a member without an uploaded path, with cur_index out of range, inside
 * rda_tracked_begin, or (resort != 0) without a resident raw scene / with no staged obstacle.  RDA_ERR_UNSUPPORTED: a member with rda_opts::duals_follow or
 * whose staged obstacles move (per-stage slots: such a scene has to be uploaded again every tick, as with rda_scene_resort).  A refused call queues nothing;
 * a refused allocation: RDA_ERR_HIP, fleet and members as they were.  Afterwards the fleet and the members are as K host-driven ticks leave them: an
 * ordinary rda_fleet_step_tracked from states_log[K] continues the loop. */
int  rda_fleet_rollout(rda_fleet *f, int K, const double *states /*B*3*/, const double *ref_speed /*B*/,
                       const int32_t *cur_index /*B*/, double threshold, int ind_range, int goal_margin, int resort,
                       const double *nom_u /*B*2*T or NULL = resident*/,
                       double *states_log /*(K+1)*B*3*/, double *u_log /*K*B*2*/, int32_t *index_log /*K*B*/,
                       rda_info *info_log /*K*B, may be NULL*/, int32_t *arrived_at /*B, -1 = not arrived*/);
/* of the last tick of the last rda_fleet_rollout, what rda_fleet_step_tracked returns besides the logged values: every member's full controls out_u (the
 * resident nominal controls of its next tick) and end_heading (the heading of the last waypoint of the member's device path, quirk Q12) - for a caller that
 * mirrors the members on the host, like Fleet.rollout.  No device work.  RDA_ERR_ARG before the first rollout. */
int  rda_fleet_rollout_last(rda_fleet *f, double *out_u /*B*2*T or NULL*/, double *end_heading /*B or NULL*/);
/* The rollout for scenes that MOVE between ticks (BASELINE config C4, the reference's dynamic_obs loop): rda_fleet_rollout's arguments, logs, arrival rule
 * and refusals, but members whose staged obstacles move (per-stage slots) are taken, and members with static scenes may be mixed in.  `base` is every
 * member's resident raw geometry as the call finds it (snapshot on the device); at tick k of the call the resident geometry is base + vel * (dt * k) - one
 * product dt * k, one product, one sum, each rounded separately; polygons: their nvert vertices; circles: the centre, never the radius - and the tick's
 * per-stage slots are rebuilt from it by the launches of rda_fleet_scene_resort.  Every obstacle with a velocity moves, also below the 0.01 m/s under which
 * motion is not PREDICTED (tools/closed_loop_host.c:60-66).  No world-border reflection.  After the call the resident geometry is where the obstacles are
 * when tick K would start: rda_fleet_scene_resort + rda_fleet_step_tracked continue the loop, a second rollout takes it as its base.
 * resort != 0: re-ranked about the advancing robot on every tick; resort = 0: rebuilt in the staged order (members staged with order = 0 only).
 * Given a state, tick k computes bit for bit what rda_fleet_upload_scenes (the geometry of tick k, robot_xy = the state, the same order) +
 * rda_fleet_step_tracked compute.  clearance_log [K][B] (may be NULL): member i's clearance after tick k - state k+1 against ALL obstacles of its raw scene
 * at tick k+1 (scenarios.clearance for a polygon robot: separating axes against polygons, centre-to-edge distance minus the radius against circles;
 * negative = overlap; +inf without a raw scene).  Additional refusals: RDA_ERR_ARG for resort = 0 with a member staged with order != 0; RDA_ERR_UNSUPPORTED
 * for moving slots staged by the host (rda_upload_obstacles per_t: nothing to move) and, with a clearance log, for a norm2 (circle) robot.  A refused call
 * queues nothing and leaves the resident geometry untouched.  rda_fleet_rollout_last serves this entry too. */
int  rda_fleet_rollout_moving(rda_fleet *f, int K, const double *states /*B*3*/, const double *ref_speed /*B*/,
                              const int32_t *cur_index /*B*/, double threshold, int ind_range, int goal_margin, int resort,
                              const double *nom_u /*B*2*T or NULL = resident*/,
                              double *states_log /*(K+1)*B*3*/, double *u_log /*K*B*2*/, int32_t *index_log /*K*B*/,
                              rda_info *info_log /*K*B, may be NULL*/, int32_t *arrived_at /*B, -1 = not arrived*/,
                              double *clearance_log /*K*B, or NULL*/);
/* The two rollouts above for members whose paths have GEAR PIECES (reverse parking, the reference's example/reverse with enable_reverse=True): what MPC._piece,
 * MPC._end (mpc.py:166-187) and the upload of the piece that comes into force do between two ticks, done by the gear form of the advance kernel.  moving = 0:
 * rda_fleet_rollout's arguments, logs and refusals (clearance_log must be NULL); moving != 0: rda_fleet_rollout_moving's.  Differences: every member's pieces
 * are those of rda_upload_path_pieces (its rda_upload_path path is neither needed nor read, and a host-driven tick afterwards still uses it); ref_speed [B] is
 * UNSIGNED - the tracker's speed on piece p is the single product gear[p] * ref_speed; piece0 [B] is the piece in force at tick 0 and cur_index [B] an index
 * within it.  Rule of the tick that ends with min_index in piece p of length Lp: with min_index >= Lp - goal_margin and p + 1 < P the member has NOT arrived -
 * the tick's first control is applied as usual, piece p + 1 is in force from the next tick on with cur_index = 0 and its signed speed, and the nominal
 * controls are kept; with p + 1 == P it arrives as in rda_fleet_rollout and stays on its last piece; otherwise nothing changes.  piece_log [K][B]: the piece
 * in force during tick k; index_log is the index within that piece.  Given a state, a tick computes bit for bit what rda_upload_path of the piece (on the tick
 * it comes into force) + rda_fleet_scene_resort / rda_fleet_upload_scenes + rda_fleet_step_tracked compute.  Additional refusals (RDA_ERR_ARG): a member
 * without resident pieces, piece0[i] outside [0, P_i), cur_index[i] outside that piece, a missing piece0 / piece_log.  A refused call queues nothing; a
 * refused allocation: RDA_ERR_HIP, fleet and members as they were.  Members as each other's obstacles and lidar rollouts are not served with gear pieces.
 * rda_fleet_rollout_last serves this entry too (end_heading: of the piece of the last tick). */
int  rda_fleet_rollout_gears(rda_fleet *f, int K, const double *states /*B*3*/, const double *ref_speed /*B, unsigned*/,
                             const int32_t *piece0 /*B*/, const int32_t *cur_index /*B*/, double threshold, int ind_range, int goal_margin,
                             int resort, int moving, const double *nom_u /*B*2*T or NULL = resident*/,
                             double *states_log /*(K+1)*B*3*/, double *u_log /*K*B*2*/, int32_t *index_log /*K*B*/,
                             rda_info *info_log /*K*B, may be NULL*/, int32_t *arrived_at /*B, -1 = not arrived*/,
                             int32_t *piece_log /*K*B*/, double *clearance_log /*K*B, or NULL*/);
/* of the last rda_fleet_rollout_gears, what the host needs to continue: every member's piece after its last tick (the last piece for a member that arrived)
 * and the heading the last waypoint of every piece has now (quirk Q12), member-major [sum P_i].  Either may be NULL.  No device work.  RDA_ERR_ARG unless the
 * fleet's last rollout was a gear rollout. */
int  rda_fleet_rollout_last_pieces(rda_fleet *f, int32_t *piece /*B or NULL*/, double *end_headings /*sum P_i or NULL*/);
/* every member's clearance (as in clearance_log above) at states [B][3] against its resident raw scene as it stands: one launch, one wait.
 * The figure (scenarios.clearance is the specification; a member without a scene: +inf) is the smallest over the member's obstacles of
 *   polygon  overlapping: minus the penetration depth (the smallest overlap over the outward edge normals of footprint and obstacle); apart: the distance
 *            where a vertex faces an edge, and where two vertices face each other the separating-axis gap - positive, never above the distance
 *   circle   the distance of the centre to the footprint's boundary, negative when the centre lies in the footprint, minus the radius
 * Convex polygons of either winding (obstacles, and the footprint: the rows of G in either order), read off the sign of the shoelace sum; a repeated
 * vertex is allowed (zero-length edges are skipped).  Not defined: non-convex polygons, polygons with a zero shoelace sum.
 * RDA_ERR_UNSUPPORTED: a norm2 robot; RDA_ERR_ARG: a member inside rda_tracked_begin. */
int  rda_fleet_clearance(rda_fleet *f, const double *states /*B*3*/, double *clearance /*B*/);
/* Members that avoid each other: every other member is an ordinary moving polygon obstacle of member i's raw scene, staged on the device
 * (scene::k_peers_fleet; scenarios.peer_obstacles of the Python package is the specification).  rda_fleet_upload_scenes with a larger scene: member i's
 * resident raw scene becomes its counts[i] own obstacles followed by B - 1 PEER ROWS, row counts[i] + (j < i ? j : j - 1) for member j: kind 0, nvert R, the
 * vertices of j's footprint at states[j] - Rot(theta_j) rv_j + p_j, rv_j the body-frame intersections of consecutive rows of j's G x <= h - and the velocity
 * (v cos a, v sin a), (v, w) = controls[j] the control j applied on the previous tick (zeros before its first tick and once it has arrived), a = theta_j for
 * Ackermann and differential robots, a = w for omni (the rule of the rollout's kinematic step); products rounded separately.  The conversion kernels are
 * those of every other scene: peers compete with the own obstacles for the N slots by distance (ranked about states[i], order = 1) and are predicted stage
 * by stage at constant velocity.  The slots are always built for nt = T + 1 stages, because the host does not see the velocities the device writes.  Every
 * member's scene set is grown before any is committed; the fleet remembers counts.  Runs on the fleet's stream behind whatever the members have queued and
 * returns when the staging is done.  B = 1: no peer rows (counts[0] = 0: as rda_upload_scene with n = 0).
 * RDA_ERR_UNSUPPORTED: a norm2 (circle) robot, a robot whose consecutive rows do not intersect, R > E (a footprint does not fit a polygon row), a member with
 * rda_opts::duals_follow, a circle obstacle with E < 3.  RDA_ERR_ARG: a missing array, a negative count, nvert outside 0..E, a member inside
 * rda_tracked_begin.  A refused allocation: RDA_ERR_HIP, fleet and members as they were. */
int  rda_fleet_upload_scenes_peers(rda_fleet *f, const int32_t *counts /*B*/, const int32_t *kind, const int32_t *nvert, const double *geom,
                                   const double *vel, const double *states /*B*3*/, const double *controls /*B*2*/);
/* rda_fleet_scene_resort for such scenes: the peer rows rewritten from states and controls, then the four re-sort launches about states; no waiting, the
 * next fleet step runs behind it.  RDA_ERR_ARG unless every member's resident raw scene is the one the last rda_fleet_upload_scenes_peers of this fleet staged
 * (any other staging of a member since ends that).  Plain rda_fleet_scene_resort (and rda_fleet_rollout / _moving) on such scenes stays legal: it treats
 * the peer rows as the obstacles they are and leaves them where the last refresh put them (rda_fleet_rollout_moving moves and counts them like any row). */
int  rda_fleet_scene_resort_peers(rda_fleet *f, const double *states /*B*3*/, const double *controls /*B*2*/);
/* The rollout of such a fleet: rda_fleet_rollout_moving's arguments, logs, arrival rule and refusals without `resort` (every tick re-sorts), plus controls0
 * [B][2], the controls applied on the tick before this call (zeros at the start of a run; row K - 1 of the previous rollout's u_log to continue one).  Per
 * tick k, on the fleet's stream: (1) the peer rows from the states at the start of the tick and the controls applied one tick earlier - tick 0: states and
 * controls0, later: the device logs' states row k and controls row k - 1; (2) the re-sort launches; (3) the tick of rda_fleet_rollout_moving on the OWN rows:
 * peer rows are neither moved nor snapshotted, and clearance_log stays the clearance against the member's own obstacles; (4) peer_clearance_log [K][B] (may
 * be NULL): member i's separation from the nearest other member at state k+1 (scenarios.peer_clearance: separating axes of the two footprints, negative =
 * overlap; +inf for B = 1).  Still one host wait.  Given the states, the previous controls and the own geometry of tick k, a tick computes bit for bit what
 * rda_fleet_upload_scenes_peers + rda_fleet_step_tracked compute.  After the call the own geometry stands where tick K finds it; the PEER ROWS ARE THOSE OF
 * TICK K - 1: refresh them (rda_fleet_scene_resort_peers, or the next rollout, which does) before a host-driven tick.  Additional refusal: RDA_ERR_ARG
 * without controls0 or unless the scenes are those of rda_fleet_upload_scenes_peers.  rda_fleet_rollout_last serves this entry too. */
int  rda_fleet_rollout_peers(rda_fleet *f, int K, const double *states /*B*3*/, const double *ref_speed /*B*/,
                             const int32_t *cur_index /*B*/, double threshold, int ind_range, int goal_margin,
                             const double *nom_u /*B*2*T or NULL = resident*/, const double *controls0 /*B*2*/,
                             double *states_log /*(K+1)*B*3*/, double *u_log /*K*B*2*/, int32_t *index_log /*K*B*/,
                             rda_info *info_log /*K*B, may be NULL*/, int32_t *arrived_at /*B, -1 = not arrived*/,
                             double *clearance_log /*K*B, or NULL*/, double *peer_clearance_log /*K*B, or NULL*/);
/* The second peers mode: peers predicted ALONG THEIR PLANNED TRAJECTORIES instead of at constant velocity (scene::k_build_plan_fleet in k_build_fleet's place
 * in the re-sort launch set, so the launches per tick are those of the entries above; scenarios.peer_plan_poses / peer_plan_obstacles are the specification).
 * plans [B][3][T+1]: every member's planned states, the out_s of its last solve; plan_valid [B]: 0 = member j has no plan that counts - no solve yet, after
 * rda_reset, arrived - and is predicted at constant velocity exactly as above.  The peer rows, the ranking by current distance, the competition with the own
 * obstacles for the N slots, nt = T + 1 and the padding (quirk Q3) are unchanged.  What changes is stages 1 .. T of a slot whose source row is the peer row of a
 * valid member j: stage t is the half-space form (the edge expressions, orientation test and zeroed spare rows of every polygon) of j's footprint
 * Rot(pose_t.theta) rv_j + pose_t.xy with
 *     pose_t = x_j + (q_t - P[:,1]),   q_t = P[:,t+1] for t < T,   q_T = P[:,T] + (P[:,T] - P[:,T-1])            (x, y and heading alike)
 * x_j = states[j], P = plans[j]: the plan is a sequence of displacements ANCHORED at the peer's actual state (a plant that did not follow its plan exactly
 * produces no jump at stage 1), and the LAST STAGE repeats the plan's last increment.  Every difference and sum is rounded separately, parenthesised as
 * written.  Stage 0, own obstacles and the slots of members that are not valid are bit-identical to rda_fleet_upload_scenes_peers; a padded copy of a peer
 * carries the plan too.  The scenes are the peers scenes: the two modes may alternate on the same staged fleet.  Refusals of rda_fleet_upload_scenes_peers,
 * plus RDA_ERR_ARG without plans / plan_valid; a refused allocation: RDA_ERR_HIP, fleet and members as they were.  Not covered: staging combined with lidar
 * (members that see each other through the simulated lidar: rda_fleet_rollout_lidar_peers), circle (norm2) robots, the gear pieces of enable_reverse paths. */
int  rda_fleet_upload_scenes_peers_plan(rda_fleet *f, const int32_t *counts /*B*/, const int32_t *kind, const int32_t *nvert, const double *geom,
                                        const double *vel, const double *states /*B*3*/, const double *controls /*B*2*/,
                                        const double *plans /*B*3*(T+1)*/, const int32_t *plan_valid /*B*/);
/* rda_fleet_scene_resort_peers in this mode: the peer rows rewritten, then the re-sort launches with the plans; no waiting.  Its refusals, plus RDA_ERR_ARG
 * without plans / plan_valid. */
int  rda_fleet_scene_resort_peers_plan(rda_fleet *f, const double *states /*B*3*/, const double *controls /*B*2*/,
                                       const double *plans /*B*3*(T+1)*/, const int32_t *plan_valid /*B*/);
/* rda_fleet_rollout_peers in this mode (its arguments, logs and refusals; plans0 / plan_valid0 behind them, RDA_ERR_ARG when either is missing).  Per tick k
 * the peer rows are written as there; the slots are built from the states at the start of tick k and the plans the members' solves of tick k - 1 left in
 * the fleet's result block on the device - tick 0: plans0 / plan_valid0 - and from tick 1 on a member is valid while it has not arrived (arrival tick <=
 * k - 1: predicted standing).  Still one host wait.  Given the states, the previous controls, the previous tick's out_s and the own geometry of tick k, a
 * tick computes bit for bit what rda_fleet_upload_scenes_peers_plan + rda_fleet_step_tracked compute.  rda_fleet_rollout_last serves this entry too, and
 * rda_fleet_rollout_last_plan gives the plans0 that continue it. */
int  rda_fleet_rollout_peers_plan(rda_fleet *f, int K, const double *states /*B*3*/, const double *ref_speed /*B*/,
                                  const int32_t *cur_index /*B*/, double threshold, int ind_range, int goal_margin,
                                  const double *nom_u /*B*2*T or NULL = resident*/, const double *controls0 /*B*2*/,
                                  double *states_log /*(K+1)*B*3*/, double *u_log /*K*B*2*/, int32_t *index_log /*K*B*/,
                                  rda_info *info_log /*K*B, may be NULL*/, int32_t *arrived_at /*B, -1 = not arrived*/,
                                  double *clearance_log /*K*B, or NULL*/, double *peer_clearance_log /*K*B, or NULL*/,
                                  const double *plans0 /*B*3*(T+1)*/, const int32_t *plan_valid0 /*B*/);
/* of the last tick of the last rollout (any rollout entry): every member's planned states out_s [3][T+1], what rda_fleet_step_tracked returns as out_s - the
 * plans0 of a rda_fleet_rollout_peers_plan, or the plans of a host-driven plan tick, that continues it.  No device work.  RDA_ERR_ARG before the first
 * rollout or without out_s. */
int  rda_fleet_rollout_last_plan(rda_fleet *f, double *out_s /*B*3*(T+1)*/);
/* every member's separation from the nearest other member (as in peer_clearance_log above) at states [B][3]: one launch, one wait; needs no staged scene.
 * The polygon figure of rda_fleet_clearance between two footprints, each of either winding.
 * RDA_ERR_UNSUPPORTED: a robot the clearance does not take (see rda_fleet_clearance); RDA_ERR_ARG: a member inside rda_tracked_begin. */
int  rda_fleet_peer_clearance(rda_fleet *f, const double *states /*B*3*/, double *out /*B*/);
/* A resident WORLD per member: the true obstacles a simulated lidar sees (rda_fleet_raycast, rda_fleet_rollout_lidar), kept apart from the member's raw
 * scene, which a lidar tick overwrites with boxes.  The layout of rda_fleet_upload_scenes with a vertex stride of its own: member i owns counts[i]
 * consecutive entries (0 = an empty world), kind 0 polygon / 1 circle, geom[j] = `we` vertex pairs | centre, (radius, -), 3 <= we <= RDA_EMAX; vel NULL =
 * a world that stands.  Owned by the fleet; a new upload replaces the old world.  RDA_ERR_ARG: a negative count, a missing array with a positive total,
 * nvert outside 3..we for a polygon, a kind other than 0 / 1, we out of range; a refused allocation: RDA_ERR_HIP, the old world intact. */
int  rda_fleet_upload_worlds(rda_fleet *f, const int32_t *counts /*B*/, int we, const int32_t *kind, const int32_t *nvert,
                             const double *geom /*sum(counts)*we*2*/, const double *vel /*sum(counts)*2, or NULL = standing*/);
/* The simulated sensor (World.get_lidar_scan of rda_planner_amd/world.py is the specification): every member's beams ray-cast against its resident world as
 * it stands, from states [B][3], by ONE launch of lidar::k_raycast_fleet (the member in the grid, a thread per beam) and one wait.  Beam i of a member:
 * angle_min + i * (angle_max - angle_min) / (n_beams - 1), the last one exactly angle_max, a single beam angle_min; direction (cos, sin) of heading +
 * angle.  Circle: f = o - c, b = d.f, disc = b*b - (f.f - r*r), a hit needs disc >= 0 and t = -b - sqrt(disc) >= 0 (an origin inside a circle does not see
 * it).  Polygon edge p -> q: e = q - p, w = p - o, u = q - o, den = d.x e.y - d.y e.x, t = (w.x e.y - w.y e.x) / den, the vertices' sides of the beam's line
 * side_p = w.x d.y - w.y d.x and side_q = u.x d.y - u.y d.x; a hit needs (side_p >= 0) != (side_q >= 0), den^2 > 1e-20 e.e (|d| = 1), t >= 0.  A vertex's
 * side depends on that vertex alone, so the edges that meet in it agree on it: a closed polygon has no gap at a vertex, at a repeated one, or between two
 * 1e-13 m apart.  Only an edge that lies along the beam's line to within 1e-10 rad is skipped: there sides, den and t are rounding noise, and a beam that
 * meets an edge that flat is a silhouette beam anyway (checked against exact rational ray casting, tests/ray_exact.py).  range = clip(min(range_max, all
 * hits), range_min, range_max); an empty world: range_max everywhere.  `ranges` is
 * the concatenation of the members' scans (n_beams[i] = 0: no scan).  RDA_ERR_UNSUPPORTED: more than 4096 beams; RDA_ERR_ARG: no uploaded world, a negative
 * beam count, a missing array. */
int  rda_fleet_raycast(rda_fleet *f, const int32_t *n_beams /*B*/, const double *angle_min, const double *angle_max,
                       const double *range_min, const double *range_max /*B each*/, const double *states /*B*3*/,
                       double *ranges /*sum(n_beams)*/);
/* The rollout of a fleet whose robots each carry a lidar: the loop a caller otherwise runs as World.get_lidar_scan -> rda_fleet_upload_scans ->
 * rda_fleet_step_tracked -> the plant.  rda_fleet_rollout's arguments, logs, arrival rule and refusals without `resort` (a lidar tick always stages about the
 * robot), the sensor arrays of rda_fleet_raycast, and eps, min_samples, order [B] of rda_fleet_upload_scans.  Per tick k, on the fleet's stream: the ray
 * cast from the pose the advance kernel left on the device (tick 0: the caller's) into a device ranges buffer, the scan kernel on those ranges at that
 * pose, ONE wait for the B box counts (4 * B bytes: they choose the LamMuZ launch form, apply the zero-box rule and size the staging launches), the staging
 * of rda_fleet_upload_scans with the robot position taken from the device, the tracker, the ADMM launches and the advance kernel.  moving != 0: behind
 * every tick the WORLD is put forward by the rule of rda_fleet_rollout_moving - `base` = the world as the call finds it, at tick k base + vel * (dt * k) -
 * and after the call it stands where tick K would find it.  nbox_log [K][B] (may be NULL): the boxes every member saw; clearance_log [K][B] (may be NULL):
 * state k+1 against the WORLD of tick k+1 (the true obstacles, not the boxes; +inf for an empty world; a norm2 robot: RDA_ERR_UNSUPPORTED).  Every
 * member's raw scene is grown to n_beams[i] boxes and every buffer allocated before tick 0; a refused call queues nothing and leaves world and members as
 * they were.  Given a state and the world of tick k, a tick computes bit for bit what rda_fleet_raycast, rda_fleet_upload_scans of those ranges at that
 * state and rda_fleet_step_tracked compute; afterwards fleet and members are as K such host-driven ticks leave them.  Additional refusals: RDA_ERR_ARG
 * without an uploaded world, for a negative beam count, eps <= 0, min_samples < 1 or a missing array; RDA_ERR_UNSUPPORTED for more than 4096 beams or
 * E < 4.  rda_fleet_rollout_last serves this entry too. */
int  rda_fleet_rollout_lidar(rda_fleet *f, int K, const double *states /*B*3*/, const double *ref_speed /*B*/,
                             const int32_t *cur_index /*B*/, double threshold, int ind_range, int goal_margin,
                             const double *nom_u /*B*2*T or NULL = resident*/,
                             const int32_t *n_beams /*B*/, const double *angle_min, const double *angle_max,
                             const double *range_min, const double *range_max /*B each*/,
                             double eps, int min_samples, const int32_t *order /*B*/, int moving,
                             double *states_log /*(K+1)*B*3*/, double *u_log /*K*B*2*/, int32_t *index_log /*K*B*/,
                             rda_info *info_log /*K*B, may be NULL*/, int32_t *arrived_at /*B, -1 = not arrived*/,
                             int32_t *nbox_log /*K*B, may be NULL*/, double *clearance_log /*K*B, may be NULL*/);
/* The simulated sensor of a fleet whose members SEE EACH OTHER: rda_fleet_raycast's arguments, one launch (lidar::k_raycast_fleet_peers) and one wait.
 * Member i's beams are cast against its resident world and against the footprints of all members j != i at states[j] - polygons of R vertices,
 * Rot(theta_j) rv_j + p_j with the expressions of rda_fleet_upload_scenes_peers' peer rows (scenarios.peer_footprints is the specification: the scan is
 * World.get_lidar_scan on world_i + peer_footprints(cars, states, i)).  A member never sees itself; a footprint that contains the beam origin is hit from
 * the inside like any polygon; range = clip(min(range_max, world hits, peer hits), range_min, range_max).  This is perception, not staging: nothing of
 * the members' scenes is read or written, and the peers modes (rda_fleet_*_peers) stay separate.  rda_fleet_raycast's refusals - a world must be
 * resident; count 0 per member (an empty world) is the way to see only the others - plus RDA_ERR_UNSUPPORTED for a robot the clearance does not take (a
 * norm2 robot, consecutive rows that do not intersect: see rda_fleet_clearance).  B = 1: rda_fleet_raycast. */
int  rda_fleet_raycast_peers(rda_fleet *f, const int32_t *n_beams /*B*/, const double *angle_min, const double *angle_max,
                             const double *range_min, const double *range_max /*B each*/, const double *states /*B*3*/,
                             double *ranges /*sum(n_beams)*/);
/* rda_fleet_rollout_lidar for such a fleet: its arguments, logs, arrival rule and refusals, plus peer_clearance_log.  Per tick the launches of
 * rda_fleet_rollout_lidar with the ray cast replaced by lidar::k_raycast_fleet_peers on the poses the advance kernel left for ALL members (tick 0: the
 * caller's) - no extra launch; with peer_clearance_log [K][B] one launch more, member i's separation from the nearest other member at state k+1 (as in
 * rda_fleet_rollout_peers; +inf for B = 1).  Still one short wait per tick for the 4 * B bytes of box counts, nothing else crosses the link.  Members
 * that have arrived stand where they are and are still seen.  A seen member reaches the planner as standing boxes like every lidar obstacle (no
 * velocity from perception).  `moving`, nbox_log, clearance_log (against the WORLD, the true obstacles) and rda_fleet_rollout_last keep their meaning; a
 * refused call queues nothing and leaves world and members as they were; every buffer is allocated before tick 0.  Given the states of tick k and the
 * world of tick k, a tick computes bit for bit what a host-driven tick computes: rda_fleet_raycast_peers, then rda_fleet_upload_scans of those ranges at
 * those states, then rda_fleet_step_tracked.  Additional refusal: RDA_ERR_UNSUPPORTED for a robot the clearance does not take. */
int  rda_fleet_rollout_lidar_peers(rda_fleet *f, int K, const double *states /*B*3*/, const double *ref_speed /*B*/,
                                   const int32_t *cur_index /*B*/, double threshold, int ind_range, int goal_margin,
                                   const double *nom_u /*B*2*T or NULL = resident*/,
                                   const int32_t *n_beams /*B*/, const double *angle_min, const double *angle_max,
                                   const double *range_min, const double *range_max /*B each*/,
                                   double eps, int min_samples, const int32_t *order /*B*/, int moving,
                                   double *states_log /*(K+1)*B*3*/, double *u_log /*K*B*2*/, int32_t *index_log /*K*B*/,
                                   rda_info *info_log /*K*B, may be NULL*/, int32_t *arrived_at /*B, -1 = not arrived*/,
                                   int32_t *nbox_log /*K*B, may be NULL*/, double *clearance_log /*K*B, may be NULL*/,
                                   double *peer_clearance_log /*K*B, may be NULL*/);
/* Tracked fleet lidar: the boxes of successive scans associated from tick to tick on the device, so that a lidar obstacle reaches the planner with a
 * velocity and per-stage prediction like every other obstacle.  lidar::k_track_boxes_fleet (csrc/lidar_device.h; one workgroup per member, one launch
 * whatever B is) keeps a resident table of tracks per member - at most 256, each the history of its box centres, at most 8 ticks - and computes
 * lidar.track_boxes (rda_planner_amd/lidar.py, the specification) bit for bit: centre = (((x0 + x1) + x2) + x3) * 0.25; only the first 256 boxes of a
 * scan take part; box i continues previous track j iff they are each other's nearest (lowest index among equals) and their squared distance is at most
 * gate * gate; a continued track of history h gives v = (c - h[0]) / (dt * len(h)), dt the member's rda_cfg::dt, and keeps (h + [c])[-window:]; every other
 * box gets v = 0 and starts a track; tracks nobody continues end; a scan without boxes empties the table.  Successive tracked calls are taken to be dt
 * apart (a caller that skips ticks calls rda_fleet_reset_tracks); gate / dt is also the largest speed a new track can show.  gate > 0 and 1 <= window <= 8,
 * else RDA_ERR_ARG.  A refused call or a refused allocation leaves tracks, fleet and members as they were.
 * rda_fleet_upload_scans with the tracker queued directly behind the scan kernel, in front of the one wait for the B box counts (one launch more, no
 * wait more), and the boxes staged with these velocities: every member with boxes gets slots for T + 1 stages, built by the unchanged conversion kernels
 * (a box under 0.01 m/s is not predicted, mpc.py:443).  The host does not see the velocities.  Bit for bit rda_fleet_upload_scenes of the same boxes as
 * 4-vertex polygons with lidar.track_boxes' velocities, where that call builds T + 1 stages too. */
int  rda_fleet_upload_scans_tracked(rda_fleet *f, const int32_t *n_beams, const double *ranges, const double *angle_min,
                                    const double *angle_max, const double *range_max, const double *states /*B*3*/,
                                    double eps, int min_samples, const int32_t *order /*B*/, int32_t *n_boxes /*B or NULL*/,
                                    double gate, int window);
/* rda_fleet_rollout_lidar (see = 0) or rda_fleet_rollout_lidar_peers (see != 0: a seen member is tracked like any box; peer_clearance_log is read only
 * then) with the tracker behind every tick's scan kernel and the tracked staging: their arguments, logs and refusals.  Given the states and the world of
 * tick k and the tracks of tick k - 1, a tick computes bit for bit what rda_fleet_raycast(_peers), rda_fleet_upload_scans_tracked of those ranges at those
 * states and rda_fleet_step_tracked compute.  The tracks continue those the fleet holds when the call starts. */
int  rda_fleet_rollout_lidar_tracked(rda_fleet *f, int K, const double *states /*B*3*/, const double *ref_speed /*B*/,
                                     const int32_t *cur_index /*B*/, double threshold, int ind_range, int goal_margin,
                                     const double *nom_u /*B*2*T or NULL = resident*/,
                                     const int32_t *n_beams /*B*/, const double *angle_min, const double *angle_max,
                                     const double *range_min, const double *range_max /*B each*/,
                                     double eps, int min_samples, const int32_t *order /*B*/, int moving,
                                     double *states_log /*(K+1)*B*3*/, double *u_log /*K*B*2*/, int32_t *index_log /*K*B*/,
                                     rda_info *info_log /*K*B, may be NULL*/, int32_t *arrived_at /*B, -1 = not arrived*/,
                                     int32_t *nbox_log /*K*B, may be NULL*/, double *clearance_log /*K*B, may be NULL*/,
                                     double *peer_clearance_log /*K*B, may be NULL*/, int see, double gate, int window);
/* the tracker alone, on boxes the caller supplies: n [B] boxes per member (0 .. min(cap, 4096); more than cap or negative: RDA_ERR_ARG), boxes
 * [B][cap][4][2]; vel_out [B][cap][2] (may be NULL) gets the first n[i] velocities of member i.  The table advances by one tick, nothing is staged; the
 * boxes take the place of the last scan's in the fleet's lidar block. */
int  rda_fleet_track_boxes(rda_fleet *f, const int32_t *n /*B*/, const double *boxes /*B*cap*4*2*/, int cap, double gate, int window,
                           double *vel_out /*B*cap*2 or NULL*/);
/* the table as the last tracked call left it: n [B] tracks per member (track k belongs to box k of that call; n may exceed cap: the first cap are
 * written), centres [B][cap][2] their positions, vel [B][cap][2] the velocities their boxes got, age [B][cap] the entries of their histories (1 .. 8);
 * each of the three may be NULL.  Before the first tracked call: no tracks. */
int  rda_fleet_box_tracks(rda_fleet *f, int cap, int32_t *n /*B*/, double *centres, double *vel, int32_t *age);
/* the members which [count] (NULL: every member) lose their tracks: the boxes of their next tracked tick start new ones.  An index outside the fleet:
 * RDA_ERR_ARG.  Runs on the fleet's stream. */
int  rda_fleet_reset_tracks(rda_fleet *f, const int32_t *which /*count, or NULL = all*/, int count);
/* Split stage of the lidar front end: with tol > 0 [m] every DBSCAN cluster of a scan is cut into its straight runs and every run gets its own
 * minimum-area rectangle - for scenes with walls, where the hits on an L-shaped wall, on both sides of a corridor or on the inside of a room form ONE
 * cluster whose rectangle covers the free space the robot stands in.  lidar.split_runs (rda_planner_amd/lidar.py) is the specification and
 * lidar::split_stage (csrc/lidar_device.h) takes every decision on the same numbers: within a cluster, in beam order, a run ends where two neighbours are
 * farther apart than eps (the clustering's own test); a run [a, b] of 3 or more points splits at the point farthest from the chord a-b (the lowest index
 * among equals) if that distance exceeds tol - compared as squares times the chord's squared length, no root, no division - into [a, m - 1] and [m, b],
 * until nothing splits.  Segments are numbered by cluster, then by first point; box counts, per-beam labels and the box order are then those of the
 * segments, everything behind the scan kernel (staging, tracking, rollouts) only ever sees boxes.  tol = 0 switches the stage off and is the default:
 * every call then queues and computes exactly what it did without it.  The value stays until it is set again.  A negative or non-finite tol returns
 * RDA_ERR_ARG and changes nothing.  tol has to exceed the sensor's range noise.
 * The handle's value governs rda_scan_boxes and rda_upload_scan.  The fleet's value governs every member's scan in rda_fleet_scan_boxes,
 * rda_fleet_upload_scans, rda_fleet_upload_scans_tracked, rda_fleet_rollout_lidar, rda_fleet_rollout_lidar_peers and rda_fleet_rollout_lidar_tracked;
 * the members' own values are ignored by fleet calls. */
int  rda_set_scan_split(rda_handle *h, double tol);
int  rda_fleet_set_scan_split(rda_fleet *f, double tol);
/* test hook: the geometry of the resident worlds as it stands, member-major [*n_total][*we][2] (geom and we may be NULL; *n_total = 0: no world) */
int  rda_debug_fleet_world(rda_fleet *f, double *geom, int32_t *n_total, int32_t *we);
/* steps k0 .. k1-1 of every member's uploaded trace, asynchronous; read with rda_fetch_result after rda_fleet_sync */
int  rda_fleet_enqueue_range(rda_fleet *f, int k0, int k1);
int  rda_fleet_sync(rda_fleet *f);

/* State in the reference's shapes: lam [N][T+1][E], mu [N][T+1][R], z [N][T], xi [N][T+1][2],
 * zeta [N][T], dis [T], a_lam [N][T+1][2] (para_obsA_lam), b_lam [N][T+1] (para_obsb_lam).
 * NULL pointers are skipped. */
int  rda_get_state(rda_handle *h, double *lam, double *mu, double *z, double *xi, double *zeta,
                   double *dis, double *a_lam, double *b_lam);
int  rda_set_state(rda_handle *h, const double *lam, const double *mu, const double *z,
                   const double *xi, const double *zeta, const double *dis,
                   const double *a_lam, const double *b_lam);
/* Solver history of a handle: not reference-visible state, but it picks the START of the next su interior-point solve (easy /
 * moderate / cold), so two handles return bit-identical controls only if it agrees too.  hist[0] = interior-point
 * iterations of the last su-solve (99 = none), hist[1] = consecutive solves in the hard regime, hist[2] = the previous step ended above
 * iter_threshold, hist[3] = the last su-solve started far from its solution (the two keys of su_hard_warm); lam_keep [10*T] = the inequality
 * multipliers of the last converged su-solve.  rda_create and rda_reset set (99, 0, zeros).  NULL pointers are skipped. */
#define RDA_SU_HISTORY_INTS 8   /* entries of `hist` in THIS header (round 4: 2, round 5: 4 - the array grows with the start rules, an ABI break for callers of the count-less
                                   forms: use the _n forms below).  hist[4] (round 6) = the credit of the speculative landings, rda_opts::su_land_first = 2; hist[5] > 0: one of the last four landings took three or more
                                   rounds (the next solve's interior point runs to 1e-2 x su_land_tol before it is landed); hist[6] = su-solves in a row without an interior-point iteration and with
                                   one landing round, hist[7] = the gate of the blind landings (rda_opts::su_land_blind_from) */
int  rda_get_su_history(rda_handle *h, int32_t *hist /*RDA_SU_HISTORY_INTS*/, double *lam_keep /*10*T*/);
int  rda_set_su_history(rda_handle *h, const int32_t *hist /*RDA_SU_HISTORY_INTS*/, const double *lam_keep /*10*T*/);
/* ... with the caller's own count: get writes n_hist entries (those this library does not have read 0), set reads
 * min(n_hist, RDA_SU_HISTORY_INTS) and leaves the others as they are - a caller compiled against an older or newer header stays correct */
int  rda_get_su_history_n(rda_handle *h, int32_t *hist, int n_hist, double *lam_keep /*10*T*/);
int  rda_set_su_history_n(rda_handle *h, const int32_t *hist, int n_hist, const double *lam_keep /*10*T*/);
/* Interior-point LamMuZ mode: the central-path points the sub-problems last ended on ([T][N][5][16] doubles: x | s, z of the diagonal
 * rows | s, z of the general rows, csrc/lammuz_ip_device.h) and their validity flags [T][N] - where each sub-problem's next solve starts.
 * Solver history like the su history above: it moves a result only within the centring tolerance (1e-7 mu relative), rda_reset clears
 * it.  rda_lmz_history_doubles = 80 N T, or 0 when the handle keeps none (enumeration mode, per-thread kernel, lmz_ip_warm = 0). */
int  rda_lmz_history_doubles(rda_handle *h);
int  rda_get_lmz_history(rda_handle *h, double *points, int32_t *valid);
int  rda_set_lmz_history(rda_handle *h, const double *points, const int32_t *valid);
/* debug: accumulated clock64 phase counters of the su-solves of this handle since the last call (rda_opts::su_prof), 16 values */
int  rda_debug_su_prof(rda_handle *h, long long *out16);
/* -DSU_TRACE builds only (RDA_ERR_UNSUPPORTED otherwise): per-wave (event id, clock64) pairs of the LAST su launch, out[4][cap][2] (tools/su_trace.py) */
int  rda_debug_su_trace(rda_handle *h, long long *out, int cap, int *n_out);
int  rda_debug_su_land(rda_handle *h, int32_t *out4);      /* su_land: landings accepted, refused, rounds, passes spent on landings since the last call */
int  rda_debug_su_land_n(rda_handle *h, int32_t *out, int n);   /* ... the first n <= 20 counters: [4] speculative landings (su_land_first = 2) tried, [5] accepted, [6 + k] / [12 + k] tried / accepted by the decade k = 0 .. 5 of the start's relative dual residual (< 1e-4, < 1e-3, < 1e-2, < 1e-1, < 1, >= 1) */
int  rda_debug_flush_supports(rda_handle *h);             /* forget every remembered LamMuZ support (a cache: results must not depend on it) */
int  rda_debug_slot_src(rda_handle *h, int32_t *src /*N*/, int32_t *used); /* slot -> entry of the caller's raw scene (device pipeline; used = 0: host-staged slots) */
int  rda_debug_worklist(rda_handle *h, int *rows);        /* rows on the LamMuZ work list of the last executed iteration (split launch form) */
/* debug: every call that fails changes nothing and leaks nothing (tests/test_gpu_lifecycle.py).  rda_debug_alloc_fail: in the calling thread, the
 * device or pinned allocation with index n (0 = the next one) among those the library requests from now on is refused as if the HIP allocation
 * had failed (n < 0 disarms); rda_debug_alloc_stats: the device and pinned allocations the library holds now (count, bytes), process-wide */
int  rda_debug_alloc_fail(int n);
int  rda_debug_alloc_stats(long long *live_allocs, long long *live_bytes);

/* Obstacle sharding across the GPUs of one node (one process per GPU).  Rank r owns the obstacle slots
 * [r*ceil(N/world), (r+1)*ceil(N/world)): it solves their LamMuZ problems and keeps their duals.  What the su-problem needs of
 * them forms one contiguous chunk per rank - 3 doubles per (slot, stage): a = A'lam (2) and the hinge offset lam'b + mu'h + z - zeta;
 * plus, per (stage, 8-slot block), the 5 reduced sums (sum |a|^2, sum g.a, sum g x a, the two residual partials) and one 8-byte word
 * with the near mask the su set-up reads instead of passing over the terms - replicated to every rank by ONE all-gather per ADMM
 * iteration (replaces the pool.map scatter/gather of rda_solver.py:706-725); every rank then solves the identical su-problem.  The
 * other per-row records (lam'b, mu'h + z - zeta, G'mu + xi, residual records) stay on the owning rank; for that reason
 *   - rda_opts::su_pre = 0 (the su set-up evaluating raw terms) is overridden to 1 when world > 1, and
 *   - rda_reset / rda_set_state return RDA_ERR_UNSUPPORTED on a handle with world > 1 once it has stepped (the remote slots' terms
 *     cannot be rebuilt locally; reset / restore the state BEFORE the first step, or re-create the handles).
 * rda_shard_config must precede the first step.
 * N need not be divisible by world: the shards have ceil(N / world) slots, the slots past the last obstacle carry terms the
 * su-problem ignores - this relies on the hinge of the accelerated cost: with accelerated = 0 and N % world != 0
 * rda_shard_config returns RDA_ERR_UNSUPPORTED. */
int  rda_shard_config(rda_handle *h, int rank, int world);
int  rda_shard_chunk_doubles(rda_handle *h);                       /* 3*T*Nloc + 6*T*ceil(Nloc/8), Nloc = ceil(N/world) */
int  rda_shard_get_chunk(rda_handle *h, double *host_chunk);       /* this rank's chunk  */
int  rda_shard_set_chunks(rda_handle *h, const double *host_all);  /* all `world` chunks, rank-major */
/* RCCL exchange over xGMI: rank 0 calls rda_shard_unique_id and ships the 128 bytes to the other ranks (any
 * side channel); every rank then calls rda_shard_comm_init.  From then on rda_step / rda_enqueue_step issue
 * one in-place ncclAllGather per ADMM iteration on the handle's stream. */
int  rda_shard_unique_id(rda_handle *h, void *out128);
int  rda_shard_comm_init(rda_handle *h, const void *uid128);
int  rda_shard_comm_count(rda_handle *h);                          /* ncclCommCount of the handle's communicator; 0 without one */
/* Host-driven ADMM iteration for callers that do the exchange themselves (tests, gloo, MPI):
 *   rda_admm_begin; for it: rda_admm_su(it,&stopped); if stopped break; rda_admm_lammuz; <exchange chunks>; rda_admm_finish */
int  rda_admm_begin(rda_handle *h, const double *nom_s, const double *nom_u, const double *ref_s, double ref_speed);
int  rda_admm_su(rda_handle *h, int it, int *stopped);
int  rda_admm_lammuz(rda_handle *h);
int  rda_admm_finish(rda_handle *h, double *out_u, double *out_s, rda_info *info);

/* Pure-function hooks -----------------------------------------------------------------------*/
/* B independent (obstacle, stage) sub-problems in one launch, one per wavefront.
 * A [B][E][2], b [B][E], cone [B], p [B][2] (nominal position, column t+1), phi [B] (nominal heading,
 * column t), xi [B][2], zeta [B], dbar [B]; G [R][2], h [R].  Outputs lam [B][E], mu [B][R], z [B],
 * cmh [B][4] = (cost, m, H0, H1). */
int  rda_lammuz_batch(int B, int E, int R, const double *A, const double *b, const int32_t *cone,
                      const double *p, const double *phi, const double *G, const double *h,
                      const double *xi, const double *zeta, const double *dbar, double ro2, double delta,
                      int accelerated, double *lam, double *mu, double *z, double *cmh);

/* su-problem with condensed obstacle terms a [N][T][2], cc [N][T], g [N][T][2];
 * d0 [T] initial guess; outputs s 3x(T+1), u 2xT, d [T].  Returns 0 ok, 1 not converged.
 * N = 0 (no obstacle terms) is refused here (RDA_ERR_UNSUPPORTED, like rda_create).  The su-problem itself is defined there: d keeps its
 * cost -slack_gain sum(d) and its bounds, so d = max_sd (the oracle's orc_su_solve and tests/su_kkt.py solve it so). */
int  rda_su_solve(const rda_cfg *cfg, const double *nom_s, const double *nom_u, const double *ref_s,
                  double ref_speed, const double *a, const double *cc, const double *g,
                  const double *d0, double *s, double *u, double *d, int32_t *ipm_iters);
/* ... with the caller's rda_opts (NULL = rda_opts_init): su_tol, su_split, su_accept; su_prof = 1 prints the phase cycles, 2 also one line per
 * interior-point iteration, on stderr */
int  rda_su_solve_opts(const rda_cfg *cfg, const rda_opts *opts, const double *nom_s, const double *nom_u, const double *ref_s,
                       double ref_speed, const double *a, const double *cc, const double *g,
                       const double *d0, double *s, double *u, double *d, int32_t *ipm_iters);

#ifdef __cplusplus
}
#endif
#endif
