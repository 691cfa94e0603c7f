// Caller-side obstacle pipeline on the device: what the reference does per MPC tick in Python before
// the solver is entered -
//   MPC.convert_rda_obstacle / rda_obs_distance / sort          mpc.py:189-218
//   convert_inequal_circle / convert_inequal_polygon            mpc.py:440-472
//   gen_inequal_global, is_convex_and_ordered, cross_product    mpc.py:492-549
//   RDA_solver.assign_obstacle_parameter (truncate / pad / zero rows, per-t replication)   rda_solver.py:483-526
// - as three small kernels that write the solver's obstacle slots A [N][nt][E][2], b [N][nt][E], cone [N] directly.
// The arithmetic reproduces the numpy expressions operation by operation (FMA contraction is switched off in these
// kernels), so the slots are BIT-IDENTICAL to what the Python caller stages (tests/test_gpu_scene.py).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/rda_hip.h"

namespace scene {

struct Args {
    int n, N, E, T, nt, order;
    double dt;
    const int *kind;        // [n] 0 polygon (Rpositive), 1 circle (norm2)
    const int *nvert;       // [n] polygon vertex count (<= E)
    const double *geom;     // [n][E][2]: polygon vertices | circle: centre, (radius, -)
    const double *vel;      // [n][2]
    const double *robot;    // [2] robot position used for the distance ordering
    double rx, ry; int robot_val;   // robot_val != 0: the position travels in the kernel arguments (rda_scene_resort: a resident scene re-ranked without a copy)
    double *key; int *sel;  // [n] scratch
    double *A, *b; int *cone;
    int *nonconvex;         // count of polygons failing is_convex_and_ordered (the reference prints a warning)
};

// distance key of one obstacle: rda_obs_distance, mpc.py:214-218 (circle: centre distance; polygon: nearest vertex)
__device__ __forceinline__ void keys_body(const Args &a, const int i)
{
#pragma clang fp contract(off)        // numpy does not fuse: keep every product and sum separately rounded
    if (i >= a.n) return;
    if (!a.order) { a.key[i] = (double)i; return; }
    const double x = a.robot_val ? a.rx : a.robot[0], y = a.robot_val ? a.ry : a.robot[1];
    const double *g = a.geom + (size_t)i * a.E * 2;
    if (a.kind[i] == 1) {
        double dx = x - g[0], dy = y - g[1];
        a.key[i] = sqrt(dx * dx + dy * dy);
    } else {
        double best = INFINITY;
        for (int j = 0; j < a.nvert[i]; ++j) {
            double dx = x - g[2 * j], dy = y - g[2 * j + 1];
            double d = sqrt(dx * dx + dy * dy);
            if (d < best) best = d;
        }
        a.key[i] = best;
    }
}
__global__ void k_keys(Args a) { keys_body(a, blockIdx.x * blockDim.x + threadIdx.x); }

// stable rank by key (Python's list.sort is stable); the first min(n, N) survive (rda_solver.py:491-493)
// O(n^2) compares spread over 16 lanes per key (256-thread blocks = 16 keys; launch with (n + 15) / 16 blocks): a count, so the
// result does not depend on how the compares are split
__device__ __forceinline__ void rank_body(const Args &a, const int blk)
{
    const int i = blk * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
    const bool live = i < a.n;
    const double ki = live ? a.key[i] : 0.0;
    int r = 0;
    if (live) for (int j = l; j < a.n; j += 16) { double kj = a.key[j]; r += (kj < ki) || (kj == ki && j < i); }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) r += __shfl_xor(r, off, 16);
    if (live && l == 0 && r < a.N) a.sel[r] = i;
}
__global__ void k_rank(Args a) { rank_body(a, blockIdx.x); }

// The slot rows of one polygon at one stage, shared by build_body and plan_body: all E rows zeroed (the spare rows stay zero) ...
__device__ __forceinline__ void zero_rows(double *A, double *b, const int E)
{
    for (int e = 0; e < E; ++e) { A[2 * e] = 0; A[2 * e + 1] = 0; b[e] = 0; }
}
// ... and rows 0 .. k-1 from the k vertices (px, py): the orientation test and the edge expressions of gen_inequal_global; returns is_convex_and_ordered
__device__ __forceinline__ bool polygon_rows(const double *px, const double *py, const int k, double *A, double *b)
{
#pragma clang fp contract(off)
    // is_convex_and_ordered, mpc.py:527-549
    int direction = 0; bool convex = k >= 3;
    for (int j = 0; j < k && convex; ++j) {
        int j1 = (j + 1) % k, j2 = (j + 2) % k;
        double cr = (px[j1] - px[j]) * (py[j2] - py[j]) - (py[j1] - py[j]) * (px[j2] - px[j]);
        if (cr != 0) {
            if (direction == 0) direction = cr > 0 ? 1 : -1;
            else if ((cr > 0) != (direction > 0)) convex = false;
        }
    }
    const bool cw = convex && direction <= 0;                      // order == 'CW' (direction 0 also reports CW), :500-501
    for (int j = 0; j < k; ++j) {
        int c0 = cw ? k - 1 - j : j, c1 = cw ? (k - 1 - ((j + 1) % k)) : (j + 1) % k;
        double ex = px[c1] - px[c0], ey = py[c1] - py[c0];
        double a0 = ey, a1 = -ex;                                  // A = [edge_y, -edge_x]   :505-506
        A[2 * j] = a0; A[2 * j + 1] = a1;
        b[j] = a0 * px[c0] + a1 * py[c0];   // sum(A * cur, axis=1)   :507
    }
    return convex;
}

// one thread per (slot, time slot): half-space form of the selected obstacle at time t
__device__ __forceinline__ void build_body(const Args &a, const int w)
{
#pragma clang fp contract(off)
    if (w >= a.N * a.nt) return;
    const int s = w / a.nt, t = w % a.nt;
    const int used = a.n < a.N ? a.n : a.N;
    const int i = a.sel[s < used ? s : used - 1];                 // quirk Q3: pad with copies of the last obstacle
    const int E = a.E;
    const double *g = a.geom + (size_t)i * E * 2;
    double *A = a.A + ((size_t)s * a.nt + t) * E * 2, *b = a.b + ((size_t)s * a.nt + t) * E;
    zero_rows(A, b, E);
    const double vx = a.vel[2 * i], vy = a.vel[2 * i + 1];
    const bool moving = sqrt(vx * vx + vy * vy) > 0.01;     // mpc.py:443,462
    const double tt = (double)t * a.dt;
    const double sx = moving ? vx * tt : 0.0, sy = moving ? vy * tt : 0.0;
    if (a.kind[i] == 1) {
        if (t == 0) a.cone[s] = 1;
        A[0] = 1; A[3] = 1;                                        // [[1,0],[0,1],[0,0]]   mpc.py:441
        b[0] = moving ? g[0] + sx : g[0];
        b[1] = moving ? g[1] + sy : g[1];
        b[2] = -g[2];
        return;
    }
    if (t == 0) a.cone[s] = 0;
    const int k = a.nvert[i];
    double px[16], py[16];
    for (int j = 0; j < k; ++j) { px[j] = moving ? g[2 * j] + sx : g[2 * j]; py[j] = moving ? g[2 * j + 1] + sy : g[2 * j + 1]; }
    const bool convex = polygon_rows(px, py, k, A, b);
    if (!convex && t == 0 && s < used) atomicAdd(a.nonconvex, 1);
}
__global__ void k_build(Args a) { build_body(a, blockIdx.x * blockDim.x + threadIdx.x); }

// The same three kernels for a FLEET (rda_fleet_scene_resort, round 6): blockIdx.y = the member, its Args in a device array, its robot position in
// rob [B][2] - one launch set re-sorts the resident scenes of all members about their robots (64 members x 4 launches on 64 streams cost the host
// 4 ms per fleet tick; this is 4 launches).  Same device code per member: the slots come out bit-identical to rda_scene_resort on the member.
// rob == null (rda_fleet_upload_scans: scenes staged for the first time): every member's Args are taken as they stand - its own `order`, the robot
// position its raw scene holds.  A member with n = 0 has no scene: nothing of it is read or written (build_body would index sel[used - 1]).
__device__ __forceinline__ Args fleet_args(const Args *as, const double *rob)
{
    Args a = as[blockIdx.y];
    if (rob) { a.order = 1; a.robot_val = 1; a.rx = rob[2 * blockIdx.y]; a.ry = rob[2 * blockIdx.y + 1]; }
    return a;
}
__global__ void k_keys_fleet(const Args *as, const double *rob)
{
    const Args a = fleet_args(as, rob);
    if (a.n <= 0) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.nonconvex = 0;        // (k_build, later in the stream, counts into it)
    keys_body(a, blockIdx.x * blockDim.x + threadIdx.x);
}
__global__ void k_rank_fleet(const Args *as, const double *rob) { const Args a = fleet_args(as, rob); if (a.n <= 0) return; rank_body(a, blockIdx.x); }
__global__ void k_build_fleet(const Args *as, const double *rob)
{
    const Args a = fleet_args(as, rob);
    if (a.n <= 0) return;
    build_body(a, blockIdx.x * blockDim.x + threadIdx.x);
}

// Obstacle motion between two ticks of a rollout (rda_fleet_rollout_moving): what World.step and tools/closed_loop_host.c:60-66 do on the host, for the
// whole fleet in one launch - blockIdx.y = the member, one thread per (obstacle, vertex entry).  The position is always computed from `base`, the snapshot
// of the member's raw geometry taken when the call started (k_snapshot_fleet), never incrementally: geometry at tick k = base + vel * (dt * k), every product
// and the sum separately rounded.  Polygon: entries v < nvert, both coordinates; circle: entry 0 (the centre) - the radius entry and the padding never change.
// Every obstacle moves, also those below the 0.01 m/s under which k_build does not PREDICT motion.
struct Move {
    double *geom;           // [n][E][2] the member's resident raw geometry (Args::geom)
    double *base;           // [n][E][2] its snapshot
    const double *vel;      // [n][2]
    const int *kind, *nvert;
    int n, E;
    double dt;
};
__global__ void k_snapshot_fleet(const Move *ms)
{
    const Move m = ms[blockIdx.y];
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= m.n * m.E) return;
    m.base[2 * w] = m.geom[2 * w]; m.base[2 * w + 1] = m.geom[2 * w + 1];
}
__global__ void k_move_fleet(const Move *ms, int k)
{
#pragma clang fp contract(off)
    const Move m = ms[blockIdx.y];
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= m.n * m.E) return;
    const int i = w / m.E, v = w - i * m.E;
    if (m.kind[i] == 1 ? v != 0 : v >= m.nvert[i]) return;
    const double tk = m.dt * (double)k;
    m.geom[2 * w] = m.base[2 * w] + m.vel[2 * i] * tk;
    m.geom[2 * w + 1] = m.base[2 * w + 1] + m.vel[2 * i + 1] * tk;
}

// Fleet members as each other's obstacles (rda_fleet_upload_scenes_peers, rda_fleet_scene_resort_peers, rda_fleet_rollout_peers): what
// scenarios.peer_obstacles builds on the host, written into the B - 1 rows that follow the member's own obstacles in its resident raw scene - blockIdx.y =
// the member i, one thread per (peer row, vertex entry).  Row r of the tail is member j = r < i ? r : r + 1 (ascending j without i): the R vertices of j's
// footprint Rot(theta_j) rv_j + p_j (scenarios.robot_vertices; rv: the body-frame vertices the host solves, member_move_clear) and, by the thread of entry
// 0, the row's velocity (v cos a, v sin a) with (v, w) = controls[j], a = theta_j for acker / diff and a = w for omni (scenarios.kinematic_step's rule).
// kind = 0, nvert = R and the zero padding of entries >= R are staged by the host once; nothing but the tail rows is written.
struct Peer {                 // per member: its tail (null before the peers upload) and what the others need of it
    double *geom;             // first peer row of its raw geometry: Args::geom + n_own * E * 2
    double *vel;              // ... of its velocities: Args::vel + n_own * 2
    int n_own, E, R, dynamics;     // own obstacles in front of the tail; vertex stride; robot vertices; rda_cfg::dynamics
    double rv[RDA_RMAX][2];   // body frame
};
__global__ void k_peers_fleet(const Peer *ps, const double *states, const double *controls, int B)
{
#pragma clang fp contract(off)
    const int i = blockIdx.y;
    const Peer &me = ps[i];
    const int E = me.E;
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= (B - 1) * E) return;
    const int r = w / E, v = w - r * E;
    const int j = r < i ? r : r + 1;
    const Peer &p = ps[j];
    if (v >= p.R) return;
    const double x = states[3 * j], y = states[3 * j + 1], th = states[3 * j + 2];
    const double co = cos(th), si = sin(th);
    double *g = me.geom + ((size_t)r * E + v) * 2;
    g[0] = (co * p.rv[v][0] - si * p.rv[v][1]) + x;
    g[1] = (si * p.rv[v][0] + co * p.rv[v][1]) + y;
    if (v == 0) {
        const double sp = controls[2 * j], a = p.dynamics == 2 ? controls[2 * j + 1] : th;
        me.vel[2 * r] = sp * cos(a);
        me.vel[2 * r + 1] = sp * sin(a);
    }
}

// Peers predicted along their PLANNED trajectories (rda_fleet_*_peers_plan; scenarios.peer_plan_poses / peer_plan_obstacles are the specification):
// k_build_fleet's grid and body, but stage t >= 1 of a slot whose source row is the peer row of a VALID member j is the half-space form of j's footprint
// at pose_t = x_j + (q_t - P[:,1]), q_t = P[:,t+1] for t < T and q_T = P[:,T] + (P[:,T] - P[:,T-1]): the plan P [3][T+1] (the states j's last solve left)
// taken as displacements anchored at j's state x_j at the start of the tick, all three components alike, every difference and sum rounded separately.
// Everything else - own obstacles, stage 0, peers that are not valid (no solve yet, after a reset, arrived: predicted at constant velocity as before) -
// is build_body itself; a padded copy of a peer (quirk Q3) goes through the same `sel` entry and gets the plan too.
struct Plan {
    const double *states;     // [B][3] the members' states at the start of the tick
    const double *base;       // member j's plan: base + j * stride, [3][T+1]
    size_t stride;
    const int *valid;         // [B] != 0: j's plan counts; null: arrived_at decides
    const int *arrived_at;    // [B] the rollout's log: j counts while arrived_at[j] < 0
};
__device__ __forceinline__ void plan_body(const Args &a, const int w, const Peer *ps, const Plan &pl, const int B)
{
#pragma clang fp contract(off)
    if (w >= a.N * a.nt) return;
    const int s = w / a.nt, t = w % a.nt;
    const int used = a.n < a.N ? a.n : a.N;
    const int i = a.sel[s < used ? s : used - 1];
    const int me = blockIdx.y, r = i - ps[me].n_own, T = a.T;
    const int j = r < me ? r : r + 1;
    const bool peer = r >= 0 && r < B - 1 && t >= 1 && t <= T && a.kind[i] == 0;
    if (!peer || !(pl.valid ? pl.valid[j] != 0 : pl.arrived_at[j] < 0)) { build_body(a, w); return; }
    const Peer &p = ps[j];
    const int E = a.E, R = p.R < E ? p.R : E;
    double *A = a.A + ((size_t)s * a.nt + t) * E * 2, *b = a.b + ((size_t)s * a.nt + t) * E;
    zero_rows(A, b, E);
    const double *P = pl.base + (size_t)j * pl.stride;
    double pose[3];
    for (int c = 0; c < 3; ++c) {
        const double *Pc = P + (size_t)c * (T + 1);
        const double q = t < T ? Pc[t + 1] : Pc[T] + (Pc[T] - Pc[T - 1]);
        pose[c] = pl.states[3 * j + c] + (q - Pc[1]);
    }
    const double co = cos(pose[2]), si = sin(pose[2]);
    double px[RDA_RMAX], py[RDA_RMAX];
    for (int v = 0; v < R; ++v) {
        px[v] = (co * p.rv[v][0] - si * p.rv[v][1]) + pose[0];
        py[v] = (si * p.rv[v][0] + co * p.rv[v][1]) + pose[1];
    }
    polygon_rows(px, py, R, A, b);
}
__global__ void k_build_plan_fleet(const Args *as, const double *rob, const Peer *ps, Plan pl, int B)
{
    const Args a = fleet_args(as, rob);
    if (a.n <= 0) return;
    plan_body(a, blockIdx.x * blockDim.x + threadIdx.x, ps, pl, B);
}

}  // namespace scene
