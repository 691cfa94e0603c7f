// The closed MPC loop's host half on the device (rda_fleet_rollout): what a caller does between two fleet ticks -
//   read every member's first control and its path index                    tools/closed_loop_host.c:129-133
//   the arrival rule of MPC._end (zero control from the arrival tick on)    mpc.py:166-187
//   apply the control to the member's kinematic model                       tools/closed_loop_host.c:134-136, ir-sim's env.step
//   hand the new state to the tracker and to the obstacle re-sort           rda_fleet_step_tracked / rda_fleet_scene_resort
// - as one thread per member, launched behind the launch that ends tick k.  It writes where the kernels of tick k + 1 read (track::In, the
// re-sort's robot positions), so K ticks are queued back to back and the host waits once.  Products and sums are rounded separately like
// the C expressions (no FMA contraction); sin / cos / tan come from the device maths library: the states agree with the host loop's to the
// last bits, not bit for bit - everything downstream of a given state is the same kernels on the same data.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/rda_hip.h"
#include "track_device.h"
#include "scene_device.h"

namespace rollout {

struct Member {               // per member, constant over a rollout
    const double *out_u;      // the member's result block: controls [2][T] (the first control is out_u[0], out_u[T])
    const rda_info *info;     // the tick's rda_info (device)
    int T, L, dynamics, pad;  // horizon, waypoints of the uploaded path, rda_cfg::dynamics
    double dt, wheelbase;
};

struct Logs {                 // device logs of one rollout (one block, copied to the host once)
    double *states;           // [K+1][B][3]   row 0: the caller's states (written by the host), row k + 1: after tick k
    double *u;                // [K][B][2]     applied controls
    rda_info *info;           // [K][B]
    int *index;               // [K][B]        min_index of the tick
    int *arrived_at;          // [B]           first tick with min_index >= L - goal_margin, -1: none yet
    double *end_heading;      // [B]           track::Out::end_heading of the last tick (quirk Q12: the value the last waypoint's heading now has)
};

// The gear pieces of reverse paths (rda_fleet_rollout_gears): the bookkeeping of MPC._piece / _end / _sync_path (mpc.py:139-147, 166-187) on the device.
// Per member, constant over a rollout: the resident pieces of rda_upload_path_pieces and the call's unsigned reference speed ...
struct Gears {
    double *buf;              // [sum len][3] all pieces, one behind the other (the last waypoint's heading of every piece is rewritten by the tracker, Q12)
    const int *off;           // [P+1] first waypoint of every piece
    const double *gear;       // [P] +1 / -1
    int P, hbase;             // pieces; the member's first entry of the member-major heading array (k_gear_headings)
    double ref_speed;         // unsigned: In::speed of a piece is the single product gear[p] * ref_speed
};
// ... and the tables of a gear rollout, written by the host for tick 0 and by the advance kernel for tick k + 1: the piece in force [B], what k_track_fleet
// reads as the members' paths and lengths [B] (the piece's place in `buf`), and the log piece_log [K][B] of the piece in force during tick k
struct GearTab { const Gears *rec; int *piece; double **paths; int *lens; int *piece_log; };

// One member's step between two ticks.  gt null: a plain path of m.L waypoints.  With gear pieces the arrival rule is MPC._end's: at the end of a piece
// that another one follows the member has not arrived - the control is applied, the next piece comes into force with cur_index = 0 and its signed speed; at
// the end of the last piece it arrives as a plain member does and stays on that piece.  The nominal controls are not touched (the reference keeps
// cur_vel_array over a switch).
__device__ __forceinline__ void advance_member(const Member *ms, const track::Out *trk_out, track::In *trk_in, double *rob, const Logs &lg, int k, int goal_margin,
                                               int B, int i, const GearTab *gt)
{
#pragma clang fp contract(off)        // the host loop's compiler does not fuse either: every product and sum separately rounded
    const Member m = ms[i];
    const track::Out o = trk_out[i];
    track::In in = trk_in[i];
    const size_t row = (size_t)k * B + i;
    int arrived = lg.arrived_at[i];
    const int L = gt ? gt->lens[i] : m.L;
    int p = 0;
    bool next_piece = false;
    if (gt) { p = gt->piece[i]; gt->piece_log[row] = p; }
    if (arrived < 0 && o.min_index >= L - goal_margin) {
        if (gt && p + 1 < gt->rec[i].P) next_piece = true;
        else { arrived = k; lg.arrived_at[i] = k; }
    }
    double v = 0.0, w = 0.0;
    if (arrived < 0) {
        v = m.out_u[0]; w = m.out_u[m.T];
        const double phi = in.sth;
        if (m.dynamics == 0) { in.sx += m.dt * (v * cos(phi)); in.sy += m.dt * (v * sin(phi)); in.sth += m.dt * (v * tan(w) / m.wheelbase); }
        else if (m.dynamics == 1) { in.sx += m.dt * (v * cos(phi)); in.sy += m.dt * (v * sin(phi)); in.sth += m.dt * w; }
        else { in.sx += m.dt * (v * cos(w)); in.sy += m.dt * (v * sin(w)); }
    }
    in.cur_index = o.min_index;
    if (next_piece) {
        const Gears g = gt->rec[i];
        p = p + 1;
        const int first = g.off[p];
        gt->piece[i] = p; gt->paths[i] = g.buf + 3 * (size_t)first; gt->lens[i] = g.off[p + 1] - first;
        in.cur_index = 0; in.speed = g.gear[p] * g.ref_speed;
    }
    trk_in[i] = in;
    if (rob) { rob[2 * i] = in.sx; rob[2 * i + 1] = in.sy; }
    double *s = lg.states + ((size_t)(k + 1) * B + i) * 3;
    s[0] = in.sx; s[1] = in.sy; s[2] = in.sth;
    lg.u[2 * row] = v; lg.u[2 * row + 1] = w;
    lg.index[row] = o.min_index;
    lg.info[row] = *m.info;
    lg.end_heading[i] = o.end_heading;
}

// rob: the re-sort's robot positions [B][2], null when the rollout does not re-sort
__global__ void k_rollout_advance(const Member *ms, const track::Out *trk_out, track::In *trk_in, double *rob, Logs lg, int k, int goal_margin, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    advance_member(ms, trk_out, trk_in, rob, lg, k, goal_margin, B, i, nullptr);
}
// ... of a gear rollout
__global__ void k_rollout_advance_gears(const Member *ms, const track::Out *trk_out, track::In *trk_in, double *rob, Logs lg, int k, int goal_margin, int B,
                                        GearTab gt)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    advance_member(ms, trk_out, trk_in, rob, lg, k, goal_margin, B, i, &gt);
}
// behind the last tick: the heading the last waypoint of every piece has now (quirk Q12), member-major - out[hbase + p]
__global__ void k_gear_headings(const Gears *gs, double *out, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const Gears g = gs[i];
    for (int p = 0; p < g.P; ++p) out[g.hbase + p] = g.buf[3 * (size_t)(g.off[p + 1] - 1) + 2];
}

// Robot / obstacle clearance of every member on the device (rda_fleet_rollout_moving's clearance log, rda_fleet_clearance): scenarios.clearance for a polygon
// robot against ALL n obstacles of the member's resident raw scene as it stands, not only the N staged ones.  One workgroup per member; its threads stride
// over the obstacles, the minimum is reduced by shuffles and LDS (a minimum is exact: its order is free).
//   robot vertices    body-frame intersections of consecutive rows of G x <= h (solved once on the host: Clear::rv), rotated and shifted by the state
//   winding           either, for the robot and for every obstacle polygon: `clockwise` (scenarios._clockwise) reads it off the shoelace sum of the
//                     world-frame vertices, products and sums rounded one by one; a zero sum counts as counter-clockwise
//   polygon obstacle  _poly_sep: the outward edge normals of both polygons (those of a clockwise polygon flipped), normalised with the 1e-300 floor; the
//                     larger gap wins; zero-length edges (a repeated vertex) are skipped.  Overlapping: minus the penetration depth.  Apart: the distance
//                     where a vertex faces an edge, the conservative separating-axis gap (never above the distance) where two vertices face each other
//   circle obstacle   point-segment distance of the centre to the robot's edges, negated when the centre lies in the footprint, minus the radius
// Convex polygons only; a polygon with a zero shoelace sum is not defined.  A member without a raw scene (n = 0): +inf.
struct Clear {                // per member
    const double *geom;       // [n][E][2] resident raw geometry (scene::Args::geom)
    const int *kind, *nvert;  // [n]
    int n, E, R, pad;         // R: robot vertices
    double rv[RDA_RMAX][2];   // body frame
};
constexpr int CLEAR_NT = 256;

// scenarios._clockwise: the shoelace sum of polygon V [k] is negative
__device__ __forceinline__ bool clockwise(const double *vx, const double *vy, int k)
{
#pragma clang fp contract(off)
    double s = 0.0;
    for (int i = 0; i < k; ++i) {
        const int i1 = i + 1 < k ? i + 1 : 0;
        s = s + (vx[i] * vy[i1] - vx[i1] * vy[i]);
    }
    return s < 0.0;
}

// gap of polygon W [kw] along the outward edge normals of polygon V [kv] (one half of _poly_sep); cw: V runs clockwise
__device__ __forceinline__ double sep_half(const double *vx, const double *vy, int kv, bool cw, const double *wx, const double *wy, int kw, double best)
{
#pragma clang fp contract(off)
    for (int i = 0; i < kv; ++i) {
        const int i1 = i + 1 < kv ? i + 1 : 0;
        const double ex = vx[i1] - vx[i], ey = vy[i1] - vy[i];
        if (ex == 0.0 && ey == 0.0) continue;             // a repeated vertex: no normal
        double len = sqrt(ey * ey + ex * ex);
        if (!(len > 1e-300)) len = 1e-300;
        const double nx = (cw ? -ey : ey) / len, ny = (cw ? ex : -ex) / len;
        double lo = INFINITY;
        for (int j = 0; j < kw; ++j) { const double p = nx * wx[j] + ny * wy[j]; if (p < lo) lo = p; }
        const double gap = lo - (nx * vx[i] + ny * vy[i]);
        if (gap > best) best = gap;
    }
    return best;
}

// states: [B][3] the members' states; out [B]
__global__ __launch_bounds__(CLEAR_NT) void k_clearance_fleet(const Clear *cs, const double *states, double *out, int B)
{
#pragma clang fp contract(off)
    __shared__ double rx[RDA_RMAX], ry[RDA_RMAX], part[CLEAR_NT / 64];
    const int b = blockIdx.x;
    if (b >= B) return;                                   // (uniform)
    const Clear &c = cs[b];
    const int R = c.R, E = c.E;
    if ((int)threadIdx.x < R) {
        const double x = states[3 * b], y = states[3 * b + 1], th = states[3 * b + 2];
        const double co = cos(th), si = sin(th);
        rx[threadIdx.x] = (co * c.rv[threadIdx.x][0] - si * c.rv[threadIdx.x][1]) + x;
        ry[threadIdx.x] = (si * c.rv[threadIdx.x][0] + co * c.rv[threadIdx.x][1]) + y;
    }
    __syncthreads();
    const bool rcw = clockwise(rx, ry, R);
    double best = INFINITY;
    for (int i = threadIdx.x; i < c.n; i += CLEAR_NT) {
        const double *g = c.geom + (size_t)i * E * 2;
        double d;
        if (c.kind[i] == 1) {
            const double cx = g[0], cy = g[1];
            bool inside = true;
            d = INFINITY;
            for (int j = 0; j < R; ++j) {
                const int j1 = j + 1 < R ? j + 1 : 0;
                const double ax = rx[j], ay = ry[j], abx = rx[j1] - ax, aby = ry[j1] - ay;
                double s = ((cx - ax) * abx + (cy - ay) * aby) / (abx * abx + aby * aby);
                s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
                const double px = (ax + s * abx) - cx, py = (ay + s * aby) - cy;
                const double e = sqrt(px * px + py * py);
                if (e < d) d = e;
                const double side = abx * (cy - ay) - aby * (cx - ax);
                inside = inside && (rcw ? side <= 0.0 : side >= 0.0);
            }
            d = (inside ? -d : d) - g[2];
        } else {
            int k = c.nvert[i];
            if (k > RDA_EMAX) k = RDA_EMAX;
            double qx[RDA_EMAX], qy[RDA_EMAX];
            for (int j = 0; j < k; ++j) { qx[j] = g[2 * j]; qy[j] = g[2 * j + 1]; }
            d = sep_half(rx, ry, R, rcw, qx, qy, k, -INFINITY);
            d = sep_half(qx, qy, k, clockwise(qx, qy, k), rx, ry, R, d);
        }
        if (d < best) best = d;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = fmin(best, __shfl_xor(best, off, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CLEAR_NT / 64; ++w) best = fmin(best, part[w]);
        out[b] = best;
    }
}

// Member-to-member separation (rda_fleet_rollout_peers' peer clearance log, rda_fleet_peer_clearance): scenarios.peer_clearance - for member i the minimum
// over j != i of _poly_sep(RV_i, RV_j), both footprints rotated and shifted by their states as in k_clearance_fleet.  One wave per member; its lanes stride
// over the peers, each runs sep_half both ways (footprints of either winding, as there), the minimum goes through the wave by shuffles (exact: its order is
// free).  Launched for B >= 2 only.
__device__ __forceinline__ void peer_footprint(const scene::Peer &p, const double *state, double *fx, double *fy)
{
#pragma clang fp contract(off)
    const double x = state[0], y = state[1], co = cos(state[2]), si = sin(state[2]);
    for (int v = 0; v < p.R; ++v) {
        fx[v] = (co * p.rv[v][0] - si * p.rv[v][1]) + x;
        fy[v] = (si * p.rv[v][0] + co * p.rv[v][1]) + y;
    }
}
__global__ __launch_bounds__(64) void k_peer_clearance_fleet(const scene::Peer *ps, const double *states, double *out, int B)
{
    const int i = blockIdx.x;
    if (i >= B) return;                                   // (uniform)
    double rx[RDA_RMAX], ry[RDA_RMAX], qx[RDA_RMAX], qy[RDA_RMAX];
    const int R = ps[i].R;
    peer_footprint(ps[i], states + 3 * i, rx, ry);
    const bool rcw = clockwise(rx, ry, R);
    double best = INFINITY;
    for (int j = threadIdx.x; j < B; j += 64) {
        if (j == i) continue;
        peer_footprint(ps[j], states + 3 * j, qx, qy);
        double d = sep_half(rx, ry, R, rcw, qx, qy, ps[j].R, -INFINITY);
        d = sep_half(qx, qy, ps[j].R, clockwise(qx, qy, ps[j].R), rx, ry, R, d);
        if (d < best) best = d;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = fmin(best, __shfl_xor(best, off, 64));
    if (threadIdx.x == 0) out[i] = best;
}

}  // namespace rollout
