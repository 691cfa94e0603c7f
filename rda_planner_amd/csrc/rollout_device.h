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

// rob: the re-sort's robot positions [B][2], null when the rollout does not re-sort
__global__ void k_rollout_advance(const Member *ms, const track::Out *trk_out, track::In *trk_in, double *rob, Logs lg, int k, int goal_margin, int B)
{
#pragma clang fp contract(off)        // the host loop's compiler does not fuse either: every product and sum separately rounded
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const Member m = ms[i];
    const track::Out o = trk_out[i];
    track::In in = trk_in[i];
    const size_t row = (size_t)k * B + i;
    int arrived = lg.arrived_at[i];
    if (arrived < 0 && o.min_index >= m.L - goal_margin) { arrived = k; lg.arrived_at[i] = k; }
    double v = 0.0, w = 0.0;
    if (arrived < 0) {
        v = m.out_u[0]; w = m.out_u[m.T];
        const double phi = in.sth;
        if (m.dynamics == 0) { in.sx += m.dt * (v * cos(phi)); in.sy += m.dt * (v * sin(phi)); in.sth += m.dt * (v * tan(w) / m.wheelbase); }
        else if (m.dynamics == 1) { in.sx += m.dt * (v * cos(phi)); in.sy += m.dt * (v * sin(phi)); in.sth += m.dt * w; }
        else { in.sx += m.dt * (v * cos(w)); in.sy += m.dt * (v * sin(w)); }
    }
    in.cur_index = o.min_index;
    trk_in[i] = in;
    if (rob) { rob[2 * i] = in.sx; rob[2 * i + 1] = in.sy; }
    double *s = lg.states + ((size_t)(k + 1) * B + i) * 3;
    s[0] = in.sx; s[1] = in.sy; s[2] = in.sth;
    lg.u[2 * row] = v; lg.u[2 * row + 1] = w;
    lg.index[row] = o.min_index;
    lg.info[row] = *m.info;
    lg.end_heading[i] = o.end_heading;
}

}  // namespace rollout
