// Lidar front end on the device: what the reference's lidar example does per tick in host Python before MPC.control -
//   scan_box of example/lidar_nav/lidar_path_track.py:20-60: ranges -> hit points -> DBSCAN -> one minimum-area rectangle per cluster -> world frame
// - as ONE workgroup whose hit points stay in LDS from the first stage to the last.  The specification is rda_planner_amd/lidar.py, stage by
// stage (scan_points, dbscan, convex_hull, min_area_rect, scan_box); the arithmetic follows its numpy expressions (FMA contraction is switched off),
// so that every DECISION (hit, near, core, hull turn, best edge) is taken on the same numbers up to the ulp of the device's cos / sin.
//
// DBSCAN is restated order-free: core = at least min_samples points within eps (itself included); clusters = connected components of the core points,
// numbered by their smallest core index; a border point joins the lowest-numbered cluster that has a core point within eps; the rest is noise.  That is
// the labelling of lidar.dbscan (and scikit-learn's): their depth-first expansion finishes cluster c before c + 1 starts.  Components are found by
// min-label propagation with path compression over recomputed pair tests: labels only ever decrease and always name a point of the own component, so
// concurrent updates need no ordering and the fixed point (every core point carries the smallest index of its component) is unique.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/rda_hip.h"
#include "scene_device.h"

namespace lidar {

constexpr int MAXB = 4096;              // beams (and so hit points) a scan may have
constexpr int NT = 1024;                // threads of the workgroup
constexpr int PER = MAXB / NT;          // consecutive beams of a thread
constexpr int NW = NT / 64;
constexpr int NONE = 0x7fffffff;        // label of a point that is not core / cluster key of a noise point
// LDS: px, py [MAXB] doubles | ia, ib [MAXB] ints | ic [MAXB + 1] ints | scan scratch [32] ints
constexpr size_t LDS_BYTES = 2 * MAXB * sizeof(double) + (3 * MAXB + 1 + 32) * sizeof(int);

struct Args {
    int n_beams; const double *ranges;              // [n_beams]
    double angle_min, angle_max, range_max;
    double sx, sy, sth;                              // sensor pose in the world frame
    double eps; int min_samples;
    double *boxes;                                   // [MAXB][4][2] world frame, counter-clockwise, cluster order (device memory)
    int *count;                                      // [0] boxes, [1] hits (pinned host memory: the host waits for the kernel and reads them)
    int *labels_h;                                   // (may be null) [n_beams] -2 miss, -1 noise, >= 0 cluster, pinned host memory
    double *boxes_h;                                 // (may be null) the host's copy of `boxes`, pinned host memory
    double split_tol;                                // 0: one box per cluster | > 0 [m]: one per straight run (split_stage); count[0], labels_h, boxes: segments
};

extern __shared__ __attribute__((aligned(16))) double smem_lidar[];

// exclusive prefix sum of one int per thread in thread order; `total` = the sum over the workgroup
__device__ __forceinline__ int block_scan(const int v, int *wtot, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(inc, off); if (lane >= off) inc += t; }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    if (wave == 0) {
        const int w = lane < NW ? wtot[lane] : 0;
        int winc = w;
#pragma unroll
        for (int off = 1; off < NW; off <<= 1) { const int t = __shfl_up(winc, off); if (lane >= off) winc += t; }
        if (lane < NW) wtot[lane] = winc - w;
        if (lane == NW - 1) wtot[NW] = winc;
    }
    __syncthreads();
    const int r = wtot[wave] + inc - v;
    total = wtot[NW];
    __syncthreads();                                 // (wtot is reused by the next scan)
    return r;
}

__device__ __forceinline__ bool near(const double xi, const double yi, const double xj, const double yj, const double eps2)
{
#pragma clang fp contract(off)
    const double dx = xi - xj, dy = yi - yj;
    return dx * dx + dy * dy <= eps2;
}

// extents of the hull vertices k = k0, k0 + stride, ... along the direction of hull edge e and across it (min_area_rect: a = H @ u, b = H @ v)
struct Extent { double ux, uy, lo, hi, wlo, whi; };
__device__ __forceinline__ Extent edge_extent(const double *px, const double *py, const int *hull, const int h, const int e, const int k0, const int stride)
{
#pragma clang fp contract(off)
    const int p0 = hull[e], p1 = hull[e + 1 < h ? e + 1 : 0];
    const double ex = px[p1] - px[p0], ey = py[p1] - py[p0];
    const double nrm = sqrt(ex * ex + ey * ey);
    Extent x;
    x.ux = ex / nrm; x.uy = ey / nrm;
    const double vx = -x.uy, vy = x.ux;
    x.lo = INFINITY; x.hi = -INFINITY; x.wlo = INFINITY; x.whi = -INFINITY;
    for (int k = k0; k < h; k += stride) {
        const double hx = px[hull[k]], hy = py[hull[k]];
        const double a = hx * x.ux + hy * x.uy, b = hx * vx + hy * vy;
        x.lo = fmin(x.lo, a); x.hi = fmax(x.hi, a); x.wlo = fmin(x.wlo, b); x.whi = fmax(x.whi, b);
    }
    return x;
}

// The split stage (Args::split_tol > 0; lidar.split_runs is the specification, expression by expression): every cluster is cut into its straight runs,
// the labels in ic become SEGMENT numbers and the hull stage boxes segments.  Called by the whole workgroup with the final cluster labels in ic [nh] and
// the hits in beam order; returns the number of segments.  What it leaves: px, py, ic [nh] permuted alike into (cluster, beam) order with the noise
// behind (the sort that follows takes any order), ic = the segment of the point at that position (-1 noise), and split_pos(ia)[i] = the position of hit i.
//   order     the hits are in beam order already, so a cluster is a few STRETCHES of consecutive hits (one, unless clusters interleave): the heads of the R
//             stretches are compacted by a block_scan, and stretch r starts at the number of hits in stretches of a lower cluster or of the same cluster
//             and a lower r - R * R integer steps over R threads instead of an nh * nh rank pass; R is the number of clusters plus a few
//   runs      a run starts where the cluster changes or the gap rule fails (`near` on neighbours).  start[p] = the first position of p's run, end[first] =
//             its last one; both from a second block_scan over the run heads
//   rounds    every run [a, b] with b - a >= 2 that has not been found straight is tested at once, a thread per position: s_p as the specification
//             writes it, the maximum over a < p < b by a 64-bit LDS atomic max on the bits of s_p (non-negative doubles order like their bit patterns;
//             a wave that lies inside one run reduces by shuffles first and issues one atomic), then the lowest p at the maximum by an atomic min if
//             that maximum exceeds the bound.  A run that splits at m becomes [a, m - 1] and [m, b]; one that does not is marked final.  A run's test
//             reads nothing but that run, so the rounds reach the fixed point of the specification whatever their order; they end when nothing splits
//   slots     a run that can split has >= 3 points, so the heads of two such runs are >= 3 apart and head / 3 is a slot of its own for the maximum and
//             the split point: SPLIT_SLOTS of 12 bytes instead of MAXB.  The head resets its slot at the end of the round
//   numbers   segments are numbered in position order of their heads (cluster, then first point): a third block_scan
// LDS: nothing added.  Four u16 arrays [MAXB] over ia | ib (positions fit 13 bits) - stretch / run heads, start (stretch bases before), pos, end - and
// the slots over ic once the labels in it have been used.  Every barrier is reached by the whole workgroup.
typedef unsigned short u16;
constexpr int SPLIT_SLOTS = (MAXB - 3) / 3 + 1;           // the last head that can split is MAXB - 3
constexpr int SPLIT_FINAL = 0x8000;                       // in end[head]: the run has been found straight
static_assert(MAXB < SPLIT_FINAL, "a position and the final mark share a u16");
static_assert(4 * MAXB * sizeof(u16) <= 2 * MAXB * sizeof(int), "heads, start, pos, end lie in ia | ib");
static_assert(SPLIT_SLOTS * (sizeof(unsigned long long) + sizeof(int)) <= (MAXB + 1) * sizeof(int), "the slots lie in ic");
static_assert((2 * MAXB * sizeof(double) + 2 * MAXB * sizeof(int)) % sizeof(unsigned long long) == 0, "ic is aligned for the 64-bit slots");
__device__ __forceinline__ const u16 *split_pos(const int *ia) { return reinterpret_cast<const u16 *>(ia) + 2 * MAXB; }

__device__ __forceinline__ int split_stage(double *px, double *py, int *ia, int *ic, int *wtot, const int nh, const double eps2, const double tol)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63;
    u16 *hl = reinterpret_cast<u16 *>(ia), *start = hl + MAXB, *pos = hl + 2 * MAXB, *end = hl + 3 * MAXB;
    int *first_noise = wtot + NW + 1, *changed = wtot + NW + 2;                 // (behind what block_scan uses)
    if (tid == 0) *first_noise = nh;

    // ---- (cluster, beam) order: stretches of consecutive hits with one label ----------------------------------------------------------------------
    int heads = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { const int i = tid * PER + k; heads += (i < nh && (i == 0 || ic[i] != ic[i - 1])) ? 1 : 0; }
    int R;
    int r0 = block_scan(heads, wtot, R);
    {
        int o = r0;
#pragma unroll
        for (int k = 0; k < PER; ++k) { const int i = tid * PER + k; if (i < nh && (i == 0 || ic[i] != ic[i - 1])) hl[o++] = (u16)i; }
    }
    __syncthreads();
    for (int r = tid; r < R; r += NT) {                                         // start[r] = where stretch r begins
        const int c = ic[hl[r]] < 0 ? NONE : ic[hl[r]];
        int base = 0, j0 = hl[0];
        for (int q = 0; q < R; ++q) {
            const int j1 = q + 1 < R ? hl[q + 1] : nh;
            const int cq = ic[j0] < 0 ? NONE : ic[j0];
            if (cq < c || (cq == c && q < r)) base += j1 - j0;
            j0 = j1;
        }
        start[r] = (u16)base;
    }
    __syncthreads();
    {
        double tx[PER], ty[PER]; int tc[PER], tp[PER];
        int o = r0 - 1;                                                         // (a thread's first hit is a head or belongs to the stretch before)
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid * PER + k;
            tp[k] = 0;
            if (i < nh) {
                if (i == 0 || ic[i] != ic[i - 1]) ++o;
                tp[k] = start[o] + (i - hl[o]); tx[k] = px[i]; ty[k] = py[i]; tc[k] = ic[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid * PER + k;
            if (i < nh) { px[tp[k]] = tx[k]; py[tp[k]] = ty[k]; ic[tp[k]] = tc[k]; pos[i] = (u16)tp[k]; }
        }
        __syncthreads();
    }

    // ---- runs: a head where the cluster changes or the gap rule fails; a noise point is a run of its own that nobody tests ----------------------
    bool hd[PER];
    heads = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int p = tid * PER + k;
        hd[k] = false;
        if (p < nh) {
            const int c = ic[p];
            hd[k] = p == 0 || c < 0 || ic[p - 1] != c || !near(px[p - 1], py[p - 1], px[p], py[p], eps2);
            if (c < 0 && (p == 0 || ic[p - 1] >= 0)) *first_noise = p;
            heads += hd[k] ? 1 : 0;
        }
    }
    int R2;
    r0 = block_scan(heads, wtot, R2);
    {
        int o = r0;
#pragma unroll
        for (int k = 0; k < PER; ++k) if (hd[k]) hl[o++] = (u16)(tid * PER + k);
    }
    __syncthreads();
    {
        int o = r0 - 1;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int p = tid * PER + k;
            if (p < nh) {
                if (hd[k]) { ++o; end[p] = (u16)((o + 1 < R2 ? hl[o + 1] : nh) - 1); }
                start[p] = hl[o];
            }
        }
    }
    const int ncp = *first_noise;                                               // clustered points: positions 0 .. ncp - 1
    unsigned long long *smax = reinterpret_cast<unsigned long long *>(ic);      // (the labels in ic have been used: block_scan's barriers lie between)
    int *arg = reinterpret_cast<int *>(smax + SPLIT_SLOTS);
    for (int s = tid; s < SPLIT_SLOTS; s += NT) { smax[s] = 0ull; arg[s] = NONE; }
    __syncthreads();

    // ---- rounds of the end-point fit -------------------------------------------------------------------------------------------------------------
    const double tol2 = tol * tol;
    for (;;) {
        if (tid == 0) *changed = 0;
        int ra[PER], rb[PER]; double sv[PER], thr[PER]; bool act[PER], open[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int p = k * NT + tid;                                         // (a wave's lanes on consecutive positions)
            ra[k] = 0; rb[k] = 0; sv[k] = 0.0; thr[k] = 0.0; act[k] = false; open[k] = false;
            if (p < ncp) {
                const int a = start[p], e = end[a], b = e & (SPLIT_FINAL - 1);
                ra[k] = a; rb[k] = b;
                open[k] = !(e & SPLIT_FINAL) && b - a >= 2;
                if (open[k] && p > a && p < b) {
                    const double ex = px[b] - px[a], ey = py[b] - py[a];
                    const double L2 = ex * ex + ey * ey;
                    const double rx = px[p] - px[a], ry = py[p] - py[a];
                    if (L2 > 0) { const double cr = rx * ey - ry * ex; sv[k] = cr * cr; thr[k] = tol2 * L2; }
                    else { sv[k] = rx * rx + ry * ry; thr[k] = tol2; }
                    act[k] = true;
                }
            }
            unsigned long long bits = act[k] ? (unsigned long long)__double_as_longlong(sv[k]) : 0ull;
            const int a0 = __shfl(ra[k], 0);
            if (__all(act[k] && ra[k] == a0)) {                                 // the wave lies inside one run: one atomic
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) { const unsigned long long o = __shfl_xor(bits, off); bits = o > bits ? o : bits; }
                if (lane == 0) atomicMax(&smax[a0 / 3], bits);
            } else if (act[k]) atomicMax(&smax[ra[k] / 3], bits);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k)                                           // the lowest position at the maximum, if the maximum is beyond the bound
            if (act[k] && (unsigned long long)__double_as_longlong(sv[k]) == smax[ra[k] / 3] && sv[k] > thr[k]) atomicMin(&arg[ra[k] / 3], k * NT + tid);
        __syncthreads();
        int m[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) m[k] = open[k] ? arg[ra[k] / 3] : NONE;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int p = k * NT + tid;
            if (!open[k]) continue;
            if (m[k] != NONE) {                                                 // [a, b] -> [a, m - 1], [m, b]
                if (p >= m[k]) start[p] = (u16)m[k];
                if (p == m[k]) end[p] = (u16)rb[k];
                if (p == ra[k]) { end[p] = (u16)(m[k] - 1); *changed = 1; }
            } else if (p == ra[k]) end[p] = (u16)(rb[k] | SPLIT_FINAL);
            if (p == ra[k]) { smax[p / 3] = 0ull; arg[p / 3] = NONE; }
        }
        __syncthreads();
        const int again = *changed;
        __syncthreads();
        if (!again) break;
    }

    // ---- segment numbers in position order of the run heads ---------------------------------------------------------------------------------------
    heads = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { const int p = tid * PER + k; hd[k] = p < ncp && start[p] == p; heads += hd[k] ? 1 : 0; }
    int nseg;
    r0 = block_scan(heads, wtot, nseg);
    {
        int o = r0 - 1;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int p = tid * PER + k;
            if (hd[k]) ++o;
            if (p < nh) ic[p] = p < ncp ? o : -1;                               // (the slots are dead: the last round ended with a barrier)
        }
    }
    __syncthreads();
    return nseg;
}

// one scan by one workgroup of NT threads with LDS_BYTES of dynamic LDS (every return below is taken by the whole workgroup)
__device__ __forceinline__ void scan_body(const Args &a)
{
#pragma clang fp contract(off)        // numpy does not fuse: keep every product and sum separately rounded
    double *px = smem_lidar, *py = px + MAXB;
    int *ia = reinterpret_cast<int *>(py + MAXB), *ib = ia + MAXB, *ic = ib + MAXB, *wtot = ic + MAXB + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = a.n_beams;

    // ---- points: scan_points.  A thread owns PER consecutive beams, so the hits stay in beam order -----------------------------------------------
    const double thr = a.range_max - 0.01;
    const double step = nb > 1 ? (a.angle_max - a.angle_min) / (double)(nb - 1) : 0.0;       // np.linspace: start + i * step, the last one = stop
    double hx[PER], hy[PER]; bool hit[PER]; int cnt = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int b = tid * PER + k;
        hit[k] = false; hx[k] = 0; hy[k] = 0;
        if (b < nb) {
            const double r = a.ranges[b];
            if (r < thr) {                                                                   // (a NaN range is a miss)
                const double ang = (nb > 1 && b == nb - 1) ? a.angle_max : (double)b * step + a.angle_min;
                hit[k] = true; hx[k] = r * cos(ang); hy[k] = r * sin(ang); ++cnt;
            }
        }
    }
    int nh;
    const int first = block_scan(cnt, wtot, nh);
    {
        int o = first;
#pragma unroll
        for (int k = 0; k < PER; ++k) if (hit[k]) { px[o] = hx[k]; py[o] = hy[k]; ++o; }
    }
    __syncthreads();

    // ---- core points; ia = component label (own index), NONE for the others ----------------------------------------------------------------------
    const double eps2 = a.eps * a.eps;
    volatile int *lab = ia;
    for (int i = tid; i < nh; i += NT) {
        const double xi = px[i], yi = py[i];
        int c = 0;
        for (int j = 0; j < nh; ++j) c += near(xi, yi, px[j], py[j], eps2) ? 1 : 0;
        ia[i] = c >= a.min_samples ? i : NONE;
    }
    __syncthreads();

    // ---- connected components of the core points --------------------------------------------------------------------------------------------------
    for (;;) {
        if (tid == 0) wtot[0] = 0;
        __syncthreads();
        for (int i = tid; i < nh; i += NT) {
            const int mine = lab[i];
            if (mine == NONE) continue;
            const double xi = px[i], yi = py[i];
            int best = mine;
            for (int j = 0; j < nh; ++j) {
                const int lj = lab[j];
                if (lj < best && near(xi, yi, px[j], py[j], eps2)) best = lj;
            }
            for (int hop = 0; hop < MAXB; ++hop) { const int up = lab[best]; if (up >= best) break; best = up; }     // to the root as it stands
            if (best < mine) { lab[i] = best; wtot[0] = 1; }
        }
        __syncthreads();
        const int again = wtot[0];
        __syncthreads();
        if (!again) break;
    }

    // ---- cluster numbers: roots in index order; ib[root] = number --------------------------------------------------------------------------------
    int roots = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { const int p = tid * PER + k; roots += (p < nh && ia[p] == p) ? 1 : 0; }
    int nclus;
    {
        int o = block_scan(roots, wtot, nclus);
#pragma unroll
        for (int k = 0; k < PER; ++k) { const int p = tid * PER + k; if (p < nh && ia[p] == p) ib[p] = o++; }
    }
    __syncthreads();
    // final label of every point -> ic
    for (int i = tid; i < nh; i += NT) {
        int root = ia[i];
        if (root == NONE) {                                                    // border point: the lowest-numbered cluster with a core point in reach
            const double xi = px[i], yi = py[i];
            for (int j = 0; j < nh; ++j) {
                const int lj = ia[j];
                if (lj < root && near(xi, yi, px[j], py[j], eps2)) root = lj;
            }
        }
        ic[i] = root == NONE ? -1 : ib[root];
    }
    __syncthreads();
    // ---- (split_tol > 0) clusters -> straight runs: from here on a "cluster" is a segment, ic is indexed through split_pos -------------------------
    const bool split = a.split_tol > 0 && nclus > 0;                           // (uniform)
    if (split) nclus = split_stage(px, py, ia, ic, wtot, nh, eps2, a.split_tol);
    if (a.labels_h) {
        const u16 *pos = split_pos(ia);
        int o = first;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int b = tid * PER + k;
            if (b < nb) a.labels_h[b] = hit[k] ? ic[split ? (int)pos[o] : o] : -2;
            if (hit[k]) ++o;
        }
    }
    if (nh < 4) nclus = 0;                                                     // scan_box: fewer than 4 hits give no box
    if (tid == 0) { a.count[0] = nclus; a.count[1] = nh; }
    if (nclus == 0) return;

    // ---- sort the points by (cluster, x, y): every cluster becomes one segment in the order the monotone chain wants ----------------------------
    for (int i = tid; i < nh; i += NT) {
        const int ci = ic[i] < 0 ? NONE : ic[i];
        const double xi = px[i], yi = py[i];
        int r = 0;
        for (int j = 0; j < nh; ++j) {
            const int cj = ic[j] < 0 ? NONE : ic[j];
            const double xj = px[j], yj = py[j];
            const bool lt = cj != ci ? cj < ci : (xj != xi ? xj < xi : (yj != yi ? yj < yi : j < i));
            r += lt ? 1 : 0;
        }
        ia[i] = r;                                                             // (< nh whatever the values are)
    }
    __syncthreads();
    {
        double tx[PER], ty[PER]; int tc[PER], tr[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + k * NT;
            if (i < nh) { tx[k] = px[i]; ty[k] = py[i]; tc[k] = ic[i] < 0 ? NONE : ic[i]; tr[k] = ia[i]; }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + k * NT;
            if (i < nh) { px[tr[k]] = tx[k]; py[tr[k]] = ty[k]; ib[tr[k]] = tc[k]; }
        }
        if (tid == 0) ic[nclus] = nh;
        __syncthreads();
    }
    for (int p = tid; p < nh; p += NT) {                                        // ic[c] = first point of cluster c, ic[nclus] = end of the last one
        const int c = ib[p];
        if (p == 0 || ib[p - 1] != c) ic[c == NONE ? nclus : c] = p;
    }
    __syncthreads();

    // ---- one wave per cluster: convex_hull, min_area_rect, world frame.  ia / ib [segment] = the index stacks of the lower / upper chain ---------
    const double cs = cos(a.sth), sn = sin(a.sth);
    for (int c0 = 0; c0 < nclus; c0 += NW) {
        const int c = c0 + wave;
        const bool live = c < nclus;
        int s = 0, m = 0;
        if (live) { s = ic[c]; m = ic[c + 1] - s; if (s < 0 || m < 0 || s + m > nh) m = 0; }
        int *lo = ia + s, *up = ib + s;
        int nl = 0, nu = 0;
        if (live && lane == 0) {                                               // Andrew's monotone chain; equal points are taken once (np.unique)
            for (int p = s; p < s + m; ++p) {
                if (p > s && px[p] == px[p - 1] && py[p] == py[p - 1]) continue;
                while (nl >= 2) {
                    const int o = lo[nl - 2], q = lo[nl - 1];
                    const double ax = px[q] - px[o], ay = py[q] - py[o], bx = px[p] - px[o], by = py[p] - py[o];
                    if (ax * by - ay * bx <= 0) --nl; else break;
                }
                lo[nl++] = p;
            }
            for (int p = s + m - 1; p >= s; --p) {
                if (p < s + m - 1 && px[p] == px[p + 1] && py[p] == py[p + 1]) continue;
                while (nu >= 2) {
                    const int o = up[nu - 2], q = up[nu - 1];
                    const double ax = px[q] - px[o], ay = py[q] - py[o], bx = px[p] - px[o], by = py[p] - py[o];
                    if (ax * by - ay * bx <= 0) --nu; else break;
                }
                up[nu++] = p;
            }
        }
        __syncthreads();
        nl = __shfl(nl, 0); nu = __shfl(nu, 0);
        // hull = lower[:-1] + upper[:-1], gathered behind the lower chain (a hull has at most as many vertices as the segment has points)
        int h = nl <= 1 ? nl : nl + nu - 2;
        if (h > m) h = m;
        if (live && nl > 1) for (int k = lane; k < nu - 1; k += 64) { const int dst = nl - 1 + k; if (dst < h) lo[dst] = up[k]; }
        __syncthreads();
        if (live && h >= 1) {
            double ux = 1.0, uy = 0.0, l0 = 0.0, l1 = 0.0, w0 = 0.0, w1 = 0.0, cx = 0.0, cy = 0.0;
            if (h == 1) { cx = px[lo[0]]; cy = py[lo[0]]; }
            else {
                const int ne = h > 2 ? h : 1;                                  // a two-point hull has one edge
                double barea = 0.0; int be = NONE;
                for (int e = lane; e < ne; e += 64) {
                    const Extent x = edge_extent(px, py, lo, h, e, 0, 1);
                    const double area = (x.hi - x.lo) * (x.whi - x.wlo);
                    if (be == NONE || area < barea) { barea = area; be = e; }
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {                      // least area, the lowest edge index among equals
                    const double oa = __shfl_xor(barea, off); const int oe = __shfl_xor(be, off);
                    if (oe != NONE && (be == NONE || oa < barea || (oa == barea && oe < be))) { barea = oa; be = oe; }
                }
                be = __shfl(be, 0);
                if (be < 0 || be >= ne) be = 0;
                Extent x = edge_extent(px, py, lo, h, be, lane, 64);
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    x.lo = fmin(x.lo, __shfl_xor(x.lo, off)); x.hi = fmax(x.hi, __shfl_xor(x.hi, off));
                    x.wlo = fmin(x.wlo, __shfl_xor(x.wlo, off)); x.whi = fmax(x.whi, __shfl_xor(x.whi, off));
                }
                ux = x.ux; uy = x.uy; l0 = x.lo; l1 = x.hi; w0 = x.wlo; w1 = x.whi;
            }
            const double min_width = 0.01;
            if (l1 - l0 < min_width) { const double mid = 0.5 * (l0 + l1); l0 = mid - 0.5 * min_width; l1 = mid + 0.5 * min_width; }
            if (w1 - w0 < min_width) { const double mid = 0.5 * (w0 + w1); w0 = mid - 0.5 * min_width; w1 = mid + 0.5 * min_width; }
            if (lane < 4) {
                const double al = (lane == 0 || lane == 3) ? l0 : l1, aw = lane < 2 ? w0 : w1;
                const double vx = -uy, vy = ux;
                const double bx = cx + al * ux + aw * vx, by = cy + al * uy + aw * vy;
                const double wx = a.sx + (cs * bx + (-sn) * by), wy = a.sy + (sn * bx + cs * by);
                const size_t at = ((size_t)c * 4 + lane) * 2;
                a.boxes[at] = wx; a.boxes[at + 1] = wy;
                if (a.boxes_h) { a.boxes_h[at] = wx; a.boxes_h[at + 1] = wy; }
            }
        }
    }
}

__global__ __launch_bounds__(NT) void k_scan(const Args a) { scan_body(a); }

// The same for a FLEET (rda_fleet_scan_boxes / rda_fleet_upload_scans): blockIdx.x = the member, its Args (own beams, field of view, pose, box buffer,
// count words) in a device array.  Same device code per member, one workgroup each: boxes, labels and counts are bit-identical to k_scan's.
__global__ __launch_bounds__(NT) void k_scan_fleet(const Args *as)
{
    const Args a = as[blockIdx.x];
    if (a.n_beams <= 0) { if (threadIdx.x == 0) { a.count[0] = 0; a.count[1] = 0; } return; }
    scan_body(a);
}

// ... with the sensor pose read from device memory, poses [B][3] (rda_fleet_rollout_lidar: the pose is where rollout::k_rollout_advance left it, the host
// does not know it when it queues the launch; Args::ranges then points at what k_raycast_fleet wrote).  Same body: bit-identical to k_scan_fleet at that pose.
__global__ __launch_bounds__(NT) void k_scan_fleet_at(const Args *as, const double *poses)
{
    Args a = as[blockIdx.x];
    if (a.n_beams <= 0) { if (threadIdx.x == 0) { a.count[0] = 0; a.count[1] = 0; } return; }
    a.sx = poses[3 * blockIdx.x]; a.sy = poses[3 * blockIdx.x + 1]; a.sth = poses[3 * blockIdx.x + 2];
    scan_body(a);
}

// The sensor itself (rda_fleet_raycast, rda_fleet_rollout_lidar): exact ray casting of every member's beams against its resident WORLD - the true
// obstacles, kept apart from the raw scene that a lidar tick overwrites with boxes.  The specification is World.get_lidar_scan (rda_planner_amd/world.py),
// expression by expression (FMA contraction off):
//   beam i     angle_min + i * (angle_max - angle_min) / (n_beams - 1), the last one exactly angle_max, a single beam angle_min (scan_body's rule =
//              np.linspace); direction (cos, sin) of heading + angle, origin the pose's x, y
//   circle     f = o - c, b = d.f, disc = b * b - (f.f - r * r); a hit: disc >= 0 and t = -b - sqrt(disc) >= 0 (an origin inside the circle: no hit)
//   edge p->q  e = q - p, w = p - o, u = q - o, den = d.x e.y - d.y e.x, t = (w.x e.y - w.y e.x) / den, and the side of the beam's line that each vertex
//              lies on: side_p = w.x d.y - w.y d.x, side_q = u.x d.y - u.y d.x; a hit: (side_p >= 0) != (side_q >= 0), den^2 > 1e-20 e.e (|d| = 1),
//              t >= 0; only the polygon's nvert vertices.  A vertex's side is computed from that vertex alone, so the two edges that meet in it read
//              the SAME number and exactly one of them is crossed where the boundary passes through the line: no gap at a vertex, at a repeated
//              vertex (a zero-length edge has den = 0) or between two vertices 1e-13 m apart.  (Before, each edge tested 0 <= s <= 1 with its own
//              quotient s = side_p / den and skipped |den| <= 1e-12: both tests could fail at a shared vertex, and the beam went through the corner
//              of a closed polygon.)  The guard on den is relative: it skips an edge that lies ALONG the beam's line, |sin| of the angle between them
//              <= 1e-10.  There both sides and den are rounding noise (4e-16 relative) and t would be noise over noise - a return at 0 m on a beam
//              that points away from the edge.  The edge's neighbours, which cross the line at an angle, carry its end points.  A beam that meets an
//              edge that flat is a silhouette beam (its range moves by metres under 1e-9 rad), so the guard opens no gap for a conditioned beam.
//              Held to exact rational ray casting by tests/ray_exact.py on the grid of tests/ray_grid.py
//   range      clip(min(range_max, all hits), range_min, range_max); an empty world: range_max everywhere
// One launch for the fleet: blockIdx.y = the member, a thread per beam, RAY_NT beams (one wave) per workgroup, so B * ceil(n_beams / 64) workgroups - 1088
// at 64 members x 1080 beams.  The member's world goes through LDS in tiles of RAY_TILE obstacles; every lane reads the same obstacle at the same time
// (broadcast reads, no bank conflict).  The minimum over obstacles is exact, its order free.  The obstacles are not split over workgroups: at the sizes
// this is for (B >= 16, >= 360 beams) the beams alone give 96 .. 1088 waves, and a split would cost an initialising launch and atomics on the ranges.
struct Ray {                  // per member
    const double *geom;       // [n][E][2] the member's world: polygon vertices | circle: centre, (radius, -)
    const int *kind, *nvert;  // [n] 0 polygon, 1 circle | polygon vertex count (3 .. E)
    int n, E;
    int n_beams, pad;
    double angle_min, angle_max, range_min, range_max;
    double *ranges;           // [n_beams] device memory
};
constexpr int RAY_NT = 64, RAY_TILE = 32;

// one beam (origin o, direction d) against a circle g = centre, (radius, -) | against the polygon edge p -> q: `rng` becomes the hit's range when it is nearer
__device__ __forceinline__ void ray_circle(const double ox, const double oy, const double dx, const double dy, const double *g, double &rng)
{
#pragma clang fp contract(off)
    const double fx = ox - g[0], fy = oy - g[1];
    const double bq = dx * fx + dy * fy;
    const double disc = bq * bq - ((fx * fx + fy * fy) - g[2] * g[2]);
    if (disc >= 0) { const double t = -bq - sqrt(disc); if (t >= 0 && t < rng) rng = t; }
}
__device__ __forceinline__ void ray_edge(const double ox, const double oy, const double dx, const double dy, const double px, const double py,
                                         const double qx, const double qy, double &rng)
{
#pragma clang fp contract(off)
    const double ex = qx - px, ey = qy - py;
    const double den = dx * ey - dy * ex;
    const double wx = px - ox, wy = py - oy, ux = qx - ox, uy = qy - oy;
    const double side_p = wx * dy - wy * dx, side_q = ux * dy - uy * dx;
    if ((side_p >= 0) != (side_q >= 0) && den * den > 1e-20 * (ex * ex + ey * ey)) {
        const double t = (wx * ey - wy * ex) / den;
        if (t >= 0 && t < rng) rng = t;
    }
}
// the member's direction of beam b (live beams only) and its world, tile by tile through tg / tk / tv: the part the two ray casters share.  Every barrier is
// reached by the whole workgroup; returns min(range_max, world hits)
__device__ __forceinline__ double ray_world(const Ray &r, const int E, const bool live, const double ox, const double oy, const double dx, const double dy,
                                            double *tg, int *tk, int *tv)
{
    double rng = r.range_max;
    for (int o0 = 0; o0 < r.n; o0 += RAY_TILE) {
        const int m = r.n - o0 < RAY_TILE ? r.n - o0 : RAY_TILE;
        __syncthreads();                                                                 // (the tile before this one has been read)
        for (int w = threadIdx.x; w < m * E * 2; w += RAY_NT) tg[w] = r.geom[(size_t)o0 * E * 2 + w];
        for (int w = threadIdx.x; w < m; w += RAY_NT) { tk[w] = r.kind[o0 + w]; tv[w] = r.nvert[o0 + w]; }
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < m; ++j) {
            const double *g = tg + j * E * 2;
            if (tk[j] == 1) { ray_circle(ox, oy, dx, dy, g, rng); continue; }
            const int nv = tv[j] < E ? tv[j] : E;
            for (int k = 0; k < nv; ++k) {
                const int k1 = k + 1 < nv ? k + 1 : 0;
                ray_edge(ox, oy, dx, dy, g[2 * k], g[2 * k + 1], g[2 * k1], g[2 * k1 + 1], rng);
            }
        }
    }
    return rng;
}
__device__ __forceinline__ void ray_direction(const Ray &r, const int b, const double heading, double &dx, double &dy)
{
#pragma clang fp contract(off)
    const int nb = r.n_beams;
    const double step = nb > 1 ? (r.angle_max - r.angle_min) / (double)(nb - 1) : 0.0;
    const double ang = (nb > 1 && b == nb - 1) ? r.angle_max : (double)b * step + r.angle_min;
    const double th = heading + ang;
    dx = cos(th); dy = sin(th);
}

__global__ __launch_bounds__(RAY_NT) void k_raycast_fleet(const Ray *rs, const double *poses)
{
#pragma clang fp contract(off)        // numpy does not fuse: keep every product and sum separately rounded
    __shared__ double tg[RAY_TILE * RDA_EMAX * 2];
    __shared__ int tk[RAY_TILE], tv[RAY_TILE];
    const Ray r = rs[blockIdx.y];
    const int nb = r.n_beams, E = r.E < RDA_EMAX ? r.E : RDA_EMAX;
    if ((int)(blockIdx.x * RAY_NT) >= nb) return;                                        // (the whole workgroup: the grid is sized by the longest scan)
    const int b = blockIdx.x * RAY_NT + threadIdx.x;
    const bool live = b < nb;
    const double ox = poses[3 * blockIdx.y], oy = poses[3 * blockIdx.y + 1];
    double dx = 1.0, dy = 0.0;
    if (live) ray_direction(r, b, poses[3 * blockIdx.y + 2], dx, dy);
    const double rng = ray_world(r, E, live, ox, oy, dx, dy, tg, tk, tv);
    if (live) r.ranges[b] = fmin(fmax(rng, r.range_min), r.range_max);                   // np.clip
}

// The sensor that also sees the other MEMBERS (rda_fleet_raycast_peers, rda_fleet_rollout_lidar_peers): k_raycast_fleet - same grid, same beam rule, same
// world loop - and behind the world the footprints of the members j != i at the poses of the same array, as polygons of ps[j].R vertices
// (scenarios.peer_footprints is the specification: robot_vertices(cars[j], states[j]), ascending j).  The B - 1 peers go through LDS in tiles of RAY_TILE:
// for a tile, lane w < m takes peer row p0 + w (row r is member j = r < i ? r : r + 1, the mapping of scene::k_peers_fleet), computes cos / sin of that ONE
// heading and writes the R vertices with k_peers_fleet's expressions, (co rv.x - si rv.y) + x | (si rv.x + co rv.y) + y, at a stride of RDA_RMAX vertices;
// then every beam runs ray_edge over the R edges of each footprint, all lanes on the same vertex (broadcast reads).  So the trigonometry costs one cos / sin
// pair per peer and workgroup, never per beam.  A member does not see itself; a peer that contains the origin is hit from the inside like any polygon.  The
// minimum over world and peers is exact, its order free.  The lane that owns a peer also drops it when it is out of reach - centre farther from the origin
// than range_max plus the footprint's radius, so no hit of it can lower the minimum: the result is the same bit for bit, and a beam pays the edge tests
// (two side values each and a double division where the edge is crossed) only for the members its lidar can reach, not for all B - 1.
// LDS: the peer tile reuses the world tile's block (the world has been read when the first peer tile is written), so the launch costs what k_raycast_fleet's
// does, 32 * 8 * 2 doubles + 2 * 32 ints = 4352 B per workgroup of one wave: 32 resident workgroups (the wave limit of a CU) hold 136 KiB of its 160 KiB, the
// LDS does not bound the occupancy.  Workgroups: B * ceil(n_beams / 64), 1088 at 64 members x 1080 beams, as many as the blind caster; each tests
// at most 63 * 4 peer edges per beam besides the world's (all members within reach of each other).
static_assert(RDA_RMAX <= RDA_EMAX, "a peer tile lies in the world tile's block");
__global__ __launch_bounds__(RAY_NT) void k_raycast_fleet_peers(const Ray *rs, const scene::Peer *ps, const double *poses, int B)
{
#pragma clang fp contract(off)
    __shared__ double tg[RAY_TILE * RDA_EMAX * 2];
    __shared__ int tk[RAY_TILE], tv[RAY_TILE];
    const int i = blockIdx.y;
    const Ray r = rs[i];
    const int nb = r.n_beams, E = r.E < RDA_EMAX ? r.E : RDA_EMAX;
    if ((int)(blockIdx.x * RAY_NT) >= nb) return;                                        // (the whole workgroup)
    const int b = blockIdx.x * RAY_NT + threadIdx.x;
    const bool live = b < nb;
    const double ox = poses[3 * i], oy = poses[3 * i + 1];
    double dx = 1.0, dy = 0.0;
    if (live) ray_direction(r, b, poses[3 * i + 2], dx, dy);
    double rng = ray_world(r, E, live, ox, oy, dx, dy, tg, tk, tv);
    for (int p0 = 0; p0 < B - 1; p0 += RAY_TILE) {
        const int m = B - 1 - p0 < RAY_TILE ? B - 1 - p0 : RAY_TILE;
        __syncthreads();                                                                 // (the world's last tile | the peer tile before this one has been read)
        if ((int)threadIdx.x < m) {
            const int row = p0 + threadIdx.x, j = row < i ? row : row + 1;
            const scene::Peer &p = ps[j];
            const int R = p.R < RDA_RMAX ? p.R : RDA_RMAX;
            const double x = poses[3 * j], y = poses[3 * j + 1], th = poses[3 * j + 2];
            // out of reach: every point of the footprint lies within rad of (x, y), so a hit is at least |p_j - o| - rad away; beyond range_max it
            // cannot lower min(range_max, ...) (the margin of 1e-6 relative stands for the rounding of these few operations)
            double rad2 = 0.0;
            for (int v = 0; v < R; ++v) rad2 = fmax(rad2, p.rv[v][0] * p.rv[v][0] + p.rv[v][1] * p.rv[v][1]);
            const double reach = (r.range_max + sqrt(rad2)) * 1.000001, cx = x - ox, cy = y - oy;
            const bool near_enough = !(cx * cx + cy * cy > reach * reach);                  // (a NaN pose is kept: the edge tests then hit nothing, as before)
            if (near_enough) {
                const double co = cos(th), si = sin(th);
                double *g = tg + threadIdx.x * RDA_RMAX * 2;
                for (int v = 0; v < R; ++v) {
                    g[2 * v] = (co * p.rv[v][0] - si * p.rv[v][1]) + x;
                    g[2 * v + 1] = (si * p.rv[v][0] + co * p.rv[v][1]) + y;
                }
            }
            tv[threadIdx.x] = near_enough ? R : 0;
        }
        __syncthreads();
        if (!live) continue;
        for (int q = 0; q < m; ++q) {
            const double *g = tg + q * RDA_RMAX * 2;
            const int nv = tv[q];
            for (int k = 0; k < nv; ++k) {
                const int k1 = k + 1 < nv ? k + 1 : 0;
                ray_edge(ox, oy, dx, dy, g[2 * k], g[2 * k + 1], g[2 * k1], g[2 * k1 + 1], rng);
            }
        }
    }
    if (live) r.ranges[b] = fmin(fmax(rng, r.range_min), r.range_max);                   // np.clip
}

// the boxes as a raw scene in the layout scene_stage uploads (rda_hip.hip): polygons of 4 vertices, no velocity, the robot position for the ordering
__global__ void k_scene_fill(const double *boxes, const int n, const int E, double *geom, double *vel, double *robot, int *nonconvex, int *kind, int *nvert,
                             const double rx, const double ry)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { robot[0] = rx; robot[1] = ry; *nonconvex = 0; }
    if (i >= n) return;
    double *g = geom + (size_t)i * E * 2;
    for (int e = 0; e < E; ++e) { g[2 * e] = e < 4 ? boxes[(size_t)i * 8 + 2 * e] : 0.0; g[2 * e + 1] = e < 4 ? boxes[(size_t)i * 8 + 2 * e + 1] : 0.0; }
    vel[2 * i] = 0.0; vel[2 * i + 1] = 0.0;
    kind[i] = 0; nvert[i] = 4;
}


// k_scene_fill for every member of a fleet in one launch (blockIdx.y = the member; n = 0: a member without boxes, nothing is written)
struct Fill {
    const double *boxes; int n, E;
    double *geom, *vel, *robot; int *nonconvex, *kind, *nvert;
    double rx, ry;
    const double *rob;        // (may be null) the robot position [2] in device memory, taken instead of rx, ry (rda_fleet_rollout_lidar: where the advance kernel wrote it)
    const double *vel_in;     // (may be null: zeros) the boxes' velocities [n][2] in device memory, where k_track_boxes_fleet wrote them
};
__global__ void k_scene_fill_fleet(const Fill *fs)
{
    const Fill f = fs[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (f.n <= 0) return;
    if (i == 0) { f.robot[0] = f.rob ? f.rob[0] : f.rx; f.robot[1] = f.rob ? f.rob[1] : f.ry; *f.nonconvex = 0; }
    if (i >= f.n) return;
    double *g = f.geom + (size_t)i * f.E * 2;
    for (int e = 0; e < f.E; ++e) { g[2 * e] = e < 4 ? f.boxes[(size_t)i * 8 + 2 * e] : 0.0; g[2 * e + 1] = e < 4 ? f.boxes[(size_t)i * 8 + 2 * e + 1] : 0.0; }
    f.vel[2 * i] = f.vel_in ? f.vel_in[2 * i] : 0.0; f.vel[2 * i + 1] = f.vel_in ? f.vel_in[2 * i + 1] : 0.0;
    f.kind[i] = 0; f.nvert[i] = 4;
}

// Boxes tracked from tick to tick (rda_fleet_upload_scans_tracked, rda_fleet_rollout_lidar_tracked, rda_fleet_track_boxes): a velocity for every box of
// this tick's scan from a resident table of tracks per member.  The specification is lidar.track_boxes (rda_planner_amd/lidar.py), expression by expression
// (FMA contraction off; only +, -, * and / on doubles occur), so velocities and table are bit-identical to it on the same boxes:
//   centre       (((x0 + x1) + x2) + x3) * 0.25 per coordinate, the corners in the order scan_body writes them
//   which boxes  the first m = min(n, MAX_TRACKS); the others get velocity 0 and leave no track
//   association  mutual nearest neighbour on d2 = dx * dx + dy * dy against the previous tracks' positions: fwd[i] = the lowest j at the minimum of row i,
//                back[j] = the lowest i at the minimum of column j; box i continues track j = fwd[i] iff back[j] == i and d2 <= gate * gate.  Independent of
//                the order of the boxes, which follows the cluster order and changes from tick to tick
//   continued    history h (oldest first, len entries): v = (c - h[0]) / (dt * len), the new history (h + [c])[-window:].  The difference over the track's
//                AGE, not over one tick: beam spacing / dt puts 2 - 3 m/s of noise on a one-tick difference
//   otherwise    v = 0, history [c]; tracks nobody continues end; the new table holds track i = box i, count m
// One workgroup of TRK_NT = MAX_TRACKS threads per member (blockIdx.x), one launch whatever B is.  The table is double-buffered: buffer `par` is read, buffer
// par ^ 1 written, so no thread overwrites what another still reads and a caller that gives up the tick keeps the old table by not switching.  LDS: the new
// centres and the previous positions (both at most MAX_TRACKS, so the previous positions are one tile), the two index arrays - 4 * 256 doubles + 2 * 256 ints
// = 10 KiB; every lane of a wave reads the same opposite entry at the same time (broadcast reads, no bank conflict).  Thread t serves box t in the row phase
// and previous track t in the column phase; every barrier is reached by the whole workgroup.  The box count is read from where the scan kernel wrote it
// (pinned host memory, the same stream: the launch sits behind the scan and in front of the tick's wait for the counts).
constexpr int MAX_TRACKS = 256, TRK_HIST = 8, TRK_NT = MAX_TRACKS;
struct Track {                // per member
    const double *boxes;      // [n][4][2] this tick's boxes (device memory)
    const int *count;         // [0] = n, where the scan kernel wrote it
    int *cnt[2];              // [1] tracks in the table, per buffer
    int *len[2];              // [MAX_TRACKS] entries of every track's history
    double *hist[2];          // [MAX_TRACKS][TRK_HIST][2] oldest first
    double *tvel[2];          // [MAX_TRACKS][2] the velocity the track's box got (rda_fleet_box_tracks)
    double *vel;              // [MAXB][2] every box's velocity, what k_scene_fill_fleet reads
    double dt;                // the member's sample time: successive launches are taken to be dt apart
};
__global__ __launch_bounds__(TRK_NT) void k_track_boxes_fleet(const Track *ts, const int par, const double gate, const int window)
{
#pragma clang fp contract(off)        // numpy does not fuse: keep every product and sum separately rounded
    __shared__ double cx[MAX_TRACKS], cy[MAX_TRACKS], qx[MAX_TRACKS], qy[MAX_TRACKS];
    __shared__ int fwd[MAX_TRACKS], back[MAX_TRACKS];
    const Track t = ts[blockIdx.x];
    const int tid = threadIdx.x;
    int n = *(const volatile int *)t.count, np = *t.cnt[par];
    n = n < 0 ? 0 : (n > MAXB ? MAXB : n);
    np = np < 0 ? 0 : (np > MAX_TRACKS ? MAX_TRACKS : np);
    const int m = n < MAX_TRACKS ? n : MAX_TRACKS;
    const int *plen = t.len[par]; const double *ph = t.hist[par];
    if (tid < m) {
        const double *b = t.boxes + (size_t)tid * 8;
        cx[tid] = (((b[0] + b[2]) + b[4]) + b[6]) * 0.25;
        cy[tid] = (((b[1] + b[3]) + b[5]) + b[7]) * 0.25;
    }
    int hl = 0;
    if (tid < np) {
        hl = plen[tid]; hl = hl < 1 ? 1 : (hl > TRK_HIST ? TRK_HIST : hl);
        qx[tid] = ph[((size_t)tid * TRK_HIST + hl - 1) * 2]; qy[tid] = ph[((size_t)tid * TRK_HIST + hl - 1) * 2 + 1];
    }
    __syncthreads();
    double best = 0.0;
    if (tid < m) {                                   // row tid: the nearest previous track
        int bj = -1;
        const double x = cx[tid], y = cy[tid];
        for (int j = 0; j < np; ++j) {
            const double dx = x - qx[j], dy = y - qy[j], d2 = dx * dx + dy * dy;
            if (bj < 0 || d2 < best) { best = d2; bj = j; }
        }
        fwd[tid] = bj;
    }
    if (tid < np) {                                  // column tid: the nearest new box
        int bi = -1; double bd = 0.0;
        const double x = qx[tid], y = qy[tid];
        for (int i = 0; i < m; ++i) {
            const double dx = cx[i] - x, dy = cy[i] - y, d2 = dx * dx + dy * dy;
            if (bi < 0 || d2 < bd) { bd = d2; bi = i; }
        }
        back[tid] = bi;
    }
    __syncthreads();
    int *nlen = t.len[par ^ 1]; double *nh = t.hist[par ^ 1], *nv = t.tvel[par ^ 1];
    if (tid < m) {
        const int j = fwd[tid];
        const double x = cx[tid], y = cy[tid];
        double vx = 0.0, vy = 0.0;
        double *h = nh + (size_t)tid * TRK_HIST * 2;
        int l = 0;
        if (j >= 0 && back[j] == tid && best <= gate * gate) {
            int pl = plen[j]; pl = pl < 1 ? 1 : (pl > TRK_HIST ? TRK_HIST : pl);
            const double *o = ph + (size_t)j * TRK_HIST * 2;
            const double span = t.dt * (double)pl;
            vx = (x - o[0]) / span; vy = (y - o[1]) / span;
            const int from = pl + 1 > window ? pl + 1 - window : 0;        // (h + [c])[-window:]
            for (int k = from; k < pl; ++k) { h[2 * l] = o[2 * k]; h[2 * l + 1] = o[2 * k + 1]; ++l; }
        }
        h[2 * l] = x; h[2 * l + 1] = y;
        nlen[tid] = l + 1;
        nv[2 * tid] = vx; nv[2 * tid + 1] = vy;
        t.vel[2 * tid] = vx; t.vel[2 * tid + 1] = vy;
    }
    for (int i = MAX_TRACKS + tid; i < n; i += TRK_NT) { t.vel[2 * i] = 0.0; t.vel[2 * i + 1] = 0.0; }
    if (tid == 0) *t.cnt[par ^ 1] = m;
}

}  // namespace lidar
