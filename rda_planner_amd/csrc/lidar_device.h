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
    if (a.labels_h) {
        int o = first;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int b = tid * PER + k;
            if (b < nb) a.labels_h[b] = hit[k] ? ic[o] : -2;
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
//   edge p->q  e = q - p, w = p - o, den = d.x e.y - d.y e.x, t = (w.x e.y - w.y e.x) / den, s = (w.x d.y - w.y d.x) / den;
//              a hit: |den| > 1e-12, t >= 0, 0 <= s <= 1; only the polygon's nvert vertices
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
    if (live) {
        const double step = nb > 1 ? (r.angle_max - r.angle_min) / (double)(nb - 1) : 0.0;
        const double ang = (nb > 1 && b == nb - 1) ? r.angle_max : (double)b * step + r.angle_min;
        const double th = poses[3 * blockIdx.y + 2] + ang;
        dx = cos(th); dy = sin(th);
    }
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
            if (tk[j] == 1) {
                const double fx = ox - g[0], fy = oy - g[1];
                const double bq = dx * fx + dy * fy;
                const double disc = bq * bq - ((fx * fx + fy * fy) - g[2] * g[2]);
                if (disc >= 0) { const double t = -bq - sqrt(disc); if (t >= 0 && t < rng) rng = t; }
                continue;
            }
            const int nv = tv[j] < E ? tv[j] : E;
            for (int k = 0; k < nv; ++k) {
                const int k1 = k + 1 < nv ? k + 1 : 0;
                const double px = g[2 * k], py = g[2 * k + 1];
                const double ex = g[2 * k1] - px, ey = g[2 * k1 + 1] - py;
                const double den = dx * ey - dy * ex;
                const double wx = px - ox, wy = py - oy;
                const double t = (wx * ey - wy * ex) / den, s = (wx * dy - wy * dx) / den;
                if (fabs(den) > 1e-12 && t >= 0 && s >= 0 && s <= 1 && t < rng) rng = t;
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
    f.vel[2 * i] = 0.0; f.vel[2 * i + 1] = 0.0;
    f.kind[i] = 0; f.nvert[i] = 4;
}

}  // namespace lidar
