// The LamMuZ launches of one ADMM iteration as data: which kernels, in which order, on what grid.  A rule (solo: one handle; fleet: B members, the
// member in blockIdx.y) turns plain ints into a Plan; rda_hip.hip executes a plan launch by launch (launch_lammuz, fleet_enqueue) and reports its name
// (rda_lammuz_kernel, rda_fleet_lammuz_kernel) - both from this record, so the name a caller reads is the list of kernels that run.
// Plain C++17 without HIP types: tests/emu/lmz_plan_emu.cpp compiles the rules with g++ and tests/test_lmz_plan.py pins their grids and names.
#pragma once
#include <cstddef>
#include <cstdio>

#if defined(__HIPCC__)
#define LMZ_PLAN_HD __host__ __device__
#else
#define LMZ_PLAN_HD
#endif

namespace lmzplan {

constexpr int GS = 8;                  // slots per block partial = rows of a packed workgroup (su::GS)
constexpr int NTH = 64 * GS / 4;       // threads of a packed workgroup (2 waves)
constexpr int FPB = 256 / GS;          // block partials per workgroup of k_lmz_finalize
// workgroups of a packed launch: one per (stage, GS-slot block), rounded up to whole rounds of the 8 XCDs (block_of in rda_hip.hip; the rest are fillers)
LMZ_PLAN_HD inline int packed_grid(int T, int J) { return 8 * ((T * J + 7) / 8); }

// one id per kernel role; the solo kernel and its fleet twin (null: the fleet has none)
enum Kernel { ROWS, ROWS_DENSE, ROWS_FAST, ENUM, WAVE, IP, CP_SMALL, CP_LARGE, FINALIZE };
struct Names { const char *solo, *fleet; };
constexpr Names NAMES[FINALIZE + 1] = {
    { "k_lammuz_rows", "k_lammuz_fleet_rows" },
    { "k_lammuz_rows_dense", nullptr },
    { "k_lammuz_rows_fast", "k_lammuz_fleet_rows_fast" },
    { "k_lammuz_enum", "k_lammuz_fleet_enum" },
    { "k_lammuz", "k_lammuz_fleet" },
    { "k_lammuz_ip", "k_lammuz_ip_fleet" },
    { "k_lammuz_cp_small", "k_lammuz_cp_fleet_small" },
    { "k_lammuz_cp_large", "k_lammuz_cp_fleet_large" },
    { "k_lmz_finalize", "k_lmz_finalize_fleet" },
};
// (for the executors' static_asserts: the name in the table is the kernel symbol the id's case launches)
constexpr bool same(const char *a, const char *b) { while (*a && *a == *b) { ++a; ++b; } return *a == *b; }

struct Launch { Kernel kernel; int grid, block; };      // grid.x and block.x (the fleet executor adds grid.y = B)
struct Plan {                                            // at most three launches, in issue order
    int n = 0; Launch l[3] = {};
    Plan &then(Kernel k, int grid, int block) { l[n++] = Launch{ k, grid, block }; return *this; }
};
constexpr size_t NAME_CAP = 96;                          // the longest joined name (three fleet kernels) has 62 characters
// the plan's kernel names joined by '+'
inline void name(const Plan &p, bool fleet, char *buf, size_t cap)
{
    size_t at = 0;
    if (cap) buf[0] = 0;
    for (int i = 0; i < p.n && at < cap; ++i) {
        const Names &k = NAMES[p.l[i].kernel];
        const int w = snprintf(buf + at, cap - at, "%s%s", i ? "+" : "", fleet ? k.fleet : k.solo);
        if (w < 0) break;
        at += (size_t)w;
    }
}

// What the rules read of a handle / fleet member.  N: the slots this rank solves (Dev::Nlive; a fleet member is no shard: all of them), J: its GS-slot
// blocks per stage; ip_rows: Dev::ip_rows (interior-point mode and the row-parallel kernel takes the shape)
struct Member { int T, N, J, E, R, nt, obstacle_num, rows, lmz_mode, ip_rows, lmz_dense_from, lmz_split; };

// THE statement of "this member runs the row-parallel interior-point kernel" (else the per-thread kernel, with its quirk-Q9 branch, + the finalize
// kernel): host rules and fleet kernels alike, on a Member or on the device record
template <class M> LMZ_PLAN_HD inline bool member_ip_rows(const M &m) { return m.ip_rows && m.obstacle_num; }

inline int finalize_grid(const Member &m) { return (m.T * m.J + FPB - 1) / FPB; }       // k_lmz_finalize: block partials and the tail of the forms that do not make them
inline Kernel cp_kernel(const Member &m) { return (m.E <= 4 && m.R <= 4) ? CP_SMALL : CP_LARGE; }

// One handle.  Packed rows when the shape allows: a small grid is ONE launch that also forms the block partials; a dense grid is the common-path kernel
// + the work-list kernel, with k_lmz_finalize (partials) behind them.  One sub-problem per wave (big shapes, the no-obstacle case of quirk Q9) and the
// per-thread interior-point kernel likewise end with k_lmz_finalize.
inline Plan solo(const Member &m)
{
    const int units = m.T * GS * m.J;            // rows of the grid (a stage is padded to whole GS-slot blocks)
    Plan p;
    if (m.lmz_mode) {
        if (member_ip_rows(m)) return p.then(IP, packed_grid(m.T, m.J), NTH);
        // a thread per (slot, stage); the Q9 branch needs T threads
        return p.then(cp_kernel(m), ((m.obstacle_num ? m.N * m.T : m.T) + 63) / 64, 64).then(FINALIZE, finalize_grid(m), 256);
    }
    if (m.rows && m.obstacle_num) {
        const int nb = packed_grid(m.T, m.J), cus = (units / GS * NTH + 255) / 256;      // launch indices (XCD-aware order, a few fillers); CUs the grid asks for at one wave per SIMD
        // Grid size (in compute units at one wave per SIMD) from which the dense forms are used.  Scenes with per-stage obstacle data
        // (moving obstacles) lose the remembered support of more rows per launch, so the work list of the split form is longer and the
        // single launch stays ahead up to a larger grid: measured cross-over ~280 CUs for static scenes (N = 300, T = 20: 35.7 vs 38.7 us),
        // ~560 for moving ones (T = 30: N = 200 40.9 vs 47.1 us for the single launch, N = 300 52.2 vs 50.1, N = 400 60.7 vs 51.1).
        if (cus <= (m.nt > 1 ? m.lmz_dense_from * 7 / 4 : m.lmz_dense_from)) return p.then(ROWS, nb, NTH);
        if (!m.lmz_split) return p.then(ROWS_DENSE, nb, NTH);
        // dense grid: common path with three waves per SIMD, then the deferred rows one per wave (see lammuz_body_rows)
        int ne = units / 32; if (ne < 64) ne = 64; if (ne > 2048) ne = 2048;
        return p.then(ROWS_FAST, nb, NTH).then(ENUM, ne, NTH).then(FINALIZE, finalize_grid(m), 256);
    }
    return p.then(WAVE, m.obstacle_num ? (units + 3) / 4 : 1, 256).then(FINALIZE, finalize_grid(m), 256);
}

// B members of one shape and one LamMuZ mode (rda_fleet_create) behind one set of launches; at(i): member i as it stands now.  The fleet's own rule,
// not solo's: no dense threshold, and other clamps of the work-list grid - one rule for both would branch on its caller.  Enumeration fleets use the
// packed kernels only when every member can (rows, obstacles staged): the forms agree bit for bit, so the choice is fleet-wide.  Interior-point fleets
// launch only the forms some member needs this tick (member_ip_rows: a kernel of one form returns at once for the members of the other).
template <class At> inline Plan fleet(int B, At at)
{
    const Member m0 = at(0);
    const int nbr = m0.T * m0.J, nbp = packed_grid(m0.T, m0.J);       // one workgroup per (stage, GS-slot block), XCD-aware order
    int rows = 1, split = 1, ip_rows = 0, ip_cp = 0;
    for (int i = 0; i < B; ++i) {
        const Member m = at(i);
        if (!m.lmz_split) split = 0;
        if (!m.rows || !m.obstacle_num) rows = 0;
        if (member_ip_rows(m)) ip_rows = 1; else ip_cp = 1;
    }
    Plan p;
    if (m0.lmz_mode) {
        if (ip_rows) p.then(IP, nbp, NTH);
        if (ip_cp) p.then(cp_kernel(m0), (m0.N * m0.T + 63) / 64, 64).then(FINALIZE, finalize_grid(m0), 256);     // a thread per (slot, stage); the Q9 branch needs T threads
        return p;
    }
    if (rows && split) {
        int ne = nbr / 8; if (ne < 8) ne = 8; if (ne > 128) ne = 128;
        return p.then(ROWS_FAST, nbp, NTH).then(ENUM, ne, NTH).then(FINALIZE, finalize_grid(m0), 256);
    }
    if (rows) return p.then(ROWS, nbp, NTH);
    return p.then(WAVE, nbr * GS / 4, 256).then(FINALIZE, finalize_grid(m0), 256);
}

}  // namespace lmzplan
