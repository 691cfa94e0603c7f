// TEST INFRASTRUCTURE: the LamMuZ launch plans of rda_planner_amd/csrc/lmz_plan.h behind a C interface - the two rules and the name function the
// library itself calls, compiled without HIP (tests/test_lmz_plan.py).  Built by the test with g++ into tests/emu/_build/.
#include <cstring>
#include "../../rda_planner_amd/csrc/lmz_plan.h"

static_assert(sizeof(lmzplan::Member) == 12 * sizeof(int), "a member is 12 ints, in the order of the struct");

// n, then (kernel, grid, block) per launch: 10 ints
static int plan_out(const lmzplan::Plan &p, int *out)
{
    out[0] = p.n;
    for (int i = 0; i < p.n; ++i) { out[1 + 3 * i] = p.l[i].kernel; out[2 + 3 * i] = p.l[i].grid; out[3 + 3 * i] = p.l[i].block; }
    return p.n;
}

extern "C" {
// the kernel id of a role, -1: no such role
int lmz_plan_emu_kernel(const char *role)
{
    static const struct { const char *role; lmzplan::Kernel k; } ids[] = {
        { "rows", lmzplan::ROWS }, { "rows_dense", lmzplan::ROWS_DENSE }, { "rows_fast", lmzplan::ROWS_FAST }, { "enum", lmzplan::ENUM },
        { "wave", lmzplan::WAVE }, { "ip", lmzplan::IP }, { "cp_small", lmzplan::CP_SMALL }, { "cp_large", lmzplan::CP_LARGE },
        { "finalize", lmzplan::FINALIZE } };
    for (const auto &e : ids) if (!strcmp(e.role, role)) return e.k;
    return -1;
}
int lmz_plan_emu_solo(const lmzplan::Member *m, int *out) { return plan_out(lmzplan::solo(*m), out); }
int lmz_plan_emu_fleet(const lmzplan::Member *m, int B, int *out) { return plan_out(lmzplan::fleet(B, [m](int i) { return m[i]; }), out); }
// the joined name of a plan as plan_out wrote it
void lmz_plan_emu_name(const int *plan, int fleet, char *buf, int cap)
{
    lmzplan::Plan p;
    for (int i = 0; i < plan[0]; ++i) p.then((lmzplan::Kernel)plan[1 + 3 * i], plan[2 + 3 * i], plan[3 + 3 * i]);
    lmzplan::name(p, fleet != 0, buf, (size_t)cap);
}
}
