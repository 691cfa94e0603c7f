"""The LamMuZ launch plans (rda_planner_amd/csrc/lmz_plan.h): which kernels a step launches per ADMM iteration, on what grids, and the name the library
reports for them.  The header is plain C++, so the very rules and name function that librda_hip.so calls are compiled here with g++
(tests/emu/lmz_plan_emu.cpp) and held to literal grids: 8 slots per block partial, packed workgroups of 128 threads, 32 block partials per finalize
workgroup, packed grid 8 ceil(T J / 8).  Launches are (kernel role, grid.x, block.x) in issue order; a fleet's grid.y = B is the executor's."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("T", "N", "J", "E", "R", "nt", "obstacle_num", "rows", "lmz_mode", "ip_rows", "lmz_dense_from", "lmz_split")      # lmzplan::Member


@pytest.fixture(scope="module")
def emu():
    src, out = os.path.join(HERE, "emu", "lmz_plan_emu.cpp"), os.path.join(HERE, "emu", "_build", "liblmz_plan_emu.so")
    hdr = os.path.join(HERE, "..", "rda_planner_amd", "csrc", "lmz_plan.h")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", out, src])
    return C.CDLL(out)                  # (int arrays, ints and byte strings in, int out: ctypes' default conversions)


def member(T=10, N=24, **kw):
    """a member with all N slots staged (one time slot), enumeration mode, library defaults; J follows N"""
    m = dict(T=T, N=N, J=(N + 7) // 8, E=4, R=4, nt=1, obstacle_num=N, rows=1, lmz_mode=0, ip_rows=0, lmz_dense_from=256, lmz_split=1)
    assert set(kw) <= set(m), kw
    m.update(kw)
    return [m[f] for f in FIELDS]


def plan_of(emu, members, fleet):
    """([(role, grid, block), ...], joined name) of one member (solo rule) or a list of members (fleet rule)"""
    flat = [v for m in members for v in m]
    arr, out = (C.c_int * len(flat))(*flat), (C.c_int * 10)()
    n = emu.lmz_plan_emu_fleet(arr, len(members), out) if fleet else emu.lmz_plan_emu_solo(arr, out)
    assert 1 <= n <= 3 and out[0] == n
    roles = {emu.lmz_plan_emu_kernel(r.encode()): r for r in ("rows", "rows_dense", "rows_fast", "enum", "wave", "ip", "cp_small", "cp_large", "finalize")}
    assert len(roles) == 9 and -1 not in roles
    buf = C.create_string_buffer(96)
    emu.lmz_plan_emu_name(out, int(fleet), buf, len(buf))
    return [(roles[out[1 + 3 * i]], out[2 + 3 * i], out[3 + 3 * i]) for i in range(n)], buf.value.decode()


IP = dict(lmz_mode=1, ip_rows=1)
CP = dict(lmz_mode=1, ip_rows=0)
FIN1 = ("finalize", 1, 256)

SOLO = {
    "rows": (member(), [("rows", 32, 128)], "k_lammuz_rows"),
    "rows_off": (member(rows=0), [("wave", 60, 256), FIN1], "k_lammuz+k_lmz_finalize"),
    "nothing_staged": (member(obstacle_num=0), [("wave", 1, 256), FIN1], "k_lammuz+k_lmz_finalize"),
    "ip_rows": (member(**IP), [("ip", 32, 128)], "k_lammuz_ip"),
    "cp_large": (member(E=8, **CP), [("cp_large", 4, 64), FIN1], "k_lammuz_cp_large+k_lmz_finalize"),
    "cp_large_nothing_staged": (member(E=8, obstacle_num=0, **CP), [("cp_large", 1, 64), FIN1], "k_lammuz_cp_large+k_lmz_finalize"),
    "cp_small": (member(E=4, R=4, **CP), [("cp_small", 4, 64), FIN1], "k_lammuz_cp_small+k_lmz_finalize"),
    "cp_small_nothing_staged": (member(E=4, R=4, obstacle_num=0, **CP), [("cp_small", 1, 64), FIN1], "k_lammuz_cp_small+k_lmz_finalize"),
    # the lower clamp of the work list
    "dense_from_1": (member(lmz_dense_from=1), [("rows_fast", 32, 128), ("enum", 64, 128), FIN1], "k_lammuz_rows_fast+k_lammuz_enum+k_lmz_finalize"),
    # around the dense threshold: 250 and 260 CUs against 256
    "below_threshold": (member(20, 200), [("rows", 504, 128)], "k_lammuz_rows"),
    "above_threshold": (member(20, 208), [("rows_fast", 520, 128), ("enum", 130, 128), ("finalize", 17, 256)], "k_lammuz_rows_fast+k_lammuz_enum+k_lmz_finalize"),
    "above_threshold_no_split": (member(20, 208, lmz_split=0), [("rows_dense", 520, 128)], "k_lammuz_rows_dense"),
    "above_threshold_moving": (member(20, 208, nt=21), [("rows", 520, 128)], "k_lammuz_rows"),          # moving threshold 448
}

SPLIT = "k_lammuz_fleet_rows_fast+k_lammuz_fleet_enum+k_lmz_finalize_fleet"
FLEET = {
    "rows_split": ([member(), member()], [("rows_fast", 32, 128), ("enum", 8, 128), FIN1], SPLIT),
    "one_member_no_split": ([member(), member(lmz_split=0)], [("rows", 32, 128)], "k_lammuz_fleet_rows"),
    "one_member_nothing_staged": ([member(obstacle_num=0), member()], [("wave", 60, 256), FIN1], "k_lammuz_fleet+k_lmz_finalize_fleet"),
    "one_member_rows_off": ([member(), member(rows=0)], [("wave", 60, 256), FIN1], "k_lammuz_fleet+k_lmz_finalize_fleet"),
    "ip_all_rows": ([member(**IP), member(**IP)], [("ip", 32, 128)], "k_lammuz_ip_fleet"),
    "ip_no_rows": ([member(**CP), member(**CP)], [("cp_small", 4, 64), FIN1], "k_lammuz_cp_fleet_small+k_lmz_finalize_fleet"),
    "ip_mixed": ([member(**IP), member(obstacle_num=0, **IP)], [("ip", 32, 128), ("cp_small", 4, 64), FIN1],
                 "k_lammuz_ip_fleet+k_lammuz_cp_fleet_small+k_lmz_finalize_fleet"),
    "ip_mixed_large": ([member(E=8, obstacle_num=0, **IP), member(E=8, **IP)], [("ip", 32, 128), ("cp_large", 4, 64), FIN1],
                       "k_lammuz_ip_fleet+k_lammuz_cp_fleet_large+k_lmz_finalize_fleet"),
    # the fleet's own clamp of the work-list grid (T J / 8 in 8 .. 128), and no dense threshold
    "worklist_62": ([member(20, 200), member(20, 200)], [("rows_fast", 504, 128), ("enum", 62, 128), ("finalize", 16, 256)], SPLIT),
    "worklist_clamped": ([member(30, 400), member(30, 400)], [("rows_fast", 1504, 128), ("enum", 128, 128), ("finalize", 47, 256)], SPLIT),
}


@pytest.mark.parametrize("case", list(SOLO))
def test_solo_plan_has_these_launches_and_this_name(emu, case):
    m, launches, name = SOLO[case]
    assert plan_of(emu, [m], fleet=False) == (launches, name)


@pytest.mark.parametrize("case", list(FLEET))
def test_fleet_plan_has_these_launches_and_this_name(emu, case):
    members, launches, name = FLEET[case]
    assert plan_of(emu, members, fleet=True) == (launches, name)
