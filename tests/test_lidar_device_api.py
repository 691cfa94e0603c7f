"""The device-side lidar front end (rda_scan_boxes / rda_upload_scan) as far as it can be checked without a GPU: the two entry points are
declared, exported and documented, their ctypes prototypes follow the header, and the Python surface (`RDA_solver.scan_boxes` /
`upload_scan`, `lidar.scan_box_device`, `MPC.control(scan=)`) is there and rejects a mixed call before anything reaches a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rda_scan_boxes", "rda_upload_scan")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rda_hip.h")).read(), flags=re.S)


def _declared_args(name):
    """ctypes types of the arguments of `int name(...)` as include/rda_hip.h declares it"""
    from rda_planner_amd._capi import c_double_p, c_int_p
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), re.S)
    assert m, f"{name} is not declared in include/rda_hip.h"
    kinds = {"rda_handle *": C.c_void_p, "int": C.c_int, "double": C.c_double, "const double *": c_double_p, "double *": c_double_p,
             "int32_t *": c_int_p, "const int32_t *": c_int_p}
    out = []
    for arg in m.group(1).split(","):
        typ = re.sub(r"\s+", " ", re.match(r"\s*(.*?)(\w+)\s*$", arg, re.S).group(1)).strip()
        out.append(kinds[typ])
    return out


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_exported_and_documented(name):
    from rda_planner_amd import _lib
    assert re.search(r"\b%s\s*\(" % name, _header())
    assert hasattr(C.CDLL(_lib.build()), name), f"{name} declared in include/rda_hip.h but not exported"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [ln for ln in doc.splitlines() if name in ln]
    assert row and any("lidar_path_track.py:20-60" in ln for ln in row)


@pytest.mark.parametrize("name,nargs", [("rda_scan_boxes", 13), ("rda_upload_scan", 11)])
def test_ctypes_prototype_follows_the_header(name, nargs):
    from rda_planner_amd import _lib
    from rda_planner_amd._capi import CApi
    api = CApi(C.CDLL(_lib.build()), "rda")
    assert api.has_scan
    fn = getattr(api, name[len("rda_"):])
    want = _declared_args(name)
    assert len(want) == nargs
    assert list(fn.argtypes) == want and fn.restype is C.c_int


def test_library_rejects_bad_arguments_without_a_device():
    """the argument rules that need no handle"""
    from rda_planner_amd import _lib
    from rda_planner_amd._capi import CApi, dptr, iptr
    api = CApi(C.CDLL(_lib.build()), "rda")
    r, st, n = np.ones(8), np.zeros(3), np.zeros(1, np.int32)
    assert api.scan_boxes(None, 8, dptr(r), -1.0, 1.0, 10.0, dptr(st), 2.0, 6, iptr(n), None, 0, None) == -1        # RDA_ERR_ARG
    assert api.upload_scan(None, 8, dptr(r), -1.0, 1.0, 10.0, dptr(st), 2.0, 6, 1, None) == -1


def test_python_surface():
    from rda_planner_amd import lidar
    from rda_planner_amd.mpc import MPC
    from rda_planner_amd.rda_solver import RDA_solver
    sig = inspect.signature(lidar.scan_box_device)
    assert list(sig.parameters)[:3] == ["solver", "state", "scan_data"]
    assert sig.parameters["eps"].default == 2.0 and sig.parameters["min_samples"].default == 6
    for meth in (RDA_solver.scan_boxes, RDA_solver.upload_scan):
        p = inspect.signature(meth).parameters
        assert list(p)[1:3] == ["state", "scan_data"] and p["eps"].default == 2.0 and p["min_samples"].default == 6
    p = inspect.signature(MPC.control).parameters
    assert p["scan"].default is None and p["scan"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert list(p)[:4] == ["self", "state", "ref_speed", "obstacle_list"]              # the reference's positional arguments stay where they are


def test_control_rejects_scan_together_with_obstacles_before_any_device_call():
    """on the CPU checker backend (no device anywhere): scan + a non-empty obstacle list is the caller's mistake; scan alone asks for the
    device front end, which that backend does not have - loudly, there is no host fallback behind scan="""
    from oracle.oracle_backend import oracle_backend
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.mpc import MPC
    mpc = MPC(sc.rectangle_robot(), sc.line_path([0, 20, 0], [60, 20, 0]), receding=5, max_edge_num=4, max_obs_num=3, iter_num=1,
              time_print=False, _backend=oracle_backend)
    calls = []
    mpc.rda.upload_scan = lambda *a, **k: calls.append(a)
    state = np.array([[0.0], [20.0], [0.0]])
    scan = {"ranges": np.full(10, 5.0), "angle_min": -1.0, "angle_max": 1.0, "range_max": 10.0}
    with pytest.raises(ValueError):
        mpc.control(state, 4.0, [sc.circle(10.0, 20.0, 1.0)], scan=scan)
    assert not mpc.rda.has_scan
    with pytest.raises(RuntimeError):
        mpc.control(state, 4.0, scan=scan)
    assert calls == []
    u, info = mpc.control(state, 4.0, [sc.circle(10.0, 24.0, 1.0)])                        # the path without scan is what it was
    assert u.shape == (2, 1) and np.isfinite(u).all()
