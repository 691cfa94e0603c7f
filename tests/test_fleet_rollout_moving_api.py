"""Fleet rollout for moving scenes (rda_fleet_rollout_moving, rda_fleet_clearance, rda_debug_scene_geom; Fleet.rollout(moving=True), Fleet.clearance): what
can be checked without a GPU - the entry points are declared, exported, documented and bound with the header's argument lists, a null fleet is an argument
error, Fleet.rollout keeps its signature, and the Python interface refuses what needs no device before any library call."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rda_fleet_rollout_moving", "rda_fleet_clearance", "rda_debug_scene_geom")
RDA_ERR_ARG = -1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rda_hip.h")).read(), flags=re.S)


def _lib():
    from rda_planner_amd import _lib
    return C.CDLL(_lib.build())


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_documented(name):
    assert re.search(r"\bint\s+%s\s*\(" % name, _header()), name
    assert hasattr(_lib(), name), f"{name} declared in include/rda_hip.h but not exported"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [ln for ln in doc.splitlines() if ln.startswith("|") and "`%s`" % name in ln]
    assert row, name
    if name == "rda_fleet_rollout_moving":
        assert any("mpc.py:166-187" in ln and "dynamic_obs" in ln for ln in row)      # the loop and the arrival rule it replaces


def _header_argtypes(name):
    from rda_planner_amd._capi import Info, c_double_p, c_int_p
    kinds = {"rda_fleet *": C.c_void_p, "rda_handle *": C.c_void_p, "const int32_t *": c_int_p, "int32_t *": c_int_p, "const double *": c_double_p,
             "double *": c_double_p, "double": C.c_double, "int": C.c_int, "rda_info *": C.POINTER(Info)}
    args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), re.S).group(1)
    return [kinds[" ".join(re.match(r"\s*(.*?)(\w+)\s*$", a.strip(), re.S).group(1).split())] for a in args.split(",")]


@pytest.mark.parametrize("name,nargs", [("rda_fleet_rollout_moving", 16), ("rda_fleet_clearance", 3), ("rda_debug_scene_geom", 3)])
def test_ctypes_prototype_follows_the_header(name, nargs):
    from rda_planner_amd._capi import CApi
    api = CApi(_lib(), "rda")
    assert api.has_fleet_rollout_moving
    fn = getattr(api, name[len("rda_"):])
    want = _header_argtypes(name)
    assert len(want) == nargs
    assert list(fn.argtypes) == want and fn.restype is C.c_int


def test_moving_entry_takes_the_static_entry_s_arguments_and_a_clearance_log():
    from rda_planner_amd._capi import c_double_p
    assert _header_argtypes("rda_fleet_rollout_moving") == _header_argtypes("rda_fleet_rollout") + [c_double_p]


def test_null_arguments_are_argument_errors_without_a_device():
    from rda_planner_amd._capi import CApi, Info, dptr, iptr
    api = CApi(_lib(), "rda")
    K, B = 2, 1
    st, sp, cur = np.zeros((B, 3)), np.ones(B), np.zeros(B, np.int32)
    sl, ul, il, arr, info = np.zeros((K + 1, B, 3)), np.zeros((K, B, 2)), np.zeros((K, B), np.int32), np.zeros(B, np.int32), (Info * (K * B))()
    cl = np.zeros((K, B))
    assert api.fleet_rollout_moving(None, K, dptr(st), dptr(sp), iptr(cur), 0.1, 10, 1, 1, None, dptr(sl), dptr(ul), iptr(il), info, iptr(arr),
                                    dptr(cl)) == RDA_ERR_ARG
    assert api.fleet_clearance(None, dptr(st), dptr(np.zeros(B))) == RDA_ERR_ARG
    assert api.debug_scene_geom(None, dptr(np.zeros(8)), iptr(np.zeros(1, np.int32))) == RDA_ERR_ARG


class _Binding:
    """stands for the library binding: it answers the two capability flags and fails on any other use"""
    def __init__(self, moving):
        self.__dict__.update(has_fleet_rollout=True, has_fleet_rollout_moving=moving)

    def __getattr__(self, name):
        raise AssertionError(f"library touched: {name}")


def test_python_interface_and_refusals_before_any_device_call():
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.fleet import Fleet
    p = inspect.signature(Fleet.rollout).parameters
    assert list(p)[:5] == ["self", "states", "ref_speeds", "steps", "resort"] and p["resort"].default is True
    assert p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD and len(p) == 6
    assert list(inspect.signature(Fleet.clearance).parameters) == ["self", "states"]
    doc = " ".join(Fleet.rollout.__doc__.split())
    assert "obstacle_lists" in doc and "moving=True" in doc and "clearance=True" in doc and "steps * dt" in doc

    def member(robot):
        def no_solver(*a, **k):
            raise AssertionError("member touched")
        return types.SimpleNamespace(enable_reverse=False, _tracks=lambda kw: set(kw) <= {"threshold", "ind_range"}, goal_index_threshold=1, receding=5,
                                     car_tuple=robot, _piece=no_solver, _sync_path=no_solver)
    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    f = Fleet.__new__(Fleet)                           # no device: a binding that fails on any use
    f._handle = None
    f.api, f.members = _Binding(moving=False), [member(sc.rectangle_robot()), member(sc.rectangle_robot())]
    with pytest.raises(RuntimeError, match="rda_fleet_rollout_moving"):
        f.rollout(states, 4.0, 5, moving=True)         # a library without the entry
    with pytest.raises(RuntimeError, match="rda_fleet_clearance"):
        f.clearance(states)
    f.api, f.members = _Binding(moving=True), [member(sc.rectangle_robot()), member(sc.circle_robot())]
    with pytest.raises(RuntimeError, match="circle"):
        f.rollout(states, 4.0, 5, moving=True, clearance=True, obstacle_lists=[[], []])      # a circle robot has no clearance log
    with pytest.raises(RuntimeError, match="circle"):
        f.clearance(states)
