"""Fleet rollout for moving scenes (rda_fleet_rollout_moving, rda_fleet_clearance, rda_debug_scene_geom; Fleet.rollout(moving=True), Fleet.clearance): what
can be checked without a GPU - the entry points are declared, exported, documented and bound with the header's argument lists, a null fleet is an argument
error, Fleet.rollout keeps its signature, and the Python interface refuses what needs no device before any library call."""
import ctypes as C
import inspect

import numpy as np
import pytest

from capi_lib import RDA_ERR_ARG, Binding, bare_fleet, declared, header_argtypes, integration_rows, lib, member

NAMES = ("rda_fleet_rollout_moving", "rda_fleet_clearance", "rda_debug_scene_geom")


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_documented(name):
    assert declared(name), name
    assert hasattr(lib(), name), f"{name} declared in include/rda_hip.h but not exported"
    row = integration_rows(name)
    assert row, name
    if name == "rda_fleet_rollout_moving":
        assert any("mpc.py:166-187" in ln and "dynamic_obs" in ln for ln in row)      # the loop and the arrival rule it replaces


@pytest.mark.parametrize("name,nargs", [("rda_fleet_rollout_moving", 16), ("rda_fleet_clearance", 3), ("rda_debug_scene_geom", 3)])
def test_ctypes_prototype_follows_the_header(name, nargs):
    from rda_planner_amd._capi import CApi
    api = CApi(lib(), "rda")
    assert api.has_fleet_rollout_moving
    fn = getattr(api, name[len("rda_"):])
    want = header_argtypes(name)
    assert len(want) == nargs
    assert list(fn.argtypes) == want and fn.restype is C.c_int


def test_moving_entry_takes_the_static_entry_s_arguments_and_a_clearance_log():
    from rda_planner_amd._capi import c_double_p
    assert header_argtypes("rda_fleet_rollout_moving") == header_argtypes("rda_fleet_rollout") + [c_double_p]


def test_null_arguments_are_argument_errors_without_a_device():
    from rda_planner_amd._capi import CApi, Info, dptr, iptr
    api = CApi(lib(), "rda")
    K, B = 2, 1
    st, sp, cur = np.zeros((B, 3)), np.ones(B), np.zeros(B, np.int32)
    sl, ul, il, arr, info = np.zeros((K + 1, B, 3)), np.zeros((K, B, 2)), np.zeros((K, B), np.int32), np.zeros(B, np.int32), (Info * (K * B))()
    cl = np.zeros((K, B))
    assert api.fleet_rollout_moving(None, K, dptr(st), dptr(sp), iptr(cur), 0.1, 10, 1, 1, None, dptr(sl), dptr(ul), iptr(il), info, iptr(arr),
                                    dptr(cl)) == RDA_ERR_ARG
    assert api.fleet_clearance(None, dptr(st), dptr(np.zeros(B))) == RDA_ERR_ARG
    assert api.debug_scene_geom(None, dptr(np.zeros(8)), iptr(np.zeros(1, np.int32))) == RDA_ERR_ARG


def test_python_interface_and_refusals_before_any_device_call():
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.fleet import Fleet
    p = inspect.signature(Fleet.rollout).parameters
    assert list(p)[:5] == ["self", "states", "ref_speeds", "steps", "resort"] and p["resort"].default is True
    assert p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD and len(p) == 6
    assert list(inspect.signature(Fleet.clearance).parameters) == ["self", "states"]
    doc = " ".join(Fleet.rollout.__doc__.split())
    assert "obstacle_lists" in doc and "moving=True" in doc and "clearance=True" in doc and "steps * dt" in doc

    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    f = bare_fleet(Binding(has_fleet_rollout=True, has_fleet_rollout_moving=False), [member(car_tuple=sc.rectangle_robot()) for _ in range(2)])
    with pytest.raises(RuntimeError, match="rda_fleet_rollout_moving"):
        f.rollout(states, 4.0, 5, moving=True)         # a library without the entry
    with pytest.raises(RuntimeError, match="rda_fleet_clearance"):
        f.clearance(states)
    f.api, f.members = Binding(has_fleet_rollout=True, has_fleet_rollout_moving=True), [member(car_tuple=sc.rectangle_robot()), member(car_tuple=sc.circle_robot())]
    with pytest.raises(RuntimeError, match="circle"):
        f.rollout(states, 4.0, 5, moving=True, clearance=True, obstacle_lists=[[], []])      # a circle robot has no clearance log
    with pytest.raises(RuntimeError, match="circle"):
        f.clearance(states)
