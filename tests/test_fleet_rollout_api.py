"""Fleet rollout (rda_fleet_rollout, Fleet.rollout): what can be checked without a GPU - the entry points are declared, exported, documented and bound
with the header's argument lists, a null fleet is an argument error, and the Python interface refuses what it does not support before any device call."""
import ctypes as C
import inspect

import numpy as np
import pytest

from capi_lib import RDA_ERR_ARG, Binding, bare_fleet, declared, header_argtypes, integration_rows, lib, member

NAMES = ("rda_fleet_rollout", "rda_fleet_rollout_last")


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_documented(name):
    assert declared(name), name
    assert hasattr(lib(), name), f"{name} declared in include/rda_hip.h but not exported"
    row = integration_rows(name, table=False)
    assert row and any("mpc.py:166-187" in ln for ln in row)          # the row maps it to the reference's loop and arrival rule


@pytest.mark.parametrize("name,nargs", [("rda_fleet_rollout", 15), ("rda_fleet_rollout_last", 3)])
def test_ctypes_prototype_follows_the_header(name, nargs):
    from rda_planner_amd._capi import CApi
    api = CApi(lib(), "rda")
    assert api.has_fleet_rollout
    fn = getattr(api, name[len("rda_"):])
    want = header_argtypes(name)
    assert len(want) == nargs
    assert list(fn.argtypes) == want and fn.restype is C.c_int


def test_null_fleet_is_an_argument_error_without_a_device():
    from rda_planner_amd._capi import CApi, Info, dptr, iptr
    api = CApi(lib(), "rda")
    K, B = 2, 1
    st, sp, cur = np.zeros((B, 3)), np.ones(B), np.zeros(B, np.int32)
    sl, ul, il, arr, info = np.zeros((K + 1, B, 3)), np.zeros((K, B, 2)), np.zeros((K, B), np.int32), np.zeros(B, np.int32), (Info * (K * B))()
    assert api.fleet_rollout(None, K, dptr(st), dptr(sp), iptr(cur), 0.1, 10, 1, 1, None, dptr(sl), dptr(ul), iptr(il), info, iptr(arr)) == RDA_ERR_ARG
    assert api.fleet_rollout_last(None, None, dptr(np.zeros(B))) == RDA_ERR_ARG


def test_python_interface_and_refusals_before_any_device_call():
    from rda_planner_amd.fleet import Fleet
    p = inspect.signature(Fleet.rollout).parameters
    assert list(p)[:5] == ["self", "states", "ref_speeds", "steps", "resort"] and p["resort"].default is True
    assert p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD

    f = bare_fleet(Binding(), [member(), member(reverse=True)])         # no device: a binding that fails on any use
    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    with pytest.raises(RuntimeError):
        f.rollout(states, 4.0, 5)                      # enable_reverse=True: gear pieces are not rolled out, and there is no host fallback
    f.members = [member(), member(tracks=False)]
    with pytest.raises(RuntimeError):
        f.rollout(states, 4.0, 5)                      # a member that does not track on the device
