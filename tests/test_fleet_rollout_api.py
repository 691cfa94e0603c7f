"""Fleet rollout (rda_fleet_rollout, Fleet.rollout): what can be checked without a GPU - the entry points are declared, exported, documented and bound
with the header's argument lists, a null fleet is an argument error, and the Python interface refuses what it does not support before any device call."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rda_fleet_rollout", "rda_fleet_rollout_last")
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
    row = [ln for ln in doc.splitlines() if "`%s`" % name in ln]
    assert row and any("mpc.py:166-187" in ln for ln in row)          # the row maps it to the reference's loop and arrival rule


def _header_argtypes(name):
    from rda_planner_amd._capi import Info, c_double_p, c_int_p
    kinds = {"rda_fleet *": C.c_void_p, "const int32_t *": c_int_p, "int32_t *": c_int_p, "const double *": c_double_p, "double *": c_double_p,
             "double": C.c_double, "int": C.c_int, "rda_info *": C.POINTER(Info)}
    args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), re.S).group(1)
    return [kinds[" ".join(re.match(r"\s*(.*?)(\w+)\s*$", a.strip(), re.S).group(1).split())] for a in args.split(",")]


@pytest.mark.parametrize("name,nargs", [("rda_fleet_rollout", 15), ("rda_fleet_rollout_last", 3)])
def test_ctypes_prototype_follows_the_header(name, nargs):
    from rda_planner_amd._capi import CApi
    api = CApi(_lib(), "rda")
    assert api.has_fleet_rollout
    fn = getattr(api, name[len("rda_"):])
    want = _header_argtypes(name)
    assert len(want) == nargs
    assert list(fn.argtypes) == want and fn.restype is C.c_int


def test_null_fleet_is_an_argument_error_without_a_device():
    from rda_planner_amd._capi import CApi, Info, dptr, iptr
    api = CApi(_lib(), "rda")
    K, B = 2, 1
    st, sp, cur = np.zeros((B, 3)), np.ones(B), np.zeros(B, np.int32)
    sl, ul, il, arr, info = np.zeros((K + 1, B, 3)), np.zeros((K, B, 2)), np.zeros((K, B), np.int32), np.zeros(B, np.int32), (Info * (K * B))()
    assert api.fleet_rollout(None, K, dptr(st), dptr(sp), iptr(cur), 0.1, 10, 1, 1, None, dptr(sl), dptr(ul), iptr(il), info, iptr(arr)) == RDA_ERR_ARG
    assert api.fleet_rollout_last(None, None, dptr(np.zeros(B))) == RDA_ERR_ARG


class _NoCalls:
    """stands for the library binding: any use of it is an error"""
    def __getattr__(self, name):
        raise AssertionError(f"library touched: {name}")


def test_python_interface_and_refusals_before_any_device_call():
    from rda_planner_amd.fleet import Fleet
    p = inspect.signature(Fleet.rollout).parameters
    assert list(p)[:5] == ["self", "states", "ref_speeds", "steps", "resort"] and p["resort"].default is True
    assert p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD

    def member(reverse, tracks):
        return types.SimpleNamespace(enable_reverse=reverse, _tracks=lambda kw: tracks, goal_index_threshold=1, receding=5)
    f = Fleet.__new__(Fleet)                           # no device: a binding that fails on any use
    f.api, f._handle = _NoCalls(), None
    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    f.members = [member(False, True), member(True, True)]
    with pytest.raises(RuntimeError):
        f.rollout(states, 4.0, 5)                      # enable_reverse=True: gear pieces are not rolled out, and there is no host fallback
    f.members = [member(False, True), member(False, False)]
    with pytest.raises(RuntimeError):
        f.rollout(states, 4.0, 5)                      # a member that does not track on the device
