"""Fleet lidar (rda_fleet_scan_boxes / rda_fleet_upload_scans, Fleet.control(scans=)): what can be checked without a GPU - the two entry points are
declared, exported, documented and bound with the header's argument lists; the Python interface has the new arguments where the issue puts them."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rda_fleet_scan_boxes", "rda_fleet_upload_scans")
RDA_ERR_ARG = -1


def _header():
    return open(os.path.join(ROOT, "include", "rda_hip.h")).read()


def _lib():
    from rda_planner_amd import _lib
    return C.CDLL(_lib.build())


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_documented(name):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert hasattr(_lib(), name)
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


C_INT_P, C_DOUBLE_P = C.POINTER(C.c_int), C.POINTER(C.c_double)
TYPES = {"rda_fleet *": C.c_void_p, "const int32_t *": C_INT_P, "int32_t *": C_INT_P, "const double *": C_DOUBLE_P, "double *": C_DOUBLE_P,
         "double": C.c_double, "int": C.c_int}


def _header_argtypes(name):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, re.S).group(1)
    out = []
    for a in args.split(","):
        m = re.match(r"\s*(.*?)(\w+)\s*$", a.strip(), re.S)
        ctype = " ".join(m.group(1).split())
        out.append(TYPES[ctype])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_prototypes_equal_the_header(name):
    from rda_planner_amd._capi import CApi
    api = CApi(_lib(), "rda")
    assert api.has_fleet_scans
    fn = getattr(api, name[len("rda_"):])
    assert list(fn.argtypes) == _header_argtypes(name)
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == (13 if name.endswith("boxes") else 11)


def test_null_fleet_is_an_argument_error():
    from rda_planner_amd._capi import CApi, dptr, iptr
    api = CApi(_lib(), "rda")
    nb, r, z, st, n = np.array([3], np.int32), np.full(3, 4.0), np.zeros(1), np.zeros(3), np.zeros(1, np.int32)
    boxes, order = np.zeros((1, 3, 4, 2)), np.ones(1, np.int32)
    assert api.fleet_scan_boxes(None, iptr(nb), dptr(r), dptr(z), dptr(z), dptr(z), dptr(st), 2.0, 6, iptr(n), dptr(boxes), 3, None) == RDA_ERR_ARG
    assert api.fleet_upload_scans(None, iptr(nb), dptr(r), dptr(z), dptr(z), dptr(z), dptr(st), 2.0, 6, iptr(order), iptr(n)) == RDA_ERR_ARG


def test_python_interface():
    from rda_planner_amd import lidar
    from rda_planner_amd.fleet import Fleet
    p = inspect.signature(Fleet.control).parameters
    assert list(p)[:4] == ["self", "states", "ref_speeds", "obstacle_lists"]
    assert p["scans"].default is None and p["scan_eps"].default == 2.0 and p["scan_min_samples"].default == 6
    assert list(p).index("scans") == 4 and p["scans"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert callable(lidar.scan_box_device_fleet)
    assert list(inspect.signature(lidar.scan_box_device_fleet).parameters) == ["fleet", "states", "scans", "eps", "min_samples"]


class _NoCalls:
    """stands for the library binding: any use of it is an error"""
    def __getattr__(self, name):
        raise AssertionError(f"library touched: {name}")


def test_scans_and_obstacles_together_are_refused_before_any_library_call():
    from rda_planner_amd.fleet import Fleet
    f = Fleet.__new__(Fleet)                           # no device: members and binding that fail on any use
    f.members, f.api, f._handle = [_NoCalls(), _NoCalls()], _NoCalls(), None
    scan = {"ranges": np.full(8, 15.0), "angle_min": -1.0, "angle_max": 1.0, "range_max": 15.0}
    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    with pytest.raises(ValueError):
        f.control(states, 4.0, [[], [object()]], scans=[scan, scan])
    with pytest.raises(ValueError):
        f.control(states, 4.0, [[object()], []], [scan, scan])
