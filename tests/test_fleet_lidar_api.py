"""Fleet lidar (rda_fleet_scan_boxes / rda_fleet_upload_scans, Fleet.control(scans=)): what can be checked without a GPU - the two entry points are
declared, exported, documented and bound with the header's argument lists; the Python interface has the new arguments where the issue puts them."""
import ctypes as C
import inspect

import numpy as np
import pytest

from capi_lib import RDA_ERR_ARG, Binding, bare_fleet, declared, header_argtypes, integration_rows, lib

NAMES = ("rda_fleet_scan_boxes", "rda_fleet_upload_scans")


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_documented(name):
    assert declared(name), name
    assert hasattr(lib(), name)
    assert integration_rows(name, table=False)


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_prototypes_equal_the_header(name):
    from rda_planner_amd._capi import CApi
    api = CApi(lib(), "rda")
    assert api.has_fleet_scans
    fn = getattr(api, name[len("rda_"):])
    assert list(fn.argtypes) == header_argtypes(name)
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == (13 if name.endswith("boxes") else 11)


def test_null_fleet_is_an_argument_error():
    from rda_planner_amd._capi import CApi, dptr, iptr
    api = CApi(lib(), "rda")
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


def test_scans_and_obstacles_together_are_refused_before_any_library_call():
    f = bare_fleet(Binding(), [Binding(), Binding()])  # no device: members and binding that fail on any use
    scan = {"ranges": np.full(8, 15.0), "angle_min": -1.0, "angle_max": 1.0, "range_max": 15.0}
    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    with pytest.raises(ValueError):
        f.control(states, 4.0, [[], [object()]], scans=[scan, scan])
    with pytest.raises(ValueError):
        f.control(states, 4.0, [[object()], []], [scan, scan])
