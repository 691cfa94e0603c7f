"""Lidar boxes tracked across ticks (rda_fleet_upload_scans_tracked, rda_fleet_rollout_lidar_tracked, rda_fleet_track_boxes, rda_fleet_box_tracks,
rda_fleet_reset_tracks; Fleet.control(scans=, track=True), Fleet.rollout(lidar=, track=True)): what can be checked without a GPU - the entry points are
declared, exported, documented and bound with the header's argument lists, a null fleet is an argument error, and the Python interface refuses what it
refuses before any library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_fleet_lidar_peers_api import _Binding
from test_fleet_lidar_rollout_api import SENSOR, _header, _header_argtypes, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"rda_fleet_upload_scans_tracked": 13, "rda_fleet_rollout_lidar_tracked": 29, "rda_fleet_track_boxes": 7, "rda_fleet_box_tracks": 6,
         "rda_fleet_reset_tracks": 3}
RDA_ERR_ARG = -1


@pytest.mark.parametrize("name", sorted(NARGS))
def test_declared_exported_documented_and_bound_like_the_header(name):
    from rda_planner_amd._capi import CApi
    assert re.search(r"\bint\s+%s\s*\(" % name, _header()), name
    lib = _lib()
    assert hasattr(lib, name), f"{name} declared in include/rda_hip.h but not exported"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [ln for ln in doc.splitlines() if ln.startswith("|") and "`%s`" % name in ln], name
    api = CApi(lib, "rda")
    assert api.has_fleet_lidar_tracked is True
    fn = getattr(api, name[len("rda_"):])
    want = _header_argtypes(name)
    assert len(want) == NARGS[name]
    assert list(fn.argtypes) == want and fn.restype is C.c_int


def test_the_entries_take_the_untracked_entries_arguments():
    plain, tracked = _header_argtypes("rda_fleet_upload_scans"), _header_argtypes("rda_fleet_upload_scans_tracked")
    assert tracked[:-2] == plain and tracked[-2:] == [C.c_double, C.c_int]                # ... plus gate, window
    seeing, tracked = _header_argtypes("rda_fleet_rollout_lidar_peers"), _header_argtypes("rda_fleet_rollout_lidar_tracked")
    assert tracked[:-3] == seeing and tracked[-3:] == [C.c_int, C.c_double, C.c_int]      # ... plus see, gate, window


def test_null_arguments_are_argument_errors_without_a_device():
    from rda_planner_amd._capi import CApi, Info, dptr, iptr
    api = CApi(_lib(), "rda")
    K, B = 2, 1
    st, sp, cur, nb, one = np.zeros((B, 3)), np.ones(B), np.zeros(B, np.int32), np.full(B, 10, np.int32), np.ones(B)
    sl, ul, il, arr, info = np.zeros((K + 1, B, 3)), np.zeros((K, B, 2)), np.zeros((K, B), np.int32), np.zeros(B, np.int32), (Info * (K * B))()
    assert api.fleet_rollout_lidar_tracked(None, K, dptr(st), dptr(sp), iptr(cur), 0.1, 10, 1, None, iptr(nb), dptr(one), dptr(one), dptr(one), dptr(one),
                                           2.0, 6, iptr(cur), 0, dptr(sl), dptr(ul), iptr(il), info, iptr(arr), None, None, None, 0, 1.0,
                                           8) == RDA_ERR_ARG
    assert api.fleet_upload_scans_tracked(None, iptr(nb), dptr(np.zeros(10)), dptr(one), dptr(one), dptr(one), dptr(st), 2.0, 6, iptr(cur), None, 1.0,
                                          8) == RDA_ERR_ARG
    assert api.fleet_track_boxes(None, iptr(cur), dptr(np.zeros(8)), 1, 1.0, 8, None) == RDA_ERR_ARG
    assert api.fleet_box_tracks(None, 1, iptr(cur), None, None, None) == RDA_ERR_ARG
    assert api.fleet_reset_tracks(None, None, 0) == RDA_ERR_ARG


def test_python_interface_and_refusals_before_any_device_call():
    import types
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.fleet import Fleet
    for word in ("track=True", "rda_fleet_rollout_lidar_tracked", "track_gate", "track_window"):
        assert word in " ".join(Fleet.rollout.__doc__.split()), word
    for word in ("track=True", "rda_fleet_upload_scans_tracked", "lidar.track_boxes"):
        assert word in " ".join(Fleet.control.__doc__.split()), word

    def member():
        def no_solver(*a, **k):
            raise AssertionError("member touched")
        return types.SimpleNamespace(enable_reverse=False, _tracks=lambda kw: set(kw) <= {"threshold", "ind_range"}, goal_index_threshold=1, receding=5,
                                     car_tuple=sc.rectangle_robot(), rda_obstacle=False, obstacle_order=True, device_obstacles=True,
                                     rda=types.SimpleNamespace(has_scene=True), _piece=no_solver, _sync_path=no_solver)
    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    f = Fleet.__new__(Fleet)                           # no device: a binding that fails on any use
    f._handle = None
    f.api, f.members = _Binding(has_fleet_lidar_tracked=False, has_fleet_scans=True), [member(), member()]    # a library without the entry points
    with pytest.raises(ValueError, match="track=True tracks the boxes of lidar="):
        f.rollout(states, 4.0, 5, track=True)
    with pytest.raises(ValueError, match="track=True tracks the boxes of scans="):
        f.control(states, 4.0, track=True)
    for call in (lambda: f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], track=True), lambda: f.control(states, 4.0, scans=[None, None], track=True),
                 lambda: f.track_boxes([np.zeros((0, 4, 2))] * 2), f.box_tracks, f.reset_tracks):
        with pytest.raises(RuntimeError, match="rda_fleet_upload_scans_tracked, rda_fleet_rollout_lidar_tracked, rda_fleet_track_boxes, rda_fleet_box_tracks, "
                                               "rda_fleet_reset_tracks"):
            call()
    f.api = _Binding(has_fleet_lidar_tracked=True, has_fleet_scans=True)
    for bad in (dict(track_window=0), dict(track_window=9), dict(track_window=2.5), dict(track_gate=0.0), dict(track_gate=-1.0)):
        with pytest.raises(ValueError, match="track_gate > 0 and 1 <= track_window <= 8"):
            f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], track=True, **bad)
        with pytest.raises(ValueError, match="track_gate > 0 and 1 <= track_window <= 8"):
            f.control(states, 4.0, scans=[None, None], track=True, **bad)
    with pytest.raises(ValueError, match="one box array per member"):
        f.track_boxes([np.zeros((0, 4, 2))])
    with pytest.raises(ValueError, match="peers=True cannot be combined with lidar="):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], peers=True, track=True)
    f.api = _Binding()                                 # track not asked for: the flag is not even queried (the binding knows no such attribute)
    with pytest.raises(ValueError, match="scan_eps"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], scan_eps=0.0)
