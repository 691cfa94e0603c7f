"""Lidar boxes tracked across ticks (rda_fleet_upload_scans_tracked, rda_fleet_rollout_lidar_tracked, rda_fleet_track_boxes, rda_fleet_box_tracks,
rda_fleet_reset_tracks; Fleet.control(scans=, track=True), Fleet.rollout(lidar=, track=True)): what can be checked without a GPU - the entry points are
declared, exported, documented and bound with the header's argument lists, a null fleet is an argument error, and the Python interface refuses what it
refuses before any library call."""
import ctypes as C

import numpy as np
import pytest

from capi_lib import LIDAR_FLAGS, RDA_ERR_ARG, SENSOR, Binding, bare_fleet, declared, header_argtypes, integration_rows, lib, pipeline_member

NARGS = {"rda_fleet_upload_scans_tracked": 13, "rda_fleet_rollout_lidar_tracked": 29, "rda_fleet_track_boxes": 7, "rda_fleet_box_tracks": 6,
         "rda_fleet_reset_tracks": 3}


@pytest.mark.parametrize("name", sorted(NARGS))
def test_declared_exported_documented_and_bound_like_the_header(name):
    from rda_planner_amd._capi import CApi
    assert declared(name), name
    so = lib()
    assert hasattr(so, name), f"{name} declared in include/rda_hip.h but not exported"
    assert integration_rows(name), name
    api = CApi(so, "rda")
    assert api.has_fleet_lidar_tracked is True
    fn = getattr(api, name[len("rda_"):])
    want = header_argtypes(name)
    assert len(want) == NARGS[name]
    assert list(fn.argtypes) == want and fn.restype is C.c_int


def test_the_entries_take_the_untracked_entries_arguments():
    plain, tracked = header_argtypes("rda_fleet_upload_scans"), header_argtypes("rda_fleet_upload_scans_tracked")
    assert tracked[:-2] == plain and tracked[-2:] == [C.c_double, C.c_int]                # ... plus gate, window
    seeing, tracked = header_argtypes("rda_fleet_rollout_lidar_peers"), header_argtypes("rda_fleet_rollout_lidar_tracked")
    assert tracked[:-3] == seeing and tracked[-3:] == [C.c_int, C.c_double, C.c_int]      # ... plus see, gate, window


def test_null_arguments_are_argument_errors_without_a_device():
    from rda_planner_amd._capi import CApi, Info, dptr, iptr
    api = CApi(lib(), "rda")
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
    from rda_planner_amd.fleet import Fleet
    for word in ("track=True", "rda_fleet_rollout_lidar_tracked", "track_gate", "track_window"):
        assert word in " ".join(Fleet.rollout.__doc__.split()), word
    for word in ("track=True", "rda_fleet_upload_scans_tracked", "lidar.track_boxes"):
        assert word in " ".join(Fleet.control.__doc__.split()), word

    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    f = bare_fleet(Binding(**LIDAR_FLAGS, has_fleet_lidar_tracked=False, has_fleet_scans=True), [pipeline_member(), pipeline_member()])    # no device; a library without the entry points
    with pytest.raises(ValueError, match="track=True tracks the boxes of lidar="):
        f.rollout(states, 4.0, 5, track=True)
    with pytest.raises(ValueError, match="track=True tracks the boxes of scans="):
        f.control(states, 4.0, track=True)
    for call in (lambda: f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], track=True), lambda: f.control(states, 4.0, scans=[None, None], track=True),
                 lambda: f.track_boxes([np.zeros((0, 4, 2))] * 2), f.box_tracks, f.reset_tracks):
        with pytest.raises(RuntimeError, match="rda_fleet_upload_scans_tracked, rda_fleet_rollout_lidar_tracked, rda_fleet_track_boxes, rda_fleet_box_tracks, "
                                               "rda_fleet_reset_tracks"):
            call()
    f.api = Binding(**LIDAR_FLAGS, has_fleet_lidar_tracked=True, has_fleet_scans=True)
    for bad in (dict(track_window=0), dict(track_window=9), dict(track_window=2.5), dict(track_gate=0.0), dict(track_gate=-1.0)):
        with pytest.raises(ValueError, match="track_gate > 0 and 1 <= track_window <= 8"):
            f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], track=True, **bad)
        with pytest.raises(ValueError, match="track_gate > 0 and 1 <= track_window <= 8"):
            f.control(states, 4.0, scans=[None, None], track=True, **bad)
    with pytest.raises(ValueError, match="one box array per member"):
        f.track_boxes([np.zeros((0, 4, 2))])
    with pytest.raises(ValueError, match="peers=True cannot be combined with lidar="):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], peers=True, track=True)
    f.api = Binding(**LIDAR_FLAGS)                             # track not asked for: the flag is not even queried (the binding knows no such attribute)
    with pytest.raises(ValueError, match="scan_eps"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], scan_eps=0.0)
