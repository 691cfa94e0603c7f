"""Members that see each other in the simulated lidar (rda_fleet_raycast_peers, rda_fleet_rollout_lidar_peers; Fleet.raycast_peers,
Fleet.rollout(lidar=, see_peers=True); scenarios.peer_footprints): what can be checked without a GPU - the entry points are declared, exported, documented
and bound with the header's argument lists, a null fleet is an argument error, the Python interface takes the new switch, and everything it refuses is
refused before any library call."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from capi_lib import LIDAR_FLAGS, RDA_ERR_ARG, ROOT, SENSOR, Binding, bare_fleet, declared, header_argtypes, integration_rows, lib, pipeline_member

NARGS = {"rda_fleet_raycast_peers": 8, "rda_fleet_rollout_lidar_peers": 26}


@pytest.mark.parametrize("name", sorted(NARGS))
def test_declared_exported_documented_and_bound_like_the_header(name):
    from rda_planner_amd._capi import CApi
    assert declared(name), name
    so = lib()
    assert hasattr(so, name), f"{name} declared in include/rda_hip.h but not exported"
    assert integration_rows(name), name
    api = CApi(so, "rda")
    assert api.has_fleet_lidar_peers is True
    fn = getattr(api, name[len("rda_"):])
    want = header_argtypes(name)
    assert len(want) == NARGS[name]
    assert list(fn.argtypes) == want and fn.restype is C.c_int


def test_the_entries_take_the_blind_entries_arguments():
    from rda_planner_amd._capi import c_double_p
    assert header_argtypes("rda_fleet_raycast_peers") == header_argtypes("rda_fleet_raycast")
    blind, seeing = header_argtypes("rda_fleet_rollout_lidar"), header_argtypes("rda_fleet_rollout_lidar_peers")
    assert seeing[:-1] == blind and seeing[-1] is c_double_p                              # ... plus peer_clearance_log
    text = " ".join(re.sub(r"\n \* ", " ", open(os.path.join(ROOT, "include", "rda_hip.h")).read()).split())
    assert "rda_fleet_raycast_peers, then rda_fleet_upload_scans of those ranges at those states, then rda_fleet_step_tracked" in text      # the contract


def test_null_arguments_are_argument_errors_without_a_device():
    from rda_planner_amd._capi import CApi, Info, dptr, iptr
    api = CApi(lib(), "rda")
    K, B = 2, 1
    st, sp, cur, nb, one = np.zeros((B, 3)), np.ones(B), np.zeros(B, np.int32), np.full(B, 10, np.int32), np.ones(B)
    sl, ul, il, arr, info = np.zeros((K + 1, B, 3)), np.zeros((K, B, 2)), np.zeros((K, B), np.int32), np.zeros(B, np.int32), (Info * (K * B))()
    assert api.fleet_rollout_lidar_peers(None, K, dptr(st), dptr(sp), iptr(cur), 0.1, 10, 1, None, iptr(nb), dptr(one), dptr(one), dptr(one), dptr(one), 2.0,
                                         6, iptr(cur), 0, dptr(sl), dptr(ul), iptr(il), info, iptr(arr), None, None, None) == RDA_ERR_ARG
    assert api.fleet_raycast_peers(None, iptr(nb), dptr(one), dptr(one), dptr(one), dptr(one), dptr(st), dptr(np.zeros(10))) == RDA_ERR_ARG


def test_peer_footprints_are_the_peer_obstacles_standing():
    from rda_planner_amd import scenarios as sc
    cars = [sc.rectangle_robot(dynamics=d, wheelbase=3.0 if d == "acker" else 0) for d in ("acker", "diff", "omni", "diff")]
    states = [[10.0, 10.0, 0.3], np.array([[16.0], [11.0], [1.9]]), [12.0, 16.0, -2.4], [3.0, 4.0, 3.0]]
    for i in range(4):
        got, want = sc.peer_footprints(cars, states, i), sc.peer_obstacles(cars, states, np.zeros((4, 2)), i)
        assert len(got) == len(want) == 3
        for g, w, j in zip(got, want, [j for j in range(4) if j != i]):
            assert np.array_equal(g.vertex, w.vertex) and np.array_equal(g.vertex, sc.robot_vertices(cars[j], np.asarray(states[j], float).ravel()))
            assert g.cone_type == "Rpositive" and g.center is None and g.radius is None
            assert g.velocity.shape == (2, 1) and not g.velocity.any() and not w.velocity.any()
    assert sc.peer_footprints(cars[:1], states[:1], 0) == []


def test_python_interface_and_refusals_before_any_device_call():
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.fleet import Fleet
    assert list(inspect.signature(Fleet.raycast_peers).parameters) == ["self", "states", "sensors"]
    assert inspect.signature(Fleet.rollout).parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    doc = " ".join(Fleet.rollout.__doc__.split())
    assert all(word in doc for word in ("see_peers=True", "rda_fleet_rollout_lidar_peers", '"peer_clearance"', "standing boxes", "peer_footprints"))
    assert "see_peers" in Fleet.raycast.__doc__ and "see_peers" in Fleet.raycast_peers.__doc__ and "standing boxes" in " ".join(Fleet.raycast_peers.__doc__.split())

    member = pipeline_member
    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    f = bare_fleet(Binding(**LIDAR_FLAGS, has_fleet_lidar_peers=False), [member(), member()])        # no device; a library without the entry points
    with pytest.raises(ValueError, match="see_peers=True belongs to lidar="):
        f.rollout(states, 4.0, 5, see_peers=True)
    with pytest.raises(ValueError, match="see_peers=True belongs to lidar="):
        f.rollout(states, 4.0, 5, see_peers=True, obstacle_lists=[[], []])
    with pytest.raises(RuntimeError, match="rda_fleet_rollout_lidar_peers"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], see_peers=True)
    with pytest.raises(RuntimeError, match="rda_fleet_raycast_peers"):
        f.raycast_peers(states, [SENSOR, SENSOR])
    f.api = Binding(**LIDAR_FLAGS, has_fleet_lidar_peers=True)
    f.members = [member(), member(sc.circle_robot())]
    with pytest.raises(RuntimeError, match="circle"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], see_peers=True)
    with pytest.raises(RuntimeError, match="circle"):
        f.raycast_peers(states, [SENSOR, SENSOR])
    f.members = [member(), member()]
    with pytest.raises(ValueError, match="one sensor per member"):
        f.raycast_peers(states, [SENSOR])
    with pytest.raises(ValueError, match="one sensor per member"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR], see_peers=True)
    # what was refused stays refused, with the same exception type
    for peers in (True, "plan"):
        with pytest.raises(ValueError, match="peers=True cannot be combined with lidar="):
            f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], peers=peers)
        with pytest.raises(ValueError, match="peers=True cannot be combined with lidar="):
            f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], peers=peers, see_peers=True)
        with pytest.raises(ValueError, match="peers=True cannot be combined with lidar="):
            f.rollout(states, 4.0, 5, scans=[None, None], peers=peers)
    with pytest.raises(ValueError, match="gears=True cannot be combined"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], gears=True, see_peers=True)
    with pytest.raises(ValueError, match="world= belongs to lidar="):
        f.rollout(states, 4.0, 5, world=[[], []])
    f.api = Binding(**LIDAR_FLAGS)                             # see_peers not asked for: the flag is not even queried (the binding knows no such attribute)
    with pytest.raises(ValueError, match="scan_eps"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], scan_eps=0.0)
