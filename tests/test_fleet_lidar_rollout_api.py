"""The simulated sensor and the lidar rollout (rda_fleet_upload_worlds, rda_fleet_raycast, rda_fleet_rollout_lidar, rda_debug_fleet_world; Fleet.upload_worlds,
Fleet.raycast, Fleet.rollout(lidar=, world=)): what can be checked without a GPU - the entry points are declared, exported, documented and bound with the
header's argument lists, a null fleet is an argument error, Fleet.rollout keeps its signature and takes the new keywords, and sensors are validated before any
library call."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest

from capi_lib import RDA_ERR_ARG, SENSOR, Binding, bare_fleet, declared, header_argtypes, integration_rows, lib, member

NARGS = {"rda_fleet_upload_worlds": 7, "rda_fleet_raycast": 8, "rda_fleet_rollout_lidar": 25, "rda_debug_fleet_world": 4}


@pytest.mark.parametrize("name", sorted(NARGS))
def test_declared_exported_documented_and_bound_like_the_header(name):
    from rda_planner_amd._capi import CApi
    assert declared(name), name
    so = lib()
    assert hasattr(so, name), f"{name} declared in include/rda_hip.h but not exported"
    assert integration_rows(name), name
    api = CApi(so, "rda")
    assert api.has_fleet_rollout_lidar
    fn = getattr(api, name[len("rda_"):])
    want = header_argtypes(name)
    assert len(want) == NARGS[name]
    assert list(fn.argtypes) == want and fn.restype is C.c_int


def test_lidar_entry_takes_the_static_entry_s_arguments_without_resort():
    from rda_planner_amd._capi import c_double_p, c_int_p
    static, lidar = header_argtypes("rda_fleet_rollout"), header_argtypes("rda_fleet_rollout_lidar")
    sensor = header_argtypes("rda_fleet_raycast")[1:6]
    assert lidar[:8] == static[:8] and lidar[8] == static[9]                              # ... , goal_margin | nom_u: `resort` is gone
    assert lidar[9:14] == sensor                                                          # the sensor arrays of rda_fleet_raycast
    assert lidar[14:18] == [C.c_double, C.c_int, c_int_p, C.c_int]                        # eps, min_samples, order, moving
    assert lidar[18:23] == static[10:] and lidar[23:] == [c_int_p, c_double_p]           # the logs, then nbox_log and clearance_log


def test_null_arguments_are_argument_errors_without_a_device():
    from rda_planner_amd._capi import CApi, Info, dptr, iptr
    api = CApi(lib(), "rda")
    K, B = 2, 1
    st, sp, cur, nb, one = np.zeros((B, 3)), np.ones(B), np.zeros(B, np.int32), np.full(B, 10, np.int32), np.ones(B)
    sl, ul, il, arr, info = np.zeros((K + 1, B, 3)), np.zeros((K, B, 2)), np.zeros((K, B), np.int32), np.zeros(B, np.int32), (Info * (K * B))()
    assert api.fleet_rollout_lidar(None, K, dptr(st), dptr(sp), iptr(cur), 0.1, 10, 1, None, iptr(nb), dptr(one), dptr(one), dptr(one), dptr(one), 2.0, 6,
                                   iptr(cur), 0, dptr(sl), dptr(ul), iptr(il), info, iptr(arr), None, None) == RDA_ERR_ARG
    assert api.fleet_raycast(None, iptr(nb), dptr(one), dptr(one), dptr(one), dptr(one), dptr(st), dptr(np.zeros(10))) == RDA_ERR_ARG
    assert api.fleet_upload_worlds(None, iptr(cur), 4, None, None, None, None) == RDA_ERR_ARG
    assert api.debug_fleet_world(None, None, iptr(cur), None) == RDA_ERR_ARG


def test_sensor_mappings_are_validated():
    from rda_planner_amd.fleet import sensor_arrays
    from rda_planner_amd.world import World
    nb, lo, hi, rmin, rmax = sensor_arrays([SENSOR, types.SimpleNamespace(**dict(SENSOR, number=7, range_min=0.5))], 2)
    assert nb.dtype == np.int32 and list(nb) == [100, 7] and list(lo) == [-1.5, -1.5] and list(rmin) == [0.0, 0.5] and list(rmax) == [10.0, 10.0]
    assert all(a.dtype == np.float64 and a.flags.c_contiguous for a in (lo, hi, rmin, rmax))
    w = World({"robot": [{"sensors": [{"type": "lidar2d", "number": 33, "angle_range": 2.0, "range_max": 6.0}]}]})
    nb, lo, hi, rmin, rmax = sensor_arrays([w.lidar], 1)                                  # World.lidar has the fields
    assert (nb[0], lo[0], hi[0], rmin[0], rmax[0]) == (33, -1.0, 1.0, 0.0, 6.0)
    for bad in (None, [SENSOR], [SENSOR] * 3):
        with pytest.raises(ValueError, match="one sensor per member"):
            sensor_arrays(bad, 2)
    broken = [{k: v for k, v in SENSOR.items() if k != "range_min"}, dict(SENSOR, number=-1), dict(SENSOR, number=2.5), dict(SENSOR, angle_max=-2.0),
              dict(SENSOR, range_max=float("nan")), dict(SENSOR, range_min=11.0), dict(SENSOR, range_min=-1.0), object()]
    for s in broken:
        with pytest.raises(ValueError):
            sensor_arrays([s], 1)


def test_python_interface_and_refusals_before_any_device_call():
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.fleet import Fleet
    p = inspect.signature(Fleet.rollout).parameters
    assert list(p)[:5] == ["self", "states", "ref_speeds", "steps", "resort"] and p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(Fleet.raycast).parameters) == ["self", "states", "sensors"]
    assert list(inspect.signature(Fleet.upload_worlds).parameters) == ["self", "obstacle_lists"]
    doc = " ".join(Fleet.rollout.__doc__.split())
    assert all(word in doc for word in ("lidar=sensors", "world=obstacle_lists", "scan_eps", "scan_min_samples", '"boxes"', "rda_fleet_rollout_lidar"))

    def binding(lidar):
        return Binding(has_fleet_rollout=True, has_fleet_rollout_moving=True, has_fleet_rollout_lidar=lidar)
    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    f = bare_fleet(binding(False), [member(car_tuple=sc.rectangle_robot(), rda_obstacle=False) for _ in range(2)])      # no device: a binding that fails on any use
    with pytest.raises(RuntimeError, match="rda_fleet_rollout_lidar"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR])         # a library without the entry
    with pytest.raises(RuntimeError, match="rda_fleet_raycast"):
        f.raycast(states, [SENSOR, SENSOR])
    with pytest.raises(RuntimeError, match="rda_fleet_upload_worlds"):
        f.upload_worlds([[], []])
    f.api = binding(True)
    with pytest.raises(ValueError, match="one sensor per member"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR])
    with pytest.raises(ValueError, match="world= belongs to lidar="):
        f.rollout(states, 4.0, 5, world=[[], []])
    with pytest.raises(ValueError, match="not both"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], obstacle_lists=[[], []])
    with pytest.raises(ValueError, match="scan_eps"):
        f.rollout(states, 4.0, 5, lidar=[SENSOR, SENSOR], scan_eps=0.0)
    with pytest.raises(ValueError, match="one obstacle list per member"):
        f.upload_worlds([[]])
    with pytest.raises(ValueError, match="at most 8 vertices"):
        f.upload_worlds([[sc.regular_polygon(0.0, 0.0, 9, 1.0, 0.0)], []])
    with pytest.raises(ValueError, match="one sensor per member"):
        f.raycast(states, [SENSOR])
