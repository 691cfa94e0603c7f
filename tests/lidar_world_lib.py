"""What the fleet ray caster's and the lidar rollout's tests share (tests/test_gpu_fleet_raycast.py, tests/test_gpu_fleet_rollout_lidar.py): the lanes of
tests/fleet_twin_lib.py with their 7 obstacles per member taken as the WORLD, the three sensors, and the numpy reference - World.get_lidar_scan
itself, run on a World object that is given a pose, a sensor and an obstacle list."""
from types import SimpleNamespace

import numpy as np

from fleet_twin_lib import DT, NOBS, lane                  # noqa: F401  (the shapes of the rollout tests, not copies of them)
from rda_planner_amd import scenarios as sc
from rda_planner_amd.world import World, _Obstacle

WE = 4                                     # vertex stride of the lanes' worlds
# beams, field of view, range_max (range_min 0): half a turn ahead at 10 m, a full turn at 10 m, a full turn that sees 3 m
SENSORS = [dict(number=100, angle_min=-0.5 * np.pi, angle_max=0.5 * np.pi, range_min=0.0, range_max=10.0),
           dict(number=257, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=10.0),
           dict(number=64, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=3.0)]
EPS, MIN_SAMPLES = 2.0, 6


def at_time(obstacles, t):
    """the obstacle objects where they are at time t (position + velocity * t, no reflection)"""
    return [sc.Obstacle(None if o.center is None else o.center + o.velocity * t, o.radius, None if o.vertex is None else o.vertex + o.velocity * t,
                        o.cone_type, o.velocity.copy()) for o in obstacles]


def numpy_scan(state, sensor, obstacles):
    """World.get_lidar_scan of `sensor` at `state` against `obstacles` (scenarios.Obstacle objects): the specification's own code"""
    w = World.__new__(World)
    w.robot = SimpleNamespace(state=np.asarray(state, float).reshape(3, 1))
    w.lidar = SimpleNamespace(**sensor)
    w.obstacles = [_Obstacle("circle" if o.cone_type == "norm2" else "polygon", None if o.center is None else np.asarray(o.center, float).ravel(), o.radius,
                             None if o.vertex is None else np.asarray(o.vertex, float), np.zeros(2)) for o in obstacles]
    if sensor["number"] == 0:
        return dict(ranges=np.zeros(0), angle_min=sensor["angle_min"], angle_max=sensor["angle_max"], range_min=sensor["range_min"],
                    range_max=sensor["range_max"])
    return w.get_lidar_scan()


def flatten(obstacles, we=WE):
    """obstacle objects -> (kind, nvert, geom [n][we][2], vel [n][2]) in the layout of rda_fleet_upload_worlds"""
    n = len(obstacles)
    kind, nvert, geom, vel = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, we, 2)), np.zeros((n, 2))
    for i, o in enumerate(obstacles):
        vel[i] = np.asarray(o.velocity, float).ravel()[0:2]
        if o.cone_type == "norm2":
            kind[i] = 1
            geom[i, 0] = np.asarray(o.center, float).ravel()[0:2]
            geom[i, 1, 0] = o.radius
        else:
            V = np.asarray(o.vertex, float)
            nvert[i] = V.shape[1]
            geom[i, :V.shape[1]] = V.T
    return kind, nvert, geom, vel


def sensor_c(sensors):
    """the member-major sensor arrays of rda_fleet_raycast: n_beams, angle_min, angle_max, range_min, range_max"""
    return (np.array([s["number"] for s in sensors], np.int32),) + tuple(np.array([float(s[k]) for s in sensors])
                                                                         for k in ("angle_min", "angle_max", "range_min", "range_max"))


__all__ = ["DT", "NOBS", "WE", "SENSORS", "EPS", "MIN_SAMPLES", "lane", "at_time", "numpy_scan", "flatten", "sensor_c"]
