"""Fleet members that avoid each other (rda_fleet_upload_scenes_peers, rda_fleet_scene_resort_peers, rda_fleet_rollout_peers, rda_fleet_peer_clearance;
Fleet.control(peers=True), Fleet.rollout(peers=True), Fleet.peer_clearance): what can be checked without a GPU - the numpy specification
(scenarios.peer_obstacles, scenarios.peer_clearance), the refusals of the Python interface before any library call, the entry points in the header and the
prototype table, and on the CPU oracle the behaviour the feature is for: three robots whose paths cross drive through each other when they are blind and
keep apart when every one sees the others as moving obstacles."""
import ctypes as C
import types
from math import cos, pi, sin

import numpy as np
import pytest

from capi_lib import Binding, bare_fleet, declared, integration_rows, lib, pipeline_member
from rda_planner_amd import scenarios as sc

NAMES = ("rda_fleet_upload_scenes_peers", "rda_fleet_scene_resort_peers", "rda_fleet_rollout_peers", "rda_fleet_peer_clearance", "rda_debug_scene_vel")


# ---- the specification ------------------------------------------------------------------------------------------------------------------------------
def cars3():
    return [sc.rectangle_robot(dynamics="acker"), sc.rectangle_robot(length=1.6, width=1.0, wheelbase=0, dynamics="diff"),
            sc.rectangle_robot(length=2.0, width=1.2, wheelbase=0, dynamics="omni")]


def test_peer_obstacles_follow_the_specification():
    cars = cars3()
    states = [np.array([[4.0], [20.0], [0.3]]), np.array([7.0, 23.0, -1.1]), np.array([[9.0], [26.0], [2.0]])]
    controls = [np.array([[1.5], [0.2]]), np.array([0.8, -0.4]), np.array([[1.2], [0.7]])]
    for i in range(3):
        obs = sc.peer_obstacles(cars, states, controls, i)
        others = [j for j in range(3) if j != i]                       # ascending j without i
        assert len(obs) == 2
        for o, j in zip(obs, others):
            st = np.asarray(states[j], float).ravel()
            assert o.cone_type == "Rpositive" and o.center is None and o.radius is None
            assert np.array_equal(o.vertex, sc.robot_vertices(cars[j], st)) and o.vertex.shape == (2, 4)
            v, w = (float(x) for x in np.asarray(controls[j]).ravel())
            a = w if cars[j].dynamics == "omni" else st[2]             # kinematic_step's rule: an omni robot moves along w, the others along their heading
            assert o.velocity.shape == (2, 1) and np.array_equal(o.velocity.ravel(), [v * cos(a), v * sin(a)])
            # ... which is where kinematic_step takes the robot: position after dt = position + velocity * dt
            nxt = sc.kinematic_step(st.reshape(3, 1), np.array([[v], [w]]), cars[j], 0.1)
            assert np.allclose(nxt[0:2, 0], st[0:2] + 0.1 * o.velocity.ravel(), rtol=0, atol=1e-15)
    assert sc.peer_obstacles(cars[:1], states[:1], controls[:1], 0) == []
    zero = sc.peer_obstacles(cars, states, [np.zeros(2)] * 3, 0)
    assert all(np.array_equal(o.velocity, np.zeros((2, 1))) for o in zero)


def test_peer_clearance_on_hand_placed_rectangles():
    box = sc.rectangle_robot(length=2.0, width=1.0, wheelbase=0, dynamics="diff")         # x in [-1, 1], y in [-0.5, 0.5]
    apart = sc.peer_clearance([box, box], [np.array([0.0, 0.0, 0.0]), np.array([3.0, 0.2, 0.0])])      # faces at x = 1 and x = 2
    assert apart.shape == (2,) and np.allclose(apart, 1.0, rtol=0, atol=1e-12)
    over = sc.peer_clearance([box, box], [np.array([0.0, 0.0, 0.0]), np.array([1.5, 0.0, 0.0])])       # 0.5 m of overlap along x, 1.0 along y
    assert np.allclose(over, -0.5, rtol=0, atol=1e-12)
    turned = sc.peer_clearance([box, box], [np.array([0.0, 0.0, 0.0]), np.array([3.0, 0.0, pi / 2])])  # the second one end-on: its face at x = 2.5
    assert np.allclose(turned, 1.5, rtol=0, atol=1e-12)
    three = sc.peer_clearance([box] * 3, [np.array([0.0, 0.0, 0.0]), np.array([3.0, 0.0, 0.0]), np.array([7.0, 0.0, 0.0])])
    assert np.allclose(three, [1.0, 1.0, 2.0], rtol=0, atol=1e-12)                                     # the nearest other member counts
    alone = sc.peer_clearance([box], [np.zeros(3)])
    assert alone.shape == (1,) and alone[0] == np.inf


# ---- the entry points -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_entries_declared_bound_and_exported(name):
    from rda_planner_amd import _capi
    assert declared(name), name
    assert name[len("rda_"):] in _capi.PROTOTYPES
    api = _capi.CApi(lib(), "rda")
    assert api.has_fleet_peers is True
    fn = getattr(api, name[len("rda_"):])
    assert list(fn.argtypes) == _capi.signature(_capi.PROTOTYPES[name[len("rda_"):]])[1] and fn.restype is C.c_int
    assert integration_rows(name, table=False)


def test_null_fleet_is_an_argument_error_without_a_device():
    from rda_planner_amd._capi import CApi, dptr, iptr
    api = CApi(lib(), "rda")
    st, ctl, one = np.zeros((1, 3)), np.zeros((1, 2)), np.zeros(1, np.int32)
    assert api.fleet_upload_scenes_peers(None, iptr(one), None, None, None, None, dptr(st), dptr(ctl)) == -1
    assert api.fleet_scene_resort_peers(None, dptr(st), dptr(ctl)) == -1
    assert api.fleet_peer_clearance(None, dptr(st), dptr(np.zeros(1))) == -1
    assert api.debug_scene_vel(None, dptr(np.zeros(2)), iptr(one)) == -1
    logs = (dptr(np.zeros((2, 1, 3))), dptr(np.zeros((1, 1, 2))), iptr(one), None, iptr(one))
    assert api.fleet_rollout_peers(None, 1, dptr(st), dptr(np.ones(1)), iptr(one), 0.1, 10, 1, None, dptr(ctl), *logs, None, None) == -1


# ---- the refusals of the Python interface -----------------------------------------------------------------------------------------------------------
def _member(cone="Rpositive", **kw):
    return pipeline_member(car=types.SimpleNamespace(cone_type=cone), cur_vel_array=np.zeros((2, 5)), **kw)


@pytest.mark.parametrize("has,bad,exc", [
    (False, _member(), RuntimeError),                          # a library without the entries
    (True, _member(order=False), RuntimeError),                # peers compete for the slots by distance
    (True, _member(cone="norm2"), RuntimeError),               # a circle robot has no polygon footprint
    (True, _member(rda_obstacle=True), RuntimeError),          # obstacles converted by the caller: nothing to append the peers to
    (True, _member(tracks=False), RuntimeError),               # a member that does not track on the device
], ids=["no-entries", "obstacle_order=False", "norm2", "rda_obstacle", "not-tracked"])
def test_python_refusals_before_any_library_call(has, bad, exc):
    f = bare_fleet(Binding(has_fleet_peers=has), [_member(), bad])
    states, obs = [np.zeros((3, 1)), np.ones((3, 1))], [[], []]
    with pytest.raises(exc):
        f.control(states, 2.0, obs, peers=True)
    with pytest.raises(exc):
        f.rollout(states, 2.0, 5, obstacle_lists=obs, peers=True)
    if not has:
        with pytest.raises(exc):
            f.peer_clearance(states)


def test_python_peers_with_scans_or_lidar_is_a_value_error():
    f = bare_fleet(Binding(has_fleet_peers=True), [_member(), _member()])
    states = [np.zeros((3, 1)), np.ones((3, 1))]
    scan = dict(ranges=np.ones(8), angle_min=-1.0, angle_max=1.0, range_max=5.0)
    sensor = dict(number=8, angle_min=-1.0, angle_max=1.0, range_min=0.0, range_max=5.0)
    with pytest.raises(ValueError):
        f.control(states, 2.0, None, scans=[scan, scan], peers=True)
    with pytest.raises(ValueError):
        f.rollout(states, 2.0, 5, lidar=[sensor, sensor], peers=True)
    with pytest.raises(ValueError):
        f.rollout(states, 2.0, 5, scans=[scan, scan], peers=True)
    with pytest.raises(ValueError):
        f.rollout(states, 2.0, 5, peers=True)                  # no obstacle_lists= and no such scenes resident


# ---- the behaviour, on the CPU oracle ---------------------------------------------------------------------------------------------------------------
T, N, E, ITER, DT, SPEED, KMAX = 8, 4, 4, 2, 0.1, 2.0, 140


def crossing():
    """the three robots of tests/test_gpu_fleet_peers.py test 5: two head-on on lanes 0.8 m apart, one across; their own obstacles stand far off"""
    car = sc.rectangle_robot(length=1.6, width=1.0, wheelbase=0, dynamics="diff")
    paths = [sc.line_path([4, 20, 0], [24, 20, 0], 0.1), sc.line_path([24, 20.8, pi], [4, 20.8, pi], 0.1), sc.line_path([14, 10, pi / 2], [14, 30, pi / 2], 0.1)]
    own = [[sc.regular_polygon(5 + 3 * j, 40 + 5 * e, 4, 0.5, 0.2 * j, velocity=(0.3, 0.0) if j == 0 else (0.0, 0.0)) for j in range(3)] for e in range(3)]
    return [car] * 3, paths, own


def at(obstacles, t):
    return [sc.Obstacle(None, None, o.vertex + o.velocity * t, o.cone_type, o.velocity.copy()) for o in obstacles]


def host_loop(peers, backend):
    """the loop Fleet.rollout(peers=True) replaces, member by member -> (minimum separation per member over the ticks, arrival ticks)"""
    from rda_planner_amd.mpc import MPC
    cars, paths, own = crossing()
    ms = [MPC(cars[i], [p.copy() for p in paths[i]], receding=T, sample_time=DT, iter_num=ITER, max_edge_num=E, max_obs_num=N, time_print=False,
              _backend=backend) for i in range(3)]
    states = [paths[i][0].copy() for i in range(3)]
    controls = [np.zeros((2, 1)) for _ in range(3)]
    arrived, sep = [-1] * 3, np.full(3, np.inf)
    for k in range(KMAX):
        us = []
        for i, m in enumerate(ms):
            obstacles = at(own[i], DT * k) + (sc.peer_obstacles(cars, states, controls, i) if peers else [])
            u, info = m.control(states[i], SPEED, obstacles)
            if info["arrive"] and arrived[i] < 0:
                arrived[i] = k
            us.append(u)
        states = [sc.kinematic_step(states[i], us[i], cars[i], DT) for i in range(3)]
        controls = us
        sep = np.minimum(sep, sc.peer_clearance(cars, states))
        if min(arrived) >= 0:
            break
    return sep, arrived


def test_oracle_three_robots_collide_blind_and_keep_apart_with_peers():
    """blind: every member overlaps another one on the way (separation < 0); with peers: the separation stays positive - the threshold is contact itself,
    the margin on this scenario is about 0.6 m - and all three still arrive within 140 ticks"""
    from oracle.oracle_backend import oracle_backend
    blind, arrived_blind = host_loop(False, oracle_backend)
    seen, arrived_seen = host_loop(True, oracle_backend)
    print("blind:", blind, arrived_blind, " peers:", seen, arrived_seen)
    assert np.all(blind < 0) and min(arrived_blind) >= 0
    assert np.all(seen > 0)
    assert min(arrived_seen) >= 0 and max(arrived_seen) < KMAX
