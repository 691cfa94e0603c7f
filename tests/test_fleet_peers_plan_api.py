"""Peers predicted along their planned trajectories (rda_fleet_upload_scenes_peers_plan, rda_fleet_scene_resort_peers_plan, rda_fleet_rollout_peers_plan,
rda_fleet_rollout_last_plan; Fleet.control(peers="plan"), Fleet.rollout(peers="plan")): what can be checked without a GPU - the numpy specification
(scenarios.peer_plan_poses, scenarios.peer_plan_obstacles), the argument handling and the plan bookkeeping of `Fleet` on a stub binding, the entry points
in the header and the prototype table."""
import ctypes as C
import types
from math import cos, sin

import numpy as np
import pytest

from capi_lib import Binding, bare_fleet, declared, integration_rows, lib, pipeline_member
from rda_planner_amd import scenarios as sc

NAMES = ("rda_fleet_upload_scenes_peers_plan", "rda_fleet_scene_resort_peers_plan", "rda_fleet_rollout_peers_plan", "rda_fleet_rollout_last_plan")
T, DT = 8, 0.1


def cars3():
    return [sc.rectangle_robot(dynamics="acker"), sc.rectangle_robot(length=1.6, width=1.0, wheelbase=0, dynamics="diff"),
            sc.rectangle_robot(length=2.0, width=1.2, wheelbase=0, dynamics="omni")]


def arc_plan(x, v=2.0, w=0.8):
    t = DT * np.arange(T + 1)
    return np.array([x[0] + (v / w) * (np.sin(x[2] + w * t) - sin(x[2])), x[1] - (v / w) * (np.cos(x[2] + w * t) - cos(x[2])), x[2] + w * t])


# ---- the specification ------------------------------------------------------------------------------------------------------------------------------
def test_a_straight_constant_speed_plan_is_the_constant_velocity_prediction():
    x, v = np.array([4.0, 20.0, 0.3]), 1.7
    t = DT * np.arange(T + 1)
    P = np.array([x[0] + v * cos(x[2]) * (t - DT), x[1] + v * sin(x[2]) * (t - DT), np.full(T + 1, x[2])])       # column 1 is the state: the plan of one tick ago
    poses = sc.peer_plan_poses(x, P, T)
    assert poses.shape == (T + 1, 3)
    want = np.array([[x[0] + v * cos(x[2]) * k * DT, x[1] + v * sin(x[2]) * k * DT, x[2]] for k in range(T + 1)])
    assert np.abs(poses - want).max() <= 1e-12
    assert np.array_equal(poses[0], x)


def test_last_increment_rule_and_anchoring():
    x = np.array([4.0, 20.0, 0.3])
    P = arc_plan(np.array([3.7, 20.4, 0.25]))                      # the plant is not where the plan put it
    poses = sc.peer_plan_poses(x.reshape(3, 1), P, T)
    for t in range(1, T):
        assert np.array_equal(poses[t], x + (P[:, t + 1] - P[:, 1]))
    assert np.array_equal(poses[T], x + ((P[:, T] + (P[:, T] - P[:, T - 1])) - P[:, 1]))          # stage T: the last increment repeated
    assert np.allclose(poses[T] - poses[T - 1], P[:, T] - P[:, T - 1], rtol=0, atol=1e-12)
    assert np.abs(poses[1] - x - (P[:, 2] - P[:, 1])).max() == 0                                   # no jump at stage 1: displacements only
    shift = np.array([1.5, -2.25, 0.125])
    assert np.abs(sc.peer_plan_poses(x + shift, P, T) - (poses + shift)).max() <= 1e-12          # anchoring: every pose moves with the state
    assert np.abs(sc.peer_plan_poses(x, P + shift.reshape(3, 1), T) - poses).max() <= 1e-12      # ... and not with the plan's origin


def test_obstacle_form():
    from rda_planner_amd.mpc import MPC
    cars = cars3()
    states = [np.array([[4.0], [20.0], [0.3]]), np.array([7.0, 23.0, -1.1]), np.array([[9.0], [26.0], [2.0]])]
    controls = [np.array([[1.5], [0.2]]), np.array([0.8, -0.4]), np.array([[1.2], [0.7]])]
    plans = [arc_plan(np.asarray(s, float).ravel()) for s in states]
    valid = [1, 0, 1]
    conv = MPC.__new__(MPC)
    conv.receding, conv.dt = T, DT
    for i in range(3):
        obs = sc.peer_plan_obstacles(cars, states, controls, plans, valid, i, T, dt=DT)
        plain = sc.peer_obstacles(cars, states, controls, i)
        others = [j for j in range(3) if j != i]
        assert len(obs) == 2
        for o, p, j in zip(obs, plain, others):
            assert o.cone_type == "Rpositive" and np.array_equal(o.vertex, p.vertex) and np.array_equal(o.velocity, p.velocity)
            assert isinstance(o.A, list) and isinstance(o.b, list) and len(o.A) == len(o.b) == len(o.vertices) == T + 1
            for t in range(T + 1):
                A, b = conv.convert_inequal_polygon(o.vertices[t])
                assert np.array_equal(o.A[t], A) and np.array_equal(o.b[t], b) and o.A[t].shape == (4, 2) and o.b[t].shape == (4, 1)
            if valid[j]:
                poses = sc.peer_plan_poses(states[j], plans[j], T)
                assert all(np.array_equal(o.vertices[t], sc.robot_vertices(cars[j], poses[t])) for t in range(1, T + 1))
                assert np.array_equal(o.vertices[0], p.vertex)
            else:                                                      # no valid plan: the constant-velocity prediction of every moving polygon
                A, b = conv.convert_inequal_polygon(p.vertex, p.velocity)
                assert all(np.array_equal(x, y) for x, y in zip(o.A, A)) and all(np.array_equal(x, y) for x, y in zip(o.b, b))
    # what RDA_solver._stage takes for time-varying obstacles
    from rda_planner_amd.rda_solver import RDA_solver
    stage = types.SimpleNamespace(max_obs_num=4, max_edge_num=4, T=T)
    use, A, b, cone, per_t = RDA_solver._stage(stage, list(sc.peer_plan_obstacles(cars, states, controls, plans, valid, 0, T, dt=DT)))
    assert (use, per_t) == (4, 1) and A.shape == (4, T + 1, 4, 2) and not cone.any()


# ---- the entry points -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_entries_declared_bound_and_exported(name):
    from rda_planner_amd import _capi
    assert declared(name), name
    assert name[len("rda_"):] in _capi.PROTOTYPES
    api = _capi.CApi(lib(), "rda")
    assert api.has_fleet_peers_plan is True
    fn = getattr(api, name[len("rda_"):])
    assert list(fn.argtypes) == _capi.signature(_capi.PROTOTYPES[name[len("rda_"):]])[1] and fn.restype is C.c_int
    assert integration_rows(name, table=False)


def test_null_fleet_is_an_argument_error_without_a_device():
    from rda_planner_amd._capi import CApi, dptr, iptr
    api = CApi(lib(), "rda")
    st, ctl, one, plan = np.zeros((1, 3)), np.zeros((1, 2)), np.zeros(1, np.int32), np.zeros((1, 3, T + 1))
    assert api.fleet_upload_scenes_peers_plan(None, iptr(one), None, None, None, None, dptr(st), dptr(ctl), dptr(plan), iptr(one)) == -1
    assert api.fleet_scene_resort_peers_plan(None, dptr(st), dptr(ctl), dptr(plan), iptr(one)) == -1
    assert api.fleet_rollout_last_plan(None, dptr(plan)) == -1
    logs = (dptr(np.zeros((2, 1, 3))), dptr(np.zeros((1, 1, 2))), iptr(one), None, iptr(one))
    assert api.fleet_rollout_peers_plan(None, 1, dptr(st), dptr(np.ones(1)), iptr(one), 0.1, 10, 1, None, dptr(ctl), *logs, None, None, dptr(plan), iptr(one)) == -1


# ---- Fleet: argument handling and bookkeeping on a stub binding -------------------------------------------------------------------------------------
def _member(cone="Rpositive", **kw):
    return pipeline_member(car=types.SimpleNamespace(cone_type=cone), cur_vel_array=np.zeros((2, 5)), **kw)


def _binding(has_fleet_peers=True, has_fleet_peers_plan=True):
    return Binding(has_fleet_peers=has_fleet_peers, has_fleet_peers_plan=has_fleet_peers_plan)


STATES, OBS = [np.zeros((3, 1)), np.ones((3, 1))], [[], []]


def test_plan_mode_without_the_entry_points_raises_before_any_library_call():
    f = bare_fleet(_binding(True, False), [_member(), _member()])
    with pytest.raises(RuntimeError, match="plan"):
        f.control(STATES, 2.0, OBS, peers="plan")
    with pytest.raises(RuntimeError, match="plan"):
        f.rollout(STATES, 2.0, 5, obstacle_lists=OBS, peers="plan")


@pytest.mark.parametrize("value", ["other", "Plan", "", 2.5, [True], ("plan",)])
def test_any_other_value_of_peers_is_a_value_error(value):
    f = bare_fleet(_binding(), [_member(), _member()])
    with pytest.raises(ValueError):
        f.control(STATES, 2.0, OBS, peers=value)
    with pytest.raises(ValueError):
        f.rollout(STATES, 2.0, 5, obstacle_lists=OBS, peers=value)


@pytest.mark.parametrize("bad", [_member(order=False), _member(cone="norm2"), _member(rda_obstacle=True), _member(tracks=False)],
                         ids=["obstacle_order=False", "norm2", "rda_obstacle", "not-tracked"])
def test_plan_mode_has_the_refusals_of_the_constant_velocity_mode(bad):
    f = bare_fleet(_binding(), [_member(), bad])
    with pytest.raises(RuntimeError):
        f.control(STATES, 2.0, OBS, peers="plan")
    with pytest.raises(RuntimeError):
        f.rollout(STATES, 2.0, 5, obstacle_lists=OBS, peers="plan")
    with pytest.raises(ValueError):
        bare_fleet(_binding(), [_member(), _member()]).rollout(STATES, 2.0, 5, peers="plan")          # no obstacle_lists= and no such scenes resident


class _StubApi:
    """a binding that takes the calls of a device-tracked peers tick and answers with a fixed plan per member; it records what the plan upload was given"""
    has_fleet = has_fleet_peers = has_fleet_peers_plan = True

    def __init__(self, B, TT):
        self.B, self.T, self.uploads, self.tick = B, TT, [], 0
        self.lib = types.SimpleNamespace(rda_fleet_step_tracked=True)

    def _arr(self, p, dtype, n):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(dtype)), shape=(n,)).copy()

    def fleet_upload_scenes_peers_plan(self, h, counts, kind, nvert, geom, vel, st, ctl, plans, valid):
        self.uploads.append((self._arr(plans, C.c_double, self.B * 3 * (self.T + 1)).reshape(self.B, 3, self.T + 1), self._arr(valid, C.c_int, self.B)))
        return 0

    def fleet_upload_scenes_peers(self, *a):
        self.uploads.append(None)
        return 0

    def fleet_step_tracked(self, h, st, speed, cur, thr, rng, nom_u, out_u, out_s, info, ref, mi, eh):
        self.tick += 1
        s = np.ctypeslib.as_array(C.cast(out_s, C.POINTER(C.c_double)), shape=(self.B, 3, self.T + 1))
        for i in range(self.B):
            s[i] = 100.0 * self.tick + i
        return 0

    def failed(self, name, rc):
        return RuntimeError(name)


class _StubMember:
    """what Fleet._control_tracked and the peers checks use of an MPC member; `arrive_on`: the tick (1-based) on which it reports arrival"""
    def __init__(self, TT, arrive_on=None):
        self.receding, self.obstacle_order, self.rda_obstacle, self.device_obstacles, self.enable_reverse = TT, True, False, True, False
        self.car_tuple = types.SimpleNamespace(cone_type="Rpositive")
        self.cur_vel_array, self.state, self.cur_index, self.ticks, self.arrive_on, self.resets = np.zeros((2, TT)), np.zeros((3, 1)), 0, 0, arrive_on, 0
        E = 4
        self.rda = types.SimpleNamespace(has_scene=True, time_print=False, flatten_scene=lambda every: (len(every), np.zeros(0, np.int32), np.zeros(0, np.int32),
                                                                                                         np.zeros((0, E, 2)), np.zeros((0, 2))),
                                         pack_info=lambda ref_list, out_s, info, start: {"opt_state_list": out_s})

    def _tracks(self, kw):
        return True

    def _piece(self, state):
        self.state = state
        return [], 1

    def _sync_path(self, path):
        pass

    def _nominal_u(self):
        return None

    def _tracked_done(self, piece, u, info, mi, eh):
        self.ticks += 1
        info["arrive"] = self.arrive_on is not None and self.ticks >= self.arrive_on
        return u[:, 0:1], info

    def reset(self):
        self.resets += 1


def test_plan_bookkeeping():
    """a member's plan counts from its first tick through the fleet, holds its last opt_state_list, and stops counting on arrival and on reset"""
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd._capi import Info
    B, TT = 3, 5
    f = Fleet.__new__(Fleet)
    f.members, f.api, f._handle = [_StubMember(TT), _StubMember(TT, arrive_on=2), _StubMember(TT)], _StubApi(B, TT), None
    f._in_u, f._ref = np.zeros((B, 2, TT)), np.zeros((B, 3, TT + 1))
    f._out_u, f._out_s, f._info = np.zeros((B, 2, TT)), np.zeros((B, 3, TT + 1)), (Info * B)()
    f.batched_ticks, f._peers_staged = 0, False
    states = [np.zeros((3, 1))] * B
    assert not f.plan_valid.any()
    f.control(states, 2.0, [[], [], []], peers="plan")
    plans, valid = f.api.uploads[-1]
    assert not valid.any() and not plans.any()                         # before the first tick: nobody has a plan
    assert f.plan_valid.tolist() == [True, True, True]
    f.control(states, 2.0, [[], [], []], peers="plan")
    plans, valid = f.api.uploads[-1]
    assert valid.tolist() == [1, 1, 1] and [plans[i, 0, 0] for i in range(B)] == [100.0, 101.0, 102.0]       # the opt_state_list of tick 1
    assert f.plan_valid.tolist() == [True, False, True]                # member 1 arrived on tick 2
    f.reset([2])
    assert f.members[2].resets == 1 and f.members[0].resets == 0 and f.plan_valid.tolist() == [True, False, False]
    f.control(states, 2.0, [[], [], []], peers="plan")
    plans, valid = f.api.uploads[-1]
    assert valid.tolist() == [1, 0, 0] and plans[0, 2, 3] == 200.0
    f.control(states, 2.0, [[], [], []], peers=True)                   # the constant-velocity mode keeps the books too
    assert f.api.uploads[-1] is None and f._plans[0, 0, 0] == 400.0 and f.plan_valid.tolist() == [True, False, True]
    f.reset()
    assert not f.plan_valid.any() and [m.resets for m in f.members] == [1, 1, 2]
