"""Fleet rollout over gear pieces (rda_upload_path_pieces, rda_fleet_rollout_gears, rda_fleet_rollout_last_pieces, Fleet.rollout(gears=True),
scenarios.gear_path): what can be checked without a GPU - the entry points are declared, exported, documented and bound with the header's argument lists,
a null fleet or handle is an argument error, the Python interface refuses what it does not support before any library call, and gear_path makes the
pieces MPC.split_path is expected to cut."""
import ctypes as C

import numpy as np
import pytest

from capi_lib import RDA_ERR_ARG, Binding, bare_fleet, declared, header_argtypes, integration_rows, lib, member

NAMES = ("rda_upload_path_pieces", "rda_fleet_rollout_gears", "rda_fleet_rollout_last_pieces")


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_documented(name):
    assert declared(name), name
    assert hasattr(lib(), name), f"{name} declared in include/rda_hip.h but not exported"
    row = integration_rows(name, table=False)
    assert row and any("mpc.py:166-187" in ln or "mpc.py:232-249" in ln for ln in row)      # mapped to the reference's piece rule / split_path


@pytest.mark.parametrize("name,nargs", [("rda_upload_path_pieces", 5), ("rda_fleet_rollout_gears", 19), ("rda_fleet_rollout_last_pieces", 3)])
def test_ctypes_prototype_follows_the_header(name, nargs):
    from rda_planner_amd._capi import CApi, PROTOTYPES, signature
    api = CApi(lib(), "rda")
    assert api.has_fleet_rollout_gears
    fn = getattr(api, name[len("rda_"):])
    want = header_argtypes(name)
    assert len(want) == nargs
    assert list(fn.argtypes) == want and fn.restype is C.c_int
    assert signature(PROTOTYPES[name[len("rda_"):]]) == (C.c_int, want)


def test_null_fleet_or_handle_is_an_argument_error_without_a_device():
    from rda_planner_amd._capi import CApi, Info, dptr, iptr
    api = CApi(lib(), "rda")
    K, B = 2, 1
    st, sp, cur, p0 = np.zeros((B, 3)), np.ones(B), np.zeros(B, np.int32), np.zeros(B, np.int32)
    sl, ul, il, arr, info = np.zeros((K + 1, B, 3)), np.zeros((K, B, 2)), np.zeros((K, B), np.int32), np.zeros(B, np.int32), (Info * (K * B))()
    pl = np.zeros((K, B), np.int32)
    assert api.fleet_rollout_gears(None, K, dptr(st), dptr(sp), iptr(p0), iptr(cur), 0.1, 10, 1, 1, 0, None, dptr(sl), dptr(ul), iptr(il), info, iptr(arr),
                                   iptr(pl), None) == RDA_ERR_ARG
    assert api.fleet_rollout_last_pieces(None, iptr(p0), dptr(np.zeros(B))) == RDA_ERR_ARG
    assert api.upload_path_pieces(None, 1, iptr(np.ones(1, np.int32)), dptr(np.ones(1)), dptr(np.zeros((1, 3)))) == RDA_ERR_ARG


def test_python_refusals_before_any_library_call():
    f = bare_fleet(Binding(), [member(), member(reverse=True)])         # no device: a binding that fails on any use
    states = [np.zeros((3, 1)), np.zeros((3, 1))]
    sensor = dict(number=8, angle_min=-1.0, angle_max=1.0, range_min=0.0, range_max=5.0)
    with pytest.raises(ValueError):
        f.rollout(states, 3.0, 5, gears=True, peers=True)
    with pytest.raises(ValueError):
        f.rollout(states, 3.0, 5, gears=True, peers="plan")
    with pytest.raises(ValueError):
        f.rollout(states, 3.0, 5, gears=True, lidar=[sensor, sensor])
    with pytest.raises(ValueError):
        f.rollout(states, 3.0, 5, gears=True, scans=[{}, {}])
    f.members = [member(reverse=True), member(reverse=True, tracks=False)]
    with pytest.raises(RuntimeError):
        f.rollout(states, 3.0, 5, gears=True)          # a member that does not track on the device
    f.members = [member(), member(reverse=True)]
    with pytest.raises(RuntimeError):
        f.rollout(states, 3.0, 5)                      # without gears=True a reverse member is refused as before
    with pytest.raises(RuntimeError):
        f.rollout(states, 3.0, 5, gears=False)


def test_gear_path_against_split_path():
    """piece count, lengths and gear flags of what MPC.split_path cuts from gear_path's waypoints; headings: the nose, not the direction of travel"""
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.mpc import MPC
    path = sc.gear_path([((4, 20), (7, 20), 1), ((7, 20), (5, 20), -1), ((5, 20), (5, 21), -1), ((5, 21), (6.5, 21), 1)], 0.1)
    assert all(p.shape == (4, 1) for p in path)
    parts = MPC.split_path(None, path)
    assert [len(p) for p in parts] == [31, 21 + 11, 16]
    assert [[float(w[3, 0]) for w in p] for p in parts] == [[1.0] * 31, [-1.0] * 32, [1.0] * 16]
    assert all(w[2, 0] == 0.0 for w in parts[0] + parts[1][:21] + parts[2])
    assert np.allclose([w[2, 0] for w in parts[1][21:]], -np.pi / 2)              # backing up in +y: the nose points to -y
    assert np.allclose(np.hstack(parts[1][:21])[0], np.linspace(7, 5, 21)) and np.allclose(np.hstack(parts[2])[0], np.linspace(5, 6.5, 16))
    fwd = sc.line_path([0, 0, 0], [8, 0, 0], 0.1)      # the path tests/test_gpu_track.py builds by hand
    back = sc.line_path([8, 0, 0], [2, 0, 0], 0.1)
    hand = [np.vstack((p[0:3], [[1.0]])) for p in fwd] + [np.vstack((p[0:2], [[0.0]], [[-1.0]])) for p in back]
    made = sc.gear_path([((0, 0), (8, 0), 1), ((8, 0), (2, 0), -1)], 0.1)
    assert len(made) == len(hand) and all(np.array_equal(a, b) for a, b in zip(made, hand))
    with pytest.raises(ValueError):
        sc.gear_path([((0, 0), (1, 0), 0)])
