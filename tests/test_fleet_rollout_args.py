"""The argument table of `Fleet.rollout` (fleet.ROLLOUT_ARGS) against the checked prototypes (_capi.PROTOTYPES, which tests/test_capi_symbols.py holds
against the header): every row, resolved with values of the Python kinds a call has, gives exactly the arguments its prototype declares, each of the kind
its letter says.  No device: an argument in the wrong place is found here and not only on a GPU."""
import ctypes as C

import numpy as np
import pytest

from rda_planner_amd import fleet
from rda_planner_amd._capi import PROTOTYPES, Info, c_double_p, c_int_p

B, K, T = 2, 2, 8
KIND = {"h": lambda a: isinstance(a, C.c_void_p),
        "i": lambda a: type(a) is int,
        "d": lambda a: type(a) is float,
        "D": lambda a: a is None or isinstance(a, c_double_p),
        "I": lambda a: a is None or isinstance(a, c_int_p),
        "N": lambda a: isinstance(a, C.Array) and a._type_ is Info}


def values():
    """one value per name of the table, as `Fleet.rollout` has them: arrays where a call may also pass None, flags as bool"""
    d, i = (lambda *shape: np.zeros(shape)), (lambda *shape: np.zeros(shape, np.int32))
    return dict(F=C.c_void_p(1), K=K, states=d(B, 3), speed=d(B), cur=i(B), piece0=i(B), threshold=0.1, ind_range=10, margin=1, resort=True, moving=False,
                nom_u=d(B, 2, T), ctl0=d(B, 2), sensors=(i(B), d(B), d(B), d(B), d(B)), scan_eps=2.0, scan_min_samples=6, order=i(B),
                logs=(d(K + 1, B, 3), d(K, B, 2), i(K, B), (Info * (K * B))(), i(B)), box_log=i(K, B), clearance_log=d(K, B), peer_log=d(K, B),
                piece_log=i(K, B), plans=(d(B, 3, T + 1), i(B)), see_peers=np.bool_(True), track_gate=1.0, track_window=8)


CHOICE = [(dict(), "fleet_rollout"), (dict(moving=True), "fleet_rollout_moving"), (dict(gears=True, moving=True), "fleet_rollout_gears"),
          (dict(peers=True, moving=True), "fleet_rollout_peers"), (dict(peers=True, plan=True, moving=True), "fleet_rollout_peers_plan"),
          (dict(sensors=(), moving=True), "fleet_rollout_lidar"), (dict(sensors=(), see_peers=True), "fleet_rollout_lidar_peers"),
          (dict(sensors=(), see_peers=True, track=True), "fleet_rollout_lidar_tracked"), (dict(sensors=(), track=True), "fleet_rollout_lidar_tracked")]


def test_rollout_argument_table_matches_the_prototypes():
    assert sorted(fleet.ROLLOUT_ARGS) == sorted(n for n in PROTOTYPES if n.startswith("fleet_rollout") and "_last" not in n)
    assert len(fleet.ROLLOUT_ARGS) == 8
    for entry in fleet.ROLLOUT_ARGS:
        letters = PROTOTYPES[entry].partition(" ")[2]
        args = fleet.rollout_args(entry, values())
        assert len(args) == len(letters), (entry, len(args), len(letters))
        for n, (a, letter) in enumerate(zip(args, letters)):
            assert KIND[letter](a), (entry, n, letter, a)
    with pytest.raises(KeyError):                               # an array of another type is no argument
        fleet.rollout_args("fleet_rollout", dict(values(), cur=np.zeros(B, np.int64)))
    for asked, entry in CHOICE:                                 # the entry is chosen from the options, every one of the eight
        o = fleet.RolloutOptions(**{**dict.fromkeys(fleet.RolloutOptions._fields, False), "sensors": None, **asked})
        assert fleet.rollout_entry(o) == entry, asked
    assert {e for _, e in CHOICE} == set(fleet.ROLLOUT_ARGS)
