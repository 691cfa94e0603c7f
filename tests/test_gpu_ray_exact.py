"""-m gpu : the ray casters of the simulated sensor, lidar::k_raycast_fleet (rda_fleet_raycast) and lidar::k_raycast_fleet_peers (rda_fleet_raycast_peers),
against exact ray casting (tests/ray_exact.py) on the pinned grid of tests/ray_grid.py - beams aimed at polygon vertices, at vertices split into two 1e-13 m
apart, at the footprint corners of other members, along and away from edges on the beam's own line, and generic scans - instead of against their own specification only.

Harness: three fresh handles in one fleet, rda_fleet_upload_worlds with a vertex stride of 8, then one ray-cast launch per grid launch; no solver step runs.
  1  k_raycast_fleet on the aimed, split-vertex, generic and collinear launches
  2  k_raycast_fleet_peers on the peers launches, and on the aimed and collinear worlds, where every member is out of every other's reach: the bits of the
     blind caster
Contract, both: every conditioned beam within ray_grid.DEVICE_BOUND = 1e-9 m of the exact range, where no aimed, split, peers or away beam and at most one
generic beam per scan is not conditioned (ray_grid's caps; the reference alone decides); a beam ALONG an edge, a silhouette, within 1e-9 m of the bracket
of its sheared neighbours' exact ranges; every beam within 1e-9 m of the fixed `World.get_lidar_scan`; no -0.0.

Measured on one MI355X (the tests print them), worst |device - exact| over the conditioned beams; only the 150 along beams are not conditioned:
  k_raycast_fleet         aimed 3.55e-15 m (900 beams), split 3.55e-15 m (180), away 0 (150), generic 6.13e-14 m (8026); along (150) at most 4.44e-15 m
                          outside their bracket; |device - specification| <= 2.40e-14 m
  k_raycast_fleet_peers   peers 4.44e-15 m (240 beams), generic 1.87e-14 m (2760); |device - specification| <= 8.88e-15 m; the aimed and collinear worlds
                          bit for bit
Time: test 1 0.11 s, test 2 0.20 s, and 2 s once for the grid with its exact ranges (shared with tests/test_ray_exact.py in one process)."""
import ctypes as C
import time

import numpy as np
import pytest

import ray_grid as grid
from lidar_world_lib import flatten, numpy_scan, sensor_c
from rda_planner_amd._capi import dptr, iptr

pytestmark = pytest.mark.gpu

T, N, E, ITER, DT = 8, 4, 4, 2, 0.1


class Sim:
    """a fleet of fresh handles of the grid's three robots (nothing staged) and its worlds"""
    def __init__(self, hip):
        from rda_planner_amd.rda_solver import RDA_solver
        self.hip = hip
        self.svs = [RDA_solver(T, c, E, N, iter_num=ITER, step_time=DT, time_print=False) for c in grid.cars()]
        self.F = C.c_void_p()
        assert hip.fleet_create((C.c_void_p * 3)(*[s._be.handle for s in self.svs]), 3, C.byref(self.F)) == 0

    def close(self):
        self.hip.fleet_destroy(self.F)

    def upload(self, worlds):
        flat = [flatten(w, we=grid.EMAX) for w in worlds]
        counts = np.array([len(w) for w in worlds], np.int32)
        kind, nvert, geom = (np.ascontiguousarray(np.concatenate([f[j] for f in flat])) for j in range(3))
        assert self.hip.fleet_upload_worlds(self.F, iptr(counts), grid.EMAX, iptr(kind), iptr(nvert), dptr(geom), None) == 0

    def cast(self, launch, peers):
        """the launch's worlds uploaded, then rda_fleet_raycast_peers (peers) | rda_fleet_raycast -> [ranges of member i]"""
        self.upload([s.obstacles for s in launch.scans])
        nb, lo, hi, rmin, rmax = sensor_c([s.sensor for s in launch.scans])
        states = np.ascontiguousarray(np.array([s.state for s in launch.scans], float).reshape(3, 3))
        out = np.full(int(nb.sum()) + 1, np.nan)
        fn = self.hip.fleet_raycast_peers if peers else self.hip.fleet_raycast
        assert fn(self.F, iptr(nb), dptr(lo), dptr(hi), dptr(rmin), dptr(rmax), dptr(states), dptr(out)) == 0
        assert np.isnan(out[-1]) and np.isfinite(out[:-1]).all()            # every beam written, nothing behind the last member's scan
        return np.split(out[:-1], np.cumsum(nb)[:-1])


@pytest.fixture(scope="module")
def sim(hip):
    s = Sim(hip)
    yield s
    s.close()


@pytest.fixture(scope="module")
def cases():
    return grid.build()


@pytest.fixture(scope="module")
def blind():
    return {}                                                              # id(launch) -> the blind caster's ranges, from test 1 for test 2


def held(sub, got, what):
    """the contract on the launches `sub` with the device's ranges got[id(launch)]; prints and returns the worst figures"""
    worst, count, left, most, outside = grid.figures(sub, lambda l: got[id(l)])
    spec = 0.0
    for l in grid.launches(sub):
        for i, s in enumerate(l.scans):
            want = np.asarray(numpy_scan(s.state, s.sensor, grid.seen_by(l, i))["ranges"], float)
            spec = max(spec, float(np.abs(got[id(l)][i] - want).max()))
            assert np.all(got[id(l)][i] >= s.sensor["range_min"]) and np.all(got[id(l)][i] <= s.sensor["range_max"])
    print(f"{what}: worst |device - exact| per class", {k: f"{v:.2e}" for k, v in worst.items()}, "beams", count, "left out", left,
          f"; worst |device - specification| {spec:.2e}; beams along an edge at most {outside:.2e} m outside their bracket")
    assert all(left.get(c, 0) == 0 for c in ("aimed", "split", "peers", "away")) and most <= 1
    assert outside <= grid.DEVICE_BOUND                                      # a silhouette beam along an edge: within the bracket of its sheared neighbours
    assert not any(np.signbit(r).any() for l in grid.launches(sub) for r in got[id(l)])      # no -0.0
    assert max(worst.values()) <= grid.DEVICE_BOUND == 1e-9
    assert spec <= grid.DEVICE_BOUND
    return worst, count


def test_blind_caster_on_the_aimed_split_and_generic_launches(sim, cases, blind):
    t0 = time.perf_counter()
    sub = {"aimed": cases["aimed"], "generic": cases["generic"], "collinear": cases["collinear"]}
    for l in grid.launches(sub):
        blind[id(l)] = sim.cast(l, peers=False)
    worst, count = held(sub, blind, "k_raycast_fleet")
    assert count["aimed"] >= 900 and count["split"] >= 180 and count["aimed"] + count["split"] >= 1000
    assert count["away"] >= 150 and count["along"] >= 150 and set(worst) == {"aimed", "split", "generic", "away"}
    print(f"time {time.perf_counter() - t0:.2f} s")


def test_seeing_caster_on_the_peers_launches_and_blind_bits_on_the_aimed_worlds(sim, cases, blind):
    t0 = time.perf_counter()
    sub = {"peers": cases["peers"]}
    got = {id(l): sim.cast(l, peers=True) for l in cases["peers"]}
    worst, count = held(sub, got, "k_raycast_fleet_peers")
    assert count["peers"] >= 200
    # the aimed worlds: the members stand more than 26 m apart and see 13 m, so every peer is dropped or missed - the blind caster's bits
    # (held to the exact range in test 1)
    for l in cases["aimed"] + cases["collinear"][:grid.COL_LAUNCHES]:        # (the pinned collinear scans stand within each other's reach)
        if id(l) not in blind:
            blind[id(l)] = sim.cast(l, peers=False)
        seeing = sim.cast(l, peers=True)
        assert all(np.array_equal(a, b) for a, b in zip(seeing, blind[id(l)]))
    print(f"time {time.perf_counter() - t0:.2f} s")
