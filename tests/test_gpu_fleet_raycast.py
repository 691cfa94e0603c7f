"""-m gpu : the simulated sensor on the device (rda_fleet_upload_worlds, rda_fleet_raycast, lidar::k_raycast_fleet; Fleet.upload_worlds / Fleet.raycast) against
its specification, World.get_lidar_scan, run in numpy on the same poses, sensors and obstacles (tests/lidar_world_lib.py numpy_scan).

Tolerance: 1e-9 m on every beam.  The two sides evaluate the same expressions; they differ in the last bits of sin / cos of the beam direction (and in whether
a dot product is fused).  The numpy scan's sensitivity to the heading on these scenes is at most 5e-8 m per 1e-9 rad, so 1e-16 rad of trigonometric error is
about 1e-14 m: 1e-9 leaves five decades.  A beam may be left out only where the numpy range ITSELF moves by more than 1e-6 m when the heading is shifted by
+-1e-9 rad - a silhouette beam, which grazes a corner or a circle - and at most one per scan (on these scenes the reference has none).

Scenes: the three lanes of tests/test_gpu_fleet_rollout_moving.py (7 obstacles per member: polygons, circles and polygons, polygons) at 13 poses each with
the three sensors of the lidar rollout's test; a 70-obstacle world - more than one LDS tile of 32 - with 360 and with 64 beams; a 1-beam sensor; an empty
world; a member with 0 beams; range_min clipping; a pose inside a circle."""
import ctypes as C

import numpy as np
import pytest

from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import dptr, iptr

from fleet_twin_lib import solver
from lidar_world_lib import SENSORS, WE, flatten, lane, numpy_scan, sensor_c

pytestmark = pytest.mark.gpu

RDA_ERR_ARG, RDA_ERR_UNSUPPORTED, RDA_ERR_HIP = -1, -2, -3
TOL = 1e-9


class Sim:
    """a fleet of the three lane members (fresh handles, nothing staged) and its worlds"""
    def __init__(self, hip):
        self.hip, self.B = hip, 3
        self.svs = [solver(hip, e, scene=False)[0] for e in range(3)]
        self.F = C.c_void_p()
        assert hip.fleet_create((C.c_void_p * 3)(*[s._be.handle for s in self.svs]), 3, C.byref(self.F)) == 0

    def close(self):
        self.hip.fleet_destroy(self.F)

    def upload(self, worlds, **over):
        """rda_fleet_upload_worlds of three obstacle lists -> rc; over: arguments replaced (None = a missing array)"""
        flat = [flatten(w) for w in worlds]
        a = dict(counts=np.array([len(w) for w in worlds], np.int32), we=WE)
        for j, key in enumerate(("kind", "nvert", "geom", "vel")):
            a[key] = np.ascontiguousarray(np.concatenate([f[j] for f in flat]))
        a.update(over)
        return self.hip.fleet_upload_worlds(self.F, iptr(a["counts"]), a["we"], iptr(a["kind"]), iptr(a["nvert"]), dptr(a["geom"]), dptr(a["vel"]))

    def cast(self, poses, sensors, **over):
        """rda_fleet_raycast -> (rc, [ranges of member i]); the output lies on a NaN ground with a guard entry behind it"""
        nb, lo, hi, rmin, rmax = sensor_c(sensors)
        a = dict(n_beams=nb, angle_min=lo, angle_max=hi, range_min=rmin, range_max=rmax, states=np.ascontiguousarray(np.array(poses, float).reshape(3, 3)),
                 ranges=np.full(int(np.maximum(nb, 0).sum()) + 1, np.nan))
        a.update(over)
        rc = self.hip.fleet_raycast(self.F, iptr(a["n_beams"]), dptr(a["angle_min"]), dptr(a["angle_max"]), dptr(a["range_min"]), dptr(a["range_max"]),
                                    dptr(a["states"]), dptr(a["ranges"]))
        out = a["ranges"]
        if rc == 0 and out is not None:
            assert np.isnan(out[-1])                                       # nothing written behind the last member's scan
            return rc, np.split(out[:-1], np.cumsum(nb)[:-1])
        return rc, None


@pytest.fixture(scope="module")
def sim(hip):
    s = Sim(hip)
    yield s
    s.close()


def agree(got, state, sensor, obstacles, what):
    """one scan against World.get_lidar_scan: every beam within TOL but at most one silhouette beam; returns (largest difference, hits, beams left out)"""
    want = np.asarray(numpy_scan(state, sensor, obstacles)["ranges"], float)
    assert got.shape == want.shape, what
    if want.size == 0:
        return 0.0, 0, 0
    diff = np.abs(got - want)
    out = np.flatnonzero(~(diff <= TOL))
    if out.size:
        shifted = [np.asarray(numpy_scan([state[0], state[1], state[2] + d], sensor, obstacles)["ranges"], float) for d in (-1e-9, 1e-9)]
        moves = np.maximum(np.abs(shifted[0] - want), np.abs(shifted[1] - want))
        assert out.size <= 1 and np.all(moves[out] > 1e-6), (what, out, diff[out], moves[out])
        diff[out] = 0.0
    assert np.all(got >= sensor["range_min"]) and np.all(got <= sensor["range_max"]), what
    return float(diff.max()), int((want < sensor["range_max"]).sum()), int(out.size)


def big_world():
    """70 obstacles on a ring of 4 .. 14 m about (20, 20): circles and polygons of 3 and 4 vertices"""
    rng = np.random.default_rng(sc.SEED + 7)
    out = []
    for j in range(70):
        d, a = rng.uniform(4.0, 14.0), rng.uniform(-np.pi, np.pi)
        cx, cy = 20.0 + d * np.cos(a), 20.0 + d * np.sin(a)
        out.append(sc.circle(cx, cy, float(rng.uniform(0.2, 0.6))) if j % 3 == 0 else sc.regular_polygon(cx, cy, 3 + j % 2, float(rng.uniform(0.3, 0.8)), 0.1 * j))
    return out


def test_lanes_at_13_poses_against_get_lidar_scan(sim):
    worlds = [lane(e)[1] for e in range(3)]
    assert sim.upload(worlds) == 0
    worst, hits, left, beams = 0.0, 0, 0, 0
    for p in range(13):
        states = [[4.0 + 0.4 * p, 20.0 + 8.0 * e + 0.05 * (p % 3 - 1), 0.03 * (p - 6) * (1 + e)] for e in range(3)]
        rc, got = sim.cast(states, SENSORS)
        assert rc == 0
        for e in range(3):
            w, h, o = agree(got[e], states[e], SENSORS[e], worlds[e], (p, e))
            worst, hits, left, beams = max(worst, w), hits + h, left + o, beams + got[e].size
    print(f"lanes: {beams} beams, {hits} hits, largest |device - numpy| = {worst:.3e} m, {left} silhouette beams left out")
    assert beams == 13 * (100 + 257 + 64) and hits > 1000


def test_tiles_single_beam_empty_world_and_no_beams(sim):
    big = big_world()
    full = dict(number=360, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=15.0)
    few = dict(full, number=64)
    one = dict(full, number=1, angle_min=0.3, angle_max=1.2)                 # a single beam looks along angle_min
    none = dict(full, number=0)
    states = [[20.0, 20.0, 0.4], [19.0, 21.5, -2.0], [20.5, 19.0, 1.0]]
    assert sim.upload([big, big, big]) == 0
    rc, got = sim.cast(states, [full, few, one])
    assert rc == 0
    worst = [agree(got[i], states[i], s, big, i) for i, s in enumerate((full, few, one))]
    assert worst[0][1] > 200 and worst[1][1] > 30                            # most beams of a full turn end on one of the 70
    assert got[2].shape == (1,)
    assert sim.upload([big, [], big]) == 0                                   # member 1: an empty world; member 2: no beams
    rc, got = sim.cast(states, [few, full, none])
    assert rc == 0 and got[2].size == 0
    agree(got[0], states[0], few, big, "few")
    assert np.array_equal(got[1], np.full(360, 15.0))                        # range_max everywhere
    assert sim.upload([[], [], []]) == 0                                     # no obstacle at all
    rc, got = sim.cast(states, [few, one, none])
    assert rc == 0 and np.array_equal(got[0], np.full(64, 15.0)) and np.array_equal(got[1], [15.0])
    print("70 obstacles:", [f"{w[0]:.3e}" for w in worst])


def test_range_min_clipping_and_the_inside_a_circle_quirk(sim):
    near = [sc.circle(22.0, 20.0, 0.5), sc.regular_polygon(20.0, 23.0, 4, 0.8, 0.2), sc.circle(20.0, 20.0, 1.5)]
    sensor = dict(number=181, angle_min=-np.pi, angle_max=np.pi, range_min=2.0, range_max=8.0)
    inside = [20.3, 20.2, 0.1]                                               # inside the third circle: it is not seen, the other two are
    outside = [17.0, 20.0, 0.0]
    states = [inside, outside, inside]
    assert sim.upload([near, near, near[:2]]) == 0
    rc, got = sim.cast(states, [sensor, sensor, dict(sensor, range_min=0.0)])
    assert rc == 0
    for i, (st, se, w) in enumerate(zip(states, [sensor, sensor, dict(sensor, range_min=0.0)], [near, near, near[:2]])):
        agree(got[i], st, se, w, i)
    assert got[0].min() == 2.0 and (got[2] < 2.0).any()                      # hits nearer than range_min are reported at range_min
    clipped = np.clip(got[2], 2.0, 8.0)
    assert np.array_equal(got[0], clipped)                                   # the circle about the sensor changes nothing
    assert got[1][90] == 2.0                                                 # from outside it is seen: straight ahead at 1.5 m, reported at range_min


def test_refusals(hip, sim):
    worlds = [lane(e)[1] for e in range(3)]
    states = [[4.0, 20.0 + 8.0 * e, 0.0] for e in range(3)]
    fresh = Sim(hip)
    assert fresh.cast(states, SENSORS)[0] == RDA_ERR_ARG                     # no uploaded world
    fresh.close()
    assert sim.upload(worlds) == 0
    rc, before = sim.cast(states, SENSORS)
    assert rc == 0

    def world_kept():
        rc, now = sim.cast(states, SENSORS)
        assert rc == 0 and all(np.array_equal(x, y) for x, y in zip(now, before))
    # the world's argument rules: each refusal leaves the old world where it was
    other = [worlds[1], worlds[2], worlds[0]]
    assert sim.upload(other, counts=np.array([7, -1, 7], np.int32)) == RDA_ERR_ARG
    for key in ("counts", "kind", "nvert", "geom"):
        assert sim.upload(other, **{key: None}) == RDA_ERR_ARG, key
    for we in (2, 9):
        assert sim.upload(other, we=we) == RDA_ERR_ARG, we
    for bad in (2, WE + 1):
        nv = np.concatenate([flatten(w)[1] for w in other]); nv[np.flatnonzero(nv)[0]] = bad
        assert sim.upload(other, nvert=nv) == RDA_ERR_ARG, bad
    kd = np.concatenate([flatten(w)[0] for w in other]); kd[3] = 2
    assert sim.upload(other, kind=kd) == RDA_ERR_ARG
    world_kept()
    # a refused allocation
    rc, n = RDA_ERR_HIP, 0
    while rc == RDA_ERR_HIP and n < 40:
        hip.debug_alloc_fail(n)
        try:
            rc = sim.upload(other)
        finally:
            hip.debug_alloc_fail(-1)
        if rc == RDA_ERR_HIP:
            world_kept()
        n += 1
    assert rc == 0 and n - 1 >= 13, (rc, n)
    rc, now = sim.cast(states, SENSORS)
    assert rc == 0 and not np.array_equal(now[0], before[0])                 # the new world is in
    assert sim.upload(worlds, vel=None) == 0                                 # a standing world: no velocities
    world_kept()
    assert sim.upload([[], [], []], kind=None, nvert=None, geom=None, vel=None) == 0      # nothing to read: the arrays may be missing
    assert sim.upload(worlds) == 0
    # the sensor's argument rules
    nb = sensor_c(SENSORS)[0]
    neg = nb.copy(); neg[1] = -1
    assert sim.cast(states, SENSORS, n_beams=neg)[0] == RDA_ERR_ARG
    many = nb.copy(); many[2] = 4097
    assert sim.cast(states, SENSORS, n_beams=many)[0] == RDA_ERR_UNSUPPORTED
    for key in ("n_beams", "angle_min", "angle_max", "range_min", "range_max", "states", "ranges"):
        assert sim.cast(states, SENSORS, **{key: None})[0] == RDA_ERR_ARG, key
    assert hip.fleet_raycast(None, iptr(nb), *([dptr(np.zeros(3))] * 4), dptr(np.zeros(9)), dptr(np.zeros(500))) == RDA_ERR_ARG
    world_kept()
    wide = [dict(SENSORS[0], number=4096), SENSORS[1], SENSORS[2]]          # the largest scan there is
    rc, got = sim.cast(states, wide)
    assert rc == 0
    agree(got[0], states[0], wide[0], worlds[0], "4096 beams")


def test_python_raycast_feeds_control(hip):
    """Fleet.upload_worlds / Fleet.raycast: the scan dicts of World.get_lidar_scan, taken by Fleet.control(scans=) as they are"""
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    from fleet_twin_lib import DT, E, ITER, MARGIN, N, SPEED, T, car
    ms, worlds, states = [], [], []
    for e in range(3):
        path, scene = lane(e)
        ms.append(MPC(car(e), [p.copy() for p in path], receding=T, sample_time=DT, iter_num=ITER, max_edge_num=E, max_obs_num=N, goal_index_threshold=MARGIN))
        worlds.append(scene); states.append(path[0].copy())
    f = Fleet(ms)
    with pytest.raises(RuntimeError, match="upload_worlds"):
        f.raycast(states, SENSORS)
    f.upload_worlds(worlds)
    lidars = [SENSORS[0], dict(SENSORS[1]), __import__("types").SimpleNamespace(**SENSORS[2])]      # mappings and a World.lidar-like object
    scans = f.raycast(states, lidars)
    for e, s in enumerate(scans):
        want = numpy_scan(states[e], SENSORS[e], worlds[e])
        assert set(s) == set(want)
        assert np.abs(s["ranges"] - want["ranges"]).max() <= TOL
        assert all(s[k] == want[k] for k in want if k != "ranges"), e
    res = f.control([s.copy() for s in states], SPEED, scans=scans)
    assert all(np.isfinite(u).all() and info["iters"] >= 1 for u, info in res)
    f.close()
