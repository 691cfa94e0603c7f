"""-m gpu : the simulated sensor of a fleet whose members see each other (rda_fleet_raycast_peers, lidar::k_raycast_fleet_peers; Fleet.raycast_peers).

1  bit-identity with the blind kernel: the members are staged with rda_fleet_upload_scenes_peers at the same states, every member's peer rows are read back
   (rda_debug_scene_geom) and appended to its world as polygons; rda_fleet_raycast on those worlds must equal rda_fleet_raycast_peers on the original
   worlds for equality.  That pins the row -> member mapping (j < i / j > i), the footprint expressions (those of scene::k_peers_fleet) and the shared
   edge test.
2  the specification: World.get_lidar_scan in numpy on world_i + scenarios.peer_footprints(cars, states, i), 1e-9 m per beam, by the rule of
   tests/test_gpu_fleet_raycast.py (`agree`): a beam may be left out only where the numpy range itself moves by more than 1e-6 m under a +-1e-9 rad heading
   shift, at most one per scan.  The poses are chosen so that the numpy side alone has at most one such beam per scan; `silhouettes` checks that here.
   The error budget is that file's: same expressions, the device's cos / sin of the beam direction and of the peers' headings within a few ulp, a
   footprint vertex so within 1e-14 m, the range's sensitivity to either below 1e5 away from silhouettes.
3  34 members, 33 peers: more than one LDS tile of 32; member 0's second tile holds member 33, which stands next to it.
4  a fleet of one is rda_fleet_raycast; a member never sees itself; beams that miss read range_max.
5  refusals, the world untouched.

Shapes: rectangle robots 4.6 x 1.6 m (Ackermann with the rear axle as origin, differential and omni about the centre); scans of 65 beams (a partial
second workgroup) and of 1 beam; worlds of 4, 0 and 3 obstacles."""
import ctypes as C

import numpy as np
import pytest

from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import dptr, iptr

from lidar_world_lib import WE, flatten, numpy_scan, sensor_c

pytestmark = pytest.mark.gpu

RDA_ERR_ARG, RDA_ERR_UNSUPPORTED = -1, -2
TOL = 1e-9
T, N, E, ITER, DT = 8, 4, 4, 2, 0.1
DYN = ("acker", "diff", "omni")
FULL = dict(number=65, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=12.0)
ONE = dict(number=1, angle_min=0.5, angle_max=1.2, range_min=0.0, range_max=12.0)         # a single beam looks along angle_min
LINE = dict(number=64, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=120.0)
# three members near each other at several headings; in the last set member 1 stands inside member 0's footprint and member 0's origin inside member 1's
POSES = [[[10.0, 10.0, 0.3], [16.0, 11.0, 1.9], [12.0, 16.0, -2.4]],
         [[10.5, 9.5, -1.2], [15.0, 12.0, 0.4], [11.0, 15.0, 2.9]],
         [[9.0, 11.0, 2.2], [16.5, 10.0, -0.7], [13.0, 16.5, 0.05]],
         [[10.0, 10.0, 0.3], [10.8, 10.3, 1.2], [12.0, 16.0, -2.4]]]
SENSOR_SETS = [[FULL, FULL, ONE], [ONE, FULL, FULL], [FULL, ONE, FULL], [FULL, FULL, ONE]]


def car(e):
    return sc.rectangle_robot(dynamics=DYN[e % 3], wheelbase=3.0 if DYN[e % 3] == "acker" else 0)


def worlds3():
    return [[sc.circle(14.0, 8.0, 0.7), sc.regular_polygon(7.0, 12.0, 3, 0.9, 0.2), sc.regular_polygon(12.0, 5.5, 4, 0.8, 0.5), sc.circle(6.0, 7.0, 0.5)],
            [],
            [sc.regular_polygon(15.0, 18.0, 4, 1.0, 0.1), sc.circle(9.0, 18.0, 0.6), sc.regular_polygon(17.0, 13.0, 3, 0.8, 1.0)]]


def line_fleet():
    """34 differential robots across a line of 3 m slots along y = 20, member 0 in slot 0, member 33 in slot 1, members 1 .. 32 behind them"""
    cars = [sc.rectangle_robot(dynamics="diff", wheelbase=0) for _ in range(34)]
    slot = [0] + list(range(2, 34)) + [1]
    states = [[5.0 + 3.0 * slot[j], 20.0 + 0.3 * (j % 3), 1.2 + 0.02 * j] for j in range(34)]
    return cars, states


def silhouettes(state, sensor, obstacles):
    """beams of the numpy scan that move by more than 1e-6 m when the heading is shifted by +-1e-9 rad"""
    want = np.asarray(numpy_scan(state, sensor, obstacles)["ranges"], float)
    shifted = [np.asarray(numpy_scan([state[0], state[1], state[2] + d], sensor, obstacles)["ranges"], float) for d in (-1e-9, 1e-9)]
    return want, np.maximum(np.abs(shifted[0] - want), np.abs(shifted[1] - want)) > 1e-6


def agree(got, state, sensor, obstacles, what):
    """one scan against the specification: every beam within TOL but at most one silhouette beam (tests/test_gpu_fleet_raycast.py); the numpy side alone
    stays within that cap -> (largest difference, beams that hit, beams left out)"""
    want, sil = silhouettes(state, sensor, obstacles)
    assert sil.sum() <= 1, (what, np.flatnonzero(sil))                       # the choice of poses, checked on the CPU
    assert got.shape == want.shape, what
    diff = np.abs(got - want)
    out = np.flatnonzero(~(diff <= TOL))
    assert out.size <= 1 and np.all(sil[out]), (what, out, diff[out])
    diff[out] = 0.0
    assert np.all(got >= sensor["range_min"]) and np.all(got <= sensor["range_max"]), what
    return float(diff.max()), int((want < sensor["range_max"]).sum()), int(out.size)


class Sim:
    """a fleet of fresh handles of the given robots (nothing staged) and its worlds"""
    def __init__(self, hip, cars, t=T):
        from rda_planner_amd.rda_solver import RDA_solver
        self.hip, self.B, self.cars = hip, len(cars), cars
        self.svs = [RDA_solver(t, c, E, N, iter_num=ITER, step_time=DT, time_print=False) for c in cars]
        self.F = C.c_void_p()
        assert hip.fleet_create((C.c_void_p * self.B)(*[s._be.handle for s in self.svs]), self.B, C.byref(self.F)) == 0

    def close(self):
        self.hip.fleet_destroy(self.F)

    def upload(self, worlds):
        flat = [flatten(w) for w in worlds]
        counts = np.array([len(w) for w in worlds], np.int32)
        kind, nvert, geom, vel = (np.ascontiguousarray(np.concatenate([f[j] for f in flat])) for j in range(4))
        return self.upload_flat(counts, kind, nvert, geom)

    def upload_flat(self, counts, kind, nvert, geom):
        return self.hip.fleet_upload_worlds(self.F, iptr(counts), WE, iptr(kind), iptr(nvert), dptr(np.ascontiguousarray(geom)), None)

    def world(self):
        n, we = np.zeros(1, np.int32), np.zeros(1, np.int32)
        assert self.hip.debug_fleet_world(self.F, None, iptr(n), iptr(we)) == 0
        g = np.full((max(int(n[0]), 1), WE, 2), np.nan)
        assert self.hip.debug_fleet_world(self.F, dptr(g), iptr(n), iptr(we)) == 0 and (n[0] == 0 or we[0] == WE)
        return g[:n[0]]

    def cast(self, poses, sensors, peers, **over):
        """rda_fleet_raycast_peers (peers) | rda_fleet_raycast -> (rc, [ranges of member i]); the output lies on a NaN ground with a guard entry behind it"""
        nb, lo, hi, rmin, rmax = sensor_c(sensors)
        a = dict(n_beams=nb, angle_min=lo, angle_max=hi, range_min=rmin, range_max=rmax, states=np.ascontiguousarray(np.array(poses, float).reshape(self.B, 3)),
                 ranges=np.full(int(np.maximum(nb, 0).sum()) + 1, np.nan))
        a.update(over)
        fn = self.hip.fleet_raycast_peers if peers else self.hip.fleet_raycast
        rc = fn(self.F, iptr(a["n_beams"]), dptr(a["angle_min"]), dptr(a["angle_max"]), dptr(a["range_min"]), dptr(a["range_max"]), dptr(a["states"]),
                dptr(a["ranges"]))
        out = a["ranges"]
        if rc == 0 and out is not None:
            assert np.isnan(out[-1])                                       # nothing written behind the last member's scan
            return rc, np.split(out[:-1], np.cumsum(nb)[:-1])
        return rc, None

    def peer_rows(self, poses):
        """the members staged with rda_fleet_upload_scenes_peers (no own obstacles) at `poses`; every member's peer rows [B - 1][E][2] read back"""
        st = np.ascontiguousarray(np.array(poses, float).reshape(self.B, 3))
        assert self.hip.fleet_upload_scenes_peers(self.F, iptr(np.zeros(self.B, np.int32)), None, None, None, None, dptr(st), dptr(np.zeros((self.B, 2)))) == 0
        rows = []
        for s in self.svs:
            g, n = np.full((self.B + 3, E, 2), np.nan), np.zeros(1, np.int32)
            assert self.hip.debug_scene_geom(s._be.handle, dptr(g), iptr(n)) == 0 and n[0] == self.B - 1
            rows.append(g[:n[0]].copy())
        return rows


@pytest.fixture(scope="module")
def sim(hip):
    s = Sim(hip, [car(e) for e in range(3)])
    yield s
    s.close()


def test_equals_the_blind_kernel_on_worlds_that_hold_the_peer_rows(sim):
    assert E == WE                                                           # a peer row is a world polygon as it stands
    flat = [flatten(w) for w in worlds3()]
    seen = 0
    for poses, sensors in zip(POSES, SENSOR_SETS):
        rows = sim.peer_rows(poses)
        counts = np.array([len(f[0]) + 2 for f in flat], np.int32)
        kind = np.concatenate([np.r_[f[0], np.zeros(2, np.int32)] for f in flat]).astype(np.int32)
        nvert = np.concatenate([np.r_[f[1], np.full(2, 4, np.int32)] for f in flat]).astype(np.int32)
        geom = np.concatenate([np.concatenate([f[2], r]) for f, r in zip(flat, rows)])
        assert sim.upload_flat(counts, kind, nvert, geom) == 0
        rc, want = sim.cast(poses, sensors, peers=False)
        assert rc == 0
        assert sim.upload(worlds3()) == 0
        rc, got = sim.cast(poses, sensors, peers=True)
        assert rc == 0
        rc, blind = sim.cast(poses, sensors, peers=False)
        assert rc == 0
        for i in range(3):
            assert np.array_equal(got[i], want[i]), (poses, i)
            seen += int((got[i] != blind[i]).sum())
        # the rows are where the specification puts them: member j's footprint in row j < i ? j : j - 1 of member i
        for i in range(3):
            for r, o in enumerate(sc.peer_footprints(sim.cars, poses, i)):
                assert np.abs(rows[i][r] - o.vertex.T).max() <= 1e-12, (i, r)
    print("beams that end on a peer:", seen)
    assert seen > 40


def test_against_get_lidar_scan_on_the_world_and_the_peer_footprints(sim):
    worlds = worlds3()
    assert sim.upload(worlds) == 0
    worst, hits, left, beams = 0.0, 0, 0, 0
    for p, (poses, sensors) in enumerate(zip(POSES, SENSOR_SETS)):
        rc, got = sim.cast(poses, sensors, peers=True)
        assert rc == 0
        for i in range(3):
            w, h, o = agree(got[i], poses[i], sensors[i], worlds[i] + sc.peer_footprints(sim.cars, poses, i), (p, i))
            worst, hits, left, beams = max(worst, w), hits + h, left + o, beams + got[i].size
    print(f"{beams} beams, {hits} hits, largest |device - numpy| = {worst:.3e} m, {left} silhouette beams left out")
    assert beams == 4 * (65 + 65 + 1) and hits > 150
    # a footprint that contains the origin is hit from the inside: every beam of member 1 in the last set ends within its neighbour
    rc, got = sim.cast(POSES[3], [FULL, FULL, FULL], peers=True)
    assert rc == 0 and got[1].max() < 4.0 and got[0].max() < 4.0


def test_more_peers_than_one_tile(hip):
    cars, states = line_fleet()
    s = Sim(hip, cars)
    worlds = [[sc.circle(8.0, 26.0, 0.8)]] + [[] for _ in range(33)]
    assert s.upload(worlds) == 0
    rc, got = s.cast(states, [LINE] * 34, peers=True)
    assert rc == 0
    worst = 0.0
    for i in range(34):
        worst = max(worst, agree(got[i], states[i], LINE, worlds[i] + sc.peer_footprints(cars, states, i), i)[0])
    # member 0: row 32, the one peer of the second tile, is member 33 - without it the scan is another one
    others = sc.peer_footprints(cars, states, 0)
    without = np.asarray(numpy_scan(states[0], LINE, worlds[0] + others[:32])["ranges"], float)
    on_33 = np.flatnonzero(np.abs(got[0] - without) > 1e-3)
    print(f"34 members: largest |device - numpy| = {worst:.3e} m; member 0's beams that end on member 33: {on_33.tolist()}")
    assert on_33.size >= 1 and np.all(got[0][on_33] < without[on_33])
    s.close()


def test_a_fleet_of_one_and_self_exclusion(hip, sim):
    one = Sim(hip, [car(0)])
    assert one.upload([worlds3()[0]]) == 0
    rc, a = one.cast([POSES[0][0]], [FULL], peers=True)
    rc2, b = one.cast([POSES[0][0]], [FULL], peers=False)
    assert rc == 0 and rc2 == 0 and np.array_equal(a[0], b[0]) and (a[0] < 12.0).any()
    one.close()
    # alone in an empty world among distant peers: no beam ends on the member's own footprint, the beams that miss read range_max
    far = [[10.0, 10.0, 0.3], [40.0, 12.0, 1.9], [8.0, 45.0, -2.4]]
    wide = dict(FULL, range_max=50.0)
    assert sim.upload([[], [], []]) == 0
    rc, got = sim.cast(far, [wide] * 3, peers=True)
    assert rc == 0
    for i in range(3):
        want = np.asarray(numpy_scan(far[i], wide, sc.peer_footprints(sim.cars, far, i))["ranges"], float)
        miss = want == 50.0
        assert np.array_equal(got[i][miss], want[miss]) and miss.sum() > 50 and (~miss).any() and got[i].min() > 20.0, i
        agree(got[i], far[i], wide, sc.peer_footprints(sim.cars, far, i), i)
    # the reach of the lidar: at 29 m member 0 still ends two beams on member 1, whose centre is 30.07 m away; at 25 m nobody is within reach of anybody
    for rmax, hits in ((29.0, 2), (25.0, 0)):
        short = dict(FULL, number=360, range_max=rmax)
        rc, got = sim.cast(far, [short] * 3, peers=True)
        assert rc == 0
        for i in range(3):
            agree(got[i], far[i], short, sc.peer_footprints(sim.cars, far, i), (rmax, i))
        assert (got[0] < rmax).sum() == hits and (hits or all(np.array_equal(g, np.full(360, rmax)) for g in got)), rmax


def test_refusals(hip, sim):
    poses, sensors = POSES[0], [FULL, FULL, ONE]
    fresh = Sim(hip, [car(e) for e in range(3)])
    assert fresh.cast(poses, sensors, peers=True)[0] == RDA_ERR_ARG          # no resident world
    fresh.close()
    assert sim.upload(worlds3()) == 0
    w0 = sim.world()
    rc, before = sim.cast(poses, sensors, peers=True)
    assert rc == 0
    nb = sensor_c(sensors)[0]
    many = nb.copy(); many[1] = 4097
    assert sim.cast(poses, sensors, peers=True, n_beams=many)[0] == RDA_ERR_UNSUPPORTED
    neg = nb.copy(); neg[0] = -1
    assert sim.cast(poses, sensors, peers=True, n_beams=neg)[0] == RDA_ERR_ARG
    for key in ("n_beams", "angle_min", "angle_max", "range_min", "range_max", "states", "ranges"):
        assert sim.cast(poses, sensors, peers=True, **{key: None})[0] == RDA_ERR_ARG, key
    assert hip.fleet_raycast_peers(None, iptr(nb), *([dptr(np.zeros(3))] * 4), dptr(np.zeros(9)), dptr(np.zeros(200))) == RDA_ERR_ARG
    assert np.array_equal(sim.world(), w0) and w0.shape == (7, WE, 2)
    rc, after = sim.cast(poses, sensors, peers=True)
    assert rc == 0 and all(np.array_equal(x, y) for x, y in zip(before, after))


def test_refused_allocations_of_a_first_seeing_cast_change_nothing(hip):
    """rda_fleet_raycast_peers on a fleet that has worlds but no peer table and no ranges yet makes both: refused at each of the 8 allocations in turn
    it returns RDA_ERR_HIP, holds nothing more than before and leaves the world as it was; the call that gets through returns the ranges of an
    undisturbed twin.  B = 3, T = 5, worlds of 3, 2 and 3 obstacles, 8 beams."""
    from fleet_twin_lib import refused_in_turn
    eight = dict(number=8, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=12.0)
    worlds = [worlds3()[0][:3], worlds3()[2][:2], worlds3()[2]]
    a, b = (Sim(hip, [car(e) for e in range(3)], t=5) for _ in range(2))
    assert a.upload(worlds) == 0 and b.upload(worlds) == 0
    w0, out = a.world(), {}

    def first():
        rc, out["ranges"] = a.cast(POSES[0], [eight] * 3, peers=True)
        assert np.array_equal(a.world(), w0)
        return rc
    rc, refused = refused_in_turn(hip, first)
    print("allocations of a fleet's first rda_fleet_raycast_peers:", refused)
    assert rc == 0 and refused == 8
    rc, want = b.cast(POSES[0], [eight] * 3, peers=True)
    assert rc == 0 and all(np.array_equal(x, y) for x, y in zip(out["ranges"], want))
    assert all(len(x) == 8 and np.all(np.isfinite(x)) for x in want)
    a.close(); b.close()


def test_python_raycast_peers(hip):
    """Fleet.raycast_peers: the scan dicts of Fleet.raycast, the ranges of the specification; Fleet.raycast itself stays blind"""
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    poses = POSES[0]
    ms = [MPC(car(e), sc.line_path(poses[e], [poses[e][0] + 20.0 * np.cos(poses[e][2]), poses[e][1] + 20.0 * np.sin(poses[e][2]), poses[e][2]], 0.1),
              receding=T, sample_time=DT, iter_num=ITER, max_edge_num=E, max_obs_num=N) for e in range(3)]
    f = Fleet(ms)
    worlds = worlds3()
    f.upload_worlds(worlds)
    states = [np.array(p, float).reshape(3, 1) for p in poses]
    seeing, blind = f.raycast_peers(states, [FULL] * 3), f.raycast(states, [FULL] * 3)
    for i in range(3):
        want = numpy_scan(poses[i], FULL, worlds[i] + sc.peer_footprints([m.car_tuple for m in ms], poses, i))
        assert set(seeing[i]) == set(want) == set(blind[i])
        agree(seeing[i]["ranges"], poses[i], FULL, worlds[i] + sc.peer_footprints([m.car_tuple for m in ms], poses, i), i)
        agree(blind[i]["ranges"], poses[i], FULL, worlds[i], i)
        assert (seeing[i]["ranges"] < blind[i]["ranges"]).any()
    f.close()
