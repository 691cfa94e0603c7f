"""-m gpu : rollout::k_clearance_fleet and rollout::k_peer_clearance_fleet (rda_fleet_clearance, rda_fleet_peer_clearance) against exact geometry
(tests/clear_exact.py) on the cases of the pinned grid (tests/clear_grid.py), and their reductions beyond one wave and one stride.  No solver step runs.
Handles as in tests/test_gpu_fleet_rollout_moving.py: T = 8, N = 4, iter_num = 2; E = 8 = RDA_EMAX.
  1  the contract of tests/clear_grid.py on the device, bound 1e-9 m (the project's bound for device geometry), and the device against the fixed
     scenarios.clearance within 1e-9 m.  A fleet takes members of ONE robot size (rda_fleet_create: equal R), so the 3-, 4- and 8-edge robots are three
     fleets of 3 members - the robot, the robot with the rows of G reversed (a clockwise footprint), the robot again - each member with a resident
     raw scene of 12 grid obstacles (8 polygons: both windings x with and without a repeated vertex, 3 .. 8 entries; 4 circles), evaluated at 20 poses:
     the 12 poses the grid drew for those obstacles and 8 of them displaced
  2  n = 300 obstacles, one near: at index 0, 63, 64, 255, 256, 299; then two near ones in different waves, the smaller one in each wave in turn
  3  B = 66 members 10 m apart, one pair brought to 0.3 m: (0, 1), (1, 64), (64, 65), (2, 65); B = 2 with a clockwise footprint
  4  a member without a scene reports +inf; a circle robot is refused
Before the winding, repeated-vertex and inside fixes test 1 failed on the clockwise, repeated-vertex and enclosed-circle cases.

Measured on an MI355X (the tests print every figure): |device - exact| <= 2.1e-14 m on 'overlap', 1.5e-14 on 'face', 4.5e-15 on 'inside', 2.4e-15 on
'outside', no excess on 'corner'; |device - specification| <= 1.5e-14 m; tests 2 and 3: 8.9e-16 m and 0.  Each test takes about 1 s."""
import ctypes as C

import numpy as np
import pytest

import clear_exact as ex
import clear_grid as grid
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import dptr, iptr

from fleet_twin_lib import bare_fleet, refused_in_turn
from fleet_twin_lib import hip          # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

T, N, E, ITER, DT = 8, 4, 8, 2, 0.1
RDA_ERR_UNSUPPORTED = -2
TOL = grid.DEVICE_BOUND
REACH = 2.5              # no robot of the grid reaches further from its origin (the car's corner: 2.44 m)


class Fleet:
    """fresh handles for `cars` in one fleet"""
    def __init__(self, hip, cars):
        from rda_planner_amd.rda_solver import RDA_solver
        self.hip, self.B, self.cars = hip, len(cars), cars
        self.svs = [RDA_solver(T, c, E, N, iter_num=ITER, step_time=DT, time_print=False) for c in cars]
        self.F = C.c_void_p()
        self.rc = hip.fleet_create((C.c_void_p * self.B)(*[s._be.handle for s in self.svs]), self.B, C.byref(self.F))

    def upload(self, scenes, states):
        """rda_fleet_upload_scenes of per-member lists of ('poly', V 2 x k) | ('circle', c, r), standing, ranked by distance from `states`"""
        counts = np.array([len(s) for s in scenes], np.int32)
        n = int(counts.sum())
        kind, nvert, geom, vel = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, E, 2)), np.zeros((n, 2))
        for i, o in enumerate(o for s in scenes for o in s):
            if o[0] == "circle":
                kind[i], geom[i, 0], geom[i, 1, 0] = 1, o[1], o[2]
            else:
                nvert[i] = o[1].shape[1]
                geom[i, :nvert[i]] = o[1].T
        rob = np.ascontiguousarray(np.asarray(states, float)[:, 0:2])
        assert self.hip.fleet_upload_scenes(self.F, iptr(counts), iptr(kind), iptr(nvert), dptr(geom), dptr(vel), dptr(rob), iptr(np.ones(self.B, np.int32))) == 0
        return geom

    def clearance(self, states):
        st, got = np.ascontiguousarray(states, float), np.full(self.B, np.nan)
        assert self.hip.fleet_clearance(self.F, dptr(st), dptr(got)) == 0
        return got

    def peer_clearance(self, states):
        st, got = np.ascontiguousarray(states, float), np.full(self.B, np.nan)
        assert self.hip.fleet_peer_clearance(self.F, dptr(st), dptr(got)) == 0
        return got

    def close(self):
        self.hip.fleet_destroy(self.F)


def as_obstacle(o):
    return sc.circle(o[1][0], o[1][1], o[2]) if o[0] == "circle" else sc.Obstacle(None, None, o[1], "Rpositive", np.zeros((2, 1)))


def exact_one(car, state, o):
    RV = ex.robot_polygon(car, state)
    return ex.signed_circle(RV, o[1], o[2]) if o[0] == "circle" else ex.signed_sep(RV, o[1])


def exact_scene(car, state, scene):
    """the exact values and classes of the obstacles that can be the nearest: an obstacle is left out when even a lower bound of its distance - centre
    distance minus both reaches - lies above the smallest value found"""
    xy = np.asarray(state, float)[0:2]

    def lower(o):
        if o[0] == "circle":
            return np.linalg.norm(np.asarray(o[1]) - xy) - o[2] - REACH
        c = o[1].mean(axis=1)
        return np.linalg.norm(c - xy) - np.linalg.norm(o[1] - c[:, None], axis=0).max() - REACH
    vals, classes, best = [], [], np.inf
    for lb, j in sorted((lower(o), j) for j, o in enumerate(scene)):
        if lb > best + 1e-3:
            break
        v, c = exact_one(car, state, scene[j])
        vals.append(v); classes.append(c)
        best = min(best, v)
    return vals, classes


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------------------
def device_cases(edges):
    """-> (cars [3], scenes [3][12], poses [20][3][3]) of the fleet of `edges`-edge robots, from the grid"""
    rob, polys, circles, _ = grid.build()
    first = {3: 0, 4: 2, 6: 4, 8: 6}[edges]
    members = [(first, 0), (first + 1, 0), (first, 1)]                      # (grid robot, which half of its cases)
    cars, scenes, poses = [], [], np.zeros((20, 3, 3))
    rng = np.random.default_rng(grid.SEED + 100 + edges)
    for m, (r, half) in enumerate(members):
        car = rob[r][0]
        picked, want = [], ["overlap", "face", "corner", "face", "corner", "overlap", "face", "corner"]
        for cw in (False, True):
            for rep in (False, True):
                sub = [p for p in polys if p.robot == r and p.cw == cw and p.repeated == rep][half::2]      # every other case of the combination
                for _ in range(2):                                           # the first one of the class that is due, else the first one left
                    j = next((j for j, p in enumerate(sub) if p.cls == want[(len(picked) + 3 * half) % 8]), 0)
                    p = sub.pop(j)
                    picked.append(("poly", p.V, p.state))
        for cls in ("inside", "outside"):
            sub = [c for c in circles if c.robot == r and c.cls == cls]
            picked += [("circle", c.c, c.r, c.state) for c in sub[2 * half:2 * half + 2]]
        scene = [o[:-1] for o in picked]
        assert len(scene) == 12
        st = [o[-1] for o in picked]
        while len(st) < 20:                                                  # 8 of the 12 poses displaced by up to 0.5 m and 0.3 rad
            s = st[len(st) - 12] + np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3)])
            if all(abs(v) >= grid.MIN_ABS for v in exact_scene(car, s, scene)[0]):
                st.append(s)
        cars.append(car); scenes.append(scene); poses[:, m] = np.array(st)
    return cars, scenes, poses


def check_against_exact(cars, scenes, poses, values):
    """values [20][3] held to the contract and to scenarios.clearance -> (worst figure per class, classes seen, worst |value - specification|)"""
    worst, spec_worst = {}, 0.0
    for p in range(poses.shape[0]):
        for m, car in enumerate(cars):
            vals, classes = exact_scene(car, poses[p, m], scenes[m])
            got = values[p, m]
            fig, sign = grid.peer_figure(got, vals, classes)
            cls = classes[int(np.argmin(vals))]
            worst[cls] = max(worst.get(cls, 0.0), fig)
            want = sc.clearance(car, poses[p, m], [as_obstacle(o) for o in scenes[m]])
            spec_worst = max(spec_worst, abs(got - want))
            print(f"pose {p} member {m}: {cls:8s} exact {min(vals):+.6f}  device {got:+.6f}  figure {fig:.2e}  |device - specification| {abs(got - want):.2e}")
            assert sign and fig <= TOL, (p, m, cls, got, min(vals))
            assert abs(got - want) <= TOL, (p, m, got, want)
    return worst, spec_worst


@pytest.mark.parametrize("edges", [3, 4, 8])
def test_contract_on_the_device(hip, edges):
    """measured: |device - exact| <= 2.1e-14 m in every class, |device - specification| <= 1.5e-14 m"""
    cars, scenes, poses = device_cases(edges)
    f = Fleet(hip, cars)
    assert f.rc == 0
    f.upload(scenes, poses[0])
    values = np.array([f.clearance(poses[p]) for p in range(20)])
    f.close()
    worst, spec_worst = check_against_exact(cars, scenes, poses, values)
    print(f"{edges}-edge robots: worst figure per class", {k: f"{v:.2e}" for k, v in worst.items()}, f"; |device - specification| <= {spec_worst:.2e}")
    assert set(worst) == {"overlap", "face", "corner", "inside", "outside"}


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_strided_loop_and_four_wave_reduction(hip):
    """256 threads stride over n = 300 obstacles; four waves are reduced through LDS.  Every other obstacle is >= 35 m away."""
    rob, polys, _, _ = grid.build()
    car = rob[2][0]
    near = next(p for p in polys if p.robot == 2 and p.cls == "face" and p.cw and p.repeated)
    st = near.state
    c, s = np.cos(st[2]), np.sin(st[2])
    # a second near one: a clockwise box with a repeated vertex that reaches 0.5 m into the robot's left side (the robot's left side is y = 0.8 in its frame)
    box = np.array([[-0.5, -0.5, 0.5, 0.5, 0.5], [0.3, 2.3, 2.3, 2.3, 0.3]])
    deep = ("poly", np.ascontiguousarray(np.array([[c, -s], [s, c]]) @ box + st[0:2].reshape(2, 1)))
    v_deep, cls_deep = exact_one(car, st, deep)
    assert cls_deep == "overlap" and abs(v_deep + 0.5) <= 1e-12 and near.exact > 0.0
    far = []
    for j in range(300):
        a, d = 0.7 * j, 40.0 + j % 40
        ctr = st[0:2] + d * np.array([np.cos(a), np.sin(a)])
        far.append(("circle", ctr, 0.5 + 0.01 * (j % 50)) if j % 3 == 0 else ("poly", sc.regular_polygon(ctr[0], ctr[1], 3 + j % 6, 1.0, 0.1 * j).vertex))
    f = Fleet(hip, [car])
    assert f.rc == 0

    def run(placed):
        scene = list(far)
        for idx, o in placed.items():
            scene[idx] = o
        geom = f.upload([scene], st[None, :])
        g, n = np.full((300, E, 2), np.nan), np.zeros(1, np.int32)
        assert hip.debug_scene_geom(f.svs[0]._be.handle, dptr(g), iptr(n)) == 0 and n[0] == 300
        assert np.array_equal(g, geom)                                       # the resident rows are in the caller's order: index = the thread's i
        return f.clearance(st[None, :])[0]
    assert run({}) > 30.0
    for idx in (0, 63, 64, 255, 256, 299):
        got = run({idx: ("poly", near.V)})
        print(f"near obstacle at index {idx}: device {got:+.12f}  exact {near.exact:+.12f}  |d| {abs(got - near.exact):.2e}")
        assert abs(got - near.exact) <= TOL, idx
    for small, large in ((70, 10), (130, 10), (200, 10), (10, 200), (299, 64)):   # the smaller one in wave 1, 2, 3, 0, and in the second stride
        got = run({small: deep, large: ("poly", near.V)})
        print(f"deep obstacle at index {small}, near one at {large}: device {got:+.12f}  exact {v_deep:+.12f}")
        assert abs(got - v_deep) <= TOL, (small, large)
    f.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_peer_clearance_beyond_one_stride(hip):
    """64 lanes stride over B = 66 members.  The members stand side by side (heading pi / 2, 10 m apart in x, staggered in y so that a corner faces a
    side: class 'face', where the separating-axis value is the distance), 8.4 m of free space between neighbours"""
    B = 66
    car = sc.rectangle_robot(dynamics="diff", wheelbase=0)
    base = np.array([[10.0 * i, 0.4 * (i % 3), np.pi / 2] for i in range(B)])
    f = Fleet(hip, [car] * B)
    assert f.rc == 0
    cache = {}

    def pair(si, sj):
        key = (tuple(si), tuple(sj))
        if key not in cache:
            cache[key] = cache[(key[1], key[0])] = ex.signed_sep(ex.robot_polygon(car, si), ex.robot_polygon(car, sj))
        return cache[key]

    def exact(states):
        out = np.zeros(B)
        for i in range(B):
            dist = np.linalg.norm(states[:, 0:2] - states[i, 0:2], axis=1)
            dist[i] = np.inf
            best = np.inf
            for j in np.argsort(dist):
                if dist[j] - 2 * REACH > best:
                    break
                v, cls = pair(states[i], states[j])
                assert cls == "face", (i, j, cls)
                best = min(best, v)
            out[i] = best
        return out
    got = f.peer_clearance(base)
    want = exact(base)
    assert np.abs(got - want).max() <= TOL and np.abs(want - 8.4).max() <= 1e-9
    for a, b in ((0, 1), (1, 64), (64, 65), (2, 65)):
        states = base.copy()
        states[b] = [states[a, 0] + 1.6 + 0.3, states[a, 1] + 0.25, np.pi / 2]       # b's side 0.3 m from a's
        got, want = f.peer_clearance(states), exact(states)
        print(f"pair ({a}, {b}): device {got[a]:+.12f} {got[b]:+.12f}  exact {want[a]:+.12f}; the others: largest |device - exact| = {np.abs(got - want).max():.2e}")
        assert abs(want[a] - 0.3) <= 1e-9 and want[a] == want[b]
        assert np.abs(got - want).max() <= TOL, (a, b)
        assert np.sum(want < 1.0) == 2 and np.all(np.delete(want, [a, b]) > 5.0)
    f.close()


def test_peer_clearance_with_a_clockwise_footprint(hip):
    """B = 2, the second member's G with its rows reversed: rda_create takes such a robot (it refuses nothing about the order of the rows), and the
    separation is that of the footprints whichever way round they run"""
    rob = grid.robots()
    cars = [rob[2][0], rob[3][0]]
    assert rob[3][2] and ex.shoelace(ex.points(sc.robot_vertices(cars[1], np.zeros(3)))) < 0
    f = Fleet(hip, cars)
    assert f.rc == 0
    seen = set()
    for states in (np.array([[10.0, 20.0, 0.3], [14.0, 22.5, 1.4]]), np.array([[10.0, 20.0, 0.3], [11.0, 20.5, 1.4]]), np.array([[-60.0, 20.0, 0.3], [-55.514, 24.109, 0.3]])):
        got = f.peer_clearance(states)
        v, cls = ex.signed_sep(ex.robot_polygon(cars[0], states[0]), ex.robot_polygon(cars[1], states[1]))
        want = sc.peer_clearance(cars, states)
        print(f"{cls:8s} exact {v:+.12f}  device {got[0]:+.12f} {got[1]:+.12f}  specification {want[0]:+.12f}")
        seen.add(cls)
        assert got[0] == got[1] and grid.holds(got[0], v, cls, TOL) and np.abs(got - want).max() <= TOL
    assert seen == {"overlap", "face", "corner"}
    f.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_untouched_paths(hip):
    rob, polys, _, _ = grid.build()
    f = Fleet(hip, [rob[2][0], rob[2][0]])
    assert f.rc == 0
    near = next(p for p in polys if p.robot == 2)
    f.upload([[("poly", near.V)], []], np.array([near.state, near.state]))      # the second member has no obstacle
    got = f.clearance(np.array([near.state, near.state]))
    assert grid.holds(got[0], near.exact, near.cls, TOL) and got[1] == np.inf
    f.close()
    g = Fleet(hip, [sc.circle_robot(0.8, dynamics="diff")])
    assert g.rc == RDA_ERR_UNSUPPORTED


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_allocations_of_a_first_clearance_call_change_nothing(hip):
    """a fleet's first rda_fleet_clearance makes its move tables and the clearance log: refused at each of the 10 allocations in turn it returns
    RDA_ERR_HIP and holds nothing more than before; the call that gets through returns the doubles of an undisturbed twin.  B = 2, T = 5, N = 4, E = 4,
    three and two polygons."""
    cars = [sc.rectangle_robot(dynamics="acker"), sc.rectangle_robot(dynamics="diff", wheelbase=0)]
    states = np.array([[10.0, 20.0, 0.3], [14.0, 28.0, 1.4]])
    scenes = [[sc.regular_polygon(13.0, 21.0, 4, 0.8, 0.2), sc.regular_polygon(8.0, 23.0, 3, 0.7, 1.0), sc.regular_polygon(10.5, 20.2, 4, 0.5, 0.4)],
              [sc.regular_polygon(15.0, 31.0, 3, 0.9, 0.1), sc.regular_polygon(11.0, 27.0, 4, 0.6, 0.7)]]

    def staged():
        svs, F = bare_fleet(hip, cars)
        flat = [sv.flatten_scene(list(s)) for sv, s in zip(svs, scenes)]
        counts = np.array([f[0] for f in flat], np.int32)
        kind, nvert = (np.ascontiguousarray(np.concatenate([f[j] for f in flat]), np.int32) for j in (1, 2))
        geom, vel = (np.ascontiguousarray(np.concatenate([f[j] for f in flat]), float) for j in (3, 4))
        assert hip.fleet_upload_scenes(F, iptr(counts), iptr(kind), iptr(nvert), dptr(geom), dptr(vel), dptr(np.ascontiguousarray(states[:, 0:2])),
                                       iptr(np.ones(2, np.int32))) == 0
        return svs, F
    (sa, fa), (sb, fb) = staged(), staged()
    got, want = np.full(2, np.nan), np.full(2, np.nan)
    rc, refused = refused_in_turn(hip, lambda: hip.fleet_clearance(fa, dptr(states), dptr(got)))
    print("allocations of a fleet's first rda_fleet_clearance:", refused)
    assert rc == 0 and refused == 10
    assert hip.fleet_clearance(fb, dptr(states), dptr(want)) == 0
    assert np.array_equal(got, want) and np.all(np.isfinite(want))
    hip.fleet_destroy(fa); hip.fleet_destroy(fb)
