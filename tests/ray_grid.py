"""The pinned seeded grid on which the simulated lidar is held to tests/ray_exact.py, with the contract, the caps and the bounds.  Shared by
tests/test_ray_exact.py (the specification `World.get_lidar_scan`, on the CPU) and tests/test_gpu_ray_exact.py (lidar::k_raycast_fleet and
lidar::k_raycast_fleet_peers).  One generator, seed SEED; `build()` gives the same grid on every call and keeps it for the process.

GRID (every device launch takes three members, so the scans come in threes; vertex stride EMAX = 8)
  aimed    AIMED_LAUNCHES x 3 full-turn fans of 128 beams, range 0 .. 13 m, at poses in three regions of the 5 .. 45 m square that lie more than 26 m apart
           (so the members are out of each other's reach when the seeing caster runs on them).  Per scan PER_SCAN = 24 beams, 4 .. 6 beams apart, each
           get a convex polygon of 3 .. 8 vertices on a circle of radius 0.05 .. 0.25 m whose centre lies ON the beam, 3 .. 12 m out, with one vertex set to
           fl(o + rho d_b): the beam enters the polygon through that vertex, the vertex's neighbours lie on opposite sides of the beam, the true range is
           continuous in the heading.  Half of the polygons are clockwise; every sixth has one vertex repeated (3 .. 7 vertices plus the repeat); scan 1
           holds 12 more small obstacles between the beams, 36 in shuffled order: more than the 32 of a ray_world tile
  split    every sixth aimed polygon has its aimed vertex replaced by TWO vertices SPLIT = 1e-13 m apart, one on either side of the beam (checked exactly)
  generic  two launches of random worlds of circles and polygons (3 .. 8 vertices, either winding): a 128-beam full turn with a circle and a polygon just
           beyond range_max, the 100-beam half turn with range_min = 2.5 m above the nearest obstacles, a 1-beam sensor; an origin well inside an octagon,
           an origin well inside a circle (which it then does not see), a 65-beam fan.  The beams of the aimed scans that are not aimed, and those of the
           peers scans, count as generic too
  peers    PEER_LAUNCHES x 3 members of one robot size (4.6 x 1.6 m; Ackermann about the rear axle, differential and omni about the centre) with 12-, 12- and
           1-beam sensors.  Member 2 stands anywhere; member 1 is placed 4 .. 9 m from a footprint corner v of member 2 (`scenarios.peer_footprints`) within 25
           degrees of the corner's bisector, and its heading is atan2(v - o) - angle_b for a beam b; member 0 likewise on a corner of member 1: two aimed
           beams per launch, each entering a footprint through a corner with the corner's edges on either side
  collinear  COL_LAUNCHES x 3 fans of 129 beams (128 intervals: beam b + 64 looks the opposite way), the first COL_LATTICE launches at half-metre lattice
           origins with headings in steps of 45 degrees.  Per scan COL_PER_SCAN = 8 polygons (triangles, rectangles, either winding) with an edge
           p q = fl(o + a u), fl(o + (a + L) u) ON the line of a beam, a = 2 .. 8 m, L = 0.1 .. 1 m: the beam that runs along the edge is class 'along', a
           silhouette; the one that points away from it is class 'away', and conditioned.  u = d_b for some, -d_b for the others, so each class has the
           constructed direction and the nearly opposite one.  Two per scan have the near vertex p split into two SPLIT apart on either side of the line.
           Then COL_PINNED: six such rectangles, found by a search, on which the side test with den != 0 as its only guard reported a return at 0 m
A scan whose origin lies within ray_exact.MARGIN of a boundary, or whose aimed beam does not end on its vertex (something in front of it), is drawn again from
the same generator; nothing is excluded afterwards.

CAPS (conditions of the grid, asserted on the CPU; the reference alone decides `conditioned`): no aimed, split or peers beam fails `conditioned`; at most one
generic beam per scan does; no away beam does.  Only those may be left out of a comparison.  An along beam is never conditioned; it is held to its BRACKET
instead: within the bound of [lo, hi], the smallest and largest exact range among the beam and its neighbours sheared by up to +-1e-9 rad.

BOUNDS.  Kernels: clear_grid.DEVICE_BOUND = 1e-9 m, the project's stated bound for device geometry (the device's cos / sin may differ from numpy's d by an
ulp: 1e-14 m on a conditioned beam).  Specification: bound() = 10 x SPEC_WORST, where SPEC_WORST is the worst |World.get_lidar_scan - exact| of the FIXED
specification on this grid as tests/test_ray_exact.py::test_specification_on_the_grid prints it, rounded up - a figure of the specification on a pinned grid,
never of a kernel (the rule of tests/clear_grid.py and tests/lmz_rows_cert.py)."""
from collections import namedtuple
from fractions import Fraction as Fr
from functools import lru_cache

import numpy as np

import ray_exact as ex
from clear_grid import DEVICE_BOUND                      # noqa: F401  (1e-9 m)
from rda_planner_amd import scenarios as sc

SEED = sc.SEED + 11
EMAX = 8
AIMED_LAUNCHES, PER_SCAN, PEER_LAUNCHES = 15, 24, 120
SPLIT = 1e-13
FAN = dict(number=128, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=13.0)
REGIONS = ((5.0, 12.0, 5.0, 12.0), (38.0, 45.0, 5.0, 12.0), (20.0, 30.0, 38.0, 45.0))        # x0, x1, y0, y1 of member 0, 1, 2
PEER_FAN = dict(number=12, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=12.0)
PEER_ONE = dict(number=1, angle_min=0.4, angle_max=1.1, range_min=0.0, range_max=12.0)
DYN = ("acker", "diff", "omni")
COL_FAN = dict(number=129, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=13.0)      # 128 intervals: beam b + 64 looks the opposite way
COL_LAUNCHES, COL_LATTICE, COL_PER_SCAN = 6, 4, 8
COL_BACK = (False, True, True, False, False, True, True, False)
# pinned: (state, beam b, a, L, h, side) of rectangles p = fl(o - a d_b), q = fl(o - (a + L) d_b) behind beam b, found by a search with the rule that had
# den != 0 as its only guard: there beam b, which points AWAY from the edge, reported a return at 0.0 m (sides and den all rounding noise, t = noise / noise)
COL_PINNED = (([24.5, 15.5, 3.141592653589793], 62, 7.598, 0.715, 0.332, 1.0), ([18.419, 20.377, -2.188], 50, 4.887, 0.408, 0.132, -1.0),
              ([26.0, 38.5, 0.0], 48, 7.638, 0.916, 0.362, 1.0), ([30.5, 20.5, -0.7853981633974483], 32, 7.722, 0.832, 0.291, -1.0),
              ([28.0, 34.5, 3.141592653589793], 42, 2.634, 0.952, 0.298, 1.0), ([16.0, 32.0, 1.5707963267948966], 16, 7.291, 0.725, 0.108, 1.0))
COL_SHAPES = ("triangle", "rectangle", "split", "rectangle", "rectangle", "split", "triangle", "rectangle")

SPEC_WORST = 6.2e-14           # measured 6.13e-14 m ('generic': a circle met at a flat angle); aimed 3.6e-15, split 1.8e-15, peers 4.4e-15, away 0


def bound():
    return 10.0 * SPEC_WORST


# cls: per beam 'aimed' | 'split' | 'peers' | 'along' | 'away' | 'generic'; exact, cond: per beam from ray_exact
Scan = namedtuple("Scan", "state sensor obstacles cls exact cond lo hi")    # lo, hi: the bracket of the exact ranges for d and its sheared neighbours
Launch = namedtuple("Launch", "kind scans cars")          # cars: the three robots of a peers launch (else None); a peers scan's obstacles = its world only


def poly(V):
    return sc.Obstacle(None, None, np.ascontiguousarray(V, dtype=float), "Rpositive", np.zeros((2, 1)))


def cars():
    return [sc.rectangle_robot(dynamics=k, wheelbase=3.0 if k == "acker" else 0) for k in DYN]


def seen_by(launch, i):
    """what member i's sensor casts against: its world, and in a peers launch the other members' footprints behind it"""
    s = launch.scans[i]
    if launch.cars is None:
        return list(s.obstacles)
    return list(s.obstacles) + sc.peer_footprints(launch.cars, [x.state for x in launch.scans], i)


def _side(o, d, v):
    """the exact sign of (v - o) x d"""
    x = (Fr(float(v[0])) - Fr(float(o[0]))) * Fr(float(d[1])) - (Fr(float(v[1])) - Fr(float(o[1]))) * Fr(float(d[0]))
    return (x > 0) - (x < 0)


def random_shape(rng, centre):
    """a circle of radius 0.2 .. 0.8 m or a convex polygon of 3 .. 8 vertices on a circle of radius 0.3 .. 1 m, either winding"""
    if rng.uniform() < 0.4:
        return sc.circle(centre[0], centre[1], float(rng.uniform(0.2, 0.8)))
    k = int(rng.integers(3, EMAX + 1))
    ang = np.sort(rng.uniform(0, 2 * np.pi / k, k) + 2 * np.pi * np.arange(k) / k) + rng.uniform(-np.pi, np.pi)
    V = np.asarray(centre, float).reshape(2, 1) + rng.uniform(0.3, 1.0) * np.vstack((np.cos(ang), np.sin(ang)))
    return poly(V[:, ::-1] if rng.uniform() < 0.5 else V)


def aimed_polygon(rng, o, d, th, kind, cw):
    """a convex polygon whose vertex fl(o + rho d) the beam (o, d = (cos th, sin th)) enters through; kind 'plain' | 'repeat' | 'split' -> (V, rho)"""
    k = int(rng.integers(3, EMAX + 1 if kind == "plain" else EMAX))
    rho, r = rng.uniform(3.0, 12.0), rng.uniform(0.05, 0.25)
    v, c = o + rho * d, o + (rho + r) * d
    step = 2 * np.pi / k
    ang = th + np.pi + step * np.arange(k) + np.r_[0.0, rng.uniform(-0.3, 0.3, k - 1)] * step       # ascending: counter-clockwise, vertex 0 faces the origin
    P = c.reshape(2, 1) + r * np.vstack((np.cos(ang), np.sin(ang)))
    P[:, 0] = v
    if kind == "split":                                                     # the last vertex lies left of the beam, vertex 1 right of it
        n = np.array([-d[1], d[0]])
        left, right = v + 0.5 * SPLIT * n, v - 0.5 * SPLIT * n
        if not (_side(o, d, left) < 0 < _side(o, d, right)):               # ((v - o) x d < 0 on the left of the beam)
            return None, rho
        P = np.column_stack((left, right, P[:, 1:]))
    elif kind == "repeat":
        j = int(rng.integers(0, k))
        P = np.insert(P, j, P[:, j], axis=1)
    return poly(P[:, ::-1] if cw else P), rho


def _measure(state, sensor, obstacles, cls):
    scene = ex.Scene(obstacles)
    if not ex.origin_clear(scene, state[0:2]):
        return None
    exact, cond, lo, hi = ex.scan(scene, state, sensor)
    return Scan(np.asarray(state, float), sensor, obstacles, cls, exact, cond, lo, hi)


def aimed_scan(rng, region, fillers):
    x0, x1, y0, y1 = region
    while True:
        state = np.array([rng.uniform(x0, x1), rng.uniform(y0, y1), rng.uniform(-np.pi, np.pi)])
        d = ex.directions(state[2], FAN)
        ang = np.linspace(FAN["angle_min"], FAN["angle_max"], FAN["number"])
        beams = int(rng.integers(0, 8)) + 5 * np.arange(PER_SCAN) + rng.integers(0, 2, PER_SCAN)
        cls = np.array(["generic"] * FAN["number"], dtype=object)
        obstacles, rhos, ok = [], [], True
        for j, b in enumerate(beams):
            kind = ("split", "repeat", "plain", "plain", "plain", "plain")[j % 6]
            ob, rho = aimed_polygon(rng, state[0:2], d[b], state[2] + ang[b], kind, cw=bool(rng.integers(0, 2)))
            ok = ok and ob is not None
            obstacles.append(ob); rhos.append(rho)
            cls[b] = "split" if kind == "split" else "aimed"
        for j in range(fillers):                                           # between beams b + 2 and b + 3 of an aimed beam b, 8 .. 12 m out
            a = state[2] + 0.5 * (ang[beams[2 * j] + 2] + ang[beams[2 * j] + 3])
            c = state[0:2] + rng.uniform(8.0, 12.0) * np.array([np.cos(a), np.sin(a)])
            obstacles.append(sc.circle(c[0], c[1], 0.1) if j % 2 else sc.regular_polygon(c[0], c[1], 3 + j % 3, 0.1, 0.3 * j))
        if not ok:
            continue
        obstacles = [obstacles[i] for i in rng.permutation(len(obstacles))]
        s = _measure(state, FAN, obstacles, cls)
        if s is not None and np.abs(s.exact[beams] - np.array(rhos)).max() <= 1e-9:
            return s


def generic_launches(rng):
    def world(centre, n, lo, hi):
        out = []
        for _ in range(n):
            a, r = rng.uniform(-np.pi, np.pi), rng.uniform(lo, hi)
            out.append(random_shape(rng, (centre[0] + r * np.cos(a), centre[1] + r * np.sin(a))))
        return out

    def scan(state, sensor, obstacles):
        while True:
            s = _measure(state, sensor, obstacles, np.array(["generic"] * sensor["number"], dtype=object))
            if s is not None:
                return s
            state = state + np.r_[rng.uniform(-0.2, 0.2, 2), 0.0]

    full = dict(number=128, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=12.0)
    half = dict(number=100, angle_min=-0.5 * np.pi, angle_max=0.5 * np.pi, range_min=2.5, range_max=10.0)
    one = dict(number=1, angle_min=0.3, angle_max=1.2, range_min=0.0, range_max=12.0)
    odd = dict(number=65, angle_min=-2.0, angle_max=2.5, range_min=0.5, range_max=9.0)
    # a: a circle and a square whose nearest points lie 0.01 m and 0.05 m beyond range_max, on beams 40 and 90
    sa = np.array([14.0, 31.0, 0.7])
    da = ex.directions(sa[2], full)
    beyond = [sc.circle(*(sa[0:2] + (12.0 + 0.01 + 0.4) * da[40]), 0.4)]
    cen, across = sa[0:2] + (12.05 + 0.5) * da[90], 0.5 * np.array([-da[90][1], da[90][0]])
    beyond.append(poly(np.column_stack([cen - 0.5 * da[90], cen - across, cen + 0.5 * da[90], cen + across])))
    a = scan(sa, full, world(sa, 10, 2.0, 11.0) + beyond)
    sb = np.array([33.0, 9.0, -2.1])
    b = scan(sb, half, world(sb, 10, 1.5, 9.0))
    sc_ = np.array([24.0, 22.0, 1.3])
    c = scan(sc_, one, world(sc_, 4, 6.0, 11.0) + [sc.circle(*(sc_[0:2] + 7.0 * np.array([np.cos(1.6), np.sin(1.6)])), 0.7)])
    # d: inside an octagon of radius 4 m, 1 m off its centre, with obstacles inside and outside it; e: the same with a circle of radius 3 m
    sd = np.array([9.0, 40.0, 2.6])
    d = scan(sd, full, [sc.regular_polygon(sd[0] + 0.8, sd[1] - 0.6, 8, 4.0, 0.2)] + world(sd, 3, 1.2, 2.2) + world(sd, 4, 6.0, 10.0))
    se = np.array([41.0, 30.0, -0.4])
    e = scan(se, full, [sc.circle(se[0] - 0.7, se[1] + 0.7, 3.0)] + world(se, 3, 1.2, 2.0) + world(se, 6, 4.5, 10.0))
    sf = np.array([27.0, 27.0, 0.1])
    f = scan(sf, odd, world(sf, 9, 1.5, 8.5))
    return [Launch("generic", [a, b, c], None), Launch("generic", [d, e, f], None)]


def _corner_origin(rng, car, state):
    """an origin 4 .. 9 m in front of a footprint corner v, within 25 degrees of its bisector -> (o, v)"""
    F = sc.robot_vertices(car, np.asarray(state, float))
    k = F.shape[1]
    j = int(rng.integers(0, k))
    v, p, q = F[:, j], F[:, j - 1], F[:, (j + 1) % k]
    u = (p - v) / np.linalg.norm(p - v) + (q - v) / np.linalg.norm(q - v)          # into the footprint
    u /= np.linalg.norm(u)
    a = rng.uniform(-np.radians(25.0), np.radians(25.0))
    u = np.array([np.cos(a) * u[0] - np.sin(a) * u[1], np.sin(a) * u[0] + np.cos(a) * u[1]])
    return v - rng.uniform(4.0, 9.0) * u, v


def peer_launch(rng, robots, with_world):
    ang = np.linspace(PEER_FAN["angle_min"], PEER_FAN["angle_max"], PEER_FAN["number"])
    while True:
        states = [None, None, np.array([rng.uniform(15.0, 35.0), rng.uniform(15.0, 35.0), rng.uniform(-np.pi, np.pi)])]
        beams, corners = [0, 0], [None, None]
        for i in (1, 0):
            o, v = _corner_origin(rng, robots[i + 1], states[i + 1])
            beams[i], corners[i] = int(rng.integers(0, PEER_FAN["number"])), v
            states[i] = np.array([o[0], o[1], np.arctan2(v[1] - o[1], v[0] - o[0]) - ang[beams[i]]])
        worlds = [[], [], []]
        if with_world:                                                      # a few obstacles behind member 0 as seen from its target
            back = 2.0 * states[0][0:2] - corners[0]
            worlds[0] = [random_shape(rng, back + rng.uniform(-2.0, 2.0, 2)) for _ in range(3)]
        scans = []
        for i, sensor in enumerate((PEER_FAN, PEER_FAN, PEER_ONE)):
            cls = np.array(["generic"] * sensor["number"], dtype=object)
            if i < 2:
                cls[beams[i]] = "peers"
            s = _measure(states[i], sensor, worlds[i] + sc.peer_footprints(robots, states, i), cls)
            if s is None or (i < 2 and abs(s.exact[beams[i]] - np.linalg.norm(corners[i] - states[i][0:2])) > 1e-9):
                break
            scans.append(s._replace(obstacles=worlds[i]))
        if len(scans) == 3:
            return Launch("peers", scans, robots)


def collinear_scan(rng, region, lattice):
    """COL_PER_SCAN polygons with an edge p q = fl(o + a u), fl(o + (a + L) u) on the line of a beam b: u = d_b for the even ones (beam b runs ALONG the
    edge, beam b + 64 points AWAY from it), u = -d_b for the odd ones (the other way round); the body lies 0.1 .. 0.4 m to one side (either, so both
    windings).  Shapes in turn: triangle, rectangle, rectangle whose near vertex p is two vertices SPLIT apart on either side of the line, rectangle"""
    x0, x1, y0, y1 = region
    half = COL_FAN["number"] // 2
    while True:
        state = np.array([rng.uniform(x0, x1), rng.uniform(y0, y1), rng.uniform(-np.pi, np.pi)])
        if lattice:                                                        # half-metre lattice origins, headings in steps of 45 degrees
            state = np.array([np.round(2.0 * state[0]) / 2.0, np.round(2.0 * state[1]) / 2.0, 0.25 * np.pi * int(rng.integers(-3, 5))])
        o, d = state[0:2], ex.directions(state[2], COL_FAN)
        cls = np.array(["generic"] * COL_FAN["number"], dtype=object)
        obstacles, ok = [], True
        for j in range(COL_PER_SCAN):
            b, back = 8 * (j + 1), COL_BACK[j]
            u = -d[b] if back else d[b]
            a, L, h = rng.uniform(2.0, 8.0), rng.uniform(0.1, 1.0), rng.uniform(0.1, 0.4)
            n = (1.0 if rng.integers(0, 2) else -1.0) * np.array([-u[1], u[0]])
            p, q = o + a * u, o + (a + L) * u
            shape = COL_SHAPES[j]
            if shape == "triangle":
                V = np.column_stack((p, q, 0.5 * (p + q) + h * n))
            elif shape == "rectangle":
                V = np.column_stack((p, q, q + h * n, p + h * n))
            else:
                body, out = p + 0.5 * SPLIT * n, p - 0.5 * SPLIT * n
                ok = ok and _side(o, d[b], body) * _side(o, d[b], out) < 0
                V = np.column_stack((out, q, q + h * n, p + h * n, body))
            obstacles.append(poly(V))
            cls[b + half if back else b], cls[b if back else b + half] = "along", "away"
        if not ok:
            continue
        s = _measure(state, COL_FAN, obstacles, cls)
        if s is not None:
            return s


def pinned_scan(case):
    state, b, a, L, h, sgn = case
    state = np.array(state, float)
    o, u = state[0:2], -ex.directions(state[2], COL_FAN)[b]
    n = sgn * np.array([-u[1], u[0]])
    p, q = o + a * u, o + (a + L) * u
    cls = np.array(["generic"] * COL_FAN["number"], dtype=object)
    cls[b], cls[b + COL_FAN["number"] // 2] = "away", "along"
    return _measure(state, COL_FAN, [poly(np.column_stack((p, q, q + h * n, p + h * n)))], cls)


@lru_cache(maxsize=None)
def build():
    """-> {'aimed': [Launch], 'generic': [Launch], 'peers': [Launch], 'collinear': [Launch]}, the same on every call"""
    rng = np.random.default_rng(SEED)
    aimed = [Launch("aimed", [aimed_scan(rng, REGIONS[i], 12 if (n, i) == (0, 1) else 0) for i in range(3)], None) for n in range(AIMED_LAUNCHES)]
    generic = generic_launches(rng)
    robots = cars()
    peers = [peer_launch(rng, robots, n % 4 == 0) for n in range(PEER_LAUNCHES)]
    collinear = [Launch("collinear", [collinear_scan(rng, REGIONS[i], n < COL_LATTICE) for i in range(3)], None) for n in range(COL_LAUNCHES)]
    collinear += [Launch("collinear", [pinned_scan(c) for c in COL_PINNED[k:k + 3]], None) for k in range(0, len(COL_PINNED), 3)]
    return {"aimed": aimed, "generic": generic, "peers": peers, "collinear": collinear}


KEYS = ("aimed", "generic", "peers", "collinear")


def launches(grid):
    return [l for key in KEYS for l in grid.get(key, [])]


def figures(grid, ranges_of):
    """ranges_of(launch) -> [ranges of member i]; -> (worst |got - exact| per class over the conditioned beams, beams per class, beams left out per class,
    the largest number of generic beams left out in one scan, the farthest that an 'along' beam lies outside its bracket)"""
    worst, count, left, most, outside = {}, {}, {}, 0, 0.0
    for l in launches(grid):
        got = ranges_of(l)
        for s, g in zip(l.scans, got):
            g = np.asarray(g, float)
            assert g.shape == s.exact.shape
            diff = np.abs(g - s.exact)
            for c in set(s.cls):
                m = s.cls == c
                count[c] = count.get(c, 0) + int(m.sum())
                left[c] = left.get(c, 0) + int((m & ~s.cond).sum())
                if (m & s.cond).any():
                    worst[c] = max(worst.get(c, 0.0), float(diff[m & s.cond].max()))
            most = max(most, int(((s.cls == "generic") & ~s.cond).sum()))
            m = s.cls == "along"
            if m.any():
                outside = max(outside, float(np.maximum(np.maximum(s.lo[m] - g[m], g[m] - s.hi[m]), 0.0).max()))
    return worst, count, left, most, outside
