"""CPU: the simulated lidar's specification, `World.get_lidar_scan`, against exact ray casting (tests/ray_exact.py: rational arithmetic, every decision
exact) instead of against itself, on the pinned grid of tests/ray_grid.py.
  1  the reference on answers derived by hand
  2  the grid is what tests/ray_grid.py says it is, and stays within its caps
  3  `World.get_lidar_scan` within ray_grid.bound() of the exact range on every conditioned beam of the grid; the largest figure per class is printed
  4  teeth: the former acceptance rule (|den| > 1e-12, t >= 0, 0 <= s <= 1 with one quotient s per edge), restated here in numpy, lets aimed and
     split-vertex beams through the corner of a closed polygon

  5  teeth of the collinear class: the side test with den != 0 as its only guard, restated here, reports returns on beams that point away from an edge

Measured on the grid (tests 2 - 5 print them): 12 406 beams - 900 aimed, 180 split, 240 peers, 150 away, 150 along, 10 786 generic - of which only the
150 along beams fail `conditioned`; |specification - exact| <= 3.55e-15 m aimed, 1.78e-15 split, 4.44e-15 peers, 0 away, 6.13e-14 generic, recorded as
ray_grid.SPEC_WORST = 6.2e-14; the along beams at most 4.44e-15 m outside their bracket.  The former rule is more than 1e-3 m wrong on 7 aimed beams and on
all 180 split beams (0.065 .. 0.49 m: the far side of the polygon); with only `world.py` put back to it, test 3 reads 0.33 m aimed, 0.49 m split, 1.87 m
peers, 2.31 m generic.  Without the collinear guard 6 away beams report a return at 0 m and 4 along beams leave their bracket.  The grid with its exact
ranges takes 5 s once, each test below 0.5 s."""
from math import sqrt

import numpy as np
import pytest

import ray_exact as ex
import ray_grid as grid
from lidar_world_lib import numpy_scan
from rda_planner_amd import scenarios as sc


@pytest.fixture(scope="module")
def cases():
    return grid.build()


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------------------
def one(obstacles, o, d, rmin=0.0, rmax=20.0):
    return ex.cast_conditioned(ex.Scene(obstacles), o, d, rmin, rmax)


def test_hand_derived_answers():
    O = (0.0, 0.0)
    for turn in (1, -1):                                                   # both windings: equal answers
        square = grid.poly(np.array([[2.0, 4.0, 4.0, 2.0], [-1.0, -1.0, 1.0, 1.0]])[:, ::turn])
        assert one([square], O, (1.0, 0.0)) == (2.0, True)                 # head-on: the face x = 2
        assert one([square], O, (-1.0, 0.0)) == (20.0, True)               # behind the origin: no hit
        assert one([square], O, (2.0, 0.0)) == (2.0, True)                 # the direction's length does not matter: t = 1, range t |d| = 2
        assert one([square], O, (1.0, 0.0), rmin=3.0) == (3.0, True) and one([square], O, (1.0, 0.0), rmax=1.5) == (1.5, True)
        # the square [2, 4] x [2, 4] through its corner (2, 2) along d = (1, 1): t = 2, |d| = sqrt 2; the corner's edges lie on either side of the beam
        corner = grid.poly(np.array([[2.0, 4.0, 4.0, 2.0], [2.0, 2.0, 4.0, 4.0]])[:, ::turn])
        assert one([corner], O, (1.0, 1.0)) == (2.0 * sqrt(2.0), True) and 2.0 * sqrt(2.0) == 2.8284271247461903
        r, ok = one([corner], O, (np.cos(np.pi / 4), np.sin(np.pi / 4)))   # with the float direction the beam passes a hair beside the corner
        assert ok and abs(r - 2.0 * sqrt(2.0)) <= 1e-15
        # the 6-8-10 triangle (6, 0), (0, 8), (6, 8) along d = (3, 4): the hypotenuse x / 6 + y / 8 = 1 is met at t = 1, the point (3, 4), range 5
        tri = grid.poly(np.array([[6.0, 6.0, 0.0], [0.0, 8.0, 8.0]])[:, ::turn])
        assert one([tri], O, (3.0, 4.0)) == (5.0, True)
        assert one([tri], O, (6.0, 0.0))[0] == 6.0                         # through the vertex (6, 0) along the x axis: t = 1, range 6; a silhouette
        assert not ex.conditioned(ex.Scene([tri]), O, (6.0, 0.0), 0.0, 20.0) and ex.conditioned(ex.Scene([tri]), O, (3.0, 4.0), 0.0, 20.0)
        # an edge that lies along the ray: the triangle (2, 0), (4, 0), (3, -1) is met at the edge's first point; from a point ON the edge at once
        flat = grid.poly(np.array([[2.0, 4.0, 3.0], [0.0, 0.0, -1.0]])[:, ::turn])
        assert one([flat], O, (1.0, 0.0))[0] == 2.0 and one([flat], (3.0, 0.0), (1.0, 0.0))[0] == 0.0 and one([flat], (5.0, 0.0), (1.0, 0.0))[0] == 20.0
        # an origin inside: the square [-1, 1]^2 is hit from the inside, along (3, 4) at the face y = 1: t = 1 / 4, range 5 / 4
        box = grid.poly(np.array([[-1.0, 1.0, 1.0, -1.0], [-1.0, -1.0, 1.0, 1.0]])[:, ::turn])
        assert one([box], O, (1.0, 0.0)) == (1.0, True) and one([box], O, (3.0, 4.0)) == (1.25, True)
        # a repeated vertex changes nothing
        again = grid.poly(np.array([[2.0, 4.0, 4.0, 4.0, 2.0], [-1.0, -1.0, -1.0, 1.0, 1.0]])[:, ::turn])
        assert one([again], O, (1.0, 0.0)) == (2.0, True)
    # a circle of radius 1 about (5, 0) straight ahead: 4; about (5, 1): tangent at (5, 0), range 5, and gone under a shear: not conditioned
    assert one([sc.circle(5.0, 0.0, 1.0)], O, (1.0, 0.0)) == (4.0, True)
    assert one([sc.circle(5.0, 1.0, 1.0)], O, (1.0, 0.0)) == (5.0, False)
    assert one([sc.circle(5.0, 1.0, 1.0)], O, (1.0, 0.0), rmax=5.0) == (5.0, False)      # (sheared towards the centre it is met 1e-4 m earlier)
    assert one([sc.circle(5.0, 1.0, 1.0)], O, (1.0, 0.0), rmax=4.9) == (4.9, True)
    assert one([sc.circle(-5.0, 0.0, 1.0)], O, (1.0, 0.0)) == (20.0, True)               # behind
    # along (3, 4) to the circle of radius 5 about (6, 8): the near point is (3, 4), range 5
    assert one([sc.circle(6.0, 8.0, 5.0)], (0.0, 0.0), (3.0, 4.0))[0] == 5.0
    # an origin inside a circle does not see it: what lies behind is seen
    assert one([sc.circle(0.5, 0.0, 2.0)], O, (1.0, 0.0)) == (20.0, True)
    wall = grid.poly(np.array([[7.0, 8.0, 8.0, 7.0], [-3.0, -3.0, 3.0, 3.0]]))
    assert one([sc.circle(0.5, 0.0, 2.0), wall], O, (1.0, 0.0)) == (7.0, True)
    # the nearest of a circle's root and an edge's quotient, decided exactly: the circle about (5, 0) is met at 5 - sqrt(0.99) = 4.00501..., beside y = 0.1
    disc = sc.circle(5.0, 0.1, 1.0)
    for x, first in ((4.004, True), (4.006, False)):
        thin = grid.poly(np.array([[x, x + 1.0, x + 1.0, x], [-1.0, -1.0, 1.0, 1.0]]))
        r = one([disc, thin], O, (1.0, 0.0))[0]
        assert (r == x) == first and (first or abs(r - (5.0 - sqrt(1.0 - 0.01))) <= 1e-15)
    assert ex.less((ex.Fr(3), ex.Fr(0)), (ex.Fr(5), ex.Fr(1))) and not ex.less((ex.Fr(5), ex.Fr(1)), (ex.Fr(4), ex.Fr(0)))       # 3 < 4; 4 < 4 is false
    assert ex.less((ex.Fr(5), ex.Fr(2)), (ex.Fr(4), ex.Fr(0))) and ex.less((ex.Fr(5), ex.Fr(2)), (ex.Fr(6), ex.Fr(5)))            # 3.586 < 4, < 3.764
    assert not ex.less((ex.Fr(6), ex.Fr(5)), (ex.Fr(5), ex.Fr(2))) and ex.below((ex.Fr(5), ex.Fr(2)), ex.Fr(13)) and not ex.below((ex.Fr(5), ex.Fr(2)), ex.Fr(12))


def test_the_specification_on_the_hand_derived_answers():
    """`World.get_lidar_scan` on the same shapes: a 3-beam sensor looking along -90, 0 and 90 degrees from the origin"""
    sensor = dict(number=3, angle_min=-0.5 * np.pi, angle_max=0.5 * np.pi, range_min=0.0, range_max=20.0)
    shapes = [grid.poly(np.array([[2.0, 4.0, 4.0, 2.0], [-1.0, -1.0, 1.0, 1.0]])), sc.circle(0.0, 6.0, 1.0),
              grid.poly(np.array([[-1.0, -1.0, 1.0, 1.0], [-3.0, -5.0, -5.0, -3.0]]))]
    got = numpy_scan([0.0, 0.0, 0.0], sensor, shapes)["ranges"]
    want, cond = ex.scan(ex.Scene(shapes), np.zeros(3), sensor)[0:2]
    assert cond.all() and np.abs(want - [3.0, 2.0, 5.0]).max() <= 1e-15 and np.abs(got - want).max() <= 1e-15
    # an edge along the beam: the triangles (2, 0), (4, 0), (3, -+1) from the origin, beams along +x and (all but) -x.  The first beam is a silhouette:
    # exact 2, and 20 under the shear that turns it away from the triangle - the specification answers within that bracket; the second beam points
    # away from the edge, whose line it lies on: range_max and nothing else, no return at 0 and no -0.0
    two = dict(number=2, angle_min=0.0, angle_max=np.pi, range_min=0.0, range_max=20.0)
    for y in (-1.0, 1.0):
        for turn in (1, -1):
            flat = [grid.poly(np.array([[2.0, 4.0, 3.0], [0.0, 0.0, y]])[:, ::turn])]
            got = numpy_scan([0.0, 0.0, 0.0], two, flat)["ranges"]
            want, cond, lo, hi = ex.scan(ex.Scene(flat), np.zeros(3), two)
            assert want.tolist() == [2.0, 20.0] and cond.tolist() == [False, True] and (lo[0], hi[0]) == (2.0, 20.0)
            assert lo[0] <= got[0] <= hi[0] and got[1] == 20.0 and not np.signbit(got).any()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_grid_is_what_it_says_and_keeps_its_caps(cases):
    worst, count, left, most, _ = grid.figures(cases, lambda l: [s.exact for s in l.scans])
    print("beams per class:", count, " not conditioned:", left, " most generic beams left out in one scan:", most)
    assert count["aimed"] + count["split"] == grid.AIMED_LAUNCHES * 3 * grid.PER_SCAN >= 1000 and count["split"] == grid.AIMED_LAUNCHES * 3 * 4
    assert count["peers"] == 2 * grid.PEER_LAUNCHES >= 200
    assert left["aimed"] == 0 and left["split"] == 0 and left["peers"] == 0 and most <= 1               # the caps
    assert count["away"] == count["along"] == 3 * grid.COL_PER_SCAN * grid.COL_LAUNCHES + len(grid.COL_PINNED) and left["away"] == 0
    assert left["along"] == count["along"]                                                              # every beam along an edge is a silhouette
    col = [s for l in cases["collinear"] for s in l.scans]
    assert sum(o.vertex.shape[1] == 5 for s in col for o in s.obstacles) == 2 * 3 * grid.COL_LAUNCHES   # the split-vertex variant
    assert all((s.exact[s.cls == "away"] == s.sensor["range_max"]).all() for s in col)                  # nothing lies where the away beams look
    aimed = [s for l in cases["aimed"] for s in l.scans]
    assert len(aimed) == 45 and all(s.sensor["number"] == 128 for s in aimed) and max(len(s.obstacles) for s in aimed) == 36
    big = next(s for s in aimed if len(s.obstacles) == 36)
    assert any(o.vertex is not None and o.vertex.shape[1] >= 3 for o in big.obstacles[32:])            # aimed polygons on both sides of the tile boundary
    nv = [o.vertex.shape[1] for s in aimed for o in s.obstacles if o.vertex is not None]
    assert set(nv) == set(range(3, grid.EMAX + 1))
    area = [np.sign(ex._cross((o.vertex[0, 1] - o.vertex[0, 0], o.vertex[1, 1] - o.vertex[1, 0]), (o.vertex[0, 2] - o.vertex[0, 1], o.vertex[1, 2] - o.vertex[1, 1])))
            for s in aimed for o in s.obstacles if o.vertex is not None and o.vertex.shape[1] == 3]
    assert {-1.0, 1.0} <= set(area)                                                                     # both windings
    assert any((o.vertex[:, 1:] == o.vertex[:, :-1]).all(axis=0).any() for s in aimed for o in s.obstacles if o.vertex is not None)       # a repeated vertex
    gen = [s for l in cases["generic"] for s in l.scans]
    assert sorted(s.sensor["number"] for s in gen) == [1, 65, 100, 128, 128, 128] and any(s.sensor["range_min"] > 0 for s in gen)
    assert any((s.exact == s.sensor["range_min"]).any() and s.sensor["range_min"] > 0 for s in gen)                                        # range_min clips
    far, d = gen[0], ex.directions(gen[0].state[2], gen[0].sensor)                                      # a circle 0.01 m and a square 0.05 m beyond range_max
    assert far.exact[40] == 12.0 and far.exact[90] == 12.0
    assert abs(ex.cast(ex.Scene(far.obstacles), far.state[0:2], d[40], 0.0, 13.0) - 12.01) <= 1e-12
    assert abs(ex.cast(ex.Scene(far.obstacles), far.state[0:2], d[90], 0.0, 13.0) - 12.05) <= 1e-12
    assert (gen[3].exact < 5.0).all() and (gen[4].exact == 12.0).any()                                  # inside the octagon: every beam ends; inside the circle: not
    assert all(len(l.scans) == 3 for l in grid.launches(cases))
    # every class really ends on something
    for l in cases["aimed"] + cases["peers"]:
        for s in l.scans:
            m = s.cls != "generic"
            assert (s.exact[m] < s.sensor["range_max"]).all()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_specification_on_the_grid(cases):
    """the fixed specification within 10 x its recorded worst figure of the exact range on every conditioned beam, and that record is not exceeded"""
    got = {id(l): [numpy_scan(s.state, s.sensor, grid.seen_by(l, i))["ranges"] for i, s in enumerate(l.scans)] for l in grid.launches(cases)}
    worst, count, left, most, outside = grid.figures(cases, lambda l: got[id(l)])
    print("worst |specification - exact| per class:", {k: f"{v:.2e}" for k, v in worst.items()}, " beams:", count, " left out:", left,
          f"; beams along an edge: at most {outside:.2e} m outside their bracket")
    assert max(worst.values()) <= grid.bound() and outside <= grid.bound()
    assert not any(np.signbit(r).any() for rs in got.values() for r in rs)                             # no -0.0
    assert max(worst.values()) <= grid.SPEC_WORST and grid.bound() == 10.0 * grid.SPEC_WORST <= 1e-12


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------------------
def former_rule(o, d, V, rng):
    """the acceptance rule the specification had before, polygon edges only (the negative control)"""
    for k in range(V.shape[1]):
        p, e, w = V[:, k], V[:, (k + 1) % V.shape[1]] - V[:, k], V[:, k] - o
        den = d[:, 0] * e[1] - d[:, 1] * e[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            t, s = (w[0] * e[1] - w[1] * e[0]) / den, (w[0] * d[:, 1] - w[1] * d[:, 0]) / den
        rng = np.minimum(rng, np.where((np.abs(den) > 1e-12) & (t >= 0) & (s >= 0) & (s <= 1), t, np.inf))
    return rng


def test_the_former_rule_leaks_on_the_grid(cases):
    leaks = {"aimed": [], "split": []}
    for l in cases["aimed"]:
        for s in l.scans:
            d = ex.directions(s.state[2], s.sensor)
            got = np.full(s.sensor["number"], s.sensor["range_max"])
            for o in s.obstacles:
                if o.vertex is not None:
                    got = former_rule(s.state[0:2], d, o.vertex, got)
            for c in leaks:
                leaks[c] += [float(x) for x in np.abs(got - s.exact)[(s.cls == c) & s.cond] if x > 1e-3]
    print("beams that the former rule lets through a closed polygon: aimed", len(leaks["aimed"]), "split", len(leaks["split"]),
          f"; errors {min(leaks['aimed'] + leaks['split']):.3f} .. {max(leaks['aimed'] + leaks['split']):.3f} m")
    assert len(leaks["aimed"]) + len(leaks["split"]) >= 5
    assert len(leaks["aimed"]) >= 5                                        # shared vertices alone, without the 1e-13 m edges


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------------------
def sides_only_rule(o, d, V, rng):
    """the watertight side test with den != 0 as its only guard, polygon edges only (the second negative control): an edge that lies along the beam's
    line to within rounding is accepted on rounding noise"""
    for k in range(V.shape[1]):
        p, q = V[:, k], V[:, (k + 1) % V.shape[1]]
        e, w, u = q - p, p - o, q - o
        den = d[:, 0] * e[1] - d[:, 1] * e[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (w[0] * e[1] - w[1] * e[0]) / den
        ok = ((w[0] * d[:, 1] - w[1] * d[:, 0] >= 0) != (u[0] * d[:, 1] - u[1] * d[:, 0] >= 0)) & (den != 0) & (t >= 0)
        rng = np.minimum(rng, np.where(ok, t, np.inf))
    return rng


def test_the_side_test_without_the_collinear_guard_sees_phantoms(cases):
    phantom, outside = 0, 0
    for l in cases["collinear"]:
        for s in l.scans:
            d = ex.directions(s.state[2], s.sensor)
            got = np.full(s.sensor["number"], s.sensor["range_max"])
            for o in s.obstacles:
                got = sides_only_rule(s.state[0:2], d, o.vertex, got)
            phantom += int((np.abs(got - s.exact)[s.cls == "away"] > 1e-3).sum())
            m = s.cls == "along"
            outside += int((np.maximum(s.lo[m] - got[m], got[m] - s.hi[m]) > 1e-3).sum())
    print("without the guard: beams that point away from an edge on their line and report a return:", phantom, "; beams along an edge outside their bracket:", outside)
    assert phantom >= 5 and outside >= 3
