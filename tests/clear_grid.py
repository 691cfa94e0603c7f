"""The pinned seeded grid on which the clearance figures are held to tests/clear_exact.py, and the contract itself.  Shared by
tests/test_clearance_exact.py (the specification, on the CPU) and tests/test_gpu_clearance_exact.py (the kernels).

GRID (one generator, seed SEED; every case is classified by the exact reference, and a draw with |exact| < MIN_ABS - a sign that rounding could decide -
is drawn again from the same generator, so the grid excludes nothing afterwards):
  robots     3, 4 (the default 4.6 x 1.6 m car), 6 and 8 edges, each with the rows of G in both orders: `robot_vertices` gives the second clockwise
  polygons   for each robot x {counter-clockwise, clockwise} x {plain, one vertex repeated} PER_COMBO draws: a convex polygon of 3 .. 8 entries (3 .. 7
             vertices plus the repeated one), half-axes 0.3 .. 2 m, at 0.2 .. 6 m from the robot's origin; positions up to 100 m
  circles    radius 0.1 .. 1.5 m; for each robot CIRCLES_PER_ROBOT centres inside the footprint (a convex combination of its vertices) and as many at
             0.5 .. 6 m from its origin and outside it
  peers      PEERS pairs and triples of the robots above within 5 m of each other
CLASSES are the reference's: 'overlap', 'face', 'corner' for polygons, 'inside', 'outside' for circles (where the centre lies).

CONTRACT of a value `got` against the reference's (exact, cls), with a bound b:
  overlap, face, inside, outside   |got - exact| <= b
  corner                           0 < got <= exact + b      (the documented conservative separating-axis gap, never above the distance)
  a minimum over several peers     got <= min exact + b; got >= the smallest exact of the non-corner pairs - b; with a corner pair in play got may lie
                                   below that, but stays > 0 when nothing overlaps

BOUND.  SPEC_WORST is the worst figure of the fixed `scenarios.clearance` / `scenarios.peer_clearance` on this grid (|got - exact|; for 'corner' the
excess got - exact where positive), as tests/test_clearance_exact.py::test_specification_on_the_grid prints it, rounded up.  The specification is held to
bound() = 10 x that (the rule of tests/lmz_rows_cert.py: a measured figure of the specification on a pinned grid, never of a kernel).  The kernels are
held to 1e-9 m, the project's stated bound for device geometry against its specification."""
from collections import namedtuple

import numpy as np

import clear_exact as ex
from rda_planner_amd import scenarios as sc

SEED = sc.SEED + 1
MIN_ABS = 1e-6
PER_COMBO, CIRCLES_PER_ROBOT, PEERS = 10, 10, 40
EMAX = 8

SPEC_WORST = 1.9e-14           # measured 1.83e-14 m ('face', coordinates up to 100 m); overlap 1.78e-14, circles 8.8e-15, peers 1.36e-14, corner excess 0
DEVICE_BOUND = 1e-9


def bound():
    return 10.0 * SPEC_WORST


PolyCase = namedtuple("PolyCase", "robot state V cw repeated exact cls")
CircleCase = namedtuple("CircleCase", "robot state c r exact cls")
PeerCase = namedtuple("PeerCase", "robots states exact cls")         # exact, cls: [m][m] per ordered pair (diagonal None)


def robots():
    """[(car, edges, rows reversed)] - 8 robots; index 2 is the default car"""
    rng = np.random.default_rng(SEED)
    out = []
    for k in (3, 4, 6, 8):
        if k == 4:
            base = sc.rectangle_robot(dynamics="diff", wheelbase=0)
        else:
            ang = np.sort(rng.uniform(0, 2 * np.pi / k, k) + 2 * np.pi * np.arange(k) / k)
            G, h = sc.polygon_halfspaces(np.vstack((1.8 * np.cos(ang), 0.9 * np.sin(ang))))
            base = sc.car(G, h, "Rpositive", 0, [10, 1], [10, 0.5], "diff")
        out.append((base, k, False))
        out.append((base._replace(G=np.ascontiguousarray(base.G[::-1]), h=np.ascontiguousarray(np.asarray(base.h)[::-1])), k, True))
    return out


def convex_polygon(rng, k, centre):
    """k vertices on an ellipse in ascending angle: convex, counter-clockwise, 2 x k"""
    ang = np.sort(rng.uniform(0, 2 * np.pi / k, k) + 2 * np.pi * np.arange(k) / k) + rng.uniform(-np.pi, np.pi)
    a, b, yaw = rng.uniform(0.3, 2.0), rng.uniform(0.3, 2.0), rng.uniform(-np.pi, np.pi)
    P = np.vstack((a * np.cos(ang), b * np.sin(ang)))
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s], [s, c]]) @ P + np.asarray(centre, float).reshape(2, 1)


def _state(rng):
    return np.array([rng.uniform(-95, 95), rng.uniform(-95, 95), rng.uniform(-np.pi, np.pi)])


def build():
    """-> (robots, polygon cases, circle cases, peer cases), the same on every call"""
    rng = np.random.default_rng(SEED + 1)
    rob = robots()
    polys, circles, peers = [], [], []
    for r, (car, _, _) in enumerate(rob):
        for cw in (False, True):
            for rep in (False, True):
                n = 0
                while n < PER_COMBO:
                    st = _state(rng)
                    k = int(rng.integers(3, EMAX if rep else EMAX + 1))
                    ang = rng.uniform(-np.pi, np.pi)
                    V = convex_polygon(rng, k, st[0:2] + rng.uniform(0.2, 6.0) * np.array([np.cos(ang), np.sin(ang)]))
                    if cw:
                        V = V[:, ::-1]
                    if rep:
                        j = int(rng.integers(0, k))
                        V = np.insert(V, j, V[:, j], axis=1)      # vertex j twice in a row
                    V = np.ascontiguousarray(V)
                    val, cls = ex.signed_sep(ex.robot_polygon(car, st), V)
                    if abs(val) < MIN_ABS:
                        continue
                    polys.append(PolyCase(r, st, V, cw, rep, val, cls))
                    n += 1
        for inside in (True, False):
            n = 0
            while n < CIRCLES_PER_ROBOT:
                st = _state(rng)
                RV = ex.robot_polygon(car, st)
                if inside:
                    c = RV @ rng.dirichlet(np.ones(RV.shape[1]))
                else:
                    ang = rng.uniform(-np.pi, np.pi)
                    c = st[0:2] + rng.uniform(0.5, 6.0) * np.array([np.cos(ang), np.sin(ang)])
                rad = float(rng.uniform(0.1, 1.5))
                val, cls = ex.signed_circle(RV, c, rad)
                if abs(val) < MIN_ABS or cls != ("inside" if inside else "outside"):
                    continue
                circles.append(CircleCase(r, st, np.ascontiguousarray(c), rad, val, cls))
                n += 1
    while len(peers) < PEERS:
        m = 2 + len(peers) % 2
        who = [int(x) for x in rng.integers(0, len(rob), m)]
        st0 = _state(rng)
        sts = np.array([[st0[0] + rng.uniform(-2.5, 2.5), st0[1] + rng.uniform(-2.5, 2.5), rng.uniform(-np.pi, np.pi)] for _ in range(m)])
        val, cls = [[None] * m for _ in range(m)], [[None] * m for _ in range(m)]
        for i in range(m):
            for j in range(i + 1, m):
                v, c = ex.signed_sep(ex.robot_polygon(rob[who[i]][0], sts[i]), ex.robot_polygon(rob[who[j]][0], sts[j]))
                val[i][j] = val[j][i] = v
                cls[i][j] = cls[j][i] = c
        if any(abs(val[i][j]) < MIN_ABS for i in range(m) for j in range(m) if i != j):
            continue
        peers.append(PeerCase(who, sts, val, cls))
    return rob, polys, circles, peers


def figure(got, exact, cls):
    """the figure that the bound is applied to, and whether the sign rule of the class holds"""
    if cls == "corner":
        return max(got - exact, 0.0), got > 0.0
    return abs(got - exact), True


def holds(got, exact, cls, b):
    fig, sign = figure(got, exact, cls)
    return sign and fig <= b


def peer_figure(got, exacts, classes):
    """a member's minimum over its peers -> (figure, sign rule holds)"""
    hi = min(exacts)
    firm = [e for e, c in zip(exacts, classes) if c != "corner"]
    fig = max(got - hi, 0.0)
    if len(firm) == len(exacts):
        return max(fig, hi - got), True
    lo = min(firm, default=np.inf)
    if lo <= 0.0:                                            # an overlapping pair below the corner pairs
        return max(fig, lo - got), True
    return fig, got > 0.0


def peer_holds(got, exacts, classes, b):
    fig, sign = peer_figure(got, exacts, classes)
    return sign and fig <= b
