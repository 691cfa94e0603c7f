"""An exact reference for the project's clearance figures, written from the geometry alone.  It imports nothing of the routines it judges
(`scenarios._poly_sep`, `scenarios.clearance`, `scenarios.peer_clearance`, the device kernels); `scenarios.robot_vertices` is used for placement only.

Inputs are float64 numbers taken as the exact rationals they are (`fractions.Fraction`).  Every DECISION is exact: the orientation of a polygon (sign of
its shoelace sum), whether a point lies in a polygon, whether two polygons meet, which pair of features is nearest (squared distances and squared
normalised gaps are rationals and are compared as such).  Only the last step of a value - one square root, one division - is floating point, in mpmath
at 40 digits, rounded to float64 once.

Definitions (convex polygons, either winding, zero-length edges dropped first):
  signed_sep(P, Q) -> (value, cls)
    'overlap'  the closed polygons share a point (an edge of one crosses or touches an edge of the other, or a vertex of one lies in the other).
               value = -(penetration depth) = -min over the outward edge normals n of both polygons of the overlap of the two projections on n.
               The same number is max over n of [min_w n.w - max_v n.v]; the reference asserts that it is <= 0 exactly when the polygons meet.
    'face'     apart, and the Euclidean distance is attained between a vertex and a point strictly inside an edge
    'corner'   apart, and it is attained only between two vertices
               value (both) = the Euclidean distance = min over (vertex, edge) pairs of the point-segment distance
  signed_circle(P, c, r) -> (value, cls): the distance of c to the boundary of P, negative when c lies in the closed polygon, minus r;
    cls 'inside' | 'outside' says where the CENTRE lies
  disc_polygon(c0, r0, P): a disc robot against a polygon - the same quantity with the roles named the other way round
  disc_disc(c0, r0, c, r): |c - c0| - r - r0
Non-convex polygons and polygons of zero area are outside these definitions (ValueError for zero area)."""
from fractions import Fraction as Fr

import mpmath
import numpy as np

_MP = mpmath.mp.clone()
_MP.dps = 40


def _sqrt_ratio(num, den2):
    """float64 of num / sqrt(den2) for rationals num, den2 > 0"""
    q = _MP.mpf(num.numerator) / _MP.mpf(num.denominator)
    d = _MP.sqrt(_MP.mpf(den2.numerator) / _MP.mpf(den2.denominator))
    return float(q / d)


def _sqrt_mp(x):
    return _MP.sqrt(_MP.mpf(x.numerator) / _MP.mpf(x.denominator))


def _sqrt(x):
    return float(_sqrt_mp(x))


def points(V):
    """2 x k (or k x 2 when k != 2 rows) float array -> list of exact points"""
    V = np.asarray(V, float)
    if V.shape[0] != 2:
        V = V.T
    return [(Fr(float(V[0, i])), Fr(float(V[1, i]))) for i in range(V.shape[1])]


def shoelace(pts):
    """twice the signed area (> 0: counter-clockwise)"""
    k = len(pts)
    return sum(pts[i][0] * pts[(i + 1) % k][1] - pts[(i + 1) % k][0] * pts[i][1] for i in range(k))


def polygon(V):
    """exact vertices of V, repeated neighbours dropped, counter-clockwise"""
    pts = points(V)
    kept = []
    for p in pts:
        if not kept or p != kept[-1]:
            kept.append(p)
    while len(kept) > 1 and kept[0] == kept[-1]:
        kept.pop()
    a2 = shoelace(kept)
    if len(kept) < 3 or a2 == 0:
        raise ValueError("clear_exact: a polygon of zero area")
    return kept if a2 > 0 else kept[::-1]


def _sub(p, q):
    return (p[0] - q[0], p[1] - q[1])


def _dot(p, q):
    return p[0] * q[0] + p[1] * q[1]


def _cross(p, q):
    return p[0] * q[1] - p[1] * q[0]


def _edges(P):
    return [(P[i], P[(i + 1) % len(P)]) for i in range(len(P))]


def in_polygon(P, c):
    """c in the closed convex counter-clockwise polygon P: on the left of, or on, every edge"""
    return all(_cross(_sub(b, a), _sub(c, a)) >= 0 for a, b in _edges(P))


def _point_segment(c, a, b):
    """(squared distance of c to the closed segment ab, the nearest point lies strictly inside the segment)"""
    ab, ac = _sub(b, a), _sub(c, a)
    t, L2 = _dot(ac, ab), _dot(ab, ab)
    if t <= 0:
        return _dot(ac, ac), False
    if t >= L2:
        bc = _sub(c, b)
        return _dot(bc, bc), False
    cr = _cross(ab, ac)
    return cr * cr / L2, True


def _orient(a, b, c):
    v = _cross(_sub(b, a), _sub(c, a))
    return (v > 0) - (v < 0)


def _on_segment(a, b, c):
    """c collinear with ab: inside its bounding box"""
    return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])


def _segments_meet(a, b, c, d):
    o1, o2, o3, o4 = _orient(a, b, c), _orient(a, b, d), _orient(c, d, a), _orient(c, d, b)
    if o1 != o2 and o3 != o4:
        return True
    return (o1 == 0 and _on_segment(a, b, c)) or (o2 == 0 and _on_segment(a, b, d)) or (o3 == 0 and _on_segment(c, d, a)) or (o4 == 0 and _on_segment(c, d, b))


def polygons_meet(P, Q):
    if any(in_polygon(Q, p) for p in P) or any(in_polygon(P, q) for q in Q):
        return True
    return any(_segments_meet(a, b, c, d) for a, b in _edges(P) for c, d in _edges(Q))


def _best_axis(P, Q):
    """the outward edge normal (of either polygon) with the largest normalised gap -> (gap numerator, squared normal length); the comparison of
    num / sqrt(den2) between edges is made on sign(num) num^2 / den2"""
    best = None
    for V, W in ((P, Q), (Q, P)):
        for a, b in _edges(V):
            e = _sub(b, a)
            n = (e[1], -e[0])                                  # outward for a counter-clockwise polygon
            num = min(_dot(n, w) for w in W) - max(_dot(n, v) for v in V)
            den2 = _dot(n, n)
            key = (1 if num >= 0 else -1) * num * num / den2
            if best is None or key > best[0]:
                best = (key, num, den2)
    return best[1], best[2]


def signed_sep(P, Q):
    P, Q = polygon(P), polygon(Q)
    num, den2 = _best_axis(P, Q)
    meet = polygons_meet(P, Q)
    assert meet == (num <= 0), "clear_exact: the separating-axis theorem disagrees with the intersection test - a non-convex input?"
    if meet:
        return _sqrt_ratio(num, den2), "overlap"
    best, inner = None, False
    for V, W in ((P, Q), (Q, P)):
        for c in V:
            for a, b in _edges(W):
                d2, mid = _point_segment(c, a, b)
                if best is None or d2 < best:
                    best, inner = d2, mid
                elif d2 == best:
                    inner = inner or mid
    return _sqrt(best), "face" if inner else "corner"


def signed_circle(P, c, r):
    P = polygon(P)
    c = (Fr(float(c[0])), Fr(float(c[1])))
    d2 = min(_point_segment(c, a, b)[0] for a, b in _edges(P))
    inside = in_polygon(P, c)
    d = _sqrt_mp(d2)
    return float((-d if inside else d) - _MP.mpf(float(r))), "inside" if inside else "outside"


def disc_polygon(c0, r0, P):
    return signed_circle(P, c0, r0)


def disc_disc(c0, r0, c, r):
    d = (Fr(float(c[0])) - Fr(float(c0[0])), Fr(float(c[1])) - Fr(float(c0[1])))
    return float(_sqrt_mp(_dot(d, d)) - _MP.mpf(float(r)) - _MP.mpf(float(r0)))


def robot_polygon(car, state):
    """world-frame 2 x k float vertices of a polygon robot (placement: scenarios.robot_vertices)"""
    from rda_planner_amd import scenarios as sc
    return sc.robot_vertices(car, np.asarray(state, float).ravel())
