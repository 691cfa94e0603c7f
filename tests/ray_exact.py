"""An exact reference for the simulated lidar, written from the geometry alone.  It imports nothing of what it judges (`World.get_lidar_scan`, `lidar.py`,
the ray-cast kernels).

Inputs are float64 numbers taken as the exact rationals they are (`fractions.Fraction`).  Every DECISION is exact: whether the ray meets an edge, which hit
is the nearest, whether a circle's discriminant is >= 0 and its entering root >= 0, whether a hit lies below range_max or range_min.  A hit parameter is
kept as the pair (p, D) that stands for p - sqrt(D) with rationals p and D >= 0 (D = 0 for an edge); two of them, and one against a bound, are compared
by squaring, in rationals.  Only the last step of a value - one square root, one product - is floating point, in mpmath at 40 digits, rounded to float64 once.

CONTRACT (the documented one of the sensor):
  beam      origin o, direction the float pair d = (cos th, sin th) AS GIVEN, not renormalised; a point of the ray is o + t d, t >= 0, and the reported
            range is the Euclidean length t |d|
  polygon   the boundary of the closed polygon: its edges as closed segments, either winding, zero-length edges dropped.  The hit is the smallest
            t >= 0 at which the ray meets an edge, so an origin inside is hit from the inside.  An edge that lies along the ray is met at its first
            point on the ray
  circle    the ENTERING root only, t = (-d.f - sqrt((d.f)^2 - d.d (f.f - r^2))) / d.d with f = o - c, and only when it is >= 0: no hit when the origin
            lies inside the circle (the documented quirk of the sensor)
  range     clip(min(range_max, hits), range_min, range_max)
  conditioned(beam)   the exact range for d sheared by +-SHEAR rad, d +- SHEAR d_perp (exact), stays within MOVE of the exact range for d.  A beam that
            fails it grazes a silhouette; only such beams may be left out of a comparison
  bracket   of a beam that is not conditioned: the smallest and the largest exact range among d and its neighbours sheared by up to +-SHEAR
            (`cast_bracket`).  A silhouette beam has no one right answer, but an answer outside its bracket is wrong
Origins within MARGIN of a boundary are outside the contract (the answer is discontinuous in the origin): `origin_clear` says whether one is.

The exact pass skips an obstacle only on a conservative test made in floating point: the obstacle's bounding disc, padded by PAD = 1e-6 m (nine decades
above the rounding of the test), is missed by the ray's line, lies behind the origin or lies beyond range_max."""
from fractions import Fraction as Fr

import mpmath
import numpy as np

_MP = mpmath.mp.clone()
_MP.dps = 40

SHEAR, MOVE, MARGIN, PAD = 1e-9, 1e-6, 1e-6, 1e-6


def _pt(x, y):
    return (Fr(float(x)), Fr(float(y)))


def _sub(p, q):
    return (p[0] - q[0], p[1] - q[1])


def _dot(p, q):
    return p[0] * q[0] + p[1] * q[1]


def _cross(p, q):
    return p[0] * q[1] - p[1] * q[0]


def _mp(x):
    return _MP.mpf(x.numerator) / _MP.mpf(x.denominator)


def less(a, b):
    """p1 - sqrt(D1) < p2 - sqrt(D2) for a = (p1, D1), b = (p2, D2): sqrt(D2) - sqrt(D1) < k = p2 - p1, squared twice"""
    (p1, D1), (p2, D2) = a, b
    k = p2 - p1
    if D1 == D2:
        return k > 0
    m = D1 + D2 - k * k                                   # (sqrt(D2) - sqrt(D1))^2 < k^2  <=>  m < 2 sqrt(D1 D2)
    if k > 0:
        return D2 < D1 or m < 0 or m * m < 4 * D1 * D2
    return D2 < D1 and m > 0 and m * m > 4 * D1 * D2


def below(t, M):
    """p - sqrt(D) < sqrt(M) for t = (p, D), M >= 0"""
    p, D = t
    if p <= 0:
        return p < 0 or M > 0 or D > 0
    n = p * p - M - D                                     # p^2 < M + D + 2 sqrt(M D)
    return n < 0 or n * n < 4 * M * D


class Scene:
    """obstacles with `center` (2 numbers), `radius`, `vertex` (2 x k, None for a circle) attributes -> exact shapes and padded bounding discs"""

    def __init__(self, obstacles):
        self.shapes, cen, rad = [], [], []
        for ob in obstacles:
            if ob.vertex is None:
                c = np.asarray(ob.center, float).ravel()
                self.shapes.append(("circle", _pt(c[0], c[1]), Fr(float(ob.radius))))
                cen.append(c[0:2]); rad.append(float(ob.radius))
            else:
                V = np.asarray(ob.vertex, float)
                pts = [_pt(V[0, i], V[1, i]) for i in range(V.shape[1])]
                kept = [p for i, p in enumerate(pts) if p != pts[i - 1]] or pts[:1]      # zero-length edges dropped (also the closing one)
                self.shapes.append(("polygon", kept, None))
                m = V.mean(axis=1)
                cen.append(m); rad.append(float(np.hypot(V[0] - m[0], V[1] - m[1]).max()))
        self.cen = np.array(cen, float).reshape(len(cen), 2)
        self.rad = np.array(rad, float) + PAD

    def candidates(self, o, d, range_max):
        """indices of the obstacles that the conservative test does not rule out (o, d floats)"""
        if not len(self.rad):
            return []
        f, n = self.cen - np.asarray(o, float), float(np.hypot(d[0], d[1]))
        along, across = (f[:, 0] * d[0] + f[:, 1] * d[1]) / n, (f[:, 0] * d[1] - f[:, 1] * d[0]) / n
        return np.flatnonzero((np.abs(across) <= self.rad) & (along >= -self.rad) & (along <= range_max + self.rad)).tolist()


def polygon_hit(o, d, pts):
    """the smallest t >= 0 at which o + t d meets the boundary of the polygon, as (t, 0), or None.  side_v = (v - o) x d; the closed edge p q meets the
    ray's line iff side_p and side_q are not strictly of one sign; then d x e = side_p - side_q"""
    side = [_cross(_sub(v, o), d) for v in pts]
    best, k = None, len(pts)
    for i in range(k):
        sp, sq = side[i], side[(i + 1) % k]
        if (sp > 0 and sq > 0) or (sp < 0 and sq < 0):
            continue
        p, q = pts[i], pts[(i + 1) % k]
        if sp == 0 and sq == 0:                            # the edge lies on the line: its first point on the ray
            a = _dot(d, d)
            tp, tq = _dot(_sub(p, o), d) / a, _dot(_sub(q, o), d) / a
            if max(tp, tq) < 0:
                continue
            t = max(min(tp, tq), Fr(0))
        else:
            t = _cross(_sub(p, o), _sub(q, p)) / (sp - sq)
            if t < 0:
                continue
        if best is None or t < best:
            best = t
    return None if best is None else (best, Fr(0))


def circle_hit(o, d, c, r):
    """the entering root as (p, D) = (-b / a, disc / a^2), or None: disc >= 0, and the root is >= 0 iff b <= 0 and f.f - r^2 >= 0"""
    f = _sub(o, c)
    a, b, c0 = _dot(d, d), _dot(d, f), _dot(f, f) - r * r
    disc = b * b - a * c0
    if disc < 0 or b > 0 or c0 < 0:
        return None
    return (-b / a, disc / (a * a))


def cast(scene, o, d, range_min, range_max):
    """the exact range of one beam, rounded once: o two floats, d two floats or two Fractions"""
    of = (float(o[0]), float(o[1]))
    o = _pt(*of)
    df = (float(d[0]), float(d[1]))
    d = (d[0] if isinstance(d[0], Fr) else Fr(df[0]), d[1] if isinstance(d[1], Fr) else Fr(df[1]))
    best = None
    for j in scene.candidates(of, df, float(range_max)):
        kind, g, r = scene.shapes[j]
        hit = circle_hit(o, d, g, r) if kind == "circle" else polygon_hit(o, d, g)
        if hit is not None and (best is None or less(hit, best)):
            best = hit
    a = _dot(d, d)
    if best is None or not below(best, Fr(float(range_max)) ** 2 / a):
        return float(range_max)
    if below(best, Fr(float(range_min)) ** 2 / a):
        return float(range_min)
    return float((_mp(best[0]) - _MP.sqrt(_mp(best[1]))) * _MP.sqrt(_mp(a)))


def sheared(d, sign, shear=SHEAR):
    """d + sign shear d_perp, exact"""
    dx, dy, h = Fr(float(d[0])), Fr(float(d[1])), Fr(shear)
    return (dx - sign * h * dy, dy + sign * h * dx)


def cast_bracket(scene, o, d, range_min, range_max):
    """-> (exact range, conditioned, the smallest and the largest of the exact ranges for d and its sheared neighbours).  For a beam that is not
    conditioned the neighbours at +-1e-12 and +-1e-15 rad are taken in too: at a silhouette the range jumps, and the value at the jump (a vertex's range,
    say) is reached only in the limit of small shears - the samples at +-SHEAR alone lie a few nm to either side of it"""
    r0 = cast(scene, o, d, range_min, range_max)
    rs = [cast(scene, o, sheared(d, s), range_min, range_max) for s in (-1, 1)]
    ok = all(abs(r - r0) <= MOVE for r in rs)
    if not ok:
        rs += [cast(scene, o, sheared(d, s, h), range_min, range_max) for s in (-1, 1) for h in (1e-12, 1e-15)]
    return r0, ok, min(rs + [r0]), max(rs + [r0])


def cast_conditioned(scene, o, d, range_min, range_max):
    """-> (exact range, conditioned)"""
    return cast_bracket(scene, o, d, range_min, range_max)[0:2]


def conditioned(scene, o, d, range_min, range_max):
    return cast_conditioned(scene, o, d, range_min, range_max)[1]


def directions(heading, sensor):
    """the float directions of a sensor's beams as the sensor's contract states them: np.linspace(angle_min, angle_max, number) added to the heading,
    numpy's cos and sin -> (number, 2)"""
    th = float(heading) + np.linspace(sensor["angle_min"], sensor["angle_max"], sensor["number"])
    return np.stack((np.cos(th), np.sin(th)), axis=1)


def scan(scene, state, sensor):
    """a whole scan -> (exact ranges, conditioned, bracket low, bracket high) per beam"""
    d = directions(state[2], sensor)
    out = [cast_bracket(scene, state[0:2], d[b], sensor["range_min"], sensor["range_max"]) for b in range(d.shape[0])]
    return tuple(np.array([x[k] for x in out], bool if k == 1 else float) for k in range(4))


def origin_clear(scene, o):
    """the origin is farther than MARGIN from every boundary (exact: squared distances against MARGIN^2)"""
    o, m = _pt(o[0], o[1]), Fr(MARGIN)
    for kind, g, r in scene.shapes:
        if kind == "circle":
            f2 = _dot(_sub(o, g), _sub(o, g))
            if (r - m) ** 2 <= f2 <= (r + m) ** 2 or (r <= m and f2 <= (r + m) ** 2):
                return False
            continue
        k = len(g)
        for i in range(k):
            a, ab = g[i], _sub(g[(i + 1) % k], g[i])
            ao = _sub(o, a)
            t, L2 = _dot(ao, ab), _dot(ab, ab)
            if t <= 0 or L2 == 0:
                d2 = _dot(ao, ao)
            elif t >= L2:
                d2 = _dot(_sub(o, g[(i + 1) % k]), _sub(o, g[(i + 1) % k]))
            else:
                d2 = _cross(ab, ao) ** 2 / L2
            if d2 <= m * m:
                return False
    return True
