"""
Lidar front end of the reference's lidar demo: `scan_box` of example/lidar_nav/lidar_path_track.py:20-60 -
range scan -> points in the robot frame -> DBSCAN(eps=2.0, min_samples=6) -> one minimum-area rectangle per cluster ->
4-vertex `Rpositive` obstacles in the world frame for `MPC.control`.

The reference takes DBSCAN from scikit-learn and the rectangle from OpenCV (`cv2.minAreaRect` + `cv2.boxPoints`); OpenCV
is not available here, so both steps are restated in numpy:
  * `dbscan` reproduces scikit-learn's labelling exactly (clusters numbered by their first core point in index order,
    a border point goes to the first cluster that reaches it, noise = -1); tests pin it against sklearn.cluster.DBSCAN.
  * `min_area_rect` is the rotating-calipers rectangle over the convex hull (exact in float64; OpenCV works in float32
    and may return the corners in another order / starting corner - `MPC` re-orders vertices anyway, mpc.py:476-490).
    A cluster of collinear points gives a zero-width rectangle in OpenCV, which the reference's half-space conversion
    turns into an infinite line; here such a rectangle is given `min_width` (1 cm) so that it stays a bounded obstacle.
This is host code, like in the reference, and the SPECIFICATION of the device front end (csrc/lidar_device.h: rda_scan_boxes /
rda_upload_scan), which computes the same boxes in one kernel: `scan_box_device` below is the one-line replacement of `scan_box`,
`MPC.control(state, speed, scan=scan_data)` stages the boxes without returning them to the host at all.
"""
from collections import namedtuple

import numpy as np

Obstacle = namedtuple("obstacle", "center radius vertex cone_type velocity")

MAX_TRACKS = 256            # boxes of one scan that take part in the tracking (lidar::MAX_TRACKS)
MAX_WINDOW = 8              # the longest history a track keeps (lidar::TRK_HIST)


def scan_points(scan_data):
    """hits of a scan (`ranges`, `angle_min`, `angle_max`, `range_max`) as an (n, 2) array in the sensor frame;
    beams at (range_max - 0.01) or beyond are misses (lidar_path_track.py:27-35)"""
    ranges = np.asarray(scan_data["ranges"], float)
    angles = np.linspace(scan_data["angle_min"], scan_data["angle_max"], len(ranges))
    hit = ranges < scan_data["range_max"] - 0.01
    return np.stack((ranges[hit] * np.cos(angles[hit]), ranges[hit] * np.sin(angles[hit])), axis=1)


def dbscan(points, eps=2.0, min_samples=6):
    """labels of scikit-learn's DBSCAN (euclidean, the point itself counts as a neighbour)"""
    X = np.asarray(points, float)
    n = len(X)
    labels = np.full(n, -1, dtype=np.int64)
    if n == 0:
        return labels
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    near = d2 <= eps * eps
    core = near.sum(axis=1) >= min_samples
    cluster = 0
    for i in range(n):
        if labels[i] != -1 or not core[i]:
            continue
        labels[i] = cluster                       # depth-first expansion, like sklearn's dbscan_inner
        stack = [i]
        while stack:
            j = stack.pop()
            if core[j]:
                for k in np.flatnonzero(near[j]):
                    if labels[k] == -1:
                        labels[k] = cluster
                        stack.append(k)
        cluster += 1
    return labels


def _cross(a, b):
    return a[0] * b[1] - a[1] * b[0]


def convex_hull(points):
    """counter-clockwise hull (Andrew's monotone chain), collinear points dropped"""
    P = np.unique(np.asarray(points, float), axis=0)
    if len(P) <= 2:
        return P
    P = P[np.lexsort((P[:, 1], P[:, 0]))]

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and _cross(out[-1] - out[-2], p - out[-2]) <= 0:
                out.pop()
            out.append(p)
        return out
    lower, upper = half(P), half(P[::-1])
    return np.array(lower[:-1] + upper[:-1])


def min_area_rect(points, min_width=0.01):
    """(4, 2) corners, counter-clockwise, of the minimum-area enclosing rectangle (one side collinear with a hull edge)"""
    H = convex_hull(points)
    if len(H) == 1:
        c, u, lo, hi, wlo, whi = H[0], np.array([1.0, 0.0]), 0.0, 0.0, 0.0, 0.0
    else:
        best = None
        m = len(H)
        for i in range(m if m > 2 else 1):
            e = H[(i + 1) % m] - H[i]
            u = e / np.linalg.norm(e)
            v = np.array([-u[1], u[0]])
            a, b = H @ u, H @ v
            area = (a.max() - a.min()) * (b.max() - b.min())
            if best is None or area < best[0]:
                best = (area, u, a.min(), a.max(), b.min(), b.max())
        _, u, lo, hi, wlo, whi = best
        c = np.zeros(2)
    v = np.array([-u[1], u[0]])
    if hi - lo < min_width:
        mid = 0.5 * (lo + hi); lo, hi = mid - 0.5 * min_width, mid + 0.5 * min_width
    if whi - wlo < min_width:
        mid = 0.5 * (wlo + whi); wlo, whi = mid - 0.5 * min_width, mid + 0.5 * min_width
    return np.array([c + lo * u + wlo * v, c + hi * u + wlo * v, c + hi * u + whi * v, c + lo * u + whi * v])


def scan_box(state, scan_data, eps=2.0, min_samples=6):
    """the reference's `scan_box`: obstacles (4-vertex boxes in the world frame) seen by one scan from `state`"""
    pts = scan_points(scan_data)
    if len(pts) < 4:
        return []
    labels = dbscan(pts, eps, min_samples)
    state = np.asarray(state, float)
    rot = state[2, 0]
    R = np.array([[np.cos(rot), -np.sin(rot)], [np.sin(rot), np.cos(rot)]])
    out = []
    for label in np.unique(labels):
        if label == -1:
            continue
        box = min_area_rect(pts[labels == label])
        out.append(Obstacle(None, None, state[0:2] + R @ box.T, "Rpositive", np.zeros((2, 1))))
    return out


def scan_box_device(solver, state, scan_data, eps=2.0, min_samples=6):
    """`scan_box` computed on the device by `solver` (an `RDA_solver`, or anything that has one as `.rda`: an `MPC`):
    the same list of obstacles, corners within rounding of the host function's"""
    solver = getattr(solver, "rda", solver)
    boxes = solver.scan_boxes(state, scan_data, eps, min_samples)
    return [Obstacle(None, None, np.ascontiguousarray(b.T), "Rpositive", np.zeros((2, 1))) for b in boxes]


def scan_box_device_fleet(fleet, states, scans, eps=2.0, min_samples=6):
    """`scan_box_device` for every member of a `Fleet` in one kernel launch (rda_fleet_scan_boxes): `scans[i]` taken from
    `states[i]`; the list of the members' obstacle lists"""
    return [[Obstacle(None, None, np.ascontiguousarray(b.T), "Rpositive", np.zeros((2, 1))) for b in boxes]
            for boxes in fleet.scan_boxes(states, scans, eps, min_samples)]


def _split_tol(tol):
    tol = float(tol)
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError("scan split: tol must be finite and greater than 0")
    return tol


def end_point_fit(x, y, a, b, tol2):
    """(s, thr) of the run [a, b] (b - a >= 2) of the points x, y: s[i - a - 1] for a < i < b and the bound max s is compared with (`split_runs`)"""
    ex, ey = x[b] - x[a], y[b] - y[a]
    L2 = ex * ex + ey * ey
    rx, ry = x[a + 1:b] - x[a], y[a + 1:b] - y[a]
    if L2 > 0:
        cr = rx * ey - ry * ex
        return cr * cr, tol2 * L2
    return rx * rx + ry * ry, tol2


def split_runs(points, labels, eps, tol):
    """Segment number of every hit, (n,): the clusters of `labels` (`dbscan`'s) cut into their straight runs by the end-point fit - the specification
    of the split stage of lidar::scan_body (csrc/lidar_device.h), which takes every decision on the same numbers.  `points`: the hits in beam order
    (`scan_points`).  Noise keeps -1.  For every cluster in ascending number, its points in beam order q_0 .. q_{k-1}; every product and sum rounded
    separately, in the order written:
      gap rule       a run ends between q_i and q_{i+1} when dx * dx + dy * dy <= eps * eps is false (`dbscan`'s `near`)
      end-point fit  of a run [a, b] with b - a >= 2: e = q_b - q_a, L2 = ex * ex + ey * ey; for a < i < b r = q_i - q_a and
                     L2 > 0:  cr = rx * ey - ry * ex, s_i = cr * cr, the run splits iff max s_i > (tol * tol) * L2
                     L2 == 0 (a closed loop): s_i = rx * rx + ry * ry, the run splits iff max s_i > tol * tol
                     (no square root, no division).  The split point m is the lowest index at the maximum; the run becomes [a, m - 1] and [m, b]: the
                     corner starts the second run, no point belongs to two.  Runs of one or two points are final.
      numbering      the fixed point of this rule, segments numbered by cluster number, then by the position of the run's first point.
    Known and accepted: a cluster that crosses the first / last-beam seam is cut there by the gap rule unless every beam hits (two boxes for one wall);
    two surfaces that interleave in beam order inside one cluster break into many short runs; a convex body seen corner-on becomes two thin boxes."""
    P = np.asarray(points, float).reshape(-1, 2)
    labels = np.asarray(labels)
    eps, tol = float(eps), _split_tol(tol)
    eps2, tol2 = eps * eps, tol * tol
    seg = np.full(len(P), -1, dtype=np.int64)
    nseg = 0
    for c in np.unique(labels):
        if c < 0:
            continue
        idx = np.flatnonzero(labels == c)
        x, y = P[idx, 0], P[idx, 1]
        dx, dy = x[:-1] - x[1:], y[:-1] - y[1:]
        gap = ~(dx * dx + dy * dy <= eps2)
        heads = np.concatenate(([0], np.flatnonzero(gap) + 1, [len(idx)]))
        todo = [(int(heads[k]), int(heads[k + 1]) - 1) for k in range(len(heads) - 1)]
        starts = []
        while todo:
            a, b = todo.pop()
            m = -1
            if b - a >= 2:
                s, thr = end_point_fit(x, y, a, b, tol2)
                if s.max() > thr:
                    m = a + 1 + int(np.argmax(s))                          # (argmax: the first, so the lowest, index at the maximum)
            if m < 0:
                starts.append(a)
            else:
                todo += [(a, m - 1), (m, b)]
        starts = np.sort(np.array(starts, dtype=np.int64))
        of = np.zeros(len(idx), dtype=np.int64)
        of[starts] = 1
        seg[idx] = nseg + np.cumsum(of) - 1
        nseg += len(starts)
    return seg


def scan_box_split(state, scan_data, eps=2.0, min_samples=6, tol=0.15):
    """`scan_box` with one `min_area_rect` per segment of `split_runs`, in segment order: a concave cluster (an L-shaped wall, the two sides of a
    corridor, the inside of a room) becomes one thin box per straight run instead of one box over the free space between them.  No boxes for fewer than
    4 hits, as before; `tol` [m] finite and > 0, else a ValueError.  See `split_runs` for the rule and its accepted limits."""
    tol = _split_tol(tol)
    pts = scan_points(scan_data)
    if len(pts) < 4:
        return []
    seg = split_runs(pts, dbscan(pts, eps, min_samples), eps, tol)
    state = np.asarray(state, float)
    rot = state[2, 0]
    R = np.array([[np.cos(rot), -np.sin(rot)], [np.sin(rot), np.cos(rot)]])
    out = []
    for s in range(int(seg.max()) + 1 if len(seg) else 0):
        box = min_area_rect(pts[seg == s])
        out.append(Obstacle(None, None, state[0:2] + R @ box.T, "Rpositive", np.zeros((2, 1))))
    return out


def scan_box_split_device(solver, state, scan_data, eps=2.0, min_samples=6, tol=0.15):
    """`scan_box_split` computed on the device by `solver` (an `RDA_solver`, or anything that has one as `.rda`): the same obstacles, corners within
    rounding of the host function's"""
    solver = getattr(solver, "rda", solver)
    boxes = solver.scan_boxes(state, scan_data, eps, min_samples, split=_split_tol(tol))
    return [Obstacle(None, None, np.ascontiguousarray(b.T), "Rpositive", np.zeros((2, 1))) for b in boxes]


def scan_box_split_device_fleet(fleet, states, scans, eps=2.0, min_samples=6, tol=0.15):
    """`scan_box_split_device` for every member of a `Fleet` in one kernel launch: the list of the members' obstacle lists"""
    return [[Obstacle(None, None, np.ascontiguousarray(b.T), "Rpositive", np.zeros((2, 1))) for b in boxes]
            for boxes in fleet.scan_boxes(states, scans, eps, min_samples, split=_split_tol(tol))]


def box_centres(boxes):
    """(n, 2) centres of (n, 4, 2) boxes, the corners added in the order the scan kernel writes them: (((x0 + x1) + x2) + x3) * 0.25"""
    B = np.asarray(boxes, float).reshape(-1, 4, 2)
    return (((B[:, 0] + B[:, 1]) + B[:, 2]) + B[:, 3]) * 0.25


def track_boxes(tracks, boxes, dt, gate=1.0, window=8, max_tracks=MAX_TRACKS):
    """Velocities of this tick's `boxes` (n, 4, 2) from the tracks of the previous tick: the specification of lidar::k_track_boxes_fleet
    (csrc/lidar_device.h), which computes the same numbers bit for bit.  Returns (velocities (n, 2), tracks).
    `tracks`: None or the list this function returned one tick - `dt` - earlier; a track is the list of its past centres, oldest first, 1 .. `window`
    entries, its position the last one; track i of the returned list belongs to box i.
      which boxes  the first m = min(n, max_tracks); the others get velocity 0 and leave no track
      distance     d2[i][j] = dx * dx + dy * dy of centre i against the position of previous track j, every operation rounded separately
      association  mutual nearest neighbour: fwd[i] = the lowest j at the minimum of row i, back[j] = the lowest i at the minimum of column j; box i
                   continues track j = fwd[i] if and only if back[j] == i and d2[i][j] <= gate * gate (so the result does not depend on the order of the
                   boxes, which changes with the cluster order from tick to tick; gate / dt is also the largest speed a new track can show)
      continued    history h: v = (c - h[0]) / (dt * len(h)) - the difference over the track's age, not over one tick - and the new history is
                   (h + [c])[-window:]
      otherwise    v = 0, history [c]; previous tracks that nobody continues end; no boxes: no tracks
    Boxes are finite numbers."""
    window = int(window)
    if not 1 <= window <= MAX_WINDOW or not gate > 0 or not dt > 0:
        raise ValueError(f"track_boxes: need 1 <= window <= {MAX_WINDOW}, gate > 0 and dt > 0")
    c = box_centres(boxes)
    n = len(c)
    m = min(n, int(max_tracks))
    prev = list(tracks) if tracks else []
    vel, out = np.zeros((n, 2)), []
    fwd = back = d2 = None
    if m and prev:
        p = np.array([h[-1] for h in prev], float).reshape(-1, 2)
        dx, dy = c[:m, None, 0] - p[None, :, 0], c[:m, None, 1] - p[None, :, 1]
        d2 = dx * dx + dy * dy
        fwd, back = d2.argmin(axis=1), d2.argmin(axis=0)                      # (argmin: the first, so the lowest, index at the minimum)
    gate2 = float(gate) * float(gate)
    for i in range(m):
        ci = np.array([c[i, 0], c[i, 1]])
        j = int(fwd[i]) if fwd is not None else -1
        if j >= 0 and back[j] == i and d2[i, j] <= gate2:
            h = prev[j]
            span = float(dt) * float(len(h))
            first = np.asarray(h[0], float)
            vel[i] = (ci - first) / span
            out.append(([np.asarray(q, float) for q in h] + [ci])[-window:])
        else:
            out.append([ci])
    return vel, out


def scan_box_tracked(state, scan_data, tracks, dt, eps=2.0, min_samples=6, gate=1.0, window=8):
    """`scan_box` with the velocities of `track_boxes` in the obstacles' `velocity`: (obstacles, tracks) - `tracks` goes into the next tick's call"""
    obs = scan_box(state, scan_data, eps, min_samples)
    boxes = np.array([o.vertex.T for o in obs], float).reshape(-1, 4, 2)
    vel, tracks = track_boxes(tracks, boxes, dt, gate, window)
    return [o._replace(velocity=vel[i].reshape(2, 1).copy()) for i, o in enumerate(obs)], tracks
