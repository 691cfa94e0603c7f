"""
Headless scenario fixtures for the BASELINE configurations.

The reference's examples obtain robot geometry and obstacles from the `ir-sim` simulator
(example/*/*.py: `env.get_robot_info()`, `env.get_obstacle_info_list()`), which is not
available here.  This module builds the same kind of objects from plain numbers:

* `car_tuple`          - namedtuple 'G h cone_type wheelbase max_speed max_acce dynamics'
                          (reference rda_solver.py:35, example/path_track/path_track.py:10,20)
* `Obstacle`           - object with `.center .radius .vertex .cone_type .velocity`
                          (what mpc.py:192-203 reads)
* seeded generators for the corridor / lidar-box / dynamic-polygon / north-star scenes and the
  literal `path_track` scene of example/path_track/path_track*.yaml.

It is host-side fixture code, not part of the accelerated path.
"""
from collections import namedtuple
from math import cos, sin, tan

import numpy as np

car = namedtuple("car", "G h cone_type wheelbase max_speed max_acce dynamics")
Obstacle = namedtuple("Obstacle", "center radius vertex cone_type velocity")

SEED = 20250509


def polygon_halfspaces(vertex):
    """CCW 2xk vertices -> (A kx2, b kx1) with the reference's edge rule (mpc.py:476-510)."""
    cur = np.asarray(vertex, float)[0:2]
    nxt = np.roll(cur, -1, axis=1)
    e = nxt - cur
    A = np.stack((e[1], -e[0]), axis=1)
    b = np.sum(A * cur.T, axis=1, keepdims=True)
    return A, b


def rectangle_robot(length=4.6, width=1.6, wheelbase=3.0, dynamics="acker",
                    max_speed=(10, 1), max_acce=(10, 0.5)):
    """Rectangle robot of the example YAMLs (e.g. example/corridor/corridor.yaml:11-16).  The body
    frame origin is the rear axle for a car (x in [-(length-wheelbase)/2, (length+wheelbase)/2])
    and the centre otherwise."""
    if wheelbase:
        x0, x1 = -(length - wheelbase) / 2, (length + wheelbase) / 2
    else:
        x0, x1 = -length / 2, length / 2
    y0, y1 = -width / 2, width / 2
    G, h = polygon_halfspaces(np.array([[x0, x1, x1, x0], [y0, y0, y1, y1]]))
    return car(G, h, "Rpositive", wheelbase, list(max_speed), list(max_acce), dynamics)


def circle_robot(radius=0.8, dynamics="diff", max_speed=(10, 1), max_acce=(10, 0.5)):
    """Circle robot in the form the reference expects for `cone_type == 'norm2'` (rda_solver.py:1034-1039: ||mu[0:-1]|| <= -mu[-1];
    the body {x: G x <=_K h} is the disc of `radius` around the origin, the same encoding mpc.py:440-446 uses for circle obstacles)."""
    G = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
    h = np.array([[0.0], [0.0], [-float(radius)]])
    return car(G, h, "norm2", 0, list(max_speed), list(max_acce), dynamics)


def robot_vertices(car_tuple, state):
    """world-frame vertices (2xk) of a polygon robot at state (x, y, phi)"""
    G, h = np.asarray(car_tuple.G), np.asarray(car_tuple.h).ravel()
    k = G.shape[0]
    V = np.zeros((2, k))
    for i in range(k):
        j = (i - 1) % k
        V[:, i] = np.linalg.solve(np.vstack((G[j], G[i])), np.array([h[j], h[i]]))
    c, s = cos(state[2]), sin(state[2])
    return np.array([[c, -s], [s, c]]) @ V + np.asarray(state[0:2], float).reshape(2, 1)


def box(cx, cy, length, width, yaw, velocity=(0.0, 0.0)):
    c, s = cos(yaw), sin(yaw)
    local = np.array([[-length / 2, length / 2, length / 2, -length / 2],
                      [-width / 2, -width / 2, width / 2, width / 2]])
    V = np.array([[c, -s], [s, c]]) @ local + np.array([[cx], [cy]])
    return Obstacle(None, None, V, "Rpositive", np.array(velocity, float).reshape(2, 1))


def circle(cx, cy, radius, velocity=(0.0, 0.0)):
    return Obstacle(np.array([[cx], [cy]], float), float(radius), None, "norm2",
                    np.array(velocity, float).reshape(2, 1))


def regular_polygon(cx, cy, k, rad, yaw, velocity=(0.0, 0.0)):
    ang = yaw + 2 * np.pi * np.arange(k) / k
    V = np.vstack((cx + rad * np.cos(ang), cy + rad * np.sin(ang)))
    return Obstacle(None, None, V, "Rpositive", np.array(velocity, float).reshape(2, 1))


def line_path(start, goal, step=0.1):
    start, goal = np.asarray(start, float), np.asarray(goal, float)
    n = int(np.ceil(np.linalg.norm(goal[0:2] - start[0:2]) / step))
    th = np.arctan2(goal[1] - start[1], goal[0] - start[0])
    return [np.array([[start[0] + (goal[0] - start[0]) * i / n], [start[1] + (goal[1] - start[1]) * i / n], [th]])
            for i in range(n + 1)]


def gear_path(legs, step=0.1):
    """A path with gear flags for `MPC(enable_reverse=True)` (the reference's example/reverse): waypoints of shape (4, 1) - x, y, heading, gear -
    from straight legs `(start, goal, gear)`, each sampled like `line_path`.  On a leg with gear -1 the robot backs up, so the heading is the
    direction from goal to start.  `MPC.split_path` cuts the result where the gear flips: one piece per run of legs with the same gear."""
    out = []
    for start, goal, gear in legs:
        start, goal = np.asarray(start, float), np.asarray(goal, float)
        if gear not in (1, -1):
            raise ValueError(f"gear_path: gear = {gear!r} is neither +1 nor -1")
        nose = (goal - start)[0:2] if gear == 1 else (start - goal)[0:2]
        th = np.arctan2(nose[1], nose[0])
        out += [np.vstack((p[0:2], [[th]], [[float(gear)]])) for p in line_path(start, goal, step)]
    return out


def path_track_ref():
    """The (137,3,1) reference path of the reference's path_track examples (an INPUT fixture there:
    example/path_track/path_track_ref.npy, byte-identical copies under lidar_nav/ and dynamic_obs/); the numbers
    ship with this package as rda_planner_amd/data/path_track_ref.npy."""
    import os
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "path_track_ref.npy")
    return [np.array(x, float) for x in np.load(p, allow_pickle=False)]


# ---------------------------------------------------------------------------------------------
def scene_path_track():
    """C1: literal obstacle set of example/path_track/path_track_diff.yaml:23-36 (10 circles + 1 polygon)."""
    centres = [[20, 34], [31, 38], [10, 20], [41, 25], [20, 13], [16, 26], [10.5, 24.5], [18, 20], [16, 26], [19, 26]]
    radii = [1.5] + [1.0] * 9
    obs = [circle(c[0], c[1], r) for c, r in zip(centres, radii)]
    obs.append(Obstacle(None, None, np.array([[31, 33, 33, 31], [24, 24, 28, 28.0]]), "Rpositive", np.zeros((2, 1))))
    return obs


def scene_corridor(n_extra=14, seed=SEED):
    """C2: the six rectangles of example/corridor/corridor.yaml:22-33 + seeded 5x2 m boxes (~20 total)."""
    spec = [(30, 25, 0, 70), (30, 15, 0, 70), (10, 18.5, 1.57, 5), (23, 21.5, 1.57, 5), (36, 17, 2.1, 6), (50, 22, 4.3, 5)]
    obs = [box(x, y, ln, 2, yaw) for x, y, yaw, ln in spec]
    rng = np.random.default_rng(seed)
    for _ in range(n_extra):
        obs.append(box(rng.uniform(5, 58), rng.choice([rng.uniform(27, 32), rng.uniform(8, 13)]), 5, 2, rng.uniform(-np.pi, np.pi)))
    return obs


def scene_boxes(n, centre_lo, centre_hi, side=(0.5, 3.0), seed=SEED, keep_clear=None, clear_radius=4.0):
    """C3-style: n seeded 4-vertex boxes (lidar min-area rectangles)."""
    rng = np.random.default_rng(seed)
    obs = []
    while len(obs) < n:
        c = rng.uniform(centre_lo, centre_hi)
        if keep_clear is not None and np.min(np.linalg.norm(keep_clear - c, axis=1)) < clear_radius:
            continue
        obs.append(box(c[0], c[1], rng.uniform(*side), rng.uniform(*side), rng.uniform(-np.pi, np.pi)))
    return obs


def scene_polygons(n, lo=(10, 10), hi=(40, 40), seed=SEED, moving=False, keep_clear=None, clear_radius=3.0):
    """north-star / C4: n regular k-gons (k in {3,4}), circum-radius U[0.5,1.0]; optionally moving U[-1,1]^2 m/s."""
    rng = np.random.default_rng(seed)
    obs = []
    while len(obs) < n:
        c = rng.uniform(lo, hi)
        k = int(rng.choice([3, 4]))
        rad = rng.uniform(0.5, 1.0)
        yaw = rng.uniform(-np.pi, np.pi)
        vel = rng.uniform(-1, 1, 2) if moving else (0.0, 0.0)
        if keep_clear is not None and np.min(np.linalg.norm(keep_clear - c, axis=1)) < clear_radius:
            continue
        obs.append(regular_polygon(c[0], c[1], k, rad, yaw, vel))
    return obs


# ---------------------------------------------------------------------------------------------
def kinematic_step(state, u, car_tuple, dt):
    """what ir-sim's env.step does for the three kinematics (exact Euler as in mpc.py:293-336)"""
    x, y, phi = float(state[0, 0]), float(state[1, 0]), float(state[2, 0])
    v, w = float(u[0, 0]), float(u[1, 0])
    if car_tuple.dynamics == "acker":
        d = np.array([v * cos(phi), v * sin(phi), v * tan(w) / car_tuple.wheelbase])
    elif car_tuple.dynamics == "diff":
        d = np.array([v * cos(phi), v * sin(phi), w])
    else:
        d = np.array([v * cos(w), v * sin(w), 0.0])
    return np.array([[x], [y], [phi]]) + dt * d.reshape(3, 1)


def _clockwise(V):
    """a 2xk polygon runs clockwise: its shoelace sum sum_i (x_i y_i+1 - x_i+1 y_i), every product and sum rounded separately, is negative.  A zero sum
    (no area, or lost to rounding) counts as counter-clockwise"""
    W = np.roll(V, -1, axis=1)
    s = 0.0
    for i in range(V.shape[1]):
        s = s + (V[0, i] * W[1, i] - W[0, i] * V[1, i])
    return s < 0.0


def _poly_sep(P, Q):
    """separating-axis test for two convex polygons given as 2xk arrays -> signed gap (> 0: apart; < 0: minus the penetration depth).  Either winding:
    the edge normals of a clockwise polygon (`_clockwise`) are flipped so that they point outward.  Zero-length edges (a repeated vertex) have no normal
    and are skipped.  Apart, the value is the largest gap along an edge normal of either polygon: the Euclidean distance when that is attained between
    a vertex and an edge, smaller when it is attained between two vertices (two rectangles corner to corner on the diagonal: 1 / sqrt 2 of it) -
    conservative, never above the distance.  Non-convex input is outside the contract; so is a polygon whose shoelace sum is zero."""
    best = -np.inf
    for V, W in ((P, Q), (Q, P)):
        e = np.roll(V, -1, axis=1) - V
        nrm = np.stack((e[1], -e[0]))
        if _clockwise(V):
            nrm = -nrm
        nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=0), 1e-300)
        for i in range(V.shape[1]):
            if e[0, i] == 0.0 and e[1, i] == 0.0:
                continue
            gap = np.min(nrm[:, i] @ W) - nrm[:, i] @ V[:, i]
            best = max(best, gap)
    return best


def clearance(car_tuple, state, obstacles, t=0.0):
    """conservative robot/obstacle clearance: the smallest over the obstacles of
      polygon robot, polygon obstacle   `_poly_sep` of the footprint and the obstacle
      polygon robot, circle obstacle    the distance of the centre to the footprint's nearest edge, negated when the centre lies in the footprint, minus
                                        the radius - the signed distance of the disc to the footprint
      disc robot                        the same with the roles exchanged; disc against disc: centre distance minus both radii
    Polygons of either winding (`_clockwise` decides on which side of an edge the inside is); zero-length edges are skipped.  Negative = overlap."""
    if car_tuple.cone_type == "norm2":                     # circle robot: centre distance minus the radii
        c0 = np.asarray(state, float).ravel()[0:2]
        r0 = -float(np.asarray(car_tuple.h).ravel()[-1])
        out = np.inf
        for o in obstacles:
            if o.cone_type == "norm2":
                out = min(out, np.linalg.norm((o.center + o.velocity * t).ravel() - c0) - o.radius - r0)
            else:
                V = o.vertex + o.velocity * t
                k = V.shape[1]
                cw = _clockwise(V)
                inside = True
                d = np.inf
                for i in range(k):
                    a, b2 = V[:, i], V[:, (i + 1) % k]
                    ab = b2 - a
                    if ab[0] == 0.0 and ab[1] == 0.0:
                        continue
                    s_ = np.clip((c0 - a) @ ab / (ab @ ab), 0, 1)
                    d = min(d, np.linalg.norm(a + s_ * ab - c0))
                    side = ab[0] * (c0[1] - a[1]) - ab[1] * (c0[0] - a[0])
                    inside = inside and ((side <= 0) if cw else (side >= 0))
                out = min(out, (-d if inside else d) - r0)
        return out
    RV = robot_vertices(car_tuple, np.asarray(state, float).ravel())
    cw = _clockwise(RV)
    out = np.inf
    for o in obstacles:
        if o.cone_type == "norm2":
            c = (o.center + o.velocity * t).ravel()
            d = np.inf
            inside = True
            k = RV.shape[1]
            for i in range(k):
                a, b2 = RV[:, i], RV[:, (i + 1) % k]
                ab = b2 - a
                s = np.clip((c - a) @ ab / (ab @ ab), 0, 1)
                d = min(d, np.linalg.norm(a + s * ab - c))
                side = ab[0] * (c[1] - a[1]) - ab[1] * (c[0] - a[0])
                inside = inside and ((side <= 0) if cw else (side >= 0))
            out = min(out, (-d if inside else d) - o.radius)
        else:
            out = min(out, _poly_sep(RV, o.vertex + o.velocity * t))
    return out


# ---------------------------------------------------------------------------------------------
# Fleet members as each other's obstacles: the specification of scene::k_peers_fleet and rollout::k_peer_clearance_fleet
# (rda_fleet_upload_scenes_peers, Fleet.control(peers=True), Fleet.rollout(peers=True)) and the host loop they replace.
def peer_obstacles(cars, states, controls, i):
    """the obstacles member i sees in place of the other members, one per j != i in ascending j: member j's footprint at
    `states[j]` as a polygon that moves with the control `controls[j]` = (v, w) it applied on the previous tick (zero
    before its first tick and from its arrival tick on) along its heading - the heading of `states[j]` for acker / diff,
    w itself for omni, the rule of `kinematic_step`"""
    out = []
    for j in range(len(cars)):
        if j == i:
            continue
        st = np.asarray(states[j], float).ravel()
        v, w = (float(x) for x in np.asarray(controls[j], float).ravel()[0:2])
        a = w if cars[j].dynamics == "omni" else float(st[2])
        out.append(Obstacle(None, None, robot_vertices(cars[j], st), "Rpositive", np.array([[v * cos(a)], [v * sin(a)]])))
    return out


def peer_footprints(cars, states, i):
    """the polygon obstacles member i's LIDAR sees in place of the other members (lidar::k_raycast_fleet_peers, rda_fleet_raycast_peers,
    Fleet.raycast(see_peers=True)): `robot_vertices(cars[j], states[j])` for j != i in ascending j, with zero velocity.  The scan
    of member i is `World.get_lidar_scan` on its world followed by these."""
    return [Obstacle(None, None, robot_vertices(cars[j], np.asarray(states[j], float).ravel()), "Rpositive", np.zeros((2, 1)))
            for j in range(len(cars)) if j != i]


def peer_clearance(cars, states):
    """(B,) every member's separation from the nearest other member: min over j != i of `_poly_sep` of the two
    footprints (negative = overlap); +inf for a fleet of one"""
    RV = [robot_vertices(c, np.asarray(s, float).ravel()) for c, s in zip(cars, states)]
    B = len(RV)
    return np.array([min([_poly_sep(RV[i], RV[j]) for j in range(B) if j != i], default=np.inf) for i in range(B)])


# ---------------------------------------------------------------------------------------------
# Peers predicted along their planned trajectories: the specification of scene::k_build_plan_fleet
# (rda_fleet_*_peers_plan, Fleet.control(peers="plan"), Fleet.rollout(peers="plan")).
PlanObstacle = namedtuple("PlanObstacle", "center radius vertex cone_type velocity A b vertices")


def peer_plan_poses(state_j, plan_j, T):
    """(T+1, 3) the poses a peer is predicted at over the horizon from its state at the start of the tick and its previous
    plan P [3][T+1] (the `opt_state_list` / out_s of its last solve): pose_0 = x_j, pose_t = x_j + (q_t - P[:,1]) with
    q_t = P[:,t+1] for t < T and q_T = P[:,T] + (P[:,T] - P[:,T-1]) - the plan as displacements anchored at the actual
    state, the last increment repeated; x, y and heading alike, every difference and sum rounded separately"""
    x = np.asarray(state_j, float).ravel()[0:3]
    P = np.asarray(plan_j, float).reshape(3, T + 1)
    out = np.zeros((T + 1, 3))
    out[0] = x
    for t in range(1, T + 1):
        q = P[:, t + 1] if t < T else P[:, T] + (P[:, T] - P[:, T - 1])
        out[t] = x + (q - P[:, 1])
    return out


def _ordered_halfspaces(vertex):
    """(A kx2, b kx1) of a convex polygon as MPC.gen_inequal_global gives them: vertices reversed first when they run
    clockwise (all turns collinear counts as clockwise)"""
    V = np.asarray(vertex, float)[0:2]
    o, a, b = V, np.roll(V, -1, axis=1), np.roll(V, -2, axis=1)
    turns = (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    turns = turns[turns != 0]
    if not (turns.size and turns[0] > 0):
        V = V[:, ::-1]
    return polygon_halfspaces(V)


def peer_plan_obstacles(cars, states, controls, plans, valid, i, T, dt=0.1):
    """the obstacles of `peer_obstacles`, in its order, in the form `RDA_solver._stage` takes for time-varying obstacles
    (`isinstance(o.A, list)`), so that a host loop can stage them with `rda_obstacle=True`: `vertices`, `A`, `b` are lists
    of T + 1 per-stage arrays.  A peer j with `valid[j]` is at `peer_plan_poses(states[j], plans[j], T)`; any other peer
    (no solve yet, after a reset, arrived) is predicted at constant velocity like every moving polygon - vertex +
    velocity * (t * dt) above 0.01 m/s, standing below.  `vertex` is the footprint at stage 0, which is what ranks the
    obstacle by distance."""
    out = []
    for o, j in zip(peer_obstacles(cars, states, controls, i), [j for j in range(len(cars)) if j != i]):
        if valid[j]:
            verts = [robot_vertices(cars[j], p) for p in peer_plan_poses(states[j], plans[j], T)]
            verts[0] = o.vertex
        else:
            moving = np.linalg.norm(o.velocity) > 0.01
            verts = [o.vertex + o.velocity * (t * dt) if moving else o.vertex for t in range(T + 1)]
        hs = [_ordered_halfspaces(v) for v in verts]
        out.append(PlanObstacle(None, None, o.vertex, "Rpositive", o.velocity, [h[0] for h in hs], [h[1] for h in hs], verts))
    return out
