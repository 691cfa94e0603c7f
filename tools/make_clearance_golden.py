"""tests/golden/clearance_parent.npz: sound clearance inputs and what `scenarios.clearance` / `scenarios.peer_clearance` return for them at the commit this
is run on.  It was run on the commit BEFORE clearance learnt about winding, repeated vertices and enclosed circles, so that tests/test_clearance_exact.py
can hold the later routines to those values bit for bit.  Sound: every polygon counter-clockwise without a repeated vertex, every circle centre outside
the robot's footprint (for a disc robot: any convex counter-clockwise polygon).  Only numbers are stored; running it again on a later commit must
reproduce the file (`--check`).

    python tools/make_clearance_golden.py            # writes the file
    python tools/make_clearance_golden.py --check    # compares with the committed file, bit for bit
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from rda_planner_amd import scenarios as sc      # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "clearance_parent.npz")
EMAX = 8
N_POLY, N_CIRC, N_DISC, N_PEER = 120, 50, 30, 30


def robot(k, rng):
    """a counter-clockwise k-gon robot: the default car for k = 4, else an irregular convex polygon about the origin"""
    if k == 4:
        return sc.rectangle_robot(dynamics="diff", wheelbase=0)
    ang = np.sort(rng.uniform(0, 2 * np.pi / k, k) + 2 * np.pi * np.arange(k) / k)
    V = np.vstack((1.8 * np.cos(ang), 0.9 * np.sin(ang)))
    G, h = sc.polygon_halfspaces(V)
    return sc.car(G, h, "Rpositive", 0, [10, 1], [10, 0.5], "diff")


def outside(RV, c):
    """centre c strictly outside the counter-clockwise polygon RV (some edge sees it on its right by a margin)"""
    e = np.roll(RV, -1, axis=1) - RV
    cr = e[0] * (c[1] - RV[1]) - e[1] * (c[0] - RV[0])
    return bool(np.any(cr < -1e-3 * np.linalg.norm(e, axis=0)))


def build():
    rng = np.random.default_rng(sc.SEED + 77)
    robots = [robot(k, rng) for k in (3, 4, 6, 8)]
    out = dict(robot_R=np.array([r.G.shape[0] for r in robots], np.int32), robot_G=np.zeros((4, EMAX, 2)), robot_h=np.zeros((4, EMAX)))
    for i, r in enumerate(robots):
        out["robot_G"][i, :r.G.shape[0]] = r.G
        out["robot_h"][i, :r.G.shape[0]] = np.asarray(r.h).ravel()
    # polygon robot against one polygon / one circle, moving ones evaluated at t
    n = N_POLY + N_CIRC
    ridx, state, kind, nvert = np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros(n, np.int32), np.zeros(n, np.int32)
    geom, radius, vel, tt, want = np.zeros((n, EMAX, 2)), np.zeros(n), np.zeros((n, 2)), np.zeros(n), np.zeros(n)
    i = 0
    while i < n:
        r = int(rng.integers(0, 4))
        scale = 100.0 if i % 3 == 0 else 10.0
        st = np.array([rng.uniform(-scale, scale), rng.uniform(-scale, scale), rng.uniform(-np.pi, np.pi)])
        dist, ang = rng.choice([0.3, 1.5, 3.0, 6.0]) * rng.uniform(0.5, 1.5), rng.uniform(-np.pi, np.pi)
        c = st[0:2] + dist * np.array([np.cos(ang), np.sin(ang)])
        v = rng.uniform(-1, 1, 2) if i % 4 == 0 else np.zeros(2)
        t = float(rng.uniform(0, 2)) if i % 4 == 0 else 0.0
        if i < N_POLY:
            k = int(rng.integers(3, EMAX + 1))
            o = sc.regular_polygon(c[0], c[1], k, rng.uniform(0.3, 2.0), rng.uniform(-np.pi, np.pi), velocity=v)
            nvert[i], geom[i, :k] = k, o.vertex.T
        else:
            o = sc.circle(c[0], c[1], rng.uniform(0.1, 1.5), velocity=v)
            if not outside(sc.robot_vertices(robots[r], st), (o.center + o.velocity * t).ravel()):
                continue
            kind[i], geom[i, 0], radius[i] = 1, o.center.ravel(), o.radius
        ridx[i], state[i], vel[i], tt[i] = r, st, v, t
        want[i] = sc.clearance(robots[r], st, [o], t=t)
        i += 1
    out.update(ridx=ridx, state=state, kind=kind, nvert=nvert, geom=geom, radius=radius, vel=vel, t=tt, want=want)
    # disc robot against one counter-clockwise polygon / one circle
    d_rad, d_state, d_kind, d_nvert = np.zeros(N_DISC), np.zeros((N_DISC, 3)), np.zeros(N_DISC, np.int32), np.zeros(N_DISC, np.int32)
    d_geom, d_radius, d_want = np.zeros((N_DISC, EMAX, 2)), np.zeros(N_DISC), np.zeros(N_DISC)
    for i in range(N_DISC):
        d_rad[i] = rng.uniform(0.2, 1.0)
        st = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), 0.0])
        c = st[0:2] + rng.uniform(0.0, 4.0) * np.array([np.cos(i), np.sin(i)])
        if i % 3 == 2:
            o = sc.circle(c[0], c[1], rng.uniform(0.1, 1.5))
            d_kind[i], d_geom[i, 0], d_radius[i] = 1, o.center.ravel(), o.radius
        else:
            k = int(rng.integers(3, EMAX + 1))
            o = sc.regular_polygon(c[0], c[1], k, rng.uniform(0.3, 2.0), rng.uniform(-np.pi, np.pi))
            d_nvert[i], d_geom[i, :k] = k, o.vertex.T
        d_state[i] = st
        d_want[i] = sc.clearance(sc.circle_robot(d_rad[i]), st, [o])
    out.update(disc_rad=d_rad, disc_state=d_state, disc_kind=d_kind, disc_nvert=d_nvert, disc_geom=d_geom, disc_radius=d_radius, disc_want=d_want)
    # pairs and triples of footprints (a triple: p_ridx[:, 2] >= 0)
    p_ridx, p_state, p_want = np.full((N_PEER, 3), -1, np.int32), np.zeros((N_PEER, 3, 3)), np.full((N_PEER, 3), np.inf)
    for i in range(N_PEER):
        m = 2 + i % 2
        c0 = rng.uniform(-80, 80, 2)
        for j in range(m):
            p_ridx[i, j] = int(rng.integers(0, 4))
            p_state[i, j] = [c0[0] + rng.uniform(-4, 4), c0[1] + rng.uniform(-4, 4), rng.uniform(-np.pi, np.pi)]
        p_want[i, :m] = sc.peer_clearance([robots[k] for k in p_ridx[i, :m]], p_state[i, :m])
    out.update(peer_ridx=p_ridx, peer_state=p_state, peer_want=p_want)
    return out


if __name__ == "__main__":
    data = build()
    if "--check" in sys.argv:
        old = np.load(OUT)
        bad = [k for k in data if not np.array_equal(old[k], data[k])]
        print("differs:" if bad else "identical", bad)
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes;", "negative", int((data["want"] < 0).sum()), "of", len(data["want"]))
