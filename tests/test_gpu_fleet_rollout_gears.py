"""-m gpu : the fleet rollout over the gear pieces of reverse paths (rda_upload_path_pieces, rda_fleet_rollout_gears, rollout::k_rollout_advance_gears,
rda_fleet_rollout_last_pieces, Fleet.rollout(gears=True)) against the host-driven loop it replaces: per tick MPC._piece picks the piece, rda_upload_path
brings it to the device when it comes into force, rda_fleet_scene_resort (or rda_fleet_upload_scenes) + rda_fleet_step_tracked run the tick, MPC._end
(mpc.py:166-187) moves to the next piece or reports arrival.  Given a state and a piece, a tick of the rollout runs the same kernels on the same data as
that host-driven tick, so a twin fleet fed the rollout's logged states and pieces must reproduce it bit for bit; the piece rule is recomputed in numpy from
the logs; the plant, plain members, continuation, refusals and the Python surface complete the contract.
Shapes: T = 8, N = 4 slots, E = 4, iter_num = 2, dt = 0.1, speed 3, goal_margin 1, K = 45, 0.1 m between waypoints, 5 polygons beside every lane; the lanes lie 8 m apart and
are slanted by 0.3 rad, so that no heading is zero and the Q12 rewrites of the pieces' last waypoints are not trivially equal.
  member 0 (Ackermann)     forward 3 m, back 2 m, forward 1.5 m
  member 1 (differential)  starts in reverse (2 m), then a piece of two waypoints that is left on the tick it comes into force, then forward 1.5 m
  member 2 (omni)          a plain path of 2 m: it arrives mid-rollout
and B = 1 with member 0."""
import ctypes as C

import numpy as np
import pytest

from fleet_twin_lib import DT, DYN, E, ITER, N, RDA_ERR_ARG, RDA_ERR_HIP, RDA_ERR_UNSUPPORTED, T, FleetTwin, advanced, car, compare_ticks, info_tuple, same_logs
from fleet_twin_lib import hip          # noqa: F401  (the fixture)
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import Info, dptr, iptr

pytestmark = pytest.mark.gpu

K = 45
NOBS = 5
SPEED, MARGIN = 3.0, 1
SLANT = 0.3
LOGS = ("states", "controls", "index", "arrived_at", "piece")


def rows(points):
    return np.ascontiguousarray(np.hstack(points)[0:3, :].T, dtype=float)


def at(e, s, d=0.0):
    """the point s metres along member e's lane and d metres to its left"""
    c, n = np.cos(SLANT), np.sin(SLANT)
    return (4.0 + s * c - d * n, 20.0 + 8.0 * e + s * n + d * c)


def pieces(e, plain=False):
    """member e's pieces [(gear, [L][3])]; plain: one forward piece of 2 m for every member"""
    if plain or e == 2:
        return [(1.0, rows(sc.line_path(at(e, 0), at(e, 2), 0.1)))]
    if e == 0:
        from rda_planner_amd.mpc import MPC
        path = sc.gear_path([(at(e, 0), at(e, 3), 1), (at(e, 3), at(e, 1), -1), (at(e, 1), at(e, 2.5), 1)], 0.1)
        return [(float(p[0][3, 0]), rows(p)) for p in MPC.split_path(None, path)]
    # two consecutive pieces of the same gear: given piece by piece (MPC.split_path only cuts where the gear flips).  The robot ends the reverse piece
    # behind the 1 m mark of its lane (it is still backing up on the tick of the switch), where the second waypoint of the short piece is the nearer one
    # and the first is more than `threshold` away: min_index = 1 = L - goal_margin on the first tick of that piece.
    back = rows(sc.gear_path([(at(e, 3), at(e, 1), -1)], 0.1))
    return [(-1.0, back), (1.0, np.array([[*at(e, 1.1), SLANT], [*at(e, 1.0), SLANT]])), (1.0, rows(sc.line_path(at(e, 1), at(e, 2.5), 0.1)))]


def obstacles(e, moving=False):
    vel = lambda j: (0.2, 0.0) if moving and e < 2 and j % 2 else (0.0, 0.0)         # noqa: E731  (member 2: a scene that does not move)
    return [sc.regular_polygon(*at(e, 1.5 * j - 1.0, 2.6 if j % 2 else -2.6), 3 + j % 2, 0.8, 0.3 * j, velocity=vel(j)) for j in range(NOBS)]


def solver(hip, e, moving=False, plain=False, upload=True, **kw):
    """a fresh handle of member e: its pieces resident (rda_upload_path_pieces; NOT rda_upload_path), its raw scene resident, sorted about the start"""
    from rda_planner_amd.rda_solver import RDA_solver
    sv = RDA_solver(T, car(e), E, N, iter_num=ITER, step_time=DT, time_print=False, **kw)
    pc = pieces(e, plain)
    st = pc[0][1][0].copy()
    if upload:
        lens, gear = np.array([len(p) for _, p in pc], np.int32), np.array([g for g, _ in pc])
        assert hip.upload_path_pieces(sv._be.handle, len(pc), iptr(lens), dptr(gear), dptr(np.ascontiguousarray(np.concatenate([p for _, p in pc])))) == 0
    n, kind, nvert, geom, vel = sv.flatten_scene(obstacles(e, moving))
    kind, nvert = np.ascontiguousarray(kind, np.int32), np.ascontiguousarray(nvert, np.int32)
    geom, vel = np.ascontiguousarray(geom, float), np.ascontiguousarray(vel, float)
    assert n == NOBS and geom.shape == (NOBS, E, 2)
    assert hip.upload_scene(sv._be.handle, int(n), iptr(kind), iptr(nvert), dptr(geom), dptr(vel), dptr(st), 1, None) == 0
    return sv, st, pc, (kind, nvert, geom, vel)


class Twin(FleetTwin):
    """a fleet of fresh handles (members `which`) with their pieces and raw scenes resident"""
    def __init__(self, hip, which=(0, 1, 2), moving=False, plain=False, svs=None):
        self.which = which
        made = svs if svs is not None else [solver(hip, e, moving, plain) for e in which]
        self.make_fleet(hip, [m[0] for m in made], SPEED)
        self.zero = self.cur0
        self.states = np.ascontiguousarray(np.array([m[1] for m in made]))
        self.pieces = [m[2] for m in made]
        self.kind, self.nvert = (np.ascontiguousarray(np.concatenate([m[3][j] for m in made])) for j in (0, 1))
        self.base, self.vel = (np.ascontiguousarray(np.concatenate([m[3][j] for m in made])) for j in (2, 3))
        self.seen = set()                                                          # (member, piece) this fleet has uploaded with rda_upload_path
        self.heads = [[float(p[-1, 2]) for _, p in pc] for pc in self.pieces]      # the heading of every piece's last waypoint as host-driven ticks leave it
        self.piece = [0] * self.B                                                  # ... and the piece in force after the last of them

    def plen(self, i, p):
        return len(self.pieces[i][p][1])

    def rollout(self, k, resort, moving=0, clearance=False, piece0="zero", cur=None, nom_u="first", **over):
        """rda_fleet_rollout_gears -> (rc, dict of logs); over: arguments replaced (None = a missing array)"""
        out = self.logs(k, piece=np.int32, clearance=float if clearance else None)
        a = dict(states=self.states, ref_speed=self.speed, piece0=self.zero if isinstance(piece0, str) else piece0, cur_index=self.zero if cur is None else cur,
                 threshold=0.1, ind_range=10, goal_margin=MARGIN, nom_u=self.nom0 if isinstance(nom_u, str) else nom_u, states_log=out["states"],
                 u_log=out["controls"], index_log=out["index"], info_log=out["info"], arrived_at=out["arrived_at"], piece_log=out["piece"])
        a.update(over)
        rc = self.hip.fleet_rollout_gears(self.F, k, dptr(a["states"]), dptr(a["ref_speed"]), iptr(a["piece0"]), iptr(a["cur_index"]), a["threshold"],
                                          a["ind_range"], a["goal_margin"], resort, moving, dptr(a["nom_u"]), dptr(a["states_log"]), dptr(a["u_log"]),
                                          iptr(a["index_log"]), a["info_log"], iptr(a["arrived_at"]), iptr(a["piece_log"]), dptr(out["clearance"]))
        out["info"] = [info_tuple(i) for i in out["info"]]
        return rc, out

    def plain_rollout(self, k, resort, moving):
        """rda_fleet_rollout / rda_fleet_rollout_moving (with the clearance log) on the members' rda_upload_path paths"""
        out = self.logs(k, clearance=float if moving else None)
        args = (self.F, k, dptr(self.states), dptr(self.speed), iptr(self.zero), 0.1, 10, MARGIN, resort, dptr(self.nom0), dptr(out["states"]),
                dptr(out["controls"]), iptr(out["index"]), out["info"], iptr(out["arrived_at"]))
        rc = self.hip.fleet_rollout_moving(*args, dptr(out["clearance"])) if moving else self.hip.fleet_rollout(*args)
        out["info"] = [info_tuple(i) for i in out["info"]]
        return rc, out

    def last_pieces(self):
        piece, heads = np.full(self.B, -7, np.int32), np.full(sum(len(pc) for pc in self.pieces), np.nan)
        assert self.hip.fleet_rollout_last_pieces(self.F, iptr(piece), dptr(heads)) == 0
        cut = np.cumsum([0] + [len(pc) for pc in self.pieces])
        return piece, [list(heads[cut[i]:cut[i + 1]]) for i in range(self.B)]

    def upload_piece(self, i, p, heads=None):
        """rda_upload_path of member i's piece p (heads: with the end headings a rollout returned)"""
        P = self.pieces[i][p][1].copy()
        if heads is not None:
            P[-1, 2] = heads[i][p]
        assert self.hip.upload_path(self.svs[i]._be.handle, int(P.shape[0]), dptr(P)) == 0

    def host_tick(self, st, piece, cur, first, resort=1, geom=None):
        """one host-driven tick on the pieces `piece`, each uploaded when this fleet meets it for the first time: (re-sort | the scenes uploaded at `geom`,)
        rda_fleet_step_tracked with the signed speeds -> controls, states, infos, min_index, end_heading"""
        B, hip = self.B, self.hip
        st, cur = np.ascontiguousarray(st, float), np.ascontiguousarray(cur, np.int32)
        for i in range(B):
            if (i, int(piece[i])) not in self.seen:
                self.upload_piece(i, int(piece[i]))
                self.seen.add((i, int(piece[i])))
        speed = np.array([self.pieces[i][int(piece[i])][0] * SPEED for i in range(B)])
        if geom is not None:
            assert hip.fleet_upload_scenes(self.F, iptr(np.full(B, NOBS, np.int32)), iptr(self.kind), iptr(self.nvert), dptr(np.ascontiguousarray(geom)),
                                           dptr(self.vel), dptr(np.ascontiguousarray(st[:, 0:2])), iptr(np.full(B, 1, np.int32))) == 0
        elif resort:
            assert hip.fleet_scene_resort(self.F, dptr(st), 3) == 0
        u, s, info, mi, eh = self.step_tracked(st, cur, first, speed)
        for i in range(B):
            p = int(piece[i])
            self.heads[i][p] = float(eh[i])
            self.piece[i] = p + 1 if mi[i] >= self.plen(i, p) - MARGIN and p + 1 < len(self.pieces[i]) else p
        return u, s, info, mi, eh

    def forced(self, logs, n, resort, moving=False, cur0=None, first=True, base=None):
        """n host-driven ticks fed with the logged states, pieces and indices of a rollout (moving: and the numpy-advanced geometry of every tick, from
        `base`, the geometry the rollout found)"""
        out = []
        for k in range(n):
            cur = np.array(self.zero if cur0 is None else cur0) if k == 0 else np.where(logs["piece"][k] != logs["piece"][k - 1], 0, logs["index"][k - 1])
            geom = advanced(self.kind, self.nvert, self.base if base is None else base, self.vel, DT * k)[0] if moving else None
            out.append(self.host_tick(logs["states"][k], logs["piece"][k], cur, first and k == 0, resort, geom))
        return out


def next_inputs(logs, piece_after):
    """the cur_index of the tick behind a rollout, as MPC._end leaves it: 0 for a member whose last tick changed its piece, else the last min_index"""
    return np.ascontiguousarray(np.where(piece_after != logs["piece"][-1], 0, logs["index"][-1]).astype(np.int32))


CASES = {"resort": ((0, 1, 2), 1, 0), "no-resort": ((0, 1, 2), 0, 0), "moving": ((0, 1, 2), 1, 1), "B1": ((0,), 1, 0)}


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def run(hip, request):
    """ONE gear rollout of K ticks, what rda_fleet_rollout_last_pieces says behind it, a host-driven tick that continues it - and the teacher-forced twin of
    all of it, shared by the tests below"""
    which, resort, moving = CASES[request.param]
    a, b = Twin(hip, which, moving), Twin(hip, which, moving)
    rc, logs = a.rollout(K, resort, moving, clearance=bool(moving))
    assert rc == 0, rc
    out = dict(case=request.param, which=which, resort=resort, moving=moving, logs=logs, pieces=a.pieces, last=a.last_pieces())
    out["ticks"] = b.forced(logs, K, resort, moving)
    out["twin_last"] = (list(b.piece), [list(h) for h in b.heads])
    # the host-driven tick K: the rolled-out fleet brings the piece in force to the device with rda_upload_path, carrying the heading the rollout returned
    piece, heads = out["last"]
    cur = next_inputs(logs, piece)
    for i in range(a.B):
        a.upload_piece(i, int(piece[i]), heads)
        a.seen.add((i, int(piece[i])))
    geom = advanced(a.kind, a.nvert, a.base, a.vel, DT * K)[0] if moving else None
    out["cont_a"] = a.host_tick(logs["states"][K], piece, cur, False, resort, geom)
    out["cont_b"] = b.host_tick(logs["states"][K], piece, cur, False, resort, geom)
    a.close(); b.close()
    return out


def same_as_forced(logs, ticks):
    """the ticks of a rollout against host-driven ticks from its logged states: for every live member the first control, min_index, the ADMM iterations
    and the whole rda_info, for equality -> the number of live (member, tick) pairs"""
    return compare_ticks(logs, ticks, what=("controls", "index", "iters", "info"), arrived_too=False)


def test_teacher_forced_twin_bit_for_bit(run):
    """every tick of the rollout against the host-driven tick from the same logged state on the same piece (uploaded with rda_upload_path on the first tick
    the log names it, cur_index = 0 at a switch, speed = gear * 3): first control, min_index, the ADMM iterations and the whole rda_info of every live
    member - the same kernels on the same inputs, so equality and nothing else"""
    logs = run["logs"]
    moved = same_as_forced(logs, run["ticks"])
    assert moved >= 22 and np.abs(logs["controls"][:, 0, 0]).max() > 1.0         # the members drive: member 0's 6.5 m take 22 ticks of 0.3 m at least


def test_piece_rule(run):
    """MPC._end recomputed in numpy from index_log and the piece lengths alone: a member moves to the next piece exactly on the tick whose min_index reaches
    Lp - goal_margin while a piece follows, with that tick's control applied; it arrives on the first such tick of its LAST piece, with zero controls and a
    standing state from then on"""
    logs, pcs = run["logs"], run["pieces"]
    piece, index, arrived, U, S = logs["piece"], logs["index"], logs["arrived_at"], logs["controls"], logs["states"]
    print("piece_log\n", piece.T, "\nindex_log\n", index.T, "\narrived_at", arrived)
    for i, pc in enumerate(pcs):
        P = len(pc)
        assert piece[0, i] == 0
        want_arrival = -1
        for k in range(K):
            p = piece[k, i]
            at_end = index[k, i] >= len(pc[p][1]) - MARGIN
            switch = at_end and p + 1 < P
            if k + 1 < K:
                assert piece[k + 1, i] == p + (1 if switch else 0), (i, k)
            if switch:
                assert U[k, i, 0] != 0.0, (i, k)                                  # not an arrival: the control of a switching tick is applied
            if at_end and p + 1 == P and want_arrival < 0:
                want_arrival = k
        assert arrived[i] == want_arrival, i
        if want_arrival >= 0:
            assert np.all(U[want_arrival:, i] == 0.0) and np.all(S[want_arrival:, i] == S[want_arrival, i]), i
            assert np.all(piece[want_arrival:, i] == P - 1), i
        # reversing is seen: on every piece long enough to pick up speed the member drives in the direction of the gear
        for p, (gear, pts) in enumerate(pc):
            v = U[piece[:, i] == p, i, 0]
            if len(pts) > 2:
                assert v.size and (v.min() < -0.1 if gear < 0 else v.max() > 0.1), (i, p, gear)
        assert piece[-1, i] == P - 1, i                                           # 45 ticks are enough for every member to reach its last piece
    if run["which"] == (0, 1, 2):
        ks = np.nonzero(piece[:, 1] == 1)[0]
        assert ks.size == 1 and piece[ks[0] - 1, 1] == 0 and piece[ks[0] + 1, 1] == 2        # three pieces on three consecutive ticks
        assert 3 < arrived[2] < K - 3                                             # the plain member arrives mid-rollout


def test_kinematics_follow_the_host_loop(run):
    """states_log[k+1] against the expressions of tools/closed_loop_host.c:134-136 evaluated in numpy on states_log[k], u_log[k], switching ticks included.
    Bound 1e-13 (tests/test_gpu_fleet_rollout.py): the device's sin / cos / tan are within a few ulp of libm's, dt |v| <= 1 here, every other operation is the
    same separately rounded double operation, so the true difference is of the order of 1e-15"""
    S, U = run["logs"]["states"], run["logs"]["controls"]
    worst = 0.0
    for i, e in enumerate(run["which"]):
        wb = car(e).wheelbase
        for k in range(K):
            x, y, th = S[k, i]
            v, w = U[k, i]
            if DYN[e] == "acker":
                want = (x + DT * (v * np.cos(th)), y + DT * (v * np.sin(th)), th + DT * (v * np.tan(w) / wb))
            elif DYN[e] == "diff":
                want = (x + DT * (v * np.cos(th)), y + DT * (v * np.sin(th)), th + DT * w)
            else:
                want = (x + DT * (v * np.cos(w)), y + DT * (v * np.sin(w)), th)
            worst = max(worst, float(np.abs(S[k + 1, i] - np.array(want)).max()))
    print(f"max |state - host expression| = {worst:.3e}")
    assert worst <= 1e-13
    assert np.abs(DT * U[:, :, 0]).max() <= 1.0


def test_last_pieces_and_the_host_loop_continue(run):
    """rda_fleet_rollout_last_pieces against the twin - every member's piece after the last tick and the heading of the last waypoint of EVERY piece (Q12) -
    and a host-driven tick behind the rollout, on the rda_upload_path path, against the twin's: everything it returns"""
    piece, heads = run["last"]
    want_piece, want_heads = run["twin_last"]
    print("piece", piece, want_piece, "\nheads", heads, "\n     ", want_heads)
    assert list(piece) == want_piece
    assert heads == want_heads
    for x, y in zip(run["cont_a"], run["cont_b"]):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y


def test_second_rollout_continues_the_first(hip, run):
    """K1 ticks, then the rest continued from what the first call returned: the ticks of the one long rollout.  A scene that moves is the exception the
    moving rollout always had: the second call takes the geometry it finds as its base, base2 + vel * (dt * k) is not base + vel * (dt * (K1 + k)) to the
    last bit, so there the continued ticks are held against host-driven ticks on the geometry advanced from base2 (tests/test_gpu_fleet_rollout_moving.py)."""
    K1 = 20
    long, moving = run["logs"], run["moving"]
    a = Twin(hip, run["which"], moving)
    rc, l1 = a.rollout(K1, run["resort"], moving)
    assert rc == 0, rc
    piece, _ = a.last_pieces()
    rc, l2 = a.rollout(K - K1, run["resort"], moving, piece0=piece, cur=next_inputs(l1, piece), nom_u=None, states=np.ascontiguousarray(l1["states"][K1]))
    assert rc == 0, rc
    a.close()
    if moving:
        b = Twin(hip, run["which"], moving)
        b.forced(l1, K1, run["resort"], True)
        base2 = advanced(b.kind, b.nvert, b.base, b.vel, DT * K1)[0]
        assert same_as_forced(l2, b.forced(l2, K - K1, run["resort"], True, cur0=next_inputs(l1, piece), first=False, base=base2)) > 0
        b.close()
        assert np.array_equal(l2["piece"][-1], long["piece"][-1])
        return
    for key in ("controls", "index", "piece"):
        assert np.array_equal(np.concatenate([l1[key], l2[key]]), long[key]), key
    assert np.array_equal(np.concatenate([l1["states"], l2["states"][1:]]), long["states"])
    assert l1["info"] + l2["info"] == long["info"]
    want1 = np.where((long["arrived_at"] >= 0) & (long["arrived_at"] < K1), long["arrived_at"], -1)
    want2 = np.where(long["arrived_at"] < 0, -1, np.maximum(long["arrived_at"] - K1, 0))       # (a member that stands arrives again on the first tick)
    assert np.array_equal(l1["arrived_at"], want1) and np.array_equal(l2["arrived_at"], want2)


@pytest.mark.parametrize("moving", [0, 1], ids=["static", "moving"])
def test_plain_members_change_nothing(hip, moving):
    """a fleet of plain members only, one piece each: the logs of rda_fleet_rollout / rda_fleet_rollout_moving on a twin (rda_upload_path paths), and a piece
    log of zeros"""
    k = 12
    a, b = Twin(hip, moving=bool(moving), plain=True), Twin(hip, moving=bool(moving), plain=True)
    for i in range(b.B):
        b.upload_piece(i, 0)
    rc, la = a.rollout(k, 1, moving, clearance=bool(moving))
    assert rc == 0, rc
    rc, lb = b.plain_rollout(k, 1, moving)
    assert rc == 0, rc
    same_logs(la, lb, ("states", "controls", "index", "arrived_at") + (("clearance",) if moving else ()))
    print("arrived_at", la["arrived_at"])
    assert np.all(la["piece"] == 0) and np.abs(la["controls"][0, :, 0]).min() > 0.1      # ... of members that drive
    a.close(); b.close()


def test_refusals_queue_and_change_nothing(hip):
    """every refusal returns its code; the fleet that was refused then rolls out exactly like a twin that never was"""
    a, b = Twin(hip), Twin(hip)
    B = a.B
    for k in (0, -1, 4097):
        assert a.rollout(k, 1)[0] == RDA_ERR_ARG, k
    for key in ("states", "ref_speed", "piece0", "cur_index", "states_log", "u_log", "index_log", "arrived_at", "piece_log"):
        assert a.rollout(2, 1, **{key: None})[0] == RDA_ERR_ARG, key
    assert a.rollout(2, 1, ind_range=0)[0] == RDA_ERR_ARG and a.rollout(2, 1, goal_margin=0)[0] == RDA_ERR_ARG
    assert a.rollout(2, 1, 0, clearance=True)[0] == RDA_ERR_ARG                   # the clearance log belongs to the moving form
    for bad in (-1, len(a.pieces[1])):
        p0 = np.zeros(B, np.int32); p0[1] = bad
        assert a.rollout(2, 1, piece0=p0)[0] == RDA_ERR_ARG, bad
    for p, bad in ((0, -1), (0, a.plen(1, 0)), (1, 2)):                            # cur_index outside the piece named by piece0
        p0, cur = np.zeros(B, np.int32), np.zeros(B, np.int32)
        p0[1], cur[1] = p, bad
        assert a.rollout(2, 1, piece0=p0, cur=cur)[0] == RDA_ERR_ARG, (p, bad)
    h = a.svs[0]._be.handle
    one, gear, pts = np.ones(1, np.int32), np.ones(1), np.zeros((1, 3))
    assert hip.upload_path_pieces(h, 0, iptr(one), dptr(gear), dptr(pts)) == RDA_ERR_ARG
    assert hip.upload_path_pieces(h, 1, iptr(np.zeros(1, np.int32)), dptr(gear), dptr(pts)) == RDA_ERR_ARG
    assert hip.upload_path_pieces(h, 1, None, dptr(gear), dptr(pts)) == RDA_ERR_ARG and hip.upload_path_pieces(h, 1, iptr(one), dptr(gear), None) == RDA_ERR_ARG
    assert hip.fleet_rollout_last_pieces(a.F, None, None) == RDA_ERR_ARG          # no gear rollout yet
    rc, la = a.rollout(3, 1, info_log=None)                                       # (info_log may be missing)
    assert rc == 0
    rc, lb = b.rollout(3, 1)
    assert rc == 0
    lb["info"] = la["info"]
    same_logs(la, lb, LOGS)
    a.close(); b.close()
    # a member without resident pieces (its rda_upload_path path does not count)
    f = Twin(hip, (0,), svs=[solver(hip, 0, upload=False)])
    f.upload_piece(0, 0)
    assert f.rollout(2, 1)[0] == RDA_ERR_ARG
    f.close()
    f = Twin(hip, (0,), svs=[solver(hip, 0, duals_follow_obstacles=True)])        # a refusal of the entry it extends
    assert f.rollout(2, 1)[0] == RDA_ERR_UNSUPPORTED
    f.close()
    f = Twin(hip, (0,), svs=[solver(hip, 0, moving=True)])                        # per-stage slots: the scene moves, moving = 0 refuses it
    assert f.rollout(2, 1, 0)[0] == RDA_ERR_UNSUPPORTED
    f.close()


def test_refused_allocations_change_nothing(hip):
    """the first gear rollout of a fleet makes every table it needs - tracking, re-sort, rollout, logs (20 allocations, tests/test_gpu_fleet_rollout.py) and
    the gear tables, the piece log and the heading array (4 + 1 + 1 device arrays with their pinned mirrors: 12): refused at each of them it returns
    RDA_ERR_HIP and holds nothing more than before; the call that gets through gives the logs of an undisturbed twin.  The same for a refused upload of
    pieces, which leaves the old pieces in place."""
    def alive():
        n, by = C.c_longlong(0), C.c_longlong(0)
        assert hip.debug_alloc_stats(C.byref(n), C.byref(by)) == 0
        return n.value, by.value
    a, b = Twin(hip), Twin(hip)
    pc = a.pieces[0]
    lens, gear, pts = np.array([len(p) for _, p in pc], np.int32), np.array([g for g, _ in pc]), np.ascontiguousarray(np.concatenate([p for _, p in pc]))
    for n in range(3):                                                            # buf, off, gear
        before = alive()
        hip.debug_alloc_fail(n)
        try:
            rc = hip.upload_path_pieces(a.svs[0]._be.handle, 2, iptr(lens[:2]), dptr(gear), dptr(pts))
        finally:
            hip.debug_alloc_fail(-1)
        assert rc == RDA_ERR_HIP and alive() == before, n
    rc, n = RDA_ERR_HIP, 0
    while rc == RDA_ERR_HIP and n < 60:
        before = alive()
        hip.debug_alloc_fail(n)
        try:
            rc, la = a.rollout(K, 1)
        finally:
            hip.debug_alloc_fail(-1)
        assert rc == 0 or (rc == RDA_ERR_HIP and alive() == before), (n, rc)
        n += 1
    assert rc == 0 and n - 1 == 32, n
    rc, lb = b.rollout(K, 1)
    assert rc == 0
    same_logs(la, lb, LOGS)                                                         # (all three pieces of member 0: the refused uploads changed nothing)
    a.close(); b.close()


def reverse_fleet():
    """the three members as MPC objects and a fleet of them, after one tick of Fleet.control (it stages the scenes) -> fleet, obstacle lists, states"""
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    ms, obs, states = [], [], []
    for e in range(3):
        pc = pieces(e)
        lists = [[np.array([[x], [y], [th], [g]]) for x, y, th in pts] for g, pts in pc]
        path = [w for p in lists for w in p]
        m = MPC(car(e), path if e < 2 else [w[0:3].copy() for w in path], receding=T, sample_time=DT, iter_num=ITER, max_edge_num=E, max_obs_num=N,
                goal_index_threshold=MARGIN, enable_reverse=e < 2)
        if e == 1:
            m.curve_list = lists                       # two consecutive pieces of one gear: not what split_path makes of the flags
        if e < 2:
            assert [len(p) for p in m.curve_list] == [len(pts) for _, pts in pc]
        ms.append(m); obs.append(obstacles(e)); states.append(np.array(pc[0][1][0]).reshape(3, 1))
    f = Fleet(ms)
    res = f.control([s.copy() for s in states], SPEED, [list(o) for o in obs])
    return f, obs, [sc.kinematic_step(states[i], res[i][0], car(i), DT) for i in range(3)]


def test_python_rollout(hip):
    """Fleet.rollout(gears=True) after a tick of Fleet.control: the arrays of the C call on a twin fleet, "piece", the members' bookkeeping as MPC._end leaves
    it, the headings written back, and Fleet.control goes on on the right piece"""
    steps = 12
    fa, obs, states = reverse_fleet()
    fb, _, _ = reverse_fleet()
    out = fa.rollout([s.copy() for s in states], SPEED, steps, gears=True)
    for m in fb.members:
        m.rda.upload_path_pieces(fb._gear_pieces(m))
    st = np.ascontiguousarray(np.array([s.ravel() for s in states]))
    cur, p0 = np.array([m.cur_index for m in fb.members], np.int32), np.array([m.curve_index if m.enable_reverse else 0 for m in fb.members], np.int32)
    want = dict(states=np.zeros((steps + 1, 3, 3)), controls=np.zeros((steps, 3, 2)), index=np.zeros((steps, 3), np.int32), arrived_at=np.zeros(3, np.int32),
                piece=np.zeros((steps, 3), np.int32))
    infos = (Info * (steps * 3))()
    assert hip.fleet_rollout_gears(fb._handle, steps, dptr(st), dptr(np.full(3, SPEED)), iptr(p0), iptr(cur), 0.1, 10, MARGIN, 1, 0, None, dptr(want["states"]),
                                   dptr(want["controls"]), iptr(want["index"]), infos, iptr(want["arrived_at"]), iptr(want["piece"]), None) == 0
    assert out["piece"].shape == (steps, 3) and out["piece"].dtype == np.int32
    for key in want:
        assert np.array_equal(out[key], want[key]), key
    assert np.array_equal(out["iters"], np.array([i.iters for i in infos]).reshape(steps, 3))
    piece, heads = np.zeros(3, np.int32), np.zeros(7)
    assert hip.fleet_rollout_last_pieces(fb._handle, iptr(piece), dptr(heads)) == 0
    print("piece\n", out["piece"].T, "\narrived_at", out["arrived_at"], "after", piece)
    assert out["arrived_at"][0] < 0 and out["arrived_at"][1] < 0 and out["arrived_at"][2] >= 0 and out["piece"][:, 1].max() >= 1
    at = 0
    for i, m in enumerate(fa.members):
        pcs = fa._gear_pieces(m)
        assert [float(p[-1][2, 0]) for p in pcs] == list(heads[at:at + len(pcs)]), i
        at += len(pcs)
        assert m._dev_path_key is None
        assert np.array_equal(np.asarray(m.state).ravel(), out["states"][-1, i])
        if out["arrived_at"][i] >= 0:
            assert np.all(m.cur_vel_array == 0.0) and m._dev_u is None and m.cur_index == out["index"][-1, i]      # (the plain member)
        else:
            assert m.curve_index == piece[i]
            assert m.cur_index == (0 if piece[i] != out["piece"][-1, i] else out["index"][-1, i])
            assert m._nominal_u() is None and m.cur_vel_array.shape == (2, T) and m.cur_vel_array[0, 0] == out["controls"][-1, i, 0]
    res = fa.control([out["states"][-1, i].reshape(3, 1) for i in range(3)], SPEED, [list(o) for o in obs])
    for i, (u, info) in enumerate(res):
        assert u.shape == (2, 1) and np.isfinite(u).all() and info["iters"] >= 1
        m = fa.members[i]
        if i < 2:
            assert not info["arrive"] and m._dev_path_key[0] is m.curve_list[piece[i]]        # the piece the rollout ended on went to the device
    fa.close(); fb.close()


def test_python_rollout_against_the_host_loop(hip):
    """K ticks as one gear rollout and as the loop Fleet.control + scenarios.kinematic_step, same scene: every member goes through the same pieces, each switch
    and the arrival at most one tick apart (a last-bit difference in a state can move min_index across the boundary by one tick, and by no more).  The
    largest state difference is printed, not bounded."""
    fa, obs, states = reverse_fleet()
    fb, _, _ = reverse_fleet()
    out = fa.rollout([s.copy() for s in states], SPEED, K, gears=True)
    S, piece, arrived = np.zeros((K + 1, 3, 3)), np.zeros((K, 3), np.int32), np.full(3, -1)
    cur = [s.copy() for s in states]
    S[0] = np.array([s.ravel() for s in cur])
    for k in range(K):
        for i, m in enumerate(fb.members):
            if arrived[i] >= 0 and m.enable_reverse:                              # it stands at the end of its last piece
                m.curve_index, m.cur_index = len(m.curve_list) - 1, len(m.curve_list[-1]) - 1
            piece[k, i] = m.curve_index if m.enable_reverse else 0
        res = fb.control([s.copy() for s in cur], SPEED, [list(o) for o in obs])
        for i, (u, info) in enumerate(res):
            if info["arrive"] and arrived[i] < 0:
                arrived[i] = k
            cur[i] = sc.kinematic_step(cur[i], u, car(i), DT)
        S[k + 1] = np.array([s.ravel() for s in cur])
    print("rollout pieces\n", out["piece"].T, "\nhost loop pieces\n", piece.T, "\narrived_at", out["arrived_at"], arrived)
    print(f"max |state(rollout) - state(host loop)| over {K} ticks = {np.abs(out['states'] - S).max():.3e}")
    for i in range(3):
        ka, kb = np.nonzero(np.diff(out["piece"][:, i]))[0], np.nonzero(np.diff(piece[:, i]))[0]
        assert list(out["piece"][ka + 1, i]) == list(piece[kb + 1, i]) and len(ka) == len(fa._gear_pieces(fa.members[i])) - 1, i
        assert np.abs(ka - kb).max(initial=0) <= 1, (i, ka, kb)
        assert (out["arrived_at"][i] < 0) == (arrived[i] < 0) and abs(int(out["arrived_at"][i]) - int(arrived[i])) <= 1, i
    fa.close(); fb.close()
