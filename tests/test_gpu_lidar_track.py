"""-m gpu : lidar boxes tracked across ticks on the device and staged with velocities (lidar::k_track_boxes_fleet; rda_fleet_track_boxes, rda_fleet_box_tracks,
rda_fleet_reset_tracks, rda_fleet_upload_scans_tracked, rda_fleet_rollout_lidar_tracked; Fleet.control(scans=, track=True), Fleet.rollout(lidar=, track=True)).

1  the tracker alone against lidar.track_boxes (the specification), for equality, velocities and table, over crafted sequences
2  a host-driven tracked tick against rda_fleet_upload_scenes of the device's own boxes as polygons with the specification's velocities, on a twin
3  a tracked rollout tick against the teacher-forced host-driven tracked tick, blind and seeing (the pattern of tests/test_gpu_fleet_rollout_lidar_peers.py)
4  a box that crosses the lane: hit without track, avoided with it (tests/test_lidar_track.py has the scene's CPU numbers)
5  the untracked rollout is what it was; refusals; refused allocations change nothing
6  members in the interior-point LamMuZ mode take the tracked slots; Fleet.control(scans=, track=True) keeps the table of the specification

Shapes: those of tests/test_gpu_fleet_rollout_lidar_peers.py - T = 8, N = 4, E = 4, iter_num = 2, dt = 0.1, B = 3 on the lanes, 65 beams (a partial second
wave of the ray caster), eps 2.0, min_samples 4, K = 4; the tracker alone with 0, 5 and 257 boxes per member (none | some | more than MAX_TRACKS = 256: the
last box gets no track); the crossing scene at T = 12, 360 beams, 40 ticks."""
import ctypes as C

import numpy as np
import pytest

import lidar_track_lib as L
from fleet_twin_lib import DT, E, MARGIN, RDA_ERR_ARG, RDA_ERR_UNSUPPORTED, T, advanced, bare_fleet, car, info_tuple, refused_in_turn, same_logs
from lidar_world_lib import EPS
from rda_planner_amd import lidar
from rda_planner_amd._capi import dptr, iptr
from test_gpu_fleet_rollout_lidar import LOGS
from test_gpu_fleet_rollout_lidar_peers import BEAMS, MINS, PTwin, plant

pytestmark = pytest.mark.gpu

K, GATE, WINDOW = 4, 1.0, 8
CAP = 260


class TTwin(PTwin):
    """that file's twin with the tracked entries"""
    def rollout_tracked(self, k, moving, see, clearance=True, gate=GATE, window=WINDOW, **over):
        """rda_fleet_rollout_lidar_tracked -> (rc, dict of logs); over: arguments replaced (None = a missing array)"""
        out = self.logs(k, boxes=np.int32, clearance=float if clearance else None, peer_clearance=float if see else None)
        nb, lo, hi, rmin, rmax = self.sensors
        a = dict(states=self.states, ref_speed=self.speed, cur_index=self.cur0, threshold=0.1, ind_range=10, goal_margin=MARGIN, nom_u=self.nom0,
                 n_beams=nb, angle_min=lo, angle_max=hi, range_min=rmin, range_max=rmax, eps=EPS, min_samples=MINS, order=self.order,
                 states_log=out["states"], u_log=out["controls"], index_log=out["index"], info_log=out["info"], arrived_at=out["arrived_at"],
                 nbox_log=out["boxes"])
        a.update(over)
        rc = self.hip.fleet_rollout_lidar_tracked(self.F, k, dptr(a["states"]), dptr(a["ref_speed"]), iptr(a["cur_index"]), a["threshold"], a["ind_range"],
                                                  a["goal_margin"], dptr(a["nom_u"]), iptr(a["n_beams"]), dptr(a["angle_min"]), dptr(a["angle_max"]),
                                                  dptr(a["range_min"]), dptr(a["range_max"]), a["eps"], a["min_samples"], iptr(a["order"]), moving,
                                                  dptr(a["states_log"]), dptr(a["u_log"]), iptr(a["index_log"]), a["info_log"], iptr(a["arrived_at"]),
                                                  iptr(a["nbox_log"]), dptr(out["clearance"]), dptr(out["peer_clearance"]), see, gate, window)
        out["info"] = [info_tuple(i) for i in out["info"]]
        return rc, out

    def cast(self, st, see=0):
        nb, lo, hi, rmin, rmax = self.sensors
        ranges = np.zeros(int(nb.sum()) + 1)
        f = self.hip.fleet_raycast_peers if see else self.hip.fleet_raycast
        assert f(self.F, iptr(nb), dptr(lo), dptr(hi), dptr(rmin), dptr(rmax), dptr(st), dptr(ranges)) == 0
        return ranges

    def upload_tracked(self, st, ranges, gate=GATE, window=WINDOW, **over):
        nb, lo, hi, rmin, rmax = self.sensors
        boxes = np.full(self.B, -7, np.int32)
        a = dict(n_beams=nb, ranges=ranges, states=st, order=self.order, eps=EPS, min_samples=MINS)
        a.update(over)
        rc = self.hip.fleet_upload_scans_tracked(self.F, iptr(a["n_beams"]), dptr(a["ranges"]), dptr(lo), dptr(hi), dptr(rmax), dptr(a["states"]), a["eps"],
                                                 a["min_samples"], iptr(a["order"]), iptr(boxes), gate, window)
        return rc, boxes

    def host_tick_tracked(self, st, cur, first, geom=None, see=0):
        """one host-driven tracked tick: (the world uploaded at `geom`,) rda_fleet_raycast(_peers), rda_fleet_upload_scans_tracked, rda_fleet_step_tracked"""
        st, cur = np.ascontiguousarray(st, float), np.ascontiguousarray(cur, np.int32)
        if geom is not None:
            self.upload_world(geom)
        rc, boxes = self.upload_tracked(st, self.cast(st, see))
        assert rc == 0, rc
        return (*self.step_tracked(st, cur, first), boxes)

    def scan_boxes(self, st, ranges):
        """rda_fleet_scan_boxes: the device's boxes of these ranges, a list of (n_i, 4, 2)"""
        nb, lo, hi, rmin, rmax = self.sensors
        n, boxes = np.zeros(self.B, np.int32), np.zeros((self.B, BEAMS, 4, 2))
        assert self.hip.fleet_scan_boxes(self.F, iptr(nb), dptr(ranges), dptr(lo), dptr(hi), dptr(rmax), dptr(st), EPS, MINS, iptr(n), dptr(boxes), BEAMS,
                                         None) == 0
        return [boxes[i, :n[i]].copy() for i in range(self.B)]

    def upload_polygons(self, st, boxes, vels):
        """rda_fleet_upload_scenes of the boxes as 4-vertex polygons with these velocities"""
        counts = np.array([len(b) for b in boxes], np.int32)
        total = int(counts.sum())
        geom = np.ascontiguousarray(np.concatenate(boxes).reshape(total, 4, 2)) if total else np.zeros((1, 4, 2))
        vel = np.ascontiguousarray(np.concatenate(vels).reshape(total, 2)) if total else np.zeros((1, 2))
        kind, nvert = np.zeros(max(total, 1), np.int32), np.full(max(total, 1), 4, np.int32)
        rob = np.ascontiguousarray(st[:, 0:2])
        assert E == 4
        assert self.hip.fleet_upload_scenes(self.F, iptr(counts), iptr(kind), iptr(nvert), dptr(geom), dptr(vel), dptr(rob), iptr(self.order)) == 0

    def track(self, boxes, gate=GATE, window=WINDOW, cap=CAP):
        """rda_fleet_track_boxes of the members' (n_i, 4, 2) arrays -> (rc, list of (n_i, 2) velocities)"""
        n = np.array([len(b) for b in boxes], np.int32)
        allb, vel = np.zeros((self.B, cap, 4, 2)), np.full((self.B, cap, 2), np.nan)
        for i, b in enumerate(boxes):
            allb[i, :min(len(b), cap)] = b[:cap]
        rc = self.hip.fleet_track_boxes(self.F, iptr(n), dptr(allb), cap, gate, window, dptr(vel))
        return rc, [vel[i, :n[i]].copy() for i in range(self.B)]

    def tracks(self, cap=CAP):
        """rda_fleet_box_tracks -> list of (centres, velocities, age)"""
        n, c, v, age = np.full(self.B, -7, np.int32), np.zeros((self.B, cap, 2)), np.zeros((self.B, cap, 2)), np.zeros((self.B, cap), np.int32)
        assert self.hip.fleet_box_tracks(self.F, cap, iptr(n), dptr(c), dptr(v), iptr(age)) == 0
        return [(c[i, :n[i]].copy(), v[i, :n[i]].copy(), age[i, :n[i]].copy()) for i in range(self.B)]


def table_of(tracks, vel):
    """the specification's tracks and velocities in the layout of TTwin.tracks"""
    m = len(tracks)
    return (np.array([h[-1] for h in tracks], float).reshape(m, 2), np.asarray(vel, float)[:m].reshape(m, 2), np.array([len(h) for h in tracks], np.int32))


def same_table(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def crafted(ticks):
    """per tick the boxes of three members: none | 5 boxes that translate rigidly in shuffled order, then an empty tick, a newborn box beside an old track,
    equidistant ties and a box at the gate | 257 boxes of which every third one moves"""
    rigid, _ = L.rigid_sequence(ticks - 6)
    tail = [np.zeros((0, 4, 2)), L.boxes_at([[0.0, 0.0]]), L.boxes_at([[0.75, 0.0], [0.25, 0.0]]), L.boxes_at([[1.25, 0.0], [-0.25, 0.0]]),
            L.boxes_at([[0.5, 0.0], [-0.25, 1.0]]), np.full((1, 4, 2), [1.5, 0.0])]
    grid = np.array([[4.0 * (i % 16), 4.0 * (i // 16)] for i in range(257)])
    drift = np.array([[0.125, 0.25] if i % 3 == 0 else [0.0, 0.0] for i in range(257)])
    return [[np.zeros((0, 4, 2)), (rigid + tail)[k], L.boxes_at(grid + k * drift)] for k in range(ticks)]


@pytest.mark.parametrize("window", [8, 3])
def test_the_tracker_alone_equals_the_specification(hip, window):
    a = TTwin(hip)
    assert all(len(t[0]) == 0 for t in a.tracks())                                  # before the first tracked call: no tracks
    seq = crafted(16)
    spec = [None] * 3
    moved = 0.0
    for k, boxes in enumerate(seq):
        rc, vel = a.track(boxes, window=window)
        assert rc == 0, rc
        got = a.tracks()
        for i in range(3):
            want, spec[i] = lidar.track_boxes(spec[i], boxes[i], DT, GATE, window)
            assert np.array_equal(vel[i], want), (k, i)
            assert same_table(got[i], table_of(spec[i], want)), (k, i)
            moved = max(moved, float(np.abs(want).max()) if len(want) else 0.0)
        assert len(got[2][0]) == 256 and np.array_equal(vel[2][256], [0.0, 0.0])
    assert moved > 1.0 and got[1][2].max() <= window and got[2][2].max() == min(window, 8)
    # one member reset: the others keep their tracks, its own boxes start anew
    which = np.array([2], np.int32)
    assert hip.fleet_reset_tracks(a.F, iptr(which), 1) == 0
    after = a.tracks()
    assert len(after[2][0]) == 0 and same_table(after[1], got[1]) and same_table(after[0], got[0])
    spec[2] = None
    rc, vel = a.track(seq[-1], window=window)
    assert rc == 0
    for i in range(3):
        want, spec[i] = lidar.track_boxes(spec[i], seq[-1][i], DT, GATE, window)
        assert np.array_equal(vel[i], want), i
    assert np.array_equal(vel[2], np.zeros((257, 2)))
    assert hip.fleet_reset_tracks(a.F, None, 0) == 0 and all(len(t[0]) == 0 for t in a.tracks())
    # refusals: nothing advances
    rc, _ = a.track(seq[0])
    assert rc == 0
    before = a.tracks()
    assert a.track(seq[1], gate=0.0)[0] == RDA_ERR_ARG and a.track(seq[1], window=0)[0] == RDA_ERR_ARG and a.track(seq[1], window=9)[0] == RDA_ERR_ARG
    assert a.track(seq[1], cap=100)[0] == RDA_ERR_ARG                               # 257 boxes in rows of 100
    bad = np.array([3], np.int32)
    assert hip.fleet_reset_tracks(a.F, iptr(bad), 1) == RDA_ERR_ARG
    assert all(same_table(x, y) for x, y in zip(a.tracks(), before))
    a.close()


def test_a_host_driven_tracked_tick_equals_the_polygons_with_the_specifications_velocities(hip):
    """twin A: rda_fleet_upload_scans_tracked + rda_fleet_step_tracked; twin B: the device's boxes of the same ranges (rda_fleet_scan_boxes) uploaded as
    polygons with lidar.track_boxes' velocities (rda_fleet_upload_scenes) + rda_fleet_step_tracked.  The world moves, the robots drive: u, s and rda_info
    for equality on every tick"""
    a, b = TTwin(hip), TTwin(hip)
    st, cur = a.states.copy(), a.cur0.copy()
    spec = [None] * 3
    fastest = 0.0
    for k in range(K):
        geom = advanced(a.kind, a.nvert, a.base, a.vel, DT * k)[0]
        a.upload_world(geom)
        ranges = a.cast(st)
        boxes = a.scan_boxes(st, ranges)
        rc, nbox = a.upload_tracked(st, ranges)
        assert rc == 0 and nbox.tolist() == [len(x) for x in boxes]
        ua, sa, ia, mia, eha = a.step_tracked(st, cur, k == 0)
        vels = []
        for i in range(3):
            v, spec[i] = lidar.track_boxes(spec[i], boxes[i], DT, GATE, WINDOW)
            vels.append(v)
            fastest = max(fastest, float(np.sqrt((v * v).sum(axis=1)).max()) if len(v) else 0.0)
        assert all(same_table(x, table_of(spec[i], vels[i])) for i, x in enumerate(a.tracks()))
        b.upload_polygons(st, boxes, vels)
        ub, sb, ib, mib, ehb = b.step_tracked(st, cur, k == 0)
        print(f"tick {k}: boxes {nbox.tolist()}  fastest box so far {fastest:.3f} m/s  |du| = {np.abs(ua - ub).max():.3e}  |ds| = {np.abs(sa - sb).max():.3e}")
        assert np.array_equal(ua, ub) and np.array_equal(sa, sb) and ia == ib, k
        assert np.array_equal(mia, mib) and np.array_equal(eha, ehb)
        st = np.ascontiguousarray([plant(st[i], ua[i, :, 0], i) for i in range(3)])
        cur = mia.copy()
    assert fastest > 0.01                                                            # some box was predicted over the horizon
    a.close(); b.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["blind", "seeing"])
def run(hip, request):
    """ONE tracked rollout of K ticks over the moving world and its teacher-forced twin"""
    see = request.param
    a, b = TTwin(hip), TTwin(hip)
    rc, logs = a.rollout_tracked(K, 1, see)
    assert rc == 0, rc
    last_u, last_eh, last_s = np.full((3, 2, T), np.nan), np.full(3, np.nan), np.full((3, 3, T + 1), np.nan)
    assert hip.fleet_rollout_last(a.F, dptr(last_u), dptr(last_eh)) == 0 and hip.fleet_rollout_last_plan(a.F, dptr(last_s)) == 0
    ticks = [b.host_tick_tracked(logs["states"][k], b.cur0 if k == 0 else logs["index"][k - 1], k == 0,
                                 geom=advanced(b.kind, b.nvert, b.base, b.vel, DT * k)[0], see=see) for k in range(K)]
    out = dict(see=see, logs=logs, ticks=ticks, last=(last_u, last_s, last_eh), tracks_a=a.tracks(), tracks_b=b.tracks())
    a.close(); b.close()
    return out


def test_a_tracked_rollout_tick_equals_the_host_driven_tracked_tick(run):
    logs, B = run["logs"], 3
    assert np.all(logs["arrived_at"] == -1)
    worst = 0.0
    for k, (u, s, info, mi, eh, boxes) in enumerate(run["ticks"]):
        for i in range(B):
            nxt = plant(logs["states"][k, i], logs["controls"][k, i], i)
            worst = max(worst, float(np.abs(logs["states"][k + 1, i] - nxt).max()))
            print(f"tick {k} member {i}: boxes {logs['boxes'][k, i]} / {boxes[i]}  |du| = {np.abs(logs['controls'][k, i] - u[i, :, 0]).max():.3e}  "
                  f"index {logs['index'][k, i]} / {mi[i]}  iters {logs['info'][k * B + i][2]} / {info[i][2]}")
    for k, (u, s, info, mi, eh, boxes) in enumerate(run["ticks"]):
        for i in range(B):
            assert logs["boxes"][k, i] == boxes[i], (k, i)
            assert np.array_equal(logs["controls"][k, i], u[i, :, 0]), (k, i)
            assert logs["index"][k, i] == mi[i], (k, i)
            assert logs["info"][k * B + i] == info[i], (k, i)
    u, s, info, mi, eh, boxes = run["ticks"][K - 1]
    last_u, last_s, last_eh = run["last"]
    assert np.array_equal(last_u, u) and np.array_equal(last_s, s) and np.array_equal(last_eh, eh)
    assert worst <= 1e-13                                                            # the plant: the bound of tests/test_gpu_fleet_rollout.py
    for ta, tb in zip(run["tracks_a"], run["tracks_b"]):
        assert same_table(ta, tb)
    assert sum(len(t[0]) for t in run["tracks_a"]) > 0 and max(int(t[2].max()) for t in run["tracks_a"] if len(t[2])) > 1
    if run["see"]:
        assert logs["peer_clearance"].shape == (K, 3) and np.all(np.isfinite(logs["peer_clearance"]))


def test_members_in_the_interior_point_mode_take_the_tracked_slots(hip):
    """an `lmz_central` fleet needs nothing of its own: its tracked rollout tick equals its host-driven tracked tick like the default fleet's"""
    a, b = TTwin(hip, lmz_central=1e-3), TTwin(hip, lmz_central=1e-3)
    rc, logs = a.rollout_tracked(3, 1, 0)
    assert rc == 0, rc
    for k in range(3):
        u, s, info, mi, eh, boxes = b.host_tick_tracked(logs["states"][k], b.cur0 if k == 0 else logs["index"][k - 1], k == 0,
                                                        geom=advanced(b.kind, b.nvert, b.base, b.vel, DT * k)[0])
        for i in range(3):
            assert logs["boxes"][k, i] == boxes[i] and logs["index"][k, i] == mi[i], (k, i)
            assert np.array_equal(logs["controls"][k, i], u[i, :, 0]) and logs["info"][k * 3 + i] == info[i], (k, i)
    assert all(same_table(x, y) for x, y in zip(a.tracks(), b.tracks())) and logs["boxes"].max() > 0
    a.close(); b.close()


def test_a_crossing_box_is_hit_without_track_and_avoided_with_it(hip):
    """The two mirrored lanes of lidar_track_lib.crossing as a fleet of two, 40 ticks on the device: a 2 x 2 m box crosses each robot's lane at 2 m/s.
    On the CPU (tests/test_lidar_track.py) the minimum clearance is -0.614 m with standing boxes and +1.133 m with tracked ones; here the signs are
    asserted on the clearance log of the two rollouts."""
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    made = [L.crossing(lane) for lane in (0, 1)]
    sensors, world = [m[3] for m in made], [[m[2]] for m in made]

    def fleet():
        return Fleet([MPC(m[0], [p.copy() for p in m[1]], receding=L.T, sample_time=L.DT, iter_num=L.ITER, max_edge_num=L.E, max_obs_num=L.N,
                          goal_index_threshold=L.MARGIN) for m in made])
    states = [m[1][0].copy() for m in made]
    kw = dict(lidar=sensors, world=world, moving=True, clearance=True, scan_eps=L.EPS, scan_min_samples=L.MINS)
    fb, ft = fleet(), fleet()
    blind = fb.rollout([s.copy() for s in states], L.SPEED, L.TICKS, **kw)
    tracked = ft.rollout([s.copy() for s in states], L.SPEED, L.TICKS, track=True, track_gate=1.0, track_window=8, **kw)
    print(f"minimum clearance per lane: without track {blind['clearance'].min(axis=0)}, with track {tracked['clearance'].min(axis=0)}")
    print("boxes seen:", tracked["boxes"].T.tolist())
    tr = ft.box_tracks()
    print("tracks after the run:", [(t["centres"].tolist(), t["velocities"].tolist(), t["age"].tolist()) for t in tr])
    assert blind["clearance"].min() < 0 and tracked["clearance"].min() > 0
    ft.reset([1])
    after = ft.box_tracks()
    assert len(after[1]["age"]) == 0 and np.array_equal(after[0]["centres"], tr[0]["centres"])
    with pytest.raises(ValueError):
        ft.rollout([s.copy() for s in states], L.SPEED, 2, track=True)
    with pytest.raises(ValueError):
        ft.control([s.copy() for s in states], L.SPEED, track=True)
    with pytest.raises(ValueError):
        ft.rollout([s.copy() for s in states], L.SPEED, 2, track=True, track_window=9, **kw)
    fb.close(); ft.close()


def test_fleet_control_with_scans_tracks_the_boxes(hip):
    """Fleet.control(scans=, track=True) on the crossing lanes, the robots started 6 m down their lanes so that the whole box is in sight: after every
    tick the fleet's table equals lidar.track_boxes on the device's own boxes of the same scans (Fleet.scan_boxes), and the box is seen moving at its
    2 m/s within 1.2 m/s: either end of the 3-tick difference is off by at most one beam spacing at 10 m, 2 pi 10 / 360 = 0.175 m, so the velocity
    by at most 2 * 0.175 / 0.3 = 1.17 m/s (the numpy front end gives 2.01 m/s there)"""
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    from lidar_world_lib import at_time
    made = [L.crossing(lane) for lane in (0, 1)]
    sensors = [m[3] for m in made]
    f = Fleet([MPC(m[0], [p.copy() for p in m[1]], receding=L.T, sample_time=L.DT, iter_num=L.ITER, max_edge_num=L.E, max_obs_num=L.N,
                   goal_index_threshold=L.MARGIN) for m in made])
    states = [m[1][60].copy() for m in made]
    spec = [None, None]
    for k in range(4):
        f.upload_worlds([at_time([m[2]], L.DT * k) for m in made])
        scans = f.raycast(states, sensors)
        boxes = f.scan_boxes(states, scans, L.EPS, L.MINS)
        res = f.control([s.copy() for s in states], L.SPEED, scans=scans, scan_eps=L.EPS, scan_min_samples=L.MINS, track=True)
        got = f.box_tracks()
        for i in range(2):
            vel, spec[i] = lidar.track_boxes(spec[i], boxes[i], L.DT, 1.0, 8)
            assert len(boxes[i]) == 1
            assert same_table((got[i]["centres"], got[i]["velocities"], got[i]["age"]), table_of(spec[i], vel)), (k, i)
        states = [sc.kinematic_step(states[i], res[i][0], made[i][0], L.DT) for i in range(2)]
    print("velocities after 4 ticks:", [g["velocities"].tolist() for g in got])
    assert all(g["age"].tolist() == [4] for g in got)
    assert abs(got[0]["velocities"][0, 1] - 2.0) < 1.2 and abs(got[1]["velocities"][0, 1] + 2.0) < 1.2
    f.close()


def test_the_untracked_rollout_is_unchanged_and_refusals(hip):
    a, b, c = TTwin(hip), TTwin(hip), TTwin(hip)
    rc, la = a.rollout(3, 1, min_samples=MINS)                                      # untracked, before
    assert rc == 0
    rc, lb = b.rollout_tracked(3, 1, 0)                                             # a tracked rollout on a twin
    assert rc == 0
    rc, lc = c.rollout(3, 1, min_samples=MINS)                                      # untracked, after
    assert rc == 0
    same_logs(la, lc, LOGS)
    assert not np.array_equal(la["controls"], lb["controls"])                        # tracking is another rollout
    # on the fleet that tracked: the untracked rollout that continues equals the one on a fleet made anew over the same members
    d = TTwin(hip)
    rc, ld = d.rollout_tracked(3, 1, 0)
    assert rc == 0
    same_logs(lb, ld, LOGS)
    cont = dict(min_samples=MINS, states=np.ascontiguousarray(lb["states"][3]), cur_index=np.ascontiguousarray(lb["index"][2]), nom_u=None)
    rc, lb2 = b.rollout(2, 0, **cont)
    assert rc == 0
    d.renew()
    d.upload_world(advanced(d.kind, d.nvert, d.base, d.vel, DT * 3)[0])              # (the tracked rollout moved the world by three ticks)
    rc, ld2 = d.rollout(2, 0, **cont)
    assert rc == 0
    same_logs(lb2, ld2, LOGS)
    # refusals: the rollout's own and the tracker's, and nothing has changed - neither the world nor the tracks
    w0, t0 = b.world(), b.tracks()
    assert b.rollout_tracked(0, 0, 0)[0] == RDA_ERR_ARG
    for key in ("states", "n_beams", "range_max", "order", "u_log"):
        assert b.rollout_tracked(2, 0, 0, **{key: None})[0] == RDA_ERR_ARG, key
    for kw in (dict(gate=0.0), dict(gate=-1.0), dict(window=0), dict(window=9)):
        assert b.rollout_tracked(2, 1, 0, **kw)[0] == RDA_ERR_ARG, kw
        assert b.upload_tracked(b.states, b.cast(b.states), **kw)[0] == RDA_ERR_ARG, kw
    nb = b.sensors[0].copy(); nb[0] = 4097
    assert b.rollout_tracked(2, 0, 0, n_beams=nb)[0] == RDA_ERR_UNSUPPORTED
    assert b.upload_tracked(b.states, b.cast(b.states), order=None)[0] == RDA_ERR_ARG
    assert np.array_equal(b.world(), w0) and all(same_table(x, y) for x, y in zip(b.tracks(), t0))
    for t in (a, b, c, d):
        t.close()
    f = TTwin(hip, world=False)                                                      # no uploaded world
    assert f.rollout_tracked(2, 0, 0)[0] == RDA_ERR_ARG
    f.close()


def test_refused_allocations_change_nothing(hip):
    """a fleet's first tracked rollout makes everything before tick 0, the tracker's table among it: refused at each allocation it returns RDA_ERR_HIP,
    holds nothing more than before, has no tracks and has not touched the world; the call that gets through gives the logs of an undisturbed twin"""
    def live():
        n, by = C.c_longlong(0), C.c_longlong(0)
        assert hip.debug_alloc_stats(C.byref(n), C.byref(by)) == 0
        return n.value, by.value
    a, b = TTwin(hip), TTwin(hip)
    w0 = a.world()
    rc, n = -3, 0
    while rc == -3 and n < 120:
        before = live()
        hip.debug_alloc_fail(n)
        try:
            rc, la = a.rollout_tracked(3, 1, 1)
        finally:
            hip.debug_alloc_fail(-1)
        assert rc == 0 or (rc == -3 and live() == before and np.array_equal(a.world(), w0)), (n, rc)
        if rc == -3:
            assert all(len(t[0]) == 0 for t in a.tracks())
        n += 1
    print("allocations of a fleet's first rda_fleet_rollout_lidar_tracked:", n - 1)
    assert rc == 0 and n - 1 > 30
    rc, lb = b.rollout_tracked(3, 1, 1)
    assert rc == 0
    same_logs(la, lb, keys=("states", "controls", "index", "arrived_at", "boxes", "clearance", "peer_clearance"))
    assert all(same_table(x, y) for x, y in zip(a.tracks(), b.tracks()))
    a.close(); b.close()


class Bare:
    """a fleet of two fresh handles (T = 5) that has made none of its tables yet, with TTwin's tracker calls"""
    track, tracks = TTwin.track, TTwin.tracks

    def __init__(self, hip):
        self.hip, self.B = hip, 2
        self.svs, self.F = bare_fleet(hip, [car(0), car(1)])


def test_refused_allocations_of_the_tracker_on_a_fresh_fleet_change_nothing(hip):
    """rda_fleet_track_boxes as a fleet's first lidar call makes the tracker's table and the lidar block: refused at each of the 20 allocations in turn
    it returns RDA_ERR_HIP, holds nothing more than before and has no tracks; the call that gets through, and a second tick behind it, give the
    velocities and the table of an undisturbed twin.  B = 2, two and three boxes."""
    a, b = Bare(hip), Bare(hip)
    ticks = [[L.boxes_at(np.array([[0.0, 0.0], [3.0, 0.0]]) + k * np.array([0.05, 0.0])),
              L.boxes_at(np.array([[1.0, 2.0], [4.0, 2.0], [7.0, 2.5]]) + k * np.array([0.0, -0.03]))] for k in range(2)]
    out = {}

    def first():
        rc, out["vel"] = a.track(ticks[0], cap=4)
        assert rc == 0 or all(len(t[0]) == 0 for t in a.tracks())
        return rc
    rc, refused = refused_in_turn(hip, first)
    print("allocations of rda_fleet_track_boxes on a fresh fleet:", refused)
    assert rc == 0 and refused == 20
    rc, want = b.track(ticks[0], cap=4)
    assert rc == 0 and all(np.array_equal(x, y) for x, y in zip(out["vel"], want))
    (rca, va), (rcb, vb) = a.track(ticks[1], cap=4), b.track(ticks[1], cap=4)
    assert rca == 0 and rcb == 0 and all(np.array_equal(x, y) for x, y in zip(va, vb)) and np.abs(vb[0]).max() > 0.4
    assert all(same_table(x, y) for x, y in zip(a.tracks(cap=4), b.tracks(cap=4)))
    hip.fleet_destroy(a.F); hip.fleet_destroy(b.F)
