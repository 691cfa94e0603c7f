"""-m gpu : the lidar rollout of a fleet whose members see each other (rda_fleet_rollout_lidar_peers: lidar::k_raycast_fleet_peers in the ray caster's place,
rollout::k_peer_clearance_fleet behind the tick; Fleet.rollout(lidar=, see_peers=True)) against the host-driven loop it replaces.

6  a rollout tick equals the host-driven tick: twin A runs the rollout, twin B is fed A's logged states tick by tick and runs rda_fleet_raycast_peers ->
   rda_fleet_upload_scans -> rda_fleet_step_tracked on the world of that tick.  For equality, every tick: the first control, the path index, the whole
   rda_info (iters among it) and the box count; the last tick, of which the rollout keeps everything (rda_fleet_rollout_last / _last_plan): the full
   controls, the planned states and the end heading.  With the world moving and standing.
   The logged states are A's plant, rollout::k_rollout_advance, which this entry shares with every rollout: state k+1 against the numpy plant on state k
   and control k at 1e-13, the bound and the reasoning of tests/test_gpu_fleet_rollout.py (the device's sin / cos / tan are within a few ulp of
   libm's, dt |v| <= 1, every other operation is the same separately rounded double operation).  It is not an equality: measured here, 23 of the 24
   state vectors are equal and one heading of the Ackermann member differs by 3.5e-18 rad, one ulp of tan.
7  peer_clearance_log against scenarios.peer_clearance of the logged states, 1e-9 m (the project's bound for device geometry against its numpy
   specification, tests/test_gpu_fleet_peers.py); +inf for a fleet of one.
8  blind against seeing on crossing paths (see that test's docstring for the scene and its CPU numbers).
9  the blind rollout is what it was: the same logs before and after a seeing rollout on a twin, and on a fleet that ran a seeing rollout whether it reuses
   what that call left in the fleet or builds everything anew.

Shapes (tests/test_gpu_fleet_rollout_lidar.py): T = 8, N = 4, E = 4, iter_num = 2, dt = 0.1; B = 3 (Ackermann, differential, omni) on lanes 8 m apart, 7
obstacles per member as the world; the three sensors of that file with 65 beams each (a partial second workgroup); eps 2.0; min_samples 4, because 65 beams put only 5 .. 9 hits on a
member one lane away (at that file's 6 the blind and the seeing members count the same boxes); K = 4."""
import ctypes as C

import numpy as np
import pytest

from fleet_twin_lib import DT, DYN, E, ITER, MARGIN, N, RDA_ERR_ARG, RDA_ERR_UNSUPPORTED, SPEED, T, advanced, car, compare_ticks, info_tuple, lane, same_logs
from lidar_world_lib import EPS, SENSORS, numpy_scan, sensor_c
from rda_planner_amd import scenarios as sc
from rda_planner_amd._capi import dptr, iptr
from test_gpu_fleet_rollout_lidar import LOGS, TICK, Twin

pytestmark = pytest.mark.gpu

K, BEAMS, MINS = 4, 65, 4


class PTwin(Twin):
    """that file's Twin with 65-beam sensors, the seeing rollout and the seeing host tick"""
    def __init__(self, hip, which=(0, 1, 2), **kw):
        super().__init__(hip, which, **kw)
        self.sensors = sensor_c([dict(SENSORS[e], number=BEAMS) for e in which])

    def rollout_peers(self, k, moving, clearance=True, peer=True, **over):
        """rda_fleet_rollout_lidar_peers -> (rc, dict of logs); over: arguments replaced (None = a missing array)"""
        out = self.logs(k, boxes=np.int32, clearance=float if clearance else None, peer_clearance=float if peer else None)
        nb, lo, hi, rmin, rmax = self.sensors
        a = dict(states=self.states, ref_speed=self.speed, cur_index=self.cur0, threshold=0.1, ind_range=10, goal_margin=MARGIN, nom_u=self.nom0,
                 n_beams=nb, angle_min=lo, angle_max=hi, range_min=rmin, range_max=rmax, eps=EPS, min_samples=MINS, order=self.order,
                 states_log=out["states"], u_log=out["controls"], index_log=out["index"], info_log=out["info"], arrived_at=out["arrived_at"],
                 nbox_log=out["boxes"])
        a.update(over)
        rc = self.hip.fleet_rollout_lidar_peers(self.F, k, dptr(a["states"]), dptr(a["ref_speed"]), iptr(a["cur_index"]), a["threshold"], a["ind_range"],
                                                a["goal_margin"], dptr(a["nom_u"]), iptr(a["n_beams"]), dptr(a["angle_min"]), dptr(a["angle_max"]),
                                                dptr(a["range_min"]), dptr(a["range_max"]), a["eps"], a["min_samples"], iptr(a["order"]), moving,
                                                dptr(a["states_log"]), dptr(a["u_log"]), iptr(a["index_log"]), a["info_log"], iptr(a["arrived_at"]),
                                                iptr(a["nbox_log"]), dptr(out["clearance"]), dptr(out["peer_clearance"]))
        out["info"] = [info_tuple(i) for i in out["info"]]
        return rc, out

    def host_tick(self, st, cur, first, geom=None):
        """one host-driven tick: (the world uploaded at `geom`,) rda_fleet_raycast_peers, rda_fleet_upload_scans of those ranges at those states,
        rda_fleet_step_tracked -> controls, states, infos, min_index, end_heading, box counts"""
        B, hip = self.B, self.hip
        st, cur = np.ascontiguousarray(st, float), np.ascontiguousarray(cur, np.int32)
        if geom is not None:
            self.upload_world(geom)
        nb, lo, hi, rmin, rmax = self.sensors
        ranges, boxes = np.zeros(int(nb.sum()) + 1), np.full(B, -7, np.int32)
        assert hip.fleet_raycast_peers(self.F, iptr(nb), dptr(lo), dptr(hi), dptr(rmin), dptr(rmax), dptr(st), dptr(ranges)) == 0
        assert hip.fleet_upload_scans(self.F, iptr(nb), dptr(ranges), dptr(lo), dptr(hi), dptr(rmax), dptr(st), EPS, MINS, iptr(self.order),
                                      iptr(boxes)) == 0
        return (*self.step_tracked(st, cur, first), boxes)

    def renew(self):
        """a new fleet over the same member handles, its world uploaded again: none of the old fleet's tables is left"""
        self.close()
        self.make_fleet(self.hip, self.svs)
        self.upload_world(self.base)


def plant(state, u, i):
    """the kinematic step in the expressions of tests/test_gpu_fleet_rollout.py"""
    (x, y, th), (v, w) = state, u
    if DYN[i] == "acker":
        return np.array([x + DT * (v * np.cos(th)), y + DT * (v * np.sin(th)), th + DT * (v * np.tan(w) / car(i).wheelbase)])
    if DYN[i] == "diff":
        return np.array([x + DT * (v * np.cos(th)), y + DT * (v * np.sin(th)), th + DT * w])
    return np.array([x + DT * (v * np.cos(w)), y + DT * (v * np.sin(w)), th])


@pytest.fixture(scope="module", params=[1, 0], ids=["moving", "standing"])
def run(hip, request):
    """ONE seeing rollout of K ticks and its teacher-forced twin, shared by the tests below"""
    moving = request.param
    a, b = PTwin(hip), PTwin(hip)
    rc, logs = a.rollout_peers(K, moving)
    assert rc == 0, rc
    last_u, last_eh, last_s = np.full((3, 2, T), np.nan), np.full(3, np.nan), np.full((3, 3, T + 1), np.nan)
    assert hip.fleet_rollout_last(a.F, dptr(last_u), dptr(last_eh)) == 0 and hip.fleet_rollout_last_plan(a.F, dptr(last_s)) == 0
    ticks = [b.host_tick(logs["states"][k], b.cur0 if k == 0 else logs["index"][k - 1], k == 0,
                         geom=advanced(b.kind, b.nvert, b.base, b.vel, DT * k if moving else 0.0)[0]) for k in range(K)]
    a.close(); b.close()
    return dict(moving=moving, logs=logs, ticks=ticks, last=(last_u, last_s, last_eh))


def test_a_rollout_tick_equals_the_host_driven_tick(run):
    logs, B = run["logs"], 3
    assert np.all(logs["arrived_at"] == -1)
    worst = 0.0
    for k, (u, s, info, mi, eh, boxes) in enumerate(run["ticks"]):
        for i in range(B):
            first = np.array([u[i, 0, 0], u[i, 1, 0]])
            nxt = plant(logs["states"][k, i], logs["controls"][k, i], i)
            worst = max(worst, float(np.abs(logs["states"][k + 1, i] - nxt).max()))
            print(f"tick {k} member {i}: boxes {logs['boxes'][k, i]} / {boxes[i]}  |du| = {np.abs(logs['controls'][k, i] - first).max():.3e}  "
                  f"index {logs['index'][k, i]} / {mi[i]}  iters {logs['info'][k * B + i][2]} / {info[i][2]}  "
                  f"|state - plant| = {np.abs(logs['states'][k + 1, i] - nxt).max():.3e}")
    print(f"largest |state - numpy plant| = {worst:.3e}")
    assert compare_ticks(logs, run["ticks"], K, TICK) == K * B                                    # (nobody has arrived: every control is compared)
    u, s, info, mi, eh, boxes = run["ticks"][K - 1]
    last_u, last_s, last_eh = run["last"]
    assert np.array_equal(last_u, u) and np.array_equal(last_s, s) and np.array_equal(last_eh, eh)
    assert worst <= 1e-13 and np.abs(DT * logs["controls"][:, :, 0]).max() <= 1.0
    assert np.abs(logs["controls"][:, :, 0]).max() > 1.0                                         # the members drive


def test_the_members_are_seen(run):
    """tick 0 on the CPU: the numpy scan with the peer footprints gives members 0 and 1 other boxes than the blind scan, and the rollout logged the
    seeing count"""
    from rda_planner_amd import lidar
    logs = run["logs"]
    cars, st = [car(i) for i in range(3)], logs["states"][0]
    differ = 0
    for i in range(3):
        sensor = dict(SENSORS[i], number=BEAMS)
        seeing = lidar.scan_box(st[i].reshape(3, 1), numpy_scan(st[i], sensor, lane(i)[1] + sc.peer_footprints(cars, st, i)), EPS, MINS)
        blind = lidar.scan_box(st[i].reshape(3, 1), numpy_scan(st[i], sensor, lane(i)[1]), EPS, MINS)
        print(f"member {i}: boxes blind {len(blind)}, seeing {len(seeing)}, logged {logs['boxes'][0, i]}")
        assert logs["boxes"][0, i] == len(seeing), i
        differ += len(seeing) != len(blind)
    assert differ >= 1


def test_peer_clearance_log(hip, run):
    logs = run["logs"]
    cars = [car(i) for i in range(3)]
    worst = 0.0
    assert logs["peer_clearance"].shape == (K, 3)
    for k in range(K):
        worst = max(worst, float(np.abs(logs["peer_clearance"][k] - sc.peer_clearance(cars, logs["states"][k + 1])).max()))
    print(f"largest |peer_clearance_log - scenarios.peer_clearance| = {worst:.3e}  (values {logs['peer_clearance'].min():.3f} .. {logs['peer_clearance'].max():.3f})")
    assert worst <= 1e-9
    if run["moving"]:
        return
    one = PTwin(hip, (1,))
    rc, l1 = one.rollout_peers(2, 0)
    assert rc == 0 and np.all(np.isposinf(l1["peer_clearance"][:2])) and np.all(np.isfinite(l1["clearance"][:2]))
    one.close()
    two = PTwin(hip, (1,))                                                       # B = 1 sees what the blind rollout sees
    rc, l3 = two.rollout(2, 0, min_samples=MINS)
    assert rc == 0
    same_logs(dict(l1, peer_clearance=None), l3, LOGS)
    two.close()


def crossing():
    """two differential robots head-on on lanes 0.6 m apart, 14 m between them, an empty world, a full-turn lidar of 120 beams that sees 10 m"""
    paths = [sc.line_path([12, 20, 0], [34, 20, 0], 0.1), sc.line_path([26, 20.6, np.pi], [4, 20.6, np.pi], 0.1)]
    cars = [sc.rectangle_robot(dynamics="diff", wheelbase=0) for _ in range(2)]
    sensor = dict(number=120, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=10.0)
    return paths, cars, sensor


def test_blind_members_collide_and_seeing_members_do_not(hip):
    """Two robots drive at each other at 4 m/s on lanes 0.6 m apart (1.6 m wide: they cannot pass without giving way), 26 ticks.
    On the CPU - the host loop of numpy scan with scenarios.peer_footprints, lidar.scan_box, the oracle-backed MPC (T = 8, N = 4, E = 4, iter_num = 2)
    and scenarios.kinematic_step - the minimum member-to-member separation over the run is -1.000 m blind (ticks 13 .. 21: they drive through each
    other) and +0.474 m seeing (tick 17: they give way), so both margins of 0.1 m hold there.  Here both rollouts run on the device and the
    two signs are asserted."""
    from rda_planner_amd.fleet import Fleet
    from rda_planner_amd.mpc import MPC
    steps = 26
    paths, cars, sensor = crossing()

    def fleet():
        return Fleet([MPC(cars[i], [p.copy() for p in paths[i]], receding=T, sample_time=DT, iter_num=ITER, max_edge_num=E, max_obs_num=N,
                          goal_index_threshold=MARGIN) for i in range(2)])
    states = [paths[i][0].copy() for i in range(2)]
    fb, fs = fleet(), fleet()
    blind = fb.rollout([s.copy() for s in states], SPEED, steps, lidar=[sensor] * 2, world=[[], []])
    seeing = fs.rollout([s.copy() for s in states], SPEED, steps, lidar=[sensor] * 2, world=[[], []], see_peers=True)
    assert "peer_clearance" not in blind and seeing["peer_clearance"].shape == (steps, 2)
    sep_blind = np.array([sc.peer_clearance(cars, blind["states"][k + 1]).min() for k in range(steps)])
    sep_seeing = seeing["peer_clearance"].min(axis=1)
    print(f"minimum separation: blind {sep_blind.min():.3f} m at tick {sep_blind.argmin()}, seeing {sep_seeing.min():.3f} m at tick {sep_seeing.argmin()}")
    print("boxes seen:", seeing["boxes"].T.tolist())
    assert np.all(blind["boxes"] == 0) and (seeing["boxes"] > 0).any()
    assert sep_blind.min() < 0 and sep_seeing.min() > 0
    fb.close(); fs.close()


def test_the_blind_rollout_is_unchanged(hip):
    a, b, c = PTwin(hip), PTwin(hip), PTwin(hip)
    rc, la = a.rollout(3, 0, min_samples=MINS)                                                 # blind, before
    assert rc == 0
    rc, lb = b.rollout_peers(3, 0)                                               # a seeing rollout on a twin
    assert rc == 0
    rc, lc = c.rollout(3, 0, min_samples=MINS)                                                 # blind, after
    assert rc == 0
    same_logs(la, lc, LOGS)
    assert not np.array_equal(la["boxes"], lb["boxes"]) or not np.array_equal(la["controls"], lb["controls"])       # seeing is another rollout
    # on the fleet that saw: the blind rollout that continues, reusing what the seeing call left | on a fleet made anew over the same members
    d = PTwin(hip)
    rc, ld = d.rollout_peers(3, 0)
    assert rc == 0
    same_logs(lb, ld, keys=("states", "controls", "index", "arrived_at", "boxes", "clearance", "peer_clearance"))
    cont = dict(min_samples=MINS, states=np.ascontiguousarray(lb["states"][3]), cur_index=np.ascontiguousarray(lb["index"][2]), nom_u=None)
    rc, lb2 = b.rollout(2, 0, **cont)
    assert rc == 0
    d.renew()
    rc, ld2 = d.rollout(2, 0, **cont)
    assert rc == 0
    same_logs(lb2, ld2, LOGS)
    for t in (a, b, c, d):
        t.close()


def test_refusals(hip):
    a = PTwin(hip)
    w0 = a.world()
    assert a.rollout_peers(0, 0)[0] == RDA_ERR_ARG
    for key in ("states", "n_beams", "range_max", "order", "u_log"):
        assert a.rollout_peers(2, 0, **{key: None})[0] == RDA_ERR_ARG, key
    nb = a.sensors[0].copy(); nb[0] = 4097
    assert a.rollout_peers(2, 0, n_beams=nb)[0] == RDA_ERR_UNSUPPORTED
    assert np.array_equal(a.world(), w0)
    rc, la = a.rollout_peers(2, 1, clearance=False, peer=False, nbox_log=None, info_log=None)          # every optional log left out
    assert rc == 0 and not np.array_equal(a.world(), w0)
    b = PTwin(hip)
    rc, lb = b.rollout_peers(2, 1)
    assert rc == 0
    same_logs(dict(la, info=lb["info"]), lb, keys=("states", "controls", "index", "arrived_at"))
    a.close(); b.close()
    f = PTwin(hip, world=False)                                                  # no uploaded world
    assert f.rollout_peers(2, 0)[0] == RDA_ERR_ARG
    f.close()


def test_refused_allocations_change_nothing(hip):
    """the first seeing rollout of a fleet makes everything before tick 0, the peer table and the separation log among it: refused at each allocation it
    returns RDA_ERR_HIP, holds nothing more than before and has not touched the world; the call that gets through gives the logs of an undisturbed twin"""
    def live():
        n, by = C.c_longlong(0), C.c_longlong(0)
        assert hip.debug_alloc_stats(C.byref(n), C.byref(by)) == 0
        return n.value, by.value
    a, b = PTwin(hip), PTwin(hip)
    w0 = a.world()
    rc, n = -3, 0
    while rc == -3 and n < 90:
        before = live()
        hip.debug_alloc_fail(n)
        try:
            rc, la = a.rollout_peers(3, 1)
        finally:
            hip.debug_alloc_fail(-1)
        assert rc == 0 or (rc == -3 and live() == before and np.array_equal(a.world(), w0)), (n, rc)
        n += 1
    print("allocations of a fleet's first rda_fleet_rollout_lidar_peers:", n - 1)
    assert rc == 0 and n - 1 > 30
    rc, lb = b.rollout_peers(3, 1)
    assert rc == 0
    same_logs(la, lb, keys=("states", "controls", "index", "arrived_at", "boxes", "clearance", "peer_clearance"))
    a.close(); b.close()
