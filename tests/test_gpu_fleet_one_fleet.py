"""-m gpu : several fleet entry points in sequence on ONE fleet against the same sequence on fleets that are made anew before every step, so that every
on-first-use table set of a fleet (tracked stepping, re-sort, lidar, rollout tables and log, move / clearance tables, snapshot, clearance log, world, ray
ranges) is reused, regrown and re-compared on one side and built from nothing on the other.  Everything either side returns must be equal bit for bit.

Shapes and helpers are those of tests/test_gpu_fleet_rollout_moving.py and tests/test_gpu_fleet_rollout_lidar.py: T = 8, N = 4, E = 4, iter_num = 2, B = 3
(Ackermann, differential, omni) on their lanes, 7 obstacles per member as raw scene and as world, the three sensors of lidar_world_lib.  The sequence:
  1  rda_fleet_rollout_moving, K = 3, resort = 1, with clearance log
  2  rda_fleet_clearance at the last logged states
  3  rda_fleet_upload_worlds at the base geometry, rda_fleet_rollout_lidar, K = 3, moving = 1, with clearance and box logs, from step 1's last states
  4  rda_fleet_upload_scenes of the raw scenes at advanced(base, DT * 3) (the lidar ticks overwrote them), rda_fleet_sync
  5  rda_fleet_rollout_moving, K = 5, without clearance log (the log block is regrown)
  6  rda_fleet_rollout_moving, K = 2, with clearance log (the longer blocks are reused)
  7  rda_fleet_scene_resort and one rda_fleet_step_tracked"""
import numpy as np
import pytest

from fleet_twin_lib import DT, N, T, advanced, solver
from lidar_world_lib import SENSORS, sensor_c
from rda_planner_amd._capi import dptr, iptr
from test_gpu_fleet_rollout_lidar import Twin as LidarTwin
from test_gpu_fleet_rollout_moving import Twin

pytestmark = pytest.mark.gpu


def sequence(hip, fresh):
    """the seven steps on one set of member handles -> [(name, value)] of everything they return; fresh: a new fleet over the same handles (and its world
    uploaded again) before every step"""
    made = [solver(hip, e, 1) for e in range(3)]
    box, got = {}, []

    def fleet():
        if "tw" in box:
            if not fresh:
                return box["tw"]
            box["tw"].close()
        # the moving file's Twin, also driven through the lidar file's Twin.upload_world and Twin.rollout: of `self` they read hip, F, B, counts, kind, nvert,
        # vel, states, speed, cur0, nom0, order - which this Twin has - and sensors, which is given to it here
        tw = box["tw"] = Twin(hip, svs=made)
        tw.sensors = sensor_c(SENSORS)
        if fresh:
            LidarTwin.upload_world(tw, tw.base)
        return tw

    def keep(step, logs, tw):
        for key, val in logs.items():
            if val is not None:
                got.append((f"{step}:{key}", val))
        u, eh = np.full((tw.B, 2, T), np.nan), np.full(tw.B, np.nan)
        assert hip.fleet_rollout_last(tw.F, dptr(u), dptr(eh)) == 0
        got.extend([(f"{step}:last_u", u), (f"{step}:end_heading", eh)])

    def cont(logs, k):
        return dict(states=np.ascontiguousarray(logs["states"][k]), cur_index=np.ascontiguousarray(logs["index"][k - 1]), nom_u=None)

    tw = fleet()
    rc, l1 = tw.rollout(3, 1)                                                    # 1
    assert rc == 0, rc
    keep(1, l1, tw)
    tw = fleet()
    cl = np.full(tw.B, np.nan)                                                   # 2
    assert hip.fleet_clearance(tw.F, dptr(np.ascontiguousarray(l1["states"][3])), dptr(cl)) == 0
    got.append(("2:clearance", cl))
    tw = fleet()
    LidarTwin.upload_world(tw, tw.base)                                          # 3
    rc, l3 = LidarTwin.rollout(tw, 3, 1, **cont(l1, 3))
    assert rc == 0, rc
    keep(3, l3, tw)
    tw = fleet()
    geom = advanced(tw.kind, tw.nvert, tw.base, tw.vel, DT * 3)[0]               # 4
    rob = np.ascontiguousarray(l3["states"][3][:, 0:2])
    assert hip.fleet_upload_scenes(tw.F, iptr(tw.counts), iptr(tw.kind), iptr(tw.nvert), dptr(np.ascontiguousarray(geom)), dptr(tw.vel), dptr(rob),
                                   iptr(tw.order)) == 0
    assert hip.fleet_sync(tw.F) == 0
    tw = fleet()
    rc, l5 = tw.rollout(5, 1, clearance=False, **cont(l3, 3))                    # 5
    assert rc == 0, rc
    keep(5, l5, tw)
    tw = fleet()
    rc, l6 = tw.rollout(2, 1, **cont(l5, 5))                                     # 6
    assert rc == 0, rc
    keep(6, l6, tw)
    tw = fleet()
    tick = tw.host_tick(l6["states"][2], l6["index"][1], False, resort=True)     # 7
    got.extend((f"7:{name}", val) for name, val in zip(("u", "s", "info", "min_index", "end_heading"), tick))
    tw.close()
    return got


@pytest.fixture(scope="module")
def sides(hip):
    return sequence(hip, False), sequence(hip, True)


def test_one_fleet_equals_fresh_fleets_bit_for_bit(sides):
    """states, controls, indices, rda_info, arrival, box counts, clearances and rda_fleet_rollout_last of every step"""
    a, b = sides
    assert [name for name, _ in a] == [name for name, _ in b] and len(a) > 30
    for (name, x), (_, y) in zip(a, b):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, name


def test_the_sequence_is_not_trivial(sides):
    """the members are driven, and member 1 sees more boxes than there are slots"""
    got = dict(sides[0])
    for step in (1, 3, 5, 6):
        assert np.abs(got[f"{step}:controls"][:, :, 0]).max() > 1.0, step
    assert np.abs(got["7:u"]).max() > 0.1
    assert (got["3:boxes"][:, 1] > N).any()
    assert np.all(np.isfinite(got["2:clearance"])) and np.all(np.isfinite(got["6:clearance"])) and np.all(np.isfinite(got["3:clearance"]))
