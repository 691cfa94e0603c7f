"""-m gpu : the three fleet rollouts (rda_fleet_rollout, rda_fleet_rollout_moving, rda_fleet_rollout_lidar) for members in the interior-point LamMuZ
mode (`lmz_central=1e-3`).  The contracts are those of tests/test_gpu_fleet_rollout.py, test_gpu_fleet_rollout_moving.py and
test_gpu_fleet_rollout_lidar.py, whose lanes, twins and comparisons are used as they are (they hand their keyword arguments to the solvers): given a
state, a tick of a rollout computes bit for bit what its host-driven tick computes.  B = 2, K = 5 and every tick is compared."""
import numpy as np
import pytest

import test_gpu_fleet_rollout as static
import test_gpu_fleet_rollout_lidar as lidar
import test_gpu_fleet_rollout_moving as moving
from fleet_twin_lib import RDA_ERR_UNSUPPORTED, compare_ticks
from fleet_twin_lib import hip          # noqa: F401  (the fixture)
from lidar_world_lib import flatten, sensor_c
from rda_planner_amd import scenarios as sc

pytestmark = pytest.mark.gpu

MU, K = 1e-3, 5
ROWS = "k_lammuz_ip_fleet"


def _kernel(hip, twin):
    return hip.fleet_lammuz_kernel(twin.F).decode()


@pytest.mark.parametrize("resort", [1, 0], ids=["resort", "no-resort"])
def test_static_rollout_ticks_equal_resort_and_tracked_step(hip, resort):
    """rda_fleet_rollout on scenes that stand (members 0 and 2 of that file's lanes) against rda_fleet_scene_resort + rda_fleet_step_tracked fed the
    logged states: first control, min_index, the whole rda_info of every tick"""
    which = (0, 2)
    a, b = (static.Twin(hip, which, svs=[static.solver(hip, e, lmz_central=MU) for e in which]) for _ in range(2))
    assert _kernel(hip, a) == ROWS
    rc, logs = a.rollout(K, resort)
    assert rc == 0, rc
    ticks = b.forced(logs, K, resort)
    for k, (u, s, info, mi, eh) in enumerate(ticks):
        assert np.array_equal(logs["controls"][k], np.stack([u[:, 0, 0], u[:, 1, 0]], axis=1)), k
        assert np.array_equal(logs["index"][k], mi), k
        assert logs["info"][k * 2:k * 2 + 2] == info, k
    assert np.all(logs["arrived_at"] == -1) and np.all(logs["states"][K, :, 0] - logs["states"][0, :, 0] > 1.0)       # the members drive
    for x, y in zip(a.svs, b.svs):                              # the members are as K host-driven ticks leave them
        sa, sb = x.get_state(), y.get_state()
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), key
    a.close(); b.close()


def test_static_rollout_still_refuses_a_scene_that_moves(hip):
    which = (0, 2)
    a = static.Twin(hip, which, svs=[static.solver(hip, 0, lmz_central=MU), static.solver(hip, 2, moving=True, lmz_central=MU)])
    rc, _ = a.rollout(K, 1)
    assert rc == RDA_ERR_UNSUPPORTED
    a.close()


@pytest.mark.parametrize("resort", [1, 0], ids=["resort", "staged-order"])
def test_moving_rollout_ticks_equal_upload_and_tracked_step(hip, resort):
    """rda_fleet_rollout_moving with the clearance log, one member whose scene moves (member 0 of that file) and one whose scene stands (member 2),
    against its own host tick: that tick's geometry (advanced in numpy) uploaded, then rda_fleet_step_tracked"""
    which = (0, 2)
    a, b = (moving.Twin(hip, which, order=resort, svs=[moving.solver(hip, e, resort, lmz_central=MU) for e in which]) for _ in range(2))
    assert _kernel(hip, a) == ROWS
    rc, logs = a.rollout(K, resort)
    assert rc == 0, rc
    ticks = b.forced(logs, K, b.base, b.cur0, True)
    assert compare_ticks(logs, ticks, K, ("controls", "index", "iters", "info")) == 2 * K       # ... and the whole rda_info
    for sa, sb in zip(a.slots(), b.slots()):
        assert sa[3] == sb[3]
        for x, y in zip(sa[:3], sb[:3]):
            assert np.array_equal(x, y)
    worst = 0.0
    for k in range(K):                                          # the clearance log is against the obstacles where they are after tick k
        for i, e in enumerate(which):
            worst = max(worst, abs(logs["clearance"][k, i] - moving.reference_clearance(e, logs["states"][k + 1, i], (k + 1) * moving.DT)))
    assert worst <= 1e-9, worst                                 # (the bound of that file's clearance test)
    a.close(); b.close()


class SmallLidarTwin(lidar.Twin):
    """that file's twin with a small sensor (32 beams ahead) and a world of 3 boxes per member beside its lane"""
    def __init__(self, hip, which):
        super().__init__(hip, which, world=False, lmz_central=MU)
        flat = []
        for e in which:
            y = 20.0 + 8.0 * e
            flat.append(flatten([sc.box(7.5, y + 2.2, 2.4, 1.2, 0.0), sc.box(10.0, y - 2.2, 2.4, 1.2, 0.0, velocity=(-0.4, 0.0) if e == 0 else (0.0, 0.0)),
                                 sc.box(12.5, y + 2.2, 2.4, 1.2, 0.0)]))
        self.kind, self.nvert, self.base, self.vel = (np.ascontiguousarray(np.concatenate([f[j] for f in flat])) for j in range(4))
        self.counts = np.full(self.B, 3, np.int32)
        self.sensors = sensor_c([dict(number=32, angle_min=-0.7, angle_max=0.7, range_min=0.0, range_max=10.0)] * self.B)
        self.upload_world(self.base)


def test_lidar_rollout_ticks_equal_raycast_upload_and_tracked_step(hip, monkeypatch):
    """rda_fleet_rollout_lidar (the world moving) against rda_fleet_raycast + rda_fleet_upload_scans + rda_fleet_step_tracked on the numpy-advanced world:
    box counts, first control, min_index and the whole rda_info of every tick; the per-tick box counts choose every member's LamMuZ form"""
    which = (0, 2)
    a, b = SmallLidarTwin(hip, which), SmallLidarTwin(hip, which)
    rc, logs = a.rollout(K, 1, eps=1.0, min_samples=4)
    assert rc == 0, rc
    monkeypatch.setattr(lidar, "EPS", 1.0)                      # (the twin's host tick reads that module's constants)
    monkeypatch.setattr(lidar, "MIN_SAMPLES", 4)
    ticks = b.forced(logs, K, b.base, lambda k: lidar.DT * k, b.cur0, True)
    assert compare_ticks(logs, ticks, K, lidar.TICK) == 2 * K
    print("boxes per tick:", logs["boxes"].T.tolist())
    assert (logs["boxes"] > 0).any()                            # the sensor saw something: the row-parallel kernel ran
    last, names = logs["boxes"][K - 1], _kernel(hip, a).split("+")      # the members as the last tick staged them: each box count chose its member's form
    assert (ROWS in names) == bool((last > 0).any()) and ("k_lammuz_cp_fleet_small" in names) == bool((last == 0).any())
    a.close(); b.close()
