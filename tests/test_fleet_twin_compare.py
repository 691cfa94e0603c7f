"""The comparison the GPU tests of the fleet rollouts share (fleet_twin_lib.compare_ticks), on hand-made logs and ticks, B = 2 and K = 2, without a device:
equal logs pass; a live control, a path index, an iteration count, another field of rda_info and a box count, corrupted one at a time, each fail the
comparison that asks for that quantity - and only that one."""
import copy

import numpy as np
import pytest

from fleet_twin_lib import T, compare_ticks

B, K = 2, 2
ALL = ("controls", "stands", "index", "iters", "info", "boxes")


def made():
    """logs of a rollout in which member 1 arrives on tick 1, and the host-driven ticks that equal them"""
    rng = np.random.default_rng(7)
    infos = [(0.1 * j, 0.2 * j, 2 + j % 2, 0, 5 + j, 0) for j in range(K * B)]
    logs = dict(states=rng.normal(size=(K + 1, B, 3)), controls=rng.normal(size=(K, B, 2)), index=np.arange(K * B, dtype=np.int32).reshape(K, B),
                info=list(infos), arrived_at=np.array([-1, 1], np.int32), boxes=np.array([[3, 0], [5, 1]], np.int32))
    logs["controls"][1, 1] = 0.0                                    # it stands from its arrival on
    ticks = []
    for k in range(K):
        u = rng.normal(size=(B, 2, T))
        u[:, :, 0] = logs["controls"][k]
        if k == 1:
            u[1, :, 0] = (0.7, -0.2)                                # the solve of a member that has arrived goes on; its control is not applied
        ticks.append((u, rng.normal(size=(B, 3, T + 1)), infos[k * B:(k + 1) * B], logs["index"][k].copy(), np.zeros(B), logs["boxes"][k].copy()))
    return logs, ticks


def test_shared_comparator_finds_each_corruption_it_is_asked_for():
    logs, ticks = made()
    assert compare_ticks(logs, ticks, K, ALL) == 3                  # member 1 is live on tick 0 only
    assert compare_ticks(logs, ticks) == 3 and compare_ticks(logs, [t[:5] for t in ticks], K) == 3      # ticks without box counts, as most twins return
    with pytest.raises(AssertionError):
        compare_ticks(logs, ticks, K + 1)                           # the number of ticks
    with pytest.raises(AssertionError):
        compare_ticks(logs, ticks, K, ("controls", "indices"))      # an unknown quantity is not silently skipped

    def corrupted(what):
        bad = copy.deepcopy(logs)
        if what == "controls":
            bad["controls"][1, 0, 1] += 1e-16 + abs(bad["controls"][1, 0, 1]) * 1e-15         # a live control, in its last bits
        elif what == "stands":
            bad["controls"][1, 1, 0] = 1e-300                                               # the member that has arrived moves
        elif what == "index":
            bad["index"][1, 1] += 1
        elif what == "boxes":
            bad["boxes"][0, 1] += 1
        else:
            j, field = (2, 2) if what == "iters" else (1, 4)                                # iters | su_ipm_iters of one tick and member
            info = list(bad["info"][j])
            info[field] += 1
            bad["info"][j] = tuple(info)
        return bad
    for what in ALL:
        bad = corrupted(what)
        assert not np.array_equal(bad["controls"], logs["controls"]) or bad["info"] != logs["info"] or any(
            not np.array_equal(bad[k], logs[k]) for k in ("index", "boxes")), what
        with pytest.raises(AssertionError):
            compare_ticks(bad, ticks, K, (what,))
        with pytest.raises(AssertionError):
            compare_ticks(bad, ticks, K, ALL)
        blind = tuple(w for w in ALL if w != what and not (what == "iters" and w == "info"))    # (the whole rda_info holds the iteration count)
        assert compare_ticks(bad, ticks, K, blind) == 3, what
    # a member that has arrived: its index, info and boxes count unless the caller leaves such members out
    bad = corrupted("index")
    assert compare_ticks(bad, ticks, K, ("index",), arrived_too=False) == 3
    late = copy.deepcopy(logs)
    late["arrived_at"][1] = -1                                      # had it not arrived, its control of tick 1 would be compared
    with pytest.raises(AssertionError):
        compare_ticks(late, ticks, K, ("controls",))
