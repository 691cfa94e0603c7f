"""What `RDA_solver` and `MPC` ask of the library binding, call by call, without a device: for the five step forms, every upload / scan method
and the routes of `MPC.control`, the exact sequence of entries, their arguments, the returned `u` and `info`, the printed lines with `time_print`
on and off, and the exception of a refused call.  The binding is the recording stand-in of capi_lib (`Recorder`), injected through `_backend=`."""
from collections import namedtuple

import numpy as np
import pytest

from capi_lib import Recorder, fixed_output
from rda_planner_amd import scenarios as sc
from rda_planner_amd.mpc import MPC
from rda_planner_amd.rda_solver import RDA_solver

T, N, E = 3, 2, 4
HalfSpaces = namedtuple("HalfSpaces", "A b cone_type")
ALL_FLAGS = dict(has_scene=True, has_track=True, has_pipeline=True, has_scan=True, has_scan_split=True)
RULE, TOTAL, END = "-" * 47, "iteration time:", "=" * 46
NO_UPDATE, LMZ_FAIL = "No update of state and control vector", "Update Lam Mu Fail"
NOM_S, NOM_U = np.arange(3.0 * (T + 1)).reshape(3, T + 1), 0.5 * np.arange(2.0 * T).reshape(2, T)
REF = [np.array([[1.0 + i], [2.0 * i], [0.25], [1.0]]) for i in range(T + 1)]            # 4 rows: the solver takes the first three
STATE = np.array([[0.5], [-0.25], [0.125]])
SCAN = dict(ranges=[3.0, 3.5, 4.0, 9.0], angle_min=-1.0, angle_max=1.0, range_max=9.0)
SCAN_HEAD = [4, np.array(SCAN["ranges"]), -1.0, 1.0, 9.0, STATE.ravel(), 2.0, 6]


def solver(time_print=False, **rec_kw):
    rec = Recorder(**{**ALL_FLAGS, **rec_kw})
    s = RDA_solver(T, sc.rectangle_robot(), max_edge_num=E, max_obs_num=N, iter_num=2, time_print=time_print, _backend=lambda cfg, G, h: rec)
    return s, rec


def same_calls(got, want):
    """the recorded calls are `want`: names in order; scalars equal and of the same type, arrays equal in type and content"""
    assert [name for name, _ in got] == [name for name, _ in want]
    for (name, g), (_, w) in zip(got, want):
        if w is None:                                    # (arguments checked elsewhere)
            continue
        assert len(g) == len(w), name
        for k, (a, b) in enumerate(zip(g, w)):
            if isinstance(b, np.ndarray):
                assert isinstance(a, np.ndarray) and a.dtype == b.dtype and np.array_equal(a.ravel(), b.ravel()), (name, k, a, b)
            else:
                assert type(a) is type(b) and a == b, (name, k, a, b)


def same_lines(text, want):
    """the captured stdout, line for line; the wall-clock number behind "iteration time:" by prefix"""
    got = text.splitlines()
    assert len(got) == len(want), got
    for g, w in zip(got, want):
        assert g.startswith(TOTAL) if w == TOTAL else g == w, got


def timing_lines(time_print, timing=True, info=Recorder.INFO, threshold=0.2):
    """what `time_print` prints behind a step (reference rda_solver.py:587-601, :699)"""
    if not time_print:
        return []
    t = fixed_output(2, (3,))                             # both timing_launches calls hand back two launches: entries 0 and 1 of this
    lines = [NO_UPDATE] if info["su_status"] else []
    if timing:
        lines += ["iteration " + str(i) + " time:  " + str((t[i] + t[i]) * 1e-3) for i in range(info["iters"])]
    if info["resi_dual"] < threshold and info["resi_pri"] < threshold:
        lines.append("iteration early stop: " + str(info["iters"] - 1))
    return lines + [RULE, TOTAL, END]


def timing_calls(time_print, timing=True, begin=True):
    """the timing entries around a step: the reset in front (`begin`), else the two reads and the reset behind"""
    if not (time_print and timing):
        return []
    return [("timing_reset", [1])] if begin else [("timing_launches", [1, "out", 3, "out"]), ("timing_launches", [0, "out", 3, "out"]), ("timing_reset", [0])]


def check_info(info, ref_states, s_pos, rec_info=Recorder.INFO):
    """every key of `info`: the counters of the library's record, the optimal states as columns of the output at argument `s_pos`"""
    assert set(info) == {"ref_traj_list", "opt_state_list", "iteration_time", "resi_dual", "resi_pri", "iters", "status", "su_ipm_iters", "lmz_fail"}
    s = fixed_output(s_pos, (3, T + 1))
    assert len(info["opt_state_list"]) == T + 1 and all(np.array_equal(c, s[:, i:i + 1]) for i, c in enumerate(info["opt_state_list"]))
    assert len(info["ref_traj_list"]) == T + 1 and all(np.array_equal(a, b) for a, b in zip(info["ref_traj_list"], ref_states))
    assert 0 <= info["iteration_time"] < 60
    assert {k: info[k] for k in ("resi_dual", "resi_pri", "iters", "su_ipm_iters", "lmz_fail")} == {k: rec_info[k] for k in ("resi_dual", "resi_pri", "iters", "su_ipm_iters", "lmz_fail")}
    assert info["status"] == rec_info["su_status"]


def tracked_ref(pos):
    r = fixed_output(pos, (3, T + 1))
    return [r[:, i:i + 1] for i in range(T + 1)]


def half_spaces():
    """two obstacles in the reference's (A, b, cone) form: a triangle (3 of E = 4 edges used) and a circle"""
    tri = HalfSpaces(np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, -1.0]]), np.array([[4.0], [5.0], [-6.0]]), "Rpositive")
    disc = HalfSpaces(np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]), np.array([[7.0], [8.0], [-0.5]]), "norm2")
    A, b = np.zeros((2, 1, E, 2)), np.zeros((2, 1, E))
    A[0, 0, :3], A[1, 0, :3], b[0, 0, :3], b[1, 0, :3] = tri.A, disc.A, tri.b.ravel(), disc.b.ravel()
    return [tri, disc], [2, A, b, np.array([0, 1], np.int32), 0]


def raw_scene():
    """a flattened scene as `flatten_scene` returns it, with the index arrays in another integer type than the library's"""
    geom = np.arange(2.0 * E * 2).reshape(2, E, 2)
    scene = (2, np.array([0, 1], np.int64), np.array([4, 0], np.int64), geom, np.array([[0.5, 0.0], [0.0, -0.5]]))
    return scene, [2, np.array([0, 1], np.int32), np.array([4, 0], np.int32), geom, scene[4], np.array([0.5, -0.25]), 1]


NOMINAL = [NOM_S, NOM_U, np.hstack(REF)[0:3]]
LAST = ("last_nonconvex", [])
# name -> (the call of the step form, the library calls it makes between the timing entries, argument of out_u, of out_s, of the tracked outputs)
STEPS = {
    "solve": (lambda s: s.iterative_solve(NOM_S, NOM_U, REF, 1.5, half_spaces()[0]), [("step", NOMINAL + [1.5] + half_spaces()[1] + ["out"] * 3)], 10, 11, None),
    "scene": (lambda s: s.iterative_solve_scene(NOM_S, NOM_U, REF, 1.5, raw_scene()[0], STATE, True),
              [("step_scene", NOMINAL + [1.5] + raw_scene()[1] + ["out"] * 3)], 12, 13, None),
    "staged": (lambda s: s.iterative_solve_staged(NOM_S, NOM_U, REF, 1.5),
               [("upload_trace", [1] + NOMINAL + [np.array([1.5])]), ("enqueue_step", [0]), ("sync", []), ("fetch_result", [0, "out", "out", "out"])], 2, 3, None),
    "tracked": (lambda s: s.iterative_solve_tracked(STATE, 1.5, 4, NOM_U, threshold=0.2, ind_range=5),
                [("step_tracked", [STATE.ravel(), 1.5, 4, 0.2, 5, NOM_U, "out", "out", "out", None, "out", "out", "out"])], 7, 8, 11),
    "tracked_resident": (lambda s: s.iterative_solve_tracked(np.append(STATE.ravel(), 9.0), 2, np.int64(4)),
                         [("step_tracked", [STATE.ravel(), 2.0, 4, 0.1, 10, None, "out", "out", "out", None, "out", "out", "out"])], 7, 8, 11),
}


@pytest.mark.parametrize("time_print", [False, True])
@pytest.mark.parametrize("form", list(STEPS))
def test_step_forms(form, time_print, capsys):
    call, lib_calls, u_pos, s_pos, ref_pos = STEPS[form]
    s, rec = solver(time_print)
    out = call(s)
    same_calls(rec.calls, timing_calls(time_print) + lib_calls + timing_calls(time_print, begin=False) + [LAST])
    assert np.array_equal(out[0], fixed_output(u_pos, (2, T)))
    check_info(out[1], REF if ref_pos is None else tracked_ref(ref_pos), s_pos)
    assert len(out) == (2 if ref_pos is None else 4)
    if ref_pos is not None:
        assert out[2:] == (2, float(ref_pos + 2)) and type(out[2]) is int and type(out[3]) is float
    same_lines(capsys.readouterr().out, timing_lines(time_print))


@pytest.mark.parametrize("time_print", [False, True])
def test_tick_in_two_halves(time_print, capsys):
    """tracked_begin / tracked_finish: the timing reset in front of the first half, the report behind the second; a discarded tick returns None and
    reports nothing, whatever the library answers"""
    s, rec = solver(time_print)
    assert s.tracked_begin(STATE, 1.5, 4, NOM_U, threshold=0.2, ind_range=5) is None
    s.upload_scene_async(raw_scene()[0], STATE, False)
    u, info, mi, eh = s.tracked_finish()
    finish = ("tracked_finish", ["out", "out", "out", None, "out", "out", "out"])
    same_calls(rec.calls, timing_calls(time_print) + [("tracked_begin", [STATE.ravel(), 1.5, 4, 0.2, 5, NOM_U]), ("upload_scene_async", raw_scene()[1][:-1] + [0]),
                                                       finish] + timing_calls(time_print, begin=False) + [LAST])
    assert np.array_equal(u, fixed_output(1, (2, T))) and (mi, eh) == (2, 7.0)
    check_info(info, tracked_ref(5), 2)
    same_lines(capsys.readouterr().out, timing_lines(time_print))
    for fail in ({}, {"tracked_finish": -3}):
        s, rec = solver(time_print, fail=fail)
        s.tracked_begin(STATE, 1.5, 4)
        assert s.tracked_finish(discard=True) is None
        same_calls(rec.calls, timing_calls(time_print) + [("tracked_begin", [STATE.ravel(), 1.5, 4, 0.1, 10, None]), finish])
        assert capsys.readouterr().out == ""


@pytest.mark.parametrize("time_print", [False, True])
@pytest.mark.parametrize("timing", [False, True])
def test_printed_lines(timing, time_print, capsys):
    """the lines that depend on the step's outcome, in the epilogue's order: no update of the su-problem (with time_print only) in front of the
    per-iteration lines, no early stop above the threshold, then a failed LamMuZ row and non-convex polygons (both printed unconditionally); a library
    without the timing entries (`timing` off) prints no per-iteration lines"""
    info = dict(Recorder.INFO, su_status=1, lmz_fail=3, resi_dual=0.5)
    s, rec = solver(time_print, info=info, nonconvex=2, timing=timing)
    u, got = s.iterative_solve(NOM_S, NOM_U, REF, 1.5, half_spaces()[0])
    check_info(got, REF, 11, info)
    assert rec.names() == [name for name, _ in timing_calls(time_print, timing)] + ["step"] + [name for name, _ in timing_calls(time_print, timing, begin=False)] + ["last_nonconvex"]
    lines = timing_lines(time_print, timing, info)
    assert not time_print or lines[0] == NO_UPDATE
    same_lines(capsys.readouterr().out, lines + [LMZ_FAIL, "Warning: 2 polygon(s) constructed by vertex are not convex. Please check the vertex"])


def test_uploads_and_scans():
    s, rec = solver()
    scene, scene_args = raw_scene()
    s.upload_scene(scene, STATE, True)
    s.upload_scene_async(scene, [0.5, -0.25, 7.0], 0)
    s.upload_obstacles(half_spaces()[0])
    s.upload_obstacles([])
    s.upload_path(REF)
    s.upload_path_pieces([REF[0:3], [np.vstack((p[0:3], [[-1.0]])) for p in REF[1:3]], REF[3:4]])      # (the fourth row is the gear)
    s.scene_resort(STATE)
    boxes, labels = s.scan_boxes(STATE, SCAN, with_labels=True)
    assert np.array_equal(boxes, fixed_output(10, (4, 4, 2))[:2]) and np.array_equal(labels, np.full(4, 2, np.int32))
    assert np.array_equal(s.scan_boxes(STATE, SCAN, eps=1.0, min_samples=3, split=0.25), boxes)
    assert s.upload_scan(STATE, SCAN, split=0.25) == 2                                       # (the split is unchanged: no library call)
    assert s.upload_scan(STATE, SCAN, 1.0, 3, False) == 2                                    # ... and off again
    path = np.hstack(REF)[0:3].T
    same_calls(rec.calls, [
        ("upload_scene", scene_args + [None]), ("upload_scene_async", scene_args[:-1] + [0]),
        ("upload_obstacles", half_spaces()[1]), ("upload_obstacles", [0, None, None, None, 0]),
        ("upload_path", [T + 1, path]),
        ("upload_path_pieces", [3, np.array([3, 2, 1], np.int32), np.array([1.0, -1.0, 1.0]), path[[0, 1, 2, 1, 2, 3]]]),
        ("scene_resort", [np.array([0.5, -0.25])]),
        ("scan_boxes", SCAN_HEAD + ["out", "out", 4, "out"]),
        ("set_scan_split", [0.25]), ("scan_boxes", SCAN_HEAD[:6] + [1.0, 3, "out", "out", 4, "out"]),
        ("upload_scan", SCAN_HEAD + [1, "out"]),
        ("set_scan_split", [0.0]), ("upload_scan", SCAN_HEAD[:6] + [1.0, 3, 0, "out"])])


REFUSED = {
    "step": STEPS["solve"][0], "step_scene": STEPS["scene"][0], "step_tracked": STEPS["tracked"][0],
    "tracked_begin": lambda s: s.tracked_begin(STATE, 1.5, 4), "tracked_finish": lambda s: s.tracked_finish(),
    "upload_scene": lambda s: s.upload_scene(raw_scene()[0], STATE, True), "upload_scene_async": lambda s: s.upload_scene_async(raw_scene()[0], STATE, True),
    "upload_obstacles": lambda s: s.upload_obstacles([]), "upload_path": lambda s: s.upload_path(REF), "upload_path_pieces": lambda s: s.upload_path_pieces([REF]),
    "scene_resort": lambda s: s.scene_resort(STATE), "scan_boxes": lambda s: s.scan_boxes(STATE, SCAN), "upload_scan": lambda s: s.upload_scan(STATE, SCAN),
    "set_scan_split": lambda s: s.set_scan_split(0.25),
}


@pytest.mark.parametrize("entry", list(REFUSED))
def test_refused_call(entry, capsys):
    """a negative code is a RuntimeError that names the entry and the code, raised before anything is printed; nothing follows the refused call"""
    s, rec = solver(True, fail={entry: -3})
    with pytest.raises(RuntimeError) as e:
        REFUSED[entry](s)
    assert str(e.value) == f"rda_{entry} failed with code -3"
    assert rec.names()[-1] == entry and capsys.readouterr().out == ""


def test_refusals_with_their_own_text(capsys):
    for k, entry in enumerate(("upload_trace", "enqueue_step", "sync", "fetch_result")):
        s, rec = solver(fail={entry: -3})
        with pytest.raises(RuntimeError) as e:
            s.iterative_solve_staged(NOM_S, NOM_U, REF, 1.5)
        assert str(e.value) == "rda: the step on the staged obstacles failed with code -3"
        assert rec.names() == ["upload_trace", "enqueue_step", "sync", "fetch_result"][:k + 1]
    s, rec = solver(fail={"set_scan_split": -1})
    for _ in range(2):                                   # (a refused tolerance is not remembered)
        with pytest.raises(ValueError) as e:
            s.set_scan_split(-0.5)
        assert str(e.value) == "scan split: tol must be finite and greater than 0"
    s.set_scan_split(0.0)
    assert rec.names() == ["set_scan_split"] * 2
    s, rec = solver(has_scan_split=False)
    with pytest.raises(RuntimeError) as e:
        s.upload_scan(STATE, SCAN, split=0.25)
    assert str(e.value) == "the loaded solver library cannot split scan clusters (rda_set_scan_split, rda_fleet_set_scan_split)" and rec.calls == []


# ---- MPC.control ----------------------------------------------------------------------------------------------------------------------
PATH_STEP = 0.5


def mpc_and_twin(time_print=False, rec_kw=None, **kw):
    """an `MPC` on a recorder and an identical one that is never stepped, for the values `control` derives on the host"""
    def one():
        rec = Recorder(**{**ALL_FLAGS, **(rec_kw or {})})
        m = MPC(sc.rectangle_robot(), sc.line_path([0, 0, 0], [6, 0, 0], PATH_STEP), receding=T, iter_num=2, max_edge_num=E, max_obs_num=N,
                time_print=time_print, _backend=lambda cfg, G, h: rec, **kw)
        return m, rec
    return one() + one()[:1]


def obstacles():
    return [sc.box(3.0, 1.0, 1.0, 0.5, 0.3, velocity=(0.25, 0.0)), sc.circle(2.0, -2.0, 0.5)]


def scene_args(m, state, obs):
    n, kind, nvert, geom, vel = m.rda.flatten_scene(obs)
    return [n, kind, nvert, geom, vel, np.asarray(state, float).ravel()[0:2], int(bool(m.obstacle_order))]


def path_call(m):
    P = np.hstack(m.ref_path)[0:3].T
    return ("upload_path", [len(P), P])


def check_control(m, rec, out, u_pos, s_pos, arrive=False):
    u, info = out
    full = fixed_output(u_pos, (2, T))
    assert np.array_equal(u, full[:, 0:1]) and np.array_equal(m.cur_vel_array, full)
    assert info.pop("arrive") is arrive
    check_info(info, info["ref_traj_list"], s_pos)


@pytest.mark.parametrize("time_print", [False, True])
@pytest.mark.parametrize("device", [False, True])
def test_control_untracked(device, time_print, capsys):
    """device_track=False: the host's pre_process, then rda_step with the host's half-spaces or rda_step_scene with the raw scene"""
    m, rec, twin = mpc_and_twin(time_print, device_track=False, device_obstacles=device)
    _, speed, nom_s, ref_list = twin._begin(STATE, 1.5)
    out = m.control(STATE, 1.5, obstacles())
    nominal = [nom_s, np.zeros((2, T)), np.hstack(ref_list)[0:3], 1.5]
    if device:
        step = ("step_scene", nominal + scene_args(twin, STATE, obstacles()) + ["out"] * 3)
    else:
        n, A, b, cone, per_t = twin.rda._stage(twin.convert_rda_obstacle(obstacles(), twin.state, True))
        step = ("step", nominal + [n, A, b, cone, per_t] + ["out"] * 3)
        assert per_t == 1 and n == 2
    same_calls(rec.calls, timing_calls(time_print) + [step] + timing_calls(time_print, begin=False) + [LAST])
    check_control(m, rec, out, *((12, 13) if device else (10, 11)))
    assert all(np.array_equal(a, b) for a, b in zip(out[1]["ref_traj_list"], ref_list)) and m.cur_index == twin.cur_index
    same_lines(capsys.readouterr().out, timing_lines(time_print))


@pytest.mark.parametrize("time_print", [False, True])
@pytest.mark.parametrize("pipeline", [False, True])
def test_control_tracked(pipeline, time_print, capsys):
    """two ticks of the tracked route: the path goes up once, the nominal controls only while the device does not hold them; with the pipeline the
    scene is staged inside the open tick, without it in front of rda_step_tracked"""
    m, rec, twin = mpc_and_twin(time_print)
    m.rda.pipeline = pipeline
    state4 = np.vstack((STATE, [[1.0]]))                  # a fourth row (the gear of a reverse path) is cut off
    outs = [m.control(state4, 1.5, obstacles(), threshold=0.2), m.control(STATE, 1.5, obstacles())]
    want = [path_call(twin)]
    for tick, (thr, nom_u) in enumerate(((0.2, np.zeros((2, T))), (0.1, None))):
        head = [STATE.ravel(), 1.5, 2 * tick, thr, 10, nom_u]
        if pipeline:
            want += timing_calls(time_print) + [("tracked_begin", head), ("upload_scene_async", scene_args(twin, STATE, obstacles())),
                                                ("tracked_finish", ["out", "out", "out", None, "out", "out", "out"])]
        else:
            want += [("upload_scene", scene_args(twin, STATE, obstacles()) + [None])] + timing_calls(time_print)
            want += [("step_tracked", head + ["out", "out", "out", None, "out", "out", "out"])]
        want += timing_calls(time_print, begin=False) + [LAST]
    same_calls(rec.calls, want)
    u_pos, s_pos, ref_pos = (1, 2, 5) if pipeline else (7, 8, 11)
    for out in outs:
        check_control(m, rec, out, u_pos, s_pos)
        assert all(np.array_equal(a, b) for a, b in zip(out[1]["ref_traj_list"], tracked_ref(ref_pos)))
    assert m.cur_index == 2 and m.ref_path[-1][2, 0] == ref_pos + 2 and np.array_equal(m.state, STATE)      # quirk Q12: the device's end heading
    same_lines(capsys.readouterr().out, timing_lines(time_print) * 2)


@pytest.mark.parametrize("time_print", [False, True])
@pytest.mark.parametrize("route", ["pipeline", "serial", "untracked"])
def test_control_scan(route, time_print, capsys):
    m, rec, twin = mpc_and_twin(time_print, device_track=route != "untracked")
    m.rda.pipeline = route == "pipeline"
    out = m.control(STATE, 1.5, scan=SCAN, scan_eps=1.0, scan_min_samples=3, scan_split=0.25)
    scan = ("upload_scan", SCAN_HEAD[:6] + [1.0, 3, 1, "out"])
    split, begin, end = [("set_scan_split", [0.25])], timing_calls(time_print), timing_calls(time_print, begin=False) + [LAST]
    head = [STATE.ravel(), 1.5, 0, 0.1, 10, np.zeros((2, T))]
    if route == "pipeline":
        want = [path_call(twin)] + begin + [("tracked_begin", head)] + split + [scan, ("tracked_finish", ["out", "out", "out", None, "out", "out", "out"])] + end
        pos = (1, 2)
    elif route == "serial":
        want = [path_call(twin)] + split + [scan] + begin + [("step_tracked", head + ["out", "out", "out", None, "out", "out", "out"])] + end
        pos = (7, 8)
    else:
        _, speed, nom_s, ref_list = twin._begin(STATE, 1.5)
        want = split + [scan] + begin + [("upload_trace", [1, nom_s, np.zeros((2, T)), np.hstack(ref_list)[0:3], np.array([1.5])]), ("enqueue_step", [0]), ("sync", []),
                                         ("fetch_result", [0, "out", "out", "out"])] + end
        pos = (2, 3)
    same_calls(rec.calls, want)
    check_control(m, rec, out, *pos)
    same_lines(capsys.readouterr().out, timing_lines(time_print))
    with pytest.raises(ValueError, match="either an obstacle_list or scan="):
        m.control(STATE, 1.5, obstacles(), scan=SCAN)


class Broken:
    """an obstacle whose attributes cannot be read"""
    @property
    def cone_type(self):
        raise KeyError("broken obstacle")


@pytest.mark.parametrize("time_print", [False, True])
def test_staging_error_closes_the_open_tick(time_print, capsys):
    """staging that raises inside an open tick: rda_tracked_finish is called exactly once, as a discard, and the caller sees the staging's own exception"""
    m, rec, _ = mpc_and_twin(time_print)
    with pytest.raises(KeyError, match="broken obstacle"):
        m.control(STATE, 1.5, [Broken()])
    assert rec.names() == ["upload_path"] + ["timing_reset"] * time_print + ["tracked_begin", "tracked_finish"]
    m, rec, _ = mpc_and_twin(time_print, rec_kw=dict(fail={"upload_scan": -3, "tracked_finish": -2}))
    with pytest.raises(RuntimeError) as e:
        m.control(STATE, 1.5, scan=SCAN)
    assert str(e.value) == "rda_upload_scan failed with code -3"
    assert rec.names() == ["upload_path"] + ["timing_reset"] * time_print + ["tracked_begin", "upload_scan", "tracked_finish"]
    m, rec, _ = mpc_and_twin(time_print)                  # without the pipeline no tick is open: nothing to close
    m.rda.pipeline = False
    with pytest.raises(KeyError, match="broken obstacle"):
        m.control(STATE, 1.5, [Broken()])
    assert rec.names() == ["upload_path"] and capsys.readouterr().out == ""


def test_control_host_list_in_a_tracked_tick():
    """rda_obstacle=True: the caller's half-spaces are staged by rda_upload_obstacles, inside the open tick too"""
    m, rec, twin = mpc_and_twin(rda_obstacle=True)
    obs, staged = half_spaces()
    m.control(STATE, 1.5, obs)
    same_calls(rec.calls, [path_call(twin), ("tracked_begin", None), ("upload_obstacles", staged), ("tracked_finish", None), LAST])
