"""
`Fleet` - B independent `MPC` planners stepped together (BASELINE config C5, "batched multi-ego").

The reference has one `MPC` / `RDA_solver` object per robot and a multi-robot user calls `control` in a loop, one
CVXPY solve after the other (mpc.py:127-187).  Here the members are still ordinary `MPC` objects - own path, state,
obstacles, weights - but `Fleet.control` issues their ADMM iterations as ONE set of kernel launches with an ego
dimension in the grid (include/rda_hip.h, `rda_fleet_*`): the su-problems of all members run side by side on B compute
units and the LamMuZ grid is B times larger, which is what a 256-CU part needs.  Every member's result is identical to
what `member.control(...)` would have returned.
"""
import ctypes as C
import time
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from ._capi import Info, c_arg, dptr, iptr, f64
from .mpc import scan_split_arg
from .rda_solver import RDA_solver, scene_arrays, step_epilogue

SENSOR_FIELDS = ("number", "angle_min", "angle_max", "range_min", "range_max")
WORLD_EMAX = 8              # RDA_EMAX of include/rda_hip.h: the most vertices a world polygon may have

# the arguments of the eight rollout entries in the order of include/rda_hip.h, by name: `rollout_args` resolves a row against the values of a call.
# `logs` (s_log u_log i_log infos arrived), `sensors` (n_beams angle_min angle_max range_min range_max) and `plans` (plans valid) stand for several.
_HEAD = "F K states speed cur threshold ind_range margin"
_LIDAR = _HEAD + " nom_u sensors scan_eps scan_min_samples order moving logs box_log clearance_log"
ROLLOUT_ARGS = {
    "fleet_rollout":               _HEAD + " resort nom_u logs",
    "fleet_rollout_moving":        _HEAD + " resort nom_u logs clearance_log",
    "fleet_rollout_gears":         "F K states speed piece0 cur threshold ind_range margin resort moving nom_u logs piece_log clearance_log",
    "fleet_rollout_peers":         _HEAD + " nom_u ctl0 logs clearance_log peer_log",
    "fleet_rollout_peers_plan":    _HEAD + " nom_u ctl0 logs clearance_log peer_log plans",
    "fleet_rollout_lidar":         _LIDAR,
    "fleet_rollout_lidar_peers":   _LIDAR + " peer_log",
    "fleet_rollout_lidar_tracked": _LIDAR + " peer_log see_peers track_gate track_window",
}


def rollout_args(entry, values):
    """the positional arguments of the rollout entry `entry`: its row of ROLLOUT_ARGS resolved against `values` (name -> value, a tuple for a group)"""
    named = (values[name] for name in ROLLOUT_ARGS[entry].split())
    return [c_arg(v) for one in named for v in (one if isinstance(one, tuple) else (one,))]


# what one `Fleet.rollout` call asks for, as `Fleet._rollout_options` returns it: once it exists, every refusal that needs no library call has happened.
# sensors: the arrays of `sensor_arrays`, None without lidar=; margin: the members' common goal_index_threshold; entry: a key of ROLLOUT_ARGS
RolloutOptions = namedtuple("RolloutOptions", "resort gears peers plan see_peers track track_gate track_window split moving clearance sensors scan_eps "
                            "scan_min_samples obstacle_lists world threshold ind_range margin entry")


def rollout_entry(o):
    """the C entry point that runs the rollout of the options `o`"""
    if o.gears:
        return "fleet_rollout_gears"
    if o.peers:
        return "fleet_rollout_peers_plan" if o.plan else "fleet_rollout_peers"
    if o.sensors is not None:
        return "fleet_rollout_lidar_tracked" if o.track else "fleet_rollout_lidar_peers" if o.see_peers else "fleet_rollout_lidar"
    return "fleet_rollout_moving" if o.moving else "fleet_rollout"


def sensor_arrays(sensors, B):
    """B lidar sensors - mappings or objects (`World.lidar`) with `number`, `angle_min`, `angle_max`, `range_min`, `range_max` - as the member-major
    arrays of rda_fleet_raycast: (n_beams, angle_min, angle_max, range_min, range_max)"""
    if sensors is None or len(sensors) != B:
        raise ValueError("one sensor per member")
    rows = []
    for s in sensors:
        try:
            row = [s[k] if hasattr(s, "keys") else getattr(s, k) for k in SENSOR_FIELDS]
        except (KeyError, AttributeError, TypeError) as e:
            raise ValueError(f"a sensor needs {', '.join(SENSOR_FIELDS)}: {e!r}") from None
        n, lo, hi, rmin, rmax = int(row[0]), *(float(x) for x in row[1:])
        if n != row[0] or n < 0:
            raise ValueError(f"sensor: number = {row[0]!r} is not a beam count")
        if not all(np.isfinite([lo, hi, rmin, rmax])) or hi < lo or rmin < 0 or rmax < rmin:
            raise ValueError(f"sensor: need finite angle_min <= angle_max and 0 <= range_min <= range_max, got {row[1:]}")
        rows.append((n, lo, hi, rmin, rmax))
    cols = list(zip(*rows))
    return (np.array(cols[0], np.int32),) + tuple(f64(c) for c in cols[1:])


def peers_mode(peers):
    """the `peers=` argument of `Fleet.control` / `Fleet.rollout` -> (peers on, predicted along their plans)"""
    if isinstance(peers, str) and peers == "plan":
        return True, True
    if peers is None or isinstance(peers, (bool, int, np.bool_, np.integer)):
        return bool(peers), False
    raise ValueError(f'peers={peers!r}: False, True (constant velocity) or "plan" (along the planned trajectories)')


def states_array(states, B):
    """B states - (3,), (3, 1) or longer - as one contiguous (B, 3) array"""
    return f64([np.asarray(x, float).ravel()[0:3] for x in states], (B, 3))


class Fleet:
    def __init__(self, members):
        """members: `MPC` objects with equal receding / max_obs_num / max_edge_num / iter_num and robots with the same
        number of edges.  Either all members or none use the interior-point LamMuZ mode (`lmz_central=`; its value may differ
        per member), and no member is a circle (norm2) robot.  Anything else may differ."""
        self.members = list(members)
        if not self.members:
            raise ValueError("a fleet needs at least one member")
        self.api = self.members[0].rda._be.api
        if not self._has("has_fleet"):
            raise RuntimeError("the loaded solver library has no fleet entry points")
        B = len(self.members)
        arr = (C.c_void_p * B)(*[m.rda._be.handle for m in self.members])
        self._handle = C.c_void_p()
        rc = self.api.fleet_create(arr, B, C.byref(self._handle))
        if rc != 0:
            raise RuntimeError(f"rda_fleet_create failed with code {rc} (members must agree on T, N, E, R, iter_num; "
                               "either all members or none use lmz_central; a circle (norm2) robot cannot be a member)")
        T = self.members[0].receding
        self._in_s, self._in_u = np.zeros((B, 3, T + 1)), np.zeros((B, 2, T))
        self._ref, self._speed = np.zeros((B, 3, T + 1)), np.zeros(B)
        self._out_u, self._out_s = np.zeros((B, 2, T)), np.zeros((B, 3, T + 1))
        self._info = (Info * B)()
        self.batched_ticks = 0          # ticks whose scenes went through the one-pass staging (diagnostics)
        self._peers_staged = False      # the members' resident scenes are those of rda_fleet_upload_scenes_peers
        self._plan_state()

    def __len__(self):
        return len(self.members)

    def _call(self, name, *args):
        """the library's `name(*args)`; a negative return code raises what the binding makes of it"""
        rc = getattr(self.api, name)(*args)
        if rc < 0:
            raise self.api.failed(name, rc)
        return rc

    def _has(self, flag):
        return getattr(self.api, flag, False)

    def _plan_state(self):
        """every member's last planned states (B, 3, T+1) - the `opt_state_list` of its last tick through this fleet - and whether they count
        (B,): not before its first tick, not after `reset`, not once it has arrived.  What peers="plan" predicts the members along."""
        if getattr(self, "_plans", None) is None:
            B, T = len(self.members), self.members[0].receding
            self._plans, self._plan_valid = np.zeros((B, 3, T + 1)), np.zeros(B, np.int32)
        return self._plans, self._plan_valid

    @property
    def plan_valid(self):
        """(B,) bool: member i has a plan that peers="plan" uses"""
        return self._plan_state()[1].astype(bool)

    def _note_plan(self, i, out_s, arrived):
        plans, valid = self._plan_state()
        plans[i] = f64(out_s, plans[i].shape)
        valid[i] = 0 if arrived else 1

    def reset(self, which=None):
        """`MPC.reset` of the members `which` (indices; default: all); their plans no longer count for peers="plan" and their box tracks
        (`track=True`) end"""
        _, valid = self._plan_state()
        which = list(range(len(self.members)) if which is None else which)
        for i in which:
            self.members[i].reset()
            valid[i] = 0
        if self._has("has_fleet_lidar_tracked"):
            self.reset_tracks(which)

    def lammuz_kernel(self):
        """the LamMuZ launches the next tick issues per ADMM iteration as the members stand now (rda_fleet_lammuz_kernel): kernel names joined by '+'"""
        return self.api.fleet_lammuz_kernel(self._handle).decode()

    def close(self):
        if self._handle:
            self.api.fleet_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def control(self, states, ref_speeds, obstacle_lists=None, scans=None, scan_eps=2.0, scan_min_samples=6, peers=False, peer_controls=None,
                track=False, track_gate=1.0, track_window=8, **kwargs):
        """one MPC step of every member: `states[i]`, `ref_speeds[i]` (a scalar is shared) and `obstacle_lists[i]` are
        what `members[i].control` takes; returns the list of its `(u, info)` results.
        scans: instead of obstacle lists, `scans[i]` is the range scan (the dict `MPC.control(scan=)` takes) member i took from
        `states[i]` - all members' scans are clustered, boxed and staged on the device by one library call
        (rda_fleet_upload_scans); result i is what `members[i].control(states[i], ref_speeds[i], scan=scans[i])` returns.
        peers=True: the members avoid each other.  Every member's scene is `obstacle_lists[i]` followed by the other members as moving polygon
        obstacles - their footprints at `states`, their velocity the control `peer_controls[j]` = (v, w) they applied on the previous tick along
        their heading (default: `members[j].cur_vel_array[:, 0]`, which is zero before the first tick and once the member has arrived) - written on
        the device by rda_fleet_upload_scenes_peers; result i is what `members[i].control(states[i], ref_speeds[i], obstacle_lists[i] +
        scenarios.peer_obstacles(cars, states, peer_controls, i))` returns.  Device-tracked members with `obstacle_order=True` and polygon robots only;
        anything else raises, there is no host fallback.
        peers="plan": the same, but a member that has a plan - it went through a tick of this fleet, was not `reset` since and has not arrived - is
        predicted along it instead of at constant velocity: at stage t >= 1 its footprint stands at `scenarios.peer_plan_poses` of its state and the
        `opt_state_list` of its last tick (the plan as displacements anchored at the actual state, the last increment repeated at stage T);
        rda_fleet_upload_scenes_peers_plan, `scenarios.peer_plan_obstacles` is the specification.  Any other value of `peers` is a ValueError.
        track=True (with scans=; rda_fleet_upload_scans_tracked): the boxes are associated with those of the previous tracked tick on the device and
        staged with the velocity of their track (`lidar.track_boxes` is the specification: mutual nearest neighbour within `track_gate` metres,
        displacement over the track's age of up to `track_window` <= 8 ticks), so a lidar obstacle is predicted over the horizon like any obstacle with
        a velocity.  Successive tracked ticks are taken to be one `sample_time` apart; `reset_tracks` after a gap.  Result i is what
        `members[i].control(states[i], ref_speeds[i], lidar.scan_box_tracked(...)[0])` returns with the same tracks.  Without scans= a ValueError.
        scan_split=tol (with scans=; rda_fleet_set_scan_split): every member's clusters are cut into their straight runs on the device, one box per run
        (`lidar.scan_box_split` is the specification) - for scenes with walls, where one box per cluster covers the free space the robot stands in.
        tol [m] finite and > 0; omitted: off, also after a split tick.  Combines with track=True: the tracker only ever sees boxes."""
        B, start = len(self.members), time.time()
        if np.isscalar(ref_speeds):
            ref_speeds = [ref_speeds] * B
        split = scan_split_arg(kwargs, "Fleet.control", scans is not None, "scans=")
        if split:
            self._check_split()
        if track and scans is None:
            raise ValueError("Fleet.control: track=True tracks the boxes of scans=")
        if track:
            self._check_track(track_gate, track_window)
        peers, plan = peers_mode(peers)
        if peers:
            if scans is not None:
                raise ValueError("Fleet.control: peers=True takes obstacle_lists, not scans=")
            self._check_peers(kwargs, plan)
            if peer_controls is None:
                peer_controls = [np.asarray(m.cur_vel_array, float)[:, 0] for m in self.members]
            if len(peer_controls) != B or (obstacle_lists is not None and len(obstacle_lists) != B):
                raise ValueError("Fleet.control: one obstacle list and one peer control per member")
            ctl = f64([np.asarray(c, float).ravel()[0:2] for c in peer_controls], (B, 2))
            own = obstacle_lists if obstacle_lists is not None else [[] for _ in range(B)]
            return self._control_tracked(states, ref_speeds, own, start, stage=lambda st: self._stage_peers(own, st, ctl, plan), **kwargs)
        self._peers_staged = False
        if scans is not None:
            if obstacle_lists is not None and any(len(ol) for ol in obstacle_lists):
                raise ValueError("Fleet.control: pass either obstacle_lists or scans=, not both")
            if len(scans) != B:
                raise ValueError("Fleet.control: one scan per member")
            if not self._has("has_fleet_scans") or any(m.rda_obstacle for m in self.members):
                raise RuntimeError("Fleet.control(scans=...) needs the fleet lidar front end (rda_fleet_upload_scans); there is no host fallback")
            stage = lambda st: self.upload_scans(st, scans, scan_eps, scan_min_samples,       # noqa: E731
                                                 track=(float(track_gate), int(track_window)) if track else None, split=split)
        else:
            if obstacle_lists is None:
                obstacle_lists = [[] for _ in range(B)]
            stage = None
        if hasattr(self.api.lib, "rda_fleet_step_tracked") and all(m._tracks(kwargs) for m in self.members):
            return self._control_tracked(states, ref_speeds, obstacle_lists, start, stage=stage, **kwargs)
        if track:
            raise RuntimeError("Fleet.control(track=True) needs device-side tracking of the path on every member; there is no host fallback")
        begun = []
        for i, m in enumerate(self.members):
            cur_ref_path, speed, nom_s, ref_list = m._begin(states[i], ref_speeds[i], **kwargs)
            T = m.receding
            self._in_s[i] = f64(nom_s, (3, T + 1))
            self._in_u[i] = f64(m.cur_vel_array, (2, T))
            self._ref[i] = np.hstack(ref_list)[0:3, :]
            self._speed[i] = speed
            begun.append((cur_ref_path, ref_list))
            if stage is None:
                m._stage_obstacles(obstacle_lists[i])
        if stage is not None:
            stage(states_array([m.state for m in self.members], len(self.members)))
        self._call("fleet_step", self._handle, dptr(self._in_s), dptr(self._in_u), dptr(self._ref), dptr(self._speed),
                   dptr(self._out_u), dptr(self._out_s), self._info)
        out = []
        for i, m in enumerate(self.members):
            cur_ref_path, ref_list = begun[i]
            out.append(m._end(cur_ref_path, *self._member_done(i, start, ref_list)))
            self._note_plan(i, self._out_s[i], out[-1][1]["arrive"])
        return out

    def _member_done(self, i, start, ref_list):
        """member i's (u, info) out of the fleet's output blocks: the epilogue of a step of its own solver, without a timing printout"""
        rda = self.members[i].rda
        return step_epilogue(rda.time_print, rda.pack_info, self._info[i], start, self._out_u[i].copy(), self._out_s[i].copy(), ref_list)

    def _stage_all(self, obstacle_lists, st):
        """all members' raw scenes flattened in ONE pass over the obstacle objects and staged by one library call
        (rda_fleet_upload_scenes, no waiting); False when some member needs the per-member route (host conversion, cone
        types the reference skips, too many vertices)"""
        ms = self.members
        if not self._has("has_fleet_scenes") or any(m.rda_obstacle or not m.device_obstacles or not m.rda.has_scene for m in ms):
            return False
        flat = self._flatten(obstacle_lists)
        if flat is None:
            return False
        rob = np.ascontiguousarray(st[:, 0:2])
        order = np.fromiter((bool(m.obstacle_order) for m in ms), np.int32, len(ms))
        self._call("fleet_upload_scenes", self._handle, *map(c_arg, flat), dptr(rob), iptr(order))
        self.batched_ticks += 1
        return True

    def _flatten(self, obstacle_lists):
        """all members' obstacle lists flattened in ONE pass over the obstacle objects: the arrays (counts, kind, nvert, geom, vel) of
        rda_fleet_upload_scenes and its peers forms, or None when an obstacle cannot be staged through the device pipeline"""
        every = [o for ol in obstacle_lists for o in ol]
        scene = self.members[0].rda.flatten_scene(every)
        if scene is None or scene[0] != len(every):
            return None
        counts = np.fromiter((len(ol) for ol in obstacle_lists), np.int32, len(self.members))
        return (counts, *scene_arrays(scene))

    def _check_peers(self, kwargs, plan=False):
        """what peers=True / peers="plan" needs of the library and of every member, checked before any library call"""
        ms = self.members
        if not self._has("has_fleet_peers"):
            raise RuntimeError("the loaded solver library has no peer entry points (rda_fleet_upload_scenes_peers, rda_fleet_rollout_peers)")
        if plan and not self._has("has_fleet_peers_plan"):
            raise RuntimeError('peers="plan": the loaded solver library has no plan entry points (rda_fleet_upload_scenes_peers_plan, rda_fleet_rollout_peers_plan)')
        if any(not m.obstacle_order for m in ms):
            raise RuntimeError("peers=True ranks every member's obstacles and peers by distance: obstacle_order=False is not supported")
        if any(m.car_tuple.cone_type == "norm2" for m in ms):
            raise RuntimeError("peers=True stages footprints as polygons; a circle (norm2) robot is not supported")
        if any(m.rda_obstacle or not m.device_obstacles or not m.rda.has_scene for m in ms):
            raise RuntimeError("peers=True needs the device-side obstacle pipeline on every member (rda_obstacle=False); there is no host fallback")
        if any(m.enable_reverse for m in ms) or not all(m._tracks(kwargs) for m in ms):
            raise RuntimeError("peers=True needs device-side tracking on every member and enable_reverse=False; there is no host fallback")

    def _stage_peers(self, obstacle_lists, st, controls, plan=False):
        """`_stage_all` with the other members behind every member's own obstacles (rda_fleet_upload_scenes_peers; plan: _peers_plan with the members'
        last plans and their validity); st (B, 3), controls (B, 2)"""
        flat = self._flatten(obstacle_lists)
        if flat is None:
            raise RuntimeError("peers=True: an obstacle cannot be staged through the device pipeline; there is no host fallback")
        head = (self._handle, *map(c_arg, flat), dptr(f64(st)), dptr(f64(controls)))
        if plan:
            self._call("fleet_upload_scenes_peers_plan", *head, *map(c_arg, self._plan_state()))
        else:
            self._call("fleet_upload_scenes_peers", *head)
        self._peers_staged = True
        self.batched_ticks += 1

    def peer_clearance(self, states):
        """(B,) every member's separation from the nearest other member at `states` (rda_fleet_peer_clearance: `scenarios.peer_clearance`
        evaluated on the device, one launch; negative = overlap, +inf for a fleet of one)"""
        if not self._has("has_fleet_peers"):
            raise RuntimeError("the loaded solver library has no peer entry points (rda_fleet_peer_clearance)")
        if any(m.car_tuple.cone_type == "norm2" for m in self.members):
            raise RuntimeError("Fleet.peer_clearance is for polygon robots; a circle (norm2) robot is not supported")
        st, out = states_array(states, len(self.members)), np.zeros(len(self.members))
        self._call("fleet_peer_clearance", self._handle, dptr(st), dptr(out))
        return out

    def _scan_arrays(self, states, scans):
        """the member-major arrays of rda_fleet_scan_boxes / rda_fleet_upload_scans"""
        B = len(self.members)
        if len(scans) != B or len(states) != B:
            raise ValueError("one state and one scan per member")
        ranges = [f64(np.asarray(s["ranges"], float).ravel()) for s in scans]
        n_beams = np.fromiter((r.size for r in ranges), np.int32, B)
        allr = np.concatenate(ranges) if n_beams.sum() else np.zeros(1)
        lo, hi, rmax = (f64([float(s[k]) for s in scans]) for k in ("angle_min", "angle_max", "range_max"))
        return n_beams, allr, lo, hi, rmax, states_array(states, B)

    def _check_split(self):
        if not self._has("has_scan_split"):
            raise RuntimeError("the loaded solver library cannot split scan clusters (rda_set_scan_split, rda_fleet_set_scan_split)")

    def set_scan_split(self, tol):
        """the split tolerance [m] of every member's scan in the fleet's calls (rda_fleet_set_scan_split; the members' own values are not read): 0
        switches the stage off.  The library is called only when the value changes."""
        tol = float(tol)
        if tol == getattr(self, "_scan_split", 0.0):
            return
        self._check_split()
        rc = self.api.fleet_set_scan_split(self._handle, tol)
        if rc < 0:
            raise ValueError("scan split: tol must be finite and greater than 0") if rc == -1 else self.api.failed("fleet_set_scan_split", rc)
        self._scan_split = tol

    def scan_boxes(self, states, scans, eps=2.0, min_samples=6, split=0.0):
        """`RDA_solver.scan_boxes` for every member in one kernel launch: the list of (n_i, 4, 2) corner arrays (split = tol > 0: one per straight run)"""
        if not self._has("has_fleet_scans"):
            raise RuntimeError("the loaded solver library has no fleet lidar entry points (rda_fleet_scan_boxes)")
        self.set_scan_split(split)
        n_beams, allr, lo, hi, rmax, st = self._scan_arrays(states, scans)
        B, cap = len(self.members), max(1, int(n_beams.max()))
        boxes, n = np.zeros((B, cap, 4, 2)), np.zeros(B, np.int32)
        self._call("fleet_scan_boxes", self._handle, iptr(n_beams), dptr(allr), dptr(lo), dptr(hi), dptr(rmax), dptr(st), float(eps), int(min_samples),
                   iptr(n), dptr(boxes), cap, None)
        return [boxes[i, :n[i]].copy() for i in range(B)]

    def upload_scans(self, states, scans, eps=2.0, min_samples=6, track=None, split=0.0):
        """`RDA_solver.upload_scan` for every member (its own `obstacle_order`) in one library call; returns the box counts.
        Until `sync` or the next `control` the members are not used on their own.  track=(gate, window): the tracked form
        (rda_fleet_upload_scans_tracked, see `control`).  split = tol > 0: the boxes of `lidar.scan_box_split`."""
        if not self._has("has_fleet_scans"):
            raise RuntimeError("the loaded solver library has no fleet lidar entry points (rda_fleet_upload_scans)")
        self.set_scan_split(split)
        if track is not None:
            self._check_track(*track)
        n_beams, allr, lo, hi, rmax, st = self._scan_arrays(states, scans)
        B = len(self.members)
        order = np.fromiter((bool(m.obstacle_order) for m in self.members), np.int32, B)
        n = np.zeros(B, np.int32)
        args = (self._handle, iptr(n_beams), dptr(allr), dptr(lo), dptr(hi), dptr(rmax), dptr(st), float(eps), int(min_samples), iptr(order), iptr(n))
        if track is not None:
            self._call("fleet_upload_scans_tracked", *args, float(track[0]), int(track[1]))
        else:
            self._call("fleet_upload_scans", *args)
        return n

    def _check_track(self, gate, window):
        """what track=True needs of the library and of its two parameters, checked before any library call"""
        if not self._has("has_fleet_lidar_tracked"):
            raise RuntimeError("the loaded solver library has no box tracker (rda_fleet_upload_scans_tracked, rda_fleet_rollout_lidar_tracked, "
                               "rda_fleet_track_boxes, rda_fleet_box_tracks, rda_fleet_reset_tracks)")
        if not float(gate) > 0 or int(window) != window or not 1 <= int(window) <= 8:
            raise ValueError(f"track_gate > 0 and 1 <= track_window <= 8, got {gate!r}, {window!r}")

    def track_boxes(self, boxes, gate=1.0, window=8):
        """the tracker alone (rda_fleet_track_boxes; `lidar.track_boxes` per member, bit for bit): `boxes[i]` is member i's (n_i, 4, 2) corner array of
        this tick; the members' tables advance by one tick and nothing is staged.  Returns the list of (n_i, 2) velocities."""
        self._check_track(gate, window)
        B = len(self.members)
        if boxes is None or len(boxes) != B:
            raise ValueError("Fleet.track_boxes: one box array per member")
        arrs = [f64(b).reshape(-1, 4, 2) for b in boxes]
        n = np.fromiter((len(a) for a in arrs), np.int32, B)
        cap = max(1, int(n.max()))
        allb, vel = np.zeros((B, cap, 4, 2)), np.zeros((B, cap, 2))
        for i, a in enumerate(arrs):
            allb[i, :len(a)] = a
        self._call("fleet_track_boxes", self._handle, iptr(n), dptr(allb), cap, float(gate), int(window), dptr(vel))
        return [vel[i, :n[i]].copy() for i in range(B)]

    def box_tracks(self):
        """every member's tracks as the last tracked call left them (rda_fleet_box_tracks): a list of dicts with `centres` (n_i, 2), `velocities`
        (n_i, 2) and `age` (n_i,), the entries of the track's history; track k belongs to box k of that call"""
        self._check_track(1.0, 1)
        B, cap = len(self.members), 256
        n, c, v, age = np.zeros(B, np.int32), np.zeros((B, cap, 2)), np.zeros((B, cap, 2)), np.zeros((B, cap), np.int32)
        self._call("fleet_box_tracks", self._handle, cap, iptr(n), dptr(c), dptr(v), iptr(age))
        return [dict(centres=c[i, :n[i]].copy(), velocities=v[i, :n[i]].copy(), age=age[i, :n[i]].copy()) for i in range(B)]

    def reset_tracks(self, which=None):
        """the members `which` (indices; default: all) lose their tracks (rda_fleet_reset_tracks): after a gap in the ticks, or a jump of the robot"""
        self._check_track(1.0, 1)
        w = None if which is None else np.ascontiguousarray(list(which), np.int32)
        self._call("fleet_reset_tracks", self._handle, iptr(w), 0 if w is None else len(w))

    def upload_worlds(self, obstacle_lists):
        """every member's WORLD - the true obstacles its simulated lidar sees (`raycast`, `rollout(lidar=)`), apart from the obstacles the planner
        stages - resident on the device (rda_fleet_upload_worlds).  `obstacle_lists[i]`: the objects `control` takes (circles and polygons of up to 8
        vertices, with their velocities); an empty list is an empty world.  A new upload replaces the old worlds."""
        if not self._has("has_fleet_rollout_lidar"):
            raise RuntimeError("the loaded solver library has no world entry points (rda_fleet_upload_worlds)")
        B = len(self.members)
        if obstacle_lists is None or len(obstacle_lists) != B:
            raise ValueError("Fleet.upload_worlds: one obstacle list per member")
        every = [o for ol in obstacle_lists for o in ol]
        if any(o.cone_type not in ("norm2", "Rpositive") for o in every):
            raise ValueError("Fleet.upload_worlds: a world holds circles (norm2) and polygons (Rpositive)")
        we = max([3] + [np.asarray(o.vertex).shape[1] for o in every if o.cone_type == "Rpositive"])
        if we > WORLD_EMAX:
            raise ValueError(f"Fleet.upload_worlds: a world polygon may have at most {WORLD_EMAX} vertices")
        scene = RDA_solver._flatten_scene_numpy(SimpleNamespace(max_edge_num=we), every)
        if scene is None or scene[0] != len(every):
            raise ValueError("Fleet.upload_worlds: an obstacle cannot be expressed as a circle or a polygon with a velocity")
        counts = np.fromiter((len(ol) for ol in obstacle_lists), np.int32, B)
        self._call("fleet_upload_worlds", self._handle, iptr(counts), int(we), *map(c_arg, scene_arrays(scene)))

    def raycast(self, states, sensors):
        """every member's lidar scan of its resident world (`upload_worlds`) from `states[i]`, ray-cast on the device by one launch
        (rda_fleet_raycast; `World.get_lidar_scan` is the specification).  `sensors[i]`: a mapping or object with `number`, `angle_min`, `angle_max`,
        `range_min`, `range_max` (`World.lidar` has them).  Returns one scan dict per member in the ir-sim layout of `World.get_lidar_scan`, which
        `control(scans=)` takes as it is.  The members do not see each other here: `raycast_peers` is the scan with see_peers, what
        `rollout(lidar=, see_peers=True)` casts per tick."""
        return self._raycast(states, sensors, False)

    def raycast_peers(self, states, sensors):
        """`raycast` with see_peers: every member's scan also ends on the other members' footprints at `states` (rda_fleet_raycast_peers, one
        launch of lidar::k_raycast_fleet_peers).  The specification is `World.get_lidar_scan` on the member's world followed by
        `scenarios.peer_footprints(cars, states, i)`: polygons, a member never sees itself, an empty world (`upload_worlds` with an empty list) sees
        only the others.  Polygon robots only.  The scans go into `control(scans=)` like any other: a seen member reaches the planner as standing
        boxes, like every lidar obstacle."""
        return self._raycast(states, sensors, True)

    def _check_see_peers(self):
        """what see_peers needs of the library and of every member, checked before any library call"""
        if not self._has("has_fleet_lidar_peers"):
            raise RuntimeError("the loaded solver library has no lidar that sees the other members (rda_fleet_raycast_peers, rda_fleet_rollout_lidar_peers)")
        if any(m.car_tuple.cone_type == "norm2" for m in self.members):
            raise RuntimeError("see_peers casts against the members' footprints as polygons; a circle (norm2) robot is not supported")

    def _raycast(self, states, sensors, see_peers):
        if not self._has("has_fleet_rollout_lidar"):
            raise RuntimeError("the loaded solver library has no ray caster (rda_fleet_raycast)")
        if see_peers:
            self._check_see_peers()
        B = len(self.members)
        nb, lo, hi, rmin, rmax = sensor_arrays(sensors, B)
        if len(states) != B:
            raise ValueError("Fleet.raycast: one state per member")
        st = states_array(states, B)
        ranges = np.zeros(max(int(nb.sum()), 1))
        cast, name = (self.api.fleet_raycast_peers, "rda_fleet_raycast_peers") if see_peers else (self.api.fleet_raycast, "rda_fleet_raycast")
        rc = cast(self._handle, iptr(nb), dptr(lo), dptr(hi), dptr(rmin), dptr(rmax), dptr(st), dptr(ranges))
        if rc < 0:
            raise RuntimeError(f"{name} failed with code {rc} (worlds are uploaded with Fleet.upload_worlds)")
        cut = np.concatenate([[0], np.cumsum(nb)])
        return [{"ranges": ranges[cut[i]:cut[i + 1]].copy(), "angle_min": lo[i], "angle_max": hi[i], "range_min": rmin[i], "range_max": rmax[i],
                 "angle_increment": (hi[i] - lo[i]) / max(int(nb[i]) - 1, 1)} for i in range(B)]

    def sync(self):
        self._call("fleet_sync", self._handle)

    def rollout(self, states, ref_speeds, steps, resort=True, **kwargs):
        """`steps` closed-loop ticks of every member on the device with ONE host wait (rda_fleet_rollout): per tick what `control` does with the
        obstacles the members have staged (scenes that do not move; resort: re-sorted about every robot on every tick like `obstacle_order=True`),
        then every member's first control applied to its kinematic model and `MPC.control`'s arrival rule (`goal_index_threshold`; zero control from
        the arrival tick on).  kwargs: `threshold`, `ind_range` of `closest_point`.  Returns a dict: `states` (steps+1, B, 3) with row 0 the input,
        `controls` (steps, B, 2) as applied, `index` and `iters` (steps, B), `arrived_at` (B,) the arrival tick or -1.  Afterwards every member's
        `state`, `cur_index` and nominal controls are those of the last tick, so `control` continues the loop; the solver state of a member that has
        arrived (it keeps being stepped where it stands) is only good for `reset`.
        Further kwargs: `obstacle_lists=` stages every member's scene first as `control` does (the positions of tick 0; not needed when the scenes are
        already staged).  `moving=True` (rda_fleet_rollout_moving): scenes whose obstacles move are taken - between two ticks every obstacle is put
        forward by its velocity on the device, position at tick k = position at tick 0 + velocity * (dt * k), and the per-stage slots are rebuilt
        (`resort=False`: in the staged order, for members with `obstacle_order=False`).  The caller's obstacle objects are NOT modified: to go on with
        `control` afterwards the caller advances them by `steps * dt`.  `clearance=True` (with `moving=True`, polygon robots) adds `"clearance"`
        (steps, B): every member's clearance after each tick against all obstacles of its scene, `scenarios.clearance` evaluated on the device.
        Without `moving` a scene that moves is refused as before.
        `lidar=sensors` (rda_fleet_rollout_lidar): the members plan against what a simulated lidar sees instead of resident scenes.  `sensors[i]` is
        the sensor of `raycast`; `world=obstacle_lists` uploads the members' worlds first (`upload_worlds`; not needed when they are resident).  Per tick
        every member's world is ray-cast from its pose on the device, the scan is clustered, boxed and staged as `control(scans=)` does (`scan_eps`,
        `scan_min_samples`, the member's `obstacle_order`) with one short wait for the B box counts, then the tick runs as above.  `moving=True` puts
        the WORLD forward between ticks by the rule above, `clearance=True` logs the clearance against the world (the true obstacles, not the boxes;
        no `moving` needed).  The result has `"boxes"` (steps, B) as well: the boxes every member saw.  `resort` and `obstacle_lists` do not apply.
        `see_peers=True` (with `lidar=`; rda_fleet_rollout_lidar_peers): the members see each other in the simulated lidar.  Every tick's ray cast
        also ends on the other members' footprints at the poses of that tick (`raycast_peers`; `scenarios.peer_footprints` is the specification),
        at no extra launch; members that have arrived stand and are still seen.  A seen member reaches the planner as standing boxes, like every
        lidar obstacle, unless `track=True` estimates its velocity.  The result has `"peer_clearance"` (steps, B) as well, every member's separation from the
        nearest other member after each tick (`scenarios.peer_clearance`; negative = overlap), while `clearance=True` stays the clearance against
        the world.  Polygon robots only (a circle robot: RuntimeError); without `lidar=` it is a ValueError.  This is perception, not staging:
        `peers=` with `lidar=` stays refused.
        `track=True` (with `lidar=`; rda_fleet_rollout_lidar_tracked; `track_gate`, `track_window` as in `control`): every tick's boxes are tracked
        on the device behind the scan (one launch more per tick, no wait more) and staged with their tracks' velocities, so what the lidar sees is
        predicted over the horizon - a crossing obstacle, and with `see_peers=True` another member, is anticipated instead of met as a standing
        box.  The tracks continue those the fleet holds (`reset_tracks`, `reset`).  Without `lidar=` it is a ValueError.
        `scan_split=tol` (with `lidar=`; rda_fleet_set_scan_split): every tick's clusters are cut into their straight runs, one box per run, as in
        `control(scans=, scan_split=)`; combines with `track`, `see_peers` and `moving`.  Without `lidar=` it is a ValueError; omitted: off.
        `peers=True` (rda_fleet_rollout_peers): the members avoid each other as in `control(peers=True)`.  Before every tick the device rewrites the
        peer obstacles of every member's scene from the states of that tick and the controls applied on the tick before (tick 0: every member's
        `cur_vel_array[:, 0]`), re-sorts, and runs the tick of `moving=True` on the member's own obstacles.  `obstacle_lists=` is required on the first
        call and optional once such scenes are resident.  The result always has `"peer_clearance"` (steps, B): every member's separation from the
        nearest other member after each tick (`scenarios.peer_clearance`; negative = overlap); `clearance=True` keeps its meaning (own obstacles
        only).  `resort` does not apply, `lidar=` / `scans=` cannot be combined with it, and it has the refusals of `control(peers=True)`.
        `peers="plan"` (rda_fleet_rollout_peers_plan): as `control(peers="plan")` - tick 0 predicts every member along the plan this fleet holds of
        it (if it counts), every later tick along the plan its solve of the tick before left on the device, while it has not arrived.  Returns what
        `peers=True` returns; the same number of launches per tick.
        `gears=True` (rda_fleet_rollout_gears): members with `enable_reverse=True` are taken, plain members may be mixed in (one piece, gear +1).
        Every member's `curve_list` is uploaded, and the device does what `MPC._piece` / `_end` do between two ticks: at the end of a piece that
        another one follows the member goes on with the next piece from its index 0 at `gear * ref_speed` (`ref_speeds` unsigned, as for `control`),
        at the end of the last piece it arrives.  `moving`, `clearance`, `resort` and `obstacle_lists` keep their meaning; `peers`, `lidar` and
        `scans` cannot be combined with it.  The result has `"piece"` (steps, B) as well, the piece in force during each tick, and `index` counts
        within that piece.  Afterwards `curve_index` / `cur_index` are as `_end` leaves them and every piece's last waypoint carries the heading the
        device gave it (Q12), so `control` continues on the right piece.  Without `gears=True` such members are refused."""
        o = self._rollout_options(resort, kwargs)
        ms, B, K = self.members, len(self.members), int(steps)
        if np.isscalar(ref_speeds):
            ref_speeds = [ref_speeds] * B
        st, speed, cur, piece0, nom_u = self._gather_gears(states, ref_speeds) if o.gears else self._gather(states, ref_speeds)
        if o.world is not None:
            self.upload_worlds(o.world)
        ctl0 = f64([np.asarray(m.cur_vel_array, float)[:, 0] for m in ms], (B, 2)) if o.peers else None
        if o.peers and o.obstacle_lists is not None:
            self._stage_peers(o.obstacle_lists, st, ctl0, o.plan)
        elif o.obstacle_lists is not None:
            self._peers_staged = False
            if not self._stage_all(o.obstacle_lists, st):
                for i, m in enumerate(ms):
                    m._stage_obstacles(o.obstacle_lists[i])
        n, infos = max(K, 0), (Info * (max(K, 1) * B))()
        log = {"states": np.zeros((n + 1, B, 3)), "controls": np.zeros((n, B, 2)), "index": np.zeros((n, B), np.int32),
               "iters": np.zeros((n, B), np.int32), "arrived_at": np.zeros(B, np.int32)}
        more = (("clearance", o.clearance, float), ("boxes", o.sensors is not None, np.int32), ("peer_clearance", o.peers or o.see_peers, float),
                ("piece", o.gears, np.int32))
        log.update({name: np.zeros((n, B), kind) for name, asked, kind in more if asked})       # the logs the options add, under their result names
        if o.sensors is not None:
            self.set_scan_split(o.split)
        order = np.fromiter((bool(m.obstacle_order) for m in ms), np.int32, B)
        values = dict(o._asdict(), F=self._handle, K=K, states=st, speed=speed, cur=cur, piece0=piece0, nom_u=nom_u, ctl0=ctl0, order=order,
                      plans=self._plan_state(), logs=(log["states"], log["controls"], log["index"], infos, log["arrived_at"]), box_log=log.get("boxes"),
                      clearance_log=log.get("clearance"), peer_log=log.get("peer_clearance"), piece_log=log.get("piece"))
        self._call(o.entry, *rollout_args(o.entry, values))
        return self._rollout_done(o, K, log, infos)

    def _rollout_options(self, resort, kwargs):
        """`rollout`'s `resort` and keyword arguments as one `RolloutOptions`.  Every refusal that needs no library call happens here, in its order,
        before anything is allocated and before any member is touched."""
        ms = self.members
        kwargs = dict(kwargs)
        with_lidar, with_scans = kwargs.get("lidar") is not None, kwargs.get("scans") is not None      # scans= is only ever refused
        split = scan_split_arg(kwargs, "Fleet.rollout", with_lidar, "lidar=")
        if split:
            self._check_split()
        gears = bool(kwargs.pop("gears", False))
        peers, plan = peers_mode(kwargs.pop("peers", False))
        see_peers = bool(kwargs.pop("see_peers", False))
        track, track_gate, track_window = bool(kwargs.pop("track", False)), kwargs.pop("track_gate", 1.0), kwargs.pop("track_window", 8)
        if track and not with_lidar:
            raise ValueError("Fleet.rollout: track=True tracks the boxes of lidar=")
        if track:
            self._check_track(track_gate, track_window)
            track_gate, track_window = float(track_gate), int(track_window)
        if gears and (peers or with_lidar or with_scans):
            raise ValueError("Fleet.rollout: gears=True cannot be combined with peers / lidar= / scans=")
        if peers and (with_lidar or with_scans):
            raise ValueError("Fleet.rollout: peers=True cannot be combined with lidar= / scans=")
        if see_peers and not with_lidar:
            raise ValueError("Fleet.rollout: see_peers=True belongs to lidar= (members that avoid each other through staged scenes: peers=True)")
        if peers:
            self._check_peers({k: v for k, v in kwargs.items() if k in ("threshold", "ind_range")}, plan)
            if kwargs.get("obstacle_lists") is None and not getattr(self, "_peers_staged", False):
                raise ValueError("Fleet.rollout: peers=True needs obstacle_lists= until such scenes are resident")
        obstacle_lists, clearance = kwargs.pop("obstacle_lists", None), bool(kwargs.pop("clearance", False))
        moving = bool(kwargs.pop("moving", False)) or peers           # (the peers rollout is a moving rollout)
        lidar, world = kwargs.pop("lidar", None), kwargs.pop("world", None)
        scan_eps, scan_min_samples = float(kwargs.pop("scan_eps", 2.0)), int(kwargs.pop("scan_min_samples", 6))
        sensors = None
        if lidar is None and world is not None:
            raise ValueError("Fleet.rollout: world= belongs to lidar=")
        if lidar is not None:
            if obstacle_lists is not None:
                raise ValueError("Fleet.rollout: pass either obstacle_lists= or lidar= (with world=), not both")
            sensors = sensor_arrays(lidar, len(ms))
            if not (scan_eps > 0) or scan_min_samples < 1:
                raise ValueError("Fleet.rollout: scan_eps > 0 and scan_min_samples >= 1")
            if not self._has("has_fleet_rollout_lidar") or any(m.rda_obstacle for m in ms):
                raise RuntimeError("Fleet.rollout(lidar=...) needs the lidar rollout (rda_fleet_rollout_lidar); there is no host fallback")
            if see_peers:
                self._check_see_peers()
        # what is left beyond threshold and ind_range (scans= among it) is refused by the members
        if (not gears and any(m.enable_reverse for m in ms)) or not all(m._tracks(kwargs) for m in ms):
            raise RuntimeError("Fleet.rollout needs device-side tracking on every member and enable_reverse=False (or gears=True); there is no host fallback")
        if gears and not self._has("has_fleet_rollout_gears"):
            raise RuntimeError("the loaded solver library has no rollout over gear pieces (rda_fleet_rollout_gears)")
        if not self._has("has_fleet_rollout"):
            raise RuntimeError("the loaded solver library has no fleet rollout entry point (rda_fleet_rollout)")
        if moving and not self._has("has_fleet_rollout_moving"):
            raise RuntimeError("the loaded solver library has no rollout for moving scenes (rda_fleet_rollout_moving)")
        if clearance and not moving and lidar is None:
            raise ValueError("Fleet.rollout: clearance=True needs moving=True (the clearance log belongs to rda_fleet_rollout_moving)")
        if clearance and any(m.car_tuple.cone_type == "norm2" for m in ms):
            raise RuntimeError("Fleet.rollout: the clearance log is for polygon robots; a circle (norm2) robot is not supported")
        if obstacle_lists is not None and len(obstacle_lists) != len(ms):
            raise ValueError("Fleet.rollout: one obstacle list per member")
        margins = {int(m.goal_index_threshold) for m in ms}
        if len(margins) != 1:
            raise ValueError("Fleet.rollout: the members must share one goal_index_threshold")
        o = RolloutOptions(resort=bool(resort), gears=gears, peers=peers, plan=plan, see_peers=see_peers, track=track, track_gate=track_gate,
                           track_window=track_window, split=split, moving=moving, clearance=clearance, sensors=sensors, scan_eps=scan_eps,
                           scan_min_samples=scan_min_samples, obstacle_lists=obstacle_lists, world=world, threshold=float(kwargs.get("threshold", 0.1)),
                           ind_range=int(kwargs.get("ind_range", 10)), margin=margins.pop(), entry=None)
        return o._replace(entry=rollout_entry(o))

    def _rollout_done(self, o, K, log, infos):
        """after the rollout's entry has returned: what the last tick left on the device into the members, so `control` continues the loop; returns
        `rollout`'s result, which is `log` with the `iters` of `infos`"""
        ms = self.members
        B, T, arrived = len(ms), ms[0].receding, log["arrived_at"]
        eh = np.zeros(B)
        self._call("fleet_rollout_last", self._handle, dptr(self._out_u), dptr(eh))
        if self._has("has_fleet_peers_plan"):        # the plans the last tick left: what a peers="plan" tick that continues predicts along
            plans, valid = self._plan_state()
            self._call("fleet_rollout_last_plan", self._handle, dptr(plans))
            valid[:] = arrived < 0
        if o.gears:
            self._scatter_gears(log["piece"][K - 1], log["index"][K - 1], arrived)
        for i, m in enumerate(ms):
            path = m.ref_path
            m.state = log["states"][K, i].reshape(3, 1).copy()
            if not o.gears:
                m.cur_index = int(log["index"][K - 1, i])
                path[-1][2, 0] = eh[i]                     # quirk Q12: the device rewrote the last waypoint's heading in its copy
                if m._dev_path_key is not None and m._dev_path_key[0] is path:
                    m._dev_path_key[1][-1] = path[-1].tobytes()
            if arrived[i] >= 0:                            # like _end: the robot stands, the next solve starts from zero controls
                m.cur_vel_array = np.zeros((2, T))
                m._dev_u = None
            else:                                          # the device holds the controls of the last solve
                m.cur_vel_array = m._dev_u = self._out_u[i].copy()
        log["iters"][:] = np.array([infos[j].iters for j in range(K * B)], np.int32).reshape(K, B)
        return log

    def clearance(self, states):
        """(B,) every member's clearance at `states[i]` against ALL obstacles of the scene it has staged, as they stand on the device
        (rda_fleet_clearance: `scenarios.clearance` for polygon robots, one launch; negative = overlap, +inf without a staged scene)"""
        if not self._has("has_fleet_rollout_moving"):
            raise RuntimeError("the loaded solver library has no clearance entry point (rda_fleet_clearance)")
        if any(m.car_tuple.cone_type == "norm2" for m in self.members):
            raise RuntimeError("Fleet.clearance is for polygon robots; a circle (norm2) robot is not supported")
        st, out = states_array(states, len(self.members)), np.zeros(len(self.members))
        self._call("fleet_clearance", self._handle, dptr(st), dptr(out))
        return out

    def _gather(self, states, ref_speeds):
        """what a device-tracked tick takes from the members, before anything is staged: every member's piece of its path chosen (`_piece`) and
        brought to the device (`_sync_path`); returns the states (B, 3), the signed speeds (B,), `cur_index` (B,), the pieces, and the nominal
        controls (B, 2, T) - None while the device still holds every member's"""
        B, T = len(self.members), self.members[0].receding
        st, speed, cur = np.zeros((B, 3)), np.zeros(B), np.zeros(B, np.int32)
        pieces, resident = [], True
        for i, m in enumerate(self.members):
            cur_ref_path, gear = m._piece(states[i])
            m._sync_path(cur_ref_path)
            st[i] = np.asarray(m.state, float).ravel()[0:3]
            speed[i], cur[i] = gear * ref_speeds[i], m.cur_index
            resident = resident and m._nominal_u() is None
            pieces.append(cur_ref_path)
        return st, speed, cur, pieces, self._nominal_all(resident)

    def _nominal_all(self, resident):
        """the nominal controls (B, 2, T) of a device-tracked tick; None when the device still holds every member's (`resident`)"""
        if resident:
            return None
        T = self.members[0].receding
        for i, m in enumerate(self.members):        # some member's cur_vel_array was replaced since its last solve: send them all
            self._in_u[i] = f64(m.cur_vel_array, (2, T))
        return self._in_u

    @staticmethod
    def _gear_pieces(m):
        """a member's pieces as `MPC._piece` indexes them; a plain member is one piece with gear +1"""
        return m.curve_list if m.enable_reverse else [m.ref_path]

    def _gather_gears(self, states, ref_speeds):
        """`_gather` for `rollout(gears=True)`: ALL pieces of every member's path to the device (rda_upload_path_pieces); returns the states (B, 3),
        the UNSIGNED speeds (B,), `cur_index` (B,), the pieces in force `curve_index` (B,), and the nominal controls as `_gather` does"""
        B = len(self.members)
        st, speed, cur, piece0 = np.zeros((B, 3)), np.zeros(B), np.zeros(B, np.int32), np.zeros(B, np.int32)
        resident = True
        for i, m in enumerate(self.members):
            m._take_state(states[i])
            pieces = self._gear_pieces(m)
            piece0[i] = m.curve_index if m.enable_reverse else 0
            if piece0[i] >= len(pieces):
                raise RuntimeError(f"Fleet.rollout: member {i} is past the last piece of its path (it has arrived); update_ref_path or reset starts it again")
            m.rda.upload_path_pieces(pieces)
            st[i] = np.asarray(m.state, float).ravel()[0:3]
            speed[i], cur[i] = ref_speeds[i], m.cur_index
            resident = resident and m._nominal_u() is None
        return st, speed, cur, piece0, self._nominal_all(resident)

    def _scatter_gears(self, last_piece, last_index, arrived):
        """after a gear rollout: the headings the device gave the last waypoint of every piece (Q12) into the members' paths, and `curve_index` /
        `cur_index` as `_end` leaves them - past the last piece after arrival, index 0 of the new piece when the last tick changed it, else the last tick's
        `min_index` (`last_piece`, `last_index`: the piece in force during the last tick and its `min_index`).  The rda_upload_path copy has not seen the rewrites: the next `control` uploads again."""
        ms = self.members
        B = len(ms)
        piece, heads = np.zeros(B, np.int32), np.zeros(sum(len(self._gear_pieces(m)) for m in ms))
        self._call("fleet_rollout_last_pieces", self._handle, iptr(piece), dptr(heads))
        at = 0
        for i, m in enumerate(ms):
            pieces = self._gear_pieces(m)
            for p, pts in enumerate(pieces):
                pts[-1][2, 0] = heads[at + p]
            at += len(pieces)
            m._dev_path_key = None
            m.cur_index = int(last_index[i])
            if m.enable_reverse and arrived[i] >= 0:
                m.curve_index, m.cur_index = len(pieces), 0
            elif m.enable_reverse:
                m.curve_index = int(piece[i])
                if piece[i] != last_piece[i]:
                    m.cur_index = 0

    def _control_tracked(self, states, ref_speeds, obstacle_lists, start, threshold=0.1, ind_range=10, stage=None):
        """the same with every member's pre_process on the device (rda_fleet_step_tracked): per ego only the state, the
        signed speed and the path index travel"""
        B, T = len(self.members), self.members[0].receding
        st, speed, cur, pieces, nom_u = self._gather(states, ref_speeds)
        if stage is not None:
            stage(st)
        elif not self._stage_all(obstacle_lists, st):
            for i, m in enumerate(self.members):
                m._stage_obstacles(obstacle_lists[i])
        mi, eh = np.zeros(B, np.int32), np.zeros(B)
        self._call("fleet_step_tracked", self._handle, dptr(st), dptr(speed), iptr(cur), float(threshold), int(ind_range),
                   dptr(nom_u), dptr(self._out_u), dptr(self._out_s), self._info, dptr(self._ref), iptr(mi), dptr(eh))
        out = []
        for i, m in enumerate(self.members):
            ref_own = self._ref[i].copy()
            u, info = self._member_done(i, start, [ref_own[:, j:j + 1] for j in range(T + 1)])
            out.append(m._tracked_done(pieces[i], u, info, int(mi[i]), float(eh[i])))
            self._note_plan(i, self._out_s[i], info["arrive"])
        return out
