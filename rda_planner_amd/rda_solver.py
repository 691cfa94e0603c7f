"""
`RDA_solver` - drop-in for RDA_planner.rda_solver.RDA_solver (reference rda_solver.py:17-61).

Same constructor / method signatures and `info` keys as the reference class, but every
per-iteration computation (su-problem, the N x T LamMuZ problems, xi/zeta/residual updates)
runs inside `librda_hip.so` on an MI355X through the C-ABI of include/rda_hip.h.  This module
is host glue only: argument checking, obstacle staging into dense arrays
(assign_obstacle_parameter, reference :483-526) and packing of the `info` dict (:603-608).

There is NO CPU fallback: constructing the class without the HIP library or without a GPU
raises.  (Tests inject the CPU oracle through the private `_backend` hook to exercise the
host logic on machines without a GPU; the product never does.)
"""
import time
from math import inf  # noqa: F401  (kept for API parity with the reference module namespace)

import numpy as np

from ._capi import Cfg, Info, Opts, DYNAMICS, dptr, iptr, f64, set_fields
import ctypes as C

CONE_CODE = {"Rpositive": 0, "norm2": 1}


try:                                                     # optional C accelerator of flatten_scene (host glue; see there)
    from . import _flatten
except ImportError:
    _flatten = None


class _Backend:
    """A loaded C-ABI library plus one solver handle."""

    def __init__(self, api, cfg, G, h, opts=None):
        self.api = api
        self.handle = C.c_void_p()
        G = f64(G)
        h = f64(h).ravel()
        if opts is not None:
            rc = api.create_opts(C.byref(cfg), C.byref(opts), dptr(G), dptr(h), C.byref(self.handle))
        else:
            rc = api.create(C.byref(cfg), dptr(G), dptr(h), C.byref(self.handle))
        if rc != 0:
            raise api.failed("create", rc)

    def close(self):
        if self.handle:
            self.api.destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# RDA_* environment switches of the A/B tools and tests (tools/experiments/env_ab.sh, tests/test_gpu_switches.py): applied HERE, by the host
# package, to the rda_opts it hands to rda_create_opts - librda_hip.so itself reads no environment variable (round 5: a library call has no
# process-global configuration).  name -> (fields filled in order from a comma-separated value)
_ENV_SWITCHES = {
    "RDA_LMZ_MODE": ("lmz_mode",), "RDA_TIE_CENTRE": ("tie_centre",), "RDA_LMZ_MU": ("lmz_mu",), "RDA_SU_TOL": ("su_tol",), "RDA_SU_HARD_WARM": ("su_hard_warm",),
    "RDA_SU_TOL_EARLY": ("su_tol_early",), "RDA_LMZ_WARM": ("lmz_warm",), "RDA_LMZ_ROWS": ("lmz_rows",), "RDA_LMZ_DENSE_FROM": ("lmz_dense_from",),
    "RDA_LMZ_SPLIT": ("lmz_split",), "RDA_LMZ_IP_ROWS": ("lmz_ip_rows",), "RDA_LMZ_IP_WARM": ("lmz_ip_warm",), "RDA_SU_PRE": ("su_pre",),
    "RDA_SU_LIGHT": ("su_light",), "RDA_SU_WARM_FIRST": ("su_warm_first",), "RDA_SU_EASY_NOPRED": ("su_easy_nopred",), "RDA_SU_COLD_FROM": ("su_cold_from", "su_cold_probe"),
    "RDA_SU_EASY": ("su_easy", "su_easy_max"), "RDA_SU_WARM_CLIP": ("su_warm_clip",), "RDA_SU_WARM_ENDGAME": ("su_warm_endgame",), "RDA_SU_WARM": ("su_warm", "su_warm_cap"),
    "RDA_ZERO_COPY": ("zero_copy",), "RDA_EARLY_FINISH": ("early_finish",), "RDA_FUSE_TRACK": ("fuse_track",), "RDA_SU_PROF": ("su_prof",), "RDA_SU_SPLIT": ("su_split",),
    "RDA_DUALS_FOLLOW": ("duals_follow",), "RDA_SU_ACCEPT": ("su_accept",), "RDA_SU_LAND": ("su_land",), "RDA_SU_LAND_TOL": ("su_land_tol",), "RDA_SU_LAND_RHO": ("su_land_rho",), "RDA_SU_LAND_FIRST": ("su_land_first",), "RDA_SU_LAND_BLIND_FROM": ("su_land_blind_from",),
}


def _apply_env(o):
    """the RDA_* switches of the A/B tools, applied to an rda_opts.  Only `hip_options()` calls this: a handle created through the C API (rda_create) or from
    a raw `Opts()` + rda_opts_init ignores the environment (the library itself reads none).  A value that is not a number is an error that NAMES the variable
    (the C parser of round 4 ignored such values silently, int(float(v)) alone raised a bare ValueError at every RDA_solver construction)."""
    import os
    for name, fields in _ENV_SWITCHES.items():
        raw = os.environ.get(name)
        if not raw:
            continue
        vals = [v.strip() for v in raw.split(",")]
        for f in fields:                                   # an array field takes as many values as it has entries; what is not given stays
            cur = getattr(o, f)
            n = len(cur) if hasattr(cur, "__len__") else 1
            take, vals = vals[:n], vals[n:]
            for i, v in enumerate(take):
                if v == "":                                # an empty list element: that entry keeps its default
                    continue
                try:
                    x = float(v)
                except ValueError:
                    raise ValueError(f"environment switch {name}={raw!r}: {v!r} is not a number (rda_opts::{f}, include/rda_hip.h)") from None
                if hasattr(cur, "__len__"):
                    cur[i] = x
                elif isinstance(cur, int):
                    setattr(o, f, int(x))
                else:
                    setattr(o, f, x)
    if o.su_cold_probe < 1:
        o.su_cold_probe = 1


def hip_options(**changes):
    """rda_opts with the library defaults, the RDA_* environment switches (`_ENV_SWITCHES`), then `changes` applied (field=value)"""
    from ._lib import hip_api
    o = Opts()
    hip_api().opts_init(C.byref(o))
    _apply_env(o)
    return set_fields(o, changes, ("hip_options", "rda_opts", "include/rda_hip.h"))


def _hip_backend(cfg, G, h, opts=None):
    from ._lib import hip_api          # raises loudly when librda_hip.so / the GPU is missing
    return _Backend(hip_api(), cfg, G, h, opts if opts is not None else hip_options())


def scene_arrays(scene):
    """(kind, nvert, geom, vel) of a flattened scene (`flatten_scene`) in the types the library reads"""
    _, kind, nvert, geom, vel = scene
    return np.ascontiguousarray(kind, np.int32), np.ascontiguousarray(nvert, np.int32), f64(geom), f64(vel)


def step_epilogue(time_print, pack_info, info_c, start, out_u, out_s, ref_states, report=None):
    """what follows every step's library call: the reference's line when the su-problem made no update, the timing printout (`report`, a solver's
    `_timing_report`; a `Fleet` has none for its members), then `pack_info`'s dict.  Returns (out_u, info)."""
    if info_c.su_status and time_print:
        print("No update of state and control vector")            # reference :699
    if report is not None:
        report(info_c, start)
    return out_u, pack_info(ref_states, out_s, info_c, start)


class _StepOut:
    """the buffers a step hands its results back in: `u` (2, T), `s` (3, T+1), `info`; a tracked step also `ref` (3, T+1), the reference the
    device sampled, `mi` the new path index and `eh` the heading of the last waypoint after the tick (quirk Q12)"""

    def __init__(self, T, tracked=False):
        self.u, self.s, self.info = np.zeros((2, T)), np.zeros((3, T + 1)), Info()
        self.args = (dptr(self.u), dptr(self.s), C.byref(self.info))             # the tail of the library's argument list
        if tracked:
            self.ref, self.mi, self.eh = np.zeros((3, T + 1)), np.zeros(1, np.int32), np.zeros(1)
            self.args += (None, dptr(self.ref), iptr(self.mi), dptr(self.eh))


class RDA_solver:
    def __init__(self, receding, car_tuple, max_edge_num=5, max_obs_num=5, iter_num=2, step_time=0.1,
                 iter_threshold=0.2, process_num=4, accelerated=True, time_print=True, **kwargs) -> None:
        """kwargs: slack_gain (8), max_sd (1.0), min_sd (0.1), ro1 (200), ro2 (1), ws (1), wu (1)
        - identical meaning to the reference (rda_solver.py:24-31,196-201,218-219).
        `process_num` is accepted for compatibility and ignored: the obstacle fan-out is the
        GPU grid, not a process pool (reference :55-59,211-214)."""
        self.T = receding
        self.car_tuple = car_tuple
        self.L = car_tuple.wheelbase
        self.max_speed = np.c_[car_tuple.max_speed]
        self.max_obs_num = max_obs_num
        self.max_edge_num = max_edge_num
        self.dynamics = car_tuple.dynamics
        self.iter_num = iter_num
        self.dt = step_time
        self.acce_bound = np.c_[car_tuple.max_acce] * self.dt
        self.iter_threshold = iter_threshold
        self.accelerated = accelerated
        self.process_num = process_num
        self.time_print = time_print
        self.ws = kwargs.get("ws", 1)
        self.wu = kwargs.get("wu", 1)
        self._adjust = {"slack_gain": kwargs.get("slack_gain", 8), "max_sd": kwargs.get("max_sd", 1.0),
                        "min_sd": kwargs.get("min_sd", 0.1), "ro1": kwargs.get("ro1", 200),
                        "ro2": kwargs.get("ro2", 1)}
        if self.dynamics not in DYNAMICS:
            raise ValueError(f"unknown dynamics {self.dynamics!r}")
        if max_obs_num < 1:
            raise ValueError("max_obs_num must be >= 1")

        G = f64(car_tuple.G)
        h = f64(car_tuple.h).ravel()
        cfg = Cfg()
        cfg.T, cfg.N, cfg.E, cfg.R = receding, max_obs_num, max_edge_num, G.shape[0]
        cfg.dynamics = DYNAMICS[self.dynamics]
        cfg.accelerated = int(bool(accelerated))
        cfg.iter_num = iter_num
        cfg.robot_norm2 = int(car_tuple.cone_type == "norm2")
        cfg.dt, cfg.L = step_time, float(self.L) if self.L else 0.0
        cfg.max_speed[0], cfg.max_speed[1] = float(self.max_speed[0, 0]), float(self.max_speed[1, 0])
        cfg.acce_bound[0], cfg.acce_bound[1] = float(self.acce_bound[0, 0]), float(self.acce_bound[1, 0])
        cfg.iter_threshold = iter_threshold
        cfg.ws, cfg.wu = self.ws, self.wu
        for k, v in self._adjust.items():
            setattr(cfg, k, float(v))
        cfg.delta = kwargs.get("tie_margin", 1e-6)
        cfg.eps_u = kwargs.get("tie_control", 1e-8)
        self._cfg = cfg
        make = kwargs.get("_backend", _hip_backend)
        # LamMuZ solver (not a reference argument): None / 0 = support enumeration with the tie-breaks of DESIGN.md 2 (default),
        # lmz_central = mu > 0 selects the interior-point kernel that returns the central-path point of the reference's cone
        # program at barrier parameter mu; a norm2 (circle) robot always uses it (default mu 1e-6)
        self.lmz_central = kwargs.get("lmz_central", None)
        opts = kwargs.get("hip_opts", None)            # an rda_opts (see hip_options) for the HIP backend; None = library defaults
        if self.lmz_central and make is _hip_backend:
            # (a copy: the caller's struct may configure a second solver that is not in interior-point mode)
            opts = Opts.from_buffer_copy(opts) if opts is not None else hip_options()
            opts.lmz_mode, opts.lmz_mu = 1, float(self.lmz_central)
        # duals_follow_obstacles=True (NOT reference semantics, opt-in; rda_opts::duals_follow): when the device pipeline re-binds the obstacle
        # slots - a caller that re-sorts its list every tick, obstacle_order=True, the reference's default - the duals move with their
        # obstacles instead of staying with the slot (quirk Q5: the ADMM then never converges within iter_num).  Entry i of the obstacle
        # list must denote the same obstacle from tick to tick; needs the device-side obstacle pipeline (MPC: device_obstacles=True).
        self.duals_follow_obstacles = bool(kwargs.get("duals_follow_obstacles", False))
        if self.duals_follow_obstacles and make is _hip_backend:
            opts = Opts.from_buffer_copy(opts) if opts is not None else hip_options()
            opts.duals_follow = 1
        elif self.duals_follow_obstacles:
            # a test backend keeps the duals with their SLOTS (the reference's semantics): say so rather than hand back other semantics silently
            import warnings
            warnings.warn("duals_follow_obstacles=True is honoured by the HIP backend only; this backend keeps the duals bound to the obstacle slots", RuntimeWarning, stacklevel=2)
        self._be = make(cfg, G, h, opts) if make is _hip_backend else make(cfg, G, h)   # test backends select the mode themselves
        self._R = G.shape[0]
        self.pipeline = True        # MPC overlaps its per-tick obstacle staging with the first su-problem (set False to serialise)

    def _call(self, name, *args):
        """the library's `name(handle, *args)`; a negative return code raises what the binding makes of it"""
        rc = getattr(self._be.api, name)(self._be.handle, *args)
        if rc < 0:
            raise self._be.api.failed(name, rc)
        return rc

    # ---- runtime tunables (reference :426-434, :1055-1056) ------------------------------
    def assign_adjust_parameter(self, **kwargs):
        for k in self._adjust:
            self._adjust[k] = kwargs.get(k, self._adjust[k])
        a = self._adjust
        self._be.api.set_adjust(self._be.handle, float(a["slack_gain"]), float(a["max_sd"]),
                                float(a["min_sd"]), float(a["ro1"]), float(a["ro2"]))

    def get_adjust_parameter(self):
        d = dict(self._adjust)
        d["ws"], d["wu"] = self.ws, self.wu
        return d

    def reset(self):
        """reference :1060-1068 - clears the lam'A / lam'b products only, NOT the duals (Q6)."""
        self._be.api.reset(self._be.handle)

    # ---- obstacle staging (reference assign_obstacle_parameter :483-526) ------------------
    def _stage(self, obstacle_list):
        n = len(obstacle_list)
        N, E, T = self.max_obs_num, self.max_edge_num, self.T
        if 0 < n < N:
            # quirk Q3: the reference pads the CALLER's list in place with copies of the last entry
            obstacle_list += [obstacle_list[-1]] * (N - n)
            n = N
        use = min(n, N)
        if use == 0:
            return 0, None, None, None, 0
        per_t = any(isinstance(o.A, list) for o in obstacle_list[:use])
        nt = T + 1 if per_t else 1
        A = np.zeros((use, nt, E, 2))
        b = np.zeros((use, nt, E))
        cone = np.zeros(use, dtype=np.int32)
        for i in range(use):
            o = obstacle_list[i]
            if isinstance(o.A, list):
                k = np.shape(o.A[0])[0]
                if k > E:
                    raise ValueError(f"obstacle {i} has {k} edges > max_edge_num={E}")
                for t in range(nt):
                    A[i, t, :k] = o.A[t]
                    b[i, t, :k] = np.asarray(o.b[t]).ravel()
            else:
                k = np.shape(o.A)[0]
                if k > E:
                    raise ValueError(f"obstacle {i} has {k} edges > max_edge_num={E}")
                A[i, :, :k] = o.A
                b[i, :, :k] = np.asarray(o.b).ravel()
            cone[i] = 0 if o.cone_type == "Rpositive" else 1
        return use, A, b, cone, int(per_t)

    # ---- caller-side obstacle pipeline on the device ------------------------------------------
    @property
    def has_scene(self):
        """True when the backend converts raw obstacles (vertices / centre+radius / velocity) on the device"""
        return bool(getattr(self._be.api, "has_scene", False))

    def flatten_scene(self, obstacle_list):
        """raw obstacle objects (`.cone_type`, `.vertex` 2xk | `.center`, `.radius`, `.velocity`; the attributes the
        reference's MPC.convert_rda_obstacle reads, mpc.py:192-203) -> flat arrays for rda_upload_scene, or None if
        an object cannot be expressed (then the caller falls back to the host conversion).
        The walk over the objects is done by the C module `_flatten` (csrc/flatten_ext.c, ~10 us for 200 objects) when it is built and
        accepts the input, else by the numpy code below (~150 us): same arrays either way (tests/test_host_api.py)."""
        E = self.max_edge_num
        if _flatten is not None and len(obstacle_list):
            n = len(obstacle_list)
            kind, nvert, geom, vel = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, E, 2)), np.empty((n, 2))
            if _flatten.flatten(obstacle_list, E, kind, nvert, geom, vel) == 0:
                return n, kind, nvert, geom, vel
        return RDA_solver._flatten_scene_numpy(self, obstacle_list)          # (unbound: `self` only needs max_edge_num)

    def _flatten_scene_numpy(self, obstacle_list):
        E = self.max_edge_num
        ct = [o.cone_type for o in obstacle_list]
        n_poly, n_circ = ct.count("Rpositive"), ct.count("norm2")
        if n_poly + n_circ == len(ct):
            objs = obstacle_list
        else:                                                          # other cone types are skipped (mpc.py:196-203)
            objs = [o for o in obstacle_list if o.cone_type in ("norm2", "Rpositive")]
            ct = [o.cone_type for o in objs]
        n = len(objs)
        kind = np.zeros(n, np.int32) if n_circ == 0 else np.array([c == "norm2" for c in ct], np.int32)
        nvert = np.zeros(n, np.int32)
        geom = np.zeros((n, E, 2))
        if n == 0:
            return 0, kind, nvert, geom, np.zeros((0, 2))
        try:                                                           # 2x1 columns (what the reference's obstacles carry): one concatenate
            vel = np.concatenate([o.velocity for o in objs], axis=1, dtype=float)[0:2].T
            if vel.shape != (n, 2):
                raise ValueError
        except (ValueError, TypeError, np.exceptions.AxisError):
            # anything else the reference accepts: it only ever takes np.linalg.norm(velocity) and `velocity * t`
            # (mpc.py:447-456,465-472), so a scalar (the lidar examples pass 0) moves both coordinates alike
            vel = np.empty((n, 2))
            for i, o in enumerate(objs):
                v = np.asarray(o.velocity, float).ravel()
                if v.size == 1:
                    vel[i] = v[0]
                elif v.size >= 2:
                    vel[i] = v[0:2]
                else:
                    return None
        if vel.shape != (n, 2) or not np.all(np.isfinite(vel)):
            return None                                                # host conversion decides (and reports) instead
        circ = np.flatnonzero(kind == 1)
        if circ.size:
            if E < 3:
                return None
            geom[circ, 0, :] = np.asarray([objs[i].center for i in circ], float).reshape(circ.size, -1)[:, 0:2]
            geom[circ, 1, 0] = [float(objs[i].radius) for i in circ]
        poly = np.flatnonzero(kind == 0) if n_circ else None
        if n_poly:
            verts = [o.vertex for o in objs] if poly is None else [objs[i].vertex for i in poly]
            try:
                ks = np.array([v.shape[1] for v in verts], np.int64)
            except AttributeError:                                     # vertices given as nested lists
                ks = np.array([np.shape(v)[1] for v in verts], np.int64)
            if ks.max() > E:
                return None
            # all vertices side by side, then one scatter: vertex j of polygon i -> geom[i, j, :]
            V = np.concatenate(verts, axis=1, dtype=float)[0:2]
            rows = np.repeat(np.arange(n) if poly is None else poly, ks)
            cols = np.arange(V.shape[1]) - np.repeat(np.cumsum(ks) - ks, ks)
            geom[rows, cols, :] = V.T
            if poly is None:
                nvert[:] = ks
            else:
                nvert[poly] = ks
        return n, kind, nvert, geom, np.ascontiguousarray(vel)

    def iterative_solve_scene(self, nom_s, nom_u, ref_states, ref_speed, scene, robot_xy, order, **kwargs):
        """`iterative_solve` fed with a flattened raw scene (see `flatten_scene`): conversion to half-spaces, the
        constant-velocity prediction, distance ordering, truncation and padding all run on the device."""
        start = time.time()
        nominal = self._nominal_args(nom_s, nom_u, ref_states, ref_speed)
        return self._step("step_scene", start, ref_states, *nominal, *self._scene_args(scene, robot_xy, order))

    # ---- the step protocol: every step form is a head of its own, then `_step` or its two halves ---------------------------------------
    def _nominal_args(self, nom_s, nom_u, ref_states, ref_speed):
        """the host's nominal trajectory, reference and speed as the C arguments a step starts with (a pointer of `dptr` keeps its array alive)"""
        T = self.T
        ref = f64(np.hstack(ref_states)[0:3, :], (3, T + 1))
        return dptr(f64(nom_s, (3, T + 1))), dptr(f64(nom_u, (2, T))), dptr(ref), float(ref_speed)

    def _scene_args(self, scene, robot_xy, order):
        """a flattened scene, the robot's position and the ordering flag as the run of C arguments that rda_step_scene, rda_upload_scene and
        rda_upload_scene_async share"""
        kind, nvert, geom, vel = scene_arrays(scene)
        rob = f64(np.asarray(robot_xy, float).ravel()[0:2])
        return int(scene[0]), iptr(kind), iptr(nvert), dptr(geom), dptr(vel), dptr(rob), int(bool(order))

    def _step(self, name, start, ref_states, *args):
        """one step through the library's `name`: timing on, the call with the output buffers behind `args`, the epilogue"""
        out = _StepOut(self.T)
        self._timing_begin()
        self._call(name, *args, *out.args)
        return self._step_done(out.info, start, out.u, out.s, ref_states)

    def _step_done(self, info_c, start, out_u, out_s, ref_states):
        """the epilogue of all five step forms (`step_epilogue` with this solver's timing report)"""
        return step_epilogue(self.time_print, self.pack_info, info_c, start, out_u, out_s, ref_states, self._timing_report)

    def _tracked_head(self, state, ref_speed, cur_index, nom_u, threshold, ind_range):
        """what rda_step_tracked and rda_tracked_begin take from the caller"""
        st = f64(np.asarray(state, float).ravel()[0:3])
        un = f64(nom_u, (2, self.T)) if nom_u is not None else None
        return dptr(st), float(ref_speed), int(cur_index), float(threshold), int(ind_range), dptr(un)

    def _tracked_done(self, out, start):
        """the epilogue of a tracked step: (u, info, new cur_index, heading of the last waypoint after the tick - quirk Q12)"""
        ref_states = [out.ref[:, i:i + 1] for i in range(self.T + 1)]
        return (*self._step_done(out.info, start, out.u, out.s, ref_states), int(out.mi[0]), float(out.eh[0]))

    # ---- staging only (the solve is then issued by a Fleet for all of its members at once) -----------
    def upload_scene(self, scene, robot_xy, order):
        self._call("upload_scene", *self._scene_args(scene, robot_xy, order), None)

    def upload_obstacles(self, obstacle_list):
        n_obs, A, b, cone, per_t = self._stage(obstacle_list)
        self._call("upload_obstacles", n_obs, dptr(A), dptr(b), iptr(cone), per_t)

    def pack_info(self, ref_states, out_s, info_c, start):
        """the `info` dict of the reference (:603-608) plus the solver counters"""
        opt_state_list = [out_s[:, i:i + 1] for i in range(self.T + 1)]      # columns of an array this call owns (no copies)
        if info_c.lmz_fail:
            print("Update Lam Mu Fail")                               # reference :792,825 (printed unconditionally there too)
        last_nonconvex = getattr(self._be.api.lib, "rda_last_nonconvex", None)
        if last_nonconvex is not None:
            bad = last_nonconvex(self._be.handle)                     # polygons of the device-staged scene this step ran on
            if bad > 0:                                               # reference mpc.py:524 (one line per polygon there, with its vertices)
                print(f"Warning: {bad} polygon(s) constructed by vertex are not convex. Please check the vertex")
        return {"ref_traj_list": ref_states, "opt_state_list": opt_state_list,
                "iteration_time": time.time() - start, "resi_dual": info_c.resi_dual,
                "resi_pri": info_c.resi_pri, "iters": info_c.iters, "status": info_c.su_status,
                "su_ipm_iters": info_c.su_ipm_iters, "lmz_fail": info_c.lmz_fail}

    # ---- caller-side pre_process on the device ------------------------------------------------------
    @property
    def has_track(self):
        return bool(getattr(self._be.api, "has_track", False))

    def upload_path(self, ref_path):
        """the polyline of MPC.ref_path (list of (>=3)x1 waypoints) for `iterative_solve_tracked`"""
        P = np.ascontiguousarray(np.hstack(ref_path)[0:3, :].T, dtype=float)
        self._call("upload_path", int(P.shape[0]), dptr(P))

    def upload_path_pieces(self, pieces):
        """all gear pieces of a path (MPC.curve_list: lists of 4x1 waypoints whose last row is the gear; a list of 3x1 waypoints is a piece with
        gear +1) resident at once, for `Fleet.rollout(gears=True)` (rda_upload_path_pieces)"""
        lens = np.fromiter((len(p) for p in pieces), np.int32, len(pieces))
        gear = np.array([float(p[0][3, 0]) if np.shape(p[0])[0] > 3 else 1.0 for p in pieces])
        P = np.ascontiguousarray(np.hstack([w for p in pieces for w in p])[0:3, :].T, dtype=float)
        self._call("upload_path_pieces", len(pieces), iptr(lens), dptr(gear), dptr(P))

    def iterative_solve_tracked(self, state, ref_speed, cur_index, nom_u=None, threshold=0.1, ind_range=10):
        """`iterative_solve` with MPC.pre_process (nominal roll-out, closest waypoint, arc-length reference sampling)
        done on the device from the robot state; obstacles are whatever is staged (upload_scene / upload_obstacles).
        Returns (u, info, new cur_index, heading of the last waypoint after the tick - quirk Q12)."""
        start = time.time()
        head = self._tracked_head(state, ref_speed, cur_index, nom_u, threshold, ind_range)
        out = _StepOut(self.T, tracked=True)
        self._timing_begin()
        self._call("step_tracked", *head, *out.args)
        return self._tracked_done(out, start)

    # ---- the tracked tick in two halves: the first su-problem runs while the caller stages this tick's obstacles ------
    @property
    def has_pipeline(self):
        return self.pipeline and bool(getattr(self._be.api, "has_pipeline", False))

    def tracked_begin(self, state, ref_speed, cur_index, nom_u=None, threshold=0.1, ind_range=10):
        """queue pre_process + the first su-problem of the step (neither reads the obstacles of this tick: the first
        su-problem uses the products of the previous step, reference quirk Q4) and return without waiting"""
        self._tick_start = time.time()
        head = self._tracked_head(state, ref_speed, cur_index, nom_u, threshold, ind_range)
        self._timing_begin()
        self._call("tracked_begin", *head)

    def upload_scene_async(self, scene, robot_xy, order):
        """`upload_scene` inside an open tick: staged on the stream behind the first su-problem, no wait"""
        self._call("upload_scene_async", *self._scene_args(scene, robot_xy, order))

    def scene_resort(self, robot_xy):
        """re-rank the RESIDENT raw scene by distance to `robot_xy` and rebuild the obstacle slots on the device (the reference's per-tick
        `obstacle_list.sort(key=rda_obs_distance)`, mpc.py:205-206) - no host-to-device copy; asynchronous like `upload_scene_async`"""
        rob = f64(np.asarray(robot_xy, float).ravel()[0:2])
        self._call("scene_resort", dptr(rob))

    # ---- lidar front end on the device (rda_scan_boxes / rda_upload_scan; host specification: lidar.py) ---------------------
    @property
    def has_scan(self):
        return bool(getattr(self._be.api, "has_scan", False))

    def _scan_args(self, state, scan_data, eps, min_samples):
        ranges = f64(np.asarray(scan_data["ranges"], float).ravel())
        st = f64(np.asarray(state, float).ravel()[0:3])
        head = (int(ranges.size), dptr(ranges), float(scan_data["angle_min"]), float(scan_data["angle_max"]),
                float(scan_data["range_max"]), dptr(st), float(eps), int(min_samples))
        return head, (ranges, st)                        # (the arrays stay referenced until the call has returned)

    def set_scan_split(self, tol):
        """the split tolerance [m] of this handle's scans (rda_set_scan_split; `lidar.split_runs` is the specification): 0 switches the stage off.
        The library is called only when the value changes; one without the entry point is a RuntimeError as soon as a split is asked for."""
        tol = float(tol)
        if tol == getattr(self, "_scan_split", 0.0):
            return
        if not getattr(self._be.api, "has_scan_split", False):
            raise RuntimeError("the loaded solver library cannot split scan clusters (rda_set_scan_split, rda_fleet_set_scan_split)")
        rc = self._be.api.set_scan_split(self._be.handle, tol)          # (not `_call`: a refused tolerance is the caller's ValueError)
        if rc < 0:
            raise ValueError("scan split: tol must be finite and greater than 0") if rc == -1 else self._be.api.failed("set_scan_split", rc)
        self._scan_split = tol

    def scan_boxes(self, state, scan_data, eps=2.0, min_samples=6, with_labels=False, split=0.0):
        """`lidar.scan_box` on the device: the (n, 4, 2) corners (world frame, counter-clockwise) of one minimum-area rectangle per
        DBSCAN cluster of the scan taken from `state`; with_labels: also the per-beam labels (-2 miss, -1 noise, >= 0 cluster).
        split = tol > 0: `lidar.scan_box_split` - one rectangle per straight run, the labels are segment numbers"""
        self.set_scan_split(split)
        head, keep = self._scan_args(state, scan_data, eps, min_samples)
        cap = max(1, keep[0].size)
        boxes, n, labels = np.zeros((cap, 4, 2)), np.zeros(1, np.int32), np.zeros(cap, np.int32)
        self._call("scan_boxes", *head, iptr(n), dptr(boxes), cap, iptr(labels))
        return (boxes[:n[0]], labels[:keep[0].size]) if with_labels else boxes[:n[0]]

    def upload_scan(self, state, scan_data, eps=2.0, min_samples=6, order=True, split=0.0):
        """the boxes of `scan_boxes` staged as this solver's obstacles without leaving the device (`upload_scene` of them, robot at
        state[0:2]); usable inside an open tick like `upload_scene_async`.  Returns the number of boxes."""
        self.set_scan_split(split)
        head, keep = self._scan_args(state, scan_data, eps, min_samples)
        n = np.zeros(1, np.int32)
        self._call("upload_scan", *head, int(bool(order)), iptr(n))
        return int(n[0])

    def iterative_solve_staged(self, nom_s, nom_u, ref_states, ref_speed):
        """`iterative_solve` on the obstacles that are staged on the device already (`upload_scan`), with the host's nominal
        trajectory and reference: the device-resident step (a trace of one step: rda_upload_trace / rda_enqueue_step, which
        tests/test_gpu_parity.py pins to rda_step)"""
        lib, h = self._be.api.lib, self._be.handle
        start = time.time()
        nom_s, nom_u, ref, _ = self._nominal_args(nom_s, nom_u, ref_states, ref_speed)
        speed, out = f64([float(ref_speed)]), _StepOut(self.T)
        self._timing_begin()
        # (not `_call`: whichever of the four calls refuses, the error is this form's own)
        rc = lib.rda_upload_trace(h, 1, nom_s, nom_u, ref, dptr(speed))
        rc = rc or lib.rda_enqueue_step(h, 0) or lib.rda_sync(h)
        rc = rc or lib.rda_fetch_result(h, 0, *out.args)
        if rc < 0:
            raise RuntimeError(f"{self._be.api.prefix}: the step on the staged obstacles failed with code {rc}")
        return self._step_done(out.info, start, out.u, out.s, ref_states)

    def tracked_finish(self, discard=False):
        """queue the rest of the ADMM loop, wait, return what `iterative_solve_tracked` returns"""
        out = _StepOut(self.T, tracked=True)
        if discard:                                      # the tick is closed for a caller that is reporting an error of its own: whatever the library says
            self._be.api.tracked_finish(self._be.handle, *out.args)
            return None
        self._call("tracked_finish", *out.args)
        return self._tracked_done(out, self._tick_start)

    # ---- the reference's timing printout (rda_solver.py:587-601, `time_print`) ---------------------------------------------
    def _timing_begin(self):
        """per-kernel GPU events for this step (only when time_print is set: the events cost a few microseconds per launch)"""
        lib = self._be.api.lib
        self._timed = bool(self.time_print) and hasattr(lib, "rda_timing_launches")
        if self._timed:
            lib.rda_timing_reset(self._be.handle, 1)

    def _timing_report(self, info_c, start):
        """'iteration i time: ...' for every executed ADMM iteration (GPU time of its su + LamMuZ kernels), 'iteration early
        stop: i' when the residual test of :594 ended the loop, then the total - the lines the reference prints"""
        if not self.time_print:
            return
        if getattr(self, "_timed", False):
            lib, h = self._be.api.lib, self._be.handle
            cap = self.iter_num + 1
            per = []
            for which in (1, 0):                                   # su, LamMuZ launches in launch order
                buf, n = np.zeros(cap), C.c_int(0)
                lib.rda_timing_launches(h, which, dptr(buf), cap, C.cast(C.byref(n), C.POINTER(C.c_int)))
                per.append(buf[:min(n.value, cap)])
            lib.rda_timing_reset(h, 0)
            for i in range(info_c.iters):
                t_i = (per[0][i] if i < per[0].size else 0.0) + (per[1][i] if i < per[1].size else 0.0)
                print("iteration " + str(i) + " time: ", t_i * 1e-3)
        if info_c.resi_dual < self.iter_threshold and info_c.resi_pri < self.iter_threshold:
            print("iteration early stop: " + str(info_c.iters - 1))
        print("-----------------------------------------------")
        print("iteration time:", time.time() - start)
        print("==============================================")

    # ---- one MPC step (reference iterative_solve :573-610) --------------------------------
    def iterative_solve(self, nom_s, nom_u, ref_states, ref_speed, obstacle_list, **kwargs):
        start = time.time()
        nominal = self._nominal_args(nom_s, nom_u, ref_states, ref_speed)
        n_obs, A, b, cone, per_t = self._stage(obstacle_list)
        return self._step("step", start, ref_states, *nominal, n_obs, dptr(A), dptr(b), iptr(cone), per_t)

    # ---- state access for tests -----------------------------------------------------------
    def get_state(self):
        T, N, E, R = self.T, self.max_obs_num, self.max_edge_num, self._R
        st = {"lam": np.zeros((N, T + 1, E)), "mu": np.zeros((N, T + 1, R)), "z": np.zeros((N, T)),
              "xi": np.zeros((N, T + 1, 2)), "zeta": np.zeros((N, T)), "dis": np.zeros(T),
              "a_lam": np.zeros((N, T + 1, 2)), "b_lam": np.zeros((N, T + 1))}
        self._be.api.get_state(self._be.handle, *[dptr(st[k]) for k in
                                                   ("lam", "mu", "z", "xi", "zeta", "dis", "a_lam", "b_lam")])
        return st

    def set_state(self, st):
        arrs = [f64(st[k]) if k in st and st[k] is not None else None
                for k in ("lam", "mu", "z", "xi", "zeta", "dis", "a_lam", "b_lam")]
        self._be.api.set_state(self._be.handle, *[dptr(a) for a in arrs])
