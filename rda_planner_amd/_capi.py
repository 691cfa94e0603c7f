"""ctypes view of the C-ABI declared in include/rda_hip.h.

The binding class is parametrised by the symbol prefix: the product instantiates it on
`librda_hip.so` (symbols `rda_*`); the test suite re-uses it on its CPU checker, which
deliberately shares struct layouts and argument order (symbols `orc_*`).

Every prototype is one line of `PROTOTYPES`; tests/test_capi_symbols.py holds the table against
the header, so a new entry point is a header prototype plus one line here.
"""
import ctypes as C
import numpy as np

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)


class Cfg(C.Structure):
    _fields_ = [("T", C.c_int), ("N", C.c_int), ("E", C.c_int), ("R", C.c_int),
                ("dynamics", C.c_int), ("accelerated", C.c_int), ("iter_num", C.c_int),
                ("robot_norm2", C.c_int),
                ("dt", C.c_double), ("L", C.c_double),
                ("max_speed", C.c_double * 2), ("acce_bound", C.c_double * 2),
                ("iter_threshold", C.c_double), ("ws", C.c_double), ("wu", C.c_double),
                ("slack_gain", C.c_double), ("max_sd", C.c_double), ("min_sd", C.c_double),
                ("ro1", C.c_double), ("ro2", C.c_double),
                ("delta", C.c_double), ("eps_u", C.c_double)]


class Opts(C.Structure):
    """rda_opts of include/rda_hip.h: per-handle solver options that are not reference arguments (filled by rda_opts_init)"""
    _fields_ = [("lmz_mode", C.c_int), ("tie_centre", C.c_int), ("lmz_mu", C.c_double), ("su_tol", C.c_double * 3), ("su_tol_early", C.c_double * 3), ("su_hard_warm", C.c_double * 2),
                ("lmz_warm", C.c_int), ("lmz_rows", C.c_int), ("lmz_dense_from", C.c_int), ("lmz_split", C.c_int),
                ("lmz_ip_rows", C.c_int), ("lmz_ip_warm", C.c_int), ("su_pre", C.c_int), ("su_light", C.c_int),
                ("su_warm_first", C.c_int), ("su_warm_cap", C.c_int), ("su_easy_max", C.c_int), ("su_easy_nopred", C.c_int),
                ("su_cold_from", C.c_int), ("su_cold_probe", C.c_int), ("zero_copy", C.c_int), ("early_finish", C.c_int),
                ("fuse_track", C.c_int), ("su_prof", C.c_int), ("su_split", C.c_int), ("duals_follow", C.c_int), ("su_accept", C.c_int), ("su_first_attempt", C.c_int),
                ("su_warm", C.c_double * 2), ("su_warm_endgame", C.c_double * 2), ("su_warm_clip", C.c_double),
                ("su_easy", C.c_double * 5), ("su_land", C.c_int), ("su_land_tol", C.c_double * 3), ("su_land_rho", C.c_double), ("su_land_first", C.c_int), ("su_land_blind_from", C.c_int)]


class Info(C.Structure):
    _fields_ = [("resi_dual", C.c_double), ("resi_pri", C.c_double), ("iters", C.c_int),
                ("su_status", C.c_int), ("su_ipm_iters", C.c_int), ("lmz_fail", C.c_int)]


DYNAMICS = {"acker": 0, "diff": 1, "omni": 2}

# one letter per C type of a prototype; `v` and `s` also serve as return types
CODES = {"v": None, "i": C.c_int, "d": C.c_double, "s": C.c_char_p,
         "D": c_double_p,                   # [const] double *
         "I": c_int_p,                      # [const] int32_t *, int *
         "Q": C.POINTER(C.c_longlong),      # long long *
         "h": C.c_void_p,                   # rda_handle *, rda_fleet *, [const] void *
         "H": C.POINTER(C.c_void_p),        # rda_handle **, rda_fleet **, rda_handle *const *
         "C": C.POINTER(Cfg), "O": C.POINTER(Opts), "N": C.POINTER(Info)}

# name without prefix -> "<return> <parameters>", in the order of include/rda_hip.h
PROTOTYPES = {
    "opts_init":            "v O",
    "create":               "i CDDH",
    "create_opts":          "i CODDH",
    "destroy":              "v h",
    "set_adjust":           "i hddddd",
    "reset":                "i h",
    "strerror":             "s i",
    "device_count":         "i",
    "set_device":           "i i",
    "step":                 "i hDDDdiDDIiDDN",
    "upload_scene":         "i hiIIDDDiI",
    "step_scene":           "i hDDDdiIIDDDiDDN",
    "get_obstacles":        "i hDDII",
    "debug_scene_geom":     "i hDI",
    "debug_scene_vel":      "i hDI",
    "upload_obstacles":     "i hiDDIi",
    "upload_trace":         "i hiDDDD",
    "enqueue_step":         "i hi",
    "enqueue_range":        "i hii",
    "sync":                 "i h",
    "fetch_result":         "i hiDDN",
    "timing_reset":         "i hi",
    "timing_read":          "i hiDI",
    "timing_launches":      "i hiDiI",
    "lammuz_kernel":        "s h",
    "last_nonconvex":       "i h",
    "upload_path":          "i hiD",
    "upload_path_pieces":   "i hiIDD",
    "step_tracked":         "i hDdidiDDDNDDID",
    "tracked_begin":        "i hDdidiD",
    "upload_scene_async":   "i hiIIDDDi",
    "tracked_finish":       "i hDDNDDID",
    "scene_resort":         "i hD",
    "scan_boxes":           "i hiDdddDdiIDiI",
    "upload_scan":          "i hiDdddDdiiI",
    "fleet_create":         "i HiH",
    "fleet_destroy":        "v h",
    "fleet_size":           "i h",
    "fleet_lammuz_kernel":  "s h",
    "fleet_step":           "i hDDDDDDN",
    "fleet_upload_scenes":  "i hIIIDDDI",
    "fleet_step_tracked":   "i hDDIdiDDDNDID",
    "fleet_scene_resort":   "i hDi",
    "fleet_scan_boxes":     "i hIDDDDDdiIDiI",
    "fleet_upload_scans":   "i hIDDDDDdiII",
    "fleet_rollout":        "i hiDDIdiiiDDDINI",
    "fleet_rollout_last":   "i hDD",
    "fleet_rollout_moving": "i hiDDIdiiiDDDINID",
    "fleet_rollout_gears":  "i hiDDIIdiiiiDDDINIID",
    "fleet_rollout_last_pieces": "i hID",
    "fleet_clearance":      "i hDD",
    "fleet_upload_scenes_peers": "i hIIIDDDD",
    "fleet_scene_resort_peers":  "i hDD",
    "fleet_rollout_peers":  "i hiDDIdiiDDDDINIDD",
    "fleet_upload_scenes_peers_plan": "i hIIIDDDDDI",
    "fleet_scene_resort_peers_plan":  "i hDDDI",
    "fleet_rollout_peers_plan": "i hiDDIdiiDDDDINIDDDI",
    "fleet_rollout_last_plan":  "i hD",
    "fleet_peer_clearance": "i hDD",
    "fleet_upload_worlds":  "i hIiIIDD",
    "fleet_raycast":        "i hIDDDDDD",
    "fleet_rollout_lidar":  "i hiDDIdiiDIDDDDdiIiDDINIID",
    "fleet_raycast_peers":  "i hIDDDDDD",
    "fleet_rollout_lidar_peers": "i hiDDIdiiDIDDDDdiIiDDINIIDD",
    "fleet_upload_scans_tracked": "i hIDDDDDdiIIdi",
    "fleet_rollout_lidar_tracked": "i hiDDIdiiDIDDDDdiIiDDINIIDDidi",
    "fleet_track_boxes":    "i hIDidiD",
    "fleet_box_tracks":     "i hiIDDI",
    "fleet_reset_tracks":   "i hIi",
    "set_scan_split":       "i hd",
    "fleet_set_scan_split": "i hd",
    "debug_fleet_world":    "i hDII",
    "fleet_enqueue_range":  "i hii",
    "fleet_sync":           "i h",
    "get_state":            "i hDDDDDDDD",
    "set_state":            "i hDDDDDDDD",
    "get_su_history":       "i hID",
    "set_su_history":       "i hID",
    "get_su_history_n":     "i hIiD",
    "set_su_history_n":     "i hIiD",
    "lmz_history_doubles":  "i h",
    "get_lmz_history":      "i hDI",
    "set_lmz_history":      "i hDI",
    "debug_su_prof":        "i hQ",
    "debug_su_trace":       "i hQiI",
    "debug_su_land":        "i hI",
    "debug_su_land_n":      "i hIi",
    "debug_flush_supports": "i h",
    "debug_slot_src":       "i hII",
    "debug_worklist":       "i hI",
    "debug_alloc_fail":     "i i",
    "debug_alloc_stats":    "i QQ",
    "shard_config":         "i hii",
    "shard_chunk_doubles":  "i h",
    "shard_get_chunk":      "i hD",
    "shard_set_chunks":     "i hD",
    "shard_unique_id":      "i hh",
    "shard_comm_init":      "i hh",
    "shard_comm_count":     "i h",
    "admm_begin":           "i hDDDd",
    "admm_su":              "i hiI",
    "admm_lammuz":          "i h",
    "admm_finish":          "i hDDN",
    "lammuz_batch":         "i iiiDDIDDDDDDDddiDDDD",
    "su_solve":             "i CDDDdDDDDDDDI",
    "su_solve_opts":        "i CODDDdDDDDDDDI",
    # exported by profiling builds only (-DRDA_LMZ_CLK / -DRDA_LMZ_STATS), not in the header: the caller's buffer as an address
    "debug_lmz_clk":        "i hhi",
    "debug_lmz_stats":      "i hh",
}
PROFILING_ONLY = frozenset(("debug_lmz_clk", "debug_lmz_stats"))


def signature(proto, codes=CODES):
    """(restype, argtypes) of one table entry"""
    ret, _, params = proto.partition(" ")
    return codes[ret], [codes[c] for c in params]


def declare(lib, prefix, table, codes=CODES):
    """set restype and argtypes of every `<prefix>_<name>` of `table` that `lib` exports"""
    for name, proto in table.items():
        fn = getattr(lib, f"{prefix}_{name}", None)
        if fn is not None:
            fn.restype, fn.argtypes = signature(proto, codes)


def _pointer(a, buffer_type, pointer_type):
    """the data of the array `a` as a typed pointer that carries the array along as `_arr`, so the array lives as long as the pointer does.  Taken
    through the array's buffer: half the time of `a.ctypes.data_as`, a dozen times per tick, which pays for the calls the shared step protocol of
    rda_solver.py adds (profiles/solver_py_refactor.txt)"""
    if a is None:
        return None
    try:
        p = C.cast(buffer_type.from_buffer(a), pointer_type)
    except (TypeError, ValueError):                                    # a read-only or non-contiguous array exports no such buffer
        return a.ctypes.data_as(pointer_type)                          # (sets `_arr` itself)
    p._arr = a
    return p


def dptr(a):
    return _pointer(a, C.c_double * 0, c_double_p)


def iptr(a):
    return _pointer(a, C.c_int * 0, c_int_p)


def f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def c_arg(v):
    """a value as the C argument it is passed as: a float64 / int32 array as its pointer, a flag as 0 / 1, anything else (None, int, float, the
    handle, the `Info` array) as it is"""
    if isinstance(v, np.ndarray):
        return {"float64": dptr, "int32": iptr}[v.dtype.name](v)       # an array of any other type is no argument of the library: KeyError
    return int(v) if isinstance(v, (bool, np.bool_)) else v


def set_fields(record, changes, who):
    """`changes` (field=value) written into the ctypes `record`; an array field takes exactly as many values as it has entries, an int field an
    integral value.  who = (the caller the messages start with, the C struct, the header that lists its fields)"""
    caller, struct, header = who
    known = {f[0] for f in record._fields_}
    for k, v in changes.items():
        if k not in known:
            raise TypeError(f"{caller}: unknown {struct} field {k!r} ({header} lists them)")
        cur = getattr(record, k)
        if hasattr(cur, "__len__"):
            v = list(v)
            if len(v) != len(cur):
                raise ValueError(f"{caller}: {k} takes {len(cur)} values, got {len(v)}")
            for i, x in enumerate(v):
                cur[i] = x
        else:
            if isinstance(cur, int) and int(v) != v:
                raise ValueError(f"{caller}: {k} is an integer switch, got {v!r}")
            setattr(record, k, v)
    return record


class CApi:
    """Thin typed wrapper over `<prefix>_*` entry points of a loaded shared library."""

    def __init__(self, lib, prefix):
        self.lib, self.prefix = lib, prefix
        declare(lib, prefix, PROTOTYPES)
        has = lambda name: hasattr(lib, f"{prefix}_{name}")     # noqa: E731
        self.has_opts = has("create_opts")
        self.has_scene = has("step_scene")              # caller-side obstacle pipeline on the device (HIP library only, like all below)
        self.has_scan = has("upload_scan")              # lidar front end on the device
        self.has_track = has("step_tracked")            # caller-side pre_process on the device
        self.has_pipeline = self.has_track and has("tracked_begin")
        self.has_fleet = has("fleet_step")              # batched multi-ego stepping
        self.has_fleet_scenes = has("fleet_upload_scenes")
        self.has_fleet_scans = has("fleet_upload_scans")                    # fleet lidar: every member's scan in one launch
        self.has_fleet_rollout = has("fleet_rollout")                       # K closed-loop ticks on the device, one host wait
        self.has_fleet_rollout_moving = has("fleet_rollout_moving")         # ... for scenes that move
        self.has_fleet_rollout_lidar = has("fleet_rollout_lidar")           # ... around the simulated sensor
        self.has_fleet_rollout_gears = has("fleet_rollout_gears")           # ... over the gear pieces of reverse paths
        self.has_fleet_peers = has("fleet_rollout_peers")                   # members as each other's obstacles, staged on the device
        self.has_fleet_peers_plan = has("fleet_rollout_peers_plan")         # ... predicted along their planned trajectories
        self.has_fleet_lidar_peers = has("fleet_rollout_lidar_peers")       # members that see each other in the simulated lidar
        self.has_fleet_lidar_tracked = has("fleet_rollout_lidar_tracked")   # lidar boxes tracked across ticks, staged with velocities
        self.has_scan_split = has("set_scan_split") and has("fleet_set_scan_split")     # scan clusters cut into straight runs, one box each

    def _f(self, name):
        return getattr(self.lib, f"{self.prefix}_{name}")

    def __getattr__(self, name):
        return self._f(name)

    def failed(self, name, rc):
        """the exception of a refused call: `if rc < 0: raise api.failed("step", rc)`"""
        return RuntimeError(f"{self.prefix}_{name} failed with code {rc}")
