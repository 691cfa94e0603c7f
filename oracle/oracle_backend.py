"""ORACLE backend (test infrastructure only): lets tests run the host-side `RDA_solver` / `MPC`
classes on top of oracle/librda_oracle.so instead of the HIP library.

    solver = RDA_solver(..., _backend=oracle_backend)
"""
import contextlib
import ctypes as C

from rda_planner_amd._capi import CApi, CODES, declare, set_fields
from rda_planner_amd.rda_solver import _Backend
from . import oracle_lib

_api = None



class Switches(C.Structure):
    """orc_switches of oracle/rda_oracle.h: every process-wide switch of the oracle (defaults: orc_switches_init)"""
    _fields_ = [("su_warm", C.c_double * 2), ("su_warm_cap", C.c_int), ("su_warm_first", C.c_int),
                ("su_warm_endgame", C.c_double * 2), ("su_warm_clip", C.c_double), ("su_easy", C.c_double * 5), ("su_easy_max", C.c_int),
                ("su_tol", C.c_double * 3), ("su_tol_early", C.c_double * 3), ("su_hard_warm", C.c_double * 2),
                ("su_cold_from", C.c_int), ("su_cold_probe", C.c_int), ("su_first_attempt", C.c_int), ("su_accept", C.c_int),
                ("su_land", C.c_int), ("su_land_tol", C.c_double * 3), ("lmz_mode", C.c_int), ("tie_centre", C.c_int), ("lmz_mu", C.c_double),
                ("lmz_ipm_tol", C.c_double), ("su_trace", C.c_int), ("threads", C.c_int)]


ORC_CODES = dict(CODES, L=C.POINTER(C.c_long), W=C.POINTER(Switches))      # long *, [const] orc_switches *
# what oracle/rda_oracle.h declares beyond the shared C-ABI (rda_planner_amd/_capi.py PROTOTYPES, which CApi applies): name without prefix ->
# "<return> <parameters>"; tests/test_capi_symbols.py holds it against the header
ORC_PROTOTYPES = {
    "switches_init":        "v W",
    "get_switches":         "v W",
    "put_switches":         "v W",
    "set_threads":          "v i",
    "set_su_dump":          "v s",
    "set_su_trace":         "v i",
    "set_lmz_mode":         "v i",
    "lmz_failures":         "i h",
    "set_lmz_ipm_tol":      "v d",
    "set_lmz_ipm_mu":       "v d",
    "lammuz_ipm_one":       "i iiDDiiDdDDDdddiDDDDI",
    "set_centre":           "v i",
    "lammuz_one":           "i iiDDiDdDDDddddiDDDD",
    "set_su_warm":          "v ddi",
    "set_su_warm_endgame":  "v dd",
    "set_su_warm_clip":     "v d",
    "set_su_easy":          "v dddddi",
    "set_su_hard_warm":     "v dd",
    "set_su_cold_from":     "v ii",
    "set_su_first_attempt": "v i",
    "get_su_ipm_hist":      "v hIi",
    "set_su_tol":           "v ddd",
    "set_su_tol_early":     "v ddd",
    "set_su_accept":        "v i",
    "set_su_land":          "v i",
    "set_su_land_tol":      "v ddd",
    "get_su_land_stats":    "v L",
    "get_su_landed":        "i",
}


def api():
    global _api
    if _api is None:
        lib = oracle_lib.load()
        _api = CApi(lib, "orc")
        declare(lib, "orc", ORC_PROTOTYPES, ORC_CODES)
    return _api


@contextlib.contextmanager
def switches(**changes):
    """The oracle with `changes` (orc_switches field=value) applied for the length of the block; yields the API.  What the block found is
    put back when it ends, normally or by an exception, so blocks nest and no test states a default.  As a decorator (`@switches(...)`) it
    holds for the length of each call."""
    orc = api()
    before = Switches()
    orc.get_switches(C.byref(before))
    now = set_fields(Switches.from_buffer_copy(before), changes, ("switches", "orc_switches", "oracle/rda_oracle.h"))
    orc.put_switches(C.byref(now))
    try:
        yield orc
    finally:
        orc.put_switches(C.byref(before))


@contextlib.contextmanager
def su_dump(path):
    """every su-problem orc_admm_su solves inside the block is recorded in the file `path` (tools/su_replay.py reads it)"""
    api().set_su_dump(str(path).encode())
    try:
        yield
    finally:
        api().set_su_dump(b"")


def oracle_backend(cfg, G, h):
    return _Backend(api(), cfg, G, h)
