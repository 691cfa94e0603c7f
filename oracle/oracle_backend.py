"""ORACLE backend (test infrastructure only): lets tests run the host-side `RDA_solver` / `MPC`
classes on top of oracle/librda_oracle.so instead of the HIP library.

    solver = RDA_solver(..., _backend=oracle_backend)
"""
import ctypes as C

from rda_planner_amd._capi import CApi, CODES, declare
from rda_planner_amd.rda_solver import _Backend
from . import oracle_lib

_api = None

ORC_CODES = dict(CODES, L=C.POINTER(C.c_long))      # long *
# what oracle/rda_oracle.h declares beyond the shared C-ABI (rda_planner_amd/_capi.py PROTOTYPES, which CApi applies): name without prefix ->
# "<return> <parameters>"; tests/test_capi_symbols.py holds it against the header
ORC_PROTOTYPES = {
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


def oracle_backend(cfg, G, h):
    return _Backend(api(), cfg, G, h)
