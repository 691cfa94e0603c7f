"""What the CPU tests of the C-ABI and of `Fleet`'s refusals share: the header's text, the loaded library, the header's argument lists as ctypes, the rows
of INTEGRATION.md, the return codes, and stand-ins for the binding and for `MPC` members that fail when anything but a refusal uses them."""
import ctypes as C
import os
import re
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDA_ERR_ARG, RDA_ERR_UNSUPPORTED, RDA_ERR_HIP = -1, -2, -3
SENSOR = dict(number=100, angle_min=-1.5, angle_max=1.5, range_min=0.0, range_max=10.0)
LIDAR_FLAGS = dict(has_fleet_rollout=True, has_fleet_rollout_moving=True, has_fleet_rollout_lidar=True, has_fleet_peers=True)      # a library with the lidar rollout


def header(comments=False):
    """include/rda_hip.h, by default without its comments"""
    text = open(os.path.join(ROOT, "include", "rda_hip.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def lib():
    from rda_planner_amd import _lib
    return C.CDLL(_lib.build())


def _header_argtypes(name):
    """the parameter list of the header's `int name(...);` as ctypes"""
    from rda_planner_amd._capi import Info, c_double_p, c_int_p
    kinds = {"rda_fleet *": C.c_void_p, "rda_handle *": C.c_void_p, "const int32_t *": c_int_p, "int32_t *": c_int_p, "const double *": c_double_p,
             "double *": c_double_p, "double": C.c_double, "int": C.c_int, "rda_info *": C.POINTER(Info)}
    args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header(), re.S).group(1)
    return [kinds[" ".join(re.match(r"\s*(.*?)(\w+)\s*$", a.strip(), re.S).group(1).split())] for a in args.split(",")]


header_argtypes = _header_argtypes


def declared(name):
    """the header declares `int name(`"""
    return re.search(r"\bint\s+%s\s*\(" % name, header()) is not None


def integration_rows(name, table=True):
    """the lines of INTEGRATION.md that name the entry point in backquotes (table: only rows of a table)"""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    return [ln for ln in doc.splitlines() if "`%s`" % name in ln and (ln.startswith("|") or not table)]


class Binding:
    """stands for the library binding: it answers the capability flags it is given and fails on any other use"""
    def __init__(self, **flags):
        self.__dict__.update(flags)

    def __getattr__(self, name):
        raise AssertionError(f"library touched: {name}")


def member(tracks=True, reverse=False, **attrs):
    """stands for an `MPC` member: what every refusal of `Fleet.rollout` reads, and `attrs`; using its solver is an error"""
    def no_solver(*a, **k):
        raise AssertionError("member touched")
    return types.SimpleNamespace(enable_reverse=reverse, _tracks=lambda kw: tracks and set(kw) <= {"threshold", "ind_range"}, goal_index_threshold=1,
                                 receding=5, _piece=no_solver, _sync_path=no_solver, **attrs)


def pipeline_member(car=None, order=True, rda_obstacle=False, **kw):
    """`member` with a robot and the device-side obstacle pipeline (car: a robot or anything with `cone_type`)"""
    from rda_planner_amd import scenarios as sc
    return member(car_tuple=car or sc.rectangle_robot(), obstacle_order=order, rda_obstacle=rda_obstacle, device_obstacles=True,
                  rda=types.SimpleNamespace(has_scene=True), **kw)


def bare_fleet(api, members):
    """a `Fleet` that was never constructed: no device, the given binding and members"""
    from rda_planner_amd.fleet import Fleet
    f = Fleet.__new__(Fleet)
    f.api, f._handle, f.members = api, None, members
    return f
