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


# the arguments (the handle is argument 0) through which an entry hands results back
OUTPUTS = {"step": (10, 11, 12), "step_scene": (12, 13, 14), "step_tracked": (7, 8, 9, 11, 12, 13), "tracked_finish": (1, 2, 3, 5, 6, 7),
           "fetch_result": (2, 3, 4), "scan_boxes": (9, 10, 12), "upload_scan": (10,), "timing_launches": (2, 4)}
TIMING = ("timing_reset", "timing_launches")


def fixed_output(position, shape, dtype=float):
    """what `Recorder` writes through the output pointer at argument `position`: an int32 array is all 2, a double array counts up in eighths from
    `position`"""
    import numpy as np
    if np.dtype(dtype) == np.int32:
        return np.full(shape, 2, np.int32)
    return (position + np.arange(int(np.prod(shape))) / 8.0).reshape(shape)


class Recorder:
    """stands for a backend of `RDA_solver` (`_backend=lambda cfg, G, h: recorder`): it answers the capability flags it is given, records every call
    of the binding as (entry name, arguments after the handle) with scalars as they are, numpy copies of the input arrays and "out" for an output,
    writes `fixed_output` and `info` through the output pointers, and returns `fail[entry]` (default 0).  Calls through `.lib.rda_<entry>` are
    recorded alike; the timing entries exist only with `timing`, and rda_last_nonconvex answers `nonconvex`."""
    INFO = dict(resi_dual=0.125, resi_pri=0.0625, iters=2, su_status=0, su_ipm_iters=7, lmz_fail=0)

    def __init__(self, fail=None, timing=True, nonconvex=0, info=None, **flags):
        from rda_planner_amd._capi import CApi
        self.calls, self.fail, self.timing, self.nonconvex, self.prefix = [], dict(fail or {}), timing, nonconvex, "rda"
        self.info = dict(self.INFO, **(info or {}))
        self.api, self.handle, self.lib = self, C.c_void_p(77), _RecorderLib(self)
        self.failed = types.MethodType(CApi.failed, self)                 # the product's text
        self.__dict__.update(flags)

    def __getattr__(self, name):
        if name.startswith(("has_", "_")):
            raise AttributeError(name)
        return lambda *args: self.entry(name, *args)

    def names(self):
        return [name for name, _ in self.calls]

    def entry(self, name, *args):
        import numpy as np
        assert args and args[0] is self.handle, f"{name}: the handle comes first"
        seen = []
        for pos, a in enumerate(args[1:], 1):
            out = pos in OUTPUTS.get(name, ())
            if a is None or isinstance(a, (int, float)):
                assert not isinstance(a, bool), f"{name}: argument {pos} is a bool"
                seen.append(a)
            elif isinstance(a, C._Pointer) and hasattr(a, "_arr"):        # dptr / iptr of a numpy array
                arr = a._arr
                assert arr.flags.c_contiguous and arr.dtype == {C.c_double: np.float64, C.c_int: np.int32}[a._type_], f"{name}: argument {pos}"
                if out:
                    arr[...] = fixed_output(pos, arr.shape, arr.dtype)
                seen.append("out" if out else arr.copy())
            elif isinstance(a, C._Pointer):                               # a cast pointer to a C int that is an output
                assert out, f"{name}: argument {pos}"
                a[0] = 2
                seen.append("out")
            else:                                                         # byref(Info)
                assert out, f"{name}: argument {pos}"
                for k, v in self.info.items():
                    setattr(a._obj, k, v)
                seen.append("out")
        self.calls.append((name, seen))
        return self.nonconvex if name == "last_nonconvex" else self.fail.get(name, 0)


class _RecorderLib:
    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        entry = name[4:]
        if not name.startswith("rda_") or (entry in TIMING and not self._rec.timing):
            raise AttributeError(name)
        return lambda *args: self._rec.entry(entry, *args)


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
