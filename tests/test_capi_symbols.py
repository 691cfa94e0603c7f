"""The built librda_hip.so loads without a GPU and exports every symbol include/rda_hip.h declares."""
import ctypes
import os
import re
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "rda_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rda_[a-z_]+)\s*\(", src)))


def test_header_symbols_exported():
    from rda_planner_amd import _lib
    so = _lib.build()
    lib = ctypes.CDLL(so)
    names = _declared()
    assert len(names) >= 18, names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/rda_hip.h but not exported"


def test_struct_layouts_match_header():
    from rda_planner_amd._capi import Cfg, Info
    assert ctypes.sizeof(Cfg) == 8 * 4 + 16 * 8
    assert ctypes.sizeof(Info) == 2 * 8 + 3 * 4 + 4          # padded to 8


def test_product_path_has_no_oracle_dependency():
    """rda_planner_amd must never import / link the oracle"""
    pkg = os.path.join(ROOT, "rda_planner_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".c")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "librda_oracle" not in text, f


def test_no_device_is_a_loud_error():
    """without a GPU the product refuses to construct a solver instead of falling back"""
    import pytest
    from rda_planner_amd import _lib
    from rda_planner_amd._capi import CApi
    if CApi(ctypes.CDLL(_lib.build()), "rda").device_count() > 0:
        pytest.skip("a GPU is present")
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.rda_solver import RDA_solver
    with pytest.raises(RuntimeError):
        RDA_solver(5, sc.rectangle_robot(), time_print=False)


def test_host_side_helpers_build_and_load():
    """the C caller bench.py times (tools/closed_loop_host.c) and the flatten accelerator of the Python API (csrc/flatten_ext.c) are plain gcc
    builds: they compile, load and expose what their ctypes / import users expect (no GPU needed)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import closed_loop_host as clh
    lib = ctypes.CDLL(clh.build())
    assert hasattr(lib, "closed_loop_run")
    assert ctypes.sizeof(clh.Api) == 5 * 8 and ctypes.sizeof(clh.Scene) == 4 * 4 + 5 * 8        # struct closed_loop_api / closed_loop_scene
    src = open(os.path.join(ROOT, "tools", "closed_loop_host.c")).read()
    assert '#include "../include/rda_hip.h"' in src and "oracle" not in src                     # a caller of the C-ABI and of nothing else
    from rda_planner_amd import _lib
    assert _lib.build_flatten_ext(force=True) is not None
    import importlib
    mod = importlib.import_module("rda_planner_amd._flatten")
    assert callable(mod.flatten)


def test_integration_md_names_every_entry_point_of_the_header():
    """INTEGRATION.md is the map from the C-ABI to the reference interfaces it replaces: no function of include/rda_hip.h may be missing"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = sorted(set(re.findall(r"\b(rda_[a-z0-9_]+)\s*\(", open(os.path.join(root, "include", "rda_hip.h")).read())))
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    assert [n for n in names if n not in doc] == []


def _header_struct_fields(name, header=os.path.join("include", "rda_hip.h")):
    """[(field, 'int' | 'double', length)] of `typedef struct [<name>] { ... } <name>;` in the header, in declaration order"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, header)).read(), flags=re.S)
    body = re.search(r"typedef struct(?: %s)? \{([^{}]*)\} %s;" % (name, name), text).group(1)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(int32_t|int|double)\s+(.*)", decl.strip(), re.S)
        if not m:
            continue
        for item in m.group(2).split(","):
            mm = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*$", item)
            out.append((mm.group(1), "double" if m.group(1) == "double" else "int", int(mm.group(2) or 1)))
    return out


@pytest.mark.parametrize("cname,pyname", [("rda_opts", "Opts"), ("rda_cfg", "Cfg"), ("rda_info", "Info"), ("orc_switches", "Switches")])
def test_ctypes_structs_mirror_the_header_field_by_field(cname, pyname):
    """the ctypes mirrors of the C-ABI structs (rda_planner_amd/_capi.py) against include/rda_hip.h, and the oracle's record of switches
    (oracle/oracle_backend.py) against oracle/rda_oracle.h: names, order, types, array lengths - a field added on one side only shifts
    everything behind it silently"""
    import ctypes as C
    from rda_planner_amd import _capi
    if cname.startswith("orc_"):
        want, mirror = _header_struct_fields(cname, os.path.join("oracle", "rda_oracle.h")), _oracle()
    else:
        want, mirror = _header_struct_fields(cname), _capi
    assert len(want) >= 6
    got = []
    for fname, ftype in getattr(mirror, pyname)._fields_:
        length = getattr(ftype, "_length_", 1)
        base = getattr(ftype, "_type_", ftype) if length > 1 else ftype
        got.append((fname, "int" if base is C.c_int else "double", length))
        assert base in (C.c_int, C.c_double), (fname, base)
    assert got == want


# ---- the prototype tables (rda_planner_amd/_capi.py PROTOTYPES, oracle/oracle_backend.py ORC_PROTOTYPES) against the two headers ----------------
# (function, position, reason) where the table is deliberately looser than the header: none
PROTOTYPE_EXCEPTIONS = ()


def _ctype_rule(prefix):
    """C parameter type (no blanks around '*') -> ctypes, the fixed rule of the C-ABI; the oracle header adds `const char *` and `long *`"""
    import ctypes as C
    from rda_planner_amd import _capi as k
    rule = {"int": C.c_int, "double": C.c_double, "double*": k.c_double_p, "const double*": k.c_double_p,
            "int32_t*": k.c_int_p, "const int32_t*": k.c_int_p, "int*": k.c_int_p, "long long*": C.POINTER(C.c_longlong),
            "void*": C.c_void_p, "const void*": C.c_void_p,
            f"{prefix}_handle*": C.c_void_p, f"{prefix}_fleet*": C.c_void_p,
            f"{prefix}_handle**": C.POINTER(C.c_void_p), f"{prefix}_fleet**": C.POINTER(C.c_void_p), f"{prefix}_handle*const*": C.POINTER(C.c_void_p),
            f"{prefix}_cfg*": C.POINTER(k.Cfg), f"const {prefix}_cfg*": C.POINTER(k.Cfg),
            f"{prefix}_opts*": C.POINTER(k.Opts), f"const {prefix}_opts*": C.POINTER(k.Opts), f"{prefix}_info*": C.POINTER(k.Info)}
    if prefix == "orc":
        sw = C.POINTER(_oracle().Switches)
        rule.update({"const int*": k.c_int_p, "const orc_handle*": C.c_void_p, "const char*": C.c_char_p, "long*": C.POINTER(C.c_long),
                     "orc_switches*": sw, "const orc_switches*": sw})
    return rule


def _header_prototypes(path, prefix):
    """{name without prefix: (restype, [argtypes])} of every prototype of the header; a C type the rule does not know is a KeyError"""
    import ctypes as C
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, path)).read(), flags=re.S)
    rule, ret = _ctype_rule(prefix), {"int": C.c_int, "void": None, "const char *": C.c_char_p}
    out = {}
    for rtype, name, params in re.findall(r"^\s*(int|void|const char \*)\s*%s_(\w+)\s*\(([^()]*)\)\s*;" % prefix, src, re.M):
        args = []
        if params.strip() != "void":
            for p in params.split(","):
                ctype = re.match(r"\s*(.*?)\w+\s*$", p, re.S).group(1)
                args.append(rule[re.sub(r"\s*\*\s*", "*", " ".join(ctype.split()))])
        assert name not in out, name
        out[name] = (ret[rtype], args)
    return out


def _check_against(header, table, codes):
    from rda_planner_amd._capi import signature
    loose = {(f, i) for f, i, _ in PROTOTYPE_EXCEPTIONS}
    for name, (restype, args) in header.items():
        got_ret, got = signature(table[name], codes)
        assert got_ret is restype, name
        assert len(got) == len(args), name
        for i, (a, b) in enumerate(zip(got, args)):
            assert a is b or (name, i) in loose, (name, i, a, b)


def test_prototype_table_equals_the_header():
    """every prototype of include/rda_hip.h has its line in PROTOTYPES with exactly the header's types, and the table has nothing else but the
    two hooks of the profiling builds - a parameter added on one side only shifts everything behind it silently"""
    from rda_planner_amd._capi import CODES, PROFILING_ONLY, PROTOTYPES
    header = _header_prototypes("include/rda_hip.h", "rda")
    assert len(header) >= 85 and set(header) == set(_d[len("rda_"):] for _d in _declared())
    assert set(PROTOTYPES) == set(header) | set(PROFILING_ONLY) and not set(header) & set(PROFILING_ONLY)
    _check_against(header, PROTOTYPES, CODES)
    hip = open(os.path.join(ROOT, "rda_planner_amd", "csrc", "rda_hip.hip")).read()
    defined = set(re.findall(r'extern "C"[\w\s\*]*?\brda_(\w+)\s*\(', hip))
    assert defined - set(header) == set(PROFILING_ONLY)


def _oracle():
    import sys
    sys.path.insert(0, ROOT)
    from oracle import oracle_backend
    return oracle_backend


def test_oracle_tables_equal_the_oracle_header():
    """the same for oracle/rda_oracle.h: what it shares with the C-ABI is checked in PROTOTYPES, the rest in ORC_PROTOTYPES, and the built
    library exports no orc_ function that the header and the tables do not know"""
    import subprocess
    from rda_planner_amd._capi import CODES, PROTOTYPES
    ob = _oracle()
    header = _header_prototypes("oracle/rda_oracle.h", "orc")
    shared = {n: v for n, v in header.items() if n in PROTOTYPES}
    own = {n: v for n, v in header.items() if n not in PROTOTYPES}
    assert len(shared) >= 15 and set(own) == set(ob.ORC_PROTOTYPES)
    _check_against(shared, PROTOTYPES, CODES)
    _check_against(own, ob.ORC_PROTOTYPES, ob.ORC_CODES)
    nm = subprocess.run(["nm", "-D", "--defined-only", ob.oracle_lib.build()], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT orc_(\w+)", nm))
    assert len(exported) >= 45 and exported == set(header)


def test_prototypes_are_applied_to_the_library():
    """CApi sets every table entry the library exports (constructing it touches no device) and derives the capability flags from the symbols"""
    from rda_planner_amd import _lib
    from rda_planner_amd._capi import CApi, PROFILING_ONLY, PROTOTYPES, signature
    api = CApi(ctypes.CDLL(_lib.build()), "rda")
    flags = ("has_opts", "has_scene", "has_scan", "has_track", "has_pipeline", "has_fleet", "has_fleet_scenes", "has_fleet_scans",
             "has_fleet_rollout", "has_fleet_rollout_moving", "has_fleet_rollout_lidar")
    for name, proto in PROTOTYPES.items():
        if name in PROFILING_ONLY and not hasattr(api.lib, "rda_" + name):
            continue
        restype, argtypes = signature(proto)
        fn = getattr(api.lib, "rda_" + name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name
        assert getattr(api, name) is fn
    assert [f for f in flags if getattr(api, f) is not True] == []
    ob = _oracle()
    orc = ob.api()
    assert [f for f in flags[1:] if getattr(orc, f) is not False] == []
    for name, proto in ob.ORC_PROTOTYPES.items():
        restype, argtypes = signature(proto, ob.ORC_CODES)
        fn = getattr(orc.lib, "orc_" + name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name
    assert list(orc.lib.orc_su_solve.argtypes) == signature(PROTOTYPES["su_solve"])[1]


def test_no_prototype_is_declared_outside_the_two_tables():
    """no file of the package, the oracle, the tests or the tools assigns argtypes / restype of a C-ABI function by hand (libraries that are not the
    C-ABI - the row emulator, the C closed loop - keep their own)"""
    allowed = {os.path.join("rda_planner_amd", "_capi.py"), os.path.join("oracle", "oracle_backend.py")}
    other_libraries = ("rip_emu_solve", "closed_loop_")
    assign = re.compile(r"\.(argtypes|restype)\b[^=\n]*=(?!=)")
    strays = []
    for top in ("rda_planner_amd", "oracle", "tests", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            if top == "oracle" and dirpath != os.path.join(ROOT, top):
                continue
            for f in files:
                rel = os.path.relpath(os.path.join(dirpath, f), ROOT)
                if not f.endswith(".py") or rel in allowed:
                    continue
                for n, line in enumerate(open(os.path.join(ROOT, rel), errors="replace"), 1):
                    if assign.search(line) and not any(o in line for o in other_libraries):
                        strays.append(f"{rel}:{n}")
    assert strays == []
