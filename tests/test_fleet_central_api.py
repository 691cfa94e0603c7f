"""Fleets of members in the interior-point LamMuZ mode (`lmz_central`): what can be checked without a GPU - rda_fleet_lammuz_kernel is declared, exported
and bound, the header and rda_strerror state the new rules, and the Python constructor names them when the library refuses a fleet."""
import ctypes as C
import re
import types

import pytest

from capi_lib import RDA_ERR_UNSUPPORTED, header, lib


def test_fleet_lammuz_kernel_is_declared_exported_and_bound():
    from rda_planner_amd._capi import CApi
    assert re.search(r"\bconst\s+char\s*\*\s*rda_fleet_lammuz_kernel\s*\(\s*rda_fleet\s*\*\s*\w*\s*\)\s*;", header())
    so = lib()
    assert hasattr(so, "rda_fleet_lammuz_kernel")
    api = CApi(so, "rda")
    fn = api.fleet_lammuz_kernel
    assert list(fn.argtypes) == [C.c_void_p] and fn.restype is C.c_char_p
    assert fn(None) == b""                                  # a null fleet has no launches (no device needed)


def test_header_and_strerror_state_the_rules():
    doc = " ".join(header(comments=True).split())
    assert "ALL members or NONE" in doc and "lmz_mu may differ per member" in doc and "norm2 (circle) robot is refused" in doc
    from rda_planner_amd._capi import CApi
    msg = CApi(lib(), "rda").strerror(RDA_ERR_UNSUPPORTED).decode()
    assert "norm2 robot" in msg and "mixed LamMuZ modes in a fleet" in msg and "interior-point mode in a fleet" not in msg


class _Refusing:
    """stands for the library binding: it has the fleet entry points and refuses every fleet"""
    has_fleet = True

    def __init__(self):
        self.calls = []

    def fleet_create(self, arr, B, out):
        self.calls.append(B)
        return RDA_ERR_UNSUPPORTED

    def fleet_destroy(self, handle):
        raise AssertionError("nothing was created")


def test_constructor_names_the_rules_when_a_fleet_is_refused():
    from rda_planner_amd.fleet import Fleet
    api = _Refusing()
    members = [types.SimpleNamespace(rda=types.SimpleNamespace(_be=types.SimpleNamespace(api=api, handle=C.c_void_p(i + 1))), receding=5) for i in range(2)]
    with pytest.raises(RuntimeError) as e:
        Fleet(members)
    text = str(e.value)
    assert api.calls == [2] and f"code {RDA_ERR_UNSUPPORTED}" in text
    assert "T, N, E, R, iter_num" in text and "all members or none use lmz_central" in text and "circle (norm2) robot" in text
    assert "lmz_central" in Fleet.__init__.__doc__ and "norm2" in Fleet.__init__.__doc__
