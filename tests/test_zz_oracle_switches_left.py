"""Sorts last on purpose: after every other test of the run the oracle's switches are the defaults again - a test that changed one outside
`oracle_backend.switches(...)`, or did not put it back, is found here instead of in whatever runs after it."""
import ctypes as C

import pytest


@pytest.mark.parametrize("run", ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])          # the last test of `-m "not gpu"` and of `-m gpu`; uses no GPU
def test_no_test_left_an_oracle_switch_changed(orc, run):
    from oracle.oracle_backend import Switches
    now, init = Switches(), Switches()
    orc.get_switches(C.byref(now))
    orc.switches_init(C.byref(init))
    for field, _ in Switches._fields_:
        a, b = getattr(now, field), getattr(init, field)
        a, b = (list(a), list(b)) if hasattr(a, "__len__") else (a, b)
        assert a == b, f"orc_switches::{field} was left at {a} (default {b})"
