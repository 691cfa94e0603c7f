"""The oracle's process-wide switches are ONE record (orc_switches, oracle/rda_oracle.h): its defaults against rda_opts_init, every orc_set_*
against the fields it owns, and the context manager the tests change the oracle through (oracle/oracle_backend.py switches)."""
import ctypes as C

import pytest

from oracle.oracle_backend import Switches, api, switches

FIELDS = [f for f, _ in Switches._fields_]
# (shared field, oracle default, rda_opts default) where orc_switches_init and rda_opts_init disagree: none
DEFAULTS_THAT_DIFFER = ()


def plain(rec):
    """{field: number or tuple} of a ctypes record"""
    return {f: (tuple(v) if hasattr(v, "__len__") else v) for f, v in ((f, getattr(rec, f)) for f, _ in rec._fields_)}


def defaults():
    w = Switches()
    api().switches_init(C.byref(w))
    return plain(w)


def current():
    w = Switches()
    api().get_switches(C.byref(w))
    return plain(w)


def test_defaults_equal_rda_opts_init_in_every_shared_field():
    """what orc_switches shares by name with rda_opts (include/rda_hip.h) starts from the same value on both sides; rda_opts_init is host code
    of librda_hip.so and needs no device"""
    from rda_planner_amd import _lib
    from rda_planner_amd._capi import CApi, Opts
    o = Opts()
    CApi(C.CDLL(_lib.build()), "rda").opts_init(C.byref(o))
    hip, orc = plain(o), defaults()
    shared = [f for f in FIELDS if f in hip]
    assert shared == FIELDS[:FIELDS.index("lmz_ipm_tol")] and len(shared) == 19          # everything but the oracle's own three
    assert [(f, orc[f], hip[f]) for f in shared if orc[f] != hip[f]] == list(DEFAULTS_THAT_DIFFER)
    assert (orc["lmz_ipm_tol"], orc["su_trace"], orc["threads"]) == (1e-8, 0, 1)


def test_the_record_in_use_starts_from_the_defaults_and_put_stores_it_as_given():
    orc, was = api(), current()
    with switches():
        w = Switches()
        orc.switches_init(C.byref(w))
        orc.put_switches(C.byref(w))
        assert current() == defaults()
        w.su_cold_probe, w.lmz_mode, w.threads = 0, 7, -3          # no clamps on this way in
        w.su_tol[0] = -1.0
        orc.put_switches(C.byref(w))
        assert current() == plain(w)
    assert current() == was


# setter -> (arguments, the fields it must change and their new values); every other field keeps its value
SETTERS = {
    "set_su_warm":          ((0.5, 0.25, 7), dict(su_warm=(0.5, 0.25), su_warm_cap=7)),
    "set_su_warm_endgame":  ((0.9, 0.1), dict(su_warm_endgame=(0.9, 0.1))),
    "set_su_warm_clip":     ((0.2,), dict(su_warm_clip=0.2)),
    "set_su_easy":          ((1.0, 2.0, 3.0, 4.0, 5.0, 6), dict(su_easy=(1.0, 2.0, 3.0, 4.0, 5.0), su_easy_max=6)),
    "set_su_tol":           ((1e-3, 1e-4, 1e-5), dict(su_tol=(1e-3, 1e-4, 1e-5))),
    "set_su_tol_early":     ((1e-6, 1e-7, 1e-8), dict(su_tol_early=(1e-6, 1e-7, 1e-8))),
    "set_su_hard_warm":     ((0.0, 0.0), dict(su_hard_warm=(0.0, 0.0))),
    "set_su_cold_from":     ((3, 5), dict(su_cold_from=3, su_cold_probe=5)),
    "set_su_first_attempt": ((1,), dict(su_first_attempt=1)),
    "set_su_accept":        ((2,), dict(su_accept=2)),
    "set_su_land":          ((0,), dict(su_land=0)),
    "set_su_land_tol":      ((1e-2, 1e-2, 1e-2), dict(su_land_tol=(1e-2, 1e-2, 1e-2))),
    "set_lmz_mode":         ((1,), dict(lmz_mode=1)),
    "set_centre":           ((0,), dict(tie_centre=0)),
    "set_lmz_ipm_mu":       ((1e-3,), dict(lmz_mu=1e-3)),
    "set_lmz_ipm_tol":      ((1e-5,), dict(lmz_ipm_tol=1e-5)),
    "set_su_trace":         ((1,), dict(su_trace=1)),
    "set_threads":          ((5,), dict(threads=5)),
}


def test_every_setter_but_the_dump_file_is_covered():
    from oracle.oracle_backend import ORC_PROTOTYPES
    assert {n for n in ORC_PROTOTYPES if n.startswith("set_")} == set(SETTERS) | {"set_su_dump"}
    owned = [f for _, change in SETTERS.values() for f in change]
    assert sorted(owned) == sorted(set(FIELDS) - {"su_warm_first"})          # each field has exactly one setter; su_warm_first has none


@pytest.mark.parametrize("name", sorted(SETTERS))
def test_a_setter_changes_exactly_its_fields(name):
    args, change = SETTERS[name]
    with switches() as orc:
        before = current()
        assert all(before[f] != v for f, v in change.items()), "the case must move every field it names"
        getattr(orc, name)(*args)
        assert current() == dict(before, **change)
    assert current() == before


def test_the_setters_keep_their_clamps():
    with switches() as orc:
        was = current()
        for bad in ((0.0, 1e-4, 1e-5), (1e-3, -1.0, 1e-5), (1e-3, 1e-4, 0.0)):          # a non-positive entry: the call is ignored
            orc.set_su_tol(*bad); orc.set_su_land_tol(*bad)
            assert current() == was
        orc.set_lmz_ipm_tol(0.0); orc.set_lmz_ipm_tol(-1e-8)
        assert current() == was
        orc.set_su_cold_from(0, 0)
        assert (current()["su_cold_from"], current()["su_cold_probe"]) == (0, 1)
        orc.set_su_cold_from(4, -2)
        assert (current()["su_cold_from"], current()["su_cold_probe"]) == (4, 1)
        orc.set_lmz_mode(5)
        assert current()["lmz_mode"] == 1
        orc.set_lmz_mode(0)
        assert current()["lmz_mode"] == 0
        orc.set_su_first_attempt(3)
        assert current()["su_first_attempt"] == 1
        orc.set_threads(0)
        assert current()["threads"] == 1
    assert current() == was


def test_switches_applies_restores_and_nests():
    was = current()
    with switches(su_tol=(1e-6, 1e-7, 1e-8), lmz_mode=1) as orc:
        assert orc is api()
        outer = current()
        assert outer == dict(was, su_tol=(1e-6, 1e-7, 1e-8), lmz_mode=1)
        with switches(lmz_mode=0, threads=4):
            assert current() == dict(outer, lmz_mode=0, threads=4)
            orc.set_su_land(1 - was["su_land"])                      # a setter called inside a block is undone with it
        assert current() == outer
    assert current() == was


def test_switches_decorates_a_function_for_the_length_of_each_call():
    was = current()

    @switches(lmz_mu=0.0)
    def inside():
        return current()
    assert current() == was
    for _ in range(2):
        assert inside() == dict(was, lmz_mu=0.0)
        assert current() == was


def test_switches_restores_when_the_block_raises():
    was = current()
    with pytest.raises(ZeroDivisionError):
        with switches(su_warm=(0.0, 0.0), su_warm_cap=0):
            assert current()["su_warm"] == (0.0, 0.0)
            1 / 0
    assert current() == was


def test_switches_refuses_an_unknown_name_a_wrong_length_and_a_fraction_for_an_integer():
    was = current()
    with pytest.raises(TypeError):
        with switches(su_tolerance=(1e-9, 1e-10, 1e-11)):
            pass
    with pytest.raises(ValueError):
        with switches(su_tol=(1e-9, 1e-10)):
            pass
    with pytest.raises(ValueError):
        with switches(threads=1.5):
            pass
    assert current() == was


def test_su_dump_records_inside_the_block_only(tmp_path):
    import numpy as np
    from oracle.oracle_backend import oracle_backend, su_dump
    from rda_planner_amd import scenarios as sc
    from rda_planner_amd.rda_solver import RDA_solver
    s = RDA_solver(5, sc.rectangle_robot(), 4, 2, iter_num=2, time_print=False, _backend=oracle_backend)
    T = 5
    nom_s = np.zeros((3, T + 1)); nom_s[0] = 0.4 * np.arange(T + 1)
    step = lambda: s.iterative_solve(nom_s, np.vstack([np.full(T, 4.0), np.zeros(T)]), [nom_s[:, j:j + 1] for j in range(T + 1)], 4.0, [])      # noqa: E731
    path = tmp_path / "su.bin"
    with su_dump(path):
        step()
    size = path.stat().st_size
    assert size > 0
    step()
    assert path.stat().st_size == size
