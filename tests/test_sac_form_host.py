"""CPU suite: the SAC step-form decision (ilswiss_amd/csrc/sac_form.h) and the switch table (ilswiss_amd/csrc/switches.h), compiled for the host
(tests/harness/sac_form_host.cpp).  The one window-level and the one step-level predicate are held, over every combination of their inputs,
against the three predicates they replaced (restated literally in the harness); the switch accessors against a stub environment."""
import ctypes as C
import itertools
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE, COL, BROKEN, SPLIT, NO_PHASE, NO_FUSE, FITS, HEADS, OWN, DEFER = (1 << i for i in range(10))   # sac_form_host.cpp IN_*
VALUES = (None, b"", b"0", b"1", b"12")


def _build():
    d = tempfile.mkdtemp(prefix="sfh_")
    so = os.path.join(d, "libsfh.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-comment",
                           os.path.join(ROOT, "tests", "harness", "sac_form_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    for name, res, args in (("sfh_decide", None, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]), ("sfh_form_compares", C.c_int, [C.c_int]),
                            ("sfh_setenv", None, [C.c_char_p, C.c_char_p]), ("sfh_parse", C.c_int, [C.c_int, C.c_char_p, C.c_int]),
                            ("sfh_switch", C.c_int, [C.c_char_p])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


@pytest.fixture(scope="module")
def lib():
    return _build()


def switch_rows():
    """(name, rule, default, lifetime) of every row of the table in switches.h"""
    text = open(os.path.join(ROOT, "ilswiss_amd", "csrc", "switches.h")).read()
    rows = re.findall(r'^\s*X\((ILSX_[A-Z0-9_]+),\s*(\w+),\s*(-?\d+),\s*(\w+),\s*"[^"]+"\)', text, flags=re.M)
    assert len(rows) >= 20
    return [(n, r, int(d), l) for n, r, d, l in rows]


def test_one_predicate_equals_the_three_it_replaced(lib):
    out = (C.c_int * 14)()
    n = 0
    for cs, xcd, bits in itertools.product((1, 4), (0, 3), range(1 << 10)):
        lib.sfh_decide(cs, xcd, bits, out)
        window, w_fits, w_heads, step, s_fits, s_heads, n_own, fuse, defer, phase, own_rows, old_ok, old_possible, old_window = out
        key = (cs, xcd, bits)
        assert window == old_window and step == old_ok, key            # the restatement: sac_window_may_use_phase, sac_phase_ok
        assert old_window == (old_possible and not bits & BROKEN and not bits & COL and cs > 1 and xcd == 0), key
        assert not step or window, key                                   # step => window
        assert step == (window and bool(bits & DEFER)), key              # step <=> window and the window's deferred tail
        # the device question and the dry pass are asked only when everything before them holds, the dry pass last, each at most once
        cheap = not bits & (NO_PHASE | BROKEN | WIDE | COL) and cs > 1 and xcd == 0
        assert (w_fits, w_heads) == (int(cheap), int(cheap and bool(bits & FITS))), key
        asked = cheap and bool(bits & DEFER)                             # a step outside a deferred window asks nothing
        assert (s_fits, s_heads) == (int(asked), int(asked and bool(bits & FITS))), key
        # the form
        assert phase == step and defer == bool(bits & DEFER), key
        assert fuse == (not bits & NO_FUSE and not bits & SPLIT), key
        assert n_own == int(step) and own_rows == (step and bool(bits & OWN)), key
        n += 1
    assert n == 4096


def test_forms_compare_field_by_field(lib):
    assert lib.sfh_form_compares(-1) == 1
    for k in range(8):
        assert lib.sfh_form_compares(k) == 1, k


def _expected(rule, dflt, v):
    atoi = 0 if not v else int(v)
    return {"PRESENT": int(v is not None), "UNLESS0": int(v is None or atoi != 0), "INT": dflt if v is None else atoi}[rule]


def test_parse_rules(lib):
    for v in VALUES:
        assert lib.sfh_parse(0, v, 7) == int(v is not None), v
        assert lib.sfh_parse(1, v, 7) == {None: 1, b"": 0, b"0": 0, b"1": 1, b"12": 1}[v], v
        assert lib.sfh_parse(2, v, 7) == {None: 7, b"": 0, b"0": 0, b"1": 1, b"12": 12}[v], v
    assert lib.sfh_parse(2, b"-3", 7) == -3 and lib.sfh_parse(1, b"off", 7) == 0
    assert lib.sfh_switch(b"ILSX_NOT_A_SWITCH") == -12345


def test_every_row_reads_its_variable_by_its_rule_and_keeps_it_as_long_as_its_lifetime_says():
    lib = _build()   # a library of its own: the PROCESS accessors of this copy have not been called yet
    rows = switch_rows()
    assert {r for _, r, _, _ in rows} == {"PRESENT", "UNLESS0", "INT"} and {l for _, _, _, l in rows} == {"PROCESS", "CONTEXT", "OBJECT", "CALL"}
    for i, (name, rule, dflt, life) in enumerate(rows):
        if life == "PROCESS":   # first read under one value, then the variable changes: not seen
            first = VALUES[i % len(VALUES)]
            lib.sfh_setenv(name.encode(), first)
            assert lib.sfh_switch(name.encode()) == _expected(rule, dflt, first), (name, first)
            for v in VALUES:
                lib.sfh_setenv(name.encode(), v)
                assert lib.sfh_switch(name.encode()) == _expected(rule, dflt, first), (name, first, v)
        else:                   # read at every call of the accessor (the caller keeps a CONTEXT / OBJECT value)
            for v in VALUES + (None,):
                lib.sfh_setenv(name.encode(), v)
                assert lib.sfh_switch(name.encode()) == _expected(rule, dflt, v), (name, v)
    # a variable is nobody else's: setting one row's name changes no other row
    lib.sfh_setenv(b"ILSX_NO_PHASE", b"1")
    assert lib.sfh_switch(b"ILSX_NO_PHASE") == 1 and lib.sfh_switch(b"ILSX_SPLIT_NO_PHASE") == 0 and lib.sfh_switch(b"ILSX_SPLIT_PHASE") == 0
