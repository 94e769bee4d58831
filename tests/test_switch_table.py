"""CPU suite: every environment variable libilsx.so reads has a row in the table of INTEGRATION §6, and the table lists no variable
that nothing reads (the "every remaining switch is listed" condition, held by a test instead of by hand).  What the library reads is the
table of ilswiss_amd/csrc/switches.h — the only file of the library that touches the environment — and a row's lifetime there is in the
row's text in §6."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ilswiss_amd", "csrc")
# rows of the table for variables that Python reads, not the library
PYTHON_SIDE = {"ILSX_LIB": os.path.join("ilswiss_amd", "_lib.py"), "ILSX_GROUP_SHARE_STREAM": os.path.join("run_scripts", "_common.py")}
# how §6 words each lifetime of switches.h
LIFETIME_WORDS = {"PROCESS": "once per process", "CONTEXT": "when a context is created", "OBJECT": "at creation", "CALL": "per call"}


def read_by_the_library():
    """{name: lifetime} of the rows of switches.h"""
    text = open(os.path.join(CSRC, "switches.h")).read()
    return dict(re.findall(r'^\s*X\((ILSX_[A-Z0-9_]+),\s*\w+,\s*-?\d+,\s*(\w+),\s*"', text, flags=re.M))


def table_rows():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^## 6\. Run-time switches.*?$(.*?)(?=^## |\Z)", text, flags=re.S | re.M)
    assert m, "INTEGRATION.md has no section 6"
    return [l for l in m.group(1).splitlines() if l.startswith("| `ILSX_")]


def names_in(row):   # the first cell names the row's variables; the other cells may mention any
    return set(re.findall(r"`(ILSX_[A-Z0-9_]+)", row.split("|")[1])) | set(re.findall(r"`(ILSX_[A-Z0-9_]+)=", row))   # (or one introduced inside the text, with its value)


def listed_in_the_table():
    return set().union(*(names_in(row) for row in table_rows()))


def test_every_switch_the_library_reads_is_in_the_table_and_nothing_else():
    read, listed = set(read_by_the_library()), listed_in_the_table()
    assert len(read) >= 20, sorted(read)
    assert not (read & set(PYTHON_SIDE)), "a Python-side variable is read by the library too: drop it from PYTHON_SIDE"
    assert read - listed == set(), f"read by the library, no row in INTEGRATION §6: {sorted(read - listed)}"
    assert listed - read - set(PYTHON_SIDE) == set(), f"listed in INTEGRATION §6, read by nothing: {sorted(listed - read - set(PYTHON_SIDE))}"


def test_the_library_reads_its_environment_in_switches_h_only():
    for f in sorted(os.listdir(CSRC)):
        if f != "switches.h" and f.endswith((".hip", ".h", ".inc", ".cpp", ".c")):
            assert "getenv(" not in open(os.path.join(CSRC, f)).read(), f
    assert "getenv(" in open(os.path.join(CSRC, "switches.h")).read()


def test_every_row_says_when_its_variables_are_read():
    read, rows = read_by_the_library(), table_rows()
    assert set(read.values()) == set(LIFETIME_WORDS)
    for name, life in read.items():
        mine = [row for row in rows if name in names_in(row)]
        assert mine and any(LIFETIME_WORDS[life] in row for row in mine), (name, life, LIFETIME_WORDS[life])


def test_the_python_side_rows_are_read_where_the_list_says():
    for name, rel in PYTHON_SIDE.items():
        assert name in open(os.path.join(ROOT, rel)).read(), (name, rel)
