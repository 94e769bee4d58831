"""CPU suite: every environment variable libilsx.so reads has a row in the table of INTEGRATION §6, and the table lists no variable
that nothing reads (the "every remaining switch is listed" condition, held by a test instead of by hand)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ilswiss_amd", "csrc")
# rows of the table for variables that Python reads, not the library
PYTHON_SIDE = {"ILSX_LIB": os.path.join("ilswiss_amd", "_lib.py"), "ILSX_GROUP_SHARE_STREAM": os.path.join("run_scripts", "_common.py")}


def read_by_the_library():
    names = set()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h", ".inc")):
            names |= set(re.findall(r'getenv\(\s*"(ILSX_[A-Z0-9_]+)"\s*\)', open(os.path.join(CSRC, f)).read()))
    return names


def listed_in_the_table():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^## 6\. Run-time switches.*?$(.*?)(?=^## |\Z)", text, flags=re.S | re.M)
    assert m, "INTEGRATION.md has no section 6"
    rows = [l for l in m.group(1).splitlines() if l.startswith("| `ILSX_")]
    names = set()
    for row in rows:   # the first cell names the row's variables; the other cells may mention any
        names |= set(re.findall(r"`(ILSX_[A-Z0-9_]+)", row.split("|")[1]))
        names |= set(re.findall(r"`(ILSX_[A-Z0-9_]+)=", row))   # a variable introduced inside another row's text, with its value
    return names


def test_every_switch_the_library_reads_is_in_the_table_and_nothing_else():
    read, listed = read_by_the_library(), listed_in_the_table()
    assert len(read) >= 20, sorted(read)
    assert not (read & set(PYTHON_SIDE)), "a Python-side variable is read by the library too: drop it from PYTHON_SIDE"
    assert read - listed == set(), f"read by the library, no row in INTEGRATION §6: {sorted(read - listed)}"
    assert listed - read - set(PYTHON_SIDE) == set(), f"listed in INTEGRATION §6, read by nothing: {sorted(listed - read - set(PYTHON_SIDE))}"


def test_the_python_side_rows_are_read_where_the_list_says():
    for name, rel in PYTHON_SIDE.items():
        assert name in open(os.path.join(ROOT, rel)).read(), (name, rel)
