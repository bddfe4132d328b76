"""The PPSFM_* environment switches are read in one place (csrc/switches.hip), listed once (the table in csrc/switches.hpp) and documented in
DESIGN.md section 8: the three lists agree, and the retired switches are gone (source text only, no device)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "privacy_preserving_sfm_amd", "csrc")
RETIRED = ["PPSFM_PCG_WIDE", "PPSFM_PCG_QUAD", "PPSFM_BA_CHUNK_SPLIT", "PPSFM_BA_CHUNK_LEN", "PPSFM_ABERTH_SWEEPS"]


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _sources(top):
    for d, _, files in os.walk(top):
        for name in sorted(files):
            if not name.endswith((".pyc", ".so", ".o")):
                yield os.path.join(d, name)


def _csrc():
    return {os.path.basename(p): _read(p) for p in _sources(CSRC) if p.endswith((".hip", ".hpp", ".h", ".cpp"))}


def _table():
    """the names of the comment table in switches.hpp (a row: `//   PPSFM_NAME   values ...`)"""
    return set(re.findall(r"^//\s+(PPSFM_[A-Z0-9_]+)\s", _read(os.path.join(CSRC, "switches.hpp")), re.M))


def _design_section_8():
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    m = re.search(r"^## 8\..*?(?=^## 9\.)", text, re.M | re.S)
    assert m, "DESIGN.md has no section 8"
    return set(re.findall(r"PPSFM_[A-Z0-9_]+", m.group(0)))


def test_only_switches_hip_reads_the_environment():
    readers = sorted(name for name, text in _csrc().items() if "getenv" in text)
    assert readers == ["switches.hip"], readers


def test_switch_literals_table_and_design_agree():
    literals = set()
    for text in _csrc().values():
        literals |= set(re.findall(r'"(PPSFM_[A-Z0-9_]+)"', text))
    table, design = _table(), _design_section_8()
    assert literals, "no switch literals found"
    assert literals == table, ("not in the switches.hpp table", literals - table, "table rows nothing reads", table - literals)
    assert table == design, ("not in DESIGN.md section 8", table - design, "documented but not a switch", design - table)


def test_retired_switches_are_gone():
    found = []
    for top in ("privacy_preserving_sfm_amd/csrc", "tests", "tools"):
        for path in _sources(os.path.join(ROOT, top)):
            if os.path.abspath(path) == os.path.abspath(__file__):
                continue
            try:
                text = _read(path)
            except UnicodeDecodeError:
                continue
            found += ["%s: %s" % (os.path.relpath(path, ROOT), n) for n in RETIRED if n in text]
    assert not found, found
