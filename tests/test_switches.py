"""Every ADR_* environment variable the source reads is a row of the "Switches" table in DESIGN.md, and the table
names nothing else: a switch cannot come back (or linger after its last user went) unrecorded. Reads source text
only; loads no library."""
import re

from conftest import ROOT

SRC = [ROOT / "yolo-ad-refine_amd" / "csrc", ROOT / "yolo-ad-refine_amd" / "adrefine"]
NAME = r"ADR_[A-Z0-9_]+"
# a name inside a getenv( / getenv_is( / dw_env_on( call or an environ expression (get, index, membership test)
READS = [re.compile(r"\b(?:getenv|getenv_is|dw_env_on)\(\s*\"(%s)\"" % NAME),
         re.compile(r"environ(?:\.get\(|\[)\s*\"(%s)\"" % NAME),
         re.compile(r"\"(%s)\"\s+(?:not\s+)?in\s+(?:os\.)?environ" % NAME)]


def _source_reads():
    names = set()
    for base in SRC:
        for f in sorted(base.rglob("*")):
            if f.suffix in (".hip", ".h", ".cpp", ".py"):
                text = f.read_text()
                for rx in READS:
                    names.update(rx.findall(text))
    return names


def _table_names():
    text = (ROOT / "DESIGN.md").read_text()
    m = re.search(r"^## [0-9. ]*Switches\s*$(.*?)(?=^## |\Z)", text, re.M | re.S)
    assert m, "DESIGN.md has no section headed 'Switches'"
    rows = [ln for ln in m.group(1).splitlines() if ln.startswith("|")][2:]  # past the header and the rule
    return {n for ln in rows for n in re.findall(NAME, ln.split("|")[1])}


def test_switch_table_matches_the_source():
    src, doc = _source_reads(), _table_names()
    assert src, "found no environment reads: the patterns no longer match the source"
    assert src == doc, f"read but not in the table: {sorted(src - doc)}; in the table but not read: {sorted(doc - src)}"
