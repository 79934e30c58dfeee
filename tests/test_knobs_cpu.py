"""INTEGRATION.md's knob table (§6) against the build switches of csrc/: every `-DOCTPT_X` the table names is a
symbol some preprocessor directive of the sources reads or defines, and every `#ifndef OCTPT_X` / `#ifdef OCTPT_X`
switch of the sources has its row.  A switch removed from the code leaves the table with it, and a new one is
documented where an integrator looks for it."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "octree_pathtracing_amd" / "csrc"


def table_switches():
    """the -DOCTPT_X names in the rows of the table under '## 6. Tuning knobs'"""
    text = (ROOT / "INTEGRATION.md").read_text()
    section = text.split("## 6. Tuning knobs", 1)[1].split("\n## ", 1)[0]
    rows = [line for line in section.splitlines() if line.startswith("|")]
    assert len(rows) > 2, "knob table not found"
    return set(re.findall(r"-D(OCTPT_[A-Z0-9_]+)", "\n".join(rows)))


def source_directives():
    """(directive, rest of the line) of every preprocessor line in csrc/*.{hip,h,cpp}"""
    out = []
    files = [f for ext in ("*.hip", "*.h", "*.cpp") for f in sorted(CSRC.glob(ext))]
    assert files, "no sources found"
    for f in files:
        for line in f.read_text().splitlines():
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif|define|undef)\b(.*)", line)
            if m:
                out.append((m.group(1), m.group(2)))
    return out


def test_table_switches_exist_in_sources():
    symbols = set()
    for _, rest in source_directives():
        symbols.update(re.findall(r"\bOCTPT_[A-Z0-9_]+\b", rest))
    missing = sorted(table_switches() - symbols)
    assert not missing, f"INTEGRATION.md names build switches the sources do not have: {missing}"


def test_source_switches_are_in_table():
    switches = set()
    for directive, rest in source_directives():
        if directive in ("ifdef", "ifndef"):
            m = re.match(r"\s*(OCTPT_[A-Z0-9_]+)\b", rest)
            if m:
                switches.add(m.group(1))
    assert switches, "no build switches found"
    missing = sorted(switches - table_switches())
    assert not missing, f"build switches without a row in INTEGRATION.md's knob table: {missing}"
