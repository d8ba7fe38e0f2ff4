"""Every `file:line` citation of the reference in the interface header, the adapters, the host mirrors and the documents points
at an existing file of the reference with at least that many lines.  The files and their lengths come from tests/golden/reference_line_counts.json
(tests/golden/make_reference_line_counts.py), which is checked against the reference tree wherever that tree is present."""
import glob
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
LINE_COUNTS = os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")
CITE = re.compile(r"(?<![\w/.])((?:[\w.-]+/)*[\w.-]+\.(?:cpp|hpp|launch|xml|txt))`?:(\d+)(?:[-–](\d+))?")


def _sources():
    pats = ["include/*.h", "adapters/*.hpp", "hdl_graph_slam_amd/*.py", "hdl_graph_slam_amd/csrc/*", "oracle/*.hpp", "oracle/*.cpp", "DESIGN.md",
            "INTEGRATION.md", "bench.py", "tests/cpp/*.cpp"]
    return sorted(f for p in pats for f in glob.glob(os.path.join(ROOT, p)))


def _line_counts():
    with open(LINE_COUNTS) as fh:
        return json.load(fh)


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not present here")
def test_committed_line_counts_match_the_reference_tree():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_reference_line_counts as MC
    assert MC.line_counts(REF) == _line_counts()


def test_reference_citations_resolve():
    counts = _line_counts()
    index = {}
    for rel in counts:
        index.setdefault(os.path.basename(rel), []).append("/" + rel)
    own = {os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "**", "*"), recursive=True)}
    checked, bad = 0, []
    for src in _sources():
        text = open(src, errors="replace").read()
        for m in CITE.finditer(text):
            path, lo, hi = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
            base = os.path.basename(path)
            cands = [c for c in index.get(base, []) if c.endswith("/" + path) or "/" not in path]
            if not cands:
                if base in own or base not in index:
                    continue            # a citation of this repository's own files, or of a third-party file named in prose
                bad.append((os.path.relpath(src, ROOT), m.group(0), "no such path in the reference"))
                continue
            n_lines = max(counts[c[1:]] for c in cands)
            checked += 1
            if hi < lo or hi > n_lines:
                bad.append((os.path.relpath(src, ROOT), m.group(0), f"file has {n_lines} lines"))
    assert checked > 100, checked
    assert not bad, bad[:20]
