"""Writes tests/golden/reference_line_counts.json: the path (relative to the reference tree) and line count of every reference file a
`file:line` citation can name (.cpp / .hpp / .launch / .xml / .txt).  No content of those files, only their lengths: tests/test_citations.py
resolves the citations against this table where the reference tree is absent, and checks the table against the tree where it is present.

Re-run (where the reference tree exists): python tests/golden/make_reference_line_counts.py"""
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"
OUT = os.path.join(HERE, "reference_line_counts.json")
CITED = re.compile(r"\.(?:cpp|hpp|launch|xml|txt)$")


def line_counts(ref: str = REFERENCE) -> dict:
    out = {}
    for d, _, files in os.walk(ref):
        for f in files:
            if CITED.search(f):
                p = os.path.join(d, f)
                with open(p, errors="replace") as fh:
                    out[os.path.relpath(p, ref)] = sum(1 for _ in fh)
    return dict(sorted(out.items()))


if __name__ == "__main__":
    with open(OUT, "w") as fh:
        json.dump(line_counts(), fh, indent=0)
        fh.write("\n")
    print(OUT)
