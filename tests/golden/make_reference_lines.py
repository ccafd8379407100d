"""Regenerates tests/golden/reference_lines.json: the path of every .rs file of the
reference (relative to its root) and its number of lines, which is all that
tests/test_citations.py needs of it.

  python tests/golden/make_reference_lines.py REFERENCE_ROOT
"""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    lines = {}
    for f in sorted(glob.glob(os.path.join(ref, "**", "*.rs"), recursive=True)):
        with open(f, errors="replace") as fh:
            lines[os.path.relpath(f, ref)] = sum(1 for _ in fh)
    out = {"source": "line counts of the reference's .rs files (tests/golden/make_reference_lines.py)",
           "lines": lines}
    with open(os.path.join(HERE, "reference_lines.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
