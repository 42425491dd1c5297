"""Regenerates tests/golden/STRIP_SWEEP_CENSUS.txt: the census of the rank-strip sweep (tests/stripsweep.py) -- per case and multigrid depth the
strip, the halo rows an exchange moves and the side of every threshold the relaxation scheduler branches on; then per side the cases, shapes and
rank counts that take it.  From the table and the CPU oracle alone (the oracle confirms the number of depths of every case).  Needs no GPU.

    python tools/strip_sweep_census.py [--check]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))


def main(argv):
    from oracle import pyoracle
    from tests import stripsweep as ss
    pyoracle.build()
    problems = ss.depth_problems(pyoracle)
    for p in problems:
        print("PROBLEM:", p)
    text = ss.census_table(ss.census())
    path = os.path.join(ROOT, "tests", "golden", "STRIP_SWEEP_CENSUS.txt")
    if "--check" in argv:
        same = os.path.exists(path) and open(path).read() == text
        print("unchanged" if same else "DIFFERS from " + path)
        return 0 if same and not problems else 1
    with open(path, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
