"""Regenerates tests/golden/BCOEF_SWEEP_CENSUS.txt: the census of the face-coefficient sweep (tests/bcoefsweep.py) -- per predicate of the gradient's
mask tests, bcoef_face, the ghost gradients and the tiles of k_bcoef_fused, how many cells, faces or levels take each arm and in how many cases.
Needs no GPU.

    python tools/bcoef_sweep_census.py [--check]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))


def main(argv):
    from oracle import pyoracle
    from tests import bcoefsweep as bs
    pyoracle.build()
    s = bs.sweep_census(pyoracle)
    for p in s["problems"]:
        print("PROBLEM:", p)
    text = bs.census_table(s)
    path = os.path.join(ROOT, "tests", "golden", "BCOEF_SWEEP_CENSUS.txt")
    if "--check" in argv:
        same = os.path.exists(path) and open(path).read() == text
        print("unchanged" if same else "DIFFERS from " + path)
        return 0 if same and not s["problems"] else 1
    with open(path, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 1 if s["problems"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
