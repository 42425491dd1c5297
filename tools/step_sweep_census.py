"""Regenerates tests/golden/STEP_SWEEP_CENSUS.txt: the census of the time-step sweep (tests/stepsweep.py) on the CPU oracle -- per branch of the
time step's per-cell kernels, how many cells or faces took each arm and in how many cases.  Needs no GPU.

    python tools/step_sweep_census.py [--check]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))


def main(argv):
    from oracle import pyoracle
    from tests import stepsweep as sw
    pyoracle.build()
    s = sw.sweep_census(pyoracle)
    for p in s["problems"]:
        print("PROBLEM:", p)
    text = sw.census_table(s)
    path = os.path.join(ROOT, "tests", "golden", "STEP_SWEEP_CENSUS.txt")
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
