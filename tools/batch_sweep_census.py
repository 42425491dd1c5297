"""Regenerates tests/golden/BATCH_SWEEP_CENSUS.txt: the census of the ensemble sweep (tests/batchsweep.py) on the CPU oracle -- per batch the path
of every depth, the launches of a relax and of a cycle, the partials of the members' norm, the cycles of every member's solve and where its
residual maximum sits; the arms and the batches that take them; the mask palettes' arms; the time step's branches.  Needs no GPU.

    python tools/batch_sweep_census.py [--check]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))


def main(argv):
    from oracle import pyoracle
    from tests import batchsweep as bw
    pyoracle.build()
    s, st = bw.sweep_census(pyoracle), bw.step_census(pyoracle)
    for p in s["problems"] + st["problems"]:
        print("PROBLEM:", p)
    text = bw.census_table(s, st)
    path = os.path.join(ROOT, "tests", "golden", "BATCH_SWEEP_CENSUS.txt")
    if "--check" in argv:
        same = os.path.exists(path) and open(path).read() == text
        print("unchanged" if same else "DIFFERS from " + path)
        return 0 if same and not s["problems"] and not st["problems"] else 1
    with open(path, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 1 if s["problems"] or st["problems"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
