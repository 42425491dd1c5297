#!/usr/bin/env python
"""Ensemble of SHMIP A3 runs at 320 x 64: one batched time step of n members (suhmo_batch_timestep) against n solo steps
(suhmo_level_timestep on n ordinary levels, one after the other) in the same process.

Both sides start from the SHMIP initial state and take `--warmup` steps (past the solver-parameter thresholds at steps 2 and 50), then
`--repeat` runs of `--steps` timed steps each; the figure is the median of the runs' wall time per step (min and max shown: the spread).
Prints for every n
    (a) wall time per batched step, (b) wall time of n solo steps, (b)/(a), launches and read-backs per batched step, V-cycles per step.
    python tools/batch_bench.py [--n 1,2,4,6,8,16,32] [--steps 200] [--warmup 60] [--repeat 5]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from suhmo_amd import model, synthetic as sy    # noqa: E402

NX, NY = 320, 64


def runs(step, sync, steps, repeat):
    out = []
    for _ in range(repeat):
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,2,4,6,8,16,32")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    m = sy.shmip_a_model("A3")
    st = sy.shmip_initial_state(NX, NY, m["lx"], m["ly"])
    print("# SHMIP A3 time step, %d x %d, %d timed steps after %d, median of %d runs [min .. max], ms per step" % (NX, NY, a.steps, a.warmup, a.repeat))
    print("# n   (a) batched step         (b) n solo steps         (b)/(a)  launches/step  read-backs/step  V-cycles/step/member")
    for n in [int(x) for x in a.n.split(",")]:
        B = model.HipBatchModel(NX, NY, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, [m] * n, max_box=64)
        Ls = [model.HipModel(NX, NY, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=64) for _ in range(n)]
        for k in range(n):
            B.set_state(k, st); Ls[k].set_state(st)
        cyc = [0]

        def step_b():
            cyc[0] += B.timestep(m["dt"])[1][0]

        def step_s():
            for L in Ls:
                L.timestep(m["dt"])

        for _ in range(a.warmup):
            step_b(); step_s()
        l0, r0, c0 = B.get_option("batch_launches"), B.get_option("batch_readbacks"), cyc[0]
        ta = runs(step_b, B.member(0).level.synchronize, a.steps, a.repeat)
        nst = a.steps * a.repeat
        launches, readbacks = (B.get_option("batch_launches") - l0) / nst, (B.get_option("batch_readbacks") - r0) / nst
        tb = runs(step_s, Ls[0].level.synchronize, a.steps, a.repeat)
        print("%3d   %8.3f [%7.3f .. %7.3f]   %8.3f [%7.3f .. %7.3f]   %6.2f   %10.1f   %12.2f   %10.2f" % (
            n, ta[0], ta[1], ta[2], tb[0], tb[1], tb[2], tb[0] / ta[0], launches, readbacks, (cyc[0] - c0) / nst), flush=True)
        B.close()
        for L in Ls:
            L.close()


if __name__ == "__main__":
    main()
