#!/usr/bin/env python
"""Ensemble of SHMIP A3 runs at 320 x 64: one batched time step of n members (suhmo_batch_timestep) against n solo steps
(suhmo_level_timestep on n ordinary levels, one after the other) in the same process.  --suite B: the members are suite B's models as the
reference runs them (implicit gap-height solve, diffFactor 1, moulin source of tests/golden/shmip_B_inputs.json, cases B1 ... B5 in turn),
the batch with option implicit_gap on.  --only batch / solo: one side alone (with SUHMO_LIB: that side from another build of the library).

Both sides start from the SHMIP initial state and take `--warmup` steps (past the solver-parameter thresholds at steps 2 and 50), then
`--repeat` runs of `--steps` timed steps each; the figure is the median of the runs' wall time per step (min and max shown: the spread).
Prints for every n
    (a) wall time per batched step, (b) wall time of n solo steps, (b)/(a), launches and read-backs per batched step, V-cycles per step.
    python tools/batch_bench.py [--suite A|B] [--only both|batch|solo] [--n 1,2,4,6,8,16,32] [--steps 200] [--warmup 60] [--repeat 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np    # noqa: E402

from suhmo_amd import level as lv, model, synthetic as sy    # noqa: E402

NX, NY = 320, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def suite_b_members(n, st):
    """(model, moulin source array) of B1 ... B5 in turn; the source through HipModel.moulin_source on a level of its own"""
    binp = json.load(open(os.path.join(ROOT, "tests", "golden", "shmip_B_inputs.json")))
    made = {}
    for case in ("B1", "B2", "B3", "B4", "B5")[:n]:
        m = sy.shmip_b_model(case, binp[case])
        L = model.HipModel(NX, NY, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=64)
        L.moulin_source(np.array(binp[case]["positions"]).reshape(-1, 2), binp[case]["sigma"], binp[case]["flux"], 1.0)
        made[case] = (m, L.get("msrc"))
        L.close()
    cases = list(made)
    return [made[cases[k % len(cases)]] for k in range(n)]


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
    ap.add_argument("--suite", choices=("A", "B"), default="A")
    ap.add_argument("--only", choices=("both", "batch", "solo"), default="both")
    a = ap.parse_args()
    m = sy.shmip_a_model("A3")
    st = sy.shmip_initial_state(NX, NY, m["lx"], m["ly"])
    what = "A3" if a.suite == "A" else "suite B (implicit gap-height solve)"
    print("# SHMIP %s time step, %d x %d, %d timed steps after %d, median of %d runs [min .. max], ms per step" % (what, NX, NY, a.steps, a.warmup, a.repeat))
    print("# n   (a) batched step         (b) n solo steps         (b)/(a)  launches/step  read-backs/step  V-cycles/step/member  gap V-cycles/step/member")
    nan = (float("nan"),) * 3
    for n in [int(x) for x in a.n.split(",")]:
        members = [(m, None)] * n if a.suite == "A" else suite_b_members(n, st)
        B, Ls = None, []
        if a.only != "solo":
            kw = dict(implicit_gap=True) if a.suite == "B" else {}
            B = model.HipBatchModel(NX, NY, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, [mm for mm, _ in members], max_box=64, **kw)
        if a.only != "batch":
            Ls = [model.HipModel(NX, NY, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, mm, max_box=64) for mm, _ in members]
        for k, (_, src) in enumerate(members):
            for M in ([B.member(k)] if B else []) + Ls[k:k + 1]:
                M.set_state(st)
                if src is not None:
                    M.level.set(lv.F_MSRC, src)
        cyc = [0]

        def step_b():
            cyc[0] += sum(B.timestep(m["dt"])[1])

        def step_s():
            for L in Ls:
                L.timestep(m["dt"])

        for _ in range(a.warmup):
            if B:
                step_b()
            step_s()
        ta, tb, launches, readbacks, gap = nan, nan, float("nan"), float("nan"), float("nan")
        nst = a.steps * a.repeat
        if B:
            opt = lambda key: B.get_option(key) if a.suite == "B" or key != "batch_gap_member_cycles" else 0
            l0, r0, g0, c0 = opt("batch_launches"), opt("batch_readbacks"), opt("batch_gap_member_cycles"), cyc[0]
            ta = runs(step_b, B.member(0).level.synchronize, a.steps, a.repeat)
            launches, readbacks, gap = (opt("batch_launches") - l0) / nst, (opt("batch_readbacks") - r0) / nst, (opt("batch_gap_member_cycles") - g0) / nst / n
        if Ls:
            tb = runs(step_s, Ls[0].level.synchronize, a.steps, a.repeat)
        print("%3d   %8.3f [%7.3f .. %7.3f]   %8.3f [%7.3f .. %7.3f]   %6.2f   %10.1f   %12.2f   %10.2f   %10.2f" % (
            n, ta[0], ta[1], ta[2], tb[0], tb[1], tb[2], tb[0] / ta[0], launches, readbacks, (cyc[0] - c0) / nst / n if B else float("nan"), gap), flush=True)
        if B:
            B.close()
        for L in Ls:
            L.close()


if __name__ == "__main__":
    main()
