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

--bottom-solver: the batched step without and with the creation option bottom_solver (RelaxSolver after the bottom relaxes of every V-cycle,
one workgroup per member in one launch) against n solo steps with level option bottom_solver = 1, for two workloads at 320 x 64: SHMIP A3 and the
tutorial run's model (exec/0_convergence_channelized: moulin, ramp, diffusion, implicit gap-height solve; tools/convergence_channelized.py).  The
two batches do not compute the same bits (the option changes every cycle): V-cycles per step and member are printed next to the milliseconds.
    python tools/batch_bench.py --bottom-solver [--n 1,6,16,32] [--steps 50] [--warmup 60] [--repeat 3]

--forcing: a run is more than the step -- the water input changes every step and a diagnostic row is written.  Two ensembles, each stepped with its
forcing before and the daily row (post_proc_shmip_temporal) after EVERY step: suite F's style (the valley glacier at 256 x 64 under the seasonal
recharge, a temperature offset per member) and suite C's style (suite B's moulins at 320 x 64 under a diurnal time factor per member).  Timed
(a) through the member handles, one member at a time (suhmo_level_time_varying_recharge with the surface uploaded every call /
suhmo_level_moulin_source, suhmo_level_postproc_temporal: nothing else existed before the ensemble calls, so --only handles runs on older
trees too) and (b) through suhmo_batch_time_varying_recharge / suhmo_batch_moulin_source and suhmo_batch_postproc_temporal.
    python tools/batch_bench.py --forcing [--only both|handles|batch] [--n 1,5,16,32] [--steps 200] [--warmup 60] [--repeat 5]

--run: the time loop itself.  A suite-F-style run (the valley glacier at 320 x 64 under the seasonal recharge, a temperature offset per member,
steps of 2 h, a daily row) of `--steps` steps after `--warmup`, timed (a) as the per-call loop (time_varying_recharge + timestep per step,
postproc_partial_all + the host function per day) and (b) as ONE call of HipBatchModel.run (suhmo_batch_run), the two in alternating runs on the
same ensemble; wall time per step, median of `--repeat` runs each [min .. max].  A gain smaller than the spread is no gain.
    python tools/batch_bench.py --run [--only both|loop|run] [--n 1,5,16,32] [--steps 2000] [--warmup 200] [--repeat 3] [--balance-every N]
--balance-every N (with --run): both ways also take the water budget after every N-th step ("WATER BUDGET", include/suhmo_hip.h) -- the one
call as the series inside the run (balance_every=N: no copy and no synchronisation per row), the loop as a user writes it without the series
(mass_balance_all before the step for Bold, water_budget_all after it: two synchronising read-backs per row).
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


def bottom_solver_table(a):
    """--bottom-solver: per workload and n, the batched step with the option off and on, and n solo steps with bottom_solver = 1"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import convergence_channelized as cc
    print("# batched time step at %d x %d with and without RelaxSolver at the bottom of every V-cycle; %d timed steps after %d, median of %d runs [min .. max], ms per step"
          % (NX, NY, a.steps, a.warmup, a.repeat))
    print("# workload   n   (a) batch, bottom_solver=0    (b) batch, bottom_solver=1    (c) n solo steps, bottom_solver=1   (a)/(b)  (c)/(b)  "
          "V-cycles/step/member (a) (b)   gap V-cycles/step/member (a) (b)   launches/step (a) (b)   RelaxSolver iterations/solve (b)")
    for name in ("a3", "tutorial"):
        if name == "a3":
            m, bc, ph = sy.shmip_a_model("A3"), sy.A3_BC, sy.A3_PHYS
            st, src, ramp = sy.shmip_initial_state(NX, NY, m["lx"], m["ly"]), None, None
        else:
            m, bc, ph, ramp = dict(cc.MODEL), cc.BC, cc.PHYS, cc.ramp
            st = cc.basic_state(NX, NY)
            L = model.HipModel(NX, NY, st["dx"], st["dy"], bc, ph, m, max_box=64)
            L.moulin_source(cc.MOULIN[0], cc.MOULIN[1], cc.MOULIN[2], 1.0)
            src = L.get("msrc")
            L.close()
        implicit = bool(m.get("use_impl_diff", 0))
        for n in [int(x) for x in a.n.split(",")]:
            Bs = [model.HipBatchModel(NX, NY, st["dx"], st["dy"], bc, ph, [m] * n, max_box=64, implicit_gap=implicit, bottom_solver=on) for on in (False, True)]
            Ls = [model.HipModel(NX, NY, st["dx"], st["dy"], bc, ph, m, max_box=64) for _ in range(n)]
            for L in Ls:
                L.level.set_option("bottom_solver", 1)
            for k in range(n):
                for M in [B.member(k) for B in Bs] + [Ls[k]]:
                    M.set_state(st)
                    if src is not None:                      # (the tutorial run: its moulin, and the melt rate it starts from)
                        M.level.set(lv.F_MSRC, src)
                        M.level.set(lv.F_MR, np.full((NY, NX), m["G"] / m["L"]))
            res = []
            for B in Bs + [None]:
                cyc, stepno = [0], [0]

                def step():
                    r = float(ramp(stepno[0] * m["dt"])) if ramp else None
                    stepno[0] += 1
                    if B:
                        if r is not None:
                            for k in range(n):
                                B.set_model(k, ramp=r)
                        cyc[0] += sum(B.timestep(m["dt"])[1])
                    else:
                        for L in Ls:
                            if r is not None:
                                L._mp.ramp = r
                            cyc[0] += L.timestep(m["dt"])[1]

                for _ in range(a.warmup):
                    step()
                keys = ("batch_launches", "batch_gap_member_cycles", "bottom_solver_iterations", "bottom_solves_one_launch")
                o0, c0 = [B.get_option(k) for k in keys] if B else [0] * 4, cyc[0]
                t = runs(step, (B.member(0) if B else Ls[0]).level.synchronize, a.steps, a.repeat)
                o1 = [B.get_option(k) for k in keys] if B else [0] * 4
                nst = a.steps * a.repeat
                res.append((t, (cyc[0] - c0) / nst / n, (o1[1] - o0[1]) / nst / n, (o1[0] - o0[0]) / nst, (o1[2] - o0[2]) / max(o1[3] - o0[3], 1)))
            (ta, va, ga, la, _), (tb, vb, gb, lb, ib), (tc, vc, _, _, _) = res
            print("%-9s %3d   %8.3f [%7.3f .. %7.3f]   %8.3f [%7.3f .. %7.3f]   %8.3f [%7.3f .. %7.3f]   %6.2f   %6.2f   %6.2f %6.2f   %6.2f %6.2f   %7.1f %7.1f   %6.2f   (solo V-cycles/step/member %.2f)"
                  % (name, n, ta[0], ta[1], ta[2], tb[0], tb[1], tb[2], tc[0], tc[1], tc[2], ta[0] / tb[0], tc[0] / tb[0], va, vb, ga, gb, la, lb, ib, vc), flush=True)
            for B in Bs:
                B.close()
            for L in Ls:
                L.close()


def forcing_table(a):
    """--forcing: per ensemble and n, the forced and diagnosed step through the member handles and through the ensemble calls"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_shmip_f as rf
    print("# forced and diagnosed time step (forcing before, daily row after every step); %d timed steps after %d, median of %d runs [min .. max], ms per step"
          % (a.steps, a.warmup, a.repeat))
    print("# ensemble   n   (a) member handles       (b) ensemble calls       (a)/(b)   launches/step (a) (b)   read-backs/step (a) (b)   [counters: the batch's own; "
          "the per-level calls of (a) are not in them]")
    binp = json.load(open(os.path.join(ROOT, "tests", "golden", "shmip_B_inputs.json")))
    nan = (float("nan"),) * 3
    for name in ("suite-F", "suite-C"):
        for n in [int(x) for x in a.n.split(",")]:
            if name == "suite-F":
                m, nx, ny, dt = dict(rf.F_MODEL), rf.F_MODEL["nx"], rf.F_MODEL["ny"], 7200.0
                st = sy.valley_initial_state(nx, ny, 0.05, m["lx"], m["ly"])
                phys = dict(sy.A3_PHYS, A=2.5e-25)
                X = (np.arange(-1, nx + 1) + 0.5)[None, :] * st["dx"] + np.zeros((ny + 2, 1))
                zs = 100.0 * np.power(X + 200.0, 0.25) + X / 60.0 - np.power(2.0e10, 0.25) + 1.0
                delta = np.linspace(-6.0, 6.0, n) if n > 1 else np.zeros(1)
                models = [m] * n
            else:
                nx, ny, dt, phys = NX, NY, 3600.0, sy.A3_PHYS
                st = sy.shmip_initial_state(nx, ny)
                cases = [("B1", "B2", "B3", "B4", "B5")[k % 5] for k in range(n)]
                models = [sy.shmip_b_model(c, binp[c]) for c in cases]
                lists = [(np.array(binp[c]["positions"]).reshape(-1, 2), np.array(binp[c]["sigma"], dtype=float), np.array(binp[c]["flux"], dtype=float)) for c in cases]
                shift = np.arange(n) * 3600.0
            res = {}
            for way in ("handles", "batch"):
                if a.only not in ("both", way):
                    res[way] = (nan, float("nan"), float("nan"))
                    continue
                B = model.HipBatchModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, phys, models, max_box=64, implicit_gap=True)
                for k in range(n):
                    B.set_state(k, st)
                    if name == "suite-F":
                        B.member(k).level.set(lv.F_MR, np.full((ny, nx), m["G"] / m["L"]))
                        if way == "batch":
                            B.set_surface(k, zs)
                tm = [180.0 * 86400.0]

                def step():
                    t = tm[0]
                    tm[0] += dt
                    if name == "suite-F":
                        T_K = -16.0 * np.cos(2.0 * np.pi * t / (365.0 * 24 * 60 * 60.0)) - 5.0 + delta
                        if way == "batch":
                            B.time_varying_recharge(T_K, rf.BACKGROUND)
                        else:
                            for k in range(n):
                                B.member(k).time_varying_recharge(zs, T_K[k], rf.BACKGROUND)
                    else:
                        tf = np.maximum(0.0, 1.0 - np.sin(2.0 * np.pi * (t + shift) / 86400.0))      # a diurnal cycle, an hour's shift per member
                        if way == "batch":
                            B.moulin_source(lists, tf)
                        else:
                            for k in range(n):
                                B.member(k).moulin_source(lists[k][0], lists[k][1], lists[k][2], tf[k])
                    B.timestep(dt)
                    if way == "batch":
                        B.postproc_temporal_all()
                    else:
                        for k in range(n):
                            B.postproc_temporal(k)

                for _ in range(a.warmup):
                    step()
                l0, r0 = B.get_option("batch_launches"), B.get_option("batch_readbacks")
                t = runs(step, B.member(0).level.synchronize, a.steps, a.repeat)
                nst = a.steps * a.repeat
                res[way] = (t, (B.get_option("batch_launches") - l0) / nst, (B.get_option("batch_readbacks") - r0) / nst)
                B.close()
            (ta, la, ra), (tb, lb, rb) = res["handles"], res["batch"]
            print("%-9s %3d   %8.3f [%7.3f .. %7.3f]   %8.3f [%7.3f .. %7.3f]   %6.2f   %7.1f %7.1f   %6.2f %6.2f"
                  % (name, n, ta[0], ta[1], ta[2], tb[0], tb[1], tb[2], ta[0] / tb[0], la, lb, ra, rb), flush=True)


def run_table(a):
    """--run: per n, a run of a.steps steps through the per-call loop and through one call, alternating"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_shmip_f as rf
    m, nx, ny, dt, per_day = dict(rf.F_MODEL), NX, NY, 7200.0, 12
    st = sy.valley_initial_state(nx, ny, 0.05, m["lx"], m["ly"])
    phys = dict(sy.A3_PHYS, A=2.5e-25)
    X = (np.arange(-1, nx + 1) + 0.5)[None, :] * st["dx"] + np.zeros((ny + 2, 1))
    zs = 100.0 * np.power(X + 200.0, 0.25) + X / 60.0 - np.power(2.0e10, 0.25) + 1.0
    print("# suite-F-style run at %d x %d: %d steps of 2 h after %d, a daily row; (a) the per-call loop, (b) one call (HipBatchModel.run), alternating runs on one "
          "ensemble; median of %d runs [min .. max], ms per step" % (nx, ny, a.steps, a.warmup, a.repeat))
    print("#   n   (a) per-call loop          (b) one call               (a)/(b)   (a) - (b) [ms/step]   spread (a), (b) [ms/step]   verdict   "
          "launches/step (a) (b)   read-backs/step (a) (b)")
    for n in [int(x) for x in a.n.split(",")]:
        delta = np.linspace(-6.0, 6.0, n) if n > 1 else np.zeros(1)
        B = model.HipBatchModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, phys, [m] * n, max_box=64, implicit_gap=True)
        for k in range(n):
            B.set_state(k, st)
            B.member(k).level.set(lv.F_MR, np.full((ny, nx), m["G"] / m["L"]))
            B.set_surface(k, zs)
        tm = [180.0 * 86400.0]

        def temperatures(steps):
            t = tm[0] + dt * np.arange(steps)
            tm[0] += dt * steps
            return -16.0 * np.cos(2.0 * np.pi * t[:, None] / (365.0 * 24 * 60 * 60.0)) - 5.0 + delta[None, :]

        def loop(steps):
            T_K = temperatures(steps)
            for k in range(steps):
                B.time_varying_recharge(T_K[k], rf.BACKGROUND)
                row = a.balance_every > 0 and (k + 1) % a.balance_every == 0
                if row and B.cur_step > 0:
                    B.mass_balance_all()
                B.timestep(dt)
                if row:
                    B.water_budget_all()
                if (k + 1) % per_day == 0:
                    sums = B.postproc_partial_all()
                    for q in range(n):
                        B.members[q].postproc_temporal_host(sums[q])

        def one_call(steps):
            B.run(steps, dt, T_K=temperatures(steps), background=rf.BACKGROUND, diag_every=per_day, balance_every=a.balance_every)

        ways = [w for w in (("loop", loop), ("run", one_call)) if a.only in ("both", w[0])]
        ways[0][1](a.warmup)
        times, counts = {w: [] for w, _ in ways}, {}
        for _ in range(a.repeat):
            for w, fn in ways:
                l0, r0 = B.get_option("batch_launches"), B.get_option("batch_readbacks")
                B.member(0).level.synchronize()
                t0 = time.perf_counter()
                fn(a.steps)
                B.member(0).level.synchronize()
                times[w].append((time.perf_counter() - t0) / a.steps * 1e3)
                counts[w] = ((B.get_option("batch_launches") - l0) / a.steps, (B.get_option("batch_readbacks") - r0) / a.steps)
        B.close()
        nan = [float("nan")]
        ta, tb = times.get("loop", nan), times.get("run", nan)
        ma, mb = statistics.median(ta), statistics.median(tb)
        sa, sb = max(ta) - min(ta), max(tb) - min(tb)
        verdict = "n/a" if ma != ma or mb != mb else "no gain" if abs(ma - mb) <= max(sa, sb) else "one call faster" if mb < ma else "one call slower"
        ca, cb = counts.get("loop", (float("nan"),) * 2), counts.get("run", (float("nan"),) * 2)
        print("%5d   %8.3f [%7.3f .. %7.3f]   %8.3f [%7.3f .. %7.3f]   %6.2f   %8.3f   %7.3f %7.3f   %-15s   %7.1f %7.1f   %6.2f %6.2f"
              % (n, ma, min(ta), max(ta), mb, min(tb), max(tb), ma / mb, ma - mb, sa, sb, verdict, ca[0], cb[0], ca[1], cb[1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default=None)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--repeat", type=int, default=None)
    ap.add_argument("--bottom-solver", action="store_true")
    ap.add_argument("--suite", choices=("A", "B"), default="A")
    ap.add_argument("--forcing", action="store_true")
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--balance-every", type=int, default=0)
    ap.add_argument("--only", choices=("both", "batch", "solo", "handles", "loop", "run"), default="both")
    a = ap.parse_args()
    a.n = a.n or ("1,6,16,32" if a.bottom_solver else "1,5,16,32" if a.forcing or a.run else "1,2,4,6,8,16,32")
    a.steps, a.repeat = a.steps or (50 if a.bottom_solver else 2000 if a.run else 200), a.repeat or (3 if a.bottom_solver or a.run else 5)
    a.warmup = (200 if a.run else 60) if a.warmup is None else a.warmup
    if a.run:
        return run_table(a)
    if a.bottom_solver:
        return bottom_solver_table(a)
    if a.forcing:
        return forcing_table(a)
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
