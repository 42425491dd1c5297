#!/usr/bin/env python3
"""AmrHydro::check_fluxes (src/AmrHydro.cpp:440-590) of a run, from the device: per step and level the reference's seven lines in its format
(:582-588) -- the discharge through the four domain sides, through the ice margin and the ice-bearing domain sides, the water volume B with Bold
taken from the same call before the step -- and one closing line: (V - Vold) / dt of the last step against recharge minus outflow, the recharge
from the column sums of the SHMIP table (external + melt; level 0's, as the reference evaluates it).
    python tools/mass_balance.py [--hier [--generated-grids]] [--one-call] [--time] [cells per side of the base] [steps]
default     SHMIP A3 on one level (cells: nx, with ny = nx / 5; default 320 x 64)
--hier      cfg5 (exec/AMR_multiMoulins physics) on base + 3 levels of box unions as tools/hier_bench.py makes them (default base 256^2);
            --generated-grids: the boxes from tagging the moulin source and clustering, the reference's way, instead of synthetic.boxes_around
--one-call  the same lines from the water budget series of ONE run call (HipHierModel.run / HipBatchModel.run with balance_every=1; include/
            suhmo_hip.h, "WATER BUDGET"): B/Bold with Bold kept on the device by the tracked step, and per step the reference's line
            "Time(months) VOL_waterTot rechargeTOT ramp" (:4036-4038; VOL_waterTot here is level 0's whole volume, the reference prints its first
            column's).  Without --hier the single level runs as an ensemble of one.  With --time: the one call against the per-call loop
            (balance, step, balance: two synchronising read-backs a step) in three alternating rounds, the counters of both
--time      instead of the lines: the call against the route that existed before it -- ghosted gets of head, mask and gap height and gets of both
            face coefficients for every box (5 copies per handle) followed by the sums in numpy -- in three alternating rounds, with the launch
            and copy counts, and 20 calls in a row; without --hier on a single level of [cells]^2 (default 4096^2) whose face coefficients are
            formed from the state as loaded (UpdateOperator; no step)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from suhmo_amd import capi, level as lv, model, synthetic as sy

hier = "--hier" in sys.argv
generated = "--generated-grids" in sys.argv
timing = "--time" in sys.argv
argv = [a for a in sys.argv[1:] if not a.startswith("--")]


def lines(v, vold):
    """the seven lines of :582-588 for one level"""
    tot = v["lo_x"] + v["lo_y"] - v["hi_x"] - v["hi_y"]
    return [" Flux loX %g, hiX %g" % (v["lo_x"], v["hi_x"]), " Flux loY %g, hiY %g" % (v["lo_y"], v["hi_y"]), " Total: %g" % tot,
            " Flux dirX %g" % v["dir_x"], " Flux dirY %g" % v["dir_y"], " Total: %g" % (v["dir_x"] + v["dir_y"]), " B/Bold: %g, %g" % (v["volume"], vold["volume"])]


def generated_boxes(nb, bc, ph, mm, mo):
    """three passes of the initGrids loop, as tools/hier_bench.py --generated-grids runs them (run_C_3lev's grid parameters)"""
    params = dict(fill_ratio=0.5, block_factor=2, max_box_size=64, nesting_radius=4)
    boxes = []
    for _ in range(3):
        M = model.HipHierModel(nb, nb, 1.0e5 / nb, 1.0e5 / nb, bc, ph, mm, boxes, max_box=64)
        M.moulin_source(**mo)
        peak = float(M.get(0, 0, "msrc").max())
        maps = []
        for l in range(len(boxes) + 1):
            M.tag_cells(l, "msrc", (0.01, 0.1, 0.5)[l] * peak, 1.0e300, grow=4, granularity=params["block_factor"] // 2)
            maps.append(M.tags(l))
        new = model.generate_grids(nb, nb, bc["periodic"], maps, **params)
        M.close()
        if len(new) <= len(boxes):
            break
        boxes = new
    return boxes


def setup():
    """-> (the model, its levels' box views [l][k], dt, balance(): a list of dicts per level, recharge(): m^3/s from level 0's column sums)"""
    if hier:
        nb = int(argv[0]) if argv else 256
        bc, ph, mm, mo = sy.multimoulins_setup()
        boxes = generated_boxes(nb, bc, ph, mm, mo) if generated else sy.boxes_around(mo["positions"], nb, nb, 4, 1.0e5, 1.0e5)
        M = model.HipHierModel(nb, nb, 1.0e5 / nb, 1.0e5 / nb, bc, ph, mm, boxes, max_box=64)
        M.set_states(sy.mountain_amrm_states(nb, nb, boxes))
        M.moulin_source(**mo)
        base = model._MemberModel(M.level[0][0], mm)
        return M, M.level, mm["dt"], M.mass_balance, lambda: float(base.postproc_partial()[4:6].sum()), bc
    m = sy.A3_MODEL
    nx = int(argv[0]) if argv else (4096 if timing else m["nx"])
    ny = nx if timing else max(nx // 5, 4)
    st = sy.shmip_initial_state(nx, ny, m["lx"], m["ly"])
    M = model.HipModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=64)
    M.set_state(st)
    return M, [[M.level]], m["dt"], lambda: [M.mass_balance()], lambda: float(M.postproc_partial()[4:6].sum()), sy.A3_BC


def host_route(levels, bc):
    """the route without the call: five gets per handle, then the rule in numpy (plain sums: the order is numpy's) -> ((7,) per level, copy seconds)"""
    t0 = time.perf_counter()
    got = [[(L.get(lv.F_PHI, ghosted=True), L.get(lv.F_MASK, ghosted=True), L.get(lv.F_B, ghosted=True), L.get(lv.F_BX), L.get(lv.F_BY)) for L in bl] for bl in levels]
    t_copy = time.perf_counter() - t0
    out = []
    for l, bl in enumerate(levels):
        a = np.zeros(7)
        for L, (h, m, B, bx, by) in zip(bl, got[l]):
            # (the physical sides of level 0 under SHMIP's and cfg5's boundary values, all 0: Dirichlet -near, Neumann near; inside the domain
            #  the stored ghosts)
            if l == 0:
                for d, s, sl_g, sl_n in ((0, 0, np.s_[1:-1, 0], np.s_[1:-1, 1]), (0, 1, np.s_[1:-1, -1], np.s_[1:-1, -2]), (1, 0, np.s_[0, 1:-1], np.s_[1, 1:-1]), (1, 1, np.s_[-1, 1:-1], np.s_[-2, 1:-1])):
                    if bc["periodic"][d]:
                        continue
                    v = bc["value"][d][s]
                    h[sl_g] = 2.0 * v - h[sl_n] if bc["type"][d][s] == 0 else h[sl_n] + (-1.0 if s == 0 else 1.0) * (L.dx, L.dy)[d] * v
            for d, K, hh, area, n in ((0, bx, L.dx, L.dy, L.nx), (1, by, L.dy, L.dx, L.ny)):
                hi, lo = (h[1:-1, 1:], h[1:-1, :-1]) if d == 0 else (h[1:, 1:-1], h[:-1, 1:-1])
                mh, ml = (m[1:-1, 1:], m[1:-1, :-1]) if d == 0 else (m[1:, 1:-1], m[:-1, 1:-1])
                t = -K * ((hi - lo) * (-1.0) / hh) * area
                first, last = (np.s_[:, 0], np.s_[:, n]) if d == 0 else (np.s_[0, :], np.s_[n, :])
                dd = mh - ml
                dom = np.zeros(t.shape, dtype=bool)
                if l == 0:
                    dom[first] = dom[last] = True
                    a[2 * d] += t[first].sum(); a[2 * d + 1] += t[last].sum()
                on = dom | ~(np.abs(dd) < 1e-10)
                sign = np.where(dd > 0, 1.0, np.where(dd < 0, -1.0, 0.0))
                if l == 0:
                    e = np.zeros(t.shape); e[first] = 1.0; e[last] = -1.0
                    sign = np.where((dd == 0) & (mh > 0), e, sign)
                a[4 + d] += (np.where(on, sign, 0.0) * t).sum()
            a[6] += (np.where(m[1:-1, 1:-1] > 0, B[1:-1, 1:-1], 0.0) * L.dx * L.dy).sum()
        out.append(a)
    return out, t_copy


def one_call():
    """--one-call: the series of one run, printed as the reference prints its post_proc block; --time: against the per-call loop"""
    nstep = int(argv[1]) if len(argv) > 1 else 5
    if hier:
        nb = int(argv[0]) if argv else 256
        bc, ph, mm, mo = sy.multimoulins_setup()
        boxes = generated_boxes(nb, bc, ph, mm, mo) if generated else sy.boxes_around(mo["positions"], nb, nb, 4, 1.0e5, 1.0e5)
        def make():
            M = model.HipHierModel(nb, nb, 1.0e5 / nb, 1.0e5 / nb, bc, ph, mm, boxes, max_box=64)
            M.set_states(sy.mountain_amrm_states(nb, nb, boxes))
            return M
        run = lambda M: M.run(nstep, mm["dt"], moulins=mo, balance_every=1)
        def loop(M):
            M.moulin_source(**mo)
            for n in range(nstep):
                if n > 0:
                    M.mass_balance()
                M.timestep(mm["dt"])
                M.mass_balance()
        series = lambda M: (M.last_run["budget"], M.last_run["budget_nlev"])
        counters = lambda M: dict(budget_launches=M.hier.get_option("budget_launches"), budget_copies=M.hier.get_option("budget_copies"),
                                  balance_copies=M.hier.get_option("balance_copies"), run_readbacks=M.hier.get_option("run_readbacks"))
        dt, ramp = mm["dt"], mm.get("ramp", 1.0)
    else:
        m = sy.A3_MODEL
        nx = int(argv[0]) if argv else m["nx"]
        ny = max(nx // 5, 4)
        st = sy.shmip_initial_state(nx, ny, m["lx"], m["ly"])
        def make():
            M = model.HipBatchModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, [m], max_box=64)
            M.set_state(0, st)
            return M
        run = lambda M: M.run(nstep, m["dt"], balance_every=1)
        def loop(M):
            for n in range(nstep):
                if n > 0:
                    M.mass_balance_all()
                M.timestep(m["dt"])
                M.mass_balance_all()
        series = lambda M: (M.last_run["budget"], np.ones(M.last_run["budget_rows"], dtype=int))
        counters = lambda M: dict(batch_launches=M.get_option("batch_launches"), batch_readbacks=M.get_option("batch_readbacks"))
        dt, ramp = m["dt"], m.get("ramp", 1.0)
    if timing:
        for r in range(3):
            for name, fn in (("one call with the series", run), ("per-call loop", loop)) if r % 2 == 0 else (("per-call loop", loop), ("one call with the series", run)):
                M = make()
                t0 = time.perf_counter()
                fn(M)
                print("round %d, %-24s: %d steps in %.3f ms; %s" % (r, name, nstep, 1e3 * (time.perf_counter() - t0), counters(M)), flush=True)
                M.close()
        return
    M = make()
    run(M)
    rows, nlev = series(M)
    for n in range(rows.shape[0]):
        for l in range(int(nlev[n])):
            v = dict(zip(capi.WB_NAMES, rows[n, l].tolist()))
            print("step %d level %d" % (n + 1, l))
            print("\n".join(lines(v, dict(volume=v["volume_old"]))))
        v = dict(zip(capi.WB_NAMES, rows[n, 0].tolist()))
        print("Time(months) VOL_waterTot rechargeTOT ramp = %g %g %g %g" % ((n + 1) * dt / 2635200.0, v["volume"], v["recharge_ext"] + v["recharge_melt"], ramp))
    v = dict(zip(capi.WB_NAMES, rows[-1, 0].tolist()))
    inflow = v["lo_x"] + v["lo_y"] - v["hi_x"] - v["hi_y"]
    r = v["recharge_ext"] + v["recharge_melt"]
    print("level 0, last step: (V - Vold) / dt = %.6e m^3/s; recharge %.6e + inflow through the domain sides %.6e = %.6e m^3/s"
          % ((v["volume"] - v["volume_old"]) / dt, r, inflow, r + inflow))
    M.close()


def main():
    if "--one-call" in sys.argv:
        return one_call()
    nstep = int(argv[1]) if len(argv) > 1 else (3 if timing else 5)
    M, levels, dt, balance, recharge, bc = setup()
    sync = levels[0][0].synchronize
    if timing:
        if hier:
            for _ in range(nstep):
                M.timestep(dt)
        else:
            M.level.update_operator()                         # the face coefficients of the state as loaded: a 4096^2 level needs no step to be timed
        nbx = sum(len(bl) for bl in levels)
        H = M.hier if hier else None
        print("mass balance: boxes per level %s, %d handles, %s cells" % ([len(bl) for bl in levels], nbx, [sum(L.nx * L.ny for L in bl) for bl in levels]), flush=True)
        balance(); host_route(levels, bc)                     # (the first calls allocate)
        def call():
            n = (H.get_option("balance_launches"), H.get_option("balance_copies")) if H else (0, 0)
            v = balance()
            c = "%d launches, %d copy" % (H.get_option("balance_launches") - n[0], H.get_option("balance_copies") - n[1]) if H else "2 launches, 1 copy"
            return "%s; level 0: volume %.17g, dirX %.17g" % (c, v[0]["volume"], v[0]["dir_x"])
        def route():
            t0 = time.perf_counter()
            v, t_copy = host_route(levels, bc)
            return "%d get calls %.3f ms, numpy %.3f ms; level 0: volume %.17g, dirX %.17g" % (5 * nbx, 1e3 * t_copy, 1e3 * (time.perf_counter() - t0 - t_copy), v[0][6], v[0][4])
        def settle():
            # one small reduction and its read-back before a clock starts: timed right behind the several hundred pageable 2-D copies of the get
            # route, the call took 22 - 25 ms instead of 0.08 (profiles/r23_balance.txt); whose time that is was not looked for
            t0 = time.perf_counter()
            levels[0][0].norm(lv.F_PHI)
            sync()
            return 1e3 * (time.perf_counter() - t0)
        for r in range(3):
            for name, fn in (("the call", call), ("per-box get + numpy", route)) if r % 2 == 0 else (("per-box get + numpy", route), ("the call", call)):
                ts = settle()
                t0 = time.perf_counter()
                what = fn()
                sync()
                print("round %d, %-19s: %.3f ms in all (the reduction before the clock: %.3f ms), %s" % (r, name, 1e3 * (time.perf_counter() - t0), ts, what), flush=True)
            settle()
            t0 = time.perf_counter()
            for _ in range(20):
                balance()
            print("round %d, 20 calls in a row  : %.3f ms per call" % (r, 1e3 * (time.perf_counter() - t0) / 20), flush=True)
        M.close()
        return
    old = new = None
    for n in range(nstep):
        if n > 0:
            old = balance()                                   # Bold: the volume of the state before the step
        M.timestep(dt)
        new = balance()
        if old is None:
            old = new                                         # (before the first step no face coefficients exist: the call is refused)
        for l, (v, vo) in enumerate(zip(new, old)):
            print("step %d level %d" % (n + 1, l))
            print("\n".join(lines(v, vo)))
    v, vo = new[0], old[0]
    inflow = v["lo_x"] + v["lo_y"] - v["hi_x"] - v["hi_y"]
    r = recharge()
    print("level 0, last step: (V - Vold) / dt = %.6e m^3/s; recharge %.6e + inflow through the domain sides %.6e = %.6e m^3/s"
          % ((v["volume"] - vo["volume"]) / dt, r, inflow, r + inflow))
    M.close()


if __name__ == "__main__":
    main()
