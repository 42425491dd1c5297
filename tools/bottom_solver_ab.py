#!/usr/bin/env python3
"""A/B of the bottom solver (level option bottom_solver: 0 = the numBottom relaxes only, 1 = followed by RelaxSolver, suhmo_bottom.hip).
One line per configuration and setting: V-cycles, wall ms with the device synchronised, bottom-solver iterations per V-cycle, and how
the bottoms ran (one launch / host loop).  Configurations:
    tutorial-50      the tutorial run (exec/0_convergence_channelized/1lev, 32 x 8), its first 50 time steps
    shmip-a3-step    one SHMIP A3 time step (320 x 64, max_box 64) from the initial state
    solve-N-boxB     suhmo_level_solve at N^2 from SHMIP-A's initial head to the step >= 50 tolerances (bench.py's converged_solve),
                     with 64^2 boxes and with max_box = the level
usage: python tools/bottom_solver_ab.py [--sizes 1024,4096] [--only tutorial,a3,solve]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from suhmo_amd import synthetic as sy


def counters(L):
    return [L.get_option(k) for k in ("bottom_solver_iterations", "bottom_solves_one_launch", "bottom_solves_host_loop")]


def line(name, bottom, vcycles, ms, c0, c1, extra=""):
    it, one, host = (b - a for a, b in zip(c0, c1))
    print("%-26s bottom_solver=%d  vcycles %5d  wall %10.2f ms  bottom iterations/vcycle %6.2f  one-launch %5d  host-loop %5d%s"
          % (name, bottom, vcycles, ms, it / max(vcycles, 1), one, host, extra), flush=True)


def tutorial(bottom, steps=50):
    import convergence_channelized as cc
    from oracle import pyoracle as po
    from suhmo_amd import model
    nx, ny = 32, 8
    st, m = cc.basic_state(nx, ny), dict(cc.MODEL)
    src, _ = po.moulin_source(nx, ny, st["dx"], st["dy"], cc.MOULIN[0], cc.MOULIN[1], cc.MOULIN[2], 1.0)
    M = model.HipModel(nx, ny, st["dx"], st["dy"], cc.BC, cc.PHYS, m, max_box=8)
    M.level.set_option("bottom_solver", bottom)
    M.set_state(st)
    M.level.set(model.lv.F_MR, np.full((ny, nx), m["G"] / m["L"]))
    M.level.set(model.lv.F_MSRC, src)
    c0 = counters(M.level)
    M.level.synchronize()
    t0 = time.perf_counter()
    pv = []
    for k in range(steps):
        M._mp.ramp = float(cc.ramp(k * m["dt"]))
        pv.append(M.timestep(m["dt"]))
    M.level.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    pv = np.array(pv)
    line("tutorial-%d" % steps, bottom, int(pv[:, 1].sum()), ms, c0, counters(M.level),
         "  (first step: %d Picard, %d V-cycles)" % (pv[0, 0], pv[0, 1]))
    M.close()


def a3_step(bottom):
    from suhmo_amd import model
    m = dict(sy.A3_MODEL)
    st = sy.shmip_initial_state(m["nx"], m["ny"])
    M = model.HipModel(m["nx"], m["ny"], st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=64)
    M.level.set_option("bottom_solver", bottom)
    M.set_state(st)
    M.level.set(model.lv.F_MR, np.full((m["ny"], m["nx"]), m["G"] / m["L"]))
    c0 = counters(M.level)
    M.level.synchronize()
    t0 = time.perf_counter()
    p, v = M.timestep(m["dt"])
    M.level.synchronize()
    line("shmip-a3-step", bottom, v, 1e3 * (time.perf_counter() - t0), c0, counters(M.level), "  (%d Picard)" % p)
    M.close()


def solve(bottom, n, mb):
    from suhmo_amd import level
    f = sy.shmip_fields(n, n, ly=1.0e5)
    f.pop("bx", None); f.pop("by", None)
    sp = dict(sy.SOLVER_DEFAULT)
    L = level.HipLevel(n, n, f["dx"], f["dy"], sy.A3_BC, sy.A3_PHYS, max_box=mb)
    L.set_option("bottom_solver", bottom)
    L.set_inputs(f); L.build_mg_coefficients()
    c0 = counters(L)
    L.synchronize()
    t0 = time.perf_counter()
    it, hist = L.solve(sp)
    L.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    conv = hist[-1] <= sp["norm_thresh"] or hist[-1] <= sp["eps"] * hist[0]
    bottom_n = n >> (L.ndepth - 1)
    line("solve-%d-box%s" % (n, "level" if mb == n else mb), bottom, it, ms, c0, counters(L),
         "  (bottom %d^2, residual %.3e -> %.3e, %s)" % (bottom_n, hist[0], hist[-1], "converged" if conv else "NOT converged"))
    L.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--only", default="tutorial,a3,solve")
    args = ap.parse_args()
    only = args.only.split(",")
    for bottom in (0, 1):
        if "tutorial" in only:
            tutorial(bottom)
        if "a3" in only:
            a3_step(bottom)
        if "solve" in only:
            for n in (int(s) for s in args.sizes.split(",")):
                for mb in (64, n):
                    solve(bottom, n, mb)


if __name__ == "__main__":
    main()
