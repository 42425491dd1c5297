#!/usr/bin/env python3
"""bench.py's single-GPU workload (SHMIP-A head solve, 4096^2 cells, V-cycles timed after a warm-up) on a SLOPING bed: shmip_fields with
slope = 1e-3, so that zb varies from column to column and the level's scan of the bed (level option zb_known) answers `varying` -- every
streaming launch keeps loading the array, as it does for any level whose bed is not one value.  Prints one JSON line with ms per V-cycle, what
the level found out about the bed and how many launches took it as a scalar (0 here).  SUHMO_LIB selects the build, as for bench.py.
usage: python tools/bench_varying_bed.py [--steps 20] [--warmup 3] [--cells 4096] [--slope 1e-3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LX = 1.0e5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cells", dest="n", type=int, default=4096)
    ap.add_argument("--slope", type=float, default=1e-3)
    args = ap.parse_args()
    from suhmo_amd import capi, level, synthetic as sy
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no CPU fallback"
    n = args.n
    f = sy.shmip_fields(n, n, ly=LX, slope=args.slope)
    G = level.HipLevel(n, n, f["dx"], f["dy"], sy.A3_BC, sy.A3_PHYS, max_box=64)
    G.set_inputs(f)
    G.build_mg_coefficients()
    sp = dict(sy.SOLVER_DEFAULT)
    for _ in range(args.warmup):
        G.vcycle(sp)
    G.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        G.vcycle(sp)
    G.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / args.steps
    out = {"workload": "SHMIP-A head solve, %dx%d cells, bed slope %g" % (n, n, args.slope), "ms_per_step": ms, "steps": args.steps, "warmup": args.warmup}
    try:                                   # (a build from before the option has no such keys)
        out["zb_state"] = G.get_option("zb_state"); out["relax_zb_uniform_launches"] = G.get_option("relax_zb_uniform_launches")
    except Exception:
        out["zb_state"] = out["relax_zb_uniform_launches"] = None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
