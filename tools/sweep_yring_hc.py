#!/usr/bin/env python3
"""Chunk heights of the plain streaming launch with one ring of y-faces (level option yface_ring), on bench.py's single-GPU workload: one
level, one process; for every height the option fused_hc is set (it holds for every streaming launch of every depth) and some V-cycles are
timed.  The cycle time is confounded by the other launches' chunks, so run it under `rocprofv3 --kernel-trace` and reduce the trace with
tools/stats_by_grid.py: the launch's rows are told apart by their grids, which this script prints per height (64 work-items per workgroup,
strips x chunks workgroups).  The first and the last block run the automatic heights with yface_ring = 0 and 1.
usage: python tools/sweep_yring_hc.py [--cells 4096] [--cycles 10] [--heights 13,14,16,...]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LX = 1.0e5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", dest="n", type=int, default=4096)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--heights", default="13,14,16,17,18,19,22,40,44,48,52,56,60,64,71")
    args = ap.parse_args()
    from suhmo_amd import capi, level, synthetic as sy
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no CPU fallback"
    n = args.n
    f = sy.shmip_fields(n, n, ly=LX)
    G = level.HipLevel(n, n, f["dx"], f["dy"], sy.A3_BC, sy.A3_PHYS, max_box=64)
    G.set_inputs(f)
    G.build_mg_coefficients()
    sp = dict(sy.SOLVER_DEFAULT)
    for _ in range(3):
        G.vcycle(sp)
    G.synchronize()

    def timed(yring, hc):
        G.set_option("yface_ring", yring); G.set_option("fused_hc", hc)
        G.vcycle(sp); G.synchronize()
        before = G.get_option("relax_yring_launches")
        t0 = time.perf_counter()
        for _ in range(args.cycles):
            G.vcycle(sp)
        G.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / args.cycles
        grids = {}
        for d in (0, 1):                   # the plain launch: 2K = 4 halo columns per side of a strip of 128
            nx = n >> d
            strips = -(-nx // 120)
            w = 2 * (-(-nx // (2 * strips)))
            strips = -(-nx // w)
            grids["d%d" % d] = 64 * strips * -(-nx // hc) if hc else None
        print(json.dumps({"yface_ring": yring, "fused_hc": hc, "ms_per_vcycle": round(ms, 4), "plain_launch_grid": grids,
                          "relax_yring_launches": G.get_option("relax_yring_launches") - before}), flush=True)

    timed(0, 0)
    for hc in [int(h) for h in args.heights.split(",")]:
        timed(1, hc)
    timed(1, 0)
    timed(0, 0)


if __name__ == "__main__":
    main()
