#!/usr/bin/env python3
"""The reference's input.hydro_pp workflow (exec/AMR_multiMoulins/run_C_*lev): restart from a checkpoint, take one step with
post_proc_comparisons = true and max_level = N, and write gap height and effective pressure N = Pi - Pw of the whole hierarchy on the uniform
grid of level N into <prefix>Custom<step>.2d.hdf5 (AmrHydro::interpFinest + writePltPP, src/AmrHydro.cpp:4623-4829, 5298-5389) -- the file
an AMR run is compared with the uniform run and with other AMR depths by.
    python tools/interp_finest.py CHK --max-level N [--steps 1] [--prefix plot]
The command line runs the cfg5 physics (exec/AMR_multiMoulins; synthetic.multimoulins_setup) on the grids of the checkpoint; interp_finest()
below takes any model factory."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def interp_finest(chk, make_model, max_level, dt, steps=1, prefix="plot", before_step=None):
    """chk: a checkpoint file (suhmo_amd.checkpoint); make_model(boxes, level0) -> a HipHierModel on the checkpoint's boxes (level0: dx, dy,
    domain of level 0 as checkpoint.read_levels gives them); before_step(model): the forcing of a step (the moulin source), or None.
    -> (path of the file written, the (2, nyF, nxF) array in it, the model: the caller closes it)"""
    from suhmo_amd import checkpoint, plotfile
    hdr, levels = checkpoint.read_levels(chk)
    M = make_model([lev["boxes"] for lev in levels[1:]], levels[0])
    checkpoint.restart(chk, M)
    for _ in range(int(steps)):
        if before_step is not None:
            before_step(M)
        M.timestep(dt)
    path = plotfile.pp_name(prefix, M.cur_step)
    a = plotfile.write_pp(path, M, hdr["time"] + int(steps) * dt, max_level)
    return path, a, M


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("chk")
    ap.add_argument("--max-level", type=int, required=True)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--prefix", default="plot")
    a = ap.parse_args()
    from suhmo_amd import model, synthetic as sy
    bc, ph, mm, mo = sy.multimoulins_setup()

    def make(boxes, level0):
        d = level0["domain"]
        return model.HipHierModel(d[2] + 1, d[3] + 1, level0["dx"], level0["dy"], bc, ph, mm, boxes, max_box=64)

    path, arr, M = interp_finest(a.chk, make, a.max_level, mm["dt"], a.steps, a.prefix, lambda m: m.moulin_source(**mo))
    print("%s: step %d, %d levels -> gapHeight and N on %d x %d cells (level %d)" % (path, M.cur_step, M.hier.nlev, arr.shape[2], arr.shape[1], a.max_level))
    M.close()


if __name__ == "__main__":
    main()
