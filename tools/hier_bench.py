#!/usr/bin/env python3
"""cfg5 (exec/AMR_multiMoulins physics) time step on base + 3 AMR levels of box unions: ms per step.
    python tools/hier_bench.py [--generated-grids] [base cells per side] [steps]
--generated-grids: the hierarchy is made the reference's way instead of synthetic.boxes_around -- a level per pass of the initGrids loop, by tagging
the moulin source term on the device (suhmo_hier_tag_cells) and clustering the tags (suhmo_grids_generate) with run_C_3lev's fill_ratio,
block_factor, max_box_size, nestingRadius and tags_grow; the time of tagging, copy-out and generation is reported per level."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suhmo_amd import model, synthetic as sy
generated = "--generated-grids" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--generated-grids"]
nb = int(argv[0]) if len(argv) > 0 else 256
nstep = int(argv[1]) if len(argv) > 1 else 10
bc, ph, mm, mo = sy.multimoulins_setup()


def generated_boxes():
    """three passes of the initGrids loop.  Tagged: the moulin source term above a fraction of its peak on level 0 that rises with the level
    (0.01, 0.1, 0.5: the refined region narrows level by level, as boxes_around's radii do), buffered by tags_grow = 4; exec/AMR_multiMoulins/
    run_C_3lev/input.hydro:67-76 for the rest"""
    params = dict(fill_ratio=0.5, block_factor=2, max_box_size=64, nesting_radius=4)
    boxes = []
    for _ in range(3):
        M = model.HipHierModel(nb, nb, 1.0e5 / nb, 1.0e5 / nb, bc, ph, mm, boxes, max_box=64)
        M.moulin_source(**mo)
        peak = float(M.get(0, 0, "msrc").max())
        maps = []
        for l in range(len(boxes) + 1):
            M.level[0][0].synchronize()
            t0 = time.perf_counter()
            M.tag_cells(l, "msrc", (0.01, 0.1, 0.5)[l] * peak, 1.0e300, grow=4, granularity=params["block_factor"] // 2)
            M.level[0][0].synchronize()
            t1 = time.perf_counter()
            maps.append(M.tags(l))
            t2 = time.perf_counter()
            print("  pass %d level %d: tagging %.3f ms, copy-out of %d x %d entries %.3f ms, %d entries set" % (len(boxes) + 1, l, 1e3 * (t1 - t0),
                  maps[-1].shape[1], maps[-1].shape[0], 1e3 * (t2 - t1), int(maps[-1].sum())), flush=True)
        t0 = time.perf_counter()
        new = model.generate_grids(nb, nb, bc["periodic"], maps, **params)
        print("  pass %d: generation of %d levels %.3f ms, boxes per level %s" % (len(boxes) + 1, len(new), 1e3 * (time.perf_counter() - t0), [len(b) for b in new]), flush=True)
        M.close()
        if len(new) <= len(boxes):
            break
        boxes = new
    return boxes


boxes = generated_boxes() if generated else sy.boxes_around(mo["positions"], nb, nb, 4, 1.0e5, 1.0e5)
sts = sy.mountain_amrm_states(nb, nb, boxes)
t0 = time.perf_counter()
H = model.HipHierModel(nb, nb, sts[0][0]["dx"], sts[0][0]["dy"], bc, ph, mm, boxes, max_box=64)
H.set_states(sts)
H.moulin_source(**mo)
print("setup %.2f s, boxes per level %s, cells %s" % (time.perf_counter() - t0, [len(b) for b in boxes],
      [sum((b[2] - b[0] + 1) * (b[3] - b[1] + 1) for b in bl) for bl in boxes]), flush=True)
for _ in range(3):
    H.timestep(mm["dt"])
H.level[0][0].synchronize()
if os.environ.get("SUHMO_TIMERS"):
    from suhmo_amd import capi
    capi.lib().suhmo_timers_reset()
t0 = time.perf_counter()
c = [H.timestep(mm["dt"]) for _ in range(nstep)]
H.level[0][0].synchronize()
dt = (time.perf_counter() - t0) / nstep
print("base %d^2: %.2f ms per step, Picard %.1f, V-cycles %.1f per step" % (nb, 1e3 * dt, sum(a for a, _ in c) / nstep, sum(b for _, b in c) / nstep))
if os.environ.get("SUHMO_TIMERS"):            # named scopes (mode 2: device time per scope; serialises)
    from suhmo_amd import capi
    print(capi.timers_report())
H.close()
