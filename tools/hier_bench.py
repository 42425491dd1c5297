#!/usr/bin/env python3
"""cfg5 (exec/AMR_multiMoulins physics) time step on base + 3 AMR levels of box unions: ms per step.
    python tools/hier_bench.py [--generated-grids] [--regrid-interval N [--device-ibc] [--one-call [--plot-interval P] [--balance-every B]]] [--recharge] [--snapshot] [--flatten] [--compare] [base cells per side] [steps]
--compare: the L1, L2 and max norms of the reference's two components against a single level on the uniform grid of level 4 (random fields), on the
hierarchy --flatten uses: suhmo_hier_compare in both modes (HipHier.compare: composite, finest), in alternating rounds with the two routes that
existed before it -- one flatten to the host and the norms in numpy; the per-box get calls and, box by box, the block means and norms in numpy
(either with the time of its copies and of its host arithmetic apart) -- with the launch and copy counts.
--flatten: gap height and N = Pi - Pw of the hierarchy on the uniform grid of level 4 (HipHierModel.interp_finest's call, suhmo_hier_flatten), three
repetitions: the time of the kernels and of the copy to the host separately (the library's named timers with the device synchronised around either
part), the launch and copy counts -- and, alternating with it, the per-box get calls that bring the same fields to the host (their count and time
only: the host arithmetic that would follow is no baseline).
--plot-interval P (with --one-call): the runs of HipHierModel.run also write a plot file before every step c with (c - 1) % P == 0 (suhmo_hier_run_out:
one snapshot and one file per event, into a temporary directory); the per-call loop beside it writes none, so the difference is what the output costs.
--snapshot: one 13-component snapshot of the hierarchy (suhmo_hier_snapshot: a launch and a copy per level) against the per-box get loop for the same
data (a copy per box and field), three alternating rounds, with the launch and copy counts of both.
--balance-every B (with --one-call): both loops also take the water budget of every level after every B-th step ("WATER BUDGET", include/suhmo_hip.h):
the one call as the series inside the run (no copy and no synchronisation per row, one copy per run call), the per-call loop with mass_balance
before the step (Bold) and water_budget after it.
--device-ibc (with --regrid-interval N): the same regridding time loop on two models set up alike -- one whose regrids call the host `reload` (the
dino's initializePi and setup_iceMask in numpy on every new box, pushed through the per-box set calls), one with the IBC on the handle
(HipHierModel.set_ibc: the reload runs on the device inside suhmo_hier_regrid) -- and the time per grid-changing regrid of either, the regrid call
with its reload between two synchronisations.  The two routes differ in the ghost cells (the host route loads the formula's, the device route
fills them as the reference does), so the states are not compared.  The callback writes the dino's b = 1e-16 only on boxes where Pi == 0 occurs, which
is none on this domain; the device body tests every cell.
--one-call (with --regrid-interval N): the same regridding time loop twice in one process, on two models set up alike -- the per-call loop
(HipHierModel.tag_and_regrid, moulin_source, timestep) and HipHierModel.run (suhmo_hier_run: one call per stretch of steps that begins with a
regrid, so that the thresholds can alternate as below) -- in alternating rounds of [steps] steps; prints ms per step and ms per regrid interval of
either for every round and the spread over the rounds, and compares the two models' fields bit for bit at the end.
--regrid-interval N: the time loop regrids every N steps as AmrHydro::regrid does (HipHierModel.tag_and_regrid's body, with the per-level tag
thresholds of --generated-grids; the thresholds alternate between two sets, so that every regrid moves boxes) and prints, per regrid, the times of
tagging, clustering, hierarchy creation, the transfer's plans and launches, the moulin source term on the new boxes and the steps around it --
and, for the first regrid, what the same move costs through the host (all fields read back, the interpolation in numpy, a new model created and
loaded: what a caller can do without suhmo_hier_regrid), its valid cells compared with the device's bit for bit.
--recharge: instead of stepping, the seasonal recharge on the hierarchy's boxes: HipHierModel.time_varying_recharge (suhmo_hier_time_varying_recharge,
one launch per level) against suhmo_level_time_varying_recharge on every box handle, 50 evaluations between two synchronisations, three alternating
repetitions (with --generated-grids 256: run_C_3lev's 42 + 56 + 59 boxes).
--generated-grids: the hierarchy is made the reference's way instead of synthetic.boxes_around -- a level per pass of the initGrids loop, by tagging
the moulin source term on the device (suhmo_hier_tag_cells) and clustering the tags (suhmo_grids_generate) with run_C_3lev's fill_ratio,
block_factor, max_box_size, nestingRadius and tags_grow; the time of tagging, copy-out and generation is reported per level."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suhmo_amd import model, synthetic as sy
generated = "--generated-grids" in sys.argv
one_call = "--one-call" in sys.argv
device_ibc = "--device-ibc" in sys.argv
recharge = "--recharge" in sys.argv
snapshot = "--snapshot" in sys.argv
flatten = "--flatten" in sys.argv
compare = "--compare" in sys.argv
argv = [a for a in sys.argv[1:] if a not in ("--generated-grids", "--one-call", "--device-ibc", "--recharge", "--snapshot", "--flatten", "--compare")]
balance_every = 0
if "--balance-every" in argv:
    q = argv.index("--balance-every")
    balance_every = int(argv[q + 1])
    del argv[q:q + 2]
plot_interval = -1
if "--plot-interval" in argv:
    q = argv.index("--plot-interval")
    plot_interval = int(argv[q + 1])
    del argv[q:q + 2]
regrid_interval = 0
if "--regrid-interval" in argv:
    q = argv.index("--regrid-interval")
    regrid_interval = int(argv[q + 1])
    del argv[q:q + 2]
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


GRID_PARAMS = dict(fill_ratio=0.5, block_factor=2, max_box_size=64, nesting_radius=4)
REGRID_FIELDS = ("head", "B", "Pi", "zb", "mask", "mR", "Pw", "zs")


def host_interp(c, periodic):
    """rule (a) of "REGRID: FIELD TRANSFER" (include/suhmo_hip.h) for every cell of the full-domain array c of a level (NaN where the level has no
    cell), vectorised: the four children as one array of twice the size.  The statements of tests/regrid_ref.py, array by array"""
    import numpy as np
    ny, nx = c.shape
    p = np.pad(c, 1, constant_values=np.nan)
    if periodic[0]:
        p[1:-1, 0], p[1:-1, -1] = c[:, -1], c[:, 0]
    if periodic[1]:
        p[0, :], p[-1, :] = p[-2, :].copy(), p[1, :].copy()
    nb = lambda a, b: p[1 + b:1 + b + ny, 1 + a:1 + a + nx]
    W, E, S, N = nb(-1, 0), nb(1, 0), nb(0, -1), nb(0, 1)
    xl, xh, yl, yh = ~np.isnan(W), ~np.isnan(E), ~np.isnan(S), ~np.isnan(N)
    with np.errstate(invalid="ignore", divide="ignore"):
        s0 = np.where(xl & xh, 0.5 * (E - W), np.where(xh, E - c, np.where(xl, c - W, 0.0)))
        s1 = np.where(yl & yh, 0.5 * (N - S), np.where(yh, N - c, np.where(yl, c - S, 0.0)))
        smax, smin = c.copy(), c.copy()
        for b in (-1, 0, 1):
            for a in (-1, 0, 1):
                smax, smin = np.fmax(smax, nb(a, b)), np.fmin(smin, nb(a, b))
        ds = 0.5 * (np.abs(s0) + np.abs(s1))
        eta = np.maximum(np.minimum(np.minimum((c - smin) / ds, (smax - c) / ds), 1.0), 0.0)
        cut = ds > 0.0
        s0 = np.where(cut & xl & xh, eta * s0, s0)
        s1 = np.where(cut & yl & yh, eta * s1, s1)
    out = np.empty((2 * ny, 2 * nx))
    for q in (0, 1):
        for pp in (0, 1):
            v = c + s0 * (0.25 if pp else -0.25)
            out[q::2, pp::2] = v + s1 * (0.25 if q else -0.25)
    return out


def host_round_trip(H, new_boxes):
    """the same regrid without suhmo_hier_regrid: read back, interpolate and copy in numpy (valid cells only: the ghost fills are left out, in the
    host's favour), create a model on the new boxes and load it.  -> (times, the new model)"""
    import numpy as np
    from suhmo_amd import level as lv
    ids = dict(H.FIELDS, zs=lv.F_ZS)
    t = {}
    t0 = time.perf_counter()
    old = {nm: [[L.get(ids[nm], ghosted=True) for L in bl] for bl in H.level] for nm in REGRID_FIELDS}
    t["read back"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    new = {}
    for nm in REGRID_FIELDS:
        coarse, per_level = old[nm][0][0][1:-1, 1:-1], []
        for l, bl in enumerate(new_boxes, start=1):
            full = host_interp(coarse, bc["periodic"])
            keep = np.zeros(full.shape, dtype=bool)
            for b in bl:
                keep[b[1]:b[3] + 1, b[0]:b[2] + 1] = True
            full[~keep] = np.nan
            if l < len(H.level):
                for b, a in zip(H.hier.boxes[l - 1], old[nm][l]):
                    m = keep[b[1]:b[3] + 1, b[0]:b[2] + 1]
                    full[b[1]:b[3] + 1, b[0]:b[2] + 1][m] = a[1:-1, 1:-1][m]
            per_level.append([np.ascontiguousarray(full[b[1]:b[3] + 1, b[0]:b[2] + 1]) for b in bl])
            coarse = full
        new[nm] = per_level
    t["numpy"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    M = model.HipHierModel(nb, nb, 1.0e5 / nb, 1.0e5 / nb, bc, ph, mm, new_boxes, max_box=64)
    t["create"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    for nm in REGRID_FIELDS:
        M.level[0][0].set(ids[nm], old[nm][0][0], ghosted=True)
        for l, bl in enumerate(new_boxes, start=1):
            for k in range(len(bl)):
                M.level[l][k].set(ids[nm], new[nm][l - 1][k])
    M.level[0][0].synchronize()
    t["load"] = time.perf_counter() - t0
    return t, M, new


def timed_regrid(H, n, first):
    """the body of HipHierModel.tag_and_regrid with a clock around every part"""
    from suhmo_amd import capi, level as lv
    sync = lambda: H.level[0][0].synchronize()          # (the views change hands with the regrid)
    peak = float(H.get(0, 0, "msrc").max())
    scale = (1.0, 0.6)[n % 2]
    sync(); t0 = time.perf_counter()
    H.clear_tags()
    for l in range(min(H.hier.nlev, 3)):
        H.tag_cells(l, "msrc", scale * (0.01, 0.1, 0.5)[l] * peak, 1.0e300, grow=4, granularity=GRID_PARAMS["block_factor"] // 2)
    sync(); t1 = time.perf_counter()
    new, same = H.generate_grids(**GRID_PARAMS)
    t2 = time.perf_counter()
    host = None
    if first and not same:
        host = host_round_trip(H, new)
    t_host = time.perf_counter() - t2
    # (mode 1: host wall time per scope; both scopes end with a synchronisation of their own)
    capi.lib().suhmo_timers_enable(1); capi.lib().suhmo_timers_reset()
    t3 = time.perf_counter()
    if not same:
        H.regrid(new)
    sync(); t4 = time.perf_counter()
    rep = capi.timers_report(); capi.lib().suhmo_timers_enable(0)
    scope = {}
    for line in rep.splitlines():
        q = line.rsplit(None, 3)
        if len(q) == 4 and q[0].startswith("regrid:"):
            scope[q[0]] = 1e3 * float(q[2])
    H.moulin_source(**mo)
    sync(); t5 = time.perf_counter()
    print("regrid %d: same %s, boxes per level %s | tagging %.3f ms, clustering (copy-out + generation) %.3f ms, regrid call %.3f ms "
          "(hierarchy creation %.3f ms, transfer plans + launches %.3f ms, old hierarchy destroyed %.3f ms), moulin source on the new boxes %.3f ms"
          % (n, same, [len(b) for b in new], 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t4 - t3),
             scope.get("regrid: hierarchy creation (boxes, plans, tables)", 0.0), scope.get("regrid: transfer plans and launches", 0.0),
             scope.get("regrid: old hierarchy destroyed", 0.0), 1e3 * (t5 - t4)), flush=True)
    if host:
        import numpy as np
        t, M, ref = host
        ids = dict(H.FIELDS, zs=lv.F_ZS)
        eq = all(np.array_equal(H.level[l][k].get(ids[nm]), ref[nm][l - 1][k], equal_nan=True)
                 for nm in REGRID_FIELDS for l, bl in enumerate(new, start=1) for k in range(len(bl)))
        print("  the same move through the host: read back %.3f ms, interpolation and copy in numpy %.3f ms, new model created %.3f ms, loaded %.3f ms: "
              "%.3f ms in all; valid cells bitwise equal to the device's: %s" % (1e3 * t["read back"], 1e3 * t["numpy"], 1e3 * t["create"], 1e3 * t["load"],
              1e3 * sum(t.values()), eq), flush=True)
        M.close()
    return t5 - t0 - t_host, t_host


boxes = generated_boxes() if generated else sy.boxes_around(mo["positions"], nb, nb, 4, 1.0e5, 1.0e5)
sts = sy.mountain_amrm_states(nb, nb, boxes)


def device_ibc_rounds():
    """the regridding loop with the host `reload` and with the IBC on the handle: time per grid-changing regrid"""
    import numpy as np

    def host_reload(l, k, b):
        # MountainIBC::initializePi + setup_iceMask on the ghosted box (src/MountainSetupIBC.cpp:89-108), as a caller's callback evaluates them
        d = 1.0e5 / (nb << l)
        X, Y = np.meshgrid((np.arange(b[0] - 1, b[2] + 2) + 0.5) * d, (np.arange(b[1] - 1, b[3] + 2) + 0.5) * d)
        zs = 2.0 * (1.5e-3 * X + -1.5e-3 * Y + 100.0 + 100.0)
        Pi = sy.RHO_I * sy.GRAV * np.maximum(zs, 0.0)
        f = dict(Pi=np.ascontiguousarray(Pi), zs=np.ascontiguousarray(zs), mask=np.where(Pi > 0.0, 1.0, -1.0))
        if (Pi == 0.0).any():               # b = 1e-16 where Pi == 0 (:105-107): the transferred gap height read back, changed, loaded again.  On this
            f["B"] = np.where(Pi == 0.0, 1.0e-16, M.get(l, k, "B", ghosted=True))      # domain the ice never ends, so no box takes this branch
        return f

    for name in ("host reload", "device IBC"):
        M = model.HipHierModel(nb, nb, sts[0][0]["dx"], sts[0][0]["dy"], bc, ph, mm, boxes, max_box=64)
        M.set_states(sts)
        M.moulin_source(**mo)
        if name == "device IBC":
            M.set_ibc(model.ibc("dino"))
        sync = lambda: M.level[0][0].synchronize()
        peak = float(M.get(0, 0, "msrc").max())
        times, nbox = [], []
        for n in range(nstep):
            M.timestep(mm["dt"])
            if (n + 1) % regrid_interval:
                continue
            scale = (1.0, 0.6)[((n + 1) // regrid_interval) % 2]
            M.clear_tags()
            for l in range(min(M.hier.nlev, 3)):
                M.tag_cells(l, "msrc", scale * (0.01, 0.1, 0.5)[l] * peak, 1.0e300, grow=4, granularity=GRID_PARAMS["block_factor"] // 2)
            new, same = M.generate_grids(**GRID_PARAMS)
            if same:
                continue
            sync(); t0 = time.perf_counter()
            M.regrid(new, reload=host_reload if name == "host reload" else None)
            sync(); times.append(time.perf_counter() - t0)
            nbox.append(sum(len(bl) for bl in new))
            M.moulin_source(**mo)
        print("%-12s: %d grid-changing regrids of %d steps, %s new boxes: %.2f ms per regrid (min %.2f, max %.2f)"
              % (name, len(times), nstep, nbox, 1e3 * sum(times) / max(1, len(times)), 1e3 * min(times or [0.0]), 1e3 * max(times or [0.0])), flush=True)
        M.close()


def one_call_rounds(rounds=3):
    """the regridding loop through the per-call methods and through HipHierModel.run, alternating"""
    import numpy as np
    def setup():
        M = model.HipHierModel(nb, nb, sts[0][0]["dx"], sts[0][0]["dy"], bc, ph, mm, boxes, max_box=64)
        M.set_states(sts)
        M.moulin_source(**mo)
        for _ in range(3):
            M.timestep(mm["dt"])
        M.level[0][0].synchronize()
        return M
    P, R = setup(), setup()
    peak = float(P.get(0, 0, "msrc").max())
    # a tag variable per level (min_level = cap_level = l) with that level's threshold; the two sets alternate from regrid to regrid
    specs = lambda n: [dict(name="msrc", vmin=(1.0, 0.6)[n % 2] * f * peak, vmax=1.0e300, grow=4, min_level=l, cap_level=l) for l, f in enumerate((0.01, 0.1, 0.5))]
    def stretches(M):
        due = model.regrid_steps(M.cur_step + 1, nstep, regrid_interval)
        cuts = [M.cur_step + 1] + [c for c in due if c != M.cur_step + 1] + [M.cur_step + 1 + nstep]
        return due, [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    def per_call(M):
        due, _ = stretches(M)
        moved = 0
        for k in range(nstep):
            c = M.cur_step + 1
            if c in due:
                moved += not M.tag_and_regrid(specs((c - 1) // regrid_interval), GRID_PARAMS, max_level=3)[1]
            if k == 0 or c in due:                 # where the calls of run() below form it: their first step
                M.moulin_source(**mo)
            row = balance_every > 0 and (k + 1) % balance_every == 0
            if row and c not in due:               # (boxes a regrid has just made hold no face coefficients yet)
                M.mass_balance()
            M.timestep(mm["dt"])
            if row:
                M.water_budget()
        return len(due), moved
    import tempfile
    plots = tempfile.TemporaryDirectory() if plot_interval > 0 else None
    out = dict(plot_interval=plot_interval, final_output=False, plot_prefix=os.path.join(plots.name, "plot")) if plots else {}
    written = []
    def run(M):
        due, parts = stretches(M)
        moved = 0
        for c, n in parts:
            log = M.run(n, mm["dt"], moulins=mo, regrid_interval=regrid_interval, tag_specs=specs((c - 1) // regrid_interval), params=GRID_PARAMS, max_level=3,
                        balance_every=balance_every, **out)[3]
            moved += sum(not e["same"] for e in log)
            written.extend(M.last_run.get("plots", []))
        return len(due), moved
    ms = {"per-call loop": [], "one call": []}
    for r in range(rounds):
        for name, fn, M in (("per-call loop", per_call, P), ("one call", run, R)) if r % 2 == 0 else (("one call", run, R), ("per-call loop", per_call, P)):
            M.level[0][0].synchronize()
            t0 = time.perf_counter()
            nreg, moved = fn(M)
            M.level[0][0].synchronize()
            t = time.perf_counter() - t0
            ms[name].append(1e3 * t / nstep)
            print("round %d, %-13s: %.2f ms per step, %.2f ms per interval of %d steps (regrids included: %d, %d moved boxes), boxes per level %s"
                  % (r, name, 1e3 * t / nstep, 1e3 * t / nstep * regrid_interval, regrid_interval, nreg, moved, [len(b) for b in M.hier.boxes]), flush=True)
    for name, v in ms.items():
        print("%-13s: ms per step over the rounds: min %.2f, median %.2f, max %.2f (spread %.2f)" % (name, min(v), sorted(v)[len(v) // 2], max(v), max(v) - min(v)))
    eq = P.hier.boxes == R.hier.boxes and all(np.array_equal(P.get(l, k, nm, ghosted=True), R.get(l, k, nm, ghosted=True), equal_nan=True)
                                              for l, bl in enumerate(P.level) for k in range(len(bl)) for nm in ("head", "B", "mR", "Pw", "msrc"))
    print("the two models after %d steps each: boxes and fields (head, B, mR, Pw, msrc; ghosted) bitwise equal: %s" % (rounds * nstep, eq))
    if plots:
        print("one call: %d plot files written (every %d steps), %.1f MB each, %d snapshot launches, %d snapshot copies"
              % (len(written), plot_interval, os.path.getsize(written[-1]) / 1e6, R.hier.get_option("snapshot_launches"), R.hier.get_option("snapshot_copies")))
        plots.cleanup()
    P.close(); R.close()


def snapshot_bench(rounds=3):
    """one snapshot of the plot file's thirteen components against the per-box get loop for the same data"""
    import numpy as np
    from suhmo_amd import level as lv, plotfile
    M = model.HipHierModel(nb, nb, sts[0][0]["dx"], sts[0][0]["dy"], bc, ph, mm, boxes, max_box=64)
    M.set_states(sts)
    M.moulin_source(**mo)
    for _ in range(3):
        M.timestep(mm["dt"])
    for bl in M.level:                                       # the loop below must not be the one that allocates a field nobody holds yet
        for L in bl:
            for _, _, f in plotfile.COMPONENTS:
                L.get(f, ghosted=f not in (lv.F_QWX, lv.F_QWY))
    sync = M.level[0][0].synchronize
    nbx = sum(len(bl) for bl in M.level)
    flat = np.zeros(M.hier.snapshot(plotfile.SNAP, 1)[2].size)
    print("snapshot: boxes per level %s, %d handles with level 0, 13 components with one ghost cell: %.2f MB" % ([len(b) for b in boxes], nbx, flat.nbytes / 1e6), flush=True)
    def packed():
        M.hier.snapshot(plotfile.SNAP, 1, out=flat)
        return None
    def per_box():
        return [[L.get(f, ghosted=f not in (lv.F_QWX, lv.F_QWY)) for _, _, f in plotfile.COMPONENTS] for bl in M.level for L in bl]
    for r in range(rounds):
        for name, fn in (("one snapshot", packed), ("per-box get loop", per_box)) if r % 2 == 0 else (("per-box get loop", per_box), ("one snapshot", packed)):
            sync()
            n_l, n_c = M.hier.get_option("snapshot_launches"), M.hier.get_option("snapshot_copies")
            t0 = time.perf_counter()
            fn()
            sync()
            t = time.perf_counter() - t0
            counts = ("%d launches, %d copies" % (M.hier.get_option("snapshot_launches") - n_l, M.hier.get_option("snapshot_copies") - n_c) if fn is packed
                      else "no launch, %d copies (one per box and field)" % (13 * nbx))
            print("round %d, %-16s: %.3f ms, %s" % (r, name, 1e3 * t, counts), flush=True)
    M.close()


def flatten_bench(rounds=3, max_level=4):
    """one flatten of the reference's two components against the per-box get calls for the fields it reads"""
    import numpy as np
    from suhmo_amd import capi, level as lv
    M = model.HipHierModel(nb, nb, sts[0][0]["dx"], sts[0][0]["dy"], bc, ph, mm, boxes, max_box=64)
    M.set_states(sts)
    M.moulin_source(**mo)
    for _ in range(3):
        M.timestep(mm["dt"])
    comps = [c for _, c in M.PP_COMPONENTS]
    fields = (lv.F_B, lv.F_PI, lv.F_PW)
    for bl in M.level:                                       # (neither side is the one that allocates a field)
        for L in bl:
            for f in fields:
                L.get(f)
    sync = M.level[0][0].synchronize
    nbx = sum(len(bl) for bl in M.level)
    out = M.hier.flatten(comps, max_level)                   # (the first call allocates the scratch and the finest array)
    print("flatten: boxes per level %s, %d handles with level 0, %d components on %d x %d cells: %.1f MB"
          % ([len(b) for b in boxes], nbx, len(comps), out.shape[2], out.shape[1], out.nbytes / 1e6), flush=True)
    def flat():
        n_l, n_c = M.hier.get_option("flatten_launches"), M.hier.get_option("flatten_copies")
        capi.lib().suhmo_timers_enable(2); capi.lib().suhmo_timers_reset()
        M.hier.flatten(comps, max_level, out=out)
        rep = capi.timers_report(); capi.lib().suhmo_timers_enable(0)
        t = {}
        for line in rep.splitlines():
            q = line.rsplit(None, 3)
            if len(q) == 4 and q[0].startswith("interpFinest:"):
                t[q[0]] = 1e3 * float(q[2])
        return "kernels %.3f ms, copy to the host %.3f ms, %d launches, %d copy" % (
            t.get("interpFinest: evaluation, ghost fills, interpolation", -1.0), t.get("interpFinest: copy to the host", -1.0),
            M.hier.get_option("flatten_launches") - n_l, M.hier.get_option("flatten_copies") - n_c)
    def per_box():
        for bl in M.level:
            for L in bl:
                for f in fields:
                    L.get(f)
        return "no launch, %d copies (one per box and field)" % (len(fields) * nbx)
    for r in range(rounds):
        for name, fn in (("one flatten", flat), ("per-box get calls", per_box)) if r % 2 == 0 else (("per-box get calls", per_box), ("one flatten", flat)):
            sync()
            t0 = time.perf_counter()
            what = fn()
            sync()
            print("round %d, %-17s: %.3f ms in all, %s" % (r, name, 1e3 * (time.perf_counter() - t0), what), flush=True)
    M.close()


def compare_bench(rounds=4, exact_level=4):
    """suhmo_hier_compare, both modes, against flatten + numpy and against the per-box get loop + numpy"""
    import numpy as np
    from suhmo_amd import capi, level as lv
    M = model.HipHierModel(nb, nb, sts[0][0]["dx"], sts[0][0]["dy"], bc, ph, mm, boxes, max_box=64)
    M.set_states(sts)
    M.moulin_source(**mo)
    for _ in range(3):
        M.timestep(mm["dt"])
    comps = [c for _, c in M.PP_COMPONENTS]
    fields = (lv.F_B, lv.F_PI, lv.F_PW)
    nF = nb << exact_level
    dxF = sts[0][0]["dx"] / 2 ** exact_level
    X = lv.HipLevel(nF, nF, dxF, dxF, bc, ph, max_box=64)
    rng = np.random.default_rng(1)
    xh = {}
    for f in fields:                                         # the hierarchy's own range of values, so that no term overflows or vanishes
        a = M.level[0][0].get(f)
        xh[f] = rng.uniform(a.min(), a.max() + 1.0e-12, size=(nF, nF))
        X.set(f, xh[f])
    xc = [xh[lv.F_B], xh[lv.F_PI] - xh[lv.F_PW]]
    sync = M.level[0][0].synchronize
    H = M.hier
    nbx = sum(len(bl) for bl in M.level)
    out = H.flatten(comps, exact_level)                      # (the first calls allocate: scratch, finest array, partial buffer)
    H.compare(X, comps, exact_level, "composite"); H.compare(X, comps, exact_level, "finest")
    allb = [[(0, 0, nb - 1, nb - 1)]] + [list(bl) for bl in H.boxes]
    print("compare: boxes per level %s, %d handles with level 0, %d components against %d x %d exact cells (%.1f MB per field)"
          % ([len(b) for b in boxes], nbx, len(comps), nF, nF, xh[lv.F_B].nbytes / 1e6), flush=True)
    def counted(fn):
        keys = ("compare_launches", "compare_copies", "flatten_launches", "flatten_copies")
        n = [H.get_option(k) for k in keys]
        r = fn()
        return r, "%d + %d launches (compare + flatten), %d + %d copies" % tuple(H.get_option(k) - a for k, a in zip((keys[0], keys[2], keys[1], keys[3]), (n[0], n[2], n[1], n[3])))
    def composite():
        r, c = counted(lambda: H.compare(X, comps, exact_level, "composite"))
        return "%s; gapHeight %s" % (c, r[0])
    def finest():
        r, c = counted(lambda: H.compare(X, comps, exact_level, "finest"))
        return "%s; gapHeight %s" % (c, r[0])
    def norms_of(e, w):
        ae = np.abs(e)
        return np.array([(ae * w).sum(), np.sqrt(((e * e) * w).sum()), ae.max()])
    def flatten_host():
        t0 = time.perf_counter()
        H.flatten(comps, exact_level, out=out)
        t1 = time.perf_counter()
        r = [norms_of(out[q] - xc[q], dxF * dxF) for q in range(len(comps))]
        return "flatten %.3f ms, numpy norms %.3f ms; gapHeight %s" % (1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1), r[0])
    def per_box():
        t0 = time.perf_counter()
        got = [[[L.get(f) for f in fields + (lv.F_COVER,)] for L in bl] for bl in M.level]
        t1 = time.perf_counter()
        acc = np.zeros((len(comps), 3))
        for l, bl in enumerate(allb):
            r = 1 << (exact_level - l)
            w = (dxF * r) * (dxF * r)
            for (lo0, lo1, hi0, hi1), (b, pi, pw, cov) in zip(bl, got[l]):
                for q, c in enumerate((b, pi - pw)):
                    x = xc[q][lo1 * r:(hi1 + 1) * r, lo0 * r:(hi0 + 1) * r].reshape(hi1 - lo1 + 1, r, hi0 - lo0 + 1, r).mean(axis=(1, 3))
                    e = np.where(cov != 0, 0.0, c - x)
                    acc[q] += (np.abs(e).sum() * w, (e * e).sum() * w, 0.0)
                    acc[q, 2] = max(acc[q, 2], np.abs(e).max())
        acc[:, 1] = np.sqrt(acc[:, 1])
        return "%d get calls %.3f ms, numpy block means and norms %.3f ms; gapHeight %s" % (4 * nbx, 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1), acc[0])
    routes = [("compare, composite", composite), ("compare, finest", finest), ("flatten + numpy", flatten_host), ("per-box get + numpy", per_box)]
    for r in range(rounds):
        for name, fn in routes if r % 2 == 0 else routes[::-1]:
            sync()
            t0 = time.perf_counter()
            what = fn()
            sync()
            print("round %d, %-19s: %.3f ms in all, %s" % (r, name, 1e3 * (time.perf_counter() - t0), what), flush=True)
    X.close(); M.close()


def recharge_bench(evals=50, reps=3):
    """the hierarchy's recharge call against the per-box level calls"""
    import numpy as np
    from suhmo_amd import capi
    M = model.HipHierModel(nb, nb, sts[0][0]["dx"], sts[0][0]["dy"], bc, ph, mm, boxes, max_box=64)
    for l, bl in enumerate(M.level):
        for k, L in enumerate(bl):
            M.set_surface(l, k, np.random.default_rng([l, k]).uniform(0.0, 2000.0, size=(L.ny + 2, L.nx + 2)))
    sync, lib = M.level[0][0].synchronize, capi.lib()
    def per_box():
        for bl in M.level:
            for L in bl:
                capi.check(lib.suhmo_level_time_varying_recharge(L.h, 7.5, 1.0e-9, L.stream))
    nbx = sum(len(bl) for bl in M.level)
    print("recharge: boxes per level %s, %d handles with level 0" % ([len(b) for b in boxes], nbx), flush=True)
    for name, fn in (("hierarchy call", lambda: M.time_varying_recharge(7.5, 1.0e-9)), ("per-box calls", per_box)) * reps:
        fn(); sync()
        t0 = time.perf_counter()
        for _ in range(evals):
            fn()
        sync()
        print("%-15s %.3f ms per evaluation of all %d boxes" % (name, 1e3 * (time.perf_counter() - t0) / evals, nbx), flush=True)
    M.close()


if recharge:
    recharge_bench()
    sys.exit(0)
if snapshot:
    snapshot_bench()
    sys.exit(0)
if flatten:
    flatten_bench()
    sys.exit(0)
if compare:
    compare_bench()
    sys.exit(0)
if device_ibc:
    assert regrid_interval > 0, "--device-ibc needs --regrid-interval"
    device_ibc_rounds()
    sys.exit(0)
if one_call:
    assert regrid_interval > 0, "--one-call needs --regrid-interval"
    one_call_rounds()
    sys.exit(0)
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
if regrid_interval:
    c, t_regrid, t_other, t_last = [], 0.0, 0.0, time.perf_counter()
    for n in range(nstep):
        c.append(H.timestep(mm["dt"]))
        if (n + 1) % regrid_interval == 0:
            H.level[0][0].synchronize()
            print("steps %d..%d: %.2f ms per step" % (n + 2 - regrid_interval, n + 1, 1e3 * (time.perf_counter() - t_last) / regrid_interval), flush=True)
            tr, th = timed_regrid(H, (n + 1) // regrid_interval, (n + 1) == regrid_interval)
            t_regrid += tr; t_other += th
            t_last = time.perf_counter()
    H.level[0][0].synchronize()
    dt = (time.perf_counter() - t0 - t_regrid - t_other) / nstep
    print("regrids: %.2f ms per interval of %d steps" % (1e3 * t_regrid / max(1, nstep // regrid_interval), regrid_interval))
else:
    c = [H.timestep(mm["dt"]) for _ in range(nstep)]
    H.level[0][0].synchronize()
    dt = (time.perf_counter() - t0) / nstep
print("base %d^2: %.2f ms per step, Picard %.1f, V-cycles %.1f per step" % (nb, 1e3 * dt, sum(a for a, _ in c) / nstep, sum(b for _, b in c) / nstep))
if os.environ.get("SUHMO_TIMERS"):            # named scopes (mode 2: device time per scope; serialises)
    from suhmo_amd import capi
    print(capi.timers_report())
H.close()
