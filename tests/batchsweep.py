"""The ensemble path (suhmo_batch.hip over the launch target OnMembers of suhmo_target.h) swept over shapes, sweep counts, the arms of
batch_fas_cycle, active lists, the second stage of the members' norm and the branches of the time step: cases, seeded inputs and a census, for
tests/test_batch_sweep_cpu.py (the oracle alone) and tests/test_gpu_batch_sweep.py (the device against the oracle, bitwise).  A plain helper module
like tests/stepsweep.py and tests/bcoefsweep.py; numpy only, nothing here touches the device library.

A V-cycle / solve batch = (shape, boundary-condition row, solver row) with five members, each with its own seeded fields, BC values, physics
constants and mask palette.  The full product is not run: every shape meets every solver row once, the boundary-condition rows rotating so that
every (BC, solver row) pair occurs too (tests/test_batch_sweep_cpu.py asserts both).  A time-step batch = (shape, BC) of tests/stepsweep.py with
its option rows as members.  census_of() restates suhmo_batch_tile_ok, single_tile_of and the 4 / 2 / 1 decomposition of batch_relax in a few
lines and says, from the inputs and the oracle alone, which path every depth takes, which launches a relax issues, how many launches a cycle
is, how many partials the norm has and where each member's maximum sits."""
import contextlib
import os

import numpy as np

from suhmo_amd import synthetic as sy
from tests import bcoefsweep as bs
from tests import stepsweep as sw

BATCH_MAX = 64             # SUHMO_BATCH_MAX (suhmo_target.h)

# (nx, ny, max_box); the depth tables are the oracle's (OracleLevel.ndepth / .shape), recorded by the census
SHAPES = (
    (4, 4, 4),             # 4x4, 2x2: the minimum a batch accepts; doubly periodic (smaller than tile plus halo)
    (12, 4, 16),           # 12x4, 6x2: one partial workgroup, one partial of the norm
    (16, 16, 16),          # 16x16, 8x8, 4x4, 2x2: four single-tile depths
    (20, 12, 4),           # 20x12 (one tile of 32), 10x6
    (32, 28, 32),          # 32x28 and 16x14: exact fits of the 32- and the 16-wide single tile
    (32, 30, 32),          # one depth, just past the single tile of 32: two ragged tile rows
    (40, 24, 8),           # 2.5 tiles wide; 20x12; 10x6
    (40, 24, 4),           # not among the listed shapes: 40x24, 20x12 -- a BOTTOM that is one tile of 32 (the listed shapes reach the chunked launch of the
                           # 32-wide single tile in two batches only, under max_depth = 0)
    (72, 20, 4),           # 72x20, 36x10: both ragged, neither a single tile
    (80, 48, 16),          # tiles, tiles, one tile of 32, one of 16
    (48, 48, 16),          # tiles, one tile of 32, two of 16
    (70, 51, 64),          # one depth, odd rows
    (13, 9, 16),           # one depth, odd nx: the tile kernel refuses it -- colour passes over members
    (64, 252, 64), (64, 256, 64), (64, 260, 64),      # 63, 64 and 65 partials per member in k_norm_final_members
)
TALL = ((64, 252), (64, 256), (64, 260))
BCS = sw.BCS

# (num_smooth, num_bottom, max_depth, bottom_solver, alpha, tile_order)
ROWS = (
    (4, 16, -1, 0, 0.0, 0),        # the default
    (3, 9, -1, 0, 0.6, 1),         # 2 + 1 launches per relax; 9 = 2 chunks of 4 plus 1 on a single tile, 4 + 4 + 1 elsewhere; alpha != 0
    (1, 1, -1, 0, 0.0, 2),
    (7, 2, -1, 1, 0.0, 0),         # 4 + 2 + 1, RelaxSolver at the bottom
    (2, 0, -1, 1, 0.0, 0),         # no bottom relaxes: the bottom's FAS right-hand side from launch_fas_coarse_rhs(OnMembers), then RelaxSolver alone
    (0, 3, -1, 0, 0.0, 0),         # no smoothing: launch_prolong(OnMembers); diverges, hence fewer cycles (protocol())
    (4, 16, 0, 0, 0.0, 0),         # max_depth moves the bottom
    (4, 5, 1, 0, 0.6, 0),
)
N_MEMBERS = 5
PALETTES = ("dirty", "clean", "dirty", "one-cell", "plus-minus")       # of members 0 .. 4 (64 members: k % 5)
# (cutOffB, use_mask_gradients) of members 0 .. 4: the constants are the member's own row of the device table
SWITCHES = ((1, 1), (1, 0), (0, 1), (0, 0), (1, 1))

# batches left out, {batch id: reason}: at most one in ten, no whole shape, BC or row (tests/test_batch_sweep_cpu.py)
DROPPED = {}

SOLVE = dict(eps=1.0e-3, norm_thresh=1.0e-13, iter_min=1, imin=2, hang=0.01)      # members leave the active list at different cycles
SPIKE = 1.0e8              # the right-hand-side spike of the tall shapes: above every residual that enters a solve of the sweep (at most 3e6)


def row_name(row):
    return "s%d-b%d-d%d-rs%d-a%g-o%d" % row


def bcs_of(shape):
    """the boundary-condition rows a shape runs under: 4 x 4 doubly periodic only; odd ny skips the y-periodic rows (a condition of the level)"""
    nx, ny, _ = shape
    if (nx, ny) == (4, 4):
        return ("xy-periodic",)
    return tuple(b for b, bc in BCS.items() if not (bc["periodic"][1] and ny & 1))


def batches():
    """(batch id, shape, bc name, solver row) of every V-cycle / solve batch: every (shape, row) once, the BC rows rotating"""
    out = []
    for s, shape in enumerate(SHAPES):
        mine = bcs_of(shape)
        for r, row in enumerate(ROWS):
            b = mine[(s + r) % len(mine)]
            bid = "%dx%db%d-%s-%s" % (shape + (b, row_name(row)))
            if bid not in DROPPED:
                out.append((bid, shape, b, row))
    return out


def protocol(row):
    """(active lists of the single cycles, max_iter of the solve that follows): the num_smooth = 0 row diverges and runs fewer"""
    if row[0] == 0:
        return ([1, 1, 1, 1, 1], [1, 0, 1, 0, 1]), 2
    return ([1, 1, 1, 1, 1], [1, 0, 1, 0, 1], [0, 0, 1, 1, 0]), 6


def cycle_params(row):
    return dict(sy.SOLVER_DEFAULT, num_smooth=row[0], num_bottom=row[1], max_depth=row[2], bcoeff_otf=1)


def solve_params(row):
    return dict(cycle_params(row), max_iter=protocol(row)[1], **SOLVE)


def spike_partial(ny, k):
    """the partial workgroup (rows 4 p .. 4 p + 3 of a 64-wide level) member k's residual maximum is put into: the first, the last, a middle one,
    the one before the last, the second"""
    last = (ny + 3) // 4 - 1
    return (0, last, last // 2, last - 1, 1)[k % 5]


def spiked_rhs(shape, f, k):
    """the tall shapes: member k's right-hand side with one spike in its chosen partial, stored after the single cycles and before the solve, so
    that the maximum of the solve's first residual sits there (the cycles would have smoothed an earlier one away); None on other shapes"""
    nx, ny, _ = shape
    if (nx, ny) not in TALL:
        return None
    rhs = f["rhs"].copy()
    rhs[4 * spike_partial(ny, k) + k % 4, (7 + 11 * k) % nx] = SPIKE * (-1.0 if k & 1 else 1.0)
    return rhs


def member(shape, bcname, k):
    """(fields, BC, physics constants, palette) of member k, deterministic in the arguments: the fields as bcoefsweep.fields makes them (the
    palette's mask over the ghosted array, B with 0.0 and 1e-16 planted), BC values and constants of its own; the BC TYPES are the batch's"""
    nx, ny, _ = shape
    base, pal = BCS[bcname], PALETTES[k % 5]
    seed = [nx, ny, list(BCS).index(bcname), k, 6151]
    f = sy.random_fields(nx, ny, seed=seed, with_mask_holes=False)
    f.pop("bx"); f.pop("by")
    rng = np.random.default_rng(seed + [4099])
    r = rng.random(f["B"].shape)
    f["B"] = np.where(r < 0.03, 0.0, np.where(r < 0.06, 1.0e-16, f["B"]))
    f = sy.wrap_ghosts(f, base)
    f["mask"] = bs.palette_mask(pal, nx, ny, rng, base)
    for key in ("phi", "rhs", "aCoef", "B", "Pi", "zb", "mask"):
        f[key] = np.ascontiguousarray(f[key], dtype=np.float64)
    val = [[base["value"][d][s] + ((1.5 * k + 0.25 * d) if base["type"][d][s] == 0 else 0.004 * (k + 1) * (1 - 2 * s)) for s in range(2)] for d in range(2)]
    bc = dict(base, value=val)
    cut, mg = SWITCHES[k % 5]
    ph = dict(sy.RANDOM_PHYS, A=5e-25 * (1.0 + 0.3 * (k % 7)), cutOffbr=0.01 + 0.002 * (k % 5), omega=1e-3 * (1.0 + 0.1 * (k % 3)), cutOffB=cut,
              use_mask_gradients=mg)
    return f, bc, ph, pal


@contextlib.contextmanager
def oracle_bottom(on):
    """the oracle runs RelaxSolver after the bottom relaxes (SUHMO_ORACLE_BOTTOM, read at every cycle) inside this block, or does not"""
    old = os.environ.get("SUHMO_ORACLE_BOTTOM")
    if on:
        os.environ["SUHMO_ORACLE_BOTTOM"] = "1"
    else:
        os.environ.pop("SUHMO_ORACLE_BOTTOM", None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SUHMO_ORACLE_BOTTOM", None)
        else:
            os.environ["SUHMO_ORACLE_BOTTOM"] = old


def oracle_level(oracle, shape, f, bc, ph, row):
    nx, ny, mb = shape
    O = oracle.OracleLevel(nx, ny, f["dx"], f["dy"], bc, ph, row[4], -1.0, mb, 1)
    O.set_inputs(f)
    O.build_mg_coefficients()
    return O


# ---- the launch geometry, restated (suhmo_gsrb.hip: suhmo_batch_tile_ok, single_tile_of; suhmo_batch.hip: batch_relax, batch_fas_cycle, batch_vcycle)
def tile_ok(nx, ny, periodic):
    return not (nx & 1) and not (periodic[1] and ny & 1)


def single_tile_of(nx, ny):
    return 16 if nx <= 16 and ny <= 16 else 32 if nx <= 32 and ny <= 28 else 0


def relax_launches(nx, ny, periodic, sweeps):
    """the launches of batch_relax without the closing ghost fill: [(TS, chunks, T)], or [("colour", 1, 0)] x 2 sweeps"""
    if not tile_ok(nx, ny, periodic):
        return [("colour", 1, 0)] * (2 * sweeps)
    out, it, one = [], 0, single_tile_of(nx, ny)
    while it < sweeps:
        left = sweeps - it
        ts = 4 if left >= 4 else 2 if left >= 2 else 1
        chunks = left // ts if ts == 4 and one else 1
        out.append((ts, chunks, one if chunks > 1 else 16))
        it += ts * chunks
    return out


def sequence(launches):
    """'4x2+1': the TS sequence of a relax, chunks as a factor"""
    if not launches:
        return "none"
    if launches[0][0] == "colour":
        return "%d colour passes" % len(launches)
    return "+".join("%dx%d" % (ts, c) if c > 1 else "%d" % ts for ts, c, _ in launches)


def depth_path(nx, ny, periodic, sweeps):
    """'colour', 'T16 chunked' / 'T32 chunked' (a chunked single-tile launch is among the relax's launches), or 'tile'"""
    ls = relax_launches(nx, ny, periodic, sweeps)
    if not tile_ok(nx, ny, periodic):
        return "colour"
    for ts, c, t in ls:
        if c > 1:
            return "T%d chunked" % t
    return "tile"


def effective_depths(depths, row):
    nd = len(depths)
    return min(nd, row[2] + 1) if row[2] >= 0 else nd


def average_launches(depths, nd):
    """suhmo_batch_average_operator_all: one pass where 2^(nd - 1) divides both extents and nd <= 7, else a launch per coarse depth"""
    if nd < 2:
        return 0
    nx, ny = depths[0]
    q = 1 << (nd - 1)
    return 1 if nd <= 7 and nx % q == 0 and ny % q == 0 else nd - 1


def cycle_census(depths, periodic, row):
    """one batched V-cycle from its geometry: dict(nd, launches, relax={depth: sequence}, paths={depth: path}, rhs={depth: 'fused' / 'separate'},
    prolong={depth: 'fused' / 'separate'})"""
    S, NB, _, bsolver = row[:4]
    nd = effective_depths(depths, row)
    out = dict(nd=nd, relax={}, paths={}, rhs={}, prolong={}, ts=set())
    ok = lambda dep: tile_ok(depths[dep][0], depths[dep][1], periodic)

    def relax(dep, sweeps, observable):
        ls = relax_launches(depths[dep][0], depths[dep][1], periodic, sweeps)
        out["relax"][dep] = sequence(ls)
        out["paths"][dep] = depth_path(depths[dep][0], depths[dep][1], periodic, sweeps)
        if ls and ls[0][0] != "colour":
            out["ts"].add(sequence(ls))
        return len(ls) + (1 if sweeps > 0 and observable else 0)

    def fas(dep):
        if dep == nd - 1:
            if not bsolver:
                return relax(dep, NB, dep == 0)
            return relax(dep, NB, False) + 1 + (1 if dep == 0 else 0)
        n = relax(dep, S, False) + 1
        nxt = NB if dep + 1 == nd - 1 else S
        fused = nxt >= 1 and ok(dep + 1)
        out["rhs"][dep + 1] = "fused" if fused else "separate"
        n += 0 if fused else 1
        n += fas(dep + 1)
        fused = S >= 1 and ok(dep)
        out["prolong"][dep] = "fused" if fused else "separate"
        n += 0 if fused else 2
        return n + relax(dep, S, dep == 0)

    out["launches"] = 1 + average_launches(depths, nd) + fas(0)
    return out


def solve_launches(cyc, counts):
    """launches of suhmo_batch_solve: the initial norms (2), a cycle and its norms per cycle of the member that runs longest, the closing ghost fill"""
    return 2 + max(counts) * (cyc["launches"] + 2) + 1


def norm_partials(nx, ny):
    return ((nx + 63) // 64) * ((ny + 3) // 4)


def partial_of_max(res):
    """the partial workgroup (64 x 4 cells, x fastest) that holds the maximum of |res|"""
    j, i = np.unravel_index(np.argmax(np.abs(res)), res.shape)
    return int(j // 4) * ((res.shape[1] + 63) // 64) + int(i // 64)


def cycles_of_member(row, k):
    return sum(a[k] for a in protocol(row)[0])


def census_of(oracle, batch):
    """the oracle alone through the protocol of one batch -> dict(depths, cycle=cycle_census, np, counts=[solve cycles per member], norms,
    max_partial=[per member: partial of the residual maximum entering and leaving the solve], palette={(branch, arm): count}, problems=[...])"""
    bid, shape, b, row = batch
    nx, ny, mb = shape
    rec = dict(problems=[], counts=[], max_partial=[], palette={})
    with oracle_bottom(row[3]):
        for k in range(N_MEMBERS):
            f, bc, ph, pal = member(shape, b, k)
            for br, arms in bs.census(f, bc, ph).items():
                if br.startswith("tile "):
                    continue
                for arm, n in arms.items():
                    rec["palette"][(br, arm)] = rec["palette"].get((br, arm), 0) + n
            O = oracle_level(oracle, shape, f, bc, ph, row)
            try:
                if k == 0:
                    rec["depths"] = [O.shape(oracle.F_PHI, d)[::-1] for d in range(O.ndepth)]
                for _ in range(cycles_of_member(row, k)):
                    O.vcycle(cycle_params(row))
                if spiked_rhs(shape, f, k) is not None:
                    O.set(oracle.F_RHS, spiked_rhs(shape, f, k))
                O.residual()
                first = partial_of_max(O.get(oracle.F_RES))
                n, hist = O.solve(solve_params(row))
                rec["counts"].append(int(n))
                rec["max_partial"].append((first, partial_of_max(O.get(oracle.F_RES))))
                for d in range(O.ndepth):
                    for fid in (oracle.F_PHI, oracle.F_RES, oracle.F_RHS, oracle.F_BX, oracle.F_BY):
                        if not np.isfinite(O.get(fid, depth=d)).all():
                            rec["problems"].append("%s member %d (%s): field %d of depth %d is not finite" % (bid, k, pal, fid, d))
                if not np.isfinite(hist).all():
                    rec["problems"].append("%s member %d (%s): residual norms %r" % (bid, k, pal, list(hist)))
            finally:
                O.close()
    rec["cycle"] = cycle_census(rec["depths"], BCS[b]["periodic"], row)
    rec["np"] = norm_partials(nx, ny)
    return rec


# ---- the arms of the sweep: {arm: set of batch ids}
def arms_of(rec):
    c, out = rec["cycle"], set()
    for dep, p in c["paths"].items():
        out.add("path: " + p)
    for s in c["ts"]:
        out.add("relax: " + s)
        if s in ("4+2+1", "2+1", "1", "4"):
            out.add("decomposition: " + s)
    out |= {"coarse right-hand side: " + v for v in c["rhs"].values()} | {"prolongation: " + v for v in c["prolong"].values()}
    out.add("np: %d" % rec["np"])
    if rec["np"] > 1 and any(first == rec["np"] - 1 for first, _ in rec["max_partial"]):
        out.add("np: %d, a member's maximum in the last partial" % rec["np"])
    return out


REQUIRED_ARMS = ("path: tile", "path: T16 chunked", "path: T32 chunked", "path: colour", "decomposition: 4+2+1", "decomposition: 2+1", "decomposition: 1",
                 "decomposition: 4", "coarse right-hand side: fused", "coarse right-hand side: separate", "prolongation: fused", "prolongation: separate",
                 "np: 1", "np: 63", "np: 64", "np: 65", "np: 63, a member's maximum in the last partial", "np: 64, a member's maximum in the last partial",
                 "np: 65, a member's maximum in the last partial", "max_depth: 0", "max_depth: 1", "bottom solver: on", "bottom solver: off")


# palette arms no batch can take, with the reason; every other arm must be (tests/test_batch_sweep_cpu.py)
PALETTE_NOT_TAKEN = {("path", "four kernels (below 4 x 4)"): "a batch refuses members under 4 x 4 cells",
                     ("scan", "only ghost cells below 1e-6"): "the members' palettes do not include the two one-ghost ones"}


def sweep_census(oracle):
    """the oracle over every V-cycle / solve batch -> dict(batches={id: record}, arms={arm: set of ids}, palette={(branch, arm): [count, set of
    ids]}, problems)"""
    out = dict(batches={}, arms={}, palette={}, problems=[])
    for batch in batches():
        bid, shape, b, row = batch
        rec = out["batches"][bid] = census_of(oracle, batch)
        out["problems"] += rec["problems"]
        mine = arms_of(rec) | {"bottom solver: " + ("on" if row[3] else "off")}
        if row[2] >= 0:
            mine.add("max_depth: %d" % row[2])
        for a in mine:
            out["arms"].setdefault(a, set()).add(bid)
        for key, n in rec["palette"].items():
            t = out["palette"].setdefault(key, [0, set()])
            t[0] += n
            if n:
                t[1].add(bid)
    return out


# ---- the time step: (batch id, nx, ny, bc name, dt, member rows)
STEP_ROWS_60 = tuple(r for r in sw.ROWS if r != "hot-bed-diffusion")
STEP_ROWS_2 = ("hot-bed-diffusion", "explicit-diffusion", "implicit")
STEP_SHAPES_2 = ((12, 4), (72, 20))
# thinning (the device file's time against tests/test_gpu_step_sweep.py): the boundary-condition rows the two largest shapes run under; None: all
STEP_THINNED = {}


def step_batches():
    out = []
    for s, (nx, ny) in enumerate(sw.SHAPES):
        for q, b in enumerate(sw.BCS):
            keep = STEP_THINNED.get((nx, ny))
            if keep is None or b in keep:
                out.append(("step-%dx%d-%s-dt60" % (nx, ny, b), nx, ny, b, 60.0, STEP_ROWS_60))
            if (nx, ny) in STEP_SHAPES_2:
                out.append(("step-%dx%d-%s-dt2" % (nx, ny, b), nx, ny, b, 2.0, STEP_ROWS_2))
    return out


def step_case(batch, r):
    """the single-level case of stepsweep a member of a time-step batch is"""
    bid, nx, ny, b, dt, rows = batch
    return ("%s-%s" % (bid, r), nx, ny, b, r)


def step_census(oracle):
    """stepsweep.run_single of every member of every time-step batch -> dict(problems, arms={(branch, arm): [cells, set of member ids, set of
    shapes]}, partial_groups={shape: workgroups of a per-cell launch})"""
    out = dict(problems=[], arms={}, runs=0)
    for batch in step_batches():
        for r in batch[5]:
            case = step_case(batch, r)
            rec = sw.run_single(oracle, case, dt=batch[4])
            out["runs"] += 1
            out["problems"] += rec["problems"]
            if len(rec["iters"]) != sw.N_STEPS:
                out["problems"].append("%s: %d steps" % (case[0], len(rec["iters"])))
            for cen in rec["census"]:
                for br, arms in sw.fold_faces(sw.counts(cen)).items():
                    for arm, n in arms.items():
                        t = out["arms"].setdefault((br, arm), [0, set(), set()])
                        t[0] += n
                        if n:
                            t[1].add(case[0]); t[2].add((case[1], case[2]))
    return out


# ---- sixty-four members: (id, shape, bc name); solver row (1, 1, ...)
BIG = (("64-members-12x4", (12, 4, 16), "dirichlet"), ("64-members-40x24", (40, 24, 8), "y-periodic"))
BIG_ROW = ROWS[2]
BIG_ORACLE = (0, 1, 31, 32, 62, 63)


def big_active_lists():
    return [[int(k == 63) for k in range(BATCH_MAX)], [int(k in (0, 63)) for k in range(BATCH_MAX)], [k & 1 for k in range(BATCH_MAX)], [1] * BATCH_MAX]


def census_table(s, st=None):
    """the census as text: tests/golden/BATCH_SWEEP_CENSUS.txt (tools/batch_sweep_census.py writes it)"""
    lines = ["# census of the ensemble sweep on the CPU oracle: tests/batchsweep.py, regenerated by tools/batch_sweep_census.py",
             "# %d V-cycle / solve batches of %d members; per depth: extent, path, launches of a relax; rhs / prolongation of the depth fused into a relax (f) or"
             % (len(s["batches"]), N_MEMBERS), "# separate (s); launches of one cycle; partials of the norm; cycles of the solve per member; partial of each member's residual",
             "# maximum before / after the solve"]
    for bid, rec in s["batches"].items():
        c = rec["cycle"]
        deps = []
        for d in range(c["nd"]):
            nx, ny = rec["depths"][d]
            deps.append("%dx%d %s %s%s%s" % (nx, ny, c["paths"][d], c["relax"][d], " rhs:" + c["rhs"][d][0] if d in c["rhs"] else "",
                                             " pro:" + c["prolong"][d][0] if d in c["prolong"] else ""))
        lines.append("%-48s | %s | launches %d | np %d | cycles %s | max in %s" % (
            bid, "; ".join(deps), c["launches"], rec["np"], ",".join(str(n) for n in rec["counts"]),
            " ".join("%d/%d" % p for p in rec["max_partial"])))
    lines += ["# arms: batches in which the arm is taken", "%-56s %7s" % ("arm", "batches")]
    for a in sorted(s["arms"]):
        lines.append("%-56s %7d" % (a, len(s["arms"][a])))
    lines += ["# mask palettes through launch_bcoef_fused(OnMembers): bcoefsweep.census of every member, summed", "%-30s %-36s %9s %7s" % ("branch", "arm", "count", "batches")]
    for (br, arm), (n, ids) in s["palette"].items():
        lines.append("%-30s %-36s %9d %7d" % (br, arm, n, len(ids)))
    if st is not None:
        lines += ["# time-step batches: %d member runs x %d steps; cells or faces that took the arm, members and shapes in which at least one did" % (st["runs"], sw.N_STEPS),
                  "%-42s %-28s %9s %7s %6s" % ("branch", "arm", "cells", "members", "shapes")]
        for (br, arm), (n, cs, shp) in st["arms"].items():
            lines.append("%-42s %-28s %9d %7d %6d" % (br, arm, n, len(cs), len(shp)))
    return "\n".join(lines) + "\n"
