"""The face-coefficient kernels of suhmo_bcoef.hip (UpdateOperator = WFlx_level, fused and un-fused; AverageOperator) swept over the edges of their
tiles and over the values at which they question the ice mask: cases, seeded inputs and a census of the arms, for tests/test_bcoef_sweep_cpu.py (the
oracle alone) and tests/test_gpu_bcoef_sweep.py (the device against the oracle, bitwise).  A plain helper module like tests/stepsweep.py; numpy only,
nothing here touches the device library.

A case = (shape, boundary-condition row, physics row, mask palette).  Every shape meets every boundary-condition row twice: once with the "dirty"
palette and once with one of the other five, the physics rows rotating so that every pair of (row, row) of two different tables occurs
(tests/test_bcoef_sweep_cpu.py asserts the pairs); the full product is not run.  census() restates in numpy, from the inputs alone, the predicates
of d_gradcc_val / bcoef_tile's gradcc, bcoef_face, the ghost gradients and the ownership of faces by tiles (the constants 62 / 126 / 14 and
d_bcoef_fused's `interior`), and says per arm how many cells, faces or levels take it."""
import numpy as np

from suhmo_amd import synthetic as sy
from tests import stepsweep as sw

# ---- the kernel's geometry, restated (suhmo_bcoef.hip: bcoef_tile, d_bcoef_fused, bcoef_is_fused, suhmo_level_update_operator)
BT_Y = 14
TILE_WIDTHS = (62, 126)
WIDE_MIN_NX = 256          # bcoef_tile_x = 126 is taken on levels at least this wide
FUSED_MIN = 4              # the fused kernel runs on levels of at least 4 x 4 cells

SHAPES = (
    (2, 2), (3, 5), (5, 3),                                  # below the fused path: the four-kernel path on a whole level
    (4, 4), (5, 4),                                          # the smallest fused levels: periodic, the phi tile would hold several images of a cell
    # the 62-wide tile's edges in x (last tile column 61 wide, exactly full, 1 wide, ...), each with two ny; between them every edge in y
    # (13, 14, 15: the last tile row short by one, full, 1 tall; 28, 29, 30; 43 = 3 x 14 + 1)
    (61, 13), (61, 30), (62, 14), (62, 29), (63, 15), (63, 28), (124, 13), (124, 43), (126, 14), (126, 30), (127, 16), (127, 29), (128, 28), (128, 43),
    # the wide tile: 256 (the gate; 252 = 2 x 126 is below it), 258, 378 = 3 x 126, 380; an INTERIOR wide tile exists from 254 x 30 on
    (256, 16), (256, 31), (258, 30), (378, 16), (378, 30), (380, 31), (380, 43),
    (379, 28),                                               # not among the listed sizes: the wide tile's last column 1 wide (3 x 126 + 1), its last row full
)
LISTED_NX = (2, 3, 5, 4, 61, 62, 63, 124, 126, 127, 128, 256, 258, 378, 380)
LISTED_NY = (2, 5, 3, 4, 13, 14, 15, 28, 29, 30, 43, 16, 31)

BCS = sw.BCS               # a3, y-periodic, x-periodic, xy-periodic, dirichlet (values 2 and 900 on the x sides)
PHYS = dict([
    ("cut1-mg1", dict(sy.RANDOM_PHYS, cutOffB=1, use_mask_gradients=1)),
    ("cut1-mg0", dict(sy.RANDOM_PHYS, cutOffB=1, use_mask_gradients=0)),
    ("cut0-mg1", dict(sy.RANDOM_PHYS, cutOffB=0, use_mask_gradients=1)),
    ("cut0-mg0", dict(sy.RANDOM_PHYS, cutOffB=0, use_mask_gradients=0)),
    ("a3", dict(sy.A3_PHYS)),
])

# ---- the values of the ice mask.  The code asks `< 1e-6` (gradient, scan), `< 0` (relaxation, report), `> 0` with `fabs(mc - mm) < 1e-10`
# (bcoef_face): both sides of each in one level
BELOW = float(np.nextafter(1.0e-6, 0.0))
DIRTY = (-1.0, -0.0, 0.0, 5.0e-7, BELOW, 1.0e-6, 0.5, 1.0, 1.0 + 5.0e-11, 1.0 + 2.0e-10)
CLEAN = (1.0e-6, 0.5, 1.0, 1.0 + 5.0e-11, 1.0 + 2.0e-10)
ONE = 5.0e-7               # the single value below 1e-6 of the "clean but for one" palettes
PALETTES = ("dirty", "clean", "one-cell", "one-ghost-south", "one-ghost-east", "plus-minus")
MAX_BOX = 512              # one box per level on both sides

SCAN_UNKNOWN, SCAN_CLEAN, SCAN_DIRTY = 0, 1, 2      # level option mask_state


def cases():
    """(case id, nx, ny, bc name, physics name, palette) of every case: two per (shape, bc)"""
    out = []
    nb, nph, others = list(BCS), list(PHYS), PALETTES[1:]
    for s, (nx, ny) in enumerate(SHAPES):
        for b, bc in enumerate(nb):
            for ph, pal in ((nph[(s + b) % 5], "dirty"), (nph[(2 * s + b + 1) % 5], others[(s + b) % 5])):
                out.append(("%dx%d-%s-%s-%s" % (nx, ny, bc, ph, pal), nx, ny, bc, ph, pal))
    return out


def find(nx, ny, bc=None, ph=None, pal=None):
    """the cases of a shape that match the given rows"""
    return [c for c in cases() if (c[1], c[2]) == (nx, ny) and bc in (None, c[3]) and ph in (None, c[4]) and pal in (None, c[5])]


def _draw(rng, values, shape, weight_of_one=0.3):
    """a seeded choice per cell: 1.0 with the given weight on top of its share, the other values alike"""
    v = np.array(values)
    p = np.full(v.size, (1.0 - weight_of_one) / v.size)
    p[np.flatnonzero(v == 1.0)[0]] += weight_of_one
    return v[rng.choice(v.size, size=shape, p=p)]


def palette_mask(pal, nx, ny, rng, bc):
    """the ghosted mask of a palette: drawn over the ghosted array, so that the ghost ring carries the values too; across a periodic side the ring is
    the periodic image (synthetic.wrap_ghosts), and the single ghost cells of the two one-ghost palettes are planted after that: caller data"""
    g = (ny + 2, nx + 2)
    if pal == "plus-minus":
        m = np.where(rng.uniform(size=g) < 0.1, -1.0, 1.0)
    else:
        m = _draw(rng, DIRTY if pal == "dirty" else CLEAN, g)
    if pal == "one-cell":
        m[1 + ny // 2, 1 + nx // 3] = ONE
    m = sy.wrap_ghosts(dict(B=m.copy(), Pi=m.copy(), zb=m.copy(), mask=m), bc)["mask"]
    if pal == "one-ghost-south":
        m[0, 1 + (2 * nx) // 3] = ONE                  # the ghost cell below cell ((2 nx) // 3, 0)
    if pal == "one-ghost-east":
        m[1 + ny // 2, nx + 1] = ONE                   # the ghost cell beside cell (nx - 1, ny // 2)
    return np.ascontiguousarray(m)


def fields(case):
    """the inputs of a case, deterministic in the case: synthetic.random_fields with the palette's mask and a gap height that is 0.0 in 3 % and 1e-16
    (GapInit under thin ice) in 3 % of the ghosted cells -- never negative: Re stays real"""
    cid, nx, ny, b, ph, pal = case
    bc = BCS[b]
    seed = [nx, ny, list(BCS).index(b), PALETTES.index(pal)]
    f = sy.random_fields(nx, ny, seed=seed, with_mask_holes=False)
    f.pop("bx"); f.pop("by")
    rng = np.random.default_rng(seed + [4099])
    r = rng.random(f["B"].shape)
    f["B"] = np.where(r < 0.03, 0.0, np.where(r < 0.06, 1.0e-16, f["B"]))
    f = sy.wrap_ghosts(f, bc)
    f["mask"] = palette_mask(pal, nx, ny, rng, bc)
    for k in ("phi", "rhs", "aCoef", "B", "Pi", "zb", "mask"):
        f[k] = np.ascontiguousarray(f[k], dtype=np.float64)
    return f


def is_fused(nx, ny):
    return nx >= FUSED_MIN and ny >= FUSED_MIN


def widths_of(nx, ny):
    """the tile widths the level can run"""
    return tuple(w for w in TILE_WIDTHS if is_fused(nx, ny) and (w == 62 or nx >= WIDE_MIN_NX))


def scan_answer(f):
    """what the scan of k_bcoef_fused must find: CLEAN iff every cell and every ghost cell that is not a corner is >= 1e-6"""
    m = f["mask"].copy()
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1.0
    return SCAN_CLEAN if (m >= 1.0e-6).all() else SCAN_DIRTY


# ---- ownership of faces by tiles
def owners(nx, ny, btx):
    """(x-faces (ny, nx + 1), y-faces (ny + 1, nx), tiles): per face how many INTERIOR tiles store it and how many edge tiles do (two int maps
    stacked on axis 0), following bcoef_tile's last section; tiles = [(i0, j0, interior, nxt, nyt)]"""
    fx, fy, tiles = np.zeros((2, ny, nx + 1), dtype=int), np.zeros((2, ny + 1, nx), dtype=int), []
    for bj in range((ny + BT_Y - 1) // BT_Y):
        for bi in range((nx + btx - 1) // btx):
            i0, j0 = bi * btx, bj * BT_Y
            interior = i0 - 2 >= 0 and i0 + btx + 1 <= nx - 1 and j0 - 2 >= 0 and j0 + BT_Y + 1 <= ny - 1
            nxt = nx - i0 + 1 if (not interior and i0 + btx >= nx) else btx
            nyt = ny - j0 + 1 if (not interior and j0 + BT_Y >= ny) else BT_Y
            k = 0 if interior else 1
            fx[k, j0:min(j0 + nyt, ny), i0:i0 + nxt] += 1            # bx where j < ny
            fy[k, j0:j0 + nyt, i0:min(i0 + nxt, nx)] += 1            # by where i < nx
            tiles.append((i0, j0, interior, nxt, nyt))
    return fx, fy, tiles


def tile_of(btx, i, j):
    return (i // btx, j // BT_Y)


# ---- the census
def census(f, bc, phys):
    """{branch: {arm: count}} of one case, from its inputs alone"""
    M = f["mask"]
    ny, nx = M.shape[0] - 2, M.shape[1] - 2
    n = lambda a: int(np.count_nonzero(a))
    out = {}
    # the gradient's mask tests (d_gradcc_val, bcoef_tile's gradcc), asked of every valid cell
    hm = bool(phys.get("use_mask_gradients", 0))
    c = M[1:-1, 1:-1]
    nbs = dict(W=M[1:-1, :-2], E=M[1:-1, 2:], S=M[:-2, 1:-1], N=M[2:, 1:-1])
    ring = {k: np.zeros((ny, nx), dtype=bool) for k in nbs}
    ring["W"][:, 0] = ring["E"][:, -1] = ring["S"][0, :] = ring["N"][-1, :] = True
    for s, m in nbs.items():
        z, z0 = (c < 1e-6) | (m < 1e-6), (c < 0.0) | (m < 0.0)
        out["gradient z%s" % s] = {
            "cell itself < 1e-6": n(c < 1e-6) * hm, "neighbour alone": n(~(c < 1e-6) & (m < 1e-6)) * hm,
            "neighbour alone, in the ghost ring": n(~(c < 1e-6) & (m < 1e-6) & ring[s]) * hm, "neither": n(~z) * hm,
            "true with < 1e-6, false with < 0": n(z & ~z0) * hm, "use_mask_gradients off": 0 if hm else nx * ny}
    # bcoef_face on every face, the two directions added up
    cut = int(phys.get("cutOffB", 0)) > 0
    face = {"equal, positive": 0, "equal, not positive": 0, "unequal": 0, "0 < |difference| < 1e-10": 0, "1e-10 <= |difference| < 1e-9": 0}
    edge = {"domain face": 0, "inside": 0}
    early = {"mec < 0 && cutOffB: returns 0": 0, "mec < 0, cutOffB off": 0, "mec >= 0": 0}
    for mc, mm, dom in ((M[1:-1, 1:], M[1:-1, :-1], np.arange(nx + 1)[None, :] % nx == 0), (M[1:, 1:-1], M[:-1, 1:-1], np.arange(ny + 1)[:, None] % ny == 0)):
        dom = np.broadcast_to(dom, mc.shape)
        diff = np.abs(mc - mm)
        same = diff < 1e-10
        face["equal, positive"] += n(same & (mc > 0.0)); face["equal, not positive"] += n(same & ~(mc > 0.0)); face["unequal"] += n(~same)
        face["0 < |difference| < 1e-10"] += n(same & (diff > 0.0)); face["1e-10 <= |difference| < 1e-9"] += n(~same & (diff < 1e-9))
        edge["domain face"] += n(dom); edge["inside"] += n(~dom)
        neg = same & ~(mc > 0.0) & ~dom
        early["mec < 0 && cutOffB: returns 0"] += n(neg) * cut; early["mec < 0, cutOffB off"] += n(neg) * (not cut); early["mec >= 0"] += n(~neg)
    out["bcoef_face: masks"], out["bcoef_face: dom_edge"], out["bcoef_face: early return"] = face, edge, early
    # ghost gradients: the ghost cells of the four sides, extrapolated or a periodic image
    px, py = bc["periodic"]
    out["ghost gradient"] = {"extrapolated W": 0 if px else ny, "extrapolated E": 0 if px else ny, "extrapolated S": 0 if py else nx,
                             "extrapolated N": 0 if py else nx, "periodic image in x": 2 * ny if px else 0, "periodic image in y": 2 * nx if py else 0}
    out["path"] = {"four kernels (below 4 x 4)": int(not is_fused(nx, ny)), "fused": int(is_fused(nx, ny))}
    ans = scan_answer(f)
    inner_dirty = not (M[1:-1, 1:-1] >= 1e-6).all()
    out["scan"] = {"clean": int(ans == SCAN_CLEAN), "a cell below 1e-6": int(ans == SCAN_DIRTY and inner_dirty),
                   "only ghost cells below 1e-6": int(ans == SCAN_DIRTY and not inner_dirty)}
    # faces by owner, per tile width the level can run
    for w in TILE_WIDTHS:
        run = w in widths_of(nx, ny)
        fx, fy, tiles = owners(nx, ny, w) if run else (np.zeros((2, 0, 0), dtype=int), np.zeros((2, 0, 0), dtype=int), [])
        lastw = (nx - 1) % w + 1 if run else -1                 # cells of the last tile column / row
        lasth = (ny - 1) % BT_Y + 1 if run else -1
        out["tile %d: faces" % w] = {
            "of an INTERIOR tile": int(fx[0].sum() + fy[0].sum()), "of an edge tile": int(fx[1].sum() + fy[1].sum()),
            "E faces of the last tile column": ny if run else 0, "N faces of the last tile row": nx if run else 0}
        out["tile %d: last tile column" % w] = {"1 cell wide": int(lastw == 1), "full": int(lastw == w), "in between": int(1 < lastw < w)}
        out["tile %d: last tile row" % w] = {"1 cell tall": int(lasth == 1), "full": int(lasth == BT_Y), "in between": int(1 < lasth < BT_Y)}
    return out


# arms no case of the sweep can take, with the reason; every other arm must be taken (tests/test_bcoef_sweep_cpu.py)
NOT_TAKEN = {}


def oracle_faces(oracle, case, f=None):
    """(bx, by) of UpdateOperator on the oracle"""
    cid, nx, ny, b, ph, pal = case
    f = fields(case) if f is None else f
    O = oracle.OracleLevel(nx, ny, f["dx"], f["dy"], BCS[b], PHYS[ph], 0.0, -1.0, MAX_BOX, 1)
    try:
        O.set_inputs(f)
        O.update_operator()
        return O.get(oracle.F_BX), O.get(oracle.F_BY)
    finally:
        O.close()


def sweep_census(oracle):
    """the oracle over every case -> dict(arms={(branch, arm): [count, set of case ids, set of shapes]}, problems=[messages], ncases)"""
    out = dict(arms={}, problems=[], ncases=0)
    for case in cases():
        cid, nx, ny, b, ph, pal = case
        f = fields(case)
        try:
            bx, by = oracle_faces(oracle, case, f)
        except Exception as e:                                  # every case builds
            out["problems"].append("%s: raised %r" % (cid, e))
            continue
        out["ncases"] += 1
        if bx.shape != (ny, nx + 1) or by.shape != (ny + 1, nx) or not (np.isfinite(bx).all() and np.isfinite(by).all()):
            out["problems"].append("%s: the oracle's faces are not finite" % cid)
        if not (f["B"] >= 0.0).all():
            out["problems"].append("%s: a negative gap height" % cid)
        for br, arms in census(f, BCS[b], PHYS[ph]).items():
            for arm, k in arms.items():
                t = out["arms"].setdefault((br, arm), [0, set(), set()])
                t[0] += k
                if k:
                    t[1].add(cid); t[2].add((nx, ny))
    return out


def census_table(s):
    """the census as text: tests/golden/BCOEF_SWEEP_CENSUS.txt (tools/bcoef_sweep_census.py writes it)"""
    lines = ["# census of the face-coefficient sweep: tests/bcoefsweep.py, regenerated by tools/bcoef_sweep_census.py",
             "# %d cases; cells, faces or levels that take the arm, cases and shapes in which at least one does" % s["ncases"],
             "%-30s %-36s %9s %6s %6s" % ("branch", "arm", "count", "cases", "shapes")]
    for (br, arm), (k, cs, shp) in s["arms"].items():
        lines.append("%-30s %-36s %9d %6d %6d" % (br, arm, k, len(cs), len(shp)))
    return "\n".join(lines) + "\n"


# ---- AverageOperator and MGnewOp's coarsening: (name, nx, ny, max_box, number of depths)
AVERAGE_SHAPES = (
    ("128x128-one-pass-r64", 128, 128, 128, 7),     # k_average_faces_all walks R = 64 faces per group: a whole wave in the y-face walker
    ("256x256-per-depth", 256, 256, 256, 8),        # eight depths: avg_faces_one_pass says no, one launch per depth
    ("64x32-boxes-of-16", 64, 32, 16, 4),           # many boxes, shallow
)


def average_fields(nx, ny, kind, bc):
    """inputs of an AverageOperator case: "dirty" -- random_fields with the dirty palette over the ghosted mask; "smooth" -- SHMIP's sheet"""
    if kind == "smooth":
        return sy.shmip_fields(nx, ny)
    f = sy.random_fields(nx, ny, seed=[nx, ny, 77], with_mask_holes=False)
    f.pop("bx"); f.pop("by")
    f = sy.wrap_ghosts(f, bc)
    f["mask"] = palette_mask("dirty", nx, ny, np.random.default_rng([nx, ny, 78]), bc)
    return f
