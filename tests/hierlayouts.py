"""Box-union hierarchy layouts for the sweeps of tests/test_hier_layouts_cpu.py and tests/test_gpu_hier_layouts.py: a validity rule, a seeded
generator, layouts built on purpose (FEATURES), a re-cutting of the same unions and input fields that cross the operator's thresholds.
numpy only; nothing here touches the device library.

unfilled_corners, reflux_orders and cut_signature mirror two loops of oracle/amrm.c (the prolongation's window and the reflux) to say when two
cuttings of the same unions must give the same bits.  They are validated only indirectly: tests/test_hier_layouts_cpu.py asserts that the
oracle's bits agree wherever the signatures do, and its docstring holds the reference lines behind either cause.

boxes[l - 1] = list of (lo0, lo1, hi0, hi1) in the index space of level l (domain (nx0 << l) x (ny0 << l)), as OracleAmrM and HipHier take them."""
import numpy as np

from suhmo_amd import synthetic as sy

NX0, NY0 = 32, 16
# use_mask_gradients and cutOffB on, B drawn on both sides of cutOffbr and maxOffbr (adversarial_fields)
ADV_PHYS = dict(sy.CFG3_PHYS, use_mask_gradients=1, cutOffbr=0.008, maxOffbr=0.012, cutOffB=1)


def _wrapped(c, n, periodic):
    """cell c = [i, j] of a level of size n after the periodic wrap; None when it lies outside a non-periodic side"""
    c = list(c)
    for d in range(2):
        if 0 <= c[d] < n[d]:
            continue
        if not periodic[d]:
            return None
        c[d] %= n[d]
    return c


def level_mask(nx, ny, bl):
    m = np.zeros((ny, nx), dtype=bool)
    for lo0, lo1, hi0, hi1 in bl:
        m[lo1:hi1 + 1, lo0:hi0 + 1] = True
    return m


def valid(nx0, ny0, periodic, boxes):
    """the rule of suhmo_hier_create (include/suhmo_hip.h) and or_amrm_create: boxes coarse-aligned (even lower corner, odd upper corner), inside
    the refined domain, disjoint within a level; for l >= 2 coarsen(box) grown by 2 lies in the union of level l - 1 after the periodic wrap, or
    outside a non-periodic domain"""
    below = None
    for l, bl in enumerate(boxes, start=1):
        nx, ny = nx0 << l, ny0 << l
        m = np.zeros((ny, nx), dtype=bool)
        for lo0, lo1, hi0, hi1 in bl:
            if (lo0 & 1) or (lo1 & 1) or not (hi0 & 1) or not (hi1 & 1) or lo0 < 0 or lo1 < 0 or hi0 >= nx or hi1 >= ny or hi0 < lo0 or hi1 < lo1:
                return False
            if m[lo1:hi1 + 1, lo0:hi0 + 1].any():
                return False
            m[lo1:hi1 + 1, lo0:hi0 + 1] = True
        if below is not None:
            for lo0, lo1, hi0, hi1 in bl:
                for J in range(lo1 // 2 - 2, hi1 // 2 + 3):
                    for I in range(lo0 // 2 - 2, hi0 // 2 + 3):
                        c = _wrapped((I, J), (nx // 2, ny // 2), periodic)
                        if c is not None and not below[c[1], c[0]]:
                            return False
        below = m
    return True


def _eroded(m, periodic, r=2):
    """cells whose (2r + 1)^2 neighbourhood lies in m after the wrap; outside a non-periodic domain counts as inside"""
    ny, nx = m.shape
    p = np.pad(m, r, mode="constant", constant_values=True)
    if periodic[0]:
        p[:, :r], p[:, -r:] = p[:, nx:nx + r].copy(), p[:, r:2 * r].copy()
    if periodic[1]:
        p[:r, :], p[-r:, :] = p[ny:ny + r, :].copy(), p[r:2 * r, :].copy()
    out = np.ones_like(m)
    for dj in range(2 * r + 1):
        for di in range(2 * r + 1):
            out &= p[dj:dj + ny, di:di + nx]
    return out


def _draw_bc(rng, periodic):
    """boundary types and values as _random_tile_case (tests/test_gpu_parity.py) draws them; where a direction is not periodic at least one
    of the non-periodic sides is Dirichlet, so that the only singular problem of the sweep is the doubly periodic one"""
    bc = dict(type=[[int(rng.integers(0, 2)), int(rng.integers(0, 2))], [int(rng.integers(0, 2)), int(rng.integers(0, 2))]],
              value=[[float(rng.uniform(-5, 5)), float(rng.uniform(-0.05, 0.05))], [float(rng.uniform(-0.05, 0.05)), float(rng.uniform(-5, 5))]],
              periodic=list(periodic))
    sides = [(d, s) for d in range(2) if not periodic[d] for s in range(2)]
    if sides and all(bc["type"][d][s] == 1 for d, s in sides):
        d, s = sides[int(rng.integers(0, len(sides)))]
        bc["type"][d][s] = 0
    return bc


EXTENTS = (1, 1, 1, 2, 2, 3, 4, 6, 8, 12, 16, 24)        # of a rectangle, in cells of the level below


def generate(seed, nx0=NX0, ny0=NY0):
    """(bc, boxes), deterministic in seed.  The periodicity runs through all four combinations (seed % 4) and the number of levels through 2, 3, 4
    ((seed // 4) % 3); everything else is drawn: 1 to 6 boxes per level, rectangles in the cells of the level below, seeded at a cell of that
    level's union eroded by 2 (four times in ten at one on a domain side; after a rectangle against a periodic
    side, at the cell across the wrap) and grown towards extents of 1 to 24 coarse cells as far as the eroded union and the other rectangles allow,
    some of them split into two abutting boxes"""
    periodic = [seed % 4 & 1, seed % 4 >> 1]
    nref = 1 + (seed // 4) % 3
    for attempt in range(64):                             # a level below that leaves no room for a box: draw again
        rng = np.random.default_rng([int(seed), 4021, attempt])
        bc = _draw_bc(rng, periodic)
        boxes = _draw_boxes(rng, periodic, nref, nx0, ny0)
        if all(boxes):
            return bc, boxes
    raise RuntimeError("no hierarchy of %d levels found for seed %d" % (nref + 1, seed))


def _draw_boxes(rng, periodic, nref, nx0, ny0):
    boxes, below = [], np.ones((ny0, nx0), dtype=bool)
    for l in range(1, nref + 1):
        ny, nx = below.shape                              # rectangles live in the cells of level l - 1
        free = below if l == 1 else _eroded(below, periodic)
        free = free.copy()
        rects, want, across = [], int(rng.integers(1, 7)), None
        while len(rects) < want and free.any():
            js, is_ = np.nonzero(free)
            if rng.random() < 0.4:                        # start on a domain side: boxes against the sides, neighbours through the wrap
                side = (is_ == 0) | (is_ == nx - 1) | (js == 0) | (js == ny - 1)
                if side.any():
                    js, is_ = js[side], is_[side]
            n = int(rng.integers(0, js.size))
            i0 = i1 = int(is_[n]); j0 = j1 = int(js[n])
            if across is not None and free[across[1], across[0]]:
                i0 = i1 = across[0]; j0 = j1 = across[1]
            across = None
            w, h = int(rng.choice(EXTENTS)), int(rng.choice(EXTENTS))
            stuck = 0
            while stuck < 4 and (i1 - i0 + 1 < w or j1 - j0 + 1 < h):
                side = int(rng.integers(0, 4))
                grown = False
                if side == 0 and i1 - i0 + 1 < w and i0 > 0 and free[j0:j1 + 1, i0 - 1].all():
                    i0 -= 1; grown = True
                if side == 1 and i1 - i0 + 1 < w and i1 < nx - 1 and free[j0:j1 + 1, i1 + 1].all():
                    i1 += 1; grown = True
                if side == 2 and j1 - j0 + 1 < h and j0 > 0 and free[j0 - 1, i0:i1 + 1].all():
                    j0 -= 1; grown = True
                if side == 3 and j1 - j0 + 1 < h and j1 < ny - 1 and free[j1 + 1, i0:i1 + 1].all():
                    j1 += 1; grown = True
                stuck = 0 if grown else stuck + 1
            free[j0:j1 + 1, i0:i1 + 1] = False
            # against a periodic side: the next rectangle starts across the wrap
            if periodic[0] and (i0 == 0) != (i1 == nx - 1):
                across = (nx - 1 if i0 == 0 else 0, int(rng.integers(j0, j1 + 1)))
            elif periodic[1] and (j0 == 0) != (j1 == ny - 1):
                across = (int(rng.integers(i0, i1 + 1)), ny - 1 if j0 == 0 else 0)
            parts = [(i0, j0, i1, j1)]
            if len(rects) + 1 < want and rng.random() < 0.4:
                if i1 > i0 and (j1 == j0 or rng.random() < 0.5):
                    c = int(rng.integers(i0, i1))
                    parts = [(i0, j0, c, j1), (c + 1, j0, i1, j1)]
                elif j1 > j0:
                    c = int(rng.integers(j0, j1))
                    parts = [(i0, j0, i1, c), (i0, c + 1, i1, j1)]
            rects += parts
        bl = [(2 * a, 2 * b, 2 * c + 1, 2 * d + 1) for a, b, c, d in rects]
        boxes.append(bl)
        below = level_mask(2 * nx, 2 * ny, bl)
    return boxes


def recut(seed, boxes, periodic=None, nx0=NX0, ny0=NY0):
    """the same unions cut at other even coordinates: every level's union is covered again, scanning its coarse cells row by row (odd seeds: column
    by column), by rectangles of drawn largest extents.  With `periodic` given, the first of 16 such cuttings that differs from `boxes` and has
    their cut_signature(), if there is one (else the first)"""
    first = None
    for attempt in range(16 if periodic is not None else 1):
        rc = _recut(np.random.default_rng([int(seed), 977, attempt]), (seed + attempt) & 1, boxes, nx0, ny0)
        first = rc if first is None else first
        if periodic is not None and rc != boxes and cut_signature(nx0, ny0, periodic, rc) == cut_signature(nx0, ny0, periodic, boxes):
            return rc
    return first


def _recut(rng, transposed, boxes, nx0, ny0):
    out = []
    for l, bl in enumerate(boxes, start=1):
        m = level_mask(nx0 << l, ny0 << l, bl)[::2, ::2].copy()
        if transposed:
            m = m.T.copy()
        ny, nx = m.shape
        rects = []
        for j in range(ny):
            for i in range(nx):
                if not m[j, i]:
                    continue
                w, h = int(rng.choice(EXTENTS[3:])), int(rng.choice(EXTENTS[3:]))
                i1 = i
                while i1 + 1 < nx and i1 - i + 1 < w and m[j, i1 + 1]:
                    i1 += 1
                j1 = j
                while j1 + 1 < ny and j1 - j + 1 < h and m[j1 + 1, i:i1 + 1].all():
                    j1 += 1
                m[j:j1 + 1, i:i1 + 1] = False
                rects.append((j, i, j1, i1) if transposed else (i, j, i1, j1))
        out.append([(2 * a, 2 * b, 2 * c + 1, 2 * d + 1) for a, b, c, d in rects])
    return out


def reflux_orders(nx0, ny0, periodic, boxes):
    """The other thing a cutting can change: a coarse cell with coarse-fine faces of more than one fine box (at a re-entrant corner of the union, in
    a gap one coarse cell wide) takes the flux-register increments of its faces one after the other, in the order (fine box, direction, side)
    of the boxes that own the faces -- floating-point additions in an order the box list decides.  Returns {(level, coarse cell): faces in
    that order} for the cells with more than one face."""
    out = {}
    for l, bl in enumerate(boxes, start=1):
        n = ((nx0 << l) // 2, (ny0 << l) // 2)
        cov = level_mask(nx0 << l, ny0 << l, bl)[::2, ::2]
        for lo0, lo1, hi0, hi1 in bl:
            cb = (lo0 // 2, lo1 // 2, hi0 // 2, hi1 // 2)
            for d in range(2):
                for s in range(2):
                    o = cb[d] - 1 if s == 0 else cb[2 + d] + 1
                    for t in range(cb[1 - d], cb[3 - d] + 1):
                        c = _wrapped((o, t) if d == 0 else (t, o), n, periodic)
                        if c is not None and not cov[c[1], c[0]]:
                            out.setdefault((l, c[0], c[1]), []).append((d, s))
    return {k: tuple(v) for k, v in out.items() if len(v) > 1}


def cut_signature(nx0, ny0, periodic, boxes):
    """two cuttings of the same unions with the same signature must give the same bits (tests/test_hier_layouts_cpu.py)"""
    return unfilled_corners(nx0, ny0, periodic, boxes), reflux_orders(nx0, ny0, periodic, boxes)


def unfilled_corners(nx0, ny0, periodic, boxes):
    """What a cutting can change (see test_recut_changes_no_bit_where_it_must_not): the corner cells of coarsen(box) grown by one that lie across a
    non-periodic domain side while the cell next to them inside the domain belongs to the level too.  AMRProlongS_2 reads them, and neither the
    boundary condition of the box (side cells only) nor the corner copier (valid cells only) writes them; had the cut not been there, the cell
    would be a side cell of the box and hold the boundary condition.  Returns the set of (level, ghost cell, the box corner diagonal to it)."""
    out = set()
    for l, bl in enumerate(boxes, start=1):
        n = ((nx0 << l) // 2, (ny0 << l) // 2)
        cov = level_mask(nx0 << l, ny0 << l, bl)[::2, ::2]
        for lo0, lo1, hi0, hi1 in bl:
            cb = (lo0 // 2, lo1 // 2, hi0 // 2, hi1 // 2)
            for gi, vi in ((cb[0] - 1, cb[0]), (cb[2] + 1, cb[2])):
                for gj, vj in ((cb[1] - 1, cb[1]), (cb[3] + 1, cb[3])):
                    off = [not 0 <= gi < n[0], not 0 <= gj < n[1]]
                    for d in range(2):
                        if not off[d] or periodic[d] or (off[1 - d] and not periodic[1 - d]):
                            continue
                        c = _wrapped((vi, gj) if d == 0 else (gi, vj), n, periodic)
                        if cov[c[1], c[0]]:
                            out.add((l, (gi, gj), (vi, vj)))
    return out


def cf_ghosts_across_periodic(nx0, ny0, periodic, boxes):
    """the ghost cells (sides of the ring, as tests/ghostring.py walks them) of the boxes of levels >= 1 that lie outside the domain across a periodic
    side and that ghostring.cell_kind calls coarse-fine: no box of the level holds the wrapped cell.  PiecewiseLinearFillPatch of the oracle
    (or_pwl_fill) leaves them alone, the device fills them from the wrapped coarse cell, and which of the two the reference's Chombo does is
    unpinned -- a time step reads them (CellToEdge of B), so tests/stepsweep.py keeps the layouts where this is 0"""
    from tests import ghostring as gr
    n = 0
    for l, bl in enumerate(boxes, start=1):
        dom = (nx0 << l, ny0 << l)
        for b in bl:
            for _, d, s in gr.SIDES:
                for i, j in gr.side_cells(b, d, s):
                    if not (0 <= i < dom[0] and 0 <= j < dom[1]) and gr.cell_kind(i, j, dom, periodic, bl) == "coarse-fine":
                        n += 1
    return n


def analytic_fields(nx0, ny0, boxes, bc):
    """synthetic.amrm_fields on the nx0 x ny0 base, with the ghost cells of B, Pi, zb and the mask across a periodic side replaced by the periodic
    image (synthetic.wrap_ghosts on every level's whole domain, then cut per box).  The library takes these ghost cells from the caller and asks
    for exactly that: the face coefficient of domain face 0 is computed from the ghost on its low side and that of face nxd from the ghost on
    its high side, and the two are ONE face of a periodic level (a reflux across the wrap reads either).  The analytic B of amrm_fields is
    periodic in x and y only up to the rounding of sin and cos: unwrapped, the oracle's own BX differs between face 0 and face nxd in the last
    bit after the first operator update, and a coarse cell with a coarse-fine face on the wrap gets another residual on the device (face 0)
    than on the oracle (face nxd) -- which a generated layout found (FEATURES["x-wrap-two-faces"])."""
    kw = dict(lx=float(nx0), ly=float(ny0), moulin=(0.3 * nx0 + 0.015625, 0.5 * ny0 + 0.015625, 1.0, 30.0))
    fs = sy.amrm_fields(nx0, ny0, boxes, **kw)
    if not (bc["periodic"][0] or bc["periodic"][1]):
        return fs
    whole = sy.amrm_fields(nx0, ny0, [[(0, 0, (nx0 << l) - 1, (ny0 << l) - 1)] for l in range(1, len(boxes) + 1)], **kw)
    for l in range(len(boxes) + 1):
        w = sy.wrap_ghosts(whole[0] if l == 0 else whole[l][0], bc)
        for f, (lo0, lo1, hi0, hi1) in zip([fs[0]] if l == 0 else fs[l], [(0, 0, nx0 - 1, ny0 - 1)] if l == 0 else boxes[l - 1]):
            for k in ("B", "Pi", "zb", "mask"):
                f[k] = np.ascontiguousarray(w[k][lo1:hi1 + 3, lo0:hi0 + 3])
    return fs


def adversarial_fields(nx0, ny0, boxes, bc, seed):
    """analytic_fields with B and the mask replaced: per level, drawn cell by cell over the level's whole ghosted domain, B on both sides of cutOffbr
    and maxOffbr of ADV_PHYS and about 8 % of the mask at -1; periodic-wrapped as synthetic.wrap_ghosts does, then cut per box, so that two
    cuttings of a level see the same data"""
    fs = analytic_fields(nx0, ny0, boxes, bc)
    lo, hi = ADV_PHYS["cutOffbr"], ADV_PHYS["maxOffbr"]
    for l in range(len(boxes) + 1):
        rng = np.random.default_rng([int(seed), 5113, l])
        nx, ny = nx0 << l, ny0 << l
        w = dict(B=rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), size=(ny + 2, nx + 2)),
                 mask=np.where(rng.random((ny + 2, nx + 2)) < 0.08, -1.0, 1.0))
        for a in w.values():
            if bc["periodic"][1]:
                a[0, :], a[-1, :] = a[-2, :].copy(), a[1, :].copy()
            if bc["periodic"][0]:
                a[:, 0], a[:, -1] = a[:, -2].copy(), a[:, 1].copy()
        for f, (lo0, lo1, hi0, hi1) in zip([fs[0]] if l == 0 else fs[l], [(0, 0, nx - 1, ny - 1)] if l == 0 else boxes[l - 1]):
            for k, a in w.items():
                f[k] = np.ascontiguousarray(a[lo1:hi1 + 3, lo0:hi0 + 3])
    return fs


_NP = dict(type=[[0, 1], [1, 0]], value=[[3.0, 0.01], [-0.02, 7.0]], periodic=[0, 0])
_PY = dict(type=[[0, 1], [1, 1]], value=[[2.0, -0.03], [0.0, 0.0]], periodic=[0, 1])
_PX = dict(type=[[1, 1], [1, 0]], value=[[0.0, 0.0], [0.02, -4.0]], periodic=[1, 0])
_PXY = dict(type=[[0, 0], [0, 0]], value=[[0.0, 0.0], [0.0, 0.0]], periodic=[1, 1])

# layouts built on purpose, on the 32 x 16 base (level 1: 64 x 32, level 2: 128 x 64, level 3: 256 x 128): name -> (bc, boxes)
FEATURES = {
    # boxes of 2 x 2, 2 x n and n x 2 cells (block_factor 2), free-standing and abutting, on levels 1 and 2
    "tiny-boxes": (_NP, [[(8, 4, 39, 27), (44, 10, 45, 11), (50, 4, 51, 19), (52, 4, 53, 5), (44, 28, 61, 29)],
                         [(24, 16, 25, 17), (30, 16, 31, 39), (32, 16, 33, 17), (40, 30, 71, 31)]]),
    # boxes in two opposite corners of a non-periodic domain, refined in the corner down to level 3
    "domain-corner": (_NP, [[(0, 0, 15, 11), (48, 20, 63, 31)], [(0, 0, 15, 11)], [(0, 0, 15, 11)]]),
    # two boxes that touch at one corner only; a level-2 box 2 cells from that corner
    "corner-touch": (_PY, [[(16, 8, 31, 19), (32, 20, 47, 27)], [(48, 28, 59, 35)]]),
    # the cut between two boxes ends on the side of a third; a level-2 box across the junction
    "t-junction": (_NP, [[(16, 8, 47, 15), (16, 16, 27, 27), (28, 16, 47, 27)], [(48, 28, 67, 43)]]),
    # x periodic: a box that spans the period (its own neighbour); on level 2 a box against face 0 with no box across the wrap (the coarse-fine
    # stencils and the reflux cross coarse face 0 == face nxd) and one away from it
    "x-wrap-self": (_PX, [[(0, 8, 63, 19)], [(0, 20, 31, 31), (64, 22, 95, 29)]]),
    # x periodic: two boxes that are neighbours only through the wrap, on levels 1 and 2
    "x-wrap-pair": (_PX, [[(0, 4, 15, 19), (48, 4, 63, 19)], [(0, 12, 19, 31), (108, 12, 127, 31)]]),
    # doubly periodic: four boxes that meet in the wrapped corner, a level-2 box in that corner
    "xy-wrap-corner": (_PXY, [[(0, 0, 15, 7), (48, 0, 63, 7), (0, 24, 15, 31), (48, 24, 63, 31)], [(0, 0, 15, 7)]]),
    # a box from side to side of a non-periodic direction, in x on levels 1 and 2, in y on level 1
    "span-x": (_NP, [[(0, 8, 63, 15)], [(0, 20, 127, 27)]]),
    "span-y": (_NP, [[(24, 0, 35, 31)]]),
    # level 1 an L; level-2 boxes whose coarsened boxes grown by 2 just fit into either arm, one of them reaching the cell diagonal to the
    # re-entrant corner; a level-3 box in one of them
    "reentrant-nest-2": (_NP, [[(16, 8, 31, 27), (32, 8, 47, 15)], [(40, 20, 59, 27), (68, 20, 91, 27)], [(84, 44, 115, 51)]]),
    # found by generate(5) with ghost cells that were not the periodic image (analytic_fields): x periodic, coarse cells of level 0 in column 0 with
    # a coarse-fine face of the box on their high side and, through the wrap, one of the box against x-hi; a 2 x 2 box in the corner whose
    # neighbour through the wrap is that box; a level-2 box two rows high on y-lo
    "x-wrap-two-faces": (_PX, [[(28, 0, 31, 3), (46, 0, 47, 13), (2, 0, 25, 31), (48, 0, 63, 5), (0, 0, 1, 1), (26, 0, 27, 1)],
                               [(96, 0, 109, 1), (10, 28, 25, 41)]]),
    # a level-3 box inside a level-2 box of width 6, the narrowest that can hold one
    "level3-in-width-6": (_PY, [[(16, 8, 47, 23)], [(40, 20, 45, 43)], [(84, 48, 87, 79)]]),
}
