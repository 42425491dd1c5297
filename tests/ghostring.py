"""The one-cell ghost ring of a ghosted field, compared side by side and cell kind by cell kind.

A ghost cell of a box is of one of four kinds:
  domain       outside the problem domain across a non-periodic side (the physical boundary condition),
  periodic     across a periodic side, the wrapped cell lies in a box of the same level (possibly the box itself),
  fine-fine    inside the domain, another box of the same level holds the cell (exchange),
  coarse-fine  no box of the level holds the cell (interpolated from the level below).
Corner ghost cells are left out: neither side defines them for the 5-point operator.

ring_equal(ref, dev, ...) compares the ring of two ghosted arrays bitwise, kind by kind; a failure names the side, the
kind and the first differing cell.  domain_bc_holds(a, ...) is the check that needs no oracle: on every domain side the
ring equals npref.fill_ghosts(..., homogeneous=True) of the array's own valid cells (levelGSRB's closing ghost fill,
src/VCAMRNonLinearPoissonOp.cpp:757-759), which holds after any call whose last step is a relaxation."""
import numpy as np

from tests.npref import fill_ghosts

KINDS = ("domain", "periodic", "fine-fine", "coarse-fine")
SIDES = (("x-lo", 0, 0), ("x-hi", 0, 1), ("y-lo", 1, 0), ("y-hi", 1, 1))


def side_of(a, d, s):
    """ring cells of ghosted array a along side (d, s), corners left out"""
    if d == 0:
        return a[1:-1, 0 if s == 0 else -1]
    return a[0 if s == 0 else -1, 1:-1]


def side_cells(box, d, s):
    """global (i, j) of the ghost cells along side (d, s) of box (lo0, lo1, hi0, hi1), in the order side_of returns them"""
    lo0, lo1, hi0, hi1 = box
    if d == 0:
        i = lo0 - 1 if s == 0 else hi0 + 1
        return [(i, j) for j in range(lo1, hi1 + 1)]
    j = lo1 - 1 if s == 0 else hi1 + 1
    return [(i, j) for i in range(lo0, hi0 + 1)]


def cell_kind(i, j, domain, periodic, level_boxes):
    n = domain
    c, wrapped = [i, j], False
    for d in range(2):
        if 0 <= c[d] < n[d]:
            continue
        if not periodic[d]:
            return "domain"
        c[d] %= n[d]
        wrapped = True
    held = any(b[0] <= c[0] <= b[2] and b[1] <= c[1] <= b[3] for b in level_boxes)
    if wrapped and held:
        return "periodic"
    return "fine-fine" if held else "coarse-fine"


def ring_kinds(box, domain, periodic, level_boxes=None):
    """{side name: array of kind names of its ghost cells}; level_boxes = every box of the level (default: box alone)"""
    lb = [tuple(box)] if level_boxes is None else [tuple(b) for b in level_boxes]
    return {name: np.array([cell_kind(i, j, domain, periodic, lb) for i, j in side_cells(box, d, s)])
            for name, d, s in SIDES}


def ring_equal(ref, dev, box, domain, periodic, level_boxes=None, kinds=KINDS, what=""):
    """ring of dev == ring of ref, bitwise, on the ghost cells of the given kinds; returns {kind: cells compared}"""
    assert ref.shape == dev.shape, (what, ref.shape, dev.shape)
    assert ref.shape == (box[3] - box[1] + 3, box[2] - box[0] + 3), (what, ref.shape, box)
    kd = ring_kinds(box, domain, periodic, level_boxes)
    seen = dict.fromkeys(kinds, 0)
    for name, d, s in SIDES:
        a, b, k = side_of(ref, d, s), side_of(dev, d, s), kd[name]
        cells = side_cells(box, d, s)
        for kind in kinds:
            m = k == kind
            seen[kind] += int(m.sum())
            bad = np.flatnonzero(m & ~((a == b) | (np.isnan(a) & np.isnan(b))))
            if bad.size:
                n = bad[0]
                raise AssertionError("%s: ghost ring differs on side %s (%s), first at cell (i, j) = %s: %r != %r (%d of %d cells)"
                                     % (what, name, kind, cells[n], float(b[n]), float(a[n]), bad.size, int(m.sum())))
    return seen


def domain_bc_holds(a, bc, dx, dy, box, domain, what=""):
    """the domain sides of ghosted array a hold the homogeneous boundary condition of its own valid cells; returns the cells checked"""
    g = fill_ghosts(a[1:-1, 1:-1], bc, dx, dy, homogeneous=True)
    dummy = [tuple(box)]
    kd = ring_kinds(box, domain, bc["periodic"], dummy)
    n = 0
    for name, d, s in SIDES:
        m = kd[name] == "domain"
        if not m.any():
            continue
        want, got = side_of(g, d, s), side_of(a, d, s)
        bad = np.flatnonzero(m & (want != got))
        n += int(m.sum())
        if bad.size:
            c = side_cells(box, d, s)[bad[0]]
            raise AssertionError("%s: ghost ring is not the boundary condition of the valid cells on side %s (domain), first at cell "
                                 "(i, j) = %s: %r != %r (%d of %d cells)" % (what, name, c, float(got[bad[0]]), float(want[bad[0]]),
                                                                            bad.size, int(m.sum())))
    return n


def level_ring_equal(ref, dev, domain, periodic, kinds=KINDS, what=""):
    """a single level over the whole domain (ghosted (ny + 2, nx + 2) arrays)"""
    nx, ny = domain
    return ring_equal(ref, dev, (0, 0, nx - 1, ny - 1), domain, periodic, kinds=kinds, what=what)
