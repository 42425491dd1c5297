"""tests/regrid_ref.py, the numpy twin of "REGRID: FIELD TRANSFER" (include/suhmo_hip.h), pinned by itself: against the oracle's
PiecewiseLinearFillPatch away from the domain sides, by hand at the sides, and by the properties the rule must have.  No device.

One sentence of the issue behind the rule does not hold as written and is tested as what the rule gives instead: "for an affine field eta = 1
in every cell ... at a domain side the tangential eta still evaluates to 1".  With deltasum = 0.5 (|s0| + |s1|) as FORT_INTERPLIMIT has it, a
cell on an x side of c = a I + b J sees smax - c0 or c0 - smin = |b| only (the column beyond the side is missing), so eta = min(1, 2 |b| /
(|a| + |b|)): 1 when |b| >= |a| (or b = 0, where the slope it would cut is 0), below 1 otherwise.  test_affine_fields_are_reproduced uses
dyadic affine fields for which the statement is true on every side (|a| = |b|, or along one axis) and asserts exactness in EVERY cell;
test_affine_field_steeper_across_a_side_is_cut pins the other case by hand."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import regrid_ref as rr


def test_interior_arithmetic_is_the_oracles_pwl_fill():
    from oracle import pyoracle as po
    nx0 = ny0 = 16
    patch = (4, 3, 11, 12)
    A = po.OracleAmrModel(nx0, ny0, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS, dict(sy.A3_MODEL), (patch,), max_box=16, nthreads=1)
    try:
        rng = np.random.default_rng(11)
        # smooth + rough, so that the limiter cuts in a good share of the cells and leaves the rest alone
        I, J = np.meshgrid(np.arange(nx0), np.arange(ny0))
        c = 0.35 * I - 0.2 * J + rng.uniform(-0.5, 0.5, size=(ny0, nx0))
        A.field(0, po.OM_B)[:] = 0.0
        A.field(0, po.OM_B)[1:-1, 1:-1] = c
        A.field(1, po.OM_B)[:] = -7.0
        A.fill_ghosts(1, po.OM_B, "pwl")
        g = np.array(A.field(1, po.OM_B))
    finally:
        A.close()
    lo0, lo1 = 2 * patch[0], 2 * patch[1]
    ny, nx = g.shape[0] - 2, g.shape[1] - 2
    n = cut = 0
    for jj in range(ny + 2):
        for ii in range(nx + 2):
            if 1 <= ii <= nx and 1 <= jj <= ny:
                continue
            gi, gj = lo0 + ii - 1, lo1 + jj - 1
            Ic, Jc = gi >> 1, gj >> 1
            assert 1 <= Ic <= nx0 - 2 and 1 <= Jc <= ny0 - 2          # all eight neighbours
            v, eta = rr.interp_cell(c, Ic, Jc, (nx0, ny0), (0, 0))
            assert v[gj & 1][gi & 1] == g[jj, ii], ("ghost cell", gi, gj, v[gj & 1][gi & 1], g[jj, ii])
            assert rr.pwl_cell(c, gi, gj, (nx0, ny0))[0] == g[jj, ii]
            n += 1
            cut += eta is not None and eta < 1.0
    assert n == 2 * (nx + ny) + 4
    share = cut / n
    print("limiter active in %d of %d cells (%.2f)" % (cut, n, share))
    assert 0.2 < share < 0.8
    assert np.all(g[1:-1, 1:-1] == -7.0)


AFFINE = [(1.0, 1.0), (0.5, -0.5), (-0.25, -0.25), (2.0, 0.0), (0.0, -0.125)]


@pytest.mark.parametrize("periodic", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("a,b", AFFINE)
def test_affine_fields_are_reproduced(periodic, a, b):
    nx0, ny0 = 8, 4
    I, J = np.meshgrid(np.arange(nx0), np.arange(ny0))
    c = 3.0 + a * I + b * J
    for Jc in range(ny0):
        for Ic in range(nx0):
            # (a periodic side of an affine field is a jump, not a slope: those cells are left to the other tests)
            if (periodic[0] and Ic in (0, nx0 - 1)) or (periodic[1] and Jc in (0, ny0 - 1)):
                continue
            v, eta = rr.interp_cell(c, Ic, Jc, (nx0, ny0), periodic)
            on_side = Ic in (0, nx0 - 1) or Jc in (0, ny0 - 1)
            corner = Ic in (0, nx0 - 1) and Jc in (0, ny0 - 1)
            if not on_side:
                assert eta == 1.0                            # smax - c0 = c0 - smin = |s0| + |s1| = 2 deltasum
            if on_side and not corner and a != 0.0 and b != 0.0:
                assert eta == 1.0                            # |a| = |b|: the tangential range is exactly deltasum
            for q in range(2):
                for p in range(2):
                    exact = 3.0 + a * (Ic + 0.25 * (2 * p - 1)) + b * (Jc + 0.25 * (2 * q - 1))
                    assert v[q][p] == exact, (Ic, Jc, p, q)


def test_affine_field_steeper_across_a_side_is_cut():
    # c = I + 0.25 J on x-lo: s0 = 1 one-sided and exact, s1 = 0.25 central; smin = c0 - 0.25, deltasum = 0.625, eta = 0.25 / 0.625 = 0.4
    nx0, ny0 = 8, 8
    I, J = np.meshgrid(np.arange(nx0), np.arange(ny0))
    c = 1.0 * I + 0.25 * J
    v, eta = rr.interp_cell(c, 0, 3, (nx0, ny0), (0, 0))
    assert eta == 0.25 / 0.625
    s1 = eta * 0.25
    c0 = 0.75
    assert v[0][0] == (c0 + 1.0 * -0.25) + s1 * -0.25 and v[1][1] == (c0 + 1.0 * 0.25) + s1 * 0.25
    # the same cell one column in has all its neighbours: smin = c0 - 1.25 = -2 deltasum, eta = 1, exact
    v, eta = rr.interp_cell(c, 1, 3, (nx0, ny0), (0, 0))
    assert eta == 1.0 and v[1][0] == 1.75 - 0.25 + 0.0625


HAND = np.array([[4.0, 1.0, 0.0, 2.0],
                 [2.0, 3.0, 5.0, 1.0],
                 [1.0, 1.5, 2.0, 8.0],
                 [0.0, 6.0, 1.0, 3.0]])          # HAND[J][I]


def test_hand_case_at_a_side():
    # cell (I, J) = (0, 1), c0 = 2, on x-lo of a non-periodic 4 x 4 level: N = {x}
    # s0 = c(1,1) - c0 = 3 - 2 = 1 (one-sided, not limited); s1 = 0.5 (c(0,2) - c(0,0)) = 0.5 (1 - 4) = -1.5
    # existing cells: I in {0, 1}, J in {0, 1, 2}: 4, 1, 2, 3, 1, 1.5 -> smax = 4, smin = 1
    # deltasum = 0.5 (1 + 1.5) = 1.25; etamax = 2 / 1.25 = 1.6, etamin = 1 / 1.25 = 0.8 -> eta = 0.8; s1 = 0.8 x -1.5 = -1.2 (up to rounding)
    v, eta = rr.interp_cell(HAND, 0, 1, (4, 4), (0, 0))
    assert eta == 1.0 / 1.25
    s0, s1 = 1.0, (1.0 / 1.25) * -1.5
    for q in range(2):
        for p in range(2):
            w = 2.0
            w = w + s0 * (0.25 if p else -0.25)
            w = w + s1 * (0.25 if q else -0.25)
            assert v[q][p] == w
    assert abs(v[0][0] - (2.0 - 0.25 + 0.3)) < 1e-15 and abs(v[1][1] - (2.0 + 0.25 - 0.3)) < 1e-15
    # with both slopes limited (PiecewiseLinearFillPatch's way) the normal slope would be 0.8: not what (a) does
    assert rr.limited_slopes(*rr._block(HAND, 0, 1, (4, 4), (0, 0), True), False)[0] == 0.8


def test_hand_case_at_a_corner():
    # cell (3, 3), c0 = 3, in the x-hi / y-hi corner: N = both, no slope limited although the limiter would cut
    # s0 = c0 - c(2,3) = 3 - 1 = 2; s1 = c0 - c(3,2) = 3 - 8 = -5; existing: 2, 8, 1, 3 -> smax = 8, smin = 1; deltasum = 3.5
    # etamax = 5 / 3.5, etamin = 2 / 3.5 -> eta = 4 / 7 < 1, applied to nothing
    v, eta = rr.interp_cell(HAND, 3, 3, (4, 4), (0, 0))
    assert eta == 2.0 / 3.5
    assert v[0][0] == (3.0 - 0.5) + 1.25 and v[0][1] == (3.0 + 0.5) + 1.25 and v[1][0] == (3.0 - 0.5) - 1.25 and v[1][1] == (3.0 + 0.5) - 1.25


def test_periodic_side_gives_the_central_slope_with_the_wrapped_neighbour():
    # cell (0, 1) again, x periodic: the low neighbour is column 3.  s0 = 0.5 (c(1,1) - c(3,1)) = 0.5 (3 - 1) = 1, s1 = -1.5 as before
    # all nine cells exist: 2, 4, 1 / 1, 2, 3 / 8, 1, 1.5 -> smax = 8, smin = 1; deltasum = 1.25; etamin = 0.8 -> both slopes x 0.8
    v, eta = rr.interp_cell(HAND, 0, 1, (4, 4), (1, 0))
    assert eta == 1.0 / 1.25
    s0, s1 = eta * 1.0, eta * -1.5
    assert v[0][0] == (2.0 + s0 * -0.25) + s1 * -0.25 and v[1][1] == (2.0 + s0 * 0.25) + s1 * 0.25
    # y periodic at the corner cell (3, 3): the y neighbours are rows 2 and 0, x stays one-sided
    c, ex = rr._block(HAND, 3, 3, (4, 4), (0, 1), True)
    assert [row[2] for row in ex] == [False, False, False] and ex[2][1] and c[2][1] == 2.0
    s0, s1, _, _ = rr.limited_slopes(c, ex, True)
    eta = rr.interp_cell(HAND, 3, 3, (4, 4), (0, 1))[1]
    assert s0 == 2.0 and s1 == eta * (0.5 * (2.0 - 8.0))


def test_children_average_to_the_coarse_value():
    """to 2 ulp of the largest of the five numbers involved: a child is c0 +- s0 / 4 +- s1 / 4 rounded twice, so where the slopes are large
    against c0 (a coarse value near 0 between neighbours of order 1) the rounding errors are ulps of the children, not of c0 -- no arithmetic
    can do better there"""
    rng = np.random.default_rng(3)
    c = rng.uniform(-2.0, 5.0, size=(6, 9))
    for periodic in [(0, 0), (1, 1)]:
        for J in range(6):
            for I in range(9):
                v, _ = rr.interp_cell(c, I, J, (9, 6), periodic)
                s = 0.0
                s = s + v[0][0]; s = s + v[0][1]; s = s + v[1][0]; s = s + v[1][1]
                scale = max(abs(c[J, I]), max(abs(x) for row in v for x in row))
                assert abs(s * 0.25 - c[J, I]) <= 2 * np.spacing(scale), (I, J, s * 0.25, c[J, I])


def test_copy_wins_and_old_ghost_cells_are_never_read():
    nx0 = ny0 = 8
    rng = np.random.default_rng(5)
    base = np.full((ny0 + 2, nx0 + 2), np.nan)
    base[1:-1, 1:-1] = rng.uniform(0.0, 1.0, size=(ny0, nx0))          # (the ghost ring of level 0 is not read either)
    old_boxes = [[(2, 2, 7, 9), (8, 4, 11, 9)]]
    new_boxes = [[(4, 0, 9, 7), (4, 8, 13, 13)]]
    old = []
    for lo0, lo1, hi0, hi1 in old_boxes[0]:
        a = np.full((hi1 - lo1 + 3, hi0 - lo0 + 3), np.nan)
        a[1:-1, 1:-1] = 100.0 + rng.uniform(0.0, 1.0, size=(hi1 - lo1 + 1, hi0 - lo0 + 1))
        old.append(a)
    new = rr.regrid(nx0, ny0, (0, 0), old_boxes, new_boxes, [old], base, "extrap")
    pure = rr.regrid(nx0, ny0, (0, 0), [], new_boxes, [], base, "extrap")
    was = rr.level_array(16, 16, old_boxes[0], old)
    seen_old = seen_new = 0
    for (lo0, lo1, hi0, hi1), g, gp in zip(new_boxes[0], new[0], pure[0]):
        assert not np.isnan(g).any()
        w = was[lo1:hi1 + 1, lo0:hi0 + 1]
        held = ~np.isnan(w)
        assert np.array_equal(g[1:-1, 1:-1][held], w[held])                     # the copy, bit for bit
        assert np.array_equal(g[1:-1, 1:-1][~held], gp[1:-1, 1:-1][~held])      # the interpolation elsewhere
        assert np.all(gp[1:-1, 1:-1] < 2.0)
        seen_old += int(held.sum()); seen_new += int((~held).sum())
    assert seen_old > 0 and seen_new > 0
    # box 0 lies against y-lo: its ghost row there is extrapolated from its own two first rows; the corner ghosts beyond the side stay 0
    g = new[0][0]
    assert np.array_equal(g[0, 1:-1], 2.0 * g[1, 1:-1] - g[2, 1:-1]) and g[0, 0] == 0.0 and g[0, -1] == 0.0
    # the ghost cells between the two new boxes are each other's valid cells
    assert np.array_equal(new[0][0][-1, 1:-1], new[0][1][1, 1:7]) and np.array_equal(new[0][1][0, 1:7], new[0][0][-2, 1:-1])
