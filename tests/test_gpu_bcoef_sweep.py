"""The face-coefficient kernels on the device (suhmo_bcoef.hip: k_bcoef_fused in its four instantiations, the four-kernel path on a whole level,
k_average_faces_all and its per-depth fallback, MGnewOp's coarsening) against the oracle (oracle/level_shim.c) over the sweep of tests/bcoefsweep.py,
BITWISE: every comparison is np.array_equal, there is no tolerance anywhere.  270 cases (27 shapes on the edges of the 62 x 14 and 126 x 14 tiles
x 5 boundary conditions x 2 of 5 x 6 (physics, mask palette) pairs), each under three kernel choices set with set_option: bcoef_fused = 0, the default
tile and bcoef_tile_x = 126 -- 810 compared pairs of face arrays, and the three choices against each other.  tests/test_bcoef_sweep_cpu.py holds what
the oracle alone can say about the same cases (all finite, every census arm taken).  A failure names the case, the kernel choice, the array, the
first differing face and the tile that owns it."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import bcoefsweep as bs

pytestmark = pytest.mark.gpu
SP = dict(sy.SOLVER_DEFAULT, eps=1e-10, norm_thresh=1e-13, max_iter=3, imin=6)
CHOICES = (("bcoef_fused=0", 0, 62), ("default tile", 1, 62), ("bcoef_tile_x=126", 1, 126))


@pytest.fixture(scope="module")
def hip():
    from suhmo_amd import capi, level
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return level


def same(ref, dev, what, btx=62):
    assert ref.shape == dev.shape, (what, ref.shape, dev.shape)
    if not np.array_equal(ref, dev):
        bad = np.argwhere(~(ref == dev))
        j, i = (int(x) for x in bad[0])
        raise AssertionError("%s: %d of %d faces differ, first at (i, j) = (%d, %d) of tile %s (width %d): device %r != reference %r"
                             % (what, len(bad), ref.size, i, j, bs.tile_of(btx, i, j), btx, float(dev[j, i]), float(ref[j, i])))


def device_level(hip, case, f, mb=bs.MAX_BOX):
    cid, nx, ny, b, ph, pal = case
    G = hip.HipLevel(nx, ny, f["dx"], f["dy"], bs.BCS[b], bs.PHYS[ph], 0.0, -1.0, mb)
    G.set_inputs(f)
    return G


def update(G, hip, f, fused, tile):
    """UpdateOperator under one kernel choice, on faces that hold NaN before the call (nothing of an earlier call can pass for this one's)"""
    G.set_option("bcoef_fused", fused); G.set_option("bcoef_tile_x", tile)
    G.set(hip.F_PHI, f["phi"])
    G.set(hip.F_BX, np.full(G.shape(hip.F_BX), np.nan)); G.set(hip.F_BY, np.full(G.shape(hip.F_BY), np.nan))
    G.update_operator()
    G.synchronize()                       # (the scan's answer has arrived when the next call asks)
    return G.get(hip.F_BX), G.get(hip.F_BY)


def counters(G):
    return G.get_option("mask_state"), G.get_option("mask_scans"), G.get_option("bcoef_unmasked_launches")


@pytest.mark.parametrize("case", bs.cases(), ids=lambda c: c[0])
def test_faces_bitwise_under_every_kernel_choice(oracle, hip, case):
    """a. the device against the oracle under each of the three choices; b. the three against each other on the same level object, the head set
    again before each.  The order makes the second call the one that scans the mask, so on the clean palette the third call runs the unmasked
    instantiation (of the wide tile where nx >= 256, else of the default one: bcoef_tile_x = 126 changes nothing there) and must still give
    the masked one's bits; the state the scan leaves is what the census says"""
    cid, nx, ny, b, ph, pal = case
    f = bs.fields(case)
    rbx, rby = bs.oracle_faces(oracle, case, f)
    assert np.isfinite(rbx).all() and np.isfinite(rby).all(), cid
    G = device_level(hip, case, f)
    try:
        got = []
        for name, fused, tile in CHOICES:
            bx, by = update(G, hip, f, fused, tile)
            w = 126 if (tile == 126 and nx >= bs.WIDE_MIN_NX) else 62
            same(rbx, bx, (cid, name, "bx against the oracle"), w); same(rby, by, (cid, name, "by against the oracle"), w)
            got.append((bx, by))
        for k in (0, 2):
            same(got[1][0], got[k][0], (cid, CHOICES[k][0], "bx against the default tile's")); same(got[1][1], got[k][1], (cid, CHOICES[k][0], "by against the default tile's"))
        if bs.is_fused(nx, ny):
            clean = bs.scan_answer(f) == bs.SCAN_CLEAN
            assert counters(G) == (bs.scan_answer(f), 1, 1 if clean else 0), (cid, counters(G))
        else:                             # the four-kernel path knows nothing about the mask
            assert counters(G) == (bs.SCAN_UNKNOWN, 0, 0), (cid, counters(G))
    finally:
        G.close()


# c., d.: (nx, ny, tile width)
SCAN_SHAPES = ((126, 30, 62), (258, 30, 62), (258, 30, 126), (380, 31, 126))


def palette_case(nx, ny, pal):
    cs = bs.find(nx, ny, pal=pal)
    if cs:
        return cs[0]
    b = list(bs.BCS)[(nx + ny) % 5]       # the sweep holds the shape with other palettes: the same inputs otherwise
    return ("%dx%d-%s-cut1-mg1-%s" % (nx, ny, b, pal), nx, ny, b, "cut1-mg1", pal)


@pytest.mark.parametrize("mask_known", [1, 0])
@pytest.mark.parametrize("nx,ny,tile", SCAN_SHAPES, ids=["%dx%d-tile%d" % s for s in SCAN_SHAPES])
def test_clean_palette_runs_unmasked_with_the_masked_bits(oracle, hip, nx, ny, tile, mask_known):
    """c. every value >= 1e-6, among them 0.5 next to 1 (bcoef_face sees unequal masks where the unmasked instantiation passes 1.0 and 1.0): the
    first call scans on the masked kernel, the next one runs unmasked and gives the same bits; with mask_known = 0 nothing is scanned"""
    case = palette_case(nx, ny, "clean")
    f = bs.fields(case)
    assert bs.scan_answer(f) == bs.SCAN_CLEAN and (f["mask"] == 0.5).any()
    rbx, rby = bs.oracle_faces(oracle, case, f)
    G = device_level(hip, case, f)
    try:
        G.set_option("mask_known", mask_known)
        bx1, by1 = update(G, hip, f, 1, tile)
        assert counters(G)[1:] == ((1, 0) if mask_known else (0, 0))
        bx2, by2 = update(G, hip, f, 1, tile)
        assert counters(G) == ((bs.SCAN_CLEAN, 1, 1) if mask_known else (bs.SCAN_UNKNOWN, 0, 0))
        bx3, by3 = update(G, hip, f, 1, tile)
        assert counters(G)[2] == (2 if mask_known else 0)
        for k, (bx, by) in enumerate(((bx1, by1), (bx2, by2), (bx3, by3))):
            same(rbx, bx, (case[0], "call", k, "bx against the oracle"), tile); same(rby, by, (case[0], "call", k, "by against the oracle"), tile)
            same(bx1, bx, (case[0], "call", k, "bx against the first call's"), tile); same(by1, by, (case[0], "call", k, "by against the first call's"), tile)
    finally:
        G.close()


@pytest.mark.parametrize("pal", ["one-cell", "one-ghost-south", "one-ghost-east"])
@pytest.mark.parametrize("nx,ny,tile", SCAN_SHAPES[:1] + SCAN_SHAPES[2:], ids=["%dx%d-tile%d" % s for s in SCAN_SHAPES[:1] + SCAN_SHAPES[2:]])
def test_one_value_below_1e_6_keeps_the_masked_path(oracle, hip, nx, ny, tile, pal):
    """d. the clean palette but for a single 5e-7: in a cell, in the ghost row below row 0, in the ghost column beside column nx - 1"""
    case = palette_case(nx, ny, pal)
    f = bs.fields(case)
    assert (f["mask"] < 1e-6).sum() <= 3 and bs.scan_answer(f) == bs.SCAN_DIRTY
    rbx, rby = bs.oracle_faces(oracle, case, f)
    G = device_level(hip, case, f)
    try:
        for k in range(3):
            bx, by = update(G, hip, f, 1, tile)
            same(rbx, bx, (case[0], "call", k, "bx"), tile); same(rby, by, (case[0], "call", k, "by"), tile)
        assert counters(G) == (bs.SCAN_DIRTY, 1, 0), counters(G)
    finally:
        G.close()


# ---- e. AverageOperator and MGnewOp's coarsening
AVERAGE_CASES = [(s, kind) for s in bs.AVERAGE_SHAPES for kind in (("dirty", "smooth") if s[3] >= 128 else ("dirty",))]


def average_pair(oracle, hip, shape, kind):
    name, nx, ny, mb, nd = shape
    bc, ph = (sy.A3_BC, sy.A3_PHYS) if kind == "smooth" else (bs.BCS["dirichlet"], bs.PHYS["cut1-mg1"])
    f = bs.average_fields(nx, ny, kind, bc)
    O = oracle.OracleLevel(nx, ny, f["dx"], f["dy"], bc, ph, 0.0, -1.0, mb, 2)
    G = hip.HipLevel(nx, ny, f["dx"], f["dy"], bc, ph, 0.0, -1.0, mb)
    assert O.ndepth == nd and G.ndepth == nd, (name, O.ndepth, G.ndepth)
    O.set_inputs(f); G.set_inputs(f)
    return O, G


@pytest.mark.parametrize("shape,kind", AVERAGE_CASES, ids=["%s-%s" % (s[0], k) for s, k in AVERAGE_CASES])
def test_average_operator_at_seven_and_eight_depths(oracle, hip, shape, kind):
    """after one V-cycle the faces of every depth are the oracle's, and they are what per-depth AverageOperator calls give on the same depth-0
    faces.  nd = 7: one pass, the y-face walker's group is the whole wave; nd = 8: the per-depth fallback"""
    O, G = average_pair(oracle, hip, shape, kind)
    try:
        nd = O.ndepth
        O.build_mg_coefficients(); G.build_mg_coefficients()
        O.vcycle(SP); G.vcycle(SP)
        G.synchronize()
        assert np.isfinite(O.get(oracle.F_PHI)).all(), shape[0]
        cyc = [(G.get(hip.F_BX, depth=d), G.get(hip.F_BY, depth=d)) for d in range(nd)]
        for d in range(nd):
            same(O.get(oracle.F_BX, depth=d), cyc[d][0], (shape[0], kind, "after a V-cycle: bx at depth", d))
            same(O.get(oracle.F_BY, depth=d), cyc[d][1], (shape[0], kind, "after a V-cycle: by at depth", d))
        for d in range(1, nd):
            G.set(hip.F_BX, np.full(G.shape(hip.F_BX, depth=d), np.nan), depth=d); G.set(hip.F_BY, np.full(G.shape(hip.F_BY, depth=d), np.nan), depth=d)
            G.average_operator(d)
            same(cyc[d][0], G.get(hip.F_BX, depth=d), (shape[0], kind, "average_operator(d) against the V-cycle's: bx at depth", d))
            same(cyc[d][1], G.get(hip.F_BY, depth=d), (shape[0], kind, "average_operator(d) against the V-cycle's: by at depth", d))
        same(O.get(oracle.F_PHI), G.get(hip.F_PHI), (shape[0], kind, "head after the V-cycle"))
    finally:
        O.close(); G.close()


@pytest.mark.parametrize("shape", bs.AVERAGE_SHAPES, ids=[s[0] for s in bs.AVERAGE_SHAPES])
def test_coarsened_coefficients_of_every_depth(oracle, hip, shape):
    """build_mg_coefficients with the dirty palette: coarse masks become fractions such as 0.25 and -0.5"""
    O, G = average_pair(oracle, hip, shape, "dirty")
    try:
        O.build_mg_coefficients(); G.build_mg_coefficients()
        fractions = 0
        for d in range(1, O.ndepth):
            for nm in ("F_ACOEF", "F_B", "F_PI", "F_ZB", "F_MASK"):
                ref = O.get(getattr(oracle, nm), depth=d)
                same(ref, G.get(getattr(hip, nm), depth=d), (shape[0], nm, "depth", d))
                if nm == "F_MASK":
                    fractions += int(np.count_nonzero((ref != np.round(ref)) & (np.abs(ref) < 1.0)))
        assert fractions > 0
    finally:
        O.close(); G.close()


# ---- f. the faces feed a cycle: one case per tile width, the dirty palette
CYCLE_CASES = ((128, 28, 62), (256, 16, 126))


@pytest.mark.parametrize("nx,ny,tile", CYCLE_CASES, ids=["%dx%d-tile%d" % s for s in CYCLE_CASES])
def test_two_cycles_on_the_swept_faces(oracle, hip, nx, ny, tile):
    """two V-cycles with bcoef_in_relax = 0 and two with its default: the head is the oracle's"""
    case = bs.find(nx, ny, pal="dirty")[0]
    f = bs.fields(case)
    bc, ph = bs.BCS[case[3]], bs.PHYS[case[4]]
    O = oracle.OracleLevel(nx, ny, f["dx"], f["dy"], bc, ph, 0.0, -1.0, bs.MAX_BOX, 2)
    O.set_inputs(f); O.build_mg_coefficients()
    assert O.ndepth >= 2
    ref = []
    for k in range(2):
        O.vcycle(SP)
        ref.append(O.get(oracle.F_PHI))
    O.close()
    assert np.isfinite(ref[1]).all(), case[0]
    for in_relax in (0, None):
        G = device_level(hip, case, f)
        try:
            assert G.ndepth >= 2
            G.set_option("bcoef_tile_x", tile)
            if in_relax is not None:
                G.set_option("bcoef_in_relax", in_relax)
            G.build_mg_coefficients()
            for k in range(2):
                G.vcycle(SP); G.synchronize()
                same(ref[k], G.get(hip.F_PHI), (case[0], "bcoef_in_relax", in_relax, "head after cycle", k))
        finally:
            G.close()
