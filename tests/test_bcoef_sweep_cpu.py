"""The face-coefficient sweep of tests/bcoefsweep.py on the CPU oracle alone (oracle/level_shim.c: wflx_level, or_level_average_operator): every
case builds, the oracle's faces are finite in every case (a condition of the bitwise comparison on the device, not a tolerance: no case is skipped
or filtered), the sweep contains the shapes, rows and mask values it claims, every arm of the census is taken for both tile widths (printed and
pinned by tests/golden/BCOEF_SWEEP_CENSUS.txt), and AverageOperator runs at seven and at eight depths.  tests/test_gpu_bcoef_sweep.py compares the
device with the oracle on the same cases, bitwise."""
import os

import numpy as np
import pytest

from tests import bcoefsweep as bs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "BCOEF_SWEEP_CENSUS.txt")


@pytest.fixture(scope="module")
def sweep(oracle):
    """UpdateOperator of every case on the oracle and its census, once for the module"""
    return bs.sweep_census(oracle)


def test_the_tables_hold_what_the_sweep_claims():
    cs = bs.cases()
    assert len(cs) == 2 * len(bs.SHAPES) * len(bs.BCS) and len({c[0] for c in cs}) == len(cs)
    assert max(nx * ny for nx, ny in bs.SHAPES) == 380 * 43
    assert {tuple(bc["periodic"]) for bc in bs.BCS.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)} and len(bs.BCS) == 5
    # every listed nx and every listed ny under every boundary-condition row, with the dirty palette and with another one
    for b in bs.BCS:
        for dirty in (True, False):
            mine = [c for c in cs if c[3] == b and (c[5] == "dirty") == dirty]
            assert {c[1] for c in mine} >= set(bs.LISTED_NX) and {c[2] for c in mine} >= set(bs.LISTED_NY), b
    # the x edges of the 62-wide tile each with two ny
    for nx in (61, 62, 63, 124, 126, 127, 128):
        assert len({s[1] for s in bs.SHAPES if s[0] == nx}) == 2, nx
    # pairs of rows of two tables: all of them
    pairs = lambda a, b: {(c[a], c[b]) for c in cs}
    assert len(pairs(3, 4)) == len(bs.BCS) * len(bs.PHYS) and len(pairs(3, 5)) == len(bs.BCS) * len(bs.PALETTES)
    assert len(pairs(4, 5)) == len(bs.PHYS) * len(bs.PALETTES)
    assert {(p["cutOffB"], p["use_mask_gradients"]) for p in bs.PHYS.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # (4, 4) doubly periodic: narrower than tile plus halo
    assert bs.find(4, 4, bc="xy-periodic", pal="dirty")
    # an INTERIOR tile of either width
    assert any(t[2] for t in bs.owners(126, 30, 62)[2]) and any(t[2] for t in bs.owners(380, 31, 126)[2])
    assert not any(t[2] for t in bs.owners(124, 43, 62)[2]) and not any(t[2] for t in bs.owners(256, 16, 126)[2])


def test_palettes_put_both_sides_of_every_threshold_into_the_ghosted_mask():
    assert bs.BELOW < 1.0e-6 and bs.BELOW > 5.0e-7 and set(bs.CLEAN) < set(bs.DIRTY) and min(bs.CLEAN) == 1.0e-6
    assert abs(1.0 - (1.0 + 5.0e-11)) < 1e-10 < abs(1.0 - (1.0 + 2.0e-10)) and abs((1.0 + 2.0e-10) - (1.0 + 5.0e-11)) > 1e-10
    inner = lambda a: a[1:-1, 1:-1]
    sides = lambda a: np.concatenate([a[0, 1:-1], a[-1, 1:-1], a[1:-1, 0], a[1:-1, -1]])
    for case in bs.cases():
        cid, nx, ny, b, ph, pal = case
        f = bs.fields(case)
        m, bc = f["mask"], bs.BCS[b]
        assert (f["B"] >= 0.0).all() and bs.fields(case)["mask"].tobytes() == m.tobytes(), cid
        if nx * ny >= 61 * 13:
            assert (f["B"] == 0.0).any() and (f["B"] == 1.0e-16).any(), cid
        if pal == "dirty":
            assert set(np.unique(m)) <= set(bs.DIRTY), cid
            if nx * ny >= 61 * 13:
                for v in bs.DIRTY:
                    assert (inner(m) == v).any() and (sides(m) == v).any(), (cid, v)
                assert np.signbit(m[m == 0.0]).any() and not np.signbit(m[m == 0.0]).all(), cid
            assert bs.scan_answer(f) == bs.SCAN_DIRTY or nx * ny < 16, cid
        elif pal == "clean":
            assert set(np.unique(m)) <= set(bs.CLEAN) and bs.scan_answer(f) == bs.SCAN_CLEAN, cid
        elif pal == "plus-minus":
            assert set(np.unique(m)) <= {-1.0, 1.0}, cid
        else:
            low = np.argwhere(m < 1.0e-6)
            assert bs.scan_answer(f) == bs.SCAN_DIRTY and (m[m < 1.0e-6] == bs.ONE).all(), cid
            if pal == "one-cell":          # one cell of the level (and its periodic images in the ring)
                assert (inner(m) < 1.0e-6).sum() == 1, cid
            elif pal == "one-ghost-south":
                assert len(low) == 1 and low[0][0] == 0 and 1 <= low[0][1] <= nx, cid
            else:
                assert len(low) == 1 and low[0][1] == nx + 1 and 1 <= low[0][0] <= ny, cid
        if pal in ("dirty", "clean", "plus-minus", "one-cell"):           # periodic sides: the ring is the periodic image
            if bc["periodic"][0]:
                assert np.array_equal(m[:, 0], m[:, -2]) and np.array_equal(m[:, -1], m[:, 1]), cid
            if bc["periodic"][1]:
                assert np.array_equal(m[0, :], m[-2, :]) and np.array_equal(m[-1, :], m[1, :]), cid


def test_the_plus_minus_baseline_cannot_tell_the_two_thresholds_apart():
    """why the palettes: with masks of +1 and -1 alone `< 1e-6` and `< 0` are the same question"""
    for case in bs.cases():
        if case[5] == "plus-minus":
            cen = bs.census(bs.fields(case), bs.BCS[case[3]], bs.PHYS[case[4]])
            assert all(cen["gradient z" + s]["true with < 1e-6, false with < 0"] == 0 for s in "WESN"), case[0]


def test_every_face_has_one_owner():
    """the restatement of the tiles: every face of a level is stored by exactly one tile, for both widths"""
    for nx, ny in bs.SHAPES:
        for w in bs.widths_of(nx, ny):
            fx, fy, tiles = bs.owners(nx, ny, w)
            assert (fx.sum(axis=0) == 1).all() and (fy.sum(axis=0) == 1).all(), (nx, ny, w)
            assert all(t[3] <= w + 1 and t[4] <= bs.BT_Y + 1 for t in tiles), (nx, ny, w)
    assert bs.widths_of(3, 5) == () and bs.widths_of(128, 43) == (62,) and bs.widths_of(256, 16) == (62, 126)


def test_every_case_builds_and_its_faces_are_finite(sweep):
    assert sweep["ncases"] == len(bs.cases()) == 270
    assert not sweep["problems"], "\n".join(sweep["problems"][:20])


def test_every_arm_is_taken(sweep):
    print("\n" + bs.census_table(sweep))
    missing = []
    for (br, arm), (n, cases, shapes) in sweep["arms"].items():
        if (br, arm) in bs.NOT_TAKEN:
            assert n == 0, (br, arm)
        elif len(cases) < 2 or n == 0:
            missing.append((br, arm, n, len(cases), len(shapes)))
    assert not missing, missing
    assert len(sweep["arms"]) >= 50
    for w in bs.TILE_WIDTHS:
        assert sweep["arms"][("tile %d: faces" % w, "of an INTERIOR tile")][0] > 0, w


def test_census_table_is_the_committed_one(sweep):
    """tests/golden/BCOEF_SWEEP_CENSUS.txt is what tools/bcoef_sweep_census.py writes: recorded results, regenerated when the sweep changes"""
    with open(GOLD) as f:
        assert f.read() == bs.census_table(sweep)


@pytest.mark.parametrize("name,nx,ny,mb,nd", bs.AVERAGE_SHAPES, ids=[s[0] for s in bs.AVERAGE_SHAPES])
def test_average_operator_runs_at_every_depth(oracle, name, nx, ny, mb, nd):
    bc = bs.BCS["dirichlet"]
    f = bs.average_fields(nx, ny, "dirty", bc)
    O = oracle.OracleLevel(nx, ny, f["dx"], f["dy"], bc, bs.PHYS["cut1-mg1"], 0.0, -1.0, mb, 2)
    try:
        assert O.ndepth == nd
        O.set_inputs(f)
        O.update_operator()
        for d in range(1, nd):
            O.average_operator(d)
            bx, by = O.get(oracle.F_BX, depth=d), O.get(oracle.F_BY, depth=d)
            assert bx.shape == (ny >> d, (nx >> d) + 1) and np.isfinite(bx).all() and np.isfinite(by).all(), d
            assert (bx != 0.0).any() and (by != 0.0).any(), d
    finally:
        O.close()
