"""The rank-strip sweep of tests/stripsweep.py on the CPU oracle alone: the table holds the axes it claims and every pair of their values, every side
of every threshold of the relaxation scheduler is taken (printed and pinned by tests/golden/STRIP_SWEEP_CENSUS.txt), the strips of every case have
the whole level's number of multigrid depths, the oracle stays finite through the piecewise part and the cycle part of every case, and every
relaxation and every V-cycle changes every row near a rank boundary, so that a stale halo row cannot pass for a current one.  No case is filtered:
what would be left out is named in stripsweep.EXCLUDED.  tests/test_gpu_strip_sweep.py runs the same cases on thread ranks, bitwise."""
import itertools
import os

import numpy as np
import pytest

from tests import stripsweep as ss

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "STRIP_SWEEP_CENSUS.txt")


def test_the_table_holds_what_the_sweep_claims():
    cs = ss.cases()
    assert 200 <= len(cs) <= 300 and len({c[0] for c in cs}) == len(cs)
    assert [ss.axis_values(c) for c in cs[:len(ss.ANCHORS)]] == [tuple(v[i] for v, i in zip(ss._VALUES, a)) for a in ss.ANCHORS]
    for c in cs:
        cid, nx, nyt, world, mb, halo = c[:6]
        assert nyt % world == 0 and (nyt // world) % mb == 0 and nx % 2 == 0, cid       # equal strips of whole boxes, column pairs
        assert nx <= 130 and nyt <= 384, cid
    assert max(c[1] * c[2] for c in cs) <= 130 * 384 and max(c[2] for c in cs) == 384 and max(c[1] for c in cs) == 130
    # the values the issue names, all of them
    assert {h for h, mb in ss.HEIGHTS} == {8, 12, 16, 24, 40, 48, 72, 96} and set(ss.NX) >= {18, 30, 34, 62, 64, 66, 120, 122, 124, 126, 130}
    assert ss.WORLD == (2, 3, 4) and ss.HALO == (1, 2, 3, 4, 5, 8, 9, 10, 11, 16, 24) and ss.ALPHA == (0.0, 0.5)
    assert {tuple(b["periodic"]) for b in ss.BCS.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert ss.SWEEPS == ((1,), (2,), (3,), (4,), (5,), (7,), (2, 3, 4)) and set(ss.SOLVER) == set(itertools.product((1, 2, 3, 4, 5), (1, 16)))
    assert len(ss.OPTIONS) == 21
    # halos deeper than the strip: the exchange moves min(gy, ny) rows
    assert sum(1 for c in cs if c[5] > c[2] // c[3]) >= 10
    # y-periodic on 2 ranks (both neighbours are the same rank) and on 3 and 4; x-periodic widths the tile kernel takes (a multiple of nothing: any
    # even nx) and widths the streaming kernel refuses (nx < 64)
    for w in ss.WORLD:
        assert any(c[3] == w and ss.BCS[c[6]]["periodic"][1] for c in cs), w
    xp = {c[1] for c in cs if ss.BCS[c[6]]["periodic"][0]}
    assert min(xp) < 64 <= max(xp)


def test_every_value_and_every_pair_of_values_occurs():
    vals = [ss.axis_values(c) for c in ss.cases() if c[0] not in ss.EXCLUDED]
    for a, va in enumerate(ss._VALUES):
        assert {v[a] for v in vals} == set(va), ss.AXES[a]
        for b in range(a + 1, len(ss._VALUES)):
            missing = set(itertools.product(va, ss._VALUES[b])) - {(v[a], v[b]) for v in vals}
            assert not missing, (ss.AXES[a], ss.AXES[b], sorted(missing, key=str)[:5])


def test_nothing_is_left_out():
    cs = ss.cases()
    assert len(ss.EXCLUDED) == 0 and len(ss.EXCLUDED) <= len(cs) // 20 and set(ss.EXCLUDED) <= {c[0] for c in cs}
    assert all(isinstance(r, str) and r for r in ss.EXCLUDED.values())


def test_every_side_of_every_threshold_is_taken():
    c = ss.census()
    print("\n" + "\n".join(ss.census_table(c).split("\n\n")[1].splitlines()))
    names = list(ss.sides(2, 2, 1))
    missing = []
    for t in names:
        values = {k[1] for k in c["arms"] if k[0] == t}
        assert len(values) >= 2, t
        for v in values:
            d0, co = c["arms"].get((t, v, "depth 0")), c["arms"].get((t, v, "coarse"))
            if (t, v) in ss.NOT_AT_DEPTH0:
                assert d0 is None, (t, v)
            elif d0 is None or len(d0[1]) < 2 or len(d0[2]) < 2:
                missing.append((t, v, "depth 0"))
            if (t, v) in ss.NOT_AT_COARSE:
                assert co is None, (t, v)
            elif co is None or len(co[1]) < 2:
                missing.append((t, v, "coarse"))
    assert not missing, missing
    # both sides of the true / false thresholds somewhere
    for t in names:
        if not t.startswith("tile"):
            assert {k[1] for k in c["arms"] if k[0] == t} == {True, False}, t


def test_census_table_is_the_committed_one():
    """tests/golden/STRIP_SWEEP_CENSUS.txt is what tools/strip_sweep_census.py writes: recorded results, regenerated when the sweep changes"""
    with open(GOLD) as f:
        assert f.read() == ss.census_table(ss.census())


def test_strips_have_the_whole_levels_depths(oracle):
    assert ss.depth_problems(oracle) == []
    assert ss.strip_ndepth(64, 48, 16, 48, 96) == 4 and ss.strip_ndepth(18, 8, 8, 0, 16) == 1 and ss.strip_ndepth(128, 96, 32, 96, 384) == 5


def _rows_changed(a, b):
    return (a != b).any(axis=1)


def test_the_oracle_stays_finite_and_changes_every_row_near_a_rank_boundary(oracle):
    problems = []
    for case in ss.cases():
        cid, nx, nyt, world, mb, halo, bc = case[:7]
        f = ss.fields(case)
        near = ss.rank_boundary_rows(nyt, world, halo, ss.BCS[bc]["periodic"][1])
        assert near.any(), cid
        pieces, nd = ss.oracle_pieces(oracle, case, f)
        for name, d in pieces:
            for k, v in d.items():
                if not np.isfinite(v).all():
                    problems.append("%s: %s after %s is not finite" % (cid, k, name))
        p0, p1, p5 = f["phi"], pieces[0][1]["PHI"], pieces[-1][1]["PHI"]
        if not (_rows_changed(p0, p1)[near].all() and _rows_changed(pieces[3][1]["PHI"], p5)[near].all()):
            problems.append("%s: a relaxation leaves a row near a rank boundary unchanged" % cid)
        for name, d in pieces[1:4]:
            assert np.array_equal(d["PHI"], p1), (cid, name)            # the operators between the two relaxations leave phi alone
        cy = ss.oracle_cycle(oracle, case, f)
        assert cy["ndepth"] == nd
        prev = f["phi"]
        for key in ("v1", "v2"):
            for d, (phi, res) in cy[key].items():
                if not (np.isfinite(phi).all() and np.isfinite(res).all()):
                    problems.append("%s: depth %d after %s is not finite" % (cid, d, key))
            if not _rows_changed(prev, cy[key][0][0])[near].all():
                problems.append("%s: V-cycle %s leaves a row near a rank boundary unchanged" % (cid, key))
            prev = cy[key][0][0]
        # the coarse depths: their phi is written anew in every cycle (restriction, then smoothing)
        for d in range(1, nd):
            nr = ss.rank_boundary_rows(nyt, world, halo, ss.BCS[bc]["periodic"][1], depth=d)
            if not _rows_changed(cy["v1"][d][0], cy["v2"][d][0])[nr].all():
                problems.append("%s: depth %d: the second V-cycle leaves a row near a rank boundary unchanged" % (cid, d))
        if not (np.isfinite(cy["phi"]).all() and np.isfinite(cy["res"]).all() and np.isfinite(cy["hist"]).all() and 1 <= cy["n"] <= 3):
            problems.append("%s: the solve ends in NaN or outside its iteration count (%r)" % (cid, cy["n"]))
    assert not problems, "\n".join(problems[:30])


def test_exact_sums_are_exact():
    """the reference of norm(., 2) and dot: two_prod splits every product without error, fsum adds without error"""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    x, y = rng.uniform(-900.0, 900.0, 301) * 10.0 ** rng.integers(-12, 4, 301), rng.uniform(-1.0, 1.0, 301)
    p, e = ss.two_prod(x, y)
    assert all(Fraction(a) * Fraction(b) == Fraction(c) + Fraction(d) for a, b, c, d in zip(x.tolist(), y.tolist(), p.tolist(), e.tolist()))
    s, b = ss.exact_dot(x, y)
    exact = sum(Fraction(a) * Fraction(c) for a, c in zip(x.tolist(), y.tolist()))
    assert abs(Fraction(s) - exact) <= abs(exact) * Fraction(1, 2 ** 53) and b > 0.0
    assert abs(float(np.dot(x, y)) - s) <= b
