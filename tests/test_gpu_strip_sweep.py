"""The rank-strip sweep of tests/stripsweep.py on the device: every case runs as thread ranks on one GPU (tests/test_gpu_strips.py: run_strips)
and is compared with the CPU oracle's whole level BIT FOR BIT -- GSRB is colour-Jacobi, a partition may not change a bit -- NaN equal to NaN.

(a) pieces: gsrb(sweep row), residual, apply_op, update_operator, gsrb again (the second relaxation starts from whatever Depth::phi_fresh the
    operators left): PHI, RES, LPHI, BX, BY, the max norm; norm(., 2) and dot against exact sums within the worst case over every summation order.
(b) cycle: build_mg_coefficients, two V-cycles, a solve: PHI (and PHI, RES of every coarse depth the strips hold themselves) after each V-cycle,
    PHI, RES, iteration count and residual history of the solve, the number of depths.
(c) the halo invariant, after every step of (a) and every V-cycle of (b), on every depth and every side that is a rank boundary: with
    r = suhmo_level_phi_halo_fresh(L, depth), 0 <= r <= min(gy, ny) and the halo rows 1 .. r of PHI (read off the canvas through
    suhmo_level_field_view) are the neighbouring rank's owned rows bit for bit.  An overstated count fails here before it costs a bit elsewhere.
(d) every option row runs the branch it exists for: per row the counters of stripsweep.OPTIONS are non-zero in at least one of its cases and
    the forbidden ones zero in all; along a ladder of halo depths a deeper halo never needs more exchanges per V-cycle."""
import ctypes as C

import numpy as np
import pytest

from tests import stripsweep as ss
from tests.test_gpu_strips import run_strips

pytestmark = pytest.mark.gpu

CASES = [c for c in ss.cases() if c[0] not in ss.EXCLUDED]
SEEN = {}          # option row -> {"pieces": set of case ids, "cycle": set of case ids, counter: cases in which it was non-zero on some rank}
EXCHANGES = {}     # case id -> exchanger calls of rank 0 (pieces, first V-cycle, second V-cycle, solve)


def _describe(case, what, depth, field, ref, got, jd):
    cid, nx, nyt, world, mb, halo, bc = case[:7]
    j, i = jd
    ny = (nyt // world) >> depth
    near = ss.rank_boundary_rows(nyt, world, halo, ss.BCS[bc]["periodic"][1], depth)
    jj = min(j, len(near) - 1)          # (the last face row of BY belongs to the last rank)
    return ("%s: %s, depth %d, field %s: first difference at row %d (rank %d, its row %d), column %d, %s %d halo rows of a rank boundary: "
            "device %r, oracle %r" % (cid, what, depth, field, j, jj // ny, jj % ny, i, "within" if near[jj] else "NOT within", halo, got[j, i], ref[j, i]))


def _same(case, what, depth, field, got, ref):
    d = ss.first_difference(got, ref)
    if d is not None and d[0] == "shape":
        raise AssertionError("%s: %s, depth %d, field %s: shapes %r" % (case[0], what, depth, field, d[1:]))
    assert d is None, _describe(case, what, depth, field, ref, got, d)


def _halo_rows(G, tr, depth, side, r):
    """the r halo rows of PHI beyond the strip's lower (side 0) / upper edge off the canvas, valid columns, ordered by row index"""
    from suhmo_amd import capi, level as lv
    base, pitch, origin = C.c_void_p(), C.c_long(), C.c_long()
    capi.check(capi.lib().suhmo_level_field_view(G.h, depth, lv.F_PHI, C.byref(base), C.byref(pitch), C.byref(origin)))
    nx, ny, P = G.nx >> depth, G.ny >> depth, pitch.value
    first = origin.value + (-r if side == 0 else ny) * P
    buf = np.empty(r * P)
    assert tr._hip.hipMemcpy(C.c_void_p(buf.ctypes.data), C.c_void_p(base.value + 8 * first), r * P * 8, 2) == 0     # device to host
    return buf.reshape(r, P)[:, :nx]


def _halo_invariant(case, G, rank, shared, tag, depths, log):
    """(c): every rank publishes its owned rows, all pass the barrier, every rank compares its halo rows with its neighbours' rows"""
    from suhmo_amd import capi, level as lv
    ex = G._exchanger
    halo = case[5]
    G.synchronize()
    for d in depths:
        shared[(tag, rank, d)] = G.get(lv.F_PHI, depth=d)
    ex.tr.barrier.wait()
    for d in depths:
        ny = G.ny >> d
        r = capi.lib().suhmo_level_phi_halo_fresh(G.h, d)
        assert 0 <= r <= min(halo, ny), "%s: %s: rank %d depth %d: phi_fresh = %d outside 0 .. min(%d, %d)" % (case[0], tag, rank, d, r, halo, ny)
        log[(tag, d)] = r
        for side, nb in ((0, ex.lo), (1, ex.hi)):
            if nb is None or r == 0:
                continue
            theirs = shared[(tag, nb, d)]
            want = theirs[ny - r:] if side == 0 else theirs[:r]
            got = _halo_rows(G, ex.tr, d, side, r)
            k = ss.first_difference(got, want)
            if k is not None:
                hr = r - k[0] if side == 0 else k[0] + 1
                raise AssertionError("%s: halo invariant after %s: rank %d, depth %d, field PHI, %s side (neighbour rank %d): %d halo rows counted current, "
                                     "halo row %d column %d holds %r, the neighbour's row %d holds %r"
                                     % (case[0], tag, rank, d, "lower" if side == 0 else "upper", nb, r, hr, k[1], got[k], ny - hr if side == 0 else hr - 1, want[k]))


def _counters(G):
    return {c: G.get_option(c) for c in ss.COUNTERS}


def _note(case, part, parts):
    """(d): what the case's ranks counted; the forbidden counters of the row and the branches nothing reaches are zero"""
    opt = case[8]
    row = SEEN.setdefault(opt, dict(pieces=set(), cycle=set()))
    row[part].add(case[0])
    for c in ss.COUNTERS:
        if any(p["counters"][c] for p in parts):
            row.setdefault(c, set()).add(case[0])
    for c in ss.OPTIONS[opt][2] + ss.NEVER:
        assert all(p["counters"][c] == 0 for p in parts), "%s: counter %s = %r on an option row that rules it out" % (case[0], c, [p["counters"][c] for p in parts])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pieces(case, oracle, monkeypatch):
    from suhmo_amd import level as lv
    cid, nx, nyt, world, mb, halo, bc, alpha, opt, sweeps, solver, seed = case
    for k, v in ss.environment(case).items():
        monkeypatch.setenv(k, v)
    f = ss.fields(case)
    ref, nd = ss.oracle_pieces(oracle, case, f)
    shared = {}

    def body(G, rank):
        out, log = dict(steps={}), {}
        ex = G._exchanger

        def step(name, **fields):
            out["steps"][name] = {k: G.get(fid) for k, fid in fields.items()}
            _halo_invariant(case, G, rank, shared, name, range(G.ndepth), log)

        for s in sweeps:
            G.gsrb(s)
        step("gsrb", PHI=lv.F_PHI)
        G.residual()
        step("residual", PHI=lv.F_PHI, RES=lv.F_RES)
        out["norm0"] = G.norm(lv.F_RES, 0)
        assert log[("residual", 0)] >= 1, "%s: the residual read the halo, yet no halo row counts as current" % cid
        G.apply_op()
        step("apply_op", PHI=lv.F_PHI, LPHI=lv.F_LPHI)
        G.update_operator()
        step("update_operator", PHI=lv.F_PHI, BX=lv.F_BX, BY=lv.F_BY)
        for s in sweeps:
            G.gsrb(s)
        step("gsrb again", PHI=lv.F_PHI)
        out["norm2"], out["dot"] = G.norm(lv.F_RES, 2), G.dot(lv.F_RES, lv.F_PHI)
        out["ndepth"], out["counters"], out["calls"], out["fresh"] = G.ndepth, _counters(G), ex.calls, log
        return out

    parts = run_strips(world, f, ss.BCS[bc], ss.PHYS, alpha, ss.BETA, body, halo=halo, max_box=mb)
    assert all(p["ndepth"] == nd for p in parts), (cid, [p["ndepth"] for p in parts], nd)
    for name, want in ref:
        for k, w in want.items():
            if k == "norm0":
                continue
            got = [p["steps"][name][k] for p in parts]
            g = np.vstack([a[:-1] for a in got] + [got[-1][-1:]]) if k == "BY" else np.vstack(got)      # the shared face row once
            _same(case, "pieces, after " + name, 0, k, g, w)
    n0 = dict(ref)["residual"]["norm0"]
    assert all(p["norm0"] == n0 for p in parts), "%s: max norm of RES: ranks %r, oracle %r" % (cid, [p["norm0"] for p in parts], n0)
    # norm(RES, 2) and dot(RES, PHI): any order of summation stays within (n - 1) 2^-53 sum |x_i y_i| of the exact sum; every rank holds the same bits
    res, phi = dict(ref)["residual"]["RES"], dict(ref)["gsrb again"]["PHI"]
    s2, b2 = ss.exact_dot(res, res)
    sd, bd = ss.exact_dot(res, phi)
    print("%s: norm2 %r exact %r bound %.3e | dot %r exact %r bound %.3e" % (cid, parts[0]["norm2"], np.sqrt(s2), ss.norm2_bound(s2, b2), parts[0]["dot"], sd, bd))
    assert len({p["norm2"] for p in parts}) == 1 and len({p["dot"] for p in parts}) == 1, cid
    assert abs(parts[0]["norm2"] - np.sqrt(s2)) <= ss.norm2_bound(s2, b2), (cid, parts[0]["norm2"], np.sqrt(s2), ss.norm2_bound(s2, b2))
    assert abs(parts[0]["dot"] - sd) <= bd, (cid, parts[0]["dot"], sd, bd)
    _note(case, "pieces", parts)
    EXCHANGES.setdefault(cid, {})["pieces"] = parts[0]["calls"]


def _cycle_body(case, shared):
    from suhmo_amd import capi, level as lv
    sp = ss.solver_params(case)

    def body(G, rank):
        out, log = {}, {}
        ex = G._exchanger
        G.build_mg_coefficients()
        da = capi.lib().suhmo_level_agglomerated_depth(G.h)
        own = range(da if da > 0 else G.ndepth)               # the depths this strip holds itself
        calls = [ex.calls]
        for key in ("v1", "v2"):
            G.vcycle(sp)
            G.synchronize()
            out[key] = {d: (G.get(lv.F_PHI, depth=d), G.get(lv.F_RES, depth=d)) for d in own}
            _halo_invariant(case, G, rank, shared, key, own, log)
            calls.append(ex.calls)
        out["n"], out["hist"] = G.solve(sp)
        calls.append(ex.calls)
        out["phi"], out["res"] = G.get(lv.F_PHI), G.get(lv.F_RES)
        out.update(ndepth=G.ndepth, da=da, counters=_counters(G), calls=calls, fresh=log)
        return out
    return body


def _compare_cycle(case, parts, cy):
    cid = case[0]
    assert all(p["ndepth"] == cy["ndepth"] for p in parts), (cid, [p["ndepth"] for p in parts], cy["ndepth"])
    assert len({p["da"] for p in parts}) == 1, cid
    for key in ("v1", "v2"):
        for d in parts[0][key]:
            _same(case, "cycle, after V-cycle " + key[1], d, "PHI", np.vstack([p[key][d][0] for p in parts]), cy[key][d][0])
            _same(case, "cycle, after V-cycle " + key[1], d, "RES", np.vstack([p[key][d][1] for p in parts]), cy[key][d][1])
    assert all(p["n"] == cy["n"] for p in parts), "%s: solve: iterations %r, oracle %d" % (cid, [p["n"] for p in parts], cy["n"])
    for p in parts:
        assert ss.first_difference(p["hist"][None, :], cy["hist"][None, :]) is None, "%s: residual history %r, oracle %r" % (cid, p["hist"], cy["hist"])
    _same(case, "cycle, after the solve", 0, "PHI", np.vstack([p["phi"] for p in parts]), cy["phi"])
    _same(case, "cycle, after the solve", 0, "RES", np.vstack([p["res"] for p in parts]), cy["res"])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cycle(case, oracle, monkeypatch):
    cid, nx, nyt, world, mb, halo, bc, alpha = case[:8]
    for k, v in ss.environment(case).items():
        monkeypatch.setenv(k, v)
    f = ss.fields(case)
    cy = ss.oracle_cycle(oracle, case, f)
    parts = run_strips(world, f, ss.BCS[bc], ss.PHYS, alpha, ss.BETA, _cycle_body(case, {}), halo=halo, max_box=mb)
    _compare_cycle(case, parts, cy)
    assert all(p["calls"] == parts[0]["calls"] for p in parts), (cid, [p["calls"] for p in parts])         # every rank exchanges as often as its neighbours
    _note(case, "cycle", parts)
    c = parts[0]["calls"]
    EXCHANGES.setdefault(cid, {}).update(v1=c[1] - c[0], v2=c[2] - c[1], solve=c[3] - c[2])
    print("%s: halo rows of PHI counted current after each V-cycle, by depth: %r" % (cid, sorted(parts[0]["fresh"].items())))


# (shape, ranks, option row): everything but the halo depth held fixed
LADDERS = (
    ((48, 16), 64, 2, "walls", 0.0, "default", (4, 16)),
    ((96, 32), 128, 2, "walls", 0.0, "stream-k2", (4, 16)),
    ((48, 16), 64, 3, "y-periodic", 0.5, "variant-0", (3, 16)),
    ((24, 24), 64, 4, "xy-periodic", 0.0, "tile-s2", (2, 1)),
)


@pytest.mark.parametrize("ladder", LADDERS, ids=["%dx%dx%d-%s" % (l[1], l[0][0], l[2], l[5]) for l in LADDERS])
def test_a_deeper_halo_never_needs_more_exchanges_per_vcycle(ladder, oracle, monkeypatch):
    """the exchanger calls of the second V-cycle, rank 0, by halo depth 1, 2, 3, 4, 5, 8, 9, 10, 11, 16, 24 (bitwise the oracle at every depth).
    Measured on an MI355X: 64x48x2 default 91 47 33 27 22 18 16 16 16 15 15; 128x96x2 stream-k2 110 57 44 33 28 22 19 19 19 18 16;
    64x48x3 variant-0 79 41 29 23 20 16 16 16 16 14 14; 64x24x4 tile-s2 26 14 10 9 8 7 7 6 6 6 6.  (While the tile launch capped its redundant
    rows at gy - need - 1 the default row needed 18 exchanges at halo 10, two more than at 9: DESIGN.md section 4.)"""
    (h, mb), nx, world, bc, alpha, opt, solver = ladder
    base = ("ladder-%dx%dx%d-%s" % (nx, h, world, opt), nx, h * world, world, mb, 0, bc, alpha, opt, (1,), solver, [nx, h, world, 977])
    for k, v in ss.environment(base).items():
        monkeypatch.setenv(k, v)
    f = ss.fields(base)
    cy = ss.oracle_cycle(oracle, base, f)                       # the halo depth does not change a bit
    per_cycle = []
    for halo in ss.HALO:
        case = (base[0] + "-halo%d" % halo,) + base[1:5] + (halo,) + base[6:]
        parts = run_strips(world, f, ss.BCS[bc], ss.PHYS, alpha, ss.BETA, _cycle_body(case, {}), halo=halo, max_box=mb)
        _compare_cycle(case, parts, cy)
        c = parts[0]["calls"]
        per_cycle.append(c[2] - c[1])
    print("%s: exchanges in the second V-cycle by halo depth %r: %r" % (base[0], ss.HALO, per_cycle))
    assert all(b <= a for a, b in zip(per_cycle, per_cycle[1:])), (base[0], ss.HALO, per_cycle)
    assert per_cycle[-1] < per_cycle[0], (base[0], per_cycle)


def test_every_option_row_ran_the_branches_it_exists_for():
    """(d), after the sweep above: per option row whose cases all ran, every counter the row exists for was non-zero in at least one case"""
    table = {}
    for c in CASES:
        table.setdefault(c[8], set()).add(c[0])
    print("\nexchanger calls per case (pieces, first V-cycle, second V-cycle, solve):")
    for cid, e in EXCHANGES.items():
        print("  %-84s %s" % (cid, " ".join("%s=%d" % kv for kv in e.items())))
    print("cases of a row in which a counter was non-zero on some rank:")
    missing, complete = [], 0
    for opt, (env, wanted, ruled_out) in ss.OPTIONS.items():
        row = SEEN.get(opt, dict(pieces=set(), cycle=set()))
        print("  %-30s %d cases: %s" % (opt, len(table[opt]), " ".join("%s=%d" % (c, len(row.get(c, ()))) for c in ss.COUNTERS if row.get(c))))
        if row["pieces"] != table[opt] or row["cycle"] != table[opt]:
            continue                                            # (a selection of the sweep ran: nothing to say about this row)
        complete += 1
        missing += [(opt, c) for c in wanted if not row.get(c)]
    assert not missing, missing
    print("%d of %d option rows ran completely" % (complete, len(ss.OPTIONS)))
