"""The ensemble path on the device (suhmo_batch_vcycle, suhmo_batch_solve, suhmo_batch_timestep: every kernel launched over OnMembers) against the
CPU oracle's run of every member ALONE over the sweep of tests/batchsweep.py, BITWISE, no tolerance: 16 shapes x 8 solver rows with rotating
boundary conditions and five members with dirty, clean, one-cell and +-1 masks; the time-step batches of the step sweep's states; two batches of
64 members.  tests/test_batch_sweep_cpu.py holds what the oracle alone can say about the same batches.  Launch counts: batch_launches is asserted
against the census's restatement of batch_vcycle / batch_solve for EVERY row, after every call.  A failure names batch (shape, BC, solver row),
member, palette, depth, field and the first differing cell."""
import ctypes as C

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import batchsweep as bw
from tests import ghostring as gr
from tests import stepsweep as sw
from tests.test_gpu_step_sweep import DIFFUSION, FACES, compare_box, same_edge_ghosts

pytestmark = pytest.mark.gpu

COEFS = ("F_ACOEF", "F_B", "F_PI", "F_ZB", "F_MASK")       # build_mg_coefficients' averages on every coarse depth


@pytest.fixture(scope="module")
def hip():
    from suhmo_amd import capi, level
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return level


@pytest.fixture(scope="module")
def hipmodel():
    from suhmo_amd import capi, model
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return model


def equal(ref, dev, what, field, depth=0):
    """dev == ref bit for bit (NaN == NaN), else the message names what, depth, field and the first differing cell"""
    assert ref.shape == dev.shape, (what, field, depth, ref.shape, dev.shape)
    bad = ~((ref == dev) | (np.isnan(ref) & np.isnan(dev)))
    if bad.any():
        j, i = (int(x) for x in np.argwhere(bad)[0])
        raise AssertionError("%s, depth %d, %s: %d of %d values differ, first at (i, j) = (%d, %d): device %r != oracle %r"
                             % (what, depth, field, int(bad.sum()), bad.size, i, j, float(dev[j, i]), float(ref[j, i])))


def same_member(oracle, hip, O, G, f, bc, what, nd, relaxed_last, ring=True):
    """member handle G against its oracle level O: head and ring, PHI / RHS / RES of every coarse depth of the cycle, the faces of every depth, the
    averaged coefficients, then the residual.  ring = False: the cycle's last operation on depth 0 is the prolongation (num_smooth = 0 above a
    coarser depth) -- the oracle's ring is then what the residual evaluation of its restriction left, the boundary condition of a head that no longer
    exists, and the device, whose restriction needs no stored ring, leaves what was there: neither is the ring of the head, no one reads either
    (the next cycle and a solve's residual fill it first), and the solve that follows is compared ring and all"""
    nx, ny = f["nx"], f["ny"]
    equal(O.get(oracle.F_PHI), G.get(hip.F_PHI), what, "head")
    gg = G.get(hip.F_PHI, ghosted=True)
    if ring:
        gr.level_ring_equal(O.get(oracle.F_PHI, ghosted=True), gg, (nx, ny), bc["periodic"], what=what + ", head")
    if relaxed_last:
        gr.domain_bc_holds(gg, bc, f["dx"], f["dy"], (0, 0, nx - 1, ny - 1), (nx, ny), what + ", head")
    for d in range(1, nd):
        for nm in ("F_PHI", "F_RHS", "F_RES"):
            equal(O.get(getattr(oracle, nm), depth=d), G.get(getattr(hip, nm), depth=d), what, nm, d)
    for d in range(nd):
        for nm in ("F_BX", "F_BY"):
            equal(O.get(getattr(oracle, nm), depth=d), G.get(getattr(hip, nm), depth=d), what, nm, d)
    for d in range(1, G.ndepth):
        for nm in COEFS:
            equal(O.get(getattr(oracle, nm), depth=d), G.get(getattr(hip, nm), depth=d), what, nm, d)
    O.residual(); G.residual()
    equal(O.get(oracle.F_RES), G.get(hip.F_RES), what, "residual")


def make_batch(hip, n, shape, b, row):
    nx, ny, mb = shape
    f0 = bw.member(shape, b, 0)[0]
    B = hip.HipBatch(n, nx, ny, f0["dx"], f0["dy"], bw.BCS[b], sy.A3_PHYS, alpha=row[4], max_box=mb, bottom_solver=bool(row[3]))
    B.set_option("tile_order", row[5])
    return B


def load_member(B, k, f, bc, ph):
    B.set_bc(k, bc); B.set_phys(k, ph)
    B.member(k).set_inputs(f); B.member(k).build_mg_coefficients()


def ring_written(cen, row):
    """the cycle's last operation on depth 0 writes the head's ring: a relaxation, or RelaxSolver's closing residual on a one-depth level"""
    return relaxed_last(cen, row) or (cen["nd"] == 1 and bool(row[3]))


def relaxed_last(cen, row):
    """the cycle ends on a relaxation of depth 0 (whose closing fill leaves the homogeneous boundary condition in the ring)"""
    return (row[0] > 0) if cen["nd"] > 1 else (row[1] > 0 and not row[3])


@pytest.mark.parametrize("batch", bw.batches(), ids=lambda b: b[0])
def test_cycles_with_active_lists_then_a_solve(oracle, hip, batch):
    bid, shape, b, row = batch
    nx, ny, mb = shape
    lists, _ = bw.protocol(row)
    sp, ssp = bw.cycle_params(row), bw.solve_params(row)
    B, Os = make_batch(hip, bw.N_MEMBERS, shape, b, row), []
    ins = [bw.member(shape, b, k) for k in range(bw.N_MEMBERS)]
    name = lambda k: "batch %s (solver row %s), member %d (%s)" % (bid, bw.row_name(row), k, ins[k][3])
    with bw.oracle_bottom(row[3]):
        try:
            for k, (f, bc, ph, pal) in enumerate(ins):
                load_member(B, k, f, bc, ph)
                Os.append(bw.oracle_level(oracle, shape, f, bc, ph, row))
            depths = [Os[0].shape(oracle.F_PHI, d)[::-1] for d in range(Os[0].ndepth)]
            assert B.ndepth == len(depths)
            cen = bw.cycle_census(depths, bw.BCS[b]["periodic"], row)
            total, late = 0, []                       # launch counts that differ: asserted after the fields, whose messages say more
            for c, active in enumerate(lists):
                before = {k: (B.member(k).get(hip.F_PHI, ghosted=True), B.member(k).get(hip.F_RES)) for k in range(bw.N_MEMBERS) if not active[k]}
                n0 = B.get_option("batch_launches")
                B.vcycle(sp, active=active)
                got = B.get_option("batch_launches") - n0
                if got != cen["launches"]:
                    late.append(("launches of cycle %d" % (c + 1), "device", got, "census", cen["launches"], cen["relax"]))
                for k in range(bw.N_MEMBERS):
                    if active[k]:
                        Os[k].vcycle(sp)
                    else:
                        equal(before[k][0], B.member(k).get(hip.F_PHI, ghosted=True), name(k) + ", not flagged in cycle %d (before as oracle)" % (c + 1), "ghosted head")
                        equal(before[k][1], B.member(k).get(hip.F_RES), name(k) + ", not flagged in cycle %d (before as oracle)" % (c + 1), "F_RES")
                total += sum(active)
            assert B.get_option("batch_member_cycles") == total and B.get_option("batch_readbacks") == 0
            for k, (f, bc, ph, pal) in enumerate(ins):
                same_member(oracle, hip, Os[k], B.member(k), f, bc, name(k) + " after %d cycles" % bw.cycles_of_member(row, k), cen["nd"], relaxed_last(cen, row), ring_written(cen, row))
            # the solve; on the tall shapes every member's residual maximum enters it in a partial of its own
            for k, (f, bc, ph, pal) in enumerate(ins):
                rhs = bw.spiked_rhs(shape, f, k)
                if rhs is not None:
                    B.member(k).set(hip.F_RHS, rhs); Os[k].set(oracle.F_RHS, rhs)
            n0 = B.get_option("batch_launches")
            iters, res = B.solve(ssp)
            want = [O.solve(ssp) for O in Os]
            counts = [w[0] for w in want]
            print(bid, "cycles per member: oracle", counts, "batch", iters, "final norms", [float(w[1][-1]) for w in want], list(res))
            for k, (f, bc, ph, pal) in enumerate(ins):
                what = name(k) + " after the solve"
                equal(Os[k].get(oracle.F_PHI), B.member(k).get(hip.F_PHI), what, "head")
                equal(Os[k].get(oracle.F_RES), B.member(k).get(hip.F_RES), what, "F_RES")
                assert iters[k] == counts[k] and res[k] == want[k][1][-1], (what, "cycles: device", iters[k], "oracle", counts[k], "final norm: device", res[k], "oracle", want[k][1][-1])
                gr.level_ring_equal(Os[k].get(oracle.F_PHI, ghosted=True), B.member(k).get(hip.F_PHI, ghosted=True), (nx, ny), bc["periodic"], what=what + ", head")
            if B.get_option("batch_launches") - n0 != bw.solve_launches(cen, counts):
                late.append(("launches of the solve", "device", B.get_option("batch_launches") - n0, "census", bw.solve_launches(cen, counts)))
            assert not late, (bid, "the fields are the oracle's; the launches are not the census's", late)
            assert B.get_option("batch_member_cycles") == total + sum(counts) and B.get_option("batch_readbacks") == 1 + max(counts)
        finally:
            for O in Os:
                O.close()
            B.close()


@pytest.mark.parametrize("case", bw.BIG, ids=lambda c: c[0])
def test_sixty_four_members(oracle, hip, case):
    """SUHMO_BATCH_MAX members: the active lists {63}, {0, 63}, the odd members and all; members 0, 1, 31, 32, 62, 63 against the oracle after every
    call that flags them, every member that is not flagged bitwise unchanged; then a solve of all 64 (gridDim.z = 64 in every launch, 16 rounds of
    the norm's second stage)"""
    bid, shape, b = case
    row, n = bw.BIG_ROW, bw.BATCH_MAX
    nx, ny, mb = shape
    sp, ssp = bw.cycle_params(row), dict(bw.solve_params(row), max_iter=2)
    B, Os = make_batch(hip, n, shape, b, row), {}
    ins = [bw.member(shape, b, k) for k in range(n)]
    name = lambda k: "batch %s (solver row %s), member %d (%s)" % (bid, bw.row_name(row), k, ins[k][3])
    try:
        for k, (f, bc, ph, pal) in enumerate(ins):
            load_member(B, k, f, bc, ph)
            if k in bw.BIG_ORACLE:
                Os[k] = bw.oracle_level(oracle, shape, f, bc, ph, row)
        O0 = Os[0]
        cen = bw.cycle_census([O0.shape(oracle.F_PHI, d)[::-1] for d in range(O0.ndepth)], bw.BCS[b]["periodic"], row)
        total = 0
        for c, active in enumerate(bw.big_active_lists()):
            before = [B.member(k).get(hip.F_PHI, ghosted=True) for k in range(n)]
            n0 = B.get_option("batch_launches")
            B.vcycle(sp, active=active)
            assert B.get_option("batch_launches") - n0 == cen["launches"], (bid, c)
            for k in range(n):
                if not active[k]:
                    equal(before[k], B.member(k).get(hip.F_PHI, ghosted=True), name(k) + ", not flagged in call %d (before as oracle)" % (c + 1), "ghosted head")
                elif k in Os:
                    Os[k].vcycle(sp)
                    f, bc, ph, pal = ins[k]
                    same_member(oracle, hip, Os[k], B.member(k), f, bc, name(k) + " after call %d" % (c + 1), cen["nd"], relaxed_last(cen, row))
                else:
                    assert not np.array_equal(before[k], B.member(k).get(hip.F_PHI, ghosted=True)), (name(k), "flagged in call", c + 1, "and unchanged")
            total += sum(active)
        assert B.get_option("batch_member_cycles") == total == 1 + 2 + 32 + 64
        iters, res = B.solve(ssp)
        for k, O in Os.items():
            it, hist = O.solve(ssp)
            assert iters[k] == it and res[k] == hist[-1], (name(k), "solve", iters[k], it, res[k], hist[-1])
            equal(O.get(oracle.F_PHI), B.member(k).get(hip.F_PHI), name(k) + " after the solve", "head")
            equal(O.get(oracle.F_RES), B.member(k).get(hip.F_RES), name(k) + " after the solve", "F_RES")
    finally:
        for O in Os.values():
            O.close()
        B.close()


def test_sixty_five_members_are_refused(hip):
    from suhmo_amd import capi
    lib = capi.lib()
    d = capi.LevelDesc()
    d.nx, d.ny, d.j0, d.ny_global, d.dx, d.dy = 12, 4, 0, 4, 3.0, 2.0
    d.nbox, d.boxes, d.max_box, d.alpha, d.beta = 0, None, 16, 0.0, -1.0
    d.bc, d.phys, d.device, d.halo_rows = hip._bc(bw.BCS["a3"]), hip._phys(sy.A3_PHYS), 0, 1
    h = C.c_void_p()
    assert lib.suhmo_batch_create(C.byref(h), C.byref(d), bw.BATCH_MAX + 1) == -1
    msg = lib.suhmo_last_error()
    assert b"n_members = 65" in msg and b"1 .. 64" in msg, msg


@pytest.mark.parametrize("batch", bw.step_batches(), ids=lambda b: b[0])
def test_time_step_batches_bitwise(oracle, hipmodel, batch):
    """two steps (the second at half the size) of a batch whose members are the option rows of the step sweep on their planted states, implicit gap
    solves among them: per member and step (picard, vcycles), the diffusion coefficients, fluxes, cell fields and head, the head's ring and the edge
    ghosts of B against stepsweep.run_single of that member alone"""
    from suhmo_amd import level as lv
    bid, nx, ny, b, dt0, rows = batch
    bc = sw.BCS[b]
    starts, stored = {}, {}
    for k, r in enumerate(rows):
        def on_start(O, st, bc_, m, src, k=k):
            starts[k] = (st, m, src)

        def on_step(step, dt, O, cen, iters, k=k):
            m = starts[k][1]
            fids = [fid for _, fid in sw.compared_fields(oracle)] + [getattr(oracle, fid) for _, fid, _ in FACES]
            if m["diffFactor"] != 0.0:
                fids += [getattr(oracle, fid) for _, fid, _ in DIFFUSION]
            stored[(k, step)] = dict(dt=dt, cen=cen, iters=iters, f={fid: np.array(O.field(fid)) for fid in fids})

        rec = sw.run_single(oracle, bw.step_case(batch, r), on_start, on_step, dt=dt0)
        assert not rec["problems"] and len(rec["iters"]) == sw.N_STEPS, rec["problems"]
    st0 = starts[0][0]
    G = hipmodel.HipBatchModel(nx, ny, st0["dx"], st0["dy"], bc, sw.PHYS, [starts[k][1] for k in range(len(rows))], max_box=16, implicit_gap=True)
    try:
        for k in range(len(rows)):
            st, m, src = starts[k]
            G.set_state(k, st)
            if src is not None:
                G.member(k).level.set(lv.F_MSRC, src)         # the oracle's array on both sides: the two exp libraries do not enter
        for step in range(sw.N_STEPS):
            dt = stored[(0, step)]["dt"]
            assert all(stored[(k, step)]["dt"] == dt for k in range(len(rows)))
            pi, nv = G.timestep(dt)
            for k, r in enumerate(rows):
                s = stored[(k, step)]
                what = (bid, "member %d (%s)" % (k, r), "step %d" % step)
                compare_box(oracle, lambda fid: s["f"][fid], lambda nm: G.get(k, nm), s["cen"], starts[k][1]["diffFactor"] != 0.0, what, True)
                assert (pi[k], nv[k]) == s["iters"], (what, "(picard, vcycles): device", (pi[k], nv[k]), "oracle", s["iters"])
                gr.level_ring_equal(s["f"][oracle.OM_H], G.get(k, "head", ghosted=True), (nx, ny), bc["periodic"], what=what + ("head",))
                same_edge_ghosts(s["f"][oracle.OM_B], G.get(k, "B", ghosted=True), s["cen"], what + ("B",))
    finally:
        G.close()
