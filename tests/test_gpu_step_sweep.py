"""The time step on the device (suhmo_level_timestep, suhmo_hier_timestep: the per-cell kernels of suhmo_step.hip and the gradient, Re and bCoef kernels
they call) against the oracle (oracle/time_loop.c, oracle/amr_step_m.c) over the sweep of tests/stepsweep.py, BITWISE, no tolerance: 4 small shapes x
5 boundary conditions x 7 option rows on one level, with branch-edge values planted in the state, and the generated and hand-made box-union layouts
of tests/hierlayouts.py x 3 models with fields that cross the thresholds cell by cell.  tests/test_step_sweep_cpu.py holds what the oracle alone
can say about the same cases (nothing hides a failure, every arm of every branch is taken).  A failure names case, step, level, box, field, the
first differing cell and the arms of the census that cell took."""
import numpy as np
import pytest

from tests import ghostring as gr
from tests import hierlayouts as hl
from tests import stepsweep as sw

pytestmark = pytest.mark.gpu
FACES = (("qwx", "OM_QWX", sw.XFACE), ("qwy", "OM_QWY", sw.YFACE))
DIFFUSION = (("dcx", "OM_DCX", sw.XFACE), ("dcy", "OM_DCY", sw.YFACE), ("dterm", "OM_DTERM", sw.CELL))


@pytest.fixture(scope="module")
def hipmodel():
    from suhmo_amd import capi, model
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return model


def same(ref, dev, cen, kind, what):
    """dev == ref bit for bit (NaN == NaN); else the message names the first differing cell (or face) and the one that differs most, relative to the
    larger of the two values, each with the census arms it took.  One head solve spreads a wrong value over the level, so the first differing
    cell seldom is where it came from; the cell that differs most, in the most local field (compare_box goes from the faces to the head), is"""
    assert ref.shape == dev.shape, (what, ref.shape, dev.shape)
    bad = ~((ref == dev) | (np.isnan(ref) & np.isnan(dev)))
    if bad.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(bad, np.abs(ref - dev) / np.maximum(np.abs(ref), np.abs(dev)), 0.0)
        rel = np.where(np.isnan(rel), np.inf, rel)            # NaN on one side only
        cell = lambda j, i: "(i, j) = (%d, %d): device %r != oracle %r; arms taken there: %s" % (
            i, j, float(dev[j, i]), float(ref[j, i]), sw.arms_at(cen, kind, j, i) or "none")
        j0, i0 = (int(x) for x in np.argwhere(bad)[0])
        j1, i1 = (int(x) for x in np.unravel_index(np.argmax(rel), rel.shape))
        raise AssertionError("%s: %d of %d %ss differ.  Largest relative difference (%.3g) at %s.  First differing %s %s"
                             % (what, int(bad.sum()), bad.size, kind, float(rel[j1, i1]), cell(j1, i1), kind, cell(j0, i0)))


def same_edge_ghosts(ref, dev, cen, what):
    """the ghost ring of the gap height without its corners (CopyGhostCells / the fills between levels; corners are never read)"""
    for name, d, s in gr.SIDES:
        a, b = gr.side_of(ref, d, s), gr.side_of(dev, d, s)
        bad = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))
        if bad.size:
            n = int(bad[0])
            j, i = (n, 0 if s == 0 else ref.shape[1] - 3) if d == 0 else (0 if s == 0 else ref.shape[0] - 3, n)
            raise AssertionError("%s: ghost cells of B differ on side %s, first at position %d: device %r != oracle %r; arms of the cell next to it: %s"
                                 % (what, name, n, float(b[n]), float(a[n]), sw.arms_at(cen, sw.CELL, j, i)))


def compare_box(oracle, ofield, dget, cen, diffusion, what, with_cd):
    """from the most local fields to the most global: the lagged diffusion coefficients, the fluxes on the faces, then the cell fields, the head last"""
    v = lambda a: np.array(a)[1:-1, 1:-1]
    for nm, fid, kind in (DIFFUSION if diffusion else ()) + FACES:
        same(np.array(ofield(getattr(oracle, fid))), dget(nm), cen, kind, what + (nm,))
    fids = dict(sw.compared_fields(oracle))
    for nm in ("mR", "rhs_h", "cd", "Re", "Pw", "B", "head"):
        if nm == "cd" and not with_cd:
            continue
        same(v(ofield(fids[nm])), dget(nm), cen, sw.CELL, what + (nm,))


@pytest.mark.parametrize("case", sw.single_cases(), ids=lambda c: c[0])
def test_single_level_step_bitwise(oracle, hipmodel, case):
    """two steps (the second at half the step size): iteration counts, head, B, mR, Pw, cd, rhs_h, Re on valid cells, qwx / qwy with the faces on the
    high sides, with diffusion DCX, DCY and DTERM, the head's ring, the edge ghosts of B"""
    from suhmo_amd import level as lv
    cid, nx, ny, b, r = case
    dev = {}

    def on_start(O, st, bc, m, src):
        G = dev["G"] = hipmodel.HipModel(nx, ny, st["dx"], st["dy"], bc, sw.PHYS, m, max_box=16)
        G.set_state(st)
        if src is not None:
            G.level.set(lv.F_MSRC, src)                   # the oracle's array on both sides: the two exp libraries do not enter

    def on_step(k, dt, O, cen, iters):
        G, bc, m = dev["G"], sw.BCS[b], sw.model_of(r)
        got = G.timestep(dt)
        what = (cid, "step %d" % k)
        compare_box(oracle, O.field, G.get, cen, m["diffFactor"] != 0.0, what, True)
        assert got == iters, (cid, "step", k, "(picard, vcycles): device", got, "oracle", iters)      # after the fields: their message says more
        gr.level_ring_equal(np.array(O.field(oracle.OM_H)), G.get("head", ghosted=True), (nx, ny), bc["periodic"], what=what + ("head",))
        same_edge_ghosts(np.array(O.field(oracle.OM_B)), G.get("B", ghosted=True), cen, what + ("B",))

    try:
        rec = sw.run_single(oracle, case, on_start, on_step)
    finally:
        if "G" in dev:
            dev["G"].close()
    assert not rec["problems"] and len(rec["iters"]) == sw.N_STEPS, rec["problems"]


UNION_FIELDS = ("head", "B", "mR", "Pw", "rhs_h", "Re")


def hier_cases():
    return [(layout, mn) for layout in sw.device_layouts() for mn in sw.HIER_MODELS]


def device_hier(hipmodel, sts, bc, m, boxes):
    G = hipmodel.HipHierModel(hl.NX0, hl.NY0, sts[0][0]["dx"], sts[0][0]["dy"], bc, hl.ADV_PHYS, m, boxes, max_box=16)
    G.set_states(sts)
    return G


@pytest.mark.parametrize("layout,model_name", hier_cases(), ids=lambda v: v if isinstance(v, str) else v[0])
def test_hierarchy_step_bitwise(oracle, hipmodel, layout, model_name):
    """two steps of a box-union hierarchy: the comparisons of tests/test_gpu_hier_timestep.py::test_hier_timestep_bitwise on every box of every level,
    the head's ring over all four kinds of ghost cell.  Where another cutting of the same unions has the same hierlayouts.cut_signature, the device
    on that cutting gives the same bits as the device on this one (level by level over the unions)."""
    name, bc, boxes, seed = layout
    dev, unions = {}, []

    def on_start(O, sts, bc_, m):
        dev["G"] = device_hier(hipmodel, sts, bc, m, boxes)

    def on_step(k, dt, O, cens, iters):
        G, m = dev["G"], sw.hier_model_of(model_name)
        got = G.timestep(dt)
        for l in range(O.nlev):
            for q, box in enumerate(O.boxes[l]):
                what = (name, model_name, "step %d" % k, "level %d" % l, "box %d %s" % (q, box))
                ofield = lambda fid: O.field(l, q, fid)
                dget = lambda nm, ghosted=False: G.get(l, q, nm, ghosted=ghosted)
                compare_box(oracle, ofield, dget, cens[(l, q)], False, what, False)
                gr.ring_equal(np.array(ofield(oracle.OM_H)), dget("head", ghosted=True), box, (hl.NX0 << l, hl.NY0 << l), bc["periodic"], O.boxes[l],
                              what=what + ("head",))
                same_edge_ghosts(np.array(ofield(oracle.OM_B)), dget("B", ghosted=True), cens[(l, q)], what + ("B",))
        assert got == iters, (name, model_name, "step", k, "(picard, vcycles): device", got, "oracle", iters)
        unions.append({nm: [union_array(G, l, boxes, nm) for l in range(O.nlev)] for nm in UNION_FIELDS})

    try:
        rec = sw.run_hier(oracle, layout, model_name, on_start, on_step)
        assert not rec["problems"] and len(rec["iters"]) == sw.N_STEPS, rec["problems"]
        rc = hl.recut(seed, boxes, bc["periodic"])
        sig = lambda bx: hl.cut_signature(hl.NX0, hl.NY0, bc["periodic"], bx)
        if rc != boxes and sig(rc) == sig(boxes):
            m = sw.hier_model_of(model_name)
            R = dev["R"] = device_hier(hipmodel, sw.hier_states(bc, rc, seed), bc, m, rc)
            for k in range(sw.N_STEPS):
                got = R.timestep(m["dt"] * (0.5 if k == 1 else 1.0))
                assert got == rec["iters"][k], (name, model_name, "recut", k, got, rec["iters"][k])
                for nm in UNION_FIELDS:
                    for l in range(len(boxes) + 1):
                        same(unions[k][nm][l], union_array(R, l, rc, nm), {}, sw.CELL,
                             (name, model_name, "the device on another cutting (as device) against the device on this one (as oracle)", "step %d" % k, "level %d" % l, nm))
    finally:
        for G in dev.values():
            G.close()


def union_array(G, l, boxes, nm):
    """valid cells of field nm of level l over the level's domain, NaN where the level has no box"""
    if l == 0:
        return G.get(0, 0, nm)
    out = np.full((hl.NY0 << l, hl.NX0 << l), np.nan)
    for q, (lo0, lo1, hi0, hi1) in enumerate(boxes[l - 1]):
        out[lo1:hi1 + 1, lo0:hi0 + 1] = G.get(l, q, nm)
    return out
