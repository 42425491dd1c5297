"""The layouts of tests/hierlayouts.py on the CPU oracle (oracle/amrm.c) alone: every layout the device sweep (tests/test_gpu_hier_layouts.py) uses
is valid and accepted, the sweep contains what it claims, the oracle stays finite on all of them with both field sets, and cutting the same unions
into other boxes changes no bit wherever it must not."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import ghostring as gr
from tests import hierlayouts as hl

SEEDS = range(24)                                         # the seeds of tests/test_gpu_hier_layouts.py
NX0, NY0 = hl.NX0, hl.NY0
SP = dict(sy.SOLVER_DEFAULT, eps=1e-9, norm_thresh=1e-14, max_iter=3, imin=30)


def layouts():
    """(name, bc, boxes, seed for recut and fields) of every layout of the sweep"""
    out = [(name, bc, boxes, 100 + n) for n, (name, (bc, boxes)) in enumerate(hl.FEATURES.items())]
    return out + [("seed-%d" % s,) + hl.generate(s) + (s,) for s in SEEDS]


def make(oracle, bc, boxes, adversarial, seed):
    fs = hl.adversarial_fields(NX0, NY0, boxes, bc, seed) if adversarial else hl.analytic_fields(NX0, NY0, boxes, bc)
    O = oracle.OracleAmrM(NX0, NY0, fs[0]["dx"], fs[0]["dy"], bc, hl.ADV_PHYS if adversarial else sy.CFG3_PHYS, boxes, max_box=16, nthreads=1)
    O.set_inputs(fs)
    return O


def heads(O, oracle):
    return [O.coarse.get(oracle.F_PHI)] + [O.level_array(l, oracle.F_PHI) for l in range(1, O.nlev)]


def test_every_layout_is_valid_and_accepted(oracle):
    """no layout is filtered: FEATURES and generate(seed) for every seed pass valid() and or_amrm_create, and so do their re-cuttings; generate
    is deterministic"""
    for name, bc, boxes, seed in layouts():
        assert 1 <= len(boxes) <= 3 and all(len(bl) >= 1 for bl in boxes), name
        rc = hl.recut(seed, boxes, bc["periodic"])
        for what, bx in (("", boxes), ("recut", rc), ("any recut", hl.recut(seed, boxes))):
            assert hl.valid(NX0, NY0, bc["periodic"], bx), (name, what)
            oracle.OracleAmrM(NX0, NY0, 1.0, 1.0, bc, sy.CFG3_PHYS, bx, max_box=16).close()
        for l, (a, b) in enumerate(zip(boxes, rc), start=1):
            assert np.array_equal(hl.level_mask(NX0 << l, NY0 << l, a), hl.level_mask(NX0 << l, NY0 << l, b)), (name, l)
    for s in (0, 5, 23):
        assert hl.generate(s) == hl.generate(s)


def test_valid_refuses_what_the_oracle_and_the_device_refuse():
    """the refused layouts of test_oracle_amrm.py::test_bad_hierarchies_are_refused (64 x 16 base) and of
    test_gpu_hier.py::test_hier_refuses_layouts_the_reference_could_not_have (64 x 32 base), and the one the latter accepts"""
    for boxes in (([(16, 8, 31, 23), (30, 8, 47, 15)],), ([(15, 8, 30, 23)],), ([(16, 8, 47, 23)], [(32, 16, 63, 47)])):
        assert not hl.valid(64, 16, [0, 1], boxes), boxes
    for boxes in ([[(33, 16, 63, 47)]], [[(32, 16, 129, 47)]], [[(32, 16, 63, 47), (48, 32, 79, 63)]], [[(32, 16, 63, 47)], [(56, 24, 135, 71)]],
                  [[(32, 16, 63, 47)], [(64, 32, 95, 63)]]):
        assert not hl.valid(64, 32, [0, 0], boxes), boxes
    assert hl.valid(64, 32, [0, 0], [[(32, 16, 63, 47)], [(72, 40, 119, 87)]])
    # a box against x-lo: nested when x is not periodic (outside the domain), not nested when it is (the wrapped cells are not refined) ...
    alone = [[(0, 4, 15, 19)], [(0, 12, 19, 31)]]
    assert hl.valid(32, 16, [0, 0], alone) and not hl.valid(32, 16, [1, 0], alone)
    # ... unless a box across the wrap holds them
    assert hl.valid(32, 16, [1, 0], [alone[0] + [(48, 4, 63, 19)], alone[1]])


def test_the_random_sweep_contains_what_it_claims():
    per, nlev, two, kinds, x_periodic = set(), set(), 0, dict.fromkeys(gr.KINDS, 0), 0
    for s in SEEDS:
        bc, boxes = hl.generate(s)
        per.add(tuple(bc["periodic"])); nlev.add(1 + len(boxes))
        for l, bl in enumerate(boxes, start=1):
            for b in bl:
                two += (b[2] - b[0] + 1 == 2) or (b[3] - b[1] + 1 == 2)
                for side, k in gr.ring_kinds(b, (NX0 << l, NY0 << l), bc["periodic"], bl).items():
                    for kind in gr.KINDS:
                        kinds[kind] += int((k == kind).sum())
                    if side.startswith("x-"):
                        x_periodic += int((k == "periodic").sum())
    assert per == {(0, 0), (0, 1), (1, 0), (1, 1)} and nlev == {2, 3, 4}, (per, nlev)
    assert two > 0 and all(v > 0 for v in kinds.values()) and x_periodic > 0, (two, kinds, x_periodic)


def test_the_features_are_what_their_names_say():
    F = hl.FEATURES
    sizes = {(b[2] - b[0] + 1, b[3] - b[1] + 1) for bl in F["tiny-boxes"][1] for b in bl}
    assert (2, 2) in sizes and any(w == 2 and h > 2 for w, h in sizes) and any(h == 2 and w > 2 for w, h in sizes)
    kinds = lambda name, l, k: gr.ring_kinds(F[name][1][l - 1][k], (NX0 << l, NY0 << l), F[name][0]["periodic"], F[name][1][l - 1])
    k = kinds("domain-corner", 3, 0)
    assert (k["x-lo"] == "domain").all() and (k["y-lo"] == "domain").all()
    assert all((v == "coarse-fine").all() for l in (0, 1) for v in kinds("corner-touch", 1, l).values())
    assert set(kinds("t-junction", 1, 0)["y-hi"]) == {"fine-fine"}
    assert all((kinds("x-wrap-self", 1, 0)[s] == "periodic").all() for s in ("x-lo", "x-hi"))
    assert (kinds("x-wrap-self", 2, 0)["x-lo"] == "coarse-fine").all()          # across face 0 == face nxd: the level below
    assert (kinds("x-wrap-pair", 1, 0)["x-lo"] == "periodic").all() and (kinds("x-wrap-pair", 1, 0)["x-hi"] == "coarse-fine").all()
    assert (kinds("x-wrap-pair", 2, 1)["x-hi"] == "periodic").all()
    k = kinds("xy-wrap-corner", 1, 0)
    assert (k["x-lo"] == "periodic").all() and (k["y-lo"] == "periodic").all()
    assert all((kinds(n, 1, 0)[s] == "domain").all() for n, d in (("span-x", "x"), ("span-y", "y")) for s in (d + "-lo", d + "-hi"))
    # nesting distance exactly 2: one cell more in either direction and the layout is refused
    for name, l, k, grow in (("reentrant-nest-2", 2, 0, (0, 0, 2, 2)), ("reentrant-nest-2", 2, 0, (0, -2, 0, 0)), ("reentrant-nest-2", 2, 1, (0, 0, 0, 2)),
                             ("level3-in-width-6", 3, 0, (-2, 0, 0, 0)), ("level3-in-width-6", 3, 0, (0, 0, 2, 0)), ("corner-touch", 2, 0, (0, 0, 2, 0))):
        boxes = [list(bl) for bl in F[name][1]]
        boxes[l - 1][k] = tuple(a + b for a, b in zip(boxes[l - 1][k], grow))
        assert not hl.valid(NX0, NY0, F[name][0]["periodic"], boxes), (name, l, k, grow)
    # (towards the re-entrant corner the box may grow in x alone or in y alone: only the cell diagonal to the corner is missing)
    for grow in ((0, 0, 2, 0), (0, 0, 0, 2)):
        boxes = [list(bl) for bl in F["reentrant-nest-2"][1][:2]]
        boxes[1][0] = tuple(a + b for a, b in zip(boxes[1][0], grow))
        assert hl.valid(NX0, NY0, [0, 0], boxes), grow
    assert F["level3-in-width-6"][1][1][0][2] - F["level3-in-width-6"][1][1][0][0] + 1 == 6


@pytest.mark.parametrize("adversarial", [False, True], ids=["analytic", "adversarial"])
def test_the_oracle_stays_finite_on_every_layout(oracle, adversarial):
    """residual, the history of a 3-cycle solve and all heads, with both field sets -- the doubly periodic layouts (a singular problem: no
    Dirichlet side) included"""
    for name, bc, boxes, seed in layouts():
        O = make(oracle, bc, boxes, adversarial, seed)
        r = O.residual()
        n, hist = O.solve(SP)
        assert n == 3 and np.isfinite(r) and r > 0.0 and np.isfinite(hist).all(), (name, r, hist)
        for l, a in enumerate(heads(O, oracle)):
            assert np.isfinite(a[~np.isnan(a)]).all(), (name, l)
        O.close()


def test_recut_changes_no_bit_where_it_must_not(oracle):
    """Cutting the unions of a hierarchy into other boxes changes no bit of the composite residual, of the heads after one V-cycle and of a 3-cycle
    solve -- on exactly the layouts where hierlayouts.cut_signature() of the two cuttings is the same, that is where BOTH of the following agree.
    Doubly periodic layouts are NOT always among them: cause (1) cannot occur there, cause (2) can (of the six doubly periodic seeds, 3, 7 and 11
    get a recut with another signature, and the oracle's bits differ on them).  Both causes are the reference's own, restated by oracle/amrm.c:

    (1) unfilled_corners.  AMRProlongS_2 (src/AMRNonLinearPoissonOp.cpp:1143-1206) copies the coarse correction into a_temp, a LevelData on the
    COARSENED FINE boxes with one ghost layer (:1156), applies the boundary condition box by box (:1159-1167; mixBCValues fills
    adjCellBox(valid, dir, side, 1), the side cells along the box's own extent and no corner, src/AmrHydro.cpp:264-305), exchanges corners
    between the boxes' VALID cells (:1170-1172), and FORT_PROLONG_2_NL reads the diagonal cell coarse(ic + offs(1), jc + offs(2))
    (src/AMRNonLinearPoissonOpF.ChF:683-686).  So a corner ghost cell of a coarsened box that lies across a non-periodic domain side is written
    by nobody (oracle/amrm.c:681-688: calloc, wrap_cell fails, box_bc fills sides only), while the same cell is a SIDE cell, holding the boundary
    condition, of a box that extends past it.  A cut that ends on a non-periodic domain side therefore changes the prolongation of the two fine
    cells in the boxes' corners at that side; the composite residual before the first cycle is the same either way.

    (2) reflux_orders.  reflux (src/VCAMRNonLinearPoissonOp.cpp:555-652; src/AMRNonLinearPoissonOp.cpp:1281-1378) zeroes the flux register
    (:564), adds the coarse fluxes (incrementCoarse, :588) and, fine box by fine box, direction by direction, side by side (:612-645), the fine
    ones (incrementFine, :636), and m_levfluxreg.reflux(a_residual, scale) (:651) adds the register to the residual -- in Chombo's
    LevelFluxRegister one coarsened fine box, direction and side after the other, each a `residual += scale * register` on the coarse cells
    outside that side.  A coarse cell outside the sides of TWO fine boxes (a re-entrant corner of the union, a gap one coarse cell wide) thus
    gets (r + a) + b or (r + b) + a depending on the order of the boxes in the layout, and floating-point addition does not commute across
    three terms.  oracle/amrm.c:563-609 restates it: the loops over fine box (:569), direction (:572) and side (:577) and the accumulation
    into lofphi at :603; the device orders the faces of a coarse cell the same way (suhmo_hier_plan.hip, "reflux: faces grouped by the coarse
    cell they feed").  LevelFluxRegister itself belongs to the Chombo fork the reference does not vendor, so the per-box order inside its
    reflux() is restated from upstream Chombo 3.2, as the head of amrm.c says.

    Neither helper is checked against anything but this test: they mirror the oracle's loops, and what validates them is that the oracle's bits
    agree on every layout of the sweep whose signatures agree (and that they disagree on most of the others: test_oracle_amrm.py's ONE / CUT
    have neither a box on a domain side nor a coarse cell with two faces).  At least 20 of the 37 layouts get a recut that differs from them and keeps their signature,
    at least 2 for each periodicity; tests/test_gpu_hier_layouts.py compares the device with itself on the same ones."""
    checked = {}
    for name, bc, boxes, seed in layouts():
        rc = hl.recut(seed, boxes, bc["periodic"])
        if hl.cut_signature(NX0, NY0, bc["periodic"], boxes) != hl.cut_signature(NX0, NY0, bc["periodic"], rc):
            continue
        per = tuple(bc["periodic"])
        checked[per] = checked.get(per, 0) + (rc != boxes)
        for adversarial in (False, True):
            res = []
            for bx in (boxes, rc):
                O = make(oracle, bc, bx, adversarial, seed)
                r = O.residual()
                O.vcycle(SP)
                h1 = heads(O, oracle)
                n, hist = O.solve(SP)
                res.append((r, h1, hist, heads(O, oracle), [O.level_array(l, oracle.F_RES) for l in range(1, O.nlev)]))
                O.close()
            a, b = res
            assert a[0] == b[0] and np.array_equal(a[2], b[2]), (name, adversarial, a[0], b[0], a[2], b[2])
            for l, (x, y) in enumerate(zip(a[1] + a[3] + a[4], b[1] + b[3] + b[4])):
                assert np.array_equal(x, y, equal_nan=True), (name, adversarial, l)
    assert all(checked.get(p, 0) >= 2 for p in ((0, 0), (0, 1), (1, 0), (1, 1))) and sum(checked.values()) >= 20, checked


def test_a_periodic_level_has_one_face_on_the_wrap(oracle):
    """with the periodic images in the ghost cells (hierlayouts.analytic_fields) the oracle's face coefficients of level 0 at face 0 and at face
    nxd (and ny) are the same bits after V-cycles that update the operator -- the device keeps one of them, and a reflux across the wrap reads
    it.  The layout is the one where that mattered: coarse cells in column 0 with a coarse-fine face on either side, one through the wrap."""
    bc, boxes = hl.FEATURES["x-wrap-two-faces"]
    two = [c for c, faces in hl.reflux_orders(NX0, NY0, bc["periodic"], boxes).items() if c[:2] == (1, 0) and set(faces) == {(0, 0), (0, 1)}]
    assert two, "no coarse cell in column 0 with coarse-fine faces on both x sides"
    for name, bc, boxes, seed in layouts():
        if not (bc["periodic"][0] or bc["periodic"][1]):
            continue
        for adversarial in (False, True):
            O = make(oracle, bc, boxes, adversarial, seed)
            O.vcycle(SP); O.vcycle(SP)
            bx, by = O.coarse.get(oracle.F_BX), O.coarse.get(oracle.F_BY)
            if bc["periodic"][0]:
                assert np.array_equal(bx[:, 0], bx[:, -1]), (name, adversarial)
            if bc["periodic"][1]:
                assert np.array_equal(by[0, :], by[-1, :]), (name, adversarial)
            O.close()
