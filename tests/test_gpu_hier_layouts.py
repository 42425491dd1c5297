"""The box-union hierarchy (suhmo_hier*.hip, the box kernels of suhmo_gsrb.hip and suhmo_hier_fill.hip, the plans of suhmo_hier_plan.hip) against
oracle/amrm.c, BITWISE, over the layouts of tests/hierlayouts.py: thirteen built on purpose (boxes of 2 cells, corners, T-junctions, boxes that
are neighbours -- or their own neighbour -- through the x wrap, nesting at the minimum distance) and 24 generated ones over all four
periodicities, 2 to 4 levels and drawn boundary conditions; with the analytic fields of synthetic.amrm_fields and with fields whose B and mask
cross the operator's thresholds cell by cell.  32 x 16 base, so every case is a handful of tiny launches.  tests/test_hier_layouts_cpu.py holds
what the oracle alone can say about the same layouts."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import ghostring as gr
from tests import hierlayouts as hl
from tests.test_gpu_hier import eq, same_levels, same_rings

pytestmark = pytest.mark.gpu
NX0, NY0 = hl.NX0, hl.NY0
SEEDS = range(24)
OPTIONS = ("fused_relax=0", "box_sweeps=2", "merged_launches=0", "push_ghosts=0,fused_relax=0", "fused_prolong=0", "incremental_residual=0", None)
UNFUSED = "fused_relax=0,fused_prolong=0,merged_launches=0"


def feature_cases():
    return [(name, adversarial) for name in hl.FEATURES for adversarial in (False, True)]


def layout(case):
    """(bc, boxes, adversarial fields?, seed of the fields and the recut)"""
    if isinstance(case, tuple):
        name, adversarial = case
        bc, boxes = hl.FEATURES[name]
        return bc, boxes, adversarial, 100 + list(hl.FEATURES).index(name)
    bc, boxes = hl.generate(case)
    return bc, boxes, case % 3 != 2, case                 # every third seed: the analytic fields


def case_id(case):
    return "%s-%s" % (case[0], "adversarial" if case[1] else "analytic") if isinstance(case, tuple) else "seed-%d" % case


def fields(bc, boxes, adversarial, seed):
    if adversarial:
        return hl.adversarial_fields(NX0, NY0, boxes, bc, seed), hl.ADV_PHYS
    return hl.analytic_fields(NX0, NY0, boxes, bc), sy.CFG3_PHYS


def device(bc, boxes, fs, ph, options=None):
    from suhmo_amd import level
    G = level.HipHier(NX0, NY0, fs[0]["dx"], fs[0]["dy"], bc, ph, boxes, max_box=16, options=options)
    G.set_inputs(fs)
    return G


def pair(oracle, bc, boxes, adversarial, seed, options=None):
    fs, ph = fields(bc, boxes, adversarial, seed)
    O = oracle.OracleAmrM(NX0, NY0, fs[0]["dx"], fs[0]["dy"], bc, ph, boxes, max_box=16, nthreads=1)
    O.set_inputs(fs)
    return O, device(bc, boxes, fs, ph, options), fs


def solver(num_smooth=4):
    return dict(sy.SOLVER_DEFAULT, eps=1e-9, norm_thresh=1e-14, max_iter=3, imin=30, num_smooth=num_smooth)


@pytest.mark.parametrize("case", feature_cases() + list(SEEDS), ids=case_id)
def test_layout_pieces_bitwise(oracle, case):
    """per level: coarse-fine interpolation + exchange (the whole ghost ring, kind by kind), the operator update, the composite residual, the
    relaxation for 2, 1, 5 and 3 sweeps, the average into the level below"""
    from suhmo_amd.level import F_PHI, F_RES, F_BX, F_BY
    bc, boxes, adversarial, seed = layout(case)
    O, G, fs = pair(oracle, bc, boxes, adversarial, seed)
    levels = range(1, O.nlev)
    for l in levels:
        O.cf_interp_phi(l); O.exchange(l, oracle.F_PHI)
        G.cf_interp(l); G.exchange(l, F_PHI)
        for k, b in enumerate(boxes[l - 1]):
            gr.ring_equal(O.box_get(l, k, oracle.F_PHI, ghosted=True), G.level[l][k].get(F_PHI, ghosted=True), b, (NX0 << l, NY0 << l),
                          bc["periodic"], boxes[l - 1], what=("ghosts", l, k))
    for l in levels:
        O.update_operator(l); G.update_operator(l)
    same_levels(O, G, oracle, ((oracle.F_BX, F_BX), (oracle.F_BY, F_BY)), "update_operator")
    O.coarse.update_operator(); G.coarse.update_operator()
    ro, rg = O.residual(), G.residual()
    assert ro == rg, (ro, rg)
    same_levels(O, G, oracle, ((oracle.F_RES, F_RES),), "residual", skip_covered=True)
    for n in (2, 1, 5, 3):
        for l in levels:
            O.cf_interp_phi(l); G.cf_interp(l)
            O.gsrb(l, n); G.gsrb(l, n)
        same_levels(O, G, oracle, ((oracle.F_PHI, F_PHI),), "gsrb %d sweeps" % n)
    for l in reversed(levels):
        O.average_down(l, oracle.F_PHI); G.average(l, F_PHI, F_PHI)
        same_levels(O, G, oracle, ((oracle.F_PHI, F_PHI),), "average of level %d" % l)
    O.close(); G.close()


@pytest.mark.parametrize("case", feature_cases() + list(SEEDS), ids=case_id)
def test_layout_pwl_fill_of_B_bitwise(oracle, case):
    """suhmo_hier_pwl_fill of B, level by level, against the oracle's PiecewiseLinearFillPatch on box unions (oracle/amr_step_m.c:mm_pwl =
    or_pwl_fill per box from the level below): every coarse-fine ghost cell of every box, CORNERS INCLUDED (the fill writes them; ghostring
    leaves them out, so the cells are walked here), inside the domain.  Coarse-fine ghost cells ACROSS a periodic side are counted and not
    compared: or_pwl_fill leaves cells outside the domain box alone (oracle/amr_step_m.c:96), the device fills them from the wrapped coarse cell
    (suhmo_hier_plan.hip: wrap_cell before the classification) -- the oracle defines nothing there to compare with.  Nothing else of the ring
    may change on the device (fine-fine and domain cells keep the caller's data)."""
    from suhmo_amd.level import F_B
    bc, boxes, adversarial, seed = layout(case)
    fs, ph = fields(bc, boxes, adversarial, seed)
    M = oracle.OracleAmrMModel(NX0, NY0, fs[0]["dx"], fs[0]["dy"], bc, ph, sy.A3_MODEL, boxes, max_box=16)
    M.field(0, 0, oracle.OM_B)[:] = fs[0]["B"]
    for l in range(1, len(boxes) + 1):
        for k, f in enumerate(fs[l]):
            M.field(l, k, oracle.OM_B)[:] = f["B"]
    G = device(bc, boxes, fs, ph)
    compared = 0
    for l in range(1, len(boxes) + 1):
        M.pwl_fill(l, oracle.OM_B); G.pwl_fill(l, F_B, F_B)
        dom = (NX0 << l, NY0 << l)
        for k, b in enumerate(boxes[l - 1]):
            ref, dev, was = M.field(l, k, oracle.OM_B), G.level[l][k].get(F_B, ghosted=True), fs[l][k]["B"]
            eq(ref[1:-1, 1:-1], dev[1:-1, 1:-1], ("valid cells", l, k))
            for jj in range(ref.shape[0]):
                for ii in ((0, ref.shape[1] - 1) if 0 < jj < ref.shape[0] - 1 else range(ref.shape[1])):
                    i, j = b[0] - 1 + ii, b[1] - 1 + jj
                    if gr.cell_kind(i, j, dom, bc["periodic"], boxes[l - 1]) != "coarse-fine":
                        assert dev[jj, ii] == was[jj, ii], ("a ghost cell that is not coarse-fine changed", l, k, (i, j))
                    elif 0 <= i < dom[0] and 0 <= j < dom[1]:
                        compared += 1
                        assert ref[jj, ii] == dev[jj, ii], ("coarse-fine ghost", l, k, (i, j), float(dev[jj, ii]), float(ref[jj, ii]))
    assert compared > 0
    M.close(); G.close()


def cycle_cases():
    return [(c, o) for c in feature_cases() for o in (None, UNFUSED)] + [(s, "drawn") for s in SEEDS]


@pytest.mark.parametrize("case,options", cycle_cases(),
                         ids=lambda v: v if isinstance(v, str) else "defaults" if v is None else case_id(v))
def test_layout_vcycle_and_solve_bitwise(oracle, case, options):
    """one V-cycle and a 3-cycle solve: heads of every box and of level 0, F_BX, the history, RES on uncovered cells, the ghost rings.  FEATURES
    with the default options and with the unfused paths; a generated layout with an option string and a num_smooth drawn from its seed."""
    from suhmo_amd.level import F_PHI, F_RES, F_BX
    bc, boxes, adversarial, seed = layout(case)
    sp = solver()
    if options == "drawn":
        rng = np.random.default_rng([seed, 31])
        options = OPTIONS[int(rng.integers(0, len(OPTIONS)))]
        sp = solver(int(rng.choice([2, 3, 4, 6])))
    O, G, fs = pair(oracle, bc, boxes, adversarial, seed, options)
    what = (case_id(case), options, sp["num_smooth"])
    O.vcycle(sp); G.vcycle(sp)
    same_levels(O, G, oracle, ((oracle.F_PHI, F_PHI), (oracle.F_BX, F_BX)), what + ("vcycle",))
    same_rings(O, G, oracle, bc, fs, what + ("vcycle",), relaxed_last=True)
    no, ho = O.solve(sp)
    ng, hg = G.solve(sp)
    assert no == ng and np.array_equal(ho, hg), (what, ho, hg)
    same_levels(O, G, oracle, ((oracle.F_PHI, F_PHI),), what + ("solve",))
    same_levels(O, G, oracle, ((oracle.F_RES, F_RES),), what + ("solve residual",), skip_covered=True)
    same_rings(O, G, oracle, bc, fs, what + ("solve",), exchange=True)
    O.close(); G.close()


@pytest.mark.parametrize("case", [(name, True) for name in hl.FEATURES] + list(SEEDS), ids=case_id)
def test_layout_recut_on_the_device(oracle, case):
    """the same unions cut into other boxes (hierlayouts.recut).  Where the two cuttings have the same hierlayouts.cut_signature the device gives the
    same bits on both (residual, history, heads of all levels).  Where they have not, the reference itself depends on the cut (tests/test_hier_layouts_cpu.py::test_recut_changes_no_bit_where_it_must_not) and
    the device follows the oracle on the other cutting too.  How many layouts are compared device against device is asserted where no device is
    needed: tests/test_hier_layouts_cpu.py::test_recut_changes_no_bit_where_it_must_not (at least 20 of the 37, at least 2 per periodicity)."""
    from suhmo_amd.level import F_PHI
    bc, boxes, adversarial, seed = layout(case)
    rc = hl.recut(seed, boxes, bc["periodic"])
    sp = solver()
    fs, ph = fields(bc, rc, adversarial, seed)
    G = device(bc, rc, fs, ph)
    rg = G.residual()
    ng, hg = G.solve(sp)
    if hl.cut_signature(NX0, NY0, bc["periodic"], boxes) == hl.cut_signature(NX0, NY0, bc["periodic"], rc):
        fs0, _ = fields(bc, boxes, adversarial, seed)
        G0 = device(bc, boxes, fs0, ph)
        r0 = G0.residual()
        n0, h0 = G0.solve(sp)
        assert r0 == rg and n0 == ng and np.array_equal(h0, hg), (r0, rg, h0, hg)
        for l in range(1, G.nlev):
            assert np.array_equal(G0.level_array(l, F_PHI), G.level_array(l, F_PHI), equal_nan=True), l
        eq(G0.coarse.get(F_PHI), G.coarse.get(F_PHI), "base phi")
        G0.close()
    else:
        O = oracle.OracleAmrM(NX0, NY0, fs[0]["dx"], fs[0]["dy"], bc, ph, rc, max_box=16, nthreads=1)
        O.set_inputs(fs)
        ro = O.residual()
        no, ho = O.solve(sp)
        assert ro == rg and no == ng and np.array_equal(ho, hg), (ro, rg, ho, hg)
        same_levels(O, G, oracle, ((oracle.F_PHI, F_PHI),), "solve on the other cutting")
        O.close()
    G.close()


@pytest.mark.parametrize("mask", ["adversarial", "clean"])
def test_mask_written_through_a_box_handle_reaches_the_cycles(oracle, mask):
    """two V-cycles, a patch of level-1 mask cells flipped from +1 to -1 through the box handle, two more, the patch flipped back, two more: the
    heads, the face coefficients and the rings stay the oracle's at every step -- whatever a box level remembers about its mask must follow the
    write.  With the adversarial mask (some cells at -1 from the start) and with a mask that is +1 everywhere before and after the patch."""
    from suhmo_amd.level import F_PHI, F_BX, F_BY, F_MASK
    bc, boxes = hl.FEATURES["reentrant-nest-2"]
    fs = hl.adversarial_fields(NX0, NY0, boxes, bc, 7)
    if mask == "clean":
        for f in [fs[0]] + [f for lev in fs[1:] for f in lev]:
            f["mask"] = np.ones_like(f["mask"])
    O = oracle.OracleAmrM(NX0, NY0, fs[0]["dx"], fs[0]["dy"], bc, hl.ADV_PHYS, boxes, max_box=16, nthreads=1)
    O.set_inputs(fs)
    G = device(bc, boxes, fs, hl.ADV_PHYS)
    sp = solver()
    before = fs[1][0]["mask"]
    patched = before.copy()
    # 2 x 3 cells against the coarse-fine seam: the two rows (level-1 j = 14, 15) above the top side of the level-2 box (which covers level-1
    # i 20..29, j 10..13), columns i = 19..21 across its x-lo corner -- the reflux and the coarse-fine stencils of that side read them.  No larger:
    # a cell whose four neighbours are masked too has no face coefficient left, lambda = 0, and the relaxation divides by 1e-16 (the oracle's head
    # reaches 1e19 one cycle after such a patch and NaN three cycles later)
    patched[7:9, 4:7] = -1.0
    assert (before[7:9, 4:7] > 0.0).any()
    step = 0
    for m in (None, patched, before):
        if m is not None:
            O.box_set(1, 0, oracle.F_MASK, m, ghosted=True); G.level[1][0].set(F_MASK, m, ghosted=True)
        for _ in range(2):
            O.vcycle(sp); G.vcycle(sp)
            step += 1
            same_levels(O, G, oracle, ((oracle.F_PHI, F_PHI), (oracle.F_BX, F_BX), (oracle.F_BY, F_BY)), ("cycle", step))
            same_rings(O, G, oracle, bc, fs, ("cycle", step), relaxed_last=True)
    assert O.residual() == G.residual()
    O.close(); G.close()
