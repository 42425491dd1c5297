"""The time step on hierarchies whose levels are unions of boxes (suhmo_hier_timestep / suhmo_hier_moulin_source) against
oracle/amr_step_m.c on the same inputs: BITWISE on every box of base + 3 levels (an L-shaped union, a disjoint box, a box on
the domain side) over several steps, explicit and with moulins + diffusion + the implicit gap-height solve (cfg4 / cfg5
physics); one box per level equals the nested-patch step (suhmo_amr_timestep)."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import ghostring as gr

pytestmark = pytest.mark.gpu
ONE = ([(32, 16, 95, 47)], [(80, 44, 159, 83)])
ONE_PATCHES = ((16, 8, 47, 23), (40, 22, 79, 41))
CUT = ([(32, 16, 63, 47), (64, 16, 95, 31), (64, 32, 95, 47)], [(80, 44, 119, 83), (120, 44, 159, 83)])
UNION = ([(32, 16, 63, 47), (64, 16, 95, 31), (0, 4, 23, 27)],
         [(72, 40, 119, 55), (72, 56, 103, 87), (8, 16, 31, 39)],
         [(160, 88, 207, 103), (24, 40, 47, 63)])
# two boxes on opposite domain sides in y, one that spans the domain's height, a finer box on either side: with SHMIP-A's Neumann sides, and
# ("periodic-") with sy.CONV_BC, periodic in y -- then the first two are neighbours THROUGH the wrap and the third is its own neighbour
WRAP = ([(32, 0, 63, 15), (32, 48, 63, 63), (80, 0, 111, 63)], [(176, 0, 207, 23), (176, 104, 207, 127)])
MOULINS = dict(positions=[(30.0e3, 9.0e3), (42.0e3, 5.5e3), (8.0e3, 4.0e3)], sigma=[900.0, 700.0, 800.0], flux=[8.0, 5.0, 3.0])
B5ISH = dict(diffFactor=1.0, use_impl_diff=1, use_moulin_source=1, distributed_input=7.93e-11)

CASES = [("union-explicit", UNION, dict(), 3), ("union-diffusion", UNION, dict(diffFactor=1.0), 2),
         ("union-moulins-implicit", UNION, B5ISH, 3), ("cut-moulins-implicit", CUT, B5ISH, 2),
         ("wrap-explicit", WRAP, dict(), 2), ("wrap-moulins-implicit", WRAP, B5ISH, 2),
         ("periodic-wrap-explicit", WRAP, dict(), 2), ("periodic-wrap-moulins-implicit", WRAP, B5ISH, 2)]


def make(oracle, boxes, m, nx0=64, ny0=32, bc=sy.A3_BC):
    from suhmo_amd import model
    sts = sy.shmip_amrm_states(nx0, ny0, boxes, rough=0.5)
    O = oracle.OracleAmrMModel(nx0, ny0, sts[0][0]["dx"], sts[0][0]["dy"], bc, sy.A3_PHYS, m, boxes, max_box=16, nthreads=2)
    G = model.HipHierModel(nx0, ny0, sts[0][0]["dx"], sts[0][0]["dy"], bc, sy.A3_PHYS, m, boxes, max_box=16)
    O.set_states(sts); G.set_states(sts)
    return O, G, sts


@pytest.mark.parametrize("name,boxes,mpo,nsteps", CASES, ids=[c[0] for c in CASES])
def test_hier_timestep_bitwise(oracle, name, boxes, mpo, nsteps):
    from suhmo_amd import level as lv
    m = dict(sy.A3_MODEL, **mpo)
    bc = sy.CONV_BC if name.startswith("periodic-") else sy.A3_BC
    O, G, sts = make(oracle, boxes, m, bc=bc)
    if m.get("use_moulin_source"):
        io, ig = O.moulin_source(**MOULINS), G.moulin_source(**MOULINS)
        assert np.max(np.abs(io - ig)) <= 1e-13 * np.max(io)
        for l in range(O.nlev):
            for k in range(len(O.boxes[l])):
                a, b = np.array(O.field(l, k, oracle.OM_MSRC))[1:-1, 1:-1], G.get(l, k, "msrc")
                assert np.max(np.abs(a - b)) <= 1e-13 * max(np.max(np.abs(a)), 1e-300), (l, k)
                G.level[l][k].set(lv.F_MSRC, a)       # continue from identical source terms (two exp libraries)
    v = lambda a: np.array(a)[1:-1, 1:-1]
    for step in range(nsteps):
        dt = m["dt"] * (0.5 if step == 1 else 1.0)       # a changing step size: the implicit gap-height operators take the new beta = dt diffFactor (no rebuild)
        co, cg = O.timestep(dt), G.timestep(dt)
        assert co == cg, (step, co, cg)
        for l in range(O.nlev):
            for k in range(len(O.boxes[l])):
                for nm, fid in (("head", oracle.OM_H), ("B", oracle.OM_B), ("mR", oracle.OM_MR), ("Pw", oracle.OM_PW), ("rhs_h", oracle.OM_RHSH),
                                ("Re", oracle.OM_RE)):
                    a, b = v(O.field(l, k, fid)), G.get(l, k, nm)
                    assert np.array_equal(a, b, equal_nan=True), (name, step, l, k, nm, float(np.nanmax(np.abs(a - b))))
                for nm, fid in (("qwx", oracle.OM_QWX), ("qwy", oracle.OM_QWY)):
                    a, b = np.array(O.field(l, k, fid)), G.get(l, k, nm)
                    assert np.array_equal(a, b, equal_nan=True), (name, step, l, k, nm)
                # the head's ghost ring after the step, every side (domain, periodic, fine-fine, coarse-fine)
                gr.ring_equal(np.array(O.field(l, k, oracle.OM_H)), G.get(l, k, "head", ghosted=True), O.boxes[l][k], (64 << l, 32 << l),
                              bc["periodic"], O.boxes[l], what=(name, step, l, k, "head"))
                a, b = np.array(O.field(l, k, oracle.OM_B)), G.get(l, k, "B", ghosted=True)
                assert np.array_equal(a[1:-1, :], b[1:-1, :]) and np.array_equal(a[:, 1:-1], b[:, 1:-1]), (name, step, l, k, "B ghosts")
    O.close(); G.close()


def test_one_box_per_level_equals_the_nested_patch_step(oracle):
    from suhmo_amd import model
    m = dict(sy.A3_MODEL, diffFactor=1.0, use_impl_diff=1)
    sts = sy.shmip_amrm_states(64, 32, ONE, rough=0.5)
    H = model.HipHierModel(64, 32, sts[0][0]["dx"], sts[0][0]["dy"], sy.A3_BC, sy.A3_PHYS, m, ONE, max_box=16)
    A = model.HipAmrModel(64, 32, sts[0][0]["dx"], sts[0][0]["dy"], sy.A3_BC, sy.A3_PHYS, m, ONE_PATCHES, max_box=16)
    H.set_states(sts)
    for l in range(3):
        A.set_state(l, sts[l][0])
    for step in range(2):
        assert H.timestep(m["dt"]) == A.timestep(m["dt"])
        for l in range(3):
            for nm in ("head", "B", "mR", "qwx"):
                assert np.array_equal(H.get(l, 0, nm), A.get(l, nm)), (step, l, nm)
    H.close(); A.close()


@pytest.mark.parametrize("case", ["32", "64"])
def test_two_level_amr_run_against_the_reference_convergence_table(case):
    """exec/0_convergence_channelized/{1,2}lev_base (base 32 x 8 / 64 x 16 + one AMR level, 7200 steps of 1 h to the steady
    channel) on the device with the grids inferred from the reference's own table (tools/infer_amr_grids.py), compared as
    CONV_ANA/scripts/launch_comparaison_AMR1.py does with the single-level run two refinements finer: the composite L2 errors of
    gap height and Reynolds number land within 1.5 % of the reference's convergence_data_2Levels.dat -- a (loose) pin of the
    Chombo-side AMR pieces (QuadCFInterp, PiecewiseLinearFillPatch, reflux, the AMR FAS cycle) that the table's RHS_moulin column
    cannot give.  head / Pw: the reference's runs are converged to the Picard tolerance only (as in the single-level table,
    DESIGN.md section 4): ours are closer to the finer run, not compared."""
    import os, sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "..", "tools"))
    import convergence_channelized as cc
    ref = {int(float(r[0])): r[1:] for r in np.loadtxt(os.path.join(here, "golden", "convergence_channelized_2Levels_reference.dat"))}
    nx0 = int(case)
    rects = cc.amr_grids()["2Levels"][case]
    exact, _ = cc.run(int(np.log2(nx0 // 32)) + 3, "hip")
    e = cc.amr_errors(nx0, rects, exact)
    assert abs(e["B"] / ref[nx0][1] - 1.0) < 0.015, (e["B"], ref[nx0][1])
    assert abs(e["Re"] / ref[nx0][3] - 1.0) < 0.015, (e["Re"], ref[nx0][3])
    assert e["head"] < ref[nx0][0]


def test_postproc_table_of_a_hierarchy(oracle):
    """the SHMIP cross-section table of a run with AMR levels: the reference evaluates it on level 0 (src/AmrHydro.cpp:3643-3700, "POST PROC --
    1 LEVEL") -- the device table of the hierarchy's base handle equals the host twin evaluated on the oracle's level-0 fields after the
    same steps (sums in another order: 1e-12)"""
    m = dict(sy.A3_MODEL, **B5ISH)
    O, G, sts = make(oracle, UNION, m)
    O.moulin_source(**MOULINS); G.moulin_source(**MOULINS)
    from suhmo_amd import level as lv
    for l in range(O.nlev):
        for k in range(len(O.boxes[l])):
            G.level[l][k].set(lv.F_MSRC, np.array(O.field(l, k, oracle.OM_MSRC))[1:-1, 1:-1])
    for step in range(2):
        assert O.timestep(m["dt"]) == G.timestep(m["dt"])
    t = G.postproc_table_device()
    g = lambda fid: np.array(O.field(0, 0, fid))
    v = lambda a: a[1:-1, 1:-1]
    mask = v(g(oracle.OM_MASK))
    src = np.where(mask > 0.0, v(g(oracle.OM_MSRC)) * m.get("ramp", 1.0) + m["distributed_input"], 0.0)
    ref = sy.shmip_postproc_table(sts[0][0]["dx"], sts[0][0]["dy"], g(oracle.OM_QWX), g(oracle.OM_CD), src, v(g(oracle.OM_MR)), v(g(oracle.OM_PW)),
                                  v(g(oracle.OM_PI)), mask, m["rho_w"])
    ok = np.isfinite(ref)
    assert np.array_equal(ok, np.isfinite(t))
    scale = np.max(np.where(ok, np.abs(ref), 0.0), axis=0)
    assert np.all(np.where(ok, np.abs(t - ref), 0.0) <= 1e-12 * np.maximum(scale, 1e-300))
