"""Moulin source term on the GPU (suhmo_level_moulin_source; Calc_moulin_integral +
Calc_moulin_source_term_distributed, src/AmrHydro.cpp:1866-2066) against the oracle.  exp() comes from two
different math libraries, so the bar here is a stated tolerance: 1e-13 relative to the largest value (the
integrals additionally differ in summation order), not bit equality.  The time step that consumes the term is
compared bit for bit by feeding both sides the same source array."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy

pytestmark = pytest.mark.gpu
RTOL = 1e-13


def moulins(n, seed, lx=1.0e5, ly=2.0e4):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(0.05 * lx, 0.95 * lx, n), rng.uniform(0.05 * ly, 0.95 * ly, n)], axis=1)
    return pos, np.full(n, 200.0), np.full(n, 90.0 / n)          # exec/B_SHMIP/B<k>/input.hydro:37-40


@pytest.mark.parametrize("nx,ny,n", [(320, 64, 1), (320, 64, 100), (1280, 256, 10)])
def test_moulin_source_matches_oracle(oracle, nx, ny, n):
    from suhmo_amd import model
    st = sy.shmip_initial_state(nx, ny)
    pos, sg, fl = moulins(n, 5) if n > 1 else (np.array([[59000.0, 8000.0]]), np.array([200.0]), np.array([90.0]))
    G = model.HipModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, sy.A3_MODEL)
    integ_g = G.moulin_source(pos, sg, fl, 0.75)
    src_g = G.get("msrc")
    src_o, integ_o = oracle.moulin_source(nx, ny, st["dx"], st["dy"], pos, sg, fl, 0.75)
    assert np.max(np.abs(integ_g - integ_o)) <= RTOL * np.max(integ_o)
    assert np.max(np.abs(src_g - src_o)) <= RTOL * np.max(src_o)
    # each moulin delivers its flux (times the time factor): sum(src) dx dy = 0.75 * sum(flux)
    assert abs(src_g.sum() * st["dx"] * st["dy"] - 0.75 * fl.sum()) < 1e-11 * fl.sum()
    assert np.count_nonzero(src_g) < src_g.size or n == 100          # far cells are exactly zero (underflow), as in the reference
    G.close()


def test_timestep_with_moulin_source_bitwise(oracle):
    from suhmo_amd import model, level as lv
    nx, ny = 160, 32
    m = dict(sy.A3_MODEL, use_moulin_source=1, ramp=0.8, distributed_input=7.93e-11)   # B_SHMIP: background input
    st = sy.shmip_initial_state(nx, ny)
    pos, sg, fl = moulins(3, 9)
    sg = sg * 8.0                                                    # a few cells wide on this coarse grid
    src, _ = oracle.moulin_source(nx, ny, st["dx"], st["dy"], pos, sg, fl, 1.0)
    O = oracle.OracleModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=32, nthreads=2)
    G = model.HipModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=32)
    O.set_state(st); G.set_state(st)
    O.field(oracle.OM_MSRC)[1:-1, 1:-1] = src
    G.level.set(lv.F_MSRC, src)
    for k in range(3):
        assert O.timestep(m["dt"]) == G.timestep(m["dt"])
        for nm, fid in (("head", oracle.OM_H), ("B", oracle.OM_B), ("rhs_h", oracle.OM_RHSH), ("mR", oracle.OM_MR)):
            a, b = np.array(O.field(fid))[1:-1, 1:-1], G.get(nm)
            assert np.array_equal(a, b), (k, nm, float(np.max(np.abs(a - b))))
    assert np.all(np.isfinite(G.get("head")))
    O.close(); G.close()


@pytest.mark.parametrize("impl", [1, 0])
def test_timestep_with_diffusion_bitwise(oracle, impl):
    """suhmo.diffFactor = 1: the diffusive term div(D grad b) in RHS_h and, with solver.use_ImplDiff, the implicit
    gap-height solve (exec/B_SHMIP/B<k>/input.hydro:31,56) -- head, gap height, D and the term itself bit for bit"""
    from suhmo_amd import model, level as lv
    nx, ny = 160, 32
    m = dict(sy.A3_MODEL, use_moulin_source=1, ramp=1.0, distributed_input=7.93e-11, diffFactor=1.0, use_impl_diff=impl)
    st = sy.shmip_initial_state(nx, ny)
    pos, sg, fl = moulins(3, 9)
    sg = sg * 8.0
    src, _ = oracle.moulin_source(nx, ny, st["dx"], st["dy"], pos, sg, fl, 1.0)
    O = oracle.OracleModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=32, nthreads=2)
    G = model.HipModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=32)
    O.set_state(st); G.set_state(st)
    O.field(oracle.OM_MSRC)[1:-1, 1:-1] = src
    G.level.set(lv.F_MSRC, src)
    for k in range(4):
        assert O.timestep(m["dt"]) == G.timestep(m["dt"]), k
        for nm, fid in (("head", oracle.OM_H), ("B", oracle.OM_B), ("rhs_h", oracle.OM_RHSH), ("mR", oracle.OM_MR)):
            a, b = np.array(O.field(fid))[1:-1, 1:-1], G.get(nm)
            assert np.array_equal(a, b), (k, nm, float(np.max(np.abs(a - b))))
    assert np.all(np.isfinite(G.get("B"))) and G.get("B").min() > 0.0
    O.close(); G.close()


def test_time_varying_recharge_and_timestep_bitwise(oracle):
    """suhmo.time_varying_input (suites D / F): the recharge field COMPUTE_TIMEVARYINGRECHARGE builds from the ice surface
    height, bitwise, and a time step consuming it as its source term"""
    from suhmo_amd import model
    nx, ny = 96, 32
    st = sy.shmip_initial_state(nx, ny)
    X = (np.arange(-1, nx + 1) + 0.5)[None, :] * st["dx"] + np.zeros((ny + 2, 1))
    zs = 6.0 * (np.sqrt(X + 5000.0) - np.sqrt(5000.0)) + 1.0 + st["zb"]           # surface of the sqrt ice sheet, 0 .. 1500 m
    m = dict(sy.A3_MODEL, use_moulin_source=1, ramp=1.0, distributed_input=0.0)
    O = oracle.OracleModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=16, nthreads=2)
    G = model.HipModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=16)
    O.set_state(st)
    G.set_state(st)
    for k, day in enumerate((200.0, 230.0)):                                        # summer: the lower part of the sheet melts
        T_K = -16.0 * np.cos(2.0 * np.pi * day / 365.0) - 5.0
        ro = oracle.time_varying_recharge(zs, T_K, 7.93e-11)
        G.time_varying_recharge(zs, T_K, 7.93e-11)
        rg = G.level.get(model.lv.F_MSRC, ghosted=True)
        assert np.array_equal(ro, rg) and ro.max() > 10.0 * 7.93e-11 and ro.min() == 7.93e-11
        O.field(oracle.OM_MSRC)[:] = ro
        assert O.timestep(m["dt"]) == G.timestep(m["dt"])
        for nm, fid in (("head", oracle.OM_H), ("B", oracle.OM_B), ("rhs_h", oracle.OM_RHSH)):
            assert np.array_equal(np.array(O.field(fid))[1:-1, 1:-1], G.get(nm)), (k, nm)
    O.close()
    G.close()


def test_moulin_source_pinned_by_the_channelized_convergence_table():
    """the RHS_moulin column of exec/0_convergence_channelized/CONV_ANA/results/convergence_data_singleLevel.dat through the
    device kernels: six rows, 5 digits (see tests/test_oracle_timeloop.py for what the column is)"""
    import os, sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "..", "tools"))
    import convergence_channelized as cc
    ref = {int(float(r[0])): r[5] for r in np.loadtxt(os.path.join(here, "golden", "convergence_channelized_singleLevel_reference.dat"))}
    got = cc.moulin_table("hip", 7)
    for nx in ref:
        # the last two rows are differences at the 1e-10 / 1e-12 level of a term of order 5: there the device exp (1e-14
        # relative to the CPU library's) shows in the fourth / second digit; the oracle matches all six rows to five
        tol = 6e-5 if nx <= 256 else (1e-3 if nx == 512 else 5e-2)
        assert abs(got[nx] - ref[nx]) <= tol * ref[nx], (nx, got[nx], ref[nx])


def test_amr_moulin_source_against_the_2_and_3_level_convergence_tables():
    """device twin of tests/test_oracle_timeloop.py::test_amr_moulin_source_pinned_by_the_2_and_3_level_convergence_tables: the
    composite moulin source term of suhmo_hier_moulin_source on the grids inferred from the reference's own tables reproduces the
    RHS_moulin column of exec/0_convergence_channelized/CONV_ANA/results/convergence_data_{2Levels,3Levels}.dat: 5 digits in the
    rows above the noise floor of two exp libraries"""
    import os, sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "..", "tools"))
    import convergence_channelized as cc
    grids = cc.amr_grids()
    checked = 0
    for name in ("2Levels", "3Levels"):
        ref = {int(float(r[0])): r[5] for r in np.loadtxt(os.path.join(here, "golden", "convergence_channelized_%s_reference.dat" % name))}
        for case, rects in grids[name].items():
            nx0 = int(case)
            if ref[nx0] < 1e-9:
                continue                                # differences of 1e-10 and below: the two exp libraries differ there
            e = cc.amr_moulin_error(nx0, rects, "hip")
            assert abs(e - ref[nx0]) <= 6e-5 * ref[nx0], (name, nx0, e, ref[nx0])
            checked += 1
    assert checked == 5


def test_moulin_entry_points_are_one_computation():
    """suhmo_level_moulin_source, suhmo_amr_moulin_source and suhmo_hier_moulin_source are one pass over their regions
    (suhmo_forcing.hip): the same nested hierarchy given as patches and as one box per level gets the same integrals and the same
    source term on every level, bit for bit; with no patch at all the single level agrees with both.  One moulin lies inside the
    finest patch, one on a coarse-fine boundary (x = 40), one at x = 10, so that the tiles of the base level beyond x = 50 take the
    underflow skip for it"""
    from suhmo_amd import model
    nx0, ny0 = 128, 16
    nested = ((8, 2, 39, 13), (24, 8, 55, 19))                   # in the coarser level's cells: x 8..40, y 2..14 and x 12..28, y 4..10
    pos, sg, fl = np.array([[20.3, 7.1], [40.0, 8.0], [10.2, 5.5]]), np.ones(3), np.array([30.0, 40.0, 20.0])
    for patches in (nested, ()):
        boxes = [[[2 * p[0], 2 * p[1], 2 * p[2] + 1, 2 * p[3] + 1]] for p in patches]
        A = model.HipAmrModel(nx0, ny0, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS, sy.A3_MODEL, patches, max_box=16)
        H = model.HipHierModel(nx0, ny0, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS, sy.A3_MODEL, boxes, max_box=16)
        ia, ih = A.moulin_source(pos, sg, fl, 0.75), H.moulin_source(pos, sg, fl, 0.75)
        assert np.all(np.isfinite(ia)) and np.all(ia > 0.0)
        assert np.array_equal(ia, ih), (ia, ih)
        for l in range(len(patches) + 1):
            a, h = A.get(l, "msrc"), H.get(l, 0, "msrc")
            assert a.max() > 0.0 and np.array_equal(a, h), (l, float(np.max(np.abs(a - h))))
        base = A.get(0, "msrc")
        assert np.all(base[:, 96:] == 0.0)                       # beyond the reach of every Gaussian: exactly zero
        if not patches:
            G = model.HipModel(nx0, ny0, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS, sy.A3_MODEL, max_box=16)
            ig = G.moulin_source(pos, sg, fl, 0.75)
            assert np.array_equal(ig, ia), (ig, ia)
            assert np.array_equal(G.get("msrc"), base)
            G.close()
        A.close(); H.close()
