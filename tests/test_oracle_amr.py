"""CPU checks of the AMR restatement (oracle/amrm.c) on nested patches: coarse-fine interpolation is exact for
quadratics, the composite operator conserves (reflux), and the 2-level FAS solve converges to a solution that is
closer to the uniformly fine one than the coarse solve is."""
import numpy as np

from suhmo_amd import synthetic as sy

BC = dict(type=[[0, 0], [1, 0]], value=[[0.0, 0.0], [0.0, 0.0]], periodic=[0, 1])     # 2lev_base/input.hydro:8-13,76


def make(oracle, nxc=64, nyc=16, patch=sy.CFG3_PATCH, bc=BC, ph=sy.CFG3_PHYS, **kw):
    c, f = sy.amr2_fields(nxc, nyc, patch, **kw)
    A = oracle.OracleAmr2(nxc, nyc, c["dx"], c["dy"], bc, ph, patch, max_box=32, nthreads=2)
    A.coarse.set_inputs(c)
    A.coarse.build_mg_coefficients()
    A.set_fine_inputs(f)
    return A, c, f


def test_cf_interp_reproduces_quadratics(oracle):
    A, c, f = make(oracle)
    q = lambda X, Y: 3.0 + 0.2 * X - 0.1 * Y + 0.01 * X * X + 0.02 * Y * Y          # separable quadratic: exact
    xc = (np.arange(64) + 0.5) * c["dx"]
    yc = (np.arange(16) + 0.5) * c["dy"]
    A.coarse.set(oracle.F_PHI, q(*np.meshgrid(xc, yc)))
    ci0, cj0, ci1, cj1 = sy.CFG3_PATCH
    xf = (np.arange(2 * ci0 - 1, 2 * ci1 + 3) + 0.5) * f["dx"]
    yf = (np.arange(2 * cj0 - 1, 2 * cj1 + 3) + 0.5) * f["dy"]
    exact = q(*np.meshgrid(xf, yf))
    A.fine_set(oracle.F_PHI, exact[1:-1, 1:-1])
    A.cf_interp()
    g = A.fine_get(oracle.F_PHI, ghosted=True)
    for sl in ((slice(1, -1), 0), (slice(1, -1), -1), (0, slice(1, -1)), (-1, slice(1, -1))):
        assert np.max(np.abs(g[sl] - exact[sl])) < 1e-12 * np.max(np.abs(exact)), sl
    A.close()


def test_two_level_solve_converges_and_beats_the_coarse_solve(oracle):
    sp = dict(sy.SOLVER_DEFAULT, eps=1e-9, norm_thresh=1e-14, max_iter=30, imin=30)
    A, c, f = make(oracle)
    r0 = A.residual()
    n, hist = A.solve(sp)
    # the coefficient bCoef(head) is rebuilt every cycle, so from a random head the residual first rises (the
    # single-level solves do the same); afterwards it falls by > 2x per cycle
    assert hist[-1] < 1e-6 * r0 and hist[-1] < 1e-9 * np.max(hist), hist
    assert np.all(hist[6:] < 0.5 * hist[5:-1]), hist
    phi_f = A.fine_get(oracle.F_PHI)
    phi_c2 = A.coarse.get(oracle.F_PHI)
    # uniformly fine reference (128 x 32) and plain coarse solve
    cf, _ = sy.amr2_fields(128, 32, (16, 8, 47, 23))
    U = oracle.OracleLevel(128, 32, cf["dx"], cf["dy"], BC, sy.CFG3_PHYS, 0.0, -1.0, 32, 2)
    U.set_inputs(cf); U.build_mg_coefficients(); U.solve(sp)
    ref = U.get(oracle.F_PHI)
    cc, _ = sy.amr2_fields(64, 16)
    Cc = oracle.OracleLevel(64, 16, cc["dx"], cc["dy"], BC, sy.CFG3_PHYS, 0.0, -1.0, 32, 2)
    Cc.set_inputs(cc); Cc.build_mg_coefficients(); Cc.solve(sp)
    ci0, cj0, ci1, cj1 = sy.CFG3_PATCH
    win = ref[2 * cj0:2 * cj1 + 2, 2 * ci0:2 * ci1 + 2]
    err_amr = np.max(np.abs(phi_f - win))
    coarse_on_fine = np.kron(Cc.get(oracle.F_PHI)[cj0:cj1 + 1, ci0:ci1 + 1], np.ones((2, 2)))
    err_coarse = np.max(np.abs(coarse_on_fine - win))
    assert err_amr < 0.7 * err_coarse, (err_amr, err_coarse)
    # covered coarse cells hold the average of the fine solution (AMRRestrictS) up to the last post-smoothing
    avg = 0.25 * (phi_f[0::2, 0::2] + phi_f[0::2, 1::2] + phi_f[1::2, 0::2] + phi_f[1::2, 1::2])
    assert np.max(np.abs(avg - phi_c2[cj0:cj1 + 1, ci0:ci1 + 1])) < 1e-3 * np.max(np.abs(avg))
    A.close(); U.close(); Cc.close()


PATCHES3 = (sy.CFG3_PATCH, (22, 11, 37, 20))      # level 2 inside level 1 ([16..47] x [8..23]) with 2+ cells of nesting


def make_n(oracle, patches, nx0=64, ny0=16, bc=BC, ph=sy.CFG3_PHYS, **kw):
    fs = sy.amr_fields(nx0, ny0, patches, **kw)
    A = oracle.OracleAmr(nx0, ny0, fs[0]["dx"], fs[0]["dy"], bc, ph, patches, max_box=32, nthreads=2)
    A.coarse.set_inputs(fs[0])
    A.coarse.build_mg_coefficients()
    for l in range(1, len(fs)):
        A.set_patch_inputs(l, fs[l])
    return A, fs


def test_n_level_code_with_two_levels_equals_the_two_level_code(oracle):
    sp = dict(sy.SOLVER_DEFAULT, eps=1e-9, norm_thresh=1e-14, max_iter=4, imin=30)
    A2, c, f = make(oracle)
    AN, fs = make_n(oracle, (sy.CFG3_PATCH,))
    assert A2.residual() == AN.residual()
    n2, h2 = A2.solve(sp)
    nn, hn = AN.solve(sp)
    assert n2 == nn and np.array_equal(h2, hn)
    assert np.array_equal(A2.fine_get(oracle.F_PHI), AN.patch_get(1, oracle.F_PHI))
    assert np.array_equal(A2.coarse.get(oracle.F_PHI), AN.coarse.get(oracle.F_PHI))
    A2.close(); AN.close()


def test_three_level_solve_converges(oracle):
    sp = dict(sy.SOLVER_DEFAULT, eps=1e-9, norm_thresh=1e-14, max_iter=30, imin=30)
    A, fs = make_n(oracle, PATCHES3)
    r0 = A.residual()
    n, hist = A.solve(sp)
    assert hist[-1] < 1e-6 * r0 and hist[-1] < 1e-9 * np.max(hist), hist
    assert np.all(hist[8:] < 0.6 * hist[7:-1]), hist
    # every coarser level holds the average of the finer one under the patch (up to the last post-smoothing)
    p2, p1 = A.patch_get(2, oracle.F_PHI), A.patch_get(1, oracle.F_PHI)
    avg = 0.25 * (p2[0::2, 0::2] + p2[0::2, 1::2] + p2[1::2, 0::2] + p2[1::2, 1::2])
    ci0, cj0, ci1, cj1 = PATCHES3[1]
    o0, o1 = 2 * sy.CFG3_PATCH[0], 2 * sy.CFG3_PATCH[1]
    win = p1[cj0 - o1:cj1 - o1 + 1, ci0 - o0:ci1 - o0 + 1]
    assert np.max(np.abs(avg - win)) < 1e-3 * np.max(np.abs(avg))
    A.close()
