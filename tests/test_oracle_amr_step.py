"""oracle/amr_step_m.c on nested patches (test infrastructure): the AMR time step's own pieces have no reference fixture (Chombo-side,
unpinned), so they are held to what they must satisfy: a one-level hierarchy IS the pinned single-level loop, the
ghost-cell interpolations are exact for the polynomials they are built for and bounded where they limit, moulins deliver
their flux over the composite grid, and the refined run stays closer to the uniformly fine one than the coarse run."""
import numpy as np

from oracle import pyoracle as po
from suhmo_amd import synthetic as sy

PATCH = (16, 8, 47, 23)


def make(nx0, ny0, patches, m=None, rough=0.5):
    m = dict(sy.A3_MODEL) if m is None else m
    sts = sy.shmip_amr_states(nx0, ny0, patches, rough=rough)
    A = po.OracleAmrModel(nx0, ny0, sts[0]["dx"], sts[0]["dy"], sy.A3_BC, sy.A3_PHYS, m, patches, max_box=16, nthreads=2)
    for l, st in enumerate(sts):
        A.set_state(l, st)
    return A, sts, m


def test_one_level_hierarchy_is_the_single_level_loop():
    A, sts, m = make(64, 32, ())
    M = po.OracleModel(64, 32, sts[0]["dx"], sts[0]["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=16, nthreads=2)
    M.set_state(sts[0])
    for k in range(3):
        assert A.timestep(m["dt"]) == M.timestep(m["dt"])
        for fid in (po.OM_H, po.OM_B, po.OM_MR, po.OM_QWX):
            assert np.array_equal(A.field(0, fid), M.field(fid))
    A.close()
    M.close()


def cell_centres(st):
    i = np.arange(st["i0"] - 1, st["i0"] + st["nx"] + 1) + 0.5
    j = np.arange(st["j0"] - 1, st["j0"] + st["ny"] + 1) + 0.5
    return np.meshgrid(i * st["dx"], j * st["dy"])


def ring(a):
    m = np.ones(a.shape, dtype=bool)
    m[1:-1, 1:-1] = False
    return m


def test_ghost_interpolations_exact_and_bounded():
    A, sts, _ = make(64, 32, (PATCH, (40, 22, 79, 41)))
    for l in (1, 2):
        Xc, Yc = cell_centres(sts[l - 1])
        Xf, Yf = cell_centres(sts[l])
        # PiecewiseLinearFillPatch reproduces a linear field (the limiter leaves eta = 1), corners included
        A.field(l - 1, po.OM_B)[:] = 3.0 + 2.0e-4 * Xc - 5.0e-4 * Yc
        A.field(l, po.OM_B)[:] = -7.0
        A.fill_ghosts(l, po.OM_B, "pwl")
        g = A.field(l, po.OM_B)
        exact = 3.0 + 2.0e-4 * Xf - 5.0e-4 * Yf
        assert np.max(np.abs(g - exact)[ring(g)]) < 1e-12 and np.all(g[1:-1, 1:-1] == -7.0)
        # ... and stays inside the range of the coarse neighbourhood for rough data (FORT_INTERPLIMIT)
        rng = np.random.default_rng(5)
        c = rng.uniform(0.0, 1.0, size=Xc.shape)
        A.field(l - 1, po.OM_B)[:] = c
        A.fill_ghosts(l, po.OM_B, "pwl")
        g = A.field(l, po.OM_B)
        assert g[ring(g)].min() >= c.min() - 1e-15 and g[ring(g)].max() <= c.max() + 1e-15
        # QuadCFInterp: exact for a quadratic (coarse and fine data sampled from it), edges only
        q = lambda X, Y: 1.0 + 1.0e-4 * X + 2.0e-4 * Y + 3.0e-9 * X * X - 2.0e-9 * Y * Y
        A.field(l - 1, po.OM_H)[:] = q(Xc, Yc)
        h = A.field(l, po.OM_H)
        h[:] = q(Xf, Yf)
        e = h.copy()
        h[0, :] = h[-1, :] = h[:, 0] = h[:, -1] = 0.0
        A.fill_ghosts(l, po.OM_H, "quad")
        edges = ring(h)
        edges[0, 0] = edges[0, -1] = edges[-1, 0] = edges[-1, -1] = False
        assert np.max(np.abs(h - e)[edges]) < 1e-9 * np.max(np.abs(e))
    A.close()


def test_moulins_deliver_their_flux_over_the_composite_grid():
    patches = (PATCH, (40, 22, 79, 41))
    A, sts, _ = make(64, 32, patches, dict(sy.A3_MODEL, use_moulin_source=1))
    pos = np.array([[52000.0, 10500.0], [20000.0, 4000.0], [80000.0, 15000.0]])
    sg, fl = np.full(3, 1500.0), np.array([30.0, 20.0, 40.0])
    integ = A.moulin_source(pos, sg, fl, 0.5)
    assert np.all(integ > 0.0)
    tot = 0.0
    for l in range(3):
        s = np.array(A.field(l, po.OM_MSRC))[1:-1, 1:-1]
        cov = np.zeros_like(s, dtype=bool)
        if l < 2:
            ci0, cj0, ci1, cj1 = patches[l]
            cov[cj0 - sts[l]["j0"]:cj1 + 1 - sts[l]["j0"], ci0 - sts[l]["i0"]:ci1 + 1 - sts[l]["i0"]] = True
            fine = np.array(A.field(l + 1, po.OM_MSRC))[1:-1, 1:-1]
            avg = 0.25 * (fine[0::2, 0::2] + fine[0::2, 1::2] + fine[1::2, 0::2] + fine[1::2, 1::2])
            assert np.allclose(s[cov].reshape(avg.shape), avg, rtol=1e-14, atol=0.0)          # CoarseAverage of the finer level
        tot += s[~cov].sum() * sts[l]["dx"] * sts[l]["dy"]
    assert abs(tot - 0.5 * fl.sum()) < 1e-11 * fl.sum()
    A.close()


def test_refined_run_is_closer_to_the_fine_run_than_the_coarse_run():
    """3 steps from a smooth state: head on the patch of a 2-level run vs a uniformly fine (128 x 64) run and vs the
    coarse (64 x 32) run injected onto the fine cells"""
    m = dict(sy.A3_MODEL)
    A, sts, _ = make(64, 32, (PATCH,), m, rough=0.3)
    fine = sy.shmip_amr_states(128, 64, (), rough=0.3)[0]
    coarse = sy.shmip_amr_states(64, 32, (), rough=0.3)[0]
    F = po.OracleModel(128, 64, fine["dx"], fine["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=16, nthreads=4)
    Cm = po.OracleModel(64, 32, coarse["dx"], coarse["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=16, nthreads=2)
    F.set_state(fine)
    Cm.set_state(coarse)
    for k in range(3):
        A.timestep(m["dt"]); F.timestep(m["dt"]); Cm.timestep(m["dt"])
    ci0, cj0, ci1, cj1 = PATCH
    hf = np.array(F.field(po.OM_H))[1:-1, 1:-1][2 * cj0:2 * cj1 + 2, 2 * ci0:2 * ci1 + 2]
    hp = np.array(A.field(1, po.OM_H))[1:-1, 1:-1]
    hc = np.repeat(np.repeat(np.array(Cm.field(po.OM_H))[1:-1, 1:-1][cj0:cj1 + 1, ci0:ci1 + 1], 2, axis=0), 2, axis=1)
    inner = (slice(4, -4), slice(4, -4))
    e_amr, e_coarse = np.max(np.abs(hp - hf)[inner]), np.max(np.abs(hc - hf)[inner])
    assert np.all(np.isfinite(hp)) and e_amr < e_coarse, (e_amr, e_coarse)
    A.close(); F.close(); Cm.close()
