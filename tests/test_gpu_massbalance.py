"""suhmo_level_mass_balance, suhmo_hier_mass_balance, suhmo_batch_mass_balance (include/suhmo_hip.h, "MASS BALANCE"; suhmo_amd/csrc/suhmo_balance.hip):
AmrHydro::check_fluxes on the device, BITWISE against the numpy twin tests/massbalance_ref.py fed from ghosted gets -- single levels at the shapes
where the walk of the first stage strides and the last column sits on and off a wave edge, under Dirichlet, Neumann and x-periodic sides with the
valley's oblique margin after a step; the hierarchies of the flatten sweep and a level of boxes beyond CAP_BOX, after a step and after a regrid;
ensembles against the twin and against the same models alone; the launch and copy counts; that the calls change nothing; every refusal."""
import ctypes as C

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import flatten_ref as fr
from tests import hierlayouts as hl
from tests import massbalance_ref as mb
from tests import reduce_ref as rr
from tests import stepsweep as sw
from tests.test_gpu_snapshot import same_bits

pytestmark = pytest.mark.gpu
DT = 60.0
MODEL = sw.model_of("explicit")


def box_data(L):
    """what the twin reads of a box, as the canvases hold it"""
    from suhmo_amd import level as lv
    return dict(head=L.get(lv.F_PHI, ghosted=True), mask=L.get(lv.F_MASK, ghosted=True), B=L.get(lv.F_B, ghosted=True), bx=L.get(lv.F_BX), by=L.get(lv.F_BY))


def level_ref(L, bc, what):
    ref = mb.balance_of_level([box_data(L)], [(0, 0, L.nx - 1, L.ny - 1)], (L.nx, L.ny), bc, L.dx, L.dy, rr.CAP_LEVEL)
    assert np.isfinite(ref).all(), (what, ref)
    return ref


def as_row(d):
    return np.array([d[k] for k in mb.NAMES])


def valley_model(nx, ny, bc, gamma=0.05, gap=0.01):
    """the valley glacier of SHMIP E on nx x ny cells, one explicit step later: an oblique ice margin, masked gradients, K = 0 outside the ice"""
    from suhmo_amd import level as lv, model
    st = sy.valley_initial_state(nx, ny, gamma, gap_init=gap)
    G = model.HipModel(nx, ny, st["dx"], st["dy"], bc, sw.PHYS, MODEL, max_box=64)
    G.set_state(st)
    G.level.set(lv.F_MR, np.full((ny, nx), MODEL["G"] / MODEL["L"]))
    G.timestep(DT)
    return G


# ------------------------------------------------------------------ 1. single levels
@pytest.mark.parametrize("bcname", [n for n, _ in mb.SINGLE_BCS])
@pytest.mark.parametrize("nx,ny", mb.SINGLE_SHAPES, ids=["%dx%d" % s for s in mb.SINGLE_SHAPES])
def test_single_levels_against_the_twin(nx, ny, bcname):
    """70 x 9 and 64 x 4: the last column off and on a wave edge; 16 x 516 and 2052 x 4: the first shapes beyond CAP_LEVEL in each direction"""
    bc = dict(mb.SINGLE_BCS)[bcname]
    G = valley_model(nx, ny, bc)
    got = as_row(G.mass_balance())
    ref = level_ref(G.level, bc, (nx, ny, bcname))
    print(nx, ny, bcname, got, ref)
    assert np.array_equal(got, ref), (nx, ny, bcname, got, ref)
    assert same_bits(got, as_row(G.mass_balance())), "the call twice"
    assert got[mb.VOLUME] > 0.0 and (got[:6] != 0.0).any()
    G.close()


# ------------------------------------------------------------------ 2. hierarchies, 4. the counters
def hier_model(nx0, ny0, bc, boxes):
    from suhmo_amd import model
    sts = sy.shmip_amrm_states(nx0, ny0, boxes, rough=0.5)
    M = model.HipHierModel(nx0, ny0, sts[0][0]["dx"], sts[0][0]["dy"], bc, sy.A3_PHYS, sy.A3_MODEL, boxes, max_box=16)
    M.set_states(sts)
    M.timestep(sy.A3_MODEL["dt"])
    return M


def load_masks(M, nx0, ny0, bc, seed):
    """every box's ice mask <- its cut of massbalance_ref.level_mask of its level: margins inside the boxes, on the sides boxes share, on coarse-fine
    sides and on the domain sides; the face coefficients stay what the step left"""
    from suhmo_amd import level as lv
    for l, bl in enumerate(fr.all_boxes(nx0, ny0, M.hier.boxes)):
        m = mb.level_mask(nx0 << l, ny0 << l, bc["periodic"], seed)
        for k, b in enumerate(bl):
            M.level[l][k].set(lv.F_MASK, mb.cut(m, b), ghosted=True)


def assert_hier_against_the_twin(M, nx0, ny0, bc, what):
    nlev = M.hier.nlev
    n_l, n_c = M.hier.get_option("balance_launches"), M.hier.get_option("balance_copies")
    got = np.array([as_row(d) for d in M.mass_balance()])
    assert M.hier.get_option("balance_launches") - n_l == nlev + 1 and M.hier.get_option("balance_copies") - n_c == 1, what
    assert got.shape == (nlev, 7)
    for l, bl in enumerate(fr.all_boxes(nx0, ny0, M.hier.boxes)):
        L0 = M.level[l][0]
        ref = mb.balance_of_level([box_data(L) for L in M.level[l]], bl, (nx0 << l, ny0 << l), bc, L0.dx, L0.dy, rr.CAP_LEVEL if l == 0 else rr.CAP_BOX)
        print(what, "level", l, got[l], ref)
        assert np.isfinite(ref).all(), (what, l, ref)
        assert np.array_equal(got[l], ref), (what, "level", l, got[l], ref)
    return got


@pytest.mark.parametrize("key", mb.HIER_KEYS, ids=[str(k) for k in mb.HIER_KEYS])
def test_hierarchies_against_the_twin(key):
    """the generated layouts of the flatten sweep (2 to 4 levels, all four periodicities), a box over the whole width, boxes two cells wide: one step
    later, as the step left the masks and with margins loaded into every box"""
    bc, boxes = fr.case(key)
    M = hier_model(hl.NX0, hl.NY0, bc, boxes)
    assert_hier_against_the_twin(M, hl.NX0, hl.NY0, bc, (key, "as stepped"))
    load_masks(M, hl.NX0, hl.NY0, bc, 7)
    got = assert_hier_against_the_twin(M, hl.NX0, hl.NY0, bc, (key, "margins"))
    assert (got[:, mb.DIR_X] != 0.0).all() and (got[:, mb.DIR_Y] != 0.0).all()
    M.close()


def test_level_0_of_a_hierarchy_has_the_bits_of_the_level_alone():
    """the second stage is per level: a base level without finer levels gives what suhmo_level_mass_balance gives on the same state"""
    from suhmo_amd import level as lv, model
    nx, ny = 70, 9
    st = sy.valley_initial_state(nx, ny, 0.05)
    G = valley_model(nx, ny, mb.NEUMANN_BC)
    H = model.HipHierModel(nx, ny, st["dx"], st["dy"], mb.NEUMANN_BC, sw.PHYS, MODEL, [], max_box=64)
    H.set_state(0, 0, st)
    H.level[0][0].set(lv.F_MR, np.full((ny, nx), MODEL["G"] / MODEL["L"]))
    H.timestep(DT)
    a, b = as_row(G.mass_balance()), as_row(H.mass_balance()[0])
    assert same_bits(a, b), (a, b)
    G.close(); H.close()


def test_boxes_beyond_the_cap_of_a_box():
    """one refined level with a box of 8 x 68 cells (17 workgroups of rows: beyond CAP_BOX in y) and one of 260 x 4 (5 workgroups of columns: beyond
    it in x); every box runs on the grid of the largest extents, 260 x 68"""
    nx0, ny0, boxes = mb.WALK_EDGE_LAYOUT
    M = hier_model(nx0, ny0, hl._NP, boxes)
    load_masks(M, nx0, ny0, hl._NP, 8)
    assert_hier_against_the_twin(M, nx0, ny0, hl._NP, "walk edges")
    M.close()


def test_after_a_regrid_the_new_boxes_are_balanced():
    from suhmo_amd import capi
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT as HDT, REGRID
    M = shmip_model()
    M.moulin_source(**MOULINS)
    M.timestep(HDT)
    assert M.hier.get_option("balance_device_bytes") == 0
    assert_hier_against_the_twin(M, 64, 32, sy.A3_BC, "before the regrid")
    assert M.hier.get_option("balance_device_bytes") > 0
    old = [list(bl) for bl in M.hier.boxes]
    boxes, same = M.tag_and_regrid(**REGRID)
    assert not same and boxes != old and len(boxes) >= 1
    assert [M.hier.get_option(k) for k in ("balance_launches", "balance_copies", "balance_device_bytes")] == [0, 0, 0], "a new handle: it holds no buffer yet"
    # the new boxes hold no face coefficients until a step has formed them: refused, nothing launched
    out = np.full((M.hier.nlev, 7), -77.0)
    rc = capi.lib().suhmo_hier_mass_balance(M.hier.h, out.ctypes.data_as(C.POINTER(C.c_double)), M.hier.stream)
    assert rc == -1 and b"face coefficients" in capi.lib().suhmo_last_error() and (out == -77.0).all() and M.hier.get_option("balance_launches") == 0
    M.moulin_source(**MOULINS)
    M.timestep(HDT)
    assert_hier_against_the_twin(M, 64, 32, sy.A3_BC, "after the regrid")
    load_masks(M, 64, 32, sy.A3_BC, 9)
    assert_hier_against_the_twin(M, 64, 32, sy.A3_BC, "after the regrid, margins")
    M.close()


# ------------------------------------------------------------------ 3. ensembles
def member_inputs(n, nx, ny):
    """n valley states that differ (the bed's slope parameter and the gap height), and the BC values of every member"""
    sts = [sy.valley_initial_state(nx, ny, 0.05 - 0.04 * k, gap_init=0.01 * (1 + 0.25 * k)) for k in range(n)]
    bcs = [dict(mb.MIXED_BC, value=[[0.02, 40.0 + k], [3.0 - 0.125 * k, -0.01]]) for k in range(n)]
    return sts, bcs


@pytest.mark.parametrize("n", [1, 5, 16])
def test_ensembles_against_the_twin_and_the_members_alone(n):
    from suhmo_amd import level as lv, model
    nx, ny = 70, 9
    sts, bcs = member_inputs(n, nx, ny)
    B = model.HipBatchModel(nx, ny, sts[0]["dx"], sts[0]["dy"], bcs, sw.PHYS, [MODEL] * n, max_box=64)
    for k in range(n):
        B.set_state(k, sts[k])
        B.member(k).level.set(lv.F_MR, np.full((ny, nx), MODEL["G"] / MODEL["L"]))
    B.timestep(DT)
    n_l, n_r = B.batch.get_option("batch_launches"), B.batch.get_option("batch_readbacks")
    got = B.mass_balance_all()
    assert B.batch.get_option("batch_launches") - n_l == 2 and B.batch.get_option("batch_readbacks") - n_r == 1
    for k in range(n):
        ref = level_ref(B.member(k).level, bcs[k], ("member", k))
        print(n, k, got[k], ref)
        assert np.array_equal(got[k], ref), (n, k, got[k], ref)
    for k in sorted({0, n // 2, n - 1}):                         # the same model alone: the same bits
        G = model.HipModel(nx, ny, sts[k]["dx"], sts[k]["dy"], bcs[k], sw.PHYS, MODEL, max_box=64)
        G.set_state(sts[k])
        G.level.set(lv.F_MR, np.full((ny, nx), MODEL["G"] / MODEL["L"]))
        G.timestep(DT)
        assert same_bits(as_row(G.mass_balance()), got[k]), (n, k)
        G.close()
    if n >= 5:                                                # a member subset: the rows without a flag keep the caller's values
        active = [k % 3 != 1 for k in range(n)]
        out = np.full((n, 7), -77.0)
        n_l, n_r = B.batch.get_option("batch_launches"), B.batch.get_option("batch_readbacks")
        assert B.mass_balance_all(active=active, out=out) is out
        assert B.batch.get_option("batch_launches") - n_l == 2 and B.batch.get_option("batch_readbacks") - n_r == 1
        for k in range(n):
            assert same_bits(out[k], got[k] if active[k] else np.full(7, -77.0)), (n, k)
        none = np.full((n, 7), -77.0)
        B.mass_balance_all(active=[False] * n, out=none)
        assert (none == -77.0).all() and B.batch.get_option("batch_readbacks") - n_r == 1
    B.close()


# ------------------------------------------------------------------ 5. read-only
def test_a_snapshot_before_and_after_is_the_same():
    from suhmo_amd import level as lv, plotfile
    bc, boxes = fr.case(2)
    M = hier_model(hl.NX0, hl.NY0, bc, boxes)
    load_masks(M, hl.NX0, hl.NY0, bc, 7)
    before = M.hier.snapshot(plotfile.SNAP, 1)[2].copy()
    faces = [[(L.get(lv.F_BX), L.get(lv.F_BY)) for L in bl] for bl in M.level]
    M.mass_balance(); M.mass_balance()
    assert same_bits(before, M.hier.snapshot(plotfile.SNAP, 1)[2])
    for bl, fl in zip(M.level, faces):
        for L, (bx, by) in zip(bl, fl):
            assert same_bits(bx, L.get(lv.F_BX)) and same_bits(by, L.get(lv.F_BY))
    M.close()
    G = valley_model(70, 9, mb.DIRICHLET_BC)
    snap = G.level.snapshot(plotfile.SNAP, 1).copy()
    G.mass_balance()
    assert same_bits(snap, G.level.snapshot(plotfile.SNAP, 1))
    G.close()


def test_a_model_balanced_between_its_steps_stays_its_twin():
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT as HDT, assert_same_state
    A, B = shmip_model(), shmip_model()
    for G in (A, B):
        G.moulin_source(**MOULINS)
    for n in range(3):
        assert A.timestep(HDT) == B.timestep(HDT)
        out = A.mass_balance()
        assert len(out) == A.hier.nlev and all(sorted(d) == sorted(mb.NAMES) and np.isfinite(as_row(d)).all() and d["volume"] > 0.0 for d in out)
    assert_same_state(A, B)
    A.close(); B.close()
    X, Y = valley_model(64, 4, mb.NEUMANN_BC), valley_model(64, 4, mb.NEUMANN_BC)
    for n in range(2):
        X.mass_balance()
        assert X.timestep(DT) == Y.timestep(DT)
    for nm in X.FIELDS:
        assert np.array_equal(X.get(nm, ghosted=True), Y.get(nm, ghosted=True), equal_nan=True), nm
    X.close(); Y.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_output_and_the_model_alone():
    from suhmo_amd import capi, level as lv, model
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT as HDT, DX0, STEP_MODEL, assert_same_state
    lib = capi.lib()
    out = np.full(8 * 7, -77.0)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    # a level no solve and no step has run on: rc -1; after a step it goes through
    st = sy.valley_initial_state(70, 9, 0.05)
    G = model.HipModel(70, 9, st["dx"], st["dy"], mb.NEUMANN_BC, sw.PHYS, MODEL, max_box=64)
    T = model.HipModel(70, 9, st["dx"], st["dy"], mb.NEUMANN_BC, sw.PHYS, MODEL, max_box=64)
    for X in (G, T):
        X.set_state(st)
        X.level.set(lv.F_MR, np.full((9, 70), MODEL["G"] / MODEL["L"]))
    assert lib.suhmo_level_mass_balance(G.level.h, dp, G.level.stream) == -1 and b"face coefficients" in lib.suhmo_last_error()
    assert lib.suhmo_level_mass_balance(G.level.h, None, G.level.stream) == -1 and lib.suhmo_level_mass_balance(None, dp, None) == -1
    assert G.timestep(DT) == T.timestep(DT)
    assert same_bits(as_row(G.mass_balance()), as_row(T.mass_balance()))
    # a rank strip: rc -5
    S = lv.HipLevel(70, 8, st["dx"], st["dy"], mb.NEUMANN_BC, sw.PHYS, max_box=64, j0=0, ny_global=16)
    S.set(lv.F_BX, np.ones((8, 71)))
    assert lib.suhmo_level_mass_balance(S.h, dp, S.stream) == -5 and b"strip" in lib.suhmo_last_error()
    S.close()
    # an ensemble with a member that has no faces yet: rc -1, whichever member it is; members without a flag are not asked
    sts, bcs = member_inputs(3, 70, 9)
    B = model.HipBatchModel(70, 9, sts[0]["dx"], sts[0]["dy"], bcs, sw.PHYS, [MODEL] * 3, max_box=64)
    for k in range(3):
        B.set_state(k, sts[k])
        B.member(k).level.set(lv.F_MR, np.full((9, 70), MODEL["G"] / MODEL["L"]))
    n_l = B.batch.get_option("batch_launches")
    assert lib.suhmo_batch_mass_balance(B.batch.h, dp, None, B.batch.stream) == -1 and b"member 0" in lib.suhmo_last_error()
    assert lib.suhmo_batch_mass_balance(B.batch.h, None, None, B.batch.stream) == -1 and lib.suhmo_batch_mass_balance(None, dp, None, None) == -1
    assert B.batch.get_option("batch_launches") == n_l
    B.timestep(DT)
    assert np.isfinite(B.mass_balance_all()).all()
    B.close()
    # hierarchies: before the first step rc -1; a box handle passed to the level call, a hierarchy on strips or created with shadow = 1: rc -5
    M, U = shmip_model(), shmip_model()
    for X in (M, U):
        X.moulin_source(**MOULINS)
    assert lib.suhmo_hier_mass_balance(M.hier.h, dp, M.hier.stream) == -1 and b"face coefficients" in lib.suhmo_last_error()
    assert lib.suhmo_hier_mass_balance(M.hier.h, None, M.hier.stream) == -1 and lib.suhmo_hier_mass_balance(None, dp, None) == -1
    assert M.timestep(HDT) == U.timestep(HDT)
    assert lib.suhmo_level_mass_balance(M.level[1][0].h, dp, M.hier.stream) == -5 and b"not built" in lib.suhmo_last_error()
    S = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, j0=0, ny_global=64)
    W = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, options="shadow=1")
    for X in (S, W):
        assert lib.suhmo_hier_mass_balance(X.hier.h, dp, X.hier.stream) == -5 and b"not built" in lib.suhmo_last_error()
        assert X.hier.get_option("balance_launches") == 0
    S.close(); W.close()
    assert M.hier.get_option("balance_launches") == 0 and (out == -77.0).all(), "nothing was launched, nothing was written"
    assert M.timestep(HDT) == U.timestep(HDT)
    assert_same_state(M, U)
    # ... and the calls the refusals were variations of go through
    capi.check(lib.suhmo_hier_mass_balance(M.hier.h, dp, M.hier.stream))
    assert not (out[:7 * M.hier.nlev] == -77.0).any() and (out[7 * M.hier.nlev:] == -77.0).all()
    for X in (G, T, M, U):
        X.close()
