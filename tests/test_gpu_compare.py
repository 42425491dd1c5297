"""suhmo_hier_compare (include/suhmo_hip.h, "COMPARE"; suhmo_amd/csrc/suhmo_compare.hip): the L1, L2 and max norms of a hierarchy's error against a
finer single-level run, BITWISE against the numpy twin tests/compare_ref.py: both modes over the layouts of the flatten sweep, the shapes at
which the walk of the first stage strides, the launch and copy counts, that the call changes nothing, a self-comparison, the hierarchy a regrid
leaves, every refusal."""
import ctypes as C

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import compare_ref as cr
from tests import flatten_ref as fr
from tests import hierlayouts as hl
from tests.test_gpu_flatten import components, load_random
from tests.test_gpu_snapshot import same_bits, stepped_model

pytestmark = pytest.mark.gpu
NX0, NY0 = hl.NX0, hl.NY0


def exact_level_of(nx0, ny0, dx0, dy0, el, bc, seed, fields, phys=sy.A3_PHYS):
    """a single level on the uniform grid of level `el` holding random `fields` -> (the level, {field: its valid cells})"""
    from suhmo_amd import level as lv
    nx, ny = nx0 << el, ny0 << el
    E = lv.HipLevel(nx, ny, dx0 / 2 ** el, dy0 / 2 ** el, bc, phys, max_box=64)
    rng = np.random.default_rng([seed, el, 4242])
    data = {}
    for f in fields:
        data[f] = np.where(rng.random((ny, nx)) < 0.3, -1.0, 1.0) if f == lv.F_MASK else rng.uniform(-1.0, 3.0, size=(ny, nx))
        E.set(f, data[f])
    return E, data


def exact_components(comps, data):
    return [cr.component(c[0], data[c[1]], data[c[2]] if len(c) > 2 else None) for c in comps]


def fields_of(comps):
    return sorted({f for c in comps for f in c[1:]})


def assert_both_modes(H, E, xs, el, comps, vals, boxes, what, nx0=NX0, ny0=NY0, modes=("composite", "finest")):
    """vals[q][l][k]: the hierarchy's component q in the valid cells; xs[q]: the exact component"""
    dx0, dy0 = H.level[0][0].dx, H.level[0][0].dy
    nlev = 1 + len(boxes)
    if "composite" in modes:
        n_l, n_c = H.get_option("compare_launches"), H.get_option("compare_copies")
        norms, terms = H.compare(E, comps, el, "composite", level_terms=True)
        assert H.get_option("compare_launches") - n_l == nlev + 1 and H.get_option("compare_copies") - n_c == 1, what
        again = H.compare(E, comps, el, "composite")
        assert same_bits(again, norms), (what, "without level_terms")
        for q in range(len(comps)):
            ref, lt = cr.composite(nx0, ny0, dx0, dy0, boxes, vals[q], xs[q], el)
            print(what, "composite", el, q, norms[q], ref)
            assert np.array_equal(norms[q], ref), (what, "composite", el, "component", q, norms[q], ref)
            assert np.array_equal(terms[:, q, :], lt), (what, "level_terms", el, "component", q, terms[:, q, :], lt)
    if "finest" in modes:
        n_l, n_c, f_l, f_c = (H.get_option(k) for k in ("compare_launches", "compare_copies", "flatten_launches", "flatten_copies"))
        norms = H.compare(E, comps, el, "finest")
        assert H.get_option("compare_launches") - n_l == 2 and H.get_option("compare_copies") - n_c == 1, what
        assert H.get_option("flatten_copies") == f_c, (what, "nothing but the result is copied")
        per_flatten = H.get_option("flatten_launches") - f_l
        flat = H.flatten(comps, el)
        assert H.get_option("flatten_launches") - f_l == 2 * per_flatten and H.get_option("flatten_copies") == f_c + 1, (what, "the flatten's own launches")
        w = E.dx * E.dy
        for q in range(len(comps)):
            ref = cr.finest(flat[q], xs[q], w)
            print(what, "finest", el, q, norms[q], ref)
            assert np.array_equal(norms[q], ref), (what, "finest", el, "component", q, norms[q], ref)


# ------------------------------------------------------------------ 1. both modes against the twin, 3. the counters
@pytest.mark.parametrize("key", [k for _, k in fr.CASES], ids=[n for n, _ in fr.CASES])
def test_both_modes_against_the_twin(key):
    """the layouts, the components and the data of the flatten sweep; the exact level at the finest level (its boxes compare cell by cell) and one
    above it, holding random fields; the level terms; FINEST against the twin's reduction of H.flatten(...) minus the exact array"""
    bc, boxes = fr.case(key)
    M = stepped_model(bc, boxes)
    vals = load_random(M, key)
    comps = components()
    top = len(boxes)
    for el in (top, top + 1):
        E, data = exact_level_of(NX0, NY0, M.level[0][0].dx, M.level[0][0].dy, el, bc, 5, fields_of(comps))
        assert_both_modes(M.hier, E, exact_components(comps, data), el, comps, vals, boxes, key)
        E.close()
    M.close()


# ------------------------------------------------------------------ 2. walk edges
def bare_hier(nx0, ny0, boxes, seed, fields):
    """a hierarchy that is never stepped, random `fields` in every box -> (H, {field: values[l][k]})"""
    from suhmo_amd import level as lv
    H = lv.HipHier(nx0, ny0, 1.0, 0.5, hl._NP, sy.A3_PHYS, boxes, max_box=64)
    vals = {f: [] for f in fields}
    for l, bl in enumerate(H.level):
        for f in fields:
            vals[f].append([])
        for k, L in enumerate(bl):
            rng = np.random.default_rng([seed, l, k])
            for f in fields:
                a = rng.uniform(-1.0, 3.0, size=(L.ny + 2, L.nx + 2))
                L.set(f, a, ghosted=True)
                vals[f][l].append(a[1:-1, 1:-1])
    return H, vals


@pytest.mark.parametrize("nx0,ny0,el,modes", [(70, 9, 0, ("composite", "finest")), (70, 9, 2, ("composite",)), (16, 516, 0, ("composite",)),
                                              (16, 516, 1, ("composite",)), (4, 130, 2, ("finest", "composite")), (6, 5, 5, ("composite",)),
                                              (66, 3, 6, ("composite",))],
                         ids=["70x9-r1", "70x9-r4", "16x516-r1", "16x516-r2", "4x130-finest", "6x5-r32", "66x3-r64"])
def test_walk_edges_on_level_0(nx0, ny0, el, modes):
    """70 x 9: not a multiple of the workgroup; 16 x 516: rows beyond CAP_LEVEL (128 workgroups of 4 rows); 4 x 130 at exact_level 2: the finest
    array has 520 rows; r = 32 and 64: the group of lanes that forms a row sum spans rows of 16 lanes, halves of a wave, the whole wave"""
    from suhmo_amd import capi, level as lv
    comps = [(capi.FLAT_FIELD, lv.F_B), (capi.FLAT_DIFF, lv.F_PI, lv.F_PW)]
    H, v = bare_hier(nx0, ny0, [], 3, fields_of(comps))
    vals = [v[lv.F_B], [[a - b for a, b in zip(la, lb)] for la, lb in zip(v[lv.F_PI], v[lv.F_PW])]]
    E, data = exact_level_of(nx0, ny0, 1.0, 0.5, el, hl._NP, 8, fields_of(comps))
    assert_both_modes(H, E, exact_components(comps, data), el, comps, vals, [], (nx0, ny0, el), nx0, ny0, modes)
    E.close()


def test_walk_edges_on_a_level_of_boxes():
    """one refined level with a box of 8 x 68 cells (17 workgroups of rows: beyond CAP_BOX in y) and one of 260 x 4 (5 workgroups of columns:
    beyond it in x); every box runs on the grid of the largest extents, 260 x 68"""
    from suhmo_amd import capi, level as lv
    nx0, ny0, boxes = 160, 48, [[(0, 0, 7, 67), (16, 80, 275, 83)]]
    comps = [(capi.FLAT_FIELD, lv.F_B), (capi.FLAT_DIFF, lv.F_PI, lv.F_PW)]
    H, v = bare_hier(nx0, ny0, boxes, 4, fields_of(comps))
    vals = [v[lv.F_B], [[a - b for a, b in zip(la, lb)] for la, lb in zip(v[lv.F_PI], v[lv.F_PW])]]
    for el in (1, 2):
        E, data = exact_level_of(nx0, ny0, 1.0, 0.5, el, hl._NP, 9, fields_of(comps))
        assert_both_modes(H, E, exact_components(comps, data), el, comps, vals, boxes, ("boxes", el), nx0, ny0, ("composite",))
        E.close()


# ------------------------------------------------------------------ 4. read-only
def test_a_snapshot_before_and_after_is_the_same():
    from suhmo_amd import plotfile
    bc, boxes = fr.case(9)
    M = stepped_model(bc, boxes)
    load_random(M, 9)
    comps = components()
    E, _ = exact_level_of(NX0, NY0, M.level[0][0].dx, M.level[0][0].dy, len(boxes) + 1, bc, 6, fields_of(comps))
    before = M.hier.snapshot(plotfile.SNAP, 1)[2].copy()
    xb = {f: E.get(f, ghosted=True) for f in fields_of(comps)}
    M.hier.compare(E, comps, len(boxes) + 1, "composite", level_terms=True)
    M.hier.compare(E, comps[:2], len(boxes) + 1, "finest")
    assert same_bits(before, M.hier.snapshot(plotfile.SNAP, 1)[2])
    assert all(same_bits(xb[f], E.get(f, ghosted=True)) for f in xb)
    E.close(); M.close()


def test_a_model_compared_between_its_steps_stays_its_twin():
    from suhmo_amd import model
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT, assert_same_state
    A, B = shmip_model(), shmip_model()
    for G in (A, B):
        G.moulin_source(**MOULINS)
    st = sy.shmip_amrm_states(256, 128, [], rough=0.5)[0][0]
    X = model.HipModel(256, 128, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, sy.A3_MODEL, max_box=64)
    X.set_state(st)
    X.timestep(DT)                                           # so that it holds Pw and Re
    A.compare(X)                                             # before the first step: the hierarchy holds no Pw yet (0.0)
    for n in range(3):
        assert A.timestep(DT) == B.timestep(DT)
        out = A.compare(X, mode=("composite", "finest")[n % 2])
        assert sorted(out) == ["N", "Pw", "Re", "gapHeight", "head"] and all(v.shape == (3,) and np.isfinite(v).all() for v in out.values())
        assert all(v[2] >= 0.0 and v[0] >= 0.0 for v in out.values()) and out["head"][2] > 0.0
    assert_same_state(A, B)
    A.close(); B.close()


# ------------------------------------------------------------------ 5. self-comparison
def test_a_level_against_itself_is_exactly_zero():
    from suhmo_amd import capi, level as lv
    comps = [(capi.FLAT_FIELD, lv.F_B), (capi.FLAT_DIFF, lv.F_PI, lv.F_PW), (capi.FLAT_FIELD, lv.F_PHI)]
    H, v = bare_hier(48, 20, [], 7, fields_of(comps))
    E = lv.HipLevel(48, 20, 1.0, 0.5, hl._NP, sy.A3_PHYS, max_box=64)
    for f in fields_of(comps):
        E.set(f, v[f][0][0])
    for mode in ("composite", "finest"):
        out = H.compare(E, comps, 0, mode)
        assert out.shape == (3, 3) and same_bits(out, np.zeros((3, 3))), (mode, out)
    E.close()


# ------------------------------------------------------------------ 6. after a regrid
def test_after_a_regrid_the_new_boxes_are_compared():
    from suhmo_amd import capi, level as lv, model
    from tests.test_gpu_regrid import load_random as load_named
    old = [[(8, 4, 23, 15)]]
    m = model.HipHierModel(NX0, NY0, 1.0, 1.0, hl._NP, hl.ADV_PHYS, sy.A3_MODEL, old, max_box=16)
    load_named(m, ("head", "Pi"), 9)
    b0 = np.random.default_rng(12).uniform(0.0, 0.4, size=(NY0 + 2, NX0 + 2))
    b0[1 + 6:1 + 10, 1 + 20:1 + 24] += 1.0                   # level-0 cells (20..23, 6..9): where the channel now is
    m.level[0][0].set(lv.F_B, b0, ghosted=True)
    m.level[1][0].set(lv.F_B, np.random.default_rng(13).uniform(0.0, 0.4, size=(14, 18)), ghosted=True)
    comps = [(capi.FLAT_FIELD, lv.F_B), (capi.FLAT_FIELD, lv.F_PI)]
    E, data = exact_level_of(NX0, NY0, 1.0, 1.0, 2, hl._NP, 10, fields_of(comps), hl.ADV_PHYS)
    xs = exact_components(comps, data)
    assert m.hier.get_option("compare_device_bytes") == 0
    m.hier.compare(E, comps, 2)                              # the old hierarchy has its partial buffer
    held = m.hier.get_option("compare_device_bytes")
    assert held > 0
    boxes, same = m.tag_and_regrid([dict(name="GapHeight", vmin=0.5, vmax=10.0, grow=1)], dict(fill_ratio=0.7, block_factor=2, max_box_size=32, nesting_radius=2))
    assert not same and boxes != old and m.hier.boxes == boxes
    assert (m.hier.get_option("compare_launches"), m.hier.get_option("compare_device_bytes")) == (0, 0), "a new handle: it holds no buffer yet"
    vals = [[[m.level[l][k].get(f) for k in range(len(bl))] for l, bl in enumerate(fr.all_boxes(NX0, NY0, boxes))] for f in (lv.F_B, lv.F_PI)]
    assert_both_modes(m.hier, E, xs, 2, comps, vals, boxes, "after the regrid")
    assert m.hier.get_option("compare_device_bytes") > 0
    E.close(); m.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_norms_and_the_hierarchy_alone():
    from suhmo_amd import capi, level as lv, model
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT, DX0, STEP_MODEL, assert_same_state
    M, T = shmip_model(), shmip_model()                      # 64 x 32 base, three levels: the finest is level 2
    for G in (M, T):
        G.moulin_source(**MOULINS)
    E = lv.HipLevel(256, 128, DX0 / 4, DX0 / 4, sy.A3_BC, sy.A3_PHYS, max_box=64)
    E.set(lv.F_B, np.ones((128, 256)))
    strip = lv.HipLevel(256, 64, DX0 / 4, DX0 / 4, sy.A3_BC, sy.A3_PHYS, max_box=64, j0=0, ny_global=128)
    strip.set(lv.F_B, np.ones((64, 256)))
    norms, terms = np.full(16 * 3, -77.0), np.full(3 * 16 * 3, -77.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    F, D, CO, FI = capi.FLAT_FIELD, capi.FLAT_DIFF, capi.CMP_COMPOSITE, capi.CMP_FINEST
    ok = [(F, lv.F_B)]

    def call(H, exact, el, mode, comps, n=None, lt=None):
        return capi.lib().suhmo_hier_compare(H.h, exact.h if exact is not None else None, el, mode, len(comps) if n is None else n, capi.flat_comps(comps),
                                             dp(norms), lt, H.stream)
    cases = [(None, 2, CO, ok, None, None, -1),              # exact NULL
             (E, 3, CO, ok, None, None, -1),                 # its extents are those of level 2
             (E, 1, CO, ok, None, None, -1),                 # exact_level below the finest level
             (E, 2, 2, ok, None, None, -1), (E, 2, -1, ok, None, None, -1),      # an unknown mode
             (E, 2, FI, ok, None, dp(terms), -1),            # level_terms in FINEST
             (E, 2, CO, [(F, lv.F_ZS)], None, None, -1), (E, 2, FI, [(D, lv.F_B, lv.F_PW)], None, None, -1),      # a field exact does not hold
             (E, 2, CO, ok, 0, None, -1), (E, 2, CO, ok * 17, None, None, -1), (E, 2, CO, [(2, lv.F_B)], None, None, -1), (E, 2, FI, [(F, 33)], None, None, -1),
             (E, 2, CO, [(F, lv.F_QWX)], None, None, -1), (E, 2, CO, [(F, lv.F_COVER)], None, None, -1), (E, 2, FI, [(D, lv.F_B, lv.F_PHI2)], None, None, -1),
             (E, 25, FI, ok, None, None, -1),                # 64 << 25 leaves int
             (strip, 2, CO, ok, None, None, -5), (strip, 2, FI, ok, None, None, -5)]
    for exact, el, mode, comps, n, lt, want in cases:
        rc = call(M.hier, exact, el, mode, comps, n, lt)
        assert rc == want and capi.lib().suhmo_last_error(), (el, mode, comps, n, rc, capi.lib().suhmo_last_error())
    assert (M.hier.get_option("compare_launches"), M.hier.get_option("flatten_launches"), M.hier.get_option("compare_copies")) == (0, 0, 0), "nothing was launched"
    # rc -2: the scratch of the flatten cannot be had
    M.hier.set_option("flatten_fail_slot", 0)
    assert call(M.hier, E, 2, FI, ok) == -2
    M.hier.set_option("flatten_fail_slot", -1)
    # r > 64 on level 0: an 8 x 4 base against level 7
    small = lv.HipHier(8, 4, 1.0, 1.0, hl._NP, sy.A3_PHYS, [], max_box=64)
    small.level[0][0].set(lv.F_B, np.ones((4, 8)))
    big = lv.HipLevel(8 << 7, 4 << 7, 1.0 / 128, 1.0 / 128, hl._NP, sy.A3_PHYS, max_box=64)
    big.set(lv.F_B, np.ones((4 << 7, 8 << 7)))
    assert call(small, big, 7, CO, ok) == -1 and b"64" in capi.lib().suhmo_last_error()
    assert small.get_option("compare_launches") == 0
    # a rank strip and a hierarchy created with shadow = 1: rc -5
    S = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, j0=0, ny_global=64)
    W = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, options="shadow=1")
    for G in (S, W):
        for mode in (CO, FI):
            assert call(G.hier, E, 2, mode, ok) == -5 and b"not built" in capi.lib().suhmo_last_error()
    S.close(); W.close()
    assert (norms == -77.0).all() and (terms == -77.0).all(), "nothing was written"
    assert M.timestep(DT) == T.timestep(DT)
    assert_same_state(M, T)
    # ... and the calls the refusals were variations of go through (r = 128 in FINEST too)
    for mode in (CO, FI):
        capi.check(call(M.hier, E, 2, mode, ok))
        assert not (norms[:3] == -77.0).any() and (norms[3:] == -77.0).all()
        norms[:3] = -77.0
    capi.check(call(small, big, 7, FI, ok))
    assert same_bits(norms[:3], np.zeros(3))
    for G in (E, strip, big):
        G.close()
    M.close(); T.close()


# ------------------------------------------------------------------ 8. the tool
def test_the_convergence_tool_through_the_device_meets_the_reference_tables():
    """tools/convergence_channelized.py --device-compare: the hip leg of amr_moulin_error through suhmo_hier_compare reproduces the RHS_moulin
    column of the reference's 2- and 3-level tables to the 6e-5 the host loop is held to (tests/test_gpu_moulin.py), in the same five rows"""
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
            e = cc.amr_moulin_error(nx0, rects, "hip", device_compare=True)
            print(name, nx0, e, cc.amr_moulin_error(nx0, rects, "hip", device_compare=False), ref[nx0])
            assert abs(e - ref[nx0]) <= 6e-5 * ref[nx0], (name, nx0, e, ref[nx0])
            checked += 1
    assert checked == 5
