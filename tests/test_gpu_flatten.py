"""suhmo_hier_flatten (include/suhmo_hip.h, "FLATTEN"; suhmo_amd/csrc/suhmo_flatten.hip): a hierarchy interpolated onto the uniform grid of its
finest resolution, BITWISE against the numpy twin tests/flatten_ref.py over generated and hand-made layouts on the 32 x 16 base of
tests/hierlayouts.py, with the fields' own ghost rings loaded with other values; the launch and copy counts; that the call changes nothing; a
field no box holds; the hierarchy a regrid leaves; every refusal; the file of writePltPP and the input.hydro_pp workflow; level 0 alone."""
import ctypes as C
import os

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import flatten_ref as fr
from tests import hierlayouts as hl
from tests.test_gpu_snapshot import same_bits, stepped_model

pytestmark = pytest.mark.gpu
NX0, NY0 = hl.NX0, hl.NY0                                   # 32 x 16: the finest array is at most 512 x 256


def components():
    from suhmo_amd import capi, level as lv
    return [(capi.FLAT_FIELD, lv.F_B), (capi.FLAT_DIFF, lv.F_PI, lv.F_PW), (capi.FLAT_FIELD, lv.F_PHI), (capi.FLAT_FIELD, lv.F_MASK)]


def load_random(M, key, seed=fr.DATA_SEED):
    """B, Pi, Pw and the mask (+-1) of every box <- flatten_ref.random_box: random valid cells and a ghost ring of OTHER random values, which a
    flatten must not read.  -> values[q][l][k]: the valid cells of component q of components(), the head as the device holds it"""
    from suhmo_amd import level as lv
    bxs = fr.all_boxes(M.level[0][0].nx, M.level[0][0].ny, M.hier.boxes)
    vals = [[[None] * len(bl) for bl in bxs] for _ in range(4)]
    for l, bl in enumerate(bxs):
        for k, b in enumerate(bl):
            L = M.level[l][k]
            a = {f: fr.random_box(seed, key, l, k, q, b, "mask" if f == lv.F_MASK else "uniform") for q, f in enumerate((lv.F_B, lv.F_PI, lv.F_PW, lv.F_MASK))}
            for f, x in a.items():
                L.set(f, x, ghosted=True)
            inner = lambda f: a[f][1:-1, 1:-1]
            vals[0][l][k], vals[1][l][k], vals[2][l][k], vals[3][l][k] = inner(lv.F_B), inner(lv.F_PI) - inner(lv.F_PW), L.get(lv.F_PHI), inner(lv.F_MASK)
    return vals


def ghost_kinds(nx0, ny0, periodic, boxes):
    """per level l >= 1: (it has coarse-fine ghost cells, it has fine-fine ghost cells) -- a ghost cell inside the domain after the wrap is the
    one or the other, as a box of the level holds it or not"""
    out = []
    for l, bl in enumerate(boxes, start=1):
        n = (nx0 << l, ny0 << l)
        m = hl.level_mask(n[0], n[1], bl)
        cf = ff = False
        for lo0, lo1, hi0, hi1 in bl:
            for j in range(lo1 - 1, hi1 + 2):
                for i in range(lo0 - 1, hi0 + 2):
                    if lo0 <= i <= hi0 and lo1 <= j <= hi1:
                        continue
                    w = hl._wrapped((i, j), n, periodic)
                    if w is not None:
                        cf, ff = cf or not m[w[1], w[0]], ff or bool(m[w[1], w[0]])
        out.append((cf, ff))
    return out


def launches_of(nx0, ny0, periodic, boxes, ncomp):
    """the count the header states"""
    nlev = 1 + len(boxes)
    return 2 * nlev + sum(ncomp * cf + (ncomp + 1) // 2 * ff for cf, ff in ghost_kinds(nx0, ny0, periodic, boxes))


def assert_equals_twin(H, bc, boxes, comps, vals, max_level, what, nx0=NX0, ny0=NY0):
    n_l, n_c = H.get_option("flatten_launches"), H.get_option("flatten_copies")
    dev = H.flatten(comps, max_level)
    assert H.get_option("flatten_launches") - n_l == launches_of(nx0, ny0, bc["periodic"], boxes, len(comps)), (what, "launches")
    assert H.get_option("flatten_copies") - n_c == 1, (what, "one copy")
    assert dev.shape == (len(comps), ny0 << max_level, nx0 << max_level)
    for q in range(len(comps)):
        ref, _ = fr.flatten(nx0, ny0, bc["periodic"], boxes, vals[q], max_level)
        bad = np.argwhere(dev[q].view(np.uint64) != ref.view(np.uint64))
        assert bad.size == 0, (what, "component", q, "max_level", max_level, "first at (j, i) =", tuple(bad[0]), len(bad), dev[q][tuple(bad[0])], ref[tuple(bad[0])])
    return dev


# ------------------------------------------------------------------ 1. bitwise against the twin, 2. the counters
@pytest.mark.parametrize("key", [k for _, k in fr.CASES], ids=[n for n, _ in fr.CASES])
def test_bitwise_against_the_twin(key):
    """seeds 0 .. 11: 2, 3 and 4 levels, all four periodicities; span-x: boxes over the whole width of a non-periodic domain; tiny-boxes: boxes 2
    cells wide.  max_level = the finest level (its boxes are copied, every other level interpolated) and the finest level + 1.  The head is
    the one a time step left (on either of its canvases), B, Pi - Pw and the mask are random with foreign ghost rings"""
    bc, boxes = fr.case(key)
    M = stepped_model(bc, boxes)
    vals = load_random(M, key)
    top = len(boxes)
    for ml in (top, top + 1):
        assert_equals_twin(M.hier, bc, boxes, components(), vals, ml, key)
    M.close()


def test_sizes_alone_launch_nothing():
    from suhmo_amd import capi
    bc, boxes = fr.case(5)
    M = stepped_model(bc, boxes)
    H = M.hier
    dims = (C.c_long * 2)(-1, -1)
    n_l, n_c = H.get_option("flatten_launches"), H.get_option("flatten_copies")
    capi.check(capi.lib().suhmo_hier_flatten(H.h, len(boxes) + 2, 4, capi.flat_comps(components()), dims, None, H.stream))
    assert (dims[0], dims[1]) == (NX0 << (len(boxes) + 2), NY0 << (len(boxes) + 2))
    assert (H.get_option("flatten_launches"), H.get_option("flatten_copies")) == (n_l, n_c) == (0, 0)
    M.close()


# ------------------------------------------------------------------ 3. read-only
def test_a_snapshot_before_and_after_is_the_same():
    from suhmo_amd import plotfile
    bc, boxes = fr.case(9)
    M = stepped_model(bc, boxes)
    load_random(M, 9)
    before = M.hier.snapshot(plotfile.SNAP, 1)[2].copy()
    assert len(plotfile.SNAP) == 13
    M.hier.flatten(components(), len(boxes) + 1)
    M.hier.flatten(components()[:2], len(boxes))
    after = M.hier.snapshot(plotfile.SNAP, 1)[2]
    assert same_bits(before, after)
    M.close()


def test_a_model_flattened_between_its_steps_stays_its_twin():
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT, assert_same_state
    A, B = shmip_model(), shmip_model()
    for G in (A, B):
        G.moulin_source(**MOULINS)
    A.interp_finest()                                        # before the first step: Pw is not held yet
    for n in range(3):
        assert A.timestep(DT) == B.timestep(DT)
        out = A.interp_finest(2 + n % 2)
        assert out["gapHeight"].shape == out["N"].shape == (32 << (2 + n % 2), 64 << (2 + n % 2)) and np.isfinite(out["N"]).all()
    assert_same_state(A, B)
    A.close(); B.close()


# ------------------------------------------------------------------ 4. a field no box holds
def test_an_unheld_field_is_zero_and_allocates_only_scratch():
    from suhmo_amd import capi, level as lv
    bc, boxes = fr.case("tiny-boxes")
    M = stepped_model(bc, boxes)
    H = M.hier
    UNHELD = lv.F_ZS                                         # nobody has loaded a surface height
    held = lambda: [H.get_option("canvas_bytes_level_%d" % l) for l in range(1, H.nlev)]
    h0 = held()
    H.flatten([(capi.FLAT_FIELD, lv.F_B)], 3)
    h1 = held()
    one = [b - a for a, b in zip(h0, h1)]                    # one scratch canvas per box
    assert all(g > 0 for g in one)
    H.flatten([(capi.FLAT_FIELD, lv.F_B)], 2)
    assert held() == h1, "the scratch is allocated on the first call only"
    out = H.flatten([(capi.FLAT_FIELD, lv.F_B), (capi.FLAT_FIELD, UNHELD), (capi.FLAT_DIFF, UNHELD, UNHELD)], 3)
    assert not out[1].any() and not out[2].any() and out[0].any()
    assert [b - a for a, b in zip(h1, held())] == [2 * g for g in one], "two more scratch canvases per box, nothing for the field"
    h3 = held()
    H.flatten([(capi.FLAT_FIELD, UNHELD), (capi.FLAT_DIFF, lv.F_B, UNHELD)], 2)
    assert held() == h3
    with pytest.raises(capi.SuhmoError) as e:                # ... on level 0 neither: the recharge still finds no surface height
        M.time_varying_recharge(7.5, 0.0)
    assert "rc=-1" in str(e.value) and "level 0, box 0" in str(e.value)
    M.close()


def test_a_failed_scratch_allocation_leaves_the_hierarchy_usable():
    """option flatten_fail_slot makes the allocation of one scratch slot of the finest level fail as an exhausted device would: rc -2, what the
    call took of that level is given back, and the level's device table still lists exactly the slots that exist -- on the first call ever
    (there is no table yet) and on a call that grows the scratch (the levels below have grown already)"""
    from suhmo_amd import capi
    bc, boxes = fr.case(7)
    top = len(boxes)
    for first in (True, False):
        M = stepped_model(bc, boxes)
        H = M.hier
        vals = load_random(M, 7)
        finest = lambda: H.get_option("canvas_bytes_level_%d" % top)
        base = finest()
        if not first:
            assert_equals_twin(H, bc, boxes, components()[:1], vals[:1], top + 1, "one slot")
        H.set_option("flatten_fail_slot", 1)
        for _ in range(2):
            with pytest.raises(capi.SuhmoError) as e:
                H.flatten(components(), top + 1)
            assert "rc=-2" in str(e.value) and "scratch of level %d" % top in str(e.value)
            assert_equals_twin(H, bc, boxes, components()[:1], vals[:1], top + 1, ("after the failure", first))
        slot = finest() - base                               # the finest level holds one slot, whatever the failed calls took and gave back
        assert slot > 0
        H.set_option("flatten_fail_slot", 3)
        with pytest.raises(capi.SuhmoError):
            H.flatten(components(), top)
        assert finest() == base + slot, "the two slots taken before the failing one were given back"
        assert_equals_twin(H, bc, boxes, components()[:3], vals[:3], top, ("three slots can be had", first))
        assert finest() == base + 3 * slot
        H.set_option("flatten_fail_slot", -1)
        for ml in (top, top + 1):
            assert_equals_twin(H, bc, boxes, components(), vals, ml, ("switch off", first))
        assert finest() == base + 4 * slot
        M.close()


def test_release_gives_the_device_memory_back():
    from suhmo_amd import capi, level as lv
    bc, boxes = fr.case(10)
    M = stepped_model(bc, boxes)
    H = M.hier
    vals = load_random(M, 10)
    held = lambda: [H.get_option("canvas_bytes_level_%d" % l) for l in range(1, H.nlev)]
    h0 = held()
    assert H.get_option("flatten_device_bytes") == 0
    assert_equals_twin(H, bc, boxes, components(), vals, len(boxes) + 1, "before")
    assert H.get_option("flatten_device_bytes") >= 4 * 8 * (NX0 * NY0 << 2 * (len(boxes) + 1)) and held() != h0
    H.set_option("flatten_release", 1)
    assert H.get_option("flatten_device_bytes") == 0 and held() == h0
    assert_equals_twin(H, bc, boxes, components(), vals, len(boxes), "after the release")
    M.close()


# ------------------------------------------------------------------ 5. after a regrid
def test_after_a_regrid_the_new_boxes_are_flattened():
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
    m.hier.flatten(comps, 2)                                 # the old hierarchy has its scratch
    boxes, same = m.tag_and_regrid([dict(name="GapHeight", vmin=0.5, vmax=10.0, grow=1)], dict(fill_ratio=0.7, block_factor=2, max_box_size=32, nesting_radius=2))
    assert not same and boxes != old and m.hier.boxes == boxes
    assert m.hier.get_option("flatten_launches") == 0, "a new handle"
    vals = [[[m.level[l][k].get(f) for k in range(len(bl))] for l, bl in enumerate(fr.all_boxes(NX0, NY0, boxes))] for f in (lv.F_B, lv.F_PI)]
    for ml in (1, 2):
        assert_equals_twin(m.hier, hl._NP, boxes, comps, vals, ml, "after the regrid")
    m.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_destination_and_the_hierarchy_alone():
    from suhmo_amd import capi, level as lv, model
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT, DX0, STEP_MODEL, assert_same_state
    M, T = shmip_model(), shmip_model()                      # 64 x 32 base, three levels
    for G in (M, T):
        G.moulin_source(**MOULINS)
    dst = np.full(2 * 256 * 128, -77.0)
    dims = (C.c_long * 2)()
    dp = dst.ctypes.data_as(C.POINTER(C.c_double))
    F, D = capi.FLAT_FIELD, capi.FLAT_DIFF
    ok = [(F, lv.F_B)]
    cases = [(0, ok, 2, -1), (17, ok * 17, 2, -1), (1, [(2, lv.F_B)], 2, -1), (1, [(-1, lv.F_B)], 2, -1), (1, [(F, -1)], 2, -1), (1, [(F, 33)], 2, -1),
             (1, [(F, lv.F_QWX)], 2, -1), (2, ok + [(F, lv.F_BY)], 2, -1), (1, [(D, lv.F_PI, lv.F_DCX)], 2, -1), (1, [(D, lv.F_PI, 40)], 2, -1),
             (1, [(F, lv.F_COVER)], 2, -1), (1, [(F, lv.F_PHI2)], 2, -1), (1, [(D, lv.F_B, lv.F_PHI2)], 2, -1), (1, ok, 1, -1), (1, ok, -1, -1),
             (1, ok, 25, -1),                                # 64 << 25 = 2^31 leaves int
             (1, ok, 31, -1), (1, ok, 64, -1),
             (1, ok, 20, -2)]                                # 2^26 x 2^25 doubles: no device holds them
    for ncomp, comps, ml, want in cases:
        rc = capi.lib().suhmo_hier_flatten(M.hier.h, ml, ncomp, capi.flat_comps(comps), dims, dp, M.hier.stream)
        assert rc == want and capi.lib().suhmo_last_error(), (ncomp, comps, ml, rc)
        assert M.hier.get_option("flatten_launches") == 0, "nothing was launched"
        assert M.timestep(DT) == T.timestep(DT), (ncomp, comps, ml)
    assert_same_state(M, T)
    # a rank strip and a hierarchy created with shadow = 1: rc -5
    S = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, j0=0, ny_global=64)
    W = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, options="shadow=1")
    for G in (S, W):
        rc = capi.lib().suhmo_hier_flatten(G.hier.h, 1, 1, capi.flat_comps(ok), dims, dp, G.hier.stream)
        assert rc == -5 and "not built" in capi.lib().suhmo_last_error().decode()
    S.close(); W.close()
    assert (dst == -77.0).all(), "nothing was written"
    # ... and the call the refusals were variations of goes through
    capi.check(capi.lib().suhmo_hier_flatten(M.hier.h, 2, 1, capi.flat_comps(ok), dims, dp, M.hier.stream))
    assert (dims[0], dims[1]) == (256, 128) and not (dst[:256 * 128] == -77.0).any() and (dst[256 * 128:] == -77.0).all()
    M.close(); T.close()


# ------------------------------------------------------------------ 7. the file, the tool
@pytest.fixture(scope="module")
def io():
    from suhmo_amd import checkpoint, plotfile
    if checkpoint.hdf5_prefix() is None and not os.path.exists(checkpoint.LIB_PATH):
        pytest.skip("no HDF5 C library on this box: the (optional) checkpoint / plot file library cannot be built")
    plotfile.build()
    return checkpoint, plotfile


def test_the_pp_file_and_the_restart_workflow(io, tmp_path):
    import importlib.util
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT, OLD
    checkpoint, plotfile = io
    M = shmip_model()
    M.moulin_source(**MOULINS)
    for _ in range(2):
        M.timestep(DT)
    path = str(tmp_path / plotfile.pp_name("plot", M.cur_step))
    a = plotfile.write_pp(path, M, 2 * DT, max_level=3)
    want = M.interp_finest(3)
    assert same_bits(a[0], want["gapHeight"]) and same_bits(a[1], want["N"])
    names, levels = plotfile.read_levels(path)
    assert names == ["gapHeight", "N"] and len(levels) == 1
    v = levels[0]
    assert v["domain"] == (0, 0, 511, 255) and v["boxes"] == [(0, 0, 511, 255)] and v["ghost"] == 0 and v["time"] == 2 * DT
    assert v["dx"] == M.level[0][0].dx / 8 and v["dy"] == M.level[0][0].dy / 8
    assert same_bits(v["fabs"][0], a)
    # the input.hydro_pp workflow: restart from a checkpoint of this state, one step, the file -- against the model stepped on
    chk = str(tmp_path / "chk000002.2d.hdf5")
    checkpoint.write(chk, M, 2 * DT, DT)
    spec = importlib.util.spec_from_file_location("interp_finest_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "interp_finest.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    p2, b, R = tool.interp_finest(chk, lambda boxes, level0: shmip_model(boxes), 3, DT, steps=1, prefix=str(tmp_path / "pp"),
                                  before_step=lambda m: m.moulin_source(**MOULINS))
    assert R.hier.boxes == [[tuple(x) for x in bl] for bl in OLD] and R.cur_step == 3 and p2 == str(tmp_path / "pp") + "Custom000003.2d.hdf5"
    M.timestep(DT)
    want = M.interp_finest(3)
    assert same_bits(b[0], want["gapHeight"]) and same_bits(b[1], want["N"])
    names2, levels2 = plotfile.read_levels(p2)
    assert names2 == names and same_bits(levels2[0]["fabs"][0], b) and levels2[0]["time"] == 2 * DT + DT
    M.close(); R.close()


# ------------------------------------------------------------------ 8. level 0 alone
@pytest.mark.parametrize("per", ["np", "pxy"])
def test_level_0_alone(per):
    from suhmo_amd import capi, level as lv, model
    bc = {"np": hl._NP, "pxy": hl._PXY}[per]
    m = model.HipHierModel(NX0, NY0, 1.0, 1.0, bc, hl.ADV_PHYS, sy.A3_MODEL, [], max_box=16)
    a = fr.random_box(3, per, 0, 0, 0, (0, 0, NX0 - 1, NY0 - 1))
    m.level[0][0].set(lv.F_B, a, ghosted=True)
    vals = [[[a[1:-1, 1:-1]]]]
    for ml in (0, 2):
        assert_equals_twin(m.hier, bc, [], [(capi.FLAT_FIELD, lv.F_B)], vals, ml, ("level 0 alone", per))
    m.close()
