"""suhmo_hier_regrid (include/suhmo_hip.h, "REGRID: FIELD TRANSFER"): a hierarchy's fields moved onto new box lists on the device, BITWISE
against the numpy twin tests/regrid_ref.py -- valid cells, the ghost ring kind by kind (tests/ghostring.py) and the ring's corners -- with the
old hierarchy's ghost rings poisoned with NaN first.  Then what a caller relies on: unlisted fields read as in a new hierarchy, nothing of
the old hierarchy survives in the time step (gap-height hierarchy, mask knowledge, plans), tag_and_regrid, and the refusals."""
import re

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import ghostring as gr
from tests import hierlayouts as hl
from tests import regrid_ref as rr

pytestmark = pytest.mark.gpu
NX0, NY0 = hl.NX0, hl.NY0                                   # 32 x 16
PER = {"np": hl._NP, "px": hl._PX, "py": hl._PY, "pxy": hl._PXY}


def field_ids():
    from suhmo_amd import level as lv
    return dict(head=lv.F_PHI, B=lv.F_B, Pi=lv.F_PI, zb=lv.F_ZB, mask=lv.F_MASK, mR=lv.F_MR, Pw=lv.F_PW, zs=lv.F_ZS)


def make(bc, boxes, nx0=NX0, ny0=NY0):
    from suhmo_amd import model
    return model.HipHierModel(nx0, ny0, 1.0, 1.0, bc, hl.ADV_PHYS, sy.A3_MODEL, boxes, max_box=16)


def load_random(m, names, seed, extra=()):
    """every box of every level gets random data in the named fields; the ghost rings of the levels >= 1 are NaN (the transfer must not
    read them).  -> {(l, k, name): the ghosted array loaded}"""
    ids = dict(field_ids(), **dict(extra))
    data = {}
    for l, bl in enumerate(m.level):
        for k, L in enumerate(bl):
            for q, nm in enumerate(names):
                rng = np.random.default_rng([seed, l, k, q])
                a = rng.uniform(-1.0, 3.0, size=(L.ny + 2, L.nx + 2))
                if l > 0:
                    a[0, :] = a[-1, :] = a[:, 0] = a[:, -1] = np.nan
                L.set(ids[nm], a, ghosted=True)
                data[(l, k, nm)] = a
    return data


def twin(periodic, old_boxes, new_boxes, data, nm, nx0=NX0, ny0=NY0):
    old = [[data[(l, k, nm)] for k in range(len(bl))] for l, bl in enumerate(old_boxes, start=1)]
    return rr.regrid(nx0, ny0, periodic, old_boxes, new_boxes, old, data[(0, 0, nm)], rr.RULES[nm])


def check_against_twin(m, bc, old_boxes, new_boxes, data, names, nx0=NX0, ny0=NY0):
    ids = field_ids()
    seen = dict.fromkeys(gr.KINDS, 0)
    for nm in names:
        ref = twin(bc["periodic"], old_boxes, new_boxes, data, nm, nx0, ny0)
        assert np.array_equal(m.level[0][0].get(ids[nm], ghosted=True), data[(0, 0, nm)]), ("level 0 is carried over unchanged", nm)
        for l, bl in enumerate(new_boxes, start=1):
            for k, b in enumerate(bl):
                dev = m.level[l][k].get(ids[nm], ghosted=True)
                what = (nm, "level", l, "box", k, b)
                bad = np.argwhere(dev[1:-1, 1:-1] != ref[l - 1][k][1:-1, 1:-1])
                assert bad.size == 0, (what, "valid cells differ, first at (j, i) =", tuple(bad[0]), len(bad))
                s = gr.ring_equal(ref[l - 1][k], dev, b, (nx0 << l, ny0 << l), bc["periodic"], bl, what=str(what))
                for kd, n in s.items():
                    seen[kd] += n
                assert np.array_equal(dev, ref[l - 1][k]), (what, "corner ghost cells differ")
    return seen


def regrid_and_check(bc, old_boxes, new_boxes, names=("head", "B", "Pi"), seed=1, fields="names"):
    assert hl.valid(NX0, NY0, bc["periodic"], old_boxes) and hl.valid(NX0, NY0, bc["periodic"], new_boxes)
    m = make(bc, old_boxes)
    try:
        data = load_random(m, names, seed)
        m.regrid(new_boxes, fields=list(names) if fields == "names" else fields)
        assert m.hier.boxes == [[tuple(b) for b in bl] for bl in new_boxes] and m.hier.nlev == 1 + len(new_boxes)
        assert len(m.level) == 1 + len(new_boxes)
        return check_against_twin(m, bc, old_boxes, new_boxes, data, names), m, data
    except BaseException:
        m.close()
        raise


ALL = ("head", "B", "Pi", "zb", "mask", "mR", "Pw", "zs")
TWO = [[(8, 4, 23, 15), (24, 4, 39, 15)]]


def test_same_boxes_in_and_out_leave_every_listed_field_unchanged():
    seen, m, data = regrid_and_check(hl._NP, TWO, TWO, names=ALL)
    ids = field_ids()
    for k in range(2):
        for nm in ALL:
            assert np.array_equal(m.level[1][k].get(ids[nm]), data[(1, k, nm)][1:-1, 1:-1]), (k, nm)
    assert seen["fine-fine"] > 0 and seen["coarse-fine"] > 0
    m.close()


def test_disjoint_new_level_is_pure_interpolation():
    new = [[(40, 16, 55, 27)]]
    seen, m, data = regrid_and_check(hl._NP, [[(8, 4, 23, 15)]], new)
    pure = rr.regrid(NX0, NY0, (0, 0), [], new, [], data[(0, 0, "B")], "copy")
    assert np.array_equal(m.level[1][0].get(field_ids()["B"], ghosted=True), pure[0][0])
    m.close()


def test_new_box_straddling_two_old_boxes_and_uncovered_ground():
    seen, m, data = regrid_and_check(hl._NP, TWO, [[(16, 8, 47, 23)]])
    dev = m.level[1][0].get(field_ids()["B"])
    # cells (16..23, 8..15) came from old box 0, (24..39, 8..15) from old box 1, the rest is new ground
    assert np.array_equal(dev[0:8, 0:8], data[(1, 0, "B")][1:-1, 1:-1][4:12, 8:16])
    assert np.array_equal(dev[0:8, 8:24], data[(1, 1, "B")][1:-1, 1:-1][4:12, 0:16])
    m.close()


THREE_OLD = [[(8, 4, 39, 27)], [(24, 12, 55, 43)]]
THREE_NEW = [[(16, 8, 55, 27)], [(48, 24, 95, 47)], [(104, 56, 167, 87)]]


def test_three_levels_read_the_new_level_below():
    """the new level 2 lies partly over level-1 cells that were themselves just interpolated (columns 40..55 of level 1 are new ground), and
    level 3 is new altogether: wrong if the levels are done out of order or read the old level l - 1"""
    seen, m, data = regrid_and_check(hl._NP, THREE_OLD, THREE_NEW)
    m.close()


@pytest.mark.parametrize("case", ["two-to-three", "three-to-two", "to-base-only", "from-base-only"])
def test_added_and_dropped_levels(case):
    old, new = {"two-to-three": (THREE_OLD[:1], THREE_NEW), "three-to-two": (THREE_NEW, THREE_OLD[:1]), "to-base-only": (THREE_NEW, []),
                "from-base-only": ([], THREE_OLD)}[case]
    seen, m, data = regrid_and_check(hl._PY, old, new)
    assert m.hier.nlev == 1 + len(new)
    m.close()


# old and new as tests/hierlayouts.generate draws them (seeds s and s + 1000: the same periodicity, another number of levels), every fourth
# new layout a re-cutting of the old unions; then, per periodicity, a new level 1 with a box against a side, one in a domain corner and
# one across the x side from it
SWEEP = [("seed-%d" % s, s) for s in range(20)] + [("sides-" + p, p) for p in PER]
AT_DOMAIN = [[(0, 0, 15, 11), (48, 20, 63, 31), (0, 12, 7, 19), (48, 0, 63, 5)]]


def sweep_pair(key):
    if isinstance(key, str):
        return PER[key], [[(8, 4, 39, 27)]], AT_DOMAIN
    bc, old = hl.generate(key)
    bc2, new = hl.generate(key + 1000)
    assert bc["periodic"] == bc2["periodic"], "the two draws of a pair differ in periodicity: the pair would have to be skipped"
    if key % 4 == 3:
        new = hl.recut(key, old)
    return bc, old, new


def test_the_sweep_has_its_pairs():
    pairs = [sweep_pair(k) for _, k in SWEEP]
    assert len(pairs) == 24
    assert {tuple(bc["periodic"]) for bc, _, _ in pairs} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert any(len(o) != len(n) for _, o, n in pairs) and any(o != n and len(o) == len(n) for _, o, n in pairs)


@pytest.mark.parametrize("name,key", SWEEP, ids=[n for n, _ in SWEEP])
def test_seeded_sweep_over_generated_layouts(name, key):
    bc, old, new = sweep_pair(key)
    old = [[tuple(b) for b in bl] for bl in old]
    new = [[tuple(b) for b in bl] for bl in new]
    seen, m, data = regrid_and_check(bc, old, new, seed=7 + (key if isinstance(key, int) else 0))
    m.close()
    if isinstance(key, str):
        want = {"np": ("domain",), "px": ("domain", "periodic"), "py": ("domain", "periodic"), "pxy": ("periodic",)}[key]
        for kd in want:
            assert seen[kd] > 0, (key, seen)


def test_a_field_that_is_not_listed_reads_as_in_a_new_hierarchy():
    from suhmo_amd import level as lv
    new = [[(16, 8, 47, 23)]]
    m = make(hl._NP, TWO)
    data = load_random(m, ("head", "B", "Pi"), 3)
    m.regrid(new, fields=["B"])
    check_against_twin(m, hl._NP, TWO, new, data, ("B",))
    fresh = make(hl._NP, new)
    for fid in (lv.F_PHI, lv.F_PI, lv.F_RE):
        assert np.array_equal(m.level[1][0].get(fid, ghosted=True), fresh.level[1][0].get(fid, ghosted=True)), fid
        assert not m.level[1][0].get(fid, ghosted=True).any()
    assert np.array_equal(m.level[0][0].get(lv.F_PHI, ghosted=True), data[(0, 0, "head")])
    m.close(); fresh.close()


def test_the_default_list_moves_exactly_the_eight_fields():
    from suhmo_amd import level as lv
    new = [[(16, 8, 47, 23)]]
    others = dict(Re=lv.F_RE, cd=lv.F_CD, msrc=lv.F_MSRC, hlag=lv.F_HLAG)
    m = make(hl._PX, TWO)
    data = load_random(m, ALL + tuple(others), 4, extra=others.items())
    m.regrid(new)
    check_against_twin(m, hl._PX, TWO, new, data, ALL)
    for nm, fid in others.items():
        assert not m.level[1][0].get(fid, ghosted=True).any(), nm
    m.close()


# ---- the time step after a regrid
OLD_S = ([(32, 16, 63, 47), (64, 16, 95, 31), (64, 32, 95, 47)], [(80, 44, 119, 83), (120, 44, 159, 83)])
NEW_S = ([(24, 12, 71, 43), (72, 20, 103, 51)], [(64, 36, 127, 75)])
MOULINS = dict(positions=[(30.0e3, 9.0e3), (42.0e3, 5.5e3), (8.0e3, 4.0e3)], sigma=[900.0, 700.0, 800.0], flux=[8.0, 5.0, 3.0])
STEP_MODEL = dict(sy.A3_MODEL, diffFactor=1.0, use_moulin_source=1, distributed_input=7.93e-11)


def shmip_model(boxes, load=True):
    from suhmo_amd import model
    sts = sy.shmip_amrm_states(64, 32, boxes, rough=0.5)
    G = model.HipHierModel(64, 32, sts[0][0]["dx"], sts[0][0]["dy"], sy.A3_BC, sy.A3_PHYS, STEP_MODEL, boxes, max_box=16)
    if load:
        G.set_states(sts)
    return G


def step(G, implicit):
    from suhmo_amd import model
    G._mp = model.model_params(dict(STEP_MODEL, use_impl_diff=int(implicit)))
    return G.timestep(STEP_MODEL["dt"])


def test_no_stale_state_after_a_regrid():
    """two steps on the old grids (one of them with the implicit gap-height solve, so that its second hierarchy exists), a regrid, then two steps
    -- against a NEW model on the new boxes loaded with the transferred fields: every field, ghosted, and the Picard and V-cycle counts equal.
    A gap-height hierarchy on the old boxes, a mask report or a plan that survived would show here"""
    from suhmo_amd import level as lv
    assert hl.valid(64, 32, sy.A3_BC["periodic"], [list(b) for b in OLD_S]) and hl.valid(64, 32, sy.A3_BC["periodic"], [list(b) for b in NEW_S])
    ids = field_ids()
    G = shmip_model(OLD_S)
    G.moulin_source(**MOULINS)
    step(G, False); step(G, True)
    G.regrid([list(b) for b in NEW_S])
    F = shmip_model(NEW_S, load=False)
    for l, bl in enumerate(G.level):
        for k, L in enumerate(bl):
            F.level[l][k].set(lv.F_ACOEF, np.zeros((L.ny, L.nx)))
            for nm, fid in ids.items():
                F.level[l][k].set(fid, L.get(fid, ghosted=True), ghosted=True)
    F.cur_step = G.cur_step
    ig, if_ = G.moulin_source(**MOULINS), F.moulin_source(**MOULINS)
    assert np.array_equal(ig, if_)
    for n, implicit in enumerate((False, True)):
        cg, cf = step(G, implicit), step(F, implicit)
        assert cg == cf, ("Picard iterations, V-cycles", n, cg, cf)
        for l, bl in enumerate(G.level):
            for k in range(len(bl)):
                for nm in G.FIELDS:
                    a, b = G.get(l, k, nm, ghosted=True), F.get(l, k, nm, ghosted=True)
                    assert np.array_equal(a, b, equal_nan=True), ("step", n, "level", l, "box", k, nm)
    G.close(); F.close()


def test_tag_and_regrid_follows_the_tagged_field():
    from suhmo_amd import level as lv
    old = [[(8, 4, 23, 15)]]
    m = make(hl._NP, old)
    load_random(m, ("head", "Pi"), 9)
    b0 = np.zeros((NY0 + 2, NX0 + 2))
    b0[1 + 6:1 + 10, 1 + 20:1 + 24] = 1.0                                  # level-0 cells (20..23, 6..9): where the channel now is
    m.level[0][0].set(lv.F_B, b0, ghosted=True)
    m.level[1][0].set(lv.F_B, np.zeros((14, 18)), ghosted=True)
    specs = [dict(name="GapHeight", vmin=0.5, vmax=10.0, grow=1)]
    params = dict(fill_ratio=0.7, block_factor=2, max_box_size=32, nesting_radius=2)
    zero_b = lambda l, k, b: {"B": np.zeros((b[3] - b[1] + 3, b[2] - b[0] + 3))}
    boxes, same = m.tag_and_regrid(specs, params, reload=zero_b)
    assert not same and len(boxes) == 1 and m.hier.boxes == boxes and boxes != old
    cover = hl.level_mask(2 * NX0, 2 * NY0, boxes[0])
    assert cover[2 * 5:2 * 11, 2 * 19:2 * 25].all() and not cover[4:16, 8:24].any()      # the grown tags are covered, the old place is not
    for k, b in enumerate(boxes[0]):
        assert not m.level[1][k].get(lv.F_B, ghosted=True).any()                          # reload went over the transferred values
    h, views = m.hier.h.value, [v for bl in m.level for v in bl]
    boxes2, same2 = m.tag_and_regrid(specs, params, reload=zero_b)
    assert same2 and boxes2 == boxes
    assert m.hier.h.value == h and all(a is b for a, b in zip(views, [v for bl in m.level for v in bl]))
    m.close()


def _rc(e):
    return int(re.search(r"rc=(-?\d+)", str(e)).group(1))


@pytest.mark.parametrize("case", ["improperly-nested", "misaligned"])
def test_refused_lists_leave_the_old_hierarchy_usable(case):
    from suhmo_amd import capi, level as lv
    bad = {"improperly-nested": [[(24, 12, 71, 43)], [(40, 20, 71, 51), (0, 0, 7, 7)]], "misaligned": [[(25, 12, 72, 43)]]}[case]
    G = shmip_model(OLD_S)
    G.moulin_source(**MOULINS)
    step(G, False)
    h, before = G.hier.h.value, G.get(1, 0, "head", ghosted=True)
    with pytest.raises(capi.SuhmoError) as e:
        G.regrid(bad)
    with pytest.raises(capi.SuhmoError) as e2:           # suhmo_hier_create's own answer to the same lists
        lv.HipHier(64, 32, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS, bad)
    assert _rc(e.value) == _rc(e2.value) and str(e.value) == str(e2.value)
    assert G.hier.h.value == h and G.hier.boxes == [list(map(tuple, bl)) for bl in OLD_S]
    assert np.array_equal(G.get(1, 0, "head", ghosted=True), before, equal_nan=True)
    # ... and goes on as a model that never tried: the same step on both
    R = shmip_model(OLD_S)
    R.moulin_source(**MOULINS)
    step(R, False)
    assert step(G, True) == step(R, True)
    for l, bl in enumerate(G.level):
        for k in range(len(bl)):
            for nm in ("head", "B", "mR"):
                assert np.array_equal(G.get(l, k, nm), R.get(l, k, nm)), (l, k, nm)
    G.close(); R.close()


def test_a_strip_descriptor_is_refused():
    from suhmo_amd import capi, level as lv
    H = lv.HipHier(64, 32, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS, [[(32, 16, 63, 47)]], max_box=16, j0=0, ny_global=64)
    with pytest.raises(capi.SuhmoError) as e:
        H.regrid([[(40, 24, 71, 55)]])
    assert _rc(e.value) == -5 and "rank strips" in str(e.value)
    assert H.h is not None and H.boxes == [[(32, 16, 63, 47)]]
    H.close()
