"""The run of a hierarchy of box unions (include/suhmo_hip.h, "THE RUN OF A HIERARCHY" and "THE REST OF tagCells"): the seasonal recharge on
every box against the per-box level call, suhmo_hier_restrict_tags against the numpy twin tests/tagsubset_ref.py, and suhmo_hier_run against
the loop of the public calls it replaces -- every field of every box (ghosted), counts, rows, box lists and the regrid log, np.array_equal
throughout.

The run tests share one set-up (64 x 32 base, SqrtIBC state with roughness, suite-A physics with diffFactor 1 and three moulins).  Its grids are
made to order: tag variable A is Pi in a band that holds the level-0 columns 20 .. 27 (cap_level 0), variable B is Pi in the band of the level-1
columns 44 .. 51 (min_level = cap_level = 1), restricted by a level-1 subset box to the rows 16 .. 47.  Pi is a monotone function of x that the
time step never writes and that `reload` evaluates anew on every new box (the reference's initializePi), so the first regrid moves the
hierarchy from OLD to GEN and every later one finds GEN again: tests/test_hier_run_cpu.py's host call gives the same lists."""
import ctypes as C
import re

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import hierlayouts as hl
from tests import tagsubset_ref as ts

pytestmark = pytest.mark.gpu
NX0, NY0 = hl.NX0, hl.NY0                                   # 32 x 16


def _rc(e):
    return int(re.search(r"rc=(-?\d+)", str(e)).group(1))


def make(bc, boxes):
    from suhmo_amd import model
    return model.HipHierModel(NX0, NY0, 1.0, 1.0, bc, hl.ADV_PHYS, sy.A3_MODEL, boxes, max_box=16)


# ------------------------------------------------------------------ 1. recharge
def load_surface(m, seed):
    """random surface heights, ghost rings included: 0.0075 zs runs over (0, 15), so a temperature of 7.5 clamps about half the cells"""
    for l, bl in enumerate(m.level):
        for k, L in enumerate(bl):
            m.set_surface(l, k, np.random.default_rng([seed, l, k]).uniform(0.0, 2000.0, size=(L.ny + 2, L.nx + 2)))


@pytest.mark.parametrize("seed", range(12))
def test_recharge_equals_the_level_call_on_every_box(seed):
    from suhmo_amd import capi, level as lv
    bc, boxes = hl.generate(seed)                           # seed % 4: the periodicity; boxes on domain sides, unions of abutting boxes
    a, b = make(bc, boxes), make(bc, boxes)
    load_surface(a, seed); load_surface(b, seed)
    before = a.hier.get_option("recharge_launches")
    a.time_varying_recharge(7.5, 1.0e-9)
    assert a.hier.get_option("recharge_launches") - before == a.hier.nlev, "one launch per level"
    clamped = free = 0
    for l, bl in enumerate(b.level):
        for k, L in enumerate(bl):
            capi.check(capi.lib().suhmo_level_time_varying_recharge(L.h, 7.5, 1.0e-9, L.stream))
            got, want = a.level[l][k].get(lv.F_MSRC, ghosted=True), L.get(lv.F_MSRC, ghosted=True)
            assert np.array_equal(got, want), (seed, l, k)
            clamped += int((want == 1.0e-9).sum()); free += int((want > 1.0e-9).sum())
    assert clamped > 0 and free > 0, "the clamp is active in part of the cells"
    a.close(); b.close()


def test_recharge_refuses_a_box_without_surface_and_writes_nothing():
    from suhmo_amd import capi, level as lv
    bc, boxes = hl.generate(5)
    m = make(bc, boxes)
    load = {}
    last = (m.hier.nlev - 1, len(m.level[-1]) - 1)
    for l, bl in enumerate(m.level):
        for k, L in enumerate(bl):
            if (l, k) != last:
                m.set_surface(l, k, np.full((L.ny + 2, L.nx + 2), 900.0))
            load[(l, k)] = np.random.default_rng([3, l, k]).uniform(size=(L.ny + 2, L.nx + 2))
            L.set(lv.F_MSRC, load[(l, k)], ghosted=True)
    n = m.hier.get_option("recharge_launches")
    with pytest.raises(capi.SuhmoError) as e:
        m.time_varying_recharge(7.5, 0.0)
    assert _rc(e.value) == -1 and "level %d, box %d" % last in str(e.value)
    assert m.hier.get_option("recharge_launches") == n
    for (l, k), a in load.items():
        assert np.array_equal(m.level[l][k].get(lv.F_MSRC, ghosted=True), a), (l, k)
    m.close()


def test_recharge_and_restrict_refuse_a_strip_descriptor():
    from suhmo_amd import capi, model
    m = model.HipHierModel(64, 32, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS, sy.A3_MODEL, [[(32, 16, 63, 47)]], max_box=16, j0=0, ny_global=64)
    with pytest.raises(capi.SuhmoError) as e:
        m.time_varying_recharge(7.5, 0.0)
    assert _rc(e.value) == -5
    with pytest.raises(capi.SuhmoError) as e:
        m.restrict_tags(0, [(0, 0, 3, 3)])
    assert _rc(e.value) == -5
    m.close()


# ------------------------------------------------------------------ 2. restrict
RESTRICT_BOXES = [[(8, 4, 39, 27)], [(24, 12, 55, 43)]]
# per level, in cells of that level: boxes against the domain sides, two that overlap, one beyond the domain
SUBSETS = {0: [(0, 0, 7, 15), (4, 8, 19, 11), (28, 14, 35, 17)], 1: [(0, 0, 63, 5), (20, 4, 33, 19), (30, 10, 41, 31)]}


def tagged_model():
    from suhmo_amd import level as lv
    m = make(hl._NP, RESTRICT_BOXES)
    for l, bl in enumerate(m.level):
        for k, L in enumerate(bl):
            L.set(lv.F_B, np.random.default_rng([17, l, k]).uniform(size=(L.ny + 2, L.nx + 2)), ghosted=True)
    return m


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("level", [0, 1])
def test_restrict_against_the_twin(g, level):
    from suhmo_amd import capi
    m = tagged_model()
    tag = lambda: m.tag_cells(level, "B", 0.6, 2.0, grow=0, granularity=g)
    tag()
    full = m.tags(level)
    assert full.any() and not full.all()
    boxes = SUBSETS[level]
    assert ts.aligned(g, boxes)
    m.restrict_tags(level, [])                               # an empty list is a no-op
    assert np.array_equal(m.tags(level), full)
    m.restrict_tags(level, boxes)
    got, want = m.tags(level), ts.restrict(full, g, boxes)
    assert np.array_equal(got, want)
    assert want.any() and (want != full).any(), "the case restricts something and keeps something"
    bad = [(boxes[0][0], boxes[0][1], boxes[0][2] + 1, boxes[0][3])] if g == 2 else [(5, 3, 4, 6)]       # misaligned / empty
    with pytest.raises(capi.SuhmoError) as e:
        m.restrict_tags(level, boxes[1:] + bad)
    assert _rc(e.value) == -1
    assert np.array_equal(m.tags(level), want), "a refused list clears nothing"
    tag()                                                    # tagging after a restrict accumulates again
    assert np.array_equal(m.tags(level), full)
    m.restrict_tags(1 - level, boxes)                        # a level without a map: nothing to do
    assert m.tags(1 - level) is None
    m.close()


# ------------------------------------------------------------------ the set-up of the run tests
OLD = [[(32, 16, 63, 47), (64, 16, 95, 31), (64, 32, 95, 47)], [(80, 44, 119, 83), (120, 44, 159, 83)]]
GEN = [[(40, 0, 55, 31), (40, 32, 55, 63)], [(88, 32, 103, 63), (88, 64, 103, 95)]]
MOULINS = dict(positions=[(30.0e3, 9.0e3), (42.0e3, 5.5e3), (8.0e3, 4.0e3)], sigma=[900.0, 700.0, 800.0], flux=[8.0, 5.0, 3.0])
STEP_MODEL = dict(sy.A3_MODEL, diffFactor=1.0, use_moulin_source=1, distributed_input=7.93e-11)
DT = STEP_MODEL["dt"]
DX0 = 1.0e5 / 64
PARAMS = dict(fill_ratio=0.7, block_factor=2, max_box_size=32, nesting_radius=2)
SUBS = [[], [(0, 16, 127, 47)], []]


def _pi(x):
    return sy.RHO_I * sy.GRAV * (6.0 * (np.sqrt(x + 5000.0) - np.sqrt(5000.0)) + 1.0)


# thresholds at cell EDGES: the centres on either side are half a cell away from them
SPECS = [dict(name="Pi", vmin=_pi(20 * DX0), vmax=_pi(28 * DX0), grow=0, cap_level=0),
         dict(name="Pi", vmin=_pi(44 * DX0 / 2), vmax=_pi(52 * DX0 / 2), grow=0, min_level=1, cap_level=1)]
REGRID = dict(tag_specs=SPECS, params=PARAMS, subsets=SUBS, max_level=2)


def analytic(l, k, b):
    """initializePi / initializeBed / setup_iceMask on a new box"""
    st = sy.shmip_amrm_states(64, 32, [[]] * (l - 1) + [[b]], rough=0.5)[l][0]
    return {q: st[q] for q in ("Pi", "zb", "mask")}


def shmip_model(boxes=OLD, mdl=STEP_MODEL):
    from suhmo_amd import model
    sts = sy.shmip_amrm_states(64, 32, boxes, rough=0.5)
    G = model.HipHierModel(64, 32, sts[0][0]["dx"], sts[0][0]["dy"], sy.A3_BC, sy.A3_PHYS, mdl, boxes, max_box=16)
    G.set_states(sts)
    return G


def loop(M, n_steps, moulin_factor=None, ramp=None, T_K=None, background=None, diag_every=0, regrid_interval=0, skip_first=False, reload=analytic):
    """the per-call loop a run replaces, in the order the header states -> (counts, rows, log, steps that formed the moulin source)"""
    from suhmo_amd import capi, model
    due = model.regrid_steps(M.cur_step + 1, n_steps, regrid_interval, skip_first)
    counts, rows, log, formed = [], [], [], []
    for k in range(n_steps):
        c, changed = M.cur_step + 1, False
        if c in due:
            boxes, same = M.tag_and_regrid(reload=reload, **REGRID)
            changed = not same
            log.append(dict(cur_step=c, same=same, boxes_per_level=[len(bl) for bl in boxes]))
        if T_K is not None:
            M.time_varying_recharge(T_K[k], background[k])
        elif k == 0 or changed or np.float64(moulin_factor[k]).tobytes() != np.float64(moulin_factor[k - 1]).tobytes():
            M.moulin_source(time_factor=moulin_factor[k], **MOULINS)
            formed.append(k)
        if ramp is not None:
            M._mp.ramp = float(ramp[k])
        counts.append(M.timestep(DT))
        if diag_every and (k + 1) % diag_every == 0:
            base, out = M.level[0][0], np.zeros(6)
            capi.check(capi.lib().suhmo_level_postproc_temporal(base.h, C.byref(M._mp), out.ctypes.data_as(C.POINTER(C.c_double)), base.stream))
            rows.append(out)
    return counts, rows, log, formed


def assert_same_state(A, B, what=""):
    assert A.hier.boxes == B.hier.boxes and A.cur_step == B.cur_step, (what, A.hier.boxes, B.hier.boxes)
    for l, bl in enumerate(A.level):
        for k in range(len(bl)):
            for nm in A.FIELDS:
                a, b = A.get(l, k, nm, ghosted=True), B.get(l, k, nm, ghosted=True)
                assert np.array_equal(a, b, equal_nan=True), (what, "level", l, "box", k, nm)


def assert_same_counts(pi, nv, counts):
    assert [(int(a), int(b)) for a, b in zip(pi, nv)] == [tuple(c) for c in counts]


FACTOR = np.array([1.0, 1.0, 0.8, 0.8, 0.8, 1.1])          # changes before steps 2 and 5, repeats elsewhere
RAMP = np.array([0.25, 0.5, 0.75, 1.0, 1.0, 1.0])


# ------------------------------------------------------------------ 3. run against the per-call loop
def test_run_equals_the_per_call_loop():
    R, L = shmip_model(), shmip_model()
    counts, _, log, formed = loop(L, 6, moulin_factor=FACTOR, ramp=RAMP, regrid_interval=2)
    assert [e["cur_step"] for e in log] == [3, 5]
    assert any(not e["same"] for e in log) and any(e["same"] for e in log), ("a regrid that moves boxes and one that finds them again", log)
    assert L.hier.boxes == GEN
    assert formed == [0, 2, 5], "first step, the regrid that moved boxes (with a new factor), the new factor"
    calls = R.hier.get_option("moulin_source_calls")
    pi, nv, rows, rlog = R.run(6, DT, moulins=MOULINS, moulin_factor=FACTOR, ramp=RAMP, regrid_interval=2, reload=analytic, **REGRID)
    assert rlog == log
    assert list(np.nonzero(R.last_run["moulin_steps"])[0]) == formed
    assert R.hier.get_option("moulin_source_calls") - calls == len(formed), "the counter is carried over the regrid"
    assert R.last_run["steps_done"] == 6 and rows.shape == (0, 6)
    assert_same_counts(pi, nv, counts)
    assert_same_state(R, L)
    R.close(); L.close()


def test_moulin_source_after_a_moving_regrid_without_a_new_factor():
    """the factor repeats across the regrid that moves boxes: the source is formed there because of the regrid alone"""
    R, L = shmip_model(), shmip_model()
    f = np.array([1.0, 1.0, 1.0, 1.0])
    counts, _, log, formed = loop(L, 4, moulin_factor=f, regrid_interval=2)
    assert [e["same"] for e in log] == [False] and formed == [0, 2]
    pi, nv, _, rlog = R.run(4, DT, moulins=MOULINS, regrid_interval=2, reload=analytic, **REGRID)          # moulin_factor None = 1.0
    assert rlog == log and list(np.nonzero(R.last_run["moulin_steps"])[0]) == formed
    assert_same_counts(pi, nv, counts)
    assert_same_state(R, L)
    R.close(); L.close()


# ------------------------------------------------------------------ 4. seasonal run with rows
SEASON_MODEL = dict(STEP_MODEL, distributed_input=0.0, ramp=1.0)
T_K = np.array([8.0, 6.0, 9.0, 3.0])
BACKGROUND = np.array([7.93e-11, 7.93e-11, 1.0e-10, 1.0e-10])


def load_season_surface(M):
    for l, bl in enumerate(M.level):
        for k in range(len(bl)):
            M.set_surface(l, k, M.get(l, k, "Pi", ghosted=True) / (sy.RHO_I * sy.GRAV))       # the ice thickness: 0 .. 1500 m, 0.0075 zs up to 11


def test_seasonal_run_with_rows():
    from suhmo_amd import level as lv
    R, L = shmip_model(mdl=SEASON_MODEL), shmip_model(mdl=SEASON_MODEL)
    load_season_surface(R); load_season_surface(L)
    counts, rows, log, _ = loop(L, 4, T_K=T_K, background=BACKGROUND, diag_every=2, regrid_interval=2)
    assert [e["same"] for e in log] == [False]
    src = L.get(0, 0, "msrc")
    assert (src == BACKGROUND[-1]).any() and (src > BACKGROUND[-1]).any(), "the clamp is active in part of the cells"
    n_read, n_launch = R.hier.get_option("run_readbacks"), R.hier.get_option("recharge_launches")
    pi, nv, rrows, rlog = R.run(4, DT, T_K=T_K, background=BACKGROUND, diag_every=2, regrid_interval=2, reload=analytic, **REGRID)
    assert rlog == log
    assert R.hier.get_option("run_readbacks") - n_read == 1, "one read-back for all rows"
    assert R.hier.get_option("recharge_launches") - n_launch == 4 * 3, "four steps, one launch per level"
    assert rrows.shape == (2, 6) and np.array_equal(rrows, np.array(rows), equal_nan=True)
    assert np.isfinite(rrows[:, [0, 4, 5]]).all()
    assert np.array_equal(R.postproc_temporal(), rows[-1], equal_nan=True)
    assert_same_counts(pi, nv, counts)
    assert_same_state(R, L)
    for l, bl in enumerate(R.level):
        for k in range(len(bl)):
            assert np.array_equal(R.level[l][k].get(lv.F_ZS, ghosted=True), L.level[l][k].get(lv.F_ZS, ghosted=True)), (l, k)
    R.close(); L.close()


# ------------------------------------------------------------------ 5. implicit gap across a regrid
def test_implicit_gap_across_a_regrid():
    """an implicit step on either side of a regrid that moves boxes.  The gap-height hierarchy of the implicit solve belongs to the handle it was
    made for: the one of the old boxes (3 + 2) goes with them, and the first implicit step after the regrid makes one on the new boxes (2 + 2)"""
    mdl = dict(STEP_MODEL, use_impl_diff=1)
    R, L = shmip_model(mdl=mdl), shmip_model(mdl=mdl)
    f = np.ones(4)
    counts, _, log, _ = loop(L, 4, moulin_factor=f, regrid_interval=2)
    assert [e["same"] for e in log] == [False]
    kw = dict(moulins=MOULINS, regrid_interval=2, reload=analytic, **REGRID)
    assert R.hier.get_option("gap_num_boxes") == -1
    p1, v1, _, log1 = R.run(2, DT, moulin_factor=f[:2], **kw)
    assert log1 == [] and R.hier.boxes == OLD and R.hier.get_option("gap_num_boxes") == sum(len(bl) for bl in OLD)
    p2, v2, _, log2 = R.run(2, DT, moulin_factor=f[2:], **kw)
    assert log2 == log and R.last_run["n_moved"] == 1
    assert R.hier.boxes == GEN and R.hier.get_option("gap_num_boxes") == sum(len(bl) for bl in GEN), "rebuilt on the new boxes"
    assert_same_counts(list(p1) + list(p2), list(v1) + list(v2), counts)
    assert_same_state(R, L)
    R.close(); L.close()


# ------------------------------------------------------------------ 5b. the surface height across a regrid
NO_ZS = ["head", "B", "Pi", "zb", "mask", "mR", "Pw"]


def test_a_seasonal_run_whose_regrid_loses_the_surface_ends_there():
    """T_K with a field list that leaves the surface height out and a reload that does not bring it: the new boxes do not hold SUHMO_F_ZS.  The
    run ends at that regrid with rc -1 naming the first such box, nothing launched on the new hierarchy, and the model goes on once the surface is
    loaded"""
    from suhmo_amd import capi
    R = shmip_model(mdl=SEASON_MODEL)
    load_season_surface(R)
    n = R.hier.get_option("recharge_launches")
    with pytest.raises(capi.SuhmoError) as e:
        R.run(4, DT, T_K=T_K, background=BACKGROUND, regrid_interval=2, reload=analytic, fields=NO_ZS, **REGRID)
    assert _rc(e.value) == -1 and "SUHMO_F_ZS" in str(e.value) and "level 1, box 0" in str(e.value)
    assert R.last_run["steps_done"] == 2 and R.last_run["n_moved"] == 1 and R.cur_step == 2
    assert R.hier.boxes == GEN, "the new hierarchy is the model's"
    assert R.hier.get_option("recharge_launches") - n == 2 * 3, "two steps on the old hierarchy, nothing on the new one"
    load_season_surface(R)
    pi, nv, _, log = R.run(2, DT, T_K=T_K[2:], background=BACKGROUND[2:], regrid_interval=2, reload=analytic, fields=NO_ZS, **REGRID)
    assert [e["same"] for e in log] == [True] and R.cur_step == 4 and all(pi > 0)
    assert all(np.isfinite(R.get(l, k, "head")).all() for l, bl in enumerate(R.level) for k in range(len(bl)))
    R.close()


def test_a_reload_that_brings_the_surface_keeps_a_seasonal_run_going():
    R = shmip_model(mdl=SEASON_MODEL)
    load_season_surface(R)

    def reload(l, k, b):
        f = analytic(l, k, b)
        f["zs"] = f["Pi"] / (sy.RHO_I * sy.GRAV)
        return f

    _, _, _, log = R.run(4, DT, T_K=T_K, background=BACKGROUND, regrid_interval=2, reload=reload, fields=NO_ZS, **REGRID)
    assert [e["same"] for e in log] == [False] and R.last_run["steps_done"] == 4
    from suhmo_amd import level as lv
    for l, bl in enumerate(GEN, start=1):
        for k, b in enumerate(bl):
            assert np.array_equal(R.level[l][k].get(lv.F_ZS, ghosted=True), reload(l, k, b)["zs"]), (l, k)
    R.close()


# ------------------------------------------------------------------ 6. two consecutive runs equal one
@pytest.mark.parametrize("split,skip", [(2, False), (3, False), (2, True)], ids=["at-a-regrid", "beside-a-regrid", "restart-skips-it"])
def test_two_runs_equal_one(split, skip):
    kw = dict(moulins=MOULINS, regrid_interval=2, reload=analytic, **REGRID)
    T = shmip_model()
    p1, v1, _, log1 = T.run(split, DT, moulin_factor=FACTOR[:split], ramp=RAMP[:split], **kw)
    p2, v2, _, log2 = T.run(6 - split, DT, moulin_factor=FACTOR[split:], ramp=RAMP[split:], skip_first_regrid=skip, **kw)
    if not skip:
        O = shmip_model()
        po, vo, _, logo = O.run(6, DT, moulin_factor=FACTOR, ramp=RAMP, **kw)
        assert [e["cur_step"] for e in logo] == [3, 5] and log1 + log2 == logo
        assert list(p1) + list(p2) == list(po) and list(v1) + list(v2) == list(vo)
    else:                                                    # the restart omits exactly the regrid before its first step
        assert log1 == [] and [e["cur_step"] for e in log2] == [5] and not log2[0]["same"]
        O = shmip_model()
        c1 = loop(O, split, moulin_factor=FACTOR[:split], ramp=RAMP[:split], regrid_interval=2)[0]
        c2 = loop(O, 6 - split, moulin_factor=FACTOR[split:], ramp=RAMP[split:], regrid_interval=2, skip_first=True)[0]
        assert_same_counts(list(p1) + list(p2), list(v1) + list(v2), c1 + c2)
    assert_same_state(T, O, (split, skip))
    T.close(); O.close()


# ------------------------------------------------------------------ 7. level ranges
def test_level_ranges_tag_exactly_their_levels():
    """on GEN every regrid finds the same grids, so the handle and its tag maps outlive the run: they must be what tagging exactly the levels of
    each variable's range gives (A: level 0; B: level 1, restricted; level 2: none, max_level - 1 = 1)"""
    R, L = shmip_model(GEN), shmip_model(GEN)
    h = R.hier.h.value
    _, _, _, log = R.run(2, DT, moulins=MOULINS, regrid_interval=1, reload=analytic, **REGRID)
    assert [e["same"] for e in log] == [True] and R.hier.h.value == h
    a, b = SPECS
    L.tag_cells(0, "Pi", a["vmin"], a["vmax"], granularity=1)
    L.tag_cells(1, "Pi", b["vmin"], b["vmax"], granularity=1)
    L.restrict_tags(1, SUBS[1])
    for l in (0, 1):
        assert R.tags(l).any() and np.array_equal(R.tags(l), L.tags(l)), l
    t1 = R.tags(1)
    assert t1[16:48, 44:52].all() and t1.sum() == 32 * 8, "the subset cut variable B's band to the rows 16 .. 47"
    assert R.tags(2) is None
    R.close(); L.close()


def test_a_variable_capped_at_level_0_never_makes_a_level_2():
    R = shmip_model()
    assert R.hier.nlev == 3
    _, _, _, log = R.run(3, DT, moulins=MOULINS, regrid_interval=1, tag_specs=SPECS[:1], params=PARAMS, reload=analytic)
    assert [e["cur_step"] for e in log] == [2, 3] and [e["same"] for e in log] == [False, True]
    assert all(len(e["boxes_per_level"]) == 1 for e in log) and R.hier.nlev == 2 and R.hier.boxes == GEN[:1]
    R.close()


# ------------------------------------------------------------------ 8. reload
def test_reload_is_called_once_per_moving_regrid_with_the_new_hierarchy():
    R = shmip_model()
    old_h, seen = R.hier.h.value, []

    def reload(l, k, b):
        seen.append((l, k, tuple(b), R.hier.h.value, [list(x) for x in R.hier.boxes]))
        f = analytic(l, k, b)
        f["zb"] = f["zb"] + 1.0e-3                              # not what the transfer brought
        return f

    _, _, _, log = R.run(4, DT, moulins=MOULINS, regrid_interval=2, reload=reload, **REGRID)
    assert [e["same"] for e in log] == [False]
    assert [(l, k, b) for l, k, b, _, _ in seen] == [(l, k, b) for l, bl in enumerate(GEN, start=1) for k, b in enumerate(bl)], "every new box once"
    assert all(h == R.hier.h.value and h != old_h and bx == [list(x) for x in GEN] for _, _, _, h, bx in seen), "called with the new handle bound"
    for l, bl in enumerate(GEN, start=1):
        for k, b in enumerate(bl):
            assert np.array_equal(R.get(l, k, "zb"), analytic(l, k, b)["zb"][1:-1, 1:-1] + 1.0e-3), (l, k)
    R.close()


def test_a_reload_that_raises_ends_the_run_and_the_model_goes_on():
    R = shmip_model()

    def reload(l, k, b):
        raise KeyError("no bed for box %d of level %d" % (k, l))

    with pytest.raises(KeyError):
        R.run(4, DT, moulins=MOULINS, regrid_interval=2, reload=reload, **REGRID)
    assert R.last_run["steps_done"] == 2 and R.cur_step == 2
    assert R.hier.boxes == GEN, "the new hierarchy is the model's"
    R.moulin_source(**MOULINS)
    R.timestep(DT)
    assert R.cur_step == 3 and all(np.isfinite(R.get(l, k, "head")).all() for l, bl in enumerate(R.level) for k in range(len(bl)))
    R.close()


# ------------------------------------------------------------------ 9. refusals launch nothing
def c_run(M, **over):
    """suhmo_hier_run with a schedule given field by field -> (rc, message)"""
    from suhmo_amd import capi
    keep = []

    def arr(x, t=np.float64):
        a = np.ascontiguousarray(x, dtype=t)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_double if t == np.float64 else C.c_int))

    sch = capi.HierSchedule(n_steps=2, dt=DT, first_cur_step=M.cur_step + 1, max_level=2)
    for key, v in over.items():
        if key == "mp":
            continue
        setattr(sch, key, arr(v) if isinstance(v, (list, np.ndarray)) else v)
    rows, pi = np.zeros((2, 6)), np.zeros(2, dtype=np.intc)
    res = capi.HierRunResult(picard_iters=arr(pi, np.intc), rows=rows.ctypes.data_as(C.POINTER(C.c_double)))
    hp = C.c_void_p(M.hier.h.value)
    rc = capi.lib().suhmo_hier_run(C.byref(hp), C.byref(over.get("mp", M._mp)), C.byref(sch), C.byref(res), M.hier.stream)
    assert hp.value == M.hier.h.value and res.steps_done == 0
    return rc, capi.lib().suhmo_last_error().decode()


def test_refusals_launch_nothing():
    from suhmo_amd import capi, model
    M, T = shmip_model(), shmip_model()
    for G in (M, T):
        G.moulin_source(**MOULINS)
    pos, sg, fl = np.array(MOULINS["positions"]).reshape(-1), np.array(MOULINS["sigma"]), np.array(MOULINS["flux"])
    tags = (capi.TagSpec * 1)(capi.TagSpec(M.FIELDS["Pi"], 0.0, 1.0, 0, 0, 0, 0, 0))
    grid = capi.GridParams(0.7, 2, 32, 2)
    two = [1.0, 1.0]
    cases = [
        (dict(n_steps=0), -1), (dict(dt=0.0), -1), (dict(first_cur_step=0), -1), (dict(diag_every=-1), -1),
        (dict(T_K=two), -1), (dict(background=two), -1),
        (dict(n_moulins=3, positions=pos, sigma=sg), -1), (dict(positions=pos, sigma=sg, flux=fl), -1), (dict(moulin_factor=two), -1),
        (dict(n_moulins=3, positions=pos, sigma=-sg, flux=fl), -1),
        (dict(T_K=two, background=two, n_moulins=3, positions=pos, sigma=sg, flux=fl), -1),
        (dict(regrid_interval=1), -1), (dict(regrid_interval=-1), -1),
        (dict(regrid_interval=1, n_tags=1, tags=tags, grid=capi.GridParams(0.7, 3, 12, 2)), -1),
        (dict(regrid_interval=1, n_tags=1, tags=tags, grid=capi.GridParams(1.5, 2, 32, 2)), -1),
        (dict(regrid_interval=1, n_tags=1, tags=tags, grid=grid, max_level=0), -1),
        (dict(T_K=two, background=two), -1),                                            # no SUHMO_F_ZS anywhere
        (dict(mp=model.model_params(dict(STEP_MODEL, use_impl_diff=1, diffFactor=0.0))), -1),
    ]
    for over, want in cases:
        rc, msg = c_run(M, **over)
        assert rc == want and msg, (over.keys(), rc, msg)
    F = shmip_model()                                        # use_moulin_source, no forcing and no source term
    rc, msg = c_run(F)
    assert rc == -1 and "source term" in msg
    S = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, j0=0, ny_global=64)
    rc, msg = c_run(S, n_moulins=3, positions=pos, sigma=sg, flux=fl)
    assert rc == -5 and "rank strips" in msg
    S.close(); F.close()
    # nothing was launched and nothing was formed: the model steps like one that was never asked
    assert M.timestep(DT) == T.timestep(DT)
    assert_same_state(M, T)
    M.close(); T.close()
