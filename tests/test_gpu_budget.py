"""The water budget on the device (include/suhmo_hip.h, "WATER BUDGET"; suhmo_amd/csrc/suhmo_balance.hip, suhmo_run.hip, suhmo_batch.hip): ten
doubles per level or member, BITWISE (np.array_equal; same_bits where NaN occurs) against the numpy twin tests/budget_ref.py, against the
mass-balance calls (the first seven values; VOLUME_OLD = the VOLUME of the mass balance made right before the tracked step) and, for the series
inside suhmo_hier_run_bud / suhmo_batch_run_bud, against the per-call loop: regrid, forcing, mass_balance, step, water_budget.  Option
track_old_volume, the launch and copy counts, bud = NULL through the new entry points, every refusal."""
import ctypes as C

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import budget_ref as br
from tests import flatten_ref as fr
from tests import hierlayouts as hl
from tests import massbalance_ref as mb
from tests import reduce_ref as rr
from tests import stepsweep as sw
from tests.test_gpu_massbalance import DT, MODEL, as_row, box_data, load_masks, member_inputs
from tests.test_massbalance_cpu import same_bits            # (scalars too: np.asarray on both sides)

pytestmark = pytest.mark.gpu
NAN = float("nan")
SHAPES = mb.SINGLE_SHAPES + ((12, 4),)                      # ... and fewer cells than one workgroup


def wb_row(d):
    return np.array([d[k] for k in br.NAMES])


def params(mp, **changes):
    """a copy of a model's suhmo_model_params_t with some members changed"""
    from suhmo_amd import capi
    out = capi.ModelParams.from_buffer_copy(mp)
    for k, v in changes.items():
        setattr(out, k, v)
    return out


def mp_dict(mp):
    return dict(use_moulin_source=int(mp.use_moulin_source), ramp=float(mp.ramp), distributed_input=float(mp.distributed_input), rho_w=float(mp.rho_w))


def budget_data(L, source):
    from suhmo_amd import level as lv
    return dict(box_data(L), mr=L.get(lv.F_MR), msrc=L.get(lv.F_MSRC) if source else None)


def level_budget_call(L, mp):
    from suhmo_amd import capi
    out = np.full(10, -77.0)
    capi.check(capi.lib().suhmo_level_water_budget(L.h, C.byref(mp), out.ctypes.data_as(C.POINTER(C.c_double)), L.stream))
    return out


def hier_budget_call(M, mp):
    from suhmo_amd import capi
    out = np.full((M.hier.nlev, 10), -77.0)
    capi.check(capi.lib().suhmo_hier_water_budget(M.hier.h, C.byref(mp), out.ctypes.data_as(C.POINTER(C.c_double)), M.hier.stream))
    return out


def source_field(ny, nx, seed):
    """a source term of both signs' worth of magnitudes, NaN-free; multiples of 2^-40 around 1e-7"""
    return np.random.default_rng([seed, nx, ny]).uniform(0.0, 2.0e-7, size=(ny, nx))


# ------------------------------------------------------------------ 1. single levels
def fresh_valley(nx, ny, bc, track):
    from suhmo_amd import level as lv, model
    st = sy.valley_initial_state(nx, ny, 0.05, gap_init=0.01)
    G = model.HipModel(nx, ny, st["dx"], st["dy"], bc, sw.PHYS, MODEL, max_box=64)
    G.set_state(st)
    G.level.set(lv.F_MR, np.full((ny, nx), MODEL["G"] / MODEL["L"]))
    if track:
        G.level.set_option("track_old_volume", 1)
    return G


@pytest.mark.parametrize("bcname", [n for n, _ in mb.SINGLE_BCS])
@pytest.mark.parametrize("nx,ny", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_single_levels(nx, ny, bcname):
    from suhmo_amd import level as lv
    bc = dict(mb.SINGLE_BCS)[bcname]
    G, U = fresh_valley(nx, ny, bc, True), fresh_valley(nx, ny, bc, False)
    assert G.level.get_option("track_old_volume") == 1 and U.level.get_option("track_old_volume") == 0
    whole, dom = [(0, 0, nx - 1, ny - 1)], (nx, ny)
    start = br.volume_of_boxes([G.level.get(lv.F_MASK, ghosted=True)], [G.level.get(lv.F_B)], G.dx, G.dy, rr.CAP_LEVEL)
    assert G.timestep(DT) == U.timestep(DT)
    first = wb_row(G.water_budget())
    assert same_bits(first[br.VOLUME_OLD], start), "the volume the first step started from, against the twin"
    between = as_row(G.mass_balance())
    assert G.timestep(DT) == U.timestep(DT)
    got = wb_row(G.water_budget())
    seven = as_row(G.mass_balance())
    print(nx, ny, bcname, got)
    assert same_bits(got[:7], seven), (got, seven)
    assert same_bits(got[br.VOLUME_OLD], between[mb.VOLUME]) and got[br.VOLUME_OLD] != got[mb.VOLUME], (got, between)
    # the recharge sums: the model's own parameters (no moulin source), then a source term and a ramp that is not 1
    ref = br.budget_of_level([budget_data(G.level, False)], whole, dom, bc, G.dx, G.dy, mp_dict(G._mp), rr.CAP_LEVEL, volume_old=between[mb.VOLUME])
    assert np.isfinite(ref).all() and np.array_equal(got, ref), (got, ref)
    assert got[br.RECH_EXT] >= 0.0 and got[br.RECH_MELT] > 0.0
    for X in (G, U):
        X.level.set(lv.F_MSRC, source_field(ny, nx, 5))
    mp = params(G._mp, use_moulin_source=1, ramp=0.625, distributed_input=7.93e-11)
    got2 = level_budget_call(G.level, mp)
    ref2 = br.budget_of_level([budget_data(G.level, True)], whole, dom, bc, G.dx, G.dy, mp_dict(mp), rr.CAP_LEVEL, volume_old=between[mb.VOLUME])
    assert np.array_equal(got2, ref2) and got2[br.RECH_EXT] > got[br.RECH_EXT], (got2, ref2)
    assert same_bits(got2, level_budget_call(G.level, mp)), "the call twice"
    # the option off: NaN, and the same step bit for bit
    off = wb_row(U.water_budget())
    assert np.isnan(off[br.VOLUME_OLD]) and same_bits(np.delete(off, br.VOLUME_OLD), np.delete(got, br.VOLUME_OLD)), (off, got)
    for nm in G.FIELDS:
        assert np.array_equal(G.get(nm, ghosted=True), U.get(nm, ghosted=True), equal_nan=True), nm
    G.close(); U.close()


# ------------------------------------------------------------------ 2. hierarchies
def hier_volumes(M, nx0, ny0):
    """the twin's k_volume of every level from the masks and gap heights as they lie on the device"""
    from suhmo_amd import level as lv
    out = []
    for l, bl in enumerate(M.level):
        out.append(br.volume_of_boxes([L.get(lv.F_MASK, ghosted=True) for L in bl], [L.get(lv.F_B) for L in bl], bl[0].dx, bl[0].dy,
                                      rr.CAP_LEVEL if l == 0 else rr.CAP_BOX))
    return np.array(out)


def assert_hier_budget(M, nx0, ny0, bc, mp, old, what):
    nlev = M.hier.nlev
    n_l, n_c = M.hier.get_option("budget_launches"), M.hier.get_option("budget_copies")
    got = hier_budget_call(M, mp)
    assert M.hier.get_option("budget_launches") - n_l == nlev + 1 and M.hier.get_option("budget_copies") - n_c == 1, what
    src = bool(mp.use_moulin_source)
    for l, bl in enumerate(fr.all_boxes(nx0, ny0, M.hier.boxes)):
        L0 = M.level[l][0]
        ref = br.budget_of_level([budget_data(L, src) for L in M.level[l]], bl, (nx0 << l, ny0 << l), bc, L0.dx, L0.dy, mp_dict(mp),
                                 rr.CAP_LEVEL if l == 0 else rr.CAP_BOX, volume_old=old[l])
        print(what, "level", l, got[l], ref)
        assert np.isfinite(np.delete(ref, br.VOLUME_OLD)).all(), (what, l, ref)
        assert same_bits(got[l], ref), (what, "level", l, got[l], ref)
    return got


def tracked_hierarchy(nx0, ny0, bc, boxes, what):
    """a hierarchy stepped with track_old_volume = 1: the mass balance right before the step (its face coefficients formed by UpdateOperator) gives
    the volume the step must keep; compared as stepped, then with margins and a source term loaded into every box (the face coefficients and the
    kept volume stay what the step left)"""
    from suhmo_amd import level as lv, model
    sts = sy.shmip_amrm_states(nx0, ny0, boxes, rough=0.5)
    M = model.HipHierModel(nx0, ny0, sts[0][0]["dx"], sts[0][0]["dy"], bc, sy.A3_PHYS, sy.A3_MODEL, boxes, max_box=16)
    M.set_states(sts)
    M.hier.set_option("track_old_volume", 1)
    assert M.hier.get_option("track_old_volume") == 1 and M.hier.get_option("budget_device_bytes") == 0
    nlev = M.hier.nlev
    for l in range(nlev):
        M.hier.update_operator(l)
    before = np.array([as_row(d) for d in M.mass_balance()])
    assert same_bits(before[:, mb.VOLUME], hier_volumes(M, nx0, ny0)), "the twin's volume-only reduction is the mass balance's VOLUME on the device too"
    n_l = M.hier.get_option("budget_launches")
    M.timestep(sy.A3_MODEL["dt"])
    assert M.hier.get_option("budget_launches") - n_l == nlev, "a tracked step: one k_volume launch per level, never one per box"
    assert M.hier.get_option("budget_copies") == 0 and M.hier.get_option("budget_device_bytes") > 0
    got = assert_hier_budget(M, nx0, ny0, bc, M._mp, before[:, mb.VOLUME], (what, "as stepped"))
    assert same_bits(got[:, :7], np.array([as_row(d) for d in M.mass_balance()]))
    assert (got[:, br.VOLUME_OLD] != got[:, mb.VOLUME]).all()
    load_masks(M, nx0, ny0, bc, 7)
    for l, bl in enumerate(M.level):
        for k, L in enumerate(bl):
            L.set(lv.F_MSRC, source_field(L.ny, L.nx, 100 * l + k))
    mp = params(M._mp, use_moulin_source=1, ramp=0.625, distributed_input=7.93e-11)
    got = assert_hier_budget(M, nx0, ny0, bc, mp, before[:, mb.VOLUME], (what, "margins, source"))
    assert same_bits(got[:, :7], np.array([as_row(d) for d in M.mass_balance()]))
    assert (got[:, br.RECH_EXT] > 0.0).all() and (got[:, br.RECH_MELT] > 0.0).all()
    assert (got[:, mb.DIR_X] != 0.0).all() and (got[:, mb.DIR_Y] != 0.0).all()
    M.close()


@pytest.mark.parametrize("key", mb.HIER_KEYS, ids=[str(k) for k in mb.HIER_KEYS])
def test_hierarchies(key):
    bc, boxes = fr.case(key)
    tracked_hierarchy(hl.NX0, hl.NY0, bc, boxes, key)


def test_boxes_beyond_the_cap_of_a_box():
    nx0, ny0, boxes = mb.WALK_EDGE_LAYOUT
    tracked_hierarchy(nx0, ny0, hl._NP, boxes, "walk edges")


def test_level_0_of_a_hierarchy_has_the_bits_of_the_level_alone():
    from suhmo_amd import level as lv, model
    nx, ny = 70, 9
    st = sy.valley_initial_state(nx, ny, 0.05, gap_init=0.01)
    G = fresh_valley(nx, ny, mb.NEUMANN_BC, True)
    H = model.HipHierModel(nx, ny, st["dx"], st["dy"], mb.NEUMANN_BC, sw.PHYS, MODEL, [], max_box=64)
    H.set_state(0, 0, st)
    H.level[0][0].set(lv.F_MR, np.full((ny, nx), MODEL["G"] / MODEL["L"]))
    H.hier.set_option("track_old_volume", 1)
    for n in range(2):
        G.timestep(DT); H.timestep(DT)
    a, b = wb_row(G.water_budget()), wb_row(H.water_budget()[0])
    assert same_bits(a, b) and np.isfinite(a).all(), (a, b)
    G.close(); H.close()


def test_after_a_regrid_the_kept_volume_is_gone_until_the_next_step():
    from suhmo_amd import capi
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT as HDT, REGRID
    M = shmip_model()
    M.hier.set_option("track_old_volume", 1)
    M.moulin_source(**MOULINS)
    M.timestep(HDT)
    before = np.array([wb_row(d) for d in M.water_budget()])
    assert np.isfinite(before).all()
    old = [list(bl) for bl in M.hier.boxes]
    boxes, same = M.tag_and_regrid(**REGRID)
    assert not same and boxes != old
    assert M.hier.get_option("track_old_volume") == 1, "the option travels to the new handle"
    assert [M.hier.get_option(k) for k in ("budget_launches", "budget_copies", "budget_device_bytes")] == [0, 0, 0], "a new handle: it holds no buffer yet"
    # the new boxes hold no face coefficients until a step or UpdateOperator forms them: refused, nothing launched
    out = np.full((M.hier.nlev, 10), -77.0)
    rc = capi.lib().suhmo_hier_water_budget(M.hier.h, C.byref(M._mp), out.ctypes.data_as(C.POINTER(C.c_double)), M.hier.stream)
    assert rc == -1 and b"face coefficients" in capi.lib().suhmo_last_error() and (out == -77.0).all() and M.hier.get_option("budget_launches") == 0
    M.moulin_source(**MOULINS)
    for l in range(M.hier.nlev):
        M.hier.update_operator(l)
    got = np.array([wb_row(d) for d in M.water_budget()])
    assert np.isnan(got[:, br.VOLUME_OLD]).all() and np.isfinite(np.delete(got, br.VOLUME_OLD, axis=1)).all(), got
    between = np.array([as_row(d) for d in M.mass_balance()])
    M.timestep(HDT)
    got = np.array([wb_row(d) for d in M.water_budget()])
    assert same_bits(got[:, br.VOLUME_OLD], between[:, mb.VOLUME]), (got, between)
    M.close()


# ------------------------------------------------------------------ 3. ensembles
ENS = dict(n=6, nx=40, ny=24)


def ensemble_models(n):
    return [sw.model_of("implicit" if k % 2 else "explicit") for k in range(n)]


def ensemble(track=True):
    from suhmo_amd import level as lv, model
    n, nx, ny = ENS["n"], ENS["nx"], ENS["ny"]
    sts, bcs = member_inputs(n, nx, ny)
    models = ensemble_models(n)
    B = model.HipBatchModel(nx, ny, sts[0]["dx"], sts[0]["dy"], bcs, sw.PHYS, models, max_box=8, implicit_gap=True)
    for k in range(n):
        B.set_state(k, sts[k])
        B.member(k).level.set(lv.F_MR, np.full((ny, nx), models[k]["G"] / models[k]["L"]))
    if track:
        B.set_option("track_old_volume", 1)
    return B, sts, bcs, models


def member_alone(k, sts, bcs, models, steps):
    from suhmo_amd import level as lv, model
    nx, ny = ENS["nx"], ENS["ny"]
    G = model.HipModel(nx, ny, sts[k]["dx"], sts[k]["dy"], bcs[k], sw.PHYS, models[k], max_box=8)
    G.set_state(sts[k])
    G.level.set(lv.F_MR, np.full((ny, nx), models[k]["G"] / models[k]["L"]))
    G.level.set_option("track_old_volume", 1)
    for _ in range(steps):
        G.timestep(DT)
    out = wb_row(G.water_budget())
    G.close()
    return out


def test_ensembles():
    n, nx, ny = ENS["n"], ENS["nx"], ENS["ny"]
    B, sts, bcs, models = ensemble()
    assert B.get_option("track_old_volume") == 1
    n_l = B.get_option("batch_launches")
    U = ensemble(track=False)[0]
    u_l = U.get_option("batch_launches")
    assert B.timestep(DT) == U.timestep(DT)
    assert (B.get_option("batch_launches") - n_l) - (U.get_option("batch_launches") - u_l) == 1, "a tracked step: ONE more launch for all members"
    between = B.mass_balance_all()
    assert B.timestep(DT) == U.timestep(DT)
    n_l, n_r = B.get_option("batch_launches"), B.get_option("batch_readbacks")
    got = B.water_budget_all()
    assert B.get_option("batch_launches") - n_l == 2 and B.get_option("batch_readbacks") - n_r == 1
    assert got.shape == (n, 10) and np.isfinite(got).all()
    assert same_bits(got[:, :7], B.mass_balance_all()) and same_bits(got[:, br.VOLUME_OLD], between[:, mb.VOLUME])
    for k in range(n):
        L = B.member(k).level
        ref = br.budget_of_level([budget_data(L, False)], [(0, 0, nx - 1, ny - 1)], (nx, ny), bcs[k], L.dx, L.dy, mp_dict(B._mp[k]), rr.CAP_LEVEL,
                                 volume_old=between[k, mb.VOLUME])
        print(k, got[k], ref)
        assert np.array_equal(got[k], ref), (k, got[k], ref)
        assert same_bits(got[k], member_alone(k, sts, bcs, models, 2)), ("the same model alone", k)
        for nm in ("head", "B", "mR"):
            assert np.array_equal(B.get(k, nm, ghosted=True), U.get(k, nm, ghosted=True), equal_nan=True), ("tracking changes no field", k, nm)
    off = U.water_budget_all()
    assert np.isnan(off[:, br.VOLUME_OLD]).all() and same_bits(np.delete(off, br.VOLUME_OLD, axis=1), np.delete(got, br.VOLUME_OLD, axis=1))
    # a subset: the rows without a flag keep the caller's values
    active = [k % 3 != 1 for k in range(n)]
    out = np.full((n, 10), -77.0)
    assert B.water_budget_all(active=active, out=out) is out
    for k in range(n):
        assert same_bits(out[k], got[k] if active[k] else np.full(10, -77.0)), k
    none = np.full((n, 10), -77.0)
    n_r = B.get_option("batch_readbacks")
    B.water_budget_all(active=[False] * n, out=none)
    assert (none == -77.0).all() and B.get_option("batch_readbacks") == n_r
    # a step that leaves members out: they keep the volume they had, the others measure anew
    mid = B.mass_balance_all()
    B.run(1, DT, active=active)
    after = B.water_budget_all()
    for k in range(n):
        assert same_bits(after[k, br.VOLUME_OLD], mid[k, mb.VOLUME] if active[k] else got[k, br.VOLUME_OLD]), k
    assert B.get_option("track_old_volume") == 1
    B.close(); U.close()


# ------------------------------------------------------------------ 4. the run of a hierarchy
T6 = np.array([8.0, 6.0, 9.0, 3.0, 7.0, 10.0])
BG6 = np.array([7.93e-11, 7.93e-11, 1.0e-10, 1.0e-10, 9.0e-11, 9.0e-11])


def budget_loop(M, n_steps, every, T_K=None, background=None, moulin_factor=None, ramp=None, diag_every=0, regrid_interval=2):
    """the loop of public calls a run with a budget replaces: regrid, forcing, mass_balance, step, water_budget"""
    from suhmo_amd import capi, model
    from tests.test_gpu_hier_run import MOULINS, DT as HDT, REGRID, analytic
    due = model.regrid_steps(M.cur_step + 1, n_steps, regrid_interval, False)
    counts, rows, wrows, nlevs, log = [], [], [], [], []
    for k in range(n_steps):
        c, changed = M.cur_step + 1, False
        if c in due:
            boxes, same = M.tag_and_regrid(reload=analytic, **REGRID)
            changed = not same
            log.append(dict(cur_step=c, same=same, boxes_per_level=[len(bl) for bl in boxes]))
        if T_K is not None:
            M.time_varying_recharge(T_K[k], background[k])
        elif k == 0 or changed or np.float64(moulin_factor[k]).tobytes() != np.float64(moulin_factor[k - 1]).tobytes():
            M.moulin_source(time_factor=moulin_factor[k], **MOULINS)
        if ramp is not None:
            M._mp.ramp = float(ramp[k])
        row = (k + 1) % every == 0
        before = None
        if row and not changed and k > 0:                    # (new boxes have no face coefficients before their first step: no mass balance there)
            before = np.array([as_row(d) for d in M.mass_balance()])
        M.hier.set_option("track_old_volume", int(row))
        counts.append(M.timestep(HDT))
        M.hier.set_option("track_old_volume", 0)
        if diag_every and (k + 1) % diag_every == 0:
            rows.append(M.postproc_temporal())
        if row:
            w = np.array([wb_row(d) for d in M.water_budget()])
            if before is not None:
                assert same_bits(w[:, br.VOLUME_OLD], before[:, mb.VOLUME]), ("Bold is the volume before the step", k)
            assert np.isfinite(w).all(), (k, w)
            wrows.append(w); nlevs.append(M.hier.nlev)
    return counts, rows, wrows, nlevs, log


def assert_budget_series(R, wrows, nlevs):
    got, gl = R.last_run["budget"], R.last_run["budget_nlev"]
    assert got.shape[0] == len(wrows) and list(gl) == nlevs and got.shape[2] == 10
    for r, w in enumerate(wrows):
        assert same_bits(got[r, :nlevs[r]], w), ("row", r, got[r], w)
        assert np.isnan(got[r, nlevs[r]:]).all(), "entries beyond nlev stay NaN"


@pytest.mark.parametrize("every", [1, 3])
def test_run_of_a_hierarchy_seasonal(every):
    from tests.test_gpu_hier_run import (shmip_model, SEASON_MODEL, load_season_surface, analytic, REGRID, DT as HDT, assert_same_state,
                                         assert_same_counts)
    R, L, N = (shmip_model(mdl=SEASON_MODEL) for _ in range(3))
    for X in (R, L, N):
        load_season_surface(X)
    counts, rows, wrows, nlevs, log = budget_loop(L, 6, every, T_K=T6, background=BG6, diag_every=2)
    assert any(not e["same"] for e in log), "a regrid that moves boxes"
    kw = dict(T_K=T6, background=BG6, diag_every=2, regrid_interval=2, reload=analytic, **REGRID)
    c0 = [R.hier.get_option(k) for k in ("budget_copies", "run_readbacks")]
    n0 = N.hier.get_option("run_readbacks")
    pi, nv, rrows, rlog = R.run(6, HDT, balance_every=every, **kw)
    npi, nnv, nrows, nlog = N.run(6, HDT, **kw)
    assert rlog == log == nlog
    assert R.hier.get_option("budget_copies") - c0[0] == 1, "one copy for the whole series, carried over the regrids"
    assert R.hier.get_option("run_readbacks") - c0[1] == N.hier.get_option("run_readbacks") - n0 == 1
    assert R.hier.get_option("track_old_volume") == 0, "the caller's setting is back"
    assert_budget_series(R, wrows, nlevs)
    assert R.last_run["budget"].shape[1] == 3, "max_level + 1 levels of room"
    assert_same_counts(pi, nv, counts); assert_same_counts(npi, nnv, counts)
    assert np.array_equal(rrows, np.array(rows), equal_nan=True) and np.array_equal(rrows, nrows, equal_nan=True)
    assert_same_state(R, L); assert_same_state(R, N)
    for X in (R, L, N):
        X.close()


def test_run_of_a_hierarchy_with_moulins_and_output(monkeypatch):
    from tests.test_gpu_hier_run import shmip_model, MOULINS, FACTOR, RAMP, analytic, REGRID, DT as HDT, assert_same_state, assert_same_counts
    from tests.test_gpu_hier_run_output import capture
    R, L, O = shmip_model(), shmip_model(), shmip_model()
    counts, _, wrows, nlevs, log = budget_loop(L, 6, 3, moulin_factor=FACTOR, ramp=RAMP)
    assert any(not e["same"] for e in log)
    kw = dict(moulins=MOULINS, moulin_factor=FACTOR, ramp=RAMP, regrid_interval=2, reload=analytic, **REGRID)
    pi, nv, _, rlog = R.run(6, HDT, balance_every=3, **kw)
    assert rlog == log
    assert_budget_series(R, wrows, nlevs)
    assert_same_counts(pi, nv, counts)
    assert_same_state(R, L)
    # ... and through suhmo_hier_run_bud with an output struct: the same series, the events of the run without a budget
    events = capture(monkeypatch, O)
    pi, nv, _, olog = O.run(6, HDT, balance_every=3, plot_interval=3, check_interval=-1, **kw)
    assert olog == log and len(events) == 3 and O.hier.get_option("run_plots") == 3
    assert_budget_series(O, wrows, nlevs)
    assert O.hier.get_option("budget_copies") == 1
    assert_same_counts(pi, nv, counts)
    assert_same_state(O, L)
    for X in (R, L, O):
        X.close()


# ------------------------------------------------------------------ 5. the run of an ensemble
@pytest.mark.parametrize("every", [1, 3])
def test_run_of_an_ensemble(every):
    n = ENS["n"]
    R, L, N = ensemble(track=False)[0], ensemble(track=False)[0], ensemble(track=False)[0]
    active = [k % 3 != 1 for k in range(n)]
    ramp = np.array([0.25, 0.5, 0.75, 1.0, 1.0, 0.875])
    wrows, pis, nvs = [], [], []
    for k in range(6):
        for q in range(n):
            L.set_model(q, ramp=float(ramp[k]))
        row = (k + 1) % every == 0
        before = L.mass_balance_all(active=active, out=np.full((n, 7), NAN)) if row and k > 0 else None
        L.set_option("track_old_volume", int(row))
        p, v, _ = L.run(1, DT, active=active)                 # (a step of a subset is a run of one step)
        L.set_option("track_old_volume", 0)
        pis.append(p[0]); nvs.append(v[0])
        if row:
            w = L.water_budget_all(active=active, out=np.full((n, 10), NAN))
            if before is not None:
                assert same_bits(w[:, br.VOLUME_OLD], before[:, mb.VOLUME]), k
            wrows.append(w)
    r0, n0 = R.get_option("batch_readbacks"), N.get_option("batch_readbacks")
    pi, nv, _ = R.run(6, DT, ramp=ramp, active=active, balance_every=every)
    npi, nnv, _ = N.run(6, DT, ramp=ramp, active=active)
    got = R.last_run["budget"]
    assert got.shape == (6 // every, n, 10) and R.last_run["budget_rows"] == 6 // every
    assert same_bits(got, np.array(wrows)), (got, wrows)
    assert all(np.isnan(got[:, k]).all() != active[k] for k in range(n)), "rows of members without a flag are untouched (NaN prefill)"
    assert np.isfinite(got[:, [k for k in range(n) if active[k]]]).all()
    assert (R.get_option("batch_readbacks") - r0) - (N.get_option("batch_readbacks") - n0) == 1, "exactly one more read-back"
    assert R.get_option("track_old_volume") == 0
    assert np.array_equal(pi, np.array(pis)) and np.array_equal(nv, np.array(nvs)) and np.array_equal(pi, npi) and np.array_equal(nv, nnv)
    for k in range(n):
        for nm in ("head", "B", "mR", "Pw", "qwx"):
            a = R.get(k, nm, ghosted=True) if active[k] or nm in ("head", "B") else None
            if a is not None:
                assert np.array_equal(a, L.get(k, nm, ghosted=True), equal_nan=True) and np.array_equal(a, N.get(k, nm, ghosted=True), equal_nan=True), (k, nm)
    for X in (R, L, N):
        X.close()


# ------------------------------------------------------------------ 6. bud = NULL through the new entry points
def hier_run_bud(X, bud, n_steps=2, moulins=True, diag_every=0, rows=None, counts=None):
    """suhmo_hier_run_bud itself, without an output struct and without regrids: -> (rc, result)"""
    from suhmo_amd import capi
    from tests.test_gpu_hier_run import MOULINS, DT as HDT
    pos, sg, fl = (np.ascontiguousarray(MOULINS[q], dtype=np.float64).reshape(-1) for q in ("positions", "sigma", "flux"))
    d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    sch = capi.HierSchedule(n_steps=n_steps, dt=HDT, first_cur_step=X.cur_step + 1, regrid_interval=0, max_level=2, diag_every=diag_every)
    if moulins:
        sch.n_moulins, sch.positions, sch.sigma, sch.flux = sg.size, d(pos), d(sg), d(fl)
    res = capi.HierRunResult()
    if rows is not None:
        res.rows = d(rows)
    if counts is not None:
        res.picard_iters, res.vcycles = (c.ctypes.data_as(C.POINTER(C.c_int)) for c in counts)
    hp = C.c_void_p(X.hier.h.value)
    rc = capi.lib().suhmo_hier_run_bud(C.byref(hp), C.byref(X._mp), C.byref(sch), None, None if bud is None else C.byref(bud), C.byref(res), X.hier.stream)
    assert hp.value == X.hier.h.value, "no regrid: the handle stays"
    return rc, res


def test_without_a_budget_the_new_entry_points_are_the_old_ones():
    from suhmo_amd import capi
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT as HDT, assert_same_state
    lib = capi.lib()
    A, B = shmip_model(), shmip_model()
    keys = ("run_readbacks", "moulin_source_calls", "budget_launches", "budget_copies", "budget_device_bytes", "balance_launches", "fused_relax_launches")
    pi, nv, rows, _ = A.run(4, HDT, moulins=MOULINS, diag_every=2)
    brows, counts = np.zeros((2, 6)), (np.zeros(4, dtype=np.intc), np.zeros(4, dtype=np.intc))
    rc, res = hier_run_bud(B, None, n_steps=4, diag_every=2, rows=brows, counts=counts)
    capi.check(rc)
    B.cur_step += res.steps_done
    assert res.steps_done == 4 and res.n_rows == 2 and list(pi) == list(counts[0]) and list(nv) == list(counts[1])
    assert np.array_equal(rows, brows, equal_nan=True)
    assert [A.hier.get_option(k) for k in keys] == [B.hier.get_option(k) for k in keys]
    assert B.hier.get_option("budget_launches") == 0 and B.hier.get_option("budget_device_bytes") == 0
    assert_same_state(A, B)
    A.close(); B.close()
    # an ensemble
    n = ENS["n"]
    X, Y = ensemble(track=False)[0], ensemble(track=False)[0]
    pi, nv, rows = X.run(3, DT, diag_every=1)
    sch = capi.BatchSchedule(n_steps=3, dt=DT, first_cur_step=1, n_members=n, diag_every=1)
    ypi, ynv, yrows = np.zeros((3, n), dtype=np.intc), np.zeros((3, n), dtype=np.intc), np.zeros((3, n, 6))
    res = capi.BatchRunResult(picard_iters=ypi.ctypes.data_as(C.POINTER(C.c_int)), vcycles=ynv.ctypes.data_as(C.POINTER(C.c_int)),
                              rows=yrows.ctypes.data_as(C.POINTER(C.c_double)))
    capi.check(lib.suhmo_batch_run_bud(Y.batch.h, Y._mp, C.byref(sch), None, None, C.byref(res), Y.batch.stream))
    assert np.array_equal(pi, ypi) and np.array_equal(nv, ynv) and np.array_equal(rows, yrows, equal_nan=True) and res.steps_done == 3
    assert [X.get_option(k) for k in ("batch_launches", "batch_readbacks")] == [Y.get_option(k) for k in ("batch_launches", "batch_readbacks")]
    for k in range(n):
        for nm in ("head", "B", "mR"):
            assert np.array_equal(X.get(k, nm, ghosted=True), Y.get(k, nm, ghosted=True), equal_nan=True), (k, nm)
    X.close(); Y.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_of_the_calls():
    from suhmo_amd import capi, level as lv, model
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT as HDT, DX0, STEP_MODEL, assert_same_state
    lib = capi.lib()
    out = np.full(8 * 10, -77.0)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    # a level: no step yet (no faces: the mass balance's refusal), NULL arguments, a source switch without a source, a rank strip
    G, T = fresh_valley(70, 9, mb.NEUMANN_BC, True), fresh_valley(70, 9, mb.NEUMANN_BC, True)
    mp = C.byref(G._mp)
    assert lib.suhmo_level_water_budget(G.level.h, mp, dp, G.level.stream) == -1 and b"face coefficients" in lib.suhmo_last_error()
    assert lib.suhmo_level_water_budget(G.level.h, None, dp, None) == -1 and lib.suhmo_level_water_budget(G.level.h, mp, None, None) == -1
    assert lib.suhmo_level_water_budget(None, mp, dp, None) == -1
    assert G.timestep(DT) == T.timestep(DT)
    src = params(G._mp, use_moulin_source=1)
    assert lib.suhmo_level_water_budget(G.level.h, C.byref(src), dp, G.level.stream) == -1 and b"SUHMO_F_MSRC" in lib.suhmo_last_error()
    assert b"the level" in lib.suhmo_last_error()
    S = lv.HipLevel(70, 8, G.dx, G.dy, mb.NEUMANN_BC, sw.PHYS, max_box=64, j0=0, ny_global=16)
    assert lib.suhmo_level_water_budget(S.h, mp, dp, S.stream) == -5 and b"strip" in lib.suhmo_last_error()
    S.close()
    assert (out == -77.0).all()
    assert G.timestep(DT) == T.timestep(DT)
    assert same_bits(wb_row(G.water_budget()), wb_row(T.water_budget()))
    # a level that has faces (UpdateOperator) and no melt rate: no time step has run
    st = sy.valley_initial_state(70, 9, 0.05)
    F = model.HipModel(70, 9, st["dx"], st["dy"], mb.NEUMANN_BC, sw.PHYS, MODEL, max_box=64)
    F.set_state(st)
    capi.check(lib.suhmo_level_update_operator(F.level.h, 0, F.level.stream))
    assert lib.suhmo_level_water_budget(F.level.h, C.byref(F._mp), dp, F.level.stream) == -1 and b"SUHMO_F_MR" in lib.suhmo_last_error()
    F.close()
    # an ensemble: whichever member it is; members without a flag are not asked
    B = ensemble()[0]
    n = B.n
    n_l = B.get_option("batch_launches")
    assert lib.suhmo_batch_water_budget(B.batch.h, B._mp, dp, None, B.batch.stream) == -1 and b"member 0" in lib.suhmo_last_error()
    assert lib.suhmo_batch_water_budget(B.batch.h, None, dp, None, None) == -1 and lib.suhmo_batch_water_budget(B.batch.h, B._mp, None, None, None) == -1
    B.timestep(DT)
    B.set_model(4, use_moulin_source=1)
    n_l = B.get_option("batch_launches")
    assert lib.suhmo_batch_water_budget(B.batch.h, B._mp, dp, None, B.batch.stream) == -1 and b"member 4" in lib.suhmo_last_error()
    only = (C.c_int * n)(*[int(k != 4) for k in range(n)])
    assert B.get_option("batch_launches") == n_l and (out == -77.0).all()
    assert lib.suhmo_batch_water_budget(B.batch.h, B._mp, dp, only, B.batch.stream) == 0
    assert (out.reshape(8, 10)[4] == -77.0).all() and not (out.reshape(8, 10)[[0, 1, 2, 3, 5]] == -77.0).any()
    B.close()
    out[:] = -77.0
    # hierarchies
    M, U = shmip_model(), shmip_model()
    for X in (M, U):
        X.moulin_source(**MOULINS)
    hmp = C.byref(M._mp)
    assert lib.suhmo_hier_water_budget(M.hier.h, hmp, dp, M.hier.stream) == -1 and b"face coefficients" in lib.suhmo_last_error()
    assert lib.suhmo_hier_water_budget(M.hier.h, None, dp, None) == -1 and lib.suhmo_hier_water_budget(M.hier.h, hmp, None, None) == -1
    assert lib.suhmo_hier_water_budget(None, hmp, dp, None) == -1
    assert M.timestep(HDT) == U.timestep(HDT)
    assert lib.suhmo_level_water_budget(M.level[1][0].h, hmp, dp, M.hier.stream) == -5 and b"not built" in lib.suhmo_last_error()
    plain = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, dict(STEP_MODEL, use_moulin_source=0), [[(32, 16, 63, 47)]], max_box=16)
    sts = sy.shmip_amrm_states(64, 32, [[(32, 16, 63, 47)]], rough=0.5)
    plain.set_states(sts)
    plain.timestep(HDT)
    assert lib.suhmo_hier_water_budget(plain.hier.h, hmp, dp, plain.hier.stream) == -1 and b"box 0 of level 0" in lib.suhmo_last_error(), "the source switch without a source"
    plain.close()
    S = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, j0=0, ny_global=64)
    W = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, options="shadow=1")
    for X in (S, W):
        assert lib.suhmo_hier_water_budget(X.hier.h, hmp, dp, X.hier.stream) == -5 and b"not built" in lib.suhmo_last_error()
        assert X.hier.get_option("budget_launches") == 0
    S.close(); W.close()
    assert M.hier.get_option("budget_launches") == 0 and (out == -77.0).all(), "nothing was launched, nothing was written"
    assert M.timestep(HDT) == U.timestep(HDT)
    assert_same_state(M, U)
    capi.check(lib.suhmo_hier_water_budget(M.hier.h, hmp, dp, M.hier.stream))
    assert not (out[:10 * M.hier.nlev].reshape(-1, 10)[:, [0, 6, 8, 9]] == -77.0).any() and (out[10 * M.hier.nlev:] == -77.0).all()
    for X in (G, T, M, U):
        X.close()


def test_refusals_of_the_runs_and_a_run_that_fails_midway():
    from suhmo_amd import capi, model
    from tests.test_gpu_hier_run import shmip_model, MOULINS, analytic, REGRID, DT as HDT, DX0, STEP_MODEL, assert_same_state
    lib = capi.lib()
    M, U = shmip_model(), shmip_model()
    rows, nlev = np.full((6, 3, 10), -77.0), np.full(6, -7, dtype=np.intc)
    dp, ip = rows.ctypes.data_as(C.POINTER(C.c_double)), nlev.ctypes.data_as(C.POINTER(C.c_int))

    run_bud = lambda X, bud, moulins=True: hier_run_bud(X, bud, moulins=moulins)

    n_l = M.hier.get_option("fused_relax_launches")
    for bud, word in ((capi.RunBudget(every=0, lev_cap=3, rows=dp, nlev=ip), b"every"), (capi.RunBudget(every=-2, lev_cap=3, rows=dp, nlev=ip), b"every"),
                      (capi.RunBudget(every=1, lev_cap=3, rows=None, nlev=ip), b"rows"), (capi.RunBudget(every=1, lev_cap=3, rows=dp, nlev=None), b"nlev"),
                      (capi.RunBudget(every=1, lev_cap=2, rows=dp, nlev=ip), b"room")):
        bud.n_rows = 99
        rc, res = run_bud(M, bud)
        assert rc == -1 and word in lib.suhmo_last_error() and res.steps_done == 0 and bud.n_rows == 0, (word, lib.suhmo_last_error())
    # the source switch with no forcing of the run to write the source and no source on the boxes: the run's own rule
    rc, res = run_bud(M, capi.RunBudget(every=1, lev_cap=3, rows=dp, nlev=ip), moulins=False)
    assert rc == -1 and b"use_moulin_source" in lib.suhmo_last_error()
    S = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, j0=0, ny_global=64)
    W = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, options="shadow=1")
    for X in (S, W):
        rc, res = run_bud(X, capi.RunBudget(every=1, lev_cap=3, rows=dp, nlev=ip))
        assert rc == -5 and res.steps_done == 0, lib.suhmo_last_error()
        X.close()
    assert (rows == -77.0).all() and (nlev == -7).all() and M.hier.get_option("fused_relax_launches") == n_l and M.hier.get_option("budget_launches") == 0
    # an ensemble
    B = ensemble(track=False)[0]
    n = B.n
    brows = np.full((2, n, 10), -77.0)
    bdp = brows.ctypes.data_as(C.POINTER(C.c_double))
    sch = capi.BatchSchedule(n_steps=2, dt=DT, first_cur_step=1, n_members=n)
    b_l = B.get_option("batch_launches")
    for bud, word in ((capi.RunBudget(every=0, rows=bdp), b"every"), (capi.RunBudget(every=1, rows=None), b"rows")):
        res = capi.BatchRunResult()
        assert lib.suhmo_batch_run_bud(B.batch.h, B._mp, C.byref(sch), None, C.byref(bud), C.byref(res), B.batch.stream) == -1 and word in lib.suhmo_last_error()
        assert res.steps_done == 0 and bud.n_rows == 0
    assert (brows == -77.0).all() and B.get_option("batch_launches") == b_l
    B.close()
    # after the refusals a step is the step of an untouched twin
    for X in (M, U):
        X.moulin_source(**MOULINS)
    assert M.timestep(HDT) == U.timestep(HDT)
    assert_same_state(M, U)
    U.close()
    # a reload that fails at the regrid before step 3 of a tracked caller: two rows are out, n_rows is exact, the caller's setting is back
    M.hier.set_option("track_old_volume", 1)

    def failing(l, k, b):
        raise RuntimeError("no data for the new boxes")

    with pytest.raises(RuntimeError):
        M.run(5, HDT, moulins=MOULINS, regrid_interval=3, reload=failing, balance_every=1, **REGRID)
    assert M.last_run["steps_done"] == 2 and M.last_run["budget"].shape[0] == 2 and list(M.last_run["budget_nlev"]) == [3, 3]
    assert np.isfinite(M.last_run["budget"]).all()
    assert M.hier.get_option("track_old_volume") == 1, "the caller's setting, on the handle the run left"
    M.close()
