"""The reference's IBC classes on the device (include/suhmo_hip.h, "INITIAL CONDITIONS") against the numpy twin tests/ibc_ref.py: the three bodies
on single levels and on the boxes of generated hierarchies, the ghost sequences of ibc_init and ibc_reload, the regrid and the run with an IBC on
the handle against the twin and against the loops of public calls they replace, and the refusals.

Exact and inexact kinds.  basic, sqrt, the reload bodies of dino and the mask use only + - * / max sqrt: every field with its ghost ring is
compared with np.array_equal.  valley's pow and dino's exp run in the device's libm, whose last bits need not be glibc's: valley's zs, zb, Pi, Pw,
head and dino's initial zb and head are held to  max |device - twin| <= BOUND * max |twin|  per field, everything else of those kinds
(mask, the pattern b == 1e-16, mR, dino's zs / Pi / Pw) exactly -- tests/test_ibc_cpu.py shows that the chosen valley inputs keep every cell 0.03 m
of ice away from the margin, so no cell is left out."""
import re

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import hierlayouts as hl
from tests import ibc_ref as ir
from tests import test_gpu_hier_run as hr

pytestmark = pytest.mark.gpu

# The largest max |device - twin| / max |twin| over every inexact field of every case of this file, measured on an MI355X (ROCm's ocml pow / exp
# against numpy's): written by `pytest tests/test_gpu_ibc.py -s | grep ratio`, the maximum of the printed values.  BOUND = 8 x that: later test
# seeds hit other pow / exp arguments.  Whatever BOUND says, a ratio above 1e-9 is a wrong formula, not rounding.
MEASURED_RATIO = 1.528e-13
BOUND = 8.0 * MEASURED_RATIO
FORMULA_BOUND = 1.0e-9

DOMAIN = dict(basic=(1.0e5, 2.0e4), sqrt=(1.0e5, 2.0e4), valley=(6000.0, 1500.0), dino=(1.0e5, 1.0e5))
PARAMS = dict(basic=[dict(slope=0.02, ice_height=500.0, gap_init=0.02)], sqrt=[dict(slope=0.02), dict(ice_height=500.0, gap_init=0.005)],
              valley=[dict(gamma=g, G=0.05) for g in (0.05, -0.5)], dino=[dict(G=0.05, L=3.0e5)])
INEXACT = dict(basic=(), sqrt=(), valley=("zs", "zb", "Pi", "Pw", "head"), dino=("zb", "head"))


def _rc(e):
    return int(re.search(r"rc=(-?\d+)", str(e)).group(1))


def fid():
    from suhmo_amd import level as lv
    return dict(head=lv.F_PHI, B=lv.F_B, Pi=lv.F_PI, zb=lv.F_ZB, mask=lv.F_MASK, zs=lv.F_ZS, Pw=lv.F_PW, mR=lv.F_MR)


def read(L):
    return {n: L.get(f, ghosted=True) for n, f in fid().items()}


def read_hier(M):
    return [[read(L) for L in bl] for bl in M.level]


def check_state(kind, got, want, what, inexact=None):
    inexact = INEXACT[kind] if inexact is None else inexact
    errs = {}
    for n in ir.NAMES:
        if n in inexact:
            err, ref = float(np.max(np.abs(got[n] - want[n]))), float(np.max(np.abs(want[n])))
            errs[n] = (err, ref)
            if ref > 0.0:                      # (a box without ice: Pi, Pw and zs are 0 everywhere, and must be exactly that)
                print("ratio %.3e %s %s %s" % (err / ref, kind, n, what))
        else:
            assert np.array_equal(got[n], want[n], equal_nan=True), (kind, n, what)      # (sqrt of a ghost cell left of x = -ice_height: NaN on both sides)
    if inexact:
        assert np.array_equal(got["B"] == 1.0e-16, want["B"] == 1.0e-16), (kind, "gap pattern", what)
    for n, (err, ref) in errs.items():
        assert err <= FORMULA_BOUND * ref, (kind, n, what, err, ref, "a wrong formula, not rounding")
    for n, (err, ref) in errs.items():
        assert err <= BOUND * ref, (kind, n, what, err, ref, BOUND)


# ------------------------------------------------------------------ 1. - 4. the bodies against the twin
BCS = dict(none=sy.A3_BC, y=sy.CONV_BC, xy=dict(sy.CONV_BC, periodic=[1, 1]))


@pytest.mark.parametrize("per", sorted(BCS))
@pytest.mark.parametrize("nx,ny", [(62, 2), (70, 5), (130, 9)])
def test_level_init_against_the_twin(nx, ny, per):
    """nx + 2 on, just over and well over a 64-thread edge, ny + 2 off a multiple of 4"""
    from suhmo_amd import model, level as lv
    bc = BCS[per]
    for kind in ir.KINDS:
        lx, ly = DOMAIN[kind]
        M = model.HipModel(nx, ny, lx / nx, ly / ny, bc, sy.A3_PHYS, sy.A3_MODEL, max_box=64)
        for kw in PARAMS[kind]:
            M.init_ibc(model.ibc(kind, **kw))
            want = ir.level_init(kind, ir.params(**kw), ir.geom(0, 0, nx, ny, lx / nx, ly / ny, periodic=bc["periodic"]))
            check_state(kind, read(M.level), want, (nx, ny, per, kw))
            assert np.array_equal(M.level.get(lv.F_ACOEF, ghosted=True), np.zeros((ny + 2, nx + 2))), "aCoef = 0"
        M.close()


@pytest.mark.parametrize("seed", range(12))
def test_hier_init_against_the_twin(seed):
    """boxes with i0, j0 > 0 on the levels of generated layouts: all four periodicities, boxes on domain sides, abutting boxes"""
    from suhmo_amd import model
    bc, boxes = hl.generate(seed)
    assert any(b[0] > 0 and b[1] > 0 for bl in boxes for b in bl)
    for kind in ir.KINDS:
        lx, ly = DOMAIN[kind]
        dx0, dy0 = lx / hl.NX0, ly / hl.NY0
        M = model.HipHierModel(hl.NX0, hl.NY0, dx0, dy0, bc, hl.ADV_PHYS, sy.A3_MODEL, boxes, max_box=16)
        kw = PARAMS[kind][seed % len(PARAMS[kind])]
        n0 = M.hier.get_option("ibc_launches")
        M.init_ibc(model.ibc(kind, **kw))
        assert M.hier.get_option("ibc_launches") - n0 == len(boxes) + 1, "one launch per level"
        want = ir.hier_init(kind, ir.params(**kw), hl.NX0, hl.NY0, dx0, dy0, tuple(bc["periodic"]), boxes)
        got = read_hier(M)
        for l, bl in enumerate(want):
            for k, w in enumerate(bl):
                # (the mask's coarse-fine ghost cells are interpolated from exact +-1 values: exact for every kind)
                check_state(kind, got[l][k], w, (seed, l, k))
        M.close()


# ------------------------------------------------------------------ 5. end to end: the device route leaves the handle as the host route does
def load_host(L, st):
    """the existing host route, with the arrays read back from the device-initialised model: suhmo_level_set_field of every field"""
    from suhmo_amd import level as lv
    f = fid()
    for n in ir.NAMES:
        L.set(f[n], st[n], ghosted=True)
    L.set(lv.F_ACOEF, np.zeros((L.ny, L.nx)))           # as set_state loads it


def small_moulins(lx, ly):
    return dict(positions=[(0.30 * lx, 0.45 * ly), (0.62 * lx, 0.30 * ly)], sigma=[0.02 * lx, 0.015 * lx], flux=[8.0, 5.0])


E_STEP_MODEL = dict(sy.shmip_e_model("E1"), use_moulin_source=1)
E2E = dict(basic=(dict(slope=0.02, ice_height=800.0), sy.A3_PHYS, hr.STEP_MODEL), sqrt=(dict(slope=0.0), sy.A3_PHYS, hr.STEP_MODEL),
           valley=(dict(gamma=0.05, G=E_STEP_MODEL["G"]), sy.E_PHYS, E_STEP_MODEL), dino=(dict(), sy.A3_PHYS, hr.STEP_MODEL))


@pytest.mark.parametrize("kind", ir.KINDS)
def test_level_stepped_after_init_ibc_equals_the_host_route(kind):
    from suhmo_amd import model
    kw, phys, mdl = E2E[kind]
    lx, ly = DOMAIN[kind]
    nx, ny = 64, 16
    A = model.HipModel(nx, ny, lx / nx, ly / ny, sy.A3_BC, phys, mdl, max_box=64)
    B = model.HipModel(nx, ny, lx / nx, ly / ny, sy.A3_BC, phys, mdl, max_box=64)
    A.init_ibc(model.ibc(kind, **kw))
    st = read(A.level)
    B.set_state(st)
    load_host(B.level, st)
    for M in (A, B):
        M.moulin_source(**small_moulins(lx, ly))
    for step in range(2):
        assert A.timestep(hr.DT) == B.timestep(hr.DT), step
    for nm in A.FIELDS:
        assert np.array_equal(A.get(nm, ghosted=True), B.get(nm, ghosted=True), equal_nan=True), (kind, nm)
    assert np.isfinite(A.get("head")).all()
    A.close(); B.close()


@pytest.mark.parametrize("kind", ir.KINDS)
def test_hierarchy_stepped_after_init_ibc_equals_the_host_route(kind):
    from suhmo_amd import model
    kw, phys, mdl = E2E[kind]
    lx, ly = DOMAIN[kind]
    bc, boxes = hl.generate(5)
    mk = lambda: model.HipHierModel(hl.NX0, hl.NY0, lx / hl.NX0, ly / hl.NY0, bc, phys, mdl, boxes, max_box=16)
    A, B = mk(), mk()
    A.init_ibc(model.ibc(kind, **kw))
    sts = read_hier(A)
    B.set_states(sts)
    for l, bl in enumerate(sts):
        for k, st in enumerate(bl):
            load_host(B.level[l][k], st)
            B.set_surface(l, k, st["zs"])
    for M in (A, B):
        M.moulin_source(**small_moulins(lx, ly))
    for step in range(2):
        assert A.timestep(hr.DT) == B.timestep(hr.DT), step
    hr.assert_same_state(A, B, kind)
    A.close(); B.close()


def test_ensemble_of_the_five_valleys_against_five_solo_models():
    from suhmo_amd import model
    cases = sorted(sy.E_GAMMA)
    nx, ny, lx, ly = 64, 16, 6000.0, 1500.0
    models = [dict(sy.shmip_e_model(c), use_moulin_source=1) for c in cases]
    phys = [dict(sy.E_PHYS, cutOffB=sy.E_CUTOFFB[c]) for c in cases]
    G = model.HipBatchModel(nx, ny, lx / nx, ly / ny, sy.A3_BC, phys, models, max_box=64, implicit_gap=True)
    ibcs = [model.ibc("valley", gamma=sy.E_GAMMA[c], G=models[0]["G"]) for c in cases]
    n0 = G.get_option("batch_launches")
    G.init_ibc_all(ibcs)
    assert G.get_option("batch_launches") - n0 == 3, "one launch for the bodies of all members, two for the ghost cells"
    solos = []
    for k, c in enumerate(cases):
        want = ir.level_init("valley", ir.params(gamma=sy.E_GAMMA[c], G=models[0]["G"]), ir.geom(0, 0, nx, ny, lx / nx, ly / ny))
        st = read(G.member(k).level)
        check_state("valley", st, want, ("member", c))
        S = model.HipModel(nx, ny, lx / nx, ly / ny, sy.A3_BC, phys[k], models[k], max_box=64)
        S.set_state(st)
        load_host(S.level, st)
        solos.append(S)
    mo = small_moulins(lx, ly)
    lists = [(mo["positions"], mo["sigma"], mo["flux"])] * len(cases)
    G.moulin_source(lists)
    for S in solos:
        S.moulin_source(**mo)
    for step in range(2):
        pi, nv = G.timestep(models[0]["dt"])
        assert list(zip(pi, nv)) == [S.timestep(models[0]["dt"]) for S in solos], step
    for k, S in enumerate(solos):
        for nm in S.FIELDS:
            assert np.array_equal(G.get(k, nm, ghosted=True), S.get(nm, ghosted=True), equal_nan=True), (cases[k], nm)
        S.close()
    G.close()


# ------------------------------------------------------------------ 6. the reload inside the regrid
def regrid_case(kind):
    """(model on OLD initialised on the device, its states read back, ibc, twin parameters, geometry)"""
    from suhmo_amd import model, level as lv
    if kind == "dino":
        c = ir.ORDER_CASE
        nx0, ny0, dx0, dy0, per = c["geo"]
        kw = dict()
    else:
        lx, ly = DOMAIN[kind]
        nx0, ny0, dx0, dy0, per = 64, 32, lx / 64, ly / 32, (0, 0)
        kw = dict(slope=0.02) if kind == "sqrt" else dict(gamma=-0.1)
    M = model.HipHierModel(nx0, ny0, dx0, dy0, sy.A3_BC, sy.A3_PHYS, hr.STEP_MODEL, hr.OLD, max_box=16)
    ibc = model.ibc(kind, **kw)
    M.init_ibc(ibc)
    if kind == "dino":
        for bl in M.level:
            for L in bl:
                L.set(lv.F_B, np.full((L.ny + 2, L.nx + 2), ir.ORDER_CASE["B"]), ghosted=True)
    return M, read_hier(M), ibc, ir.params(**kw), (nx0, ny0, dx0, dy0, per)


def never(*a, **k):
    raise AssertionError("a field was loaded from the host")


def no_host_loads(monkeypatch):
    """from here to the end of the test every per-box load from the host (suhmo_level_set_field, suhmo_level_put_box: all a reload callback can do)
    raises: the reload of a regrid can only have run on the device"""
    from suhmo_amd import capi
    monkeypatch.setattr(capi.lib(), "suhmo_level_set_field", never, raising=False)
    monkeypatch.setattr(capi.lib(), "suhmo_level_put_box", never, raising=False)


@pytest.mark.parametrize("kind", ["sqrt", "valley", "dino"])
def test_regrid_with_an_ibc_against_the_twin(kind, monkeypatch):
    assert hr.OLD == ir.ORDER_CASE["old"] and hr.GEN == ir.ORDER_CASE["new"]
    M, old, ibc, p, geo = regrid_case(kind)
    M.set_ibc(ibc)
    no_host_loads(monkeypatch)
    n0 = M.hier.get_option("ibc_launches")
    M.regrid(hr.GEN)
    assert M.hier.boxes == hr.GEN
    assert M.hier.get_option("ibc_launches") - n0 == 2 * len(hr.GEN), "the bed / Pi body and the mask body per reloaded level; the count is carried over"
    want = ir.regrid_with_reload(kind, p, *geo, hr.OLD, hr.GEN, old[1:], old[0][0])
    got = read_hier(M)
    inexact = ("zs", "zb", "Pi") if kind == "valley" else ()
    for n in ir.NAMES:
        assert np.array_equal(got[0][0][n], old[0][0][n]), ("level 0 is not touched", n)
    for l, bl in enumerate(want, start=1):
        for k, w in enumerate(bl):
            check_state(kind, got[l][k], w, ("regrid", l, k), inexact=inexact)
    if kind == "dino":
        # level 1 was reloaded BEFORE level 2 interpolated from it: the other order leaves the transferred gap height in this ghost cell
        l, k, jj, ii = ir.ORDER_CASE["where"]
        other = ir.regrid_with_reload(kind, p, *geo, hr.OLD, hr.GEN, old[1:], old[0][0], reload_first=False)
        assert got[l][k]["B"][jj, ii] == 1.0e-16 and other[l - 1][k]["B"][jj, ii] == ir.ORDER_CASE["B"]
    M.close()


@pytest.mark.parametrize("kind", ["sqrt", "dino"])
def test_regrid_with_an_ibc_against_the_public_calls(kind):
    """suhmo_hier_regrid without an IBC, then suhmo_hier_ibc_reload of levels 1, 2: bit for bit the regrid with the IBC wherever level 2 does not
    read reloaded coarse values (sqrt: everywhere) -- and where it does (the dino's ghost cell), the twin's other order"""
    A, old, ibc, p, geo = regrid_case(kind)
    C2, _, _, _, _ = regrid_case(kind)
    A.set_ibc(ibc)
    A.regrid(hr.GEN)
    C2.regrid(hr.GEN)
    C2.set_ibc(ibc)
    n0 = C2.hier.get_option("ibc_launches")
    C2.ibc_reload(1); C2.ibc_reload(2)
    assert C2.hier.get_option("ibc_launches") - n0 == 4
    a, c = read_hier(A), read_hier(C2)
    other = ir.regrid_with_reload(kind, p, *geo, hr.OLD, hr.GEN, old[1:], old[0][0], reload_first=False)
    differ = 0
    for l in range(len(a)):
        for k in range(len(a[l])):
            for n in ir.NAMES:
                if l >= 1:
                    assert np.array_equal(c[l][k][n], other[l - 1][k][n]), (kind, l, k, n)
                differ += int((a[l][k][n] != c[l][k][n]).sum())
    assert differ == (1 if kind == "dino" else 0)
    A.close(); C2.close()


# ------------------------------------------------------------------ 7. the run
def test_run_with_an_ibc_equals_the_per_call_loop(monkeypatch):
    from suhmo_amd import model
    R, L = hr.shmip_model(), hr.shmip_model()
    for M in (R, L):
        M.set_ibc(model.ibc("sqrt"))
    no_host_loads(monkeypatch)
    f = np.ones(6)
    counts, _, log, formed = hr.loop(L, 6, moulin_factor=f, regrid_interval=2, reload=None)
    assert sum(not e["same"] for e in log) == 1 and sum(e["same"] for e in log) >= 1, log
    n0 = R.hier.get_option("ibc_launches")
    pi, nv, _, rlog = R.run(6, hr.DT, moulins=hr.MOULINS, regrid_interval=2, **hr.REGRID)
    assert rlog == log and R.last_run["steps_done"] == 6
    assert R.hier.get_option("ibc_launches") - n0 == 2 * (R.hier.nlev - 1)
    hr.assert_same_counts(pi, nv, counts)
    hr.assert_same_state(R, L)
    R.close(); L.close()


VALLEY_OLD = [[(32, 16, 63, 47)]]


def test_seasonal_run_goes_on_when_the_ibc_brings_the_surface(monkeypatch):
    """T_K, a field list without the surface height and no reload: valley's reload body writes SUHMO_F_ZS on every new box"""
    from suhmo_amd import model, level as lv
    lx, ly = DOMAIN["valley"]
    mdl = dict(sy.shmip_e_model("E1"), use_moulin_source=1, distributed_input=0.0, ramp=1.0)
    M = model.HipHierModel(64, 32, lx / 64, ly / 32, sy.A3_BC, sy.E_PHYS, mdl, VALLEY_OLD, max_box=16)
    ibc = model.ibc("valley", gamma=0.05, G=mdl["G"])
    M.init_ibc(ibc)
    M.set_ibc(ibc)
    pi0 = read(M.level[0][0])["Pi"][1:-1, 1:-1]
    lo, hi = np.quantile(pi0[pi0 > 0], [0.55, 0.8])
    spec = [dict(name="Pi", vmin=float(lo), vmax=float(hi), grow=0, cap_level=0)]
    no_host_loads(monkeypatch)
    _, _, _, log = M.run(4, mdl["dt"], T_K=hr.T_K, background=hr.BACKGROUND, regrid_interval=2, fields=hr.NO_ZS, tag_specs=spec,
                         params=hr.PARAMS, max_level=1)
    assert M.last_run["steps_done"] == 4 and [e["same"] for e in log] == [False] and M.hier.boxes != VALLEY_OLD
    for k, b in enumerate(M.hier.boxes[0]):
        g = ir.box_geoms(64, 32, lx / 64, ly / 32, (0, 0), 1, [b])[0]
        X, Y = ir.positions(g)
        S = ir._valley(ir.params(gamma=0.05), X, Y - 750.0)[0]
        zs = M.level[1][k].get(lv.F_ZS, ghosted=True)
        assert np.max(np.abs(zs - S)[1:-1, 1:-1]) <= FORMULA_BOUND * np.max(np.abs(S)), k
    assert all(np.isfinite(M.get(l, k, "head")).all() for l, bl in enumerate(M.level) for k in range(len(bl)))
    M.close()


def test_seasonal_run_ends_at_the_regrid_when_the_ibc_does_not_bring_the_surface():
    from suhmo_amd import capi, model
    R = hr.shmip_model(mdl=hr.SEASON_MODEL)
    hr.load_season_surface(R)
    R.set_ibc(model.ibc("sqrt"))
    with pytest.raises(capi.SuhmoError) as e:
        R.run(4, hr.DT, T_K=hr.T_K, background=hr.BACKGROUND, regrid_interval=2, fields=hr.NO_ZS, **hr.REGRID)
    assert _rc(e.value) == -1 and "SUHMO_F_ZS" in str(e.value) and "level 1, box 0" in str(e.value)
    assert R.last_run["steps_done"] == 2 and R.hier.boxes == hr.GEN
    R.close()


# ------------------------------------------------------------------ 8. refusals
def bad_ibcs():
    from suhmo_amd import model
    unknown, nogap = model.ibc("sqrt"), model.ibc("sqrt", gap_init=0.0)
    unknown.kind = 7
    return [unknown, nogap, None]


def test_level_refusals_leave_the_model_as_it_was():
    import ctypes as C
    from suhmo_amd import capi, model, level as lv
    nx, ny = 64, 16
    mk = lambda **kw: model.HipModel(nx, ny, 1.0e5 / nx, 2.0e4 / ny, sy.A3_BC, sy.A3_PHYS, hr.STEP_MODEL, max_box=64, **kw)
    A, B = mk(), mk()
    for M in (A, B):
        M.init_ibc(model.ibc("sqrt"))
    for bad in bad_ibcs():
        with pytest.raises(capi.SuhmoError) as e:
            A.init_ibc(bad)
        assert _rc(e.value) == -1
    S = mk(j0=0, ny_global=2 * ny)
    with pytest.raises(capi.SuhmoError) as e:
        S.init_ibc(model.ibc("sqrt"))
    assert _rc(e.value) == -5
    S.close()
    # a patch of a nested hierarchy (suhmo_amr_*: the fine level as HipAmr2 creates it) and a box of a hierarchy of box unions: rc -5, nothing written.
    # (The remaining rc -5 case, levels dealt to the ranks, needs more than one rank and is not reached here.)
    good = model.ibc("sqrt")
    P = lv.HipLevel(32, 16, 0.5e5 / nx, 1.0e4 / ny, sy.A3_BC, sy.A3_PHYS, alpha=0.0, beta=-1.0, max_box=64, j0=8, ny_global=2 * ny, i0=16, nx_global=2 * nx)
    H = hr.shmip_model()
    for L in (P, H.level[1][0], H.level[2][1]):
        before = {f: np.random.default_rng([11, f]).uniform(size=(L.ny + 2, L.nx + 2)) for f in (lv.F_ZB, lv.F_MASK, lv.F_PI, lv.F_B)}
        for f, a in before.items():
            L.set(f, a, ghosted=True)
        assert capi.lib().suhmo_level_ibc_init(L.h, C.byref(good), L.stream) == -5
        assert "not built" in capi.lib().suhmo_last_error().decode()
        for f, a in before.items():
            assert np.array_equal(L.get(f, ghosted=True), a), f
    P.close(); H.close()
    # ... while a whole level written with i0 = 0 and nx_global = nx (as a hierarchy's base may be) is a whole level
    W = lv.HipLevel(nx, ny, 1.0e5 / nx, 2.0e4 / ny, sy.A3_BC, sy.A3_PHYS, alpha=0.0, beta=-1.0, max_box=64, i0=0, nx_global=nx)
    capi.check(capi.lib().suhmo_level_ibc_init(W.h, C.byref(good), W.stream))
    check_state("sqrt", read(W), ir.level_init("sqrt", ir.params(), ir.geom(0, 0, nx, ny, 1.0e5 / nx, 2.0e4 / ny)), "nx_global = nx")
    W.close()
    for M in (A, B):
        M.moulin_source(**small_moulins(1.0e5, 2.0e4))
    assert A.timestep(hr.DT) == B.timestep(hr.DT)
    for nm in A.FIELDS:
        assert np.array_equal(A.get(nm, ghosted=True), B.get(nm, ghosted=True)), nm
    A.close(); B.close()


def test_hierarchy_refusals_leave_the_model_as_it_was():
    from suhmo_amd import capi, model
    good = model.ibc("sqrt")
    A, B = hr.shmip_model(), hr.shmip_model()
    with pytest.raises(capi.SuhmoError) as e:
        A.ibc_reload(1)
    assert _rc(e.value) == -1, "no IBC on the handle"
    for bad in bad_ibcs():
        with pytest.raises(capi.SuhmoError) as e:
            A.init_ibc(bad)
        assert _rc(e.value) == -1
    for bad in bad_ibcs()[:2]:
        with pytest.raises(capi.SuhmoError) as e:
            A.set_ibc(bad)
        assert _rc(e.value) == -1
    A.set_ibc(good)
    for level in (0, -1, 3):
        with pytest.raises(capi.SuhmoError) as e:
            A.ibc_reload(level)
        assert _rc(e.value) == -1, level
    A.set_ibc(None)
    with pytest.raises(capi.SuhmoError) as e:
        A.ibc_reload(1)
    assert _rc(e.value) == -1, "set_ibc(None) clears it"
    strips = dict(j0=0, ny_global=64)
    for kw in (strips, dict(options="shadow=1")):
        S = model.HipHierModel(64, 32, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS, sy.A3_MODEL, [[(32, 16, 63, 47)]], max_box=16, **kw)
        with pytest.raises(capi.SuhmoError) as e:
            S.init_ibc(good)
        assert _rc(e.value) == -5, kw
        S.set_ibc(good)
        with pytest.raises(capi.SuhmoError) as e:
            S.ibc_reload(1)
        assert _rc(e.value) == -5, kw
        S.close()
    for M in (A, B):
        M.moulin_source(**hr.MOULINS)
    assert A.timestep(hr.DT) == B.timestep(hr.DT)
    hr.assert_same_state(A, B)
    A.close(); B.close()


def test_batch_refusals_leave_the_members_as_they_were():
    from suhmo_amd import capi, model
    nx, ny = 64, 16
    mk = lambda: model.HipBatchModel(nx, ny, 1.0e5 / nx, 2.0e4 / ny, sy.A3_BC, sy.A3_PHYS, [hr.STEP_MODEL] * 3, max_box=64)
    A, B = mk(), mk()
    rows = [model.ibc("sqrt", slope=s) for s in (0.0, 0.01, 0.02)]
    for G in (A, B):
        G.init_ibc_all(rows)
    with pytest.raises(capi.SuhmoError) as e:
        A.init_ibc_all([rows[0], model.ibc("basic"), rows[2]])
    assert _rc(e.value) == -1, "mixed kinds"
    A.init_ibc_all([rows[0], model.ibc("basic"), rows[2]], active=[1, 0, 1])      # (the kinds of the ACTIVE members are equal)
    A.init_ibc_all([rows[0], bad_ibcs()[0], rows[2]], active=[1, 0, 1])
    with pytest.raises(capi.SuhmoError) as e:
        A.init_ibc_all([rows[0], bad_ibcs()[1], rows[2]])
    assert _rc(e.value) == -1
    assert capi.lib().suhmo_batch_ibc_init(A.batch.h, None, None, A.batch.stream) == -1
    mo = small_moulins(1.0e5, 2.0e4)
    for G in (A, B):
        G.moulin_source([(mo["positions"], mo["sigma"], mo["flux"])] * 3)
    assert A.timestep(hr.DT) == B.timestep(hr.DT)
    for k in range(3):
        for nm in A.FIELDS:
            assert np.array_equal(A.get(k, nm, ghosted=True), B.get(k, nm, ghosted=True)), (k, nm)
    A.close(); B.close()
