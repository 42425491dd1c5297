"""Forcing and diagnostics of an ensemble in the launches of one member (suhmo_batch_time_varying_recharge, suhmo_batch_moulin_source,
suhmo_batch_postproc_partial / _temporal / _table; HipBatchModel.time_varying_recharge, .moulin_source, .postproc_*_all): every member bit for
bit (np.array_equal) what the per-level call on a member handle gives, the oracle where it has the routine, members that are not active left
alone, the launch / read-back counts, and the refusals.

Shapes where the kernels can go wrong rather than the workload's: A = 40 x 24 with boxes of 8 (nx % 64, nx % 16 and ny % 16 all non-zero: a
partial workgroup of columns, partial moulin tiles in both directions, 3 x 2 tiles), B = 96 x 32 with boxes of 16 (the shape of
tests/test_gpu_moulin.py::test_time_varying_recharge_and_timestep_bitwise; 6 x 2 tiles, one and a half workgroups of columns)."""
import os
import sys

import numpy as np
import pytest

from suhmo_amd import synthetic as sy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("A-40x24", 40, 24, 8), ("B-96x32", 96, 32, 16)]
RTOL = 1e-13                     # tests/test_gpu_moulin.py: the device's exp against the C library's, relative to the largest value
# the daily row against its numpy twin daily_row (tools/run_shmip_f.py): the existing suite-F test holds the device's series to the oracle's,
# which is written through that twin, to 1e-9 of the column's scale (tests/test_gpu_timestep.py::test_shmip_f_five_year_series_on_the_device);
# a single row is its own scale.  The sums run in another order on the two sides, nothing else differs.
ROW_RTOL = 1e-9


@pytest.fixture(scope="module")
def hipmodel():
    from suhmo_amd import capi, model
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return model


@pytest.fixture(scope="module")
def runf():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_shmip_f
    return run_shmip_f


def sqrt_surface(st):
    """surface of the sqrt ice sheet over the ghosted level, 1 .. 1500 m (tests/test_gpu_moulin.py)"""
    nx, ny = st["nx"], st["ny"]
    X = (np.arange(-1, nx + 1) + 0.5)[None, :] * st["dx"] + np.zeros((ny + 2, 1))
    return 6.0 * (np.sqrt(X + 5000.0) - np.sqrt(5000.0)) + 1.0 + st["zb"]


def a_batch(hipmodel, n, nx, ny, mb, st, **model):
    m = dict(sy.A3_MODEL, **model)
    return hipmodel.HipBatchModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, [dict(m) for _ in range(n)], max_box=mb)


def load_step_fields(M, seed):
    """what a time step leaves for the diagnostics (fluxes on the x-faces, channelisation degree with its ghosts, melt rate, water pressure),
    loaded through the member handle: the column kernel on a shape no step has to run on"""
    from suhmo_amd import level as lv
    L = M.level
    rng = np.random.default_rng(seed)
    L.set(lv.F_QWX, rng.uniform(-2.0, 0.5, size=(L.ny, L.nx + 1)))
    L.set(lv.F_CD, rng.uniform(0.0, 1.0, size=(L.ny + 2, L.nx + 2)), ghosted=True)
    L.set(lv.F_MR, rng.uniform(0.0, 1.0e-4, size=(L.ny, L.nx)))
    L.set(lv.F_PW, rng.uniform(0.0, 2.0e6, size=(L.ny, L.nx)))


def counters(G):
    return G.get_option("batch_launches"), G.get_option("batch_readbacks")


# ------------------------------------------------------------------ 1. recharge
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_recharge_every_member_is_the_oracles_and_the_level_calls(oracle, hipmodel, shape):
    """5 members, each with its own surface, temperature and background input: member 0 is too cold to melt anywhere (its source term is its
    background), members 1-3 melt over the lower part of the sheet, member 4 everywhere"""
    _, nx, ny, mb = shape
    st = sy.shmip_initial_state(nx, ny)
    n = 5
    zs = [sqrt_surface(st) + 10.0 * k for k in range(n)]
    T_K = np.array([-20.0, 0.5, 2.0, 5.0, 12.5])
    bg = 7.93e-11 * (1.0 + np.arange(n))
    G = a_batch(hipmodel, n, nx, ny, mb, st, use_moulin_source=1)
    T = a_batch(hipmodel, n, nx, ny, mb, st, use_moulin_source=1)
    for k in range(n):
        G.set_surface(k, zs[k])
    l0, r0 = counters(G)
    G.time_varying_recharge(T_K, bg)
    assert counters(G) == (l0 + 1, r0)
    melting = []
    for k in range(n):
        got = G.member(k).level.get(hipmodel.lv.F_MSRC, ghosted=True)
        assert np.array_equal(got, oracle.time_varying_recharge(zs[k], T_K[k], bg[k])), ("oracle", k)
        T.member(k).time_varying_recharge(zs[k], T_K[k], bg[k])
        assert np.array_equal(got, T.member(k).level.get(hipmodel.lv.F_MSRC, ghosted=True)), ("level call", k)
        melting.append(float(np.mean(got > bg[k])))
    print("share of the ghosted box that melts, per member:", melting)
    assert melting[0] == 0.0 and melting[4] == 1.0 and all(0.0 < x < 1.0 for x in melting[1:4])
    # a scalar serves every member; the surface stayed on the device
    G.time_varying_recharge(2.0, 1.0e-10)
    for k in range(n):
        assert np.array_equal(G.member(k).level.get(hipmodel.lv.F_MSRC, ghosted=True), oracle.time_varying_recharge(zs[k], 2.0, 1.0e-10)), k
    G.close(); T.close()


# ------------------------------------------------------------------ 2. moulins
def moulin_lists(nx, ny, dx, dy):
    """lists of 1, 2, 7 and 100 moulins.  The first: one narrow moulin at the centre of cell (3, 3) -- every tile but the one that holds it is
    farther than the underflow distance (39 sigma = 1950 m; the next tiles start 3750 m away) and takes the far-tile skip"""
    lx, ly = nx * dx, ny * dy
    out = [(np.array([[3.5 * dx, 3.5 * dy]]), np.array([50.0]), np.array([90.0]))]
    for n, seed in ((2, 11), (7, 12), (100, 13)):
        rng = np.random.default_rng(seed)
        pos = np.stack([rng.uniform(0.05 * lx, 0.95 * lx, n), rng.uniform(0.05 * ly, 0.95 * ly, n)], axis=1)
        out.append((pos, rng.uniform(150.0, 400.0, n), rng.uniform(0.5, 2.0, n) * 90.0 / n))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_moulin_lists_of_different_length(oracle, hipmodel, shape):
    _, nx, ny, mb = shape
    dx = dy = 312.5                                               # SHMIP's cells (320 x 64 on 100 km x 20 km)
    st = sy.shmip_initial_state(nx, ny, lx=nx * dx, ly=ny * dy)
    lists = moulin_lists(nx, ny, dx, dy)
    n = len(lists)
    tf = np.array([0.75, 1.0, 0.31, 1.6])
    G = a_batch(hipmodel, n, nx, ny, mb, st, use_moulin_source=1)
    T = a_batch(hipmodel, n, nx, ny, mb, st, use_moulin_source=1)
    l0, r0 = counters(G)
    integ = G.moulin_source(lists, tf)
    assert counters(G) == (l0 + 3, r0)
    for k, (pos, sg, fl) in enumerate(lists):
        src = G.get(k, "msrc")
        want_i = T.member(k).moulin_source(pos, sg, fl, tf[k])
        assert np.array_equal(integ[k], want_i), ("integrals against the level call", k)
        assert np.array_equal(src, T.get(k, "msrc")), ("source term against the level call", k)
        src_o, integ_o = oracle.moulin_source(nx, ny, dx, dy, pos, sg, fl, tf[k])
        assert np.max(np.abs(integ[k] - integ_o)) <= RTOL * np.max(integ_o), ("integrals against the oracle", k)
        assert np.max(np.abs(src - src_o)) <= RTOL * np.max(src_o), ("source term against the oracle", k)
        assert abs(src.sum() * dx * dy - tf[k] * fl.sum()) < 1e-11 * fl.sum(), ("delivered flux", k)
    far = G.get(0, "msrc")
    assert np.count_nonzero(far[:, 16:]) == 0 and np.count_nonzero(far[16:, :]) == 0 and np.count_nonzero(far) > 0      # the skipped tiles
    # the scratch is the batch's: a second call with shorter lists and another factor reuses it
    short = [lists[1], lists[0], lists[0], lists[2]]
    integ = G.moulin_source(short, 0.5)
    for k, (pos, sg, fl) in enumerate(short):
        assert np.array_equal(integ[k], T.member(k).moulin_source(pos, sg, fl, 0.5)) and np.array_equal(G.get(k, "msrc"), T.get(k, "msrc")), k
    G.close(); T.close()


# ------------------------------------------------------------------ 3. diagnostics of a mixed ensemble
def mixed_ensemble(hipmodel, runf, nx, ny, mb):
    """on the valley's 6000 m x 1500 m (the bands of the daily row hold cells): 0 the sqrt sheet under suite A's distributed input; 1 the same
    with moulins (ramp 0.8); 2 the valley glacier under the seasonal recharge (suite F: implicit gap-height solve, ice-free cells); 3 suite E's
    valley with the overdeepened bed (ice-free cells, masked gradients, cut-off outside the ice)"""
    lv = hipmodel.lv
    lx, ly = 6000.0, 1500.0
    sq, va, ov = sy.shmip_initial_state(nx, ny, lx, ly), sy.valley_initial_state(nx, ny, 0.05, lx, ly), sy.valley_initial_state(nx, ny, -0.5, lx, ly)
    models = [dict(sy.A3_MODEL, distributed_input=2.5e-8), dict(sy.A3_MODEL, use_moulin_source=1, ramp=0.8, distributed_input=7.93e-11),
              dict(runf.F_MODEL), dict(sy.shmip_e_model("E4"))]
    phys = [sy.A3_PHYS, sy.A3_PHYS, dict(sy.A3_PHYS, A=2.5e-25), dict(sy.E_PHYS, cutOffB=1)]
    states = [sq, sq, va, ov]
    G = hipmodel.HipBatchModel(nx, ny, sq["dx"], sq["dy"], sy.A3_BC, phys, models, max_box=mb, implicit_gap=True)
    for k in range(4):
        G.set_state(k, states[k])
    for k in (2, 3):
        G.member(k).level.set(lv.F_MR, np.full((ny, nx), models[k]["G"] / models[k]["L"]))
    X = (np.arange(-1, nx + 1) + 0.5)[None, :] * va["dx"] + np.zeros((ny + 2, 1))
    G.set_surface(2, 100.0 * np.power(X + 200.0, 0.25) + X / 60.0 - np.power(2.0e10, 0.25) + 1.0)
    dx, dy = sq["dx"], sq["dy"]
    moulins = (np.array([[10.5 * dx, 7.5 * dy], [0.52 * lx, 0.61 * ly], [0.83 * lx, 0.2 * ly]]), np.full(3, 2.0 * dx), np.full(3, 0.3))
    G.moulin_source([None, moulins, None, None], 1.0, active=[0, 1, 0, 0])
    G.time_varying_recharge(4.0, runf.BACKGROUND, active=[0, 0, 1, 0])
    return G, models, states


def test_diagnostics_of_a_mixed_ensemble(hipmodel, runf):
    _, nx, ny, mb = SHAPES[1]
    G, models, states = mixed_ensemble(hipmodel, runf, nx, ny, mb)
    n = G.n
    for step in range(3):
        G.timestep(3600.0)
    assert (states[3]["mask"][1:-1, 1:-1] < 0).sum() > 20 and (states[2]["mask"][1:-1, 1:-1] < 0).sum() > 20        # the ice-free branches are taken
    l0, r0 = counters(G)
    sums, rows, tables = G.postproc_partial_all(), G.postproc_temporal_all(), G.postproc_table_device_all()
    assert counters(G) == (l0 + 3, r0 + 3)
    assert sums.shape == (n, 8, nx) and rows.shape == (n, 6) and tables.shape == (n, nx, 8)
    dx, dy = states[0]["dx"], states[0]["dy"]
    for k in range(n):
        assert np.array_equal(sums[k], G.member(k).postproc_partial(), equal_nan=True), ("partial", k)
        assert np.array_equal(rows[k], G.postproc_temporal(k), equal_nan=True), ("temporal", k)
        assert np.array_equal(tables[k], G.postproc_table_device(k), equal_nan=True), ("table", k)
        m, mask = models[k], G.get(k, "mask")
        if m.get("use_moulin_source", 0):
            src = G.get(k, "msrc") * m["ramp"] + m["distributed_input"]
        else:
            src = np.where(mask > 0.0, m["distributed_input"], 0.0)
        twin = runf.daily_row(0.0, dx, dy, G.get(k, "qwx"), src, G.get(k, "mR"), G.get(k, "Pw"), G.get(k, "Pi"), mask, m["rho_w"])[2:8]
        print("member", k, "daily row", rows[k], "numpy twin", twin)
        assert np.all(np.isfinite(rows[k])), k
        assert np.all(np.abs(rows[k] - twin) <= ROW_RTOL * np.abs(np.array(twin))), (k, rows[k], twin)
    assert sums[3][7].sum() < sums[0][7].sum() == nx * ny                      # fewer cells count where there is no ice
    G.close()


def test_diagnostics_on_a_partial_workgroup_of_columns(hipmodel):
    """shape A (40 columns: one workgroup, partly filled), no step: the fields a step leaves are loaded, members with and without a source
    term and with ice-free cells"""
    _, nx, ny, mb = SHAPES[0]
    lv = hipmodel.lv
    lx, ly = 6000.0, 1500.0
    states = [sy.shmip_initial_state(nx, ny, lx, ly), sy.valley_initial_state(nx, ny, 0.05, lx, ly), sy.valley_initial_state(nx, ny, -0.5, lx, ly)]
    models = [dict(sy.A3_MODEL), dict(sy.A3_MODEL, use_moulin_source=1, ramp=0.7, distributed_input=7.93e-11), dict(sy.A3_MODEL, distributed_input=1.0e-6)]
    G = hipmodel.HipBatchModel(nx, ny, lx / nx, ly / ny, sy.A3_BC, sy.A3_PHYS, models, max_box=mb)
    for k in range(3):
        G.set_state(k, states[k])
        load_step_fields(G.member(k), 60 + k)
    G.member(1).level.set(lv.F_MSRC, np.random.default_rng(5).uniform(0.0, 1.0e-6, size=(ny, nx)))
    sums, rows, tables = G.postproc_partial_all(), G.postproc_temporal_all(), G.postproc_table_device_all()
    for k in range(3):
        assert np.array_equal(sums[k], G.member(k).postproc_partial()), ("partial", k)
        assert np.array_equal(rows[k], G.postproc_temporal(k)), ("temporal", k)
        assert np.array_equal(tables[k], G.postproc_table_device(k)), ("table", k)
        assert np.all(np.isfinite(rows[k])) and np.all(np.isfinite(tables[k])), k
    assert sums[0][7].sum() == nx * ny > sums[2][7].sum() > 0
    G.close()


# ------------------------------------------------------------------ 4. subsets
def test_members_that_are_not_active_are_left_alone(hipmodel):
    _, nx, ny, mb = SHAPES[0]
    lv = hipmodel.lv
    st = sy.shmip_initial_state(nx, ny, lx=nx * 312.5, ly=ny * 312.5)
    n, act = 5, [0, 1, 0, 1, 0]
    G = a_batch(hipmodel, n, nx, ny, mb, st, use_moulin_source=1, distributed_input=0.0)
    T = a_batch(hipmodel, n, nx, ny, mb, st, use_moulin_source=1, distributed_input=0.0)
    zs = sqrt_surface(st)
    sentinel = np.full((ny + 2, nx + 2), -7.0)
    for k in range(n):
        G.set_state(k, st); T.set_state(k, st)
        G.member(k).level.set(lv.F_MSRC, sentinel, ghosted=True)
        if act[k]:
            G.set_surface(k, zs + k)                                # (the others have no surface at all: nobody looks)
    msrc = lambda M, k: M.member(k).level.get(lv.F_MSRC, ghosted=True)
    G.time_varying_recharge([9.0, 3.0, 9.0, 4.0, 9.0], 1.0e-10, active=act)
    for k in range(n):
        if act[k]:
            T.member(k).time_varying_recharge(zs + k, [9.0, 3.0, 9.0, 4.0, 9.0][k], 1.0e-10)
            assert np.array_equal(msrc(G, k), msrc(T, k)), k
        else:
            assert np.array_equal(msrc(G, k), sentinel), k
    lists = moulin_lists(nx, ny, 312.5, 312.5)
    for k in range(n):
        G.member(k).level.set(lv.F_MSRC, sentinel, ghosted=True)
    integ = G.moulin_source([None, lists[2], None, lists[1], None], [9.0, 0.5, 9.0, 0.7, 9.0], active=act)
    for k in range(n):
        if act[k]:
            want = T.member(k).moulin_source(*lists[2 if k == 1 else 1], [0.5, 0.7][k // 2])
            assert np.array_equal(integ[k], want) and np.array_equal(G.get(k, "msrc"), T.get(k, "msrc")), k
        else:
            assert integ[k] is None and np.array_equal(msrc(G, k), sentinel), k
    # the inactive members' entries of a concatenated call are skipped over, not read as somebody else's
    integ2 = G.moulin_source([lists[3], lists[2], lists[0], lists[1], lists[0]], [9.0, 0.5, 9.0, 0.7, 9.0], active=act)
    for k in (1, 3):
        assert np.array_equal(integ2[k], integ[k]) and np.array_equal(G.get(k, "msrc"), T.get(k, "msrc")), k
    for k in (0, 2, 4):
        assert np.array_equal(msrc(G, k), sentinel), k
    # diagnostics: the rows of the other members keep what the caller's array held
    for k in range(n):
        G.member(k).level.set(lv.F_MSRC, np.full((ny + 2, nx + 2), 1.0e-9 * (k + 1)), ghosted=True)
        load_step_fields(G.member(k), 80 + k)
    for name, shape in (("postproc_partial_all", (8, nx)), ("postproc_temporal_all", (6,)), ("postproc_table_device_all", (nx, 8))):
        out = np.full((n,) + shape, -7.0)
        full = getattr(G, name)()
        got = getattr(G, name)(active=act, out=out)
        for k in range(n):
            assert np.array_equal(got[k], full[k] if act[k] else np.full(shape, -7.0), equal_nan=True), (name, k)
    # nobody active: nothing is launched, nothing is read back
    before = counters(G)
    none = [0] * n
    G.time_varying_recharge(1.0, 1.0, active=none)
    assert G.moulin_source([None] * n, 1.0, active=none) == [None] * n
    for name in ("postproc_partial_all", "postproc_temporal_all", "postproc_table_device_all"):
        getattr(G, name)(active=none)
    assert counters(G) == before
    G.close(); T.close()


# ------------------------------------------------------------------ 5. an F-style run
def test_suite_f_style_run_equals_five_models_run_alone(hipmodel, runf):
    """the valley glacier under the seasonal cycle with 5 temperature offsets, 6 steps of 2 h from a summer day: the ensemble forced by one
    recharge call and diagnosed by one temporal call per step against 5 HipModels, each forced (surface uploaded every step) and diagnosed
    through the level calls"""
    _, nx, ny, mb = SHAPES[1]
    lv = hipmodel.lv
    m = dict(runf.F_MODEL)
    phys = dict(sy.A3_PHYS, A=2.5e-25)
    st = sy.valley_initial_state(nx, ny, 0.05, m["lx"], m["ly"])
    X = (np.arange(-1, nx + 1) + 0.5)[None, :] * st["dx"] + np.zeros((ny + 2, 1))
    zs = 100.0 * np.power(X + 200.0, 0.25) + X / 60.0 - np.power(2.0e10, 0.25) + 1.0
    deltas = [runf.DELTA_T[c] for c in ("F1", "F2", "F3", "F4", "F5")]
    n = len(deltas)
    G = hipmodel.HipBatchModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, phys, [dict(m) for _ in range(n)], max_box=mb, implicit_gap=True)
    Ls = [hipmodel.HipModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, phys, m, max_box=mb) for _ in range(n)]
    for k in range(n):
        for M in (G.member(k), Ls[k]):
            M.set_state(st)
            M.level.set(lv.F_MR, np.full((ny, nx), m["G"] / m["L"]))
        G.set_surface(k, zs)
    tm, dt = 200.0 * 86400.0, 7200.0
    seen = set()
    for step in range(6):
        T_K = -16.0 * np.cos(2.0 * np.pi * tm / (365.0 * 24 * 60 * 60.0)) - 5.0 + np.array(deltas)
        G.time_varying_recharge(T_K, runf.BACKGROUND)
        pi, nv = G.timestep(dt)
        rows = G.postproc_temporal_all()
        for k in range(n):
            Ls[k].time_varying_recharge(zs, T_K[k], runf.BACKGROUND)
            assert (pi[k], nv[k]) == Ls[k].timestep(dt), (step, k)
            seen.add((pi[k], nv[k]))
            for nm in ("head", "B", "rhs_h", "msrc"):
                assert np.array_equal(G.get(k, nm), Ls[k].get(nm), equal_nan=True), (step, k, nm)
            assert np.array_equal(rows[k], Ls[k].postproc_temporal(), equal_nan=True), (step, k)
        tm += dt
    print("(picard iterations, V-cycles) seen:", sorted(seen), "last rows:", rows)
    assert np.all(np.isfinite(rows)) and len({tuple(r) for r in rows}) == n          # five different forcings, five different rows
    G.close()
    for L in Ls:
        L.close()


# ------------------------------------------------------------------ 6. counts
@pytest.mark.parametrize("n", [1, 6])
def test_launches_and_readbacks_do_not_grow_with_members(hipmodel, n):
    _, nx, ny, mb = SHAPES[1]
    st = sy.shmip_initial_state(nx, ny, lx=nx * 312.5, ly=ny * 312.5)
    G = a_batch(hipmodel, n, nx, ny, mb, st, use_moulin_source=1, distributed_input=0.0)
    lists = moulin_lists(nx, ny, 312.5, 312.5)
    for k in range(n):
        G.set_state(k, st)
        G.set_surface(k, sqrt_surface(st))
    for _ in range(2):                                            # (the second round: nothing is allocated any more)
        c0 = counters(G)
        G.time_varying_recharge(3.0, 1.0e-10)
        c1 = counters(G)
        G.moulin_source([lists[(k + 1) % 4] for k in range(n)], 1.0)
        c2 = counters(G)
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 0) and c2[0] - c1[0] == 3
    G.timestep(3600.0)
    for name in ("postproc_partial_all", "postproc_temporal_all", "postproc_table_device_all"):
        c0 = counters(G)
        getattr(G, name)()
        c1 = counters(G)
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 1), name
    G.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_name_the_member_and_launch_nothing(hipmodel):
    from suhmo_amd import capi
    _, nx, ny, mb = SHAPES[0]
    st = sy.shmip_initial_state(nx, ny, lx=nx * 312.5, ly=ny * 312.5)
    n = 3
    G = a_batch(hipmodel, n, nx, ny, mb, st, distributed_input=1.0e-9)
    for k in range(n):
        G.set_state(k, st)
    lists = moulin_lists(nx, ny, 312.5, 312.5)
    before = counters(G)

    def refused(what, call):
        with pytest.raises(capi.SuhmoError, match=r"rc=-1: .*member 1\b") as e:
            call()
        print(what, "->", e.value)
        assert counters(G) == before, what

    G.set_surface(0, sqrt_surface(st)); G.set_surface(2, sqrt_surface(st))
    refused("no surface height", lambda: G.time_varying_recharge(1.0, 1.0e-10))
    bad = (lists[1][0], np.array([200.0, 0.0]), lists[1][2])
    refused("sigma <= 0", lambda: G.moulin_source([lists[0], bad, lists[2]], 1.0))
    empty = (np.zeros((0, 2)), np.zeros(0), np.zeros(0))
    refused("no moulins", lambda: G.moulin_source([lists[0], empty, lists[2]], 1.0))
    for name in ("postproc_partial_all", "postproc_temporal_all", "postproc_table_device_all"):
        with pytest.raises(capi.SuhmoError, match=r"rc=-1: .*no time step has run on member 0\b"):
            getattr(G, name)()
        assert counters(G) == before
    # members 0 and 2 may go without member 1
    G.time_varying_recharge(1.0, 1.0e-10, active=[1, 0, 1])
    for k in range(n):
        load_step_fields(G.member(k), 90 + k)
    before = counters(G)
    G.set_model(1, use_moulin_source=1)                           # (member 1 has no source term)
    for name in ("postproc_partial_all", "postproc_temporal_all", "postproc_table_device_all"):
        refused("use_moulin_source without a source term", getattr(G, name))
    G.set_model(1, use_moulin_source=0)
    assert np.all(np.isfinite(G.postproc_temporal_all()[:, 4:]))  # the batch stays usable
    G.close()
