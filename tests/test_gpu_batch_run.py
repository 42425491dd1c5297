"""The time loop of an ensemble in one call (suhmo_batch_run, HipBatchModel.run; the daily row finished on the device by
d_postproc_temporal_row): bit for bit (np.array_equal; rows with equal_nan) a twin batch driven step by step through the calls that were
there before -- time_varying_recharge / moulin_source, set_model(ramp), timestep, postproc_partial_all + the host function
suhmo_postproc_temporal -- in fields, ghost rings, Picard and V-cycle counts of every step and rows; members that are not active left alone;
the launch and read-back counts; two runs against one; the row body alone on a level; the refusals.

Shapes (tests/test_gpu_batch_forcing.py): A = 40 x 24 with boxes of 8 (a partly filled workgroup of columns, partial moulin tiles), B = 96 x 32
with boxes of 16."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from suhmo_amd import synthetic as sy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("A-40x24", 40, 24, 8), ("B-96x32", 96, 32, 16)]
IDS = [s[0] for s in SHAPES]
STEP_FIELDS = ("head", "B", "mR", "Re", "Pw", "qwx", "qwy", "cd", "rhs_h")
LX, LY = 6000.0, 1500.0                  # the valley: the three bands of the daily row hold cells at both shapes


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


def valley_surface(nx, ny):
    X = (np.arange(-1, nx + 1) + 0.5)[None, :] * (LX / nx) + np.zeros((ny + 2, 1))
    return 100.0 * np.power(X + 200.0, 0.25) + X / 60.0 - np.power(2.0e10, 0.25) + 1.0


def short_valley(nx, ny):
    """the valley glacier ending at x = 5000 m: no ice (Pi = 0, mask -1, the gap of ice-free cells, head = bed) beyond, so the band
    5100 m < x < 5400 m of the daily row holds no cell that counts and its mean is 0 / 0"""
    st = sy.valley_initial_state(nx, ny, 0.05, LX, LY)
    X = (np.arange(-1, nx + 1) + 0.5)[None, :] * st["dx"] + np.zeros((ny + 2, 1))
    off = X > 5000.0
    st = dict(st)
    st["Pi"] = np.where(off, 0.0, st["Pi"]); st["mask"] = np.where(off, -1.0, st["mask"]); st["B"] = np.where(off, 1.0e-16, st["B"])
    st["head"] = np.where(off, np.maximum(st["zb"], 0.0), st["head"])
    return st


def seasonal_pair(hipmodel, runf, nx, ny, mb, n=5, short=(4,), surfaces=None):
    """two equal ensembles of suite F's model (seasonal recharge, implicit gap-height solve, ice-free cells); members in `short` on the short
    valley.  surfaces: the members of the FIRST that get a surface height (default all; the twin always gets all)"""
    lv = hipmodel.lv
    m = dict(runf.F_MODEL)
    phys = dict(sy.A3_PHYS, A=2.5e-25)
    full, cut = sy.valley_initial_state(nx, ny, 0.05, LX, LY), short_valley(nx, ny)
    zs = valley_surface(nx, ny)
    pair = []
    for which in range(2):
        G = hipmodel.HipBatchModel(nx, ny, full["dx"], full["dy"], sy.A3_BC, phys, [dict(m) for _ in range(n)], max_box=mb, implicit_gap=True)
        for k in range(n):
            G.set_state(k, cut if k in short else full)
            G.member(k).level.set(lv.F_MR, np.full((ny, nx), m["G"] / m["L"]))
            if which == 1 or surfaces is None or k in surfaces:
                G.set_surface(k, zs + 3.0 * k)
        pair.append(G)
    return pair


def seasonal_schedule(runf, n_steps, n):
    """from "melts nowhere" (the warmest member at -20 + 4 K against a surface of at least 1 m) to "melts everywhere" (the coldest at +14 K: the
    surface stays below 14 / 0.0075 = 1867 m), a background per member"""
    T_K = np.linspace(-20.0, 14.0, n_steps)[:, None] + np.linspace(0.0, 4.0, n)[None, :]
    bg = runf.BACKGROUND * (1.0 + 0.25 * np.arange(n))[None, :] + np.zeros((n_steps, 1))
    return np.ascontiguousarray(T_K), np.ascontiguousarray(bg)


def drive_twin(T, n_steps, dt, T_K=None, background=None, moulins=None, moulin_factor=None, ramp=None, diag_every=0):
    """the per-call loop: what a user of an ensemble wrote before the run existed"""
    pis, nvs, rows = [], [], []
    for k in range(n_steps):
        if T_K is not None:
            T.time_varying_recharge(T_K[k], background[k])
        if moulins is not None:
            T.moulin_source(moulins, moulin_factor[k])
        if ramp is not None:
            for q in range(T.n):
                T.set_model(q, ramp=float(ramp[k]))
        p, v = T.timestep(dt)
        pis.append(p); nvs.append(v)
        if diag_every and (k + 1) % diag_every == 0:
            sums = T.postproc_partial_all()
            rows.append([T.member(q).postproc_temporal_host(sums[q]) for q in range(T.n)])
    return np.array(pis), np.array(nvs), np.array(rows).reshape(-1, T.n, 6)


def same_member(G, T, k, what, source=True):
    for nm in STEP_FIELDS + (("msrc",) if source else ()):
        assert np.array_equal(G.get(k, nm), T.get(k, nm), equal_nan=True), (what, k, nm)
    for nm in ("head", "B", "cd") + (("msrc",) if source else ()):
        assert np.array_equal(G.get(k, nm, ghosted=True), T.get(k, nm, ghosted=True), equal_nan=True), (what, k, nm, "ghost ring")


def counters(G):
    return G.get_option("batch_launches"), G.get_option("batch_readbacks")


# ------------------------------------------------------------------ 1. the seasonal recharge
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_seasonal_recharge_run_equals_the_per_call_loop(hipmodel, runf, shape):
    _, nx, ny, mb = shape
    n, n_steps, dt = 5, 12, 7200.0
    G, T = seasonal_pair(hipmodel, runf, nx, ny, mb, n)
    T_K, bg = seasonal_schedule(runf, n_steps, n)
    pi, nv, rows = G.run(n_steps, dt, T_K=T_K, background=bg, diag_every=4)
    tpi, tnv, trows = drive_twin(T, n_steps, dt, T_K=T_K, background=bg, diag_every=4)
    print("picard iterations per step:\n", pi, "\nV-cycles per step:\n", nv, "\nrows of the last day:\n", rows[-1])
    assert pi.shape == (n_steps, n) and rows.shape == (3, n, 6) and G.cur_step == T.cur_step == n_steps
    assert np.array_equal(pi, tpi) and np.array_equal(nv, tnv) and pi.min() >= 1
    for k in range(n):
        same_member(G, T, k, "after the run")
    assert np.array_equal(rows, trows, equal_nan=True)
    # the schedule did what it says: nothing melts on the first step's forcing, everything on the last's; the short valley's upper band is
    # empty (NaN, equal on both sides), every other value is a number
    zs0 = valley_surface(nx, ny)
    assert np.all(0.01 / 86400.0 * (T_K[0, n - 1] - 0.0075 * (zs0 + 3.0 * (n - 1))) < 0.0) and np.all(0.01 / 86400.0 * (T_K[-1, 0] - 0.0075 * zs0) > 0.0)
    assert np.all(G.get(0, "msrc") > bg[-1, 0])
    assert np.all(np.isnan(rows[:, 4, 3])) and np.all(np.isnan(trows[:, 4, 3]))
    fin = np.ones((3, n, 6), dtype=bool); fin[:, 4, 3] = False
    assert np.all(np.isfinite(rows[fin]))
    assert len({tuple(r) for r in rows[-1][:, [0, 4, 5]].tolist()}) == n                 # five forcings, five rows
    G.close(); T.close()


# ------------------------------------------------------------------ 2. moulins with a time factor and a ramp
def moulin_lists(nx, ny, dx, dy):
    lx, ly = nx * dx, ny * dy
    out = [(np.array([[3.5 * dx, 3.5 * dy]]), np.array([2.0 * dx]), np.array([0.3]))]
    for n, seed in ((2, 11), (7, 12)):
        rng = np.random.default_rng(seed)
        pos = np.stack([rng.uniform(0.05 * lx, 0.95 * lx, n), rng.uniform(0.05 * ly, 0.95 * ly, n)], axis=1)
        out.append((pos, rng.uniform(1.5 * dx, 4.0 * dx, n), rng.uniform(0.5, 2.0, n) * 0.3 / n))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_moulin_schedule_with_time_factor_and_ramp(hipmodel, shape):
    _, nx, ny, mb = shape
    st = sy.shmip_initial_state(nx, ny, LX, LY)
    lists = moulin_lists(nx, ny, st["dx"], st["dy"])
    n, n_steps, dt = len(lists), 8, 3600.0
    m = dict(sy.A3_MODEL, use_moulin_source=1, distributed_input=7.93e-11)
    pair = []
    for _ in range(2):
        G = hipmodel.HipBatchModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, [dict(m) for _ in range(n)], max_box=mb)
        for k in range(n):
            G.set_state(k, st)
        pair.append(G)
    G, T = pair
    # max(1 - runoff sin(2 pi t / day), 0) with a runoff factor per member; all reach 0 on step 2 (the source term is 0 there), member 1 again
    phase = np.sin(2.0 * np.pi * (np.arange(n_steps) + 0.0) / 8.0)
    tf = np.maximum(1.0 - np.array([1.0, 1.5, 1.0])[None, :] * phase[:, None], 0.0)
    assert np.all(tf[2] == 0.0) and np.count_nonzero(tf == 0.0) > 3 and tf.max() > 2.0
    ramp = np.linspace(0.25, 1.0, n_steps)
    pi, nv, rows = G.run(n_steps, dt, moulins=lists, moulin_factor=tf, ramp=ramp, diag_every=2)
    tpi, tnv, trows = drive_twin(T, n_steps, dt, moulins=lists, moulin_factor=tf, ramp=ramp, diag_every=2)
    print("picard iterations per step:\n", pi, "\nrows of the last day:\n", rows[-1])
    assert np.array_equal(pi, tpi) and np.array_equal(nv, tnv) and pi.min() >= 1
    for k in range(n):
        same_member(G, T, k, "after the run")
        assert G.member(k).model["ramp"] == T.member(k).model["ramp"] == 1.0
    assert rows.shape == (4, n, 6) and np.array_equal(rows, trows, equal_nan=True) and np.all(np.isfinite(rows))
    assert np.all(rows[0][:, 4] < rows[-1][:, 4])                 # the recharge follows ramp x factor
    G.close(); T.close()


# ------------------------------------------------------------------ 3. implicit gap solve, RelaxSolver at the bottom
@pytest.mark.parametrize("kind", ["implicit_gap", "bottom_solver"])
def test_run_with_implicit_gap_and_with_relax_solver(hipmodel, kind):
    _, nx, ny, mb = SHAPES[1]
    sq, va = sy.shmip_initial_state(nx, ny, LX, LY), sy.valley_initial_state(nx, ny, 0.05, LX, LY)
    if kind == "implicit_gap":                                     # two implicit members (two betas of the gap operator) and an explicit one
        models = [dict(sy.shmip_e_model("E1")), dict(sy.shmip_e_model("E1"), diffFactor=0.5), dict(sy.A3_MODEL, distributed_input=2.5e-8)]
        phys = [dict(sy.E_PHYS, cutOffB=1), dict(sy.E_PHYS, cutOffB=1), sy.A3_PHYS]
        states, opts = [va, va, sq], dict(implicit_gap=True)
    else:
        models = [dict(sy.A3_MODEL, distributed_input=2.5e-8), dict(sy.A3_MODEL, distributed_input=5.79e-9)]
        phys, states, opts = [sy.A3_PHYS, sy.A3_PHYS], [sq, sq], dict(bottom_solver=True)
    n = len(models)
    pair = []
    for _ in range(2):
        G = hipmodel.HipBatchModel(nx, ny, sq["dx"], sq["dy"], sy.A3_BC, phys, models, max_box=mb, **opts)
        for k in range(n):
            G.set_state(k, states[k])
            if models[k].get("use_impl_diff"):
                G.member(k).level.set(hipmodel.lv.F_MR, np.full((ny, nx), models[k]["G"] / models[k]["L"]))
        pair.append(G)
    G, T = pair
    pi, nv, rows = G.run(6, 3600.0, diag_every=3)
    tpi, tnv, trows = drive_twin(T, 6, 3600.0, diag_every=3)
    print(kind, "picard iterations per step:\n", pi, "\nV-cycles:\n", nv)
    assert np.array_equal(pi, tpi) and np.array_equal(nv, tnv) and pi.min() >= 1
    for k in range(n):
        same_member(G, T, k, kind, source=False)
    assert rows.shape == (2, n, 6) and np.array_equal(rows, trows, equal_nan=True)
    if kind == "implicit_gap":
        assert G.get_option("batch_gap_member_cycles") == T.get_option("batch_gap_member_cycles") > 0
    else:
        assert G.get_option("bottom_solver_iterations") == T.get_option("bottom_solver_iterations") > 0
    G.close(); T.close()


# ------------------------------------------------------------------ 4. an active subset
def test_members_that_are_not_active_are_left_alone(hipmodel, runf):
    _, nx, ny, mb = SHAPES[0]
    lv = hipmodel.lv
    n, act, n_steps = 5, [0, 1, 0, 1, 0], 6
    G, T = seasonal_pair(hipmodel, runf, nx, ny, mb, n, short=(3,), surfaces=(1, 3))
    sentinel = np.full((ny + 2, nx + 2), -7.0)
    for k in range(n):
        G.member(k).level.set(lv.F_MSRC, sentinel, ghosted=True)
    before = {k: {nm: G.get(k, nm, ghosted=True) for nm in ("head", "B", "Pi", "mask", "mR")} for k in range(n) if not act[k]}
    T_K, bg = seasonal_schedule(runf, n_steps, n)
    rows = np.full((2, n, 6), -7.0)
    pi, nv, got = G.run(n_steps, 7200.0, T_K=T_K, background=bg, diag_every=3, active=act, rows=rows)
    tpi, tnv, trows = drive_twin(T, n_steps, 7200.0, T_K=T_K, background=bg, diag_every=3)
    assert got is rows
    for k in range(n):
        if act[k]:
            same_member(G, T, k, "active")
            assert np.array_equal(pi[:, k], tpi[:, k]) and np.array_equal(nv[:, k], tnv[:, k])
            assert np.array_equal(rows[:, k], trows[:, k], equal_nan=True), k
        else:
            for nm, a in before[k].items():
                assert np.array_equal(G.get(k, nm, ghosted=True), a), (k, nm)
            assert np.array_equal(G.member(k).level.get(lv.F_MSRC, ghosted=True), sentinel), k
            assert np.all(pi[:, k] == 0) and np.all(nv[:, k] == 0) and np.all(rows[:, k] == -7.0), k
    assert np.all(np.isnan(rows[:, 3, 3]))                         # (the short valley is among the active ones)
    # nobody active: nothing is launched, nothing is read back, no step is counted
    c0, step0 = counters(G), G.cur_step
    G.run(n_steps, 7200.0, T_K=T_K, background=bg, diag_every=3, active=[0] * n, rows=rows)
    assert counters(G) == c0 and G.cur_step == step0
    G.close(); T.close()


# ------------------------------------------------------------------ 5. counters
@pytest.mark.parametrize("n", [1, 6])
def test_a_runs_diagnostics_are_one_readback_and_one_launch_per_row(hipmodel, runf, n):
    _, nx, ny, mb = SHAPES[0]
    n_steps = 6
    T_K, bg = seasonal_schedule(runf, n_steps, n)
    per_row = []
    for diag_every in (1, 3):
        G, T = seasonal_pair(hipmodel, runf, nx, ny, mb, n, short=())
        g0, t0 = counters(G), counters(T)
        pi, nv, rows = G.run(n_steps, 7200.0, T_K=T_K, background=bg, diag_every=diag_every)
        drive_twin(T, n_steps, 7200.0, T_K=T_K, background=bg, diag_every=diag_every)
        g1, t1 = counters(G), counters(T)
        n_rows = n_steps // diag_every
        run_l, run_r, twin_l, twin_r = g1[0] - g0[0], g1[1] - g0[1], t1[0] - t0[0], t1[1] - t0[1]
        print("n", n, "diag_every", diag_every, "run: launches", run_l, "read-backs", run_r, " per-call loop: launches", twin_l, "read-backs", twin_r)
        assert rows.shape[0] == n_rows
        assert run_r == (twin_r - n_rows) + 1                      # the twin's read-backs are its solves' and Picard tests' + one per row
        assert run_l == twin_l + n_rows
        per_row.append(run_r)
        G.close(); T.close()
    assert per_row[0] == per_row[1]                                # whatever diag_every


# ------------------------------------------------------------------ 6. two runs against one
def test_two_consecutive_runs_equal_one(hipmodel, runf):
    _, nx, ny, mb = SHAPES[0]
    n = 3
    G, T = seasonal_pair(hipmodel, runf, nx, ny, mb, n, short=(2,))
    T_K, bg = seasonal_schedule(runf, 12, n)
    a = G.run(6, 7200.0, T_K=T_K[:6], background=bg[:6], diag_every=3)
    assert G.cur_step == 6
    b = G.run(6, 7200.0, T_K=T_K[6:], background=bg[6:], diag_every=3)
    one = T.run(12, 7200.0, T_K=T_K, background=bg, diag_every=3)
    assert G.cur_step == T.cur_step == 12
    for q in range(3):
        assert np.array_equal(np.concatenate([a[q], b[q]]), one[q], equal_nan=True), q
    for k in range(n):
        same_member(G, T, k, "6 + 6 steps against 12")
    G.close(); T.close()


# ------------------------------------------------------------------ 7. the row body alone, on a level
def load_step_fields(M, seed, holes):
    lv_ = __import__("suhmo_amd.level", fromlist=["level"])
    L = M.level
    rng = np.random.default_rng(seed)
    L.set(lv_.F_QWX, rng.uniform(-2.0, 0.5, size=(L.ny, L.nx + 1)))
    L.set(lv_.F_CD, rng.uniform(0.0, 1.0, size=(L.ny + 2, L.nx + 2)), ghosted=True)
    L.set(lv_.F_MR, rng.uniform(0.0, 1.0e-4, size=(L.ny, L.nx)))
    L.set(lv_.F_PW, rng.uniform(0.0, 2.0e6, size=(L.ny, L.nx)))
    if holes:
        L.set(lv_.F_MASK, np.where(rng.uniform(size=(L.ny + 2, L.nx + 2)) < 0.3, -1.0, 1.0), ghosted=True)


@pytest.mark.parametrize("case", [("4x4-no-band", 4, 4, 4, 4.0, 4.0, False), ("40x24-valley", 40, 24, 8, LX, LY, True), ("96x32-valley", 96, 32, 16, LX, LY, True),
                                  ("136x8-one-band", 136, 8, 8, 1360.0, 80.0, False)], ids=lambda c: c[0])
def test_row_body_on_a_level_is_the_host_function(hipmodel, case):
    _, nx, ny, mb, lx, ly, holes = case
    st = sy.shmip_initial_state(nx, ny, lx, ly)
    M = hipmodel.HipModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, dict(sy.A3_MODEL, distributed_input=2.5e-8), max_box=mb)
    M.set_state(st)
    load_step_fields(M, nx, holes)
    dev, host = M.postproc_temporal_device(), M.postproc_temporal()
    print(case[0], "device", dev, "host", host)
    assert np.array_equal(dev, host, equal_nan=True)
    bands = np.isnan(host[1:4])
    assert list(bands) == {"4x4-no-band": [True] * 3, "136x8-one-band": [False, True, True]}.get(case[0], [False] * 3)
    assert np.all(np.isfinite(dev[[0, 4, 5]]))
    M.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals_launch_nothing(hipmodel, runf):
    from suhmo_amd import capi
    _, nx, ny, mb = SHAPES[0]
    n = 3
    G, T = seasonal_pair(hipmodel, runf, nx, ny, mb, n, short=(), surfaces=(0, 2))
    T.close()
    T_K, bg = seasonal_schedule(runf, 4, n)
    st = sy.shmip_initial_state(nx, ny, LX, LY)
    lists = moulin_lists(nx, ny, st["dx"], st["dy"])
    before, step0 = counters(G), G.cur_step

    def refused(what, match, call, exc=capi.SuhmoError):
        with pytest.raises(exc, match=match) as e:
            call()
        print(what, "->", e.value)
        assert counters(G) == before and G.cur_step == step0, what

    refused("no surface height", r"rc=-1: .*member 1\b", lambda: G.run(4, 7200.0, T_K=T_K, background=bg, diag_every=2))
    bad = (lists[1][0], np.array([200.0, 0.0]), lists[1][2])
    refused("sigma <= 0", r"rc=-1: .*sigma <= 0 \(member 1\b", lambda: G.run(4, 7200.0, moulins=[lists[0], bad, lists[2]], moulin_factor=np.ones((4, n))))
    empty = (np.zeros((0, 2)), np.zeros(0), np.zeros(0))
    refused("an empty list", r"rc=-1: .*member 1\b", lambda: G.run(4, 7200.0, moulins=[lists[0], empty, lists[2]], moulin_factor=np.ones((4, n))))
    refused("n_steps < 1", r"rc=-1: .*n_steps = 0", lambda: G.run(0, 7200.0))
    refused("a schedule for another member count (Python)", r"\(n_steps, n\) = \(4, 3\)", lambda: G.run(4, 7200.0, T_K=np.zeros((4, n + 1)), background=bg), exc=ValueError)
    refused("a ramp of another length", r"\(n_steps,\)", lambda: G.run(4, 7200.0, ramp=np.ones(3)), exc=ValueError)

    def c_call_with_another_member_count():
        sch = capi.BatchSchedule(n_steps=4, dt=7200.0, first_cur_step=1, n_members=n + 1)
        capi.check(capi.lib().suhmo_batch_run(G.batch.h, G._mp, C.byref(sch), None, C.byref(capi.BatchRunResult()), G.batch.stream))
    refused("a schedule for another member count (C)", r"rc=-1: .*4 members, the batch has 3", c_call_with_another_member_count)
    refused("both kinds of forcing", r"rc=-1: .*same source term", lambda: G.run(4, 7200.0, T_K=T_K, background=bg, moulins=lists, moulin_factor=np.ones((4, n))))
    G.set_option("implicit_gap", 0)
    refused("use_impl_diff without implicit_gap", r"rc=-5: .*member 0\b", lambda: G.run(4, 7200.0, T_K=T_K, background=bg, active=[1, 0, 1]))
    G.set_option("implicit_gap", 1)
    refused("use_moulin_source without a source", r"rc=-1: .*use_moulin_source without .*member 0\b", lambda: G.run(4, 7200.0))
    # members 0 and 2 may go without member 1: the batch stays usable
    pi, nv, rows = G.run(4, 7200.0, T_K=T_K, background=bg, diag_every=2, active=[1, 0, 1])
    assert G.cur_step == 4 and np.all(pi[:, [0, 2]] >= 1) and np.all(pi[:, 1] == 0) and np.all(np.isfinite(rows[:, [0, 2]]))
    G.close()
