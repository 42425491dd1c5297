"""Plot files and checkpoints inside the run of a hierarchy (include/suhmo_hip.h, "OUTPUT INSIDE THE RUN"; suhmo_hier_run_out): the events and
every snapshot handed to the callback against a twin driven by the per-call loop, a run with output against the same run without, runs split in
two, a callback that fails, the refusals, and HipHierModel.run writing files a restart continues from.  The set-up is the run tests'
(tests/test_gpu_hier_run.py): its first regrid moves the hierarchy from OLD to GEN."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.test_gpu_hier_run import shmip_model, analytic, assert_same_state, assert_same_counts, MOULINS, REGRID, DT, OLD, GEN

pytestmark = pytest.mark.gpu
PLOT, CHECKPOINT = 0, 1


def check_comps(M):
    from suhmo_amd import checkpoint
    return checkpoint.snapshot_components(checkpoint.constants(M.model))[0]


def loop_with_output(L, n_steps, plot_interval, check_interval, regrid_interval, final=True, restart_step=0):
    """the per-call loop in the order the header states, a snapshot of the twin where the run has an event -> (events, counts)"""
    from suhmo_amd import model, plotfile
    due = model.regrid_steps(L.cur_step + 1, n_steps, regrid_interval)
    shot = lambda kind, cur: (kind, cur, [list(bl) for bl in L.hier.boxes]) + L.hier.snapshot(plotfile.SNAP if kind == PLOT else check_comps(L), 1)
    events, counts = [], []
    for k in range(n_steps):
        c, changed = L.cur_step + 1, False
        if plot_interval > 0 and (c - 1) % plot_interval == 0:
            events.append(shot(PLOT, c - 1))
        if c in due:
            _, same = L.tag_and_regrid(reload=analytic, **REGRID)
            changed = not same
        if check_interval > 0 and (c - 1) % check_interval == 0 and c - 1 != restart_step:
            events.append(shot(CHECKPOINT, c - 1))
        if k == 0 or changed:
            L.moulin_source(**MOULINS)
        counts.append(L.timestep(DT))
    if final and plot_interval >= 0:
        events.append(shot(PLOT, L.cur_step))
    if final and check_interval >= 0:
        events.append(shot(CHECKPOINT, L.cur_step))
    return events, counts


def capture(monkeypatch, M):
    """M.run's writers replaced by recorders of what the callback was handed: (kind, cur_step, boxes, level_offset, box_offset, copy of the data)"""
    from suhmo_amd import checkpoint, plotfile
    events = []

    def plot_levels(path, names, levels, time, dt=1.0, ghost=1):
        cur = int(os.path.basename(path)[len("plot"):len("plot") + 6])
        lo = np.concatenate([[0], np.cumsum([v["data"].size for v in levels])])
        events.append((PLOT, cur, [v["boxes"] for v in levels[1:]], lo, [np.array(v["offsets"]) for v in levels], np.concatenate([v["data"] for v in levels]), time))

    def chk_write(path, model, time, dt, periodic=(0, 0), extra=None, packed=False, snapshot=None, step=None):
        lo, bo, flat = snapshot
        events.append((CHECKPOINT, step, [list(bl) for bl in model.hier.boxes], np.array(lo), [np.array(b) for b in bo], flat.copy(), time))

    monkeypatch.setattr(plotfile, "write_levels", plot_levels)
    monkeypatch.setattr(checkpoint, "write", chk_write)
    return events


def assert_same_events(got, want, steps=None):
    from suhmo_amd import model
    assert [(e[0], e[1]) for e in got] == [(e[0], e[1]) for e in want]
    if steps is not None:
        assert [(e[0], e[1]) for e in got] == [(k, c) for k, c, _ in steps], "the events are output_steps's"
    for g, w in zip(got, want):
        what = ("kind", g[0], "cur_step", g[1])
        assert g[2] == w[2], what + ("the box lists",)
        assert np.array_equal(g[3], w[3]) and len(g[4]) == len(w[4]) and all(np.array_equal(a, b) for a, b in zip(g[4], w[4])), what + ("offsets",)
        assert g[5].tobytes() == w[5].tobytes(), what + ("data",)


@pytest.mark.parametrize("plot_interval", [3, 2])
def test_events_equal_the_loops(monkeypatch, plot_interval):
    from suhmo_amd import model
    R, L = shmip_model(), shmip_model()
    events = capture(monkeypatch, R)
    want, counts = loop_with_output(L, 7, plot_interval, 3, 3)
    pi, nv, _, log = R.run(7, DT, moulins=MOULINS, regrid_interval=3, reload=analytic, plot_interval=plot_interval, check_interval=3, time0=100.0, **REGRID)
    assert [e["cur_step"] for e in log] == [4, 7] and [e["same"] for e in log] == [False, True]
    assert_same_events(events, want, model.output_steps(1, 7, plot_interval, 3))
    by = {(e[0], e[1]): e for e in events}
    last_old = 3 if plot_interval == 3 else 2               # the regrid before step 4 moves the boxes: at b = 3 the plot shows the old ones, the checkpoint the new ones
    assert by[(PLOT, last_old)][2] == OLD and by[(CHECKPOINT, 3)][2] == GEN and by[(PLOT, 6)][2] == GEN
    assert [e[6] for e in events] == [100.0 + e[1] * DT for e in events], "the file's time"
    assert R.hier.get_option("run_plots") == sum(e[0] == PLOT for e in events) and R.hier.get_option("run_checkpoints") == sum(e[0] == CHECKPOINT for e in events)
    assert len(R.last_run["plots"]) == R.hier.get_option("run_plots") and len(R.last_run["checkpoints"]) == R.hier.get_option("run_checkpoints")
    assert_same_counts(pi, nv, counts)
    assert_same_state(R, L)
    R.close(); L.close()


def test_a_run_with_output_equals_the_run_without(monkeypatch):
    R, N = shmip_model(), shmip_model()
    events = capture(monkeypatch, R)
    kw = dict(moulins=MOULINS, regrid_interval=3, reload=analytic, diag_every=2, **REGRID)
    a = R.run(7, DT, plot_interval=2, check_interval=3, **kw)
    b = N.run(7, DT, **kw)
    assert len(events) == 8
    assert list(a[0]) == list(b[0]) and list(a[1]) == list(b[1]) and a[3] == b[3]
    assert a[2].shape == (3, 6) and np.array_equal(a[2], b[2], equal_nan=True)
    assert N.hier.get_option("run_plots") == 0 and N.hier.get_option("snapshot_launches") == 0
    assert R.hier.get_option("snapshot_launches") == R.hier.get_option("snapshot_copies") == 8 * 3, "carried over the regrid: a launch and a copy per level and event"
    assert_same_state(R, N)
    R.close(); N.close()


@pytest.mark.parametrize("split", [3, 4])
def test_two_runs_with_no_final_equal_one(monkeypatch, split):
    """at the regrid's b (split 3: the second run starts with the plot, the regrid and the checkpoint of b = 3) and beside it"""
    O, T = shmip_model(), shmip_model()
    kw = dict(moulins=MOULINS, regrid_interval=3, reload=analytic, plot_interval=2, check_interval=3, **REGRID)
    one = capture(monkeypatch, O)
    O.run(7, DT, **kw)
    two = capture(monkeypatch, T)
    T.run(split, DT, final_output=False, **kw)
    n1 = len(two)
    T.run(7 - split, DT, **kw)
    assert 0 < n1 < len(two)
    assert_same_events(two, one)
    assert_same_state(T, O)
    O.close(); T.close()


def c_run_out(M, n_steps, out, with_moulins=True):
    """suhmo_hier_run_out without regrids, the schedule and the output given field by field -> (rc, message, steps_done)"""
    from suhmo_amd import capi
    pos = np.ascontiguousarray(np.array(MOULINS["positions"]).reshape(-1))
    sg, fl = np.ascontiguousarray(MOULINS["sigma"], dtype=np.float64), np.ascontiguousarray(MOULINS["flux"], dtype=np.float64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    sch = capi.HierSchedule(n_steps=n_steps, dt=DT, first_cur_step=M.cur_step + 1, max_level=2)
    if with_moulins:
        sch.n_moulins, sch.positions, sch.sigma, sch.flux = 3, dp(pos), dp(sg), dp(fl)
    pi = np.zeros(n_steps, dtype=np.intc)
    res = capi.HierRunResult(picard_iters=pi.ctypes.data_as(C.POINTER(C.c_int)))
    hp = C.c_void_p(M.hier.h.value)
    rc = capi.lib().suhmo_hier_run_out(C.byref(hp), C.byref(M._mp), C.byref(sch), C.byref(out) if out is not None else None, C.byref(res), M.hier.stream)
    assert hp.value == M.hier.h.value
    return rc, capi.lib().suhmo_last_error().decode(), int(res.steps_done)


def test_a_callback_that_fails_ends_the_run():
    from suhmo_amd import capi, plotfile
    M, T = shmip_model(), shmip_model()
    seen = []

    def write(user, h, kind, cur_step, ncomp, lo, bo, data):
        seen.append((kind, cur_step, ncomp, data[66 + 1]))         # the head of cell (0, 0) of level 0: row 1, column 1 of its ghosted 66-wide fab
        return 7 if len(seen) == 2 else 0

    pc, cb = capi.snap_comps(plotfile.SNAP), capi.OUTPUT_FN(write)
    out = capi.HierOutput(1, -1, 0, 0, len(plotfile.SNAP), pc, 0, None, cb, None)
    rc, msg, done = c_run_out(M, 4, out)
    assert rc == -1 and "returned 7" in msg and "cur_step 1" in msg
    assert done == 1 and [(k, c, n) for k, c, n, _ in seen] == [(PLOT, 0, 13), (PLOT, 1, 13)]
    assert M.hier.get_option("run_plots") == 1
    M.cur_step += done
    T.moulin_source(**MOULINS)
    T.timestep(DT)
    assert seen[1][3] == T.get(0, 0, "head")[0, 0] != seen[0][3], "the second event saw the state after one step"
    assert M.timestep(DT) == T.timestep(DT)
    assert_same_state(M, T)
    M.close(); T.close()


def test_refusals_before_the_first_launch():
    from suhmo_amd import capi, level as lv, plotfile
    M, T = shmip_model(), shmip_model()
    for G in (M, T):
        G.moulin_source(**MOULINS)
    calls = []
    cb = capi.OUTPUT_FN(lambda *a: calls.append(a) or 0)
    none = capi.OUTPUT_FN()
    pc = capi.snap_comps(plotfile.SNAP)
    face = capi.snap_comps([(capi.SNAP_FIELD, lv.F_QWX)])
    too_many = capi.snap_comps([(capi.SNAP_CONST, 0, 1.0)] * 17)
    n = len(plotfile.SNAP)
    cases = [capi.HierOutput(-2, -1, 0, 0, n, pc, 0, None, cb, None), capi.HierOutput(-1, -2, 0, 0, n, pc, n, pc, cb, None),
             capi.HierOutput(1, -1, 0, 0, 0, None, 0, None, cb, None), capi.HierOutput(0, -1, 0, 0, n, None, 0, None, cb, None),
             capi.HierOutput(-1, 0, 0, 0, n, pc, 0, None, cb, None), capi.HierOutput(2, -1, 0, 0, n, pc, 0, None, none, None),
             capi.HierOutput(-1, 2, 0, 0, 0, None, n, pc, none, None), capi.HierOutput(1, -1, 0, 0, 1, face, 0, None, cb, None),
             capi.HierOutput(-1, 1, 0, 0, 0, None, 17, too_many, cb, None)]
    for q, out in enumerate(cases):
        rc, msg, done = c_run_out(M, 2, out)
        assert rc == -1 and msg and done == 0, (q, rc, msg)
    assert not calls and M.hier.get_option("snapshot_launches") == 0
    # both kinds off: the output is not looked at, the run is suhmo_hier_run's
    rc, msg, done = c_run_out(M, 1, capi.HierOutput(-1, -1, 0, 0, 0, None, 0, None, none, None))
    assert rc == 0 and done == 1
    M.cur_step += 1
    T.timestep(DT)
    assert_same_state(M, T)
    M.close(); T.close()


def test_files_of_a_run_and_a_restart_from_one(tmp_path):
    from suhmo_amd import checkpoint, plotfile
    if checkpoint.hdf5_prefix() is None and not os.path.exists(checkpoint.LIB_PATH):
        pytest.skip("no HDF5 C library on this box: the (optional) checkpoint / plot file library cannot be built")
    plotfile.build()
    R = shmip_model()
    kw = dict(moulins=MOULINS, regrid_interval=3, reload=analytic, **REGRID)
    pp, cp = str(tmp_path / "plot"), str(tmp_path / "chk")
    pi, nv, _, log = R.run(7, DT, plot_interval=2, check_interval=3, check_overwrite=False, plot_prefix=pp, check_prefix=cp, **kw)
    assert [e["same"] for e in log] == [False, True]
    assert R.last_run["plots"] == [pp + "%06d.2d.hdf5" % c for c in (0, 2, 4, 6, 7)]
    assert R.last_run["checkpoints"] == [cp + "%06d.2d.hdf5" % c for c in (3, 6, 7)]
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in R.last_run["plots"] + R.last_run["checkpoints"])
    names, levels = plotfile.read_levels(R.last_run["plots"][1])
    assert names == plotfile.NAMES and [v["boxes"] for v in levels[1:]] == OLD and levels[0]["time"] == 2 * DT
    assert [v["boxes"] for v in plotfile.read_levels(R.last_run["plots"][-1])[1][1:]] == GEN
    # the checkpoint written before step 4, after that step's regrid: a model on ITS boxes, restarted from it, reaches the run's final state
    hdr, chk = checkpoint.read_levels(R.last_run["checkpoints"][0])
    assert hdr["current_step"] == 3 and hdr["time"] == 3 * DT and [v["boxes"] for v in chk[1:]] == GEN
    B = shmip_model([v["boxes"] for v in chk[1:]])
    checkpoint.restart(R.last_run["checkpoints"][0], B)
    assert B.cur_step == 3
    p2, v2, _, log2 = B.run(4, DT, skip_first_regrid=True, restart_step=3, plot_interval=-1, check_interval=-1, **kw)
    assert [e["cur_step"] for e in log2] == [7] and log2[0]["same"]
    assert list(p2) == list(pi[3:]) and list(v2) == list(nv[3:])
    assert B.hier.boxes == R.hier.boxes and B.cur_step == R.cur_step == 7
    for l, bl in enumerate(R.level):
        for k in range(len(bl)):
            for nm in ("head", "B", "mR", "Pw", "qwx"):
                assert np.array_equal(R.get(l, k, nm), B.get(l, k, nm), equal_nan=True), (l, k, nm)
    # with check_overwrite (the default) every checkpoint goes into one file
    R.run(1, DT, check_interval=0, check_prefix=cp, **kw)
    assert R.last_run["checkpoints"] == [cp + ".2d.hdf5"] and R.last_run["plots"] == []
    assert checkpoint.read_levels(cp + ".2d.hdf5")[0]["current_step"] == 8
    R.close(); B.close()
