"""The device snapshot (include/suhmo_hip.h, "SNAPSHOT"; suhmo_amd/csrc/suhmo_snap.hip): every slice of suhmo_hier_snapshot against what
suhmo_level_get_field returns for that box, bit for bit, over generated and hand-made layouts on the 32 x 16 base of tests/hierlayouts.py; the
offsets against the numpy twin tests/snapshot_ref.py; one launch and one copy per level; a snapshot changes nothing; every refusal."""
import ctypes as C
import re

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import hierlayouts as hl
from tests import snapshot_ref as sr

pytestmark = pytest.mark.gpu
NX0, NY0 = hl.NX0, hl.NY0                                   # 32 x 16


def _rc(e):
    return int(re.search(r"rc=(-?\d+)", str(e)).group(1))


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def stepped_model(bc, boxes):
    """the SqrtIBC state of the run tests on `boxes`, one time step later: the relaxation has traded the two canvases of the head and the face
    fields of the water flux exist on every box"""
    from suhmo_amd import model
    sts = sy.shmip_amrm_states(NX0, NY0, boxes, rough=0.5)
    M = model.HipHierModel(NX0, NY0, sts[0][0]["dx"], sts[0][0]["dy"], bc, sy.A3_PHYS, sy.A3_MODEL, boxes, max_box=16)
    M.set_states(sts)
    M.timestep(sy.A3_MODEL["dt"])
    return M


def all_boxes(M):
    return [[(0, 0, NX0 - 1, NY0 - 1)]] + [list(bl) for bl in M.hier.boxes]


def load_random(M, seed):
    """random data, ghost rings included, in B, the mask and the two face fields of the water flux of every box"""
    from suhmo_amd import level as lv
    for l, bl in enumerate(M.level):
        for k, L in enumerate(bl):
            rng = np.random.default_rng([seed, l, k])
            L.set(lv.F_B, rng.uniform(0.0, 1.0, size=(L.ny + 2, L.nx + 2)), ghosted=True)
            L.set(lv.F_MASK, np.where(rng.random((L.ny + 2, L.nx + 2)) < 0.3, -1.0, 1.0), ghosted=True)
            L.set(lv.F_QWX, rng.normal(size=(L.ny, L.nx + 1)))
            L.set(lv.F_QWY, rng.normal(size=(L.ny + 1, L.nx)))


CASES = [("seed-%d" % s, s) for s in range(8)] + [("span-x", "span-x"), ("tiny-boxes", "tiny-boxes")]


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[n for n, _ in CASES])
def test_slices_equal_get(case):
    """seeds 0 .. 7: all four periodicities, boxes on domain sides; span-x: a level-1 box over the whole 64-cell width (its ghosted row of 66
    crosses the 64-thread workgroup edge) and a level-2 box of 128; tiny-boxes: boxes 2 cells wide"""
    from suhmo_amd import capi, level as lv
    bc, boxes = hl.generate(case) if isinstance(case, int) else hl.FEATURES[case]
    M = stepped_model(bc, boxes)
    load_random(M, 7 if not isinstance(case, int) else case)
    H = M.hier
    UNHELD = lv.F_ZS                                         # nobody has loaded a surface height
    comps = [(capi.SNAP_FIELD, lv.F_PHI, 0.0), (capi.SNAP_FIELD, lv.F_B, 0.0), (capi.SNAP_FIELD, lv.F_MASK, 0.0), (capi.SNAP_FACE_TO_CELL, lv.F_QWX, 0.0),
             (capi.SNAP_FACE_TO_CELL, lv.F_QWY, 0.0), (capi.SNAP_CONST, 0, 3.5), (capi.SNAP_FIELD, UNHELD, 0.0)]
    bxs = all_boxes(M)
    held = [H.get_option("canvas_bytes_level_%d" % l) for l in range(1, H.nlev)]
    shots = {}
    for ghost in (1, 0):
        n_l, n_c = H.get_option("snapshot_launches"), H.get_option("snapshot_copies")
        shots[ghost] = H.snapshot(comps, ghost)
        assert H.get_option("snapshot_launches") - n_l == H.nlev and H.get_option("snapshot_copies") - n_c == H.nlev, "one launch and one copy per level"
    assert [H.get_option("canvas_bytes_level_%d" % l) for l in range(1, H.nlev)] == held, "a snapshot allocates nothing"
    with pytest.raises(capi.SuhmoError) as e:                # ... on level 0 neither: the recharge still finds no surface height
        M.time_varying_recharge(7.5, 0.0)
    assert _rc(e.value) == -1 and "level 0, box 0" in str(e.value)
    # what every box holds, through the per-box calls (these allocate nothing that is compared afterwards)
    got = {}

    def get(l, k, field):
        if field == UNHELD:
            return None
        if (l, k, field) not in got:
            got[(l, k, field)] = M.level[l][k].get(field, ghosted=field not in (lv.F_QWX, lv.F_QWY))
        return got[(l, k, field)]

    for ghost in (1, 0):
        lo, bo, flat = shots[ghost]
        wlo, wbo, wflat = sr.pack(bxs, get, comps, ghost)
        assert np.array_equal(lo, wlo) and all(np.array_equal(a, b) for a, b in zip(bo, wbo)) and len(bo) == len(wbo), "the offsets are the twin's"
        inner = (slice(1, -1), slice(1, -1)) if ghost else (slice(None), slice(None))
        cut = (lambda a: a) if ghost else (lambda a: a[1:-1, 1:-1])
        for l, bl in enumerate(bxs):
            for k, b in enumerate(bl):
                fab = lv.snapshot_box(lo, bo, flat, len(comps), ghost, l, k, b)
                what = (case, "ghost", ghost, "level", l, "box", k)
                for q, f in ((0, lv.F_PHI), (1, lv.F_B), (2, lv.F_MASK)):
                    assert same_bits(fab[q], cut(get(l, k, f))), what + ("field", f)
                qx, qy = get(l, k, lv.F_QWX), get(l, k, lv.F_QWY)
                assert np.array_equal(fab[3][inner], 0.5 * (qx[:, :-1] + qx[:, 1:])), what + ("Qw_x",)
                assert np.array_equal(fab[4][inner], 0.5 * (qy[:-1, :] + qy[1:, :])), what + ("Qw_y",)
                if ghost:
                    ring = np.ones(fab[3].shape, dtype=bool)
                    ring[1:-1, 1:-1] = False
                    assert not fab[3][ring].any() and not fab[4][ring].any(), what + ("the ring of a face average is 0",)
                assert (fab[5] == 3.5).all() and not fab[6].any(), what
        assert same_bits(flat, wflat), (case, ghost)
    M.close()


def test_a_snapshot_changes_nothing():
    """the run tests' model, snapshots between its steps, against a twin that is never asked"""
    from suhmo_amd import plotfile
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT, assert_same_state
    A, B = shmip_model(), shmip_model()
    for G in (A, B):
        G.moulin_source(**MOULINS)
    A.hier.snapshot(plotfile.SNAP, 1)                        # before the first step: most fields are not held yet
    for _ in range(2):
        assert A.timestep(DT) == B.timestep(DT)
        A.hier.snapshot(plotfile.SNAP, 1)
        A.hier.snapshot(plotfile.SNAP[:3], 0)
    assert_same_state(A, B)
    A.close(); B.close()


def test_level_snapshot_on_a_single_level():
    from suhmo_amd import capi, level as lv, model
    m = sy.A3_MODEL
    st = sy.shmip_initial_state(64, 32, m["lx"], m["ly"])
    M = model.HipModel(64, 32, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=32)
    M.set_state(st)
    M.timestep(m["dt"])
    comps = [(capi.SNAP_FIELD, lv.F_PHI), (capi.SNAP_FACE_TO_CELL, lv.F_QWY), (capi.SNAP_CONST, 0, -2.0), (capi.SNAP_FIELD, lv.F_ZS), (capi.SNAP_FIELD, lv.F_MR)]
    for ghost in (1, 0):
        a = M.level.snapshot(comps, ghost)
        assert a.shape == (5, 32 + 2 * ghost, 64 + 2 * ghost)
        cut = (lambda x: x) if ghost else (lambda x: x[1:-1, 1:-1])
        assert same_bits(a[0], cut(M.level.get(lv.F_PHI, ghosted=True))) and same_bits(a[4], cut(M.level.get(lv.F_MR, ghosted=True)))
        qy = M.level.get(lv.F_QWY)
        want = np.zeros(a[1].shape)
        want[(slice(1, -1), slice(1, -1)) if ghost else (slice(None), slice(None))] = 0.5 * (qy[:-1, :] + qy[1:, :])
        assert np.array_equal(a[1], want) and (a[2] == -2.0).all() and not a[3].any()
    assert np.isfinite(M.level.get(lv.F_PHI)).all()
    M.close()


def test_refusals_leave_the_destination_alone():
    from suhmo_amd import capi, level as lv, model
    from tests.test_gpu_hier_run import shmip_model, MOULINS, DT, DX0, STEP_MODEL, assert_same_state
    M, T = shmip_model(), shmip_model()
    for G in (M, T):
        G.moulin_source(**MOULINS)
    nbox = sum(len(bl) for bl in M.level)
    dst = np.full(200000, -77.0)
    lo, bo, n1 = (C.c_long * (M.hier.nlev + 1))(), (C.c_long * (nbox + M.hier.nlev))(), C.c_long()
    dp = dst.ctypes.data_as(C.POINTER(C.c_double))
    F, E, K = capi.SNAP_FIELD, capi.SNAP_FACE_TO_CELL, capi.SNAP_CONST
    ok = [(F, lv.F_B)]
    cases = [(0, ok, 1, -1), (17, [(K, 0, 1.0)] * 17, 1, -1), (1, ok, 2, -1), (1, ok, -1, -1), (1, [(F, -1)], 1, -1), (1, [(F, 33)], 1, -1),
             (1, [(E, 33)], 1, -1), (1, [(F, lv.F_QWX)], 1, -1), (2, ok + [(F, lv.F_BY)], 0, -1), (1, [(E, lv.F_B)], 1, -1), (1, [(F, lv.F_COVER)], 1, -1),
             (1, [(F, lv.F_PHI2)], 0, -1), (1, [(E, lv.F_PHI2)], 1, -1), (1, [(3, lv.F_B)], 1, -1)]
    launches = M.hier.get_option("snapshot_launches")
    for ncomp, comps, ghost, want in cases:
        arr = capi.snap_comps(comps)
        rc = capi.lib().suhmo_hier_snapshot(M.hier.h, ncomp, arr, ghost, lo, bo, dp, M.hier.stream)
        assert rc == want and capi.lib().suhmo_last_error(), (ncomp, comps, ghost, rc)
        rc = capi.lib().suhmo_level_snapshot(M.level[1][0].h, ncomp, arr, ghost, C.byref(n1), dp, M.hier.stream)
        assert rc == want, ("level", ncomp, comps, ghost, rc)
    # a rank strip and a hierarchy created with shadow = 1: rc -5
    S = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, j0=0, ny_global=64)
    W = model.HipHierModel(64, 32, DX0, DX0, sy.A3_BC, sy.A3_PHYS, STEP_MODEL, [[(32, 16, 63, 47)]], max_box=16, options="shadow=1")
    arr = capi.snap_comps(ok)
    for G in (S, W):
        rc = capi.lib().suhmo_hier_snapshot(G.hier.h, 1, arr, 1, lo, bo, dp, G.hier.stream)
        assert rc == -5 and "not built" in capi.lib().suhmo_last_error().decode()
    assert capi.lib().suhmo_level_snapshot(S.level[0][0].h, 1, arr, 1, C.byref(n1), dp, S.hier.stream) == -5
    S.close(); W.close()
    assert (dst == -77.0).all(), "nothing was written"
    assert M.hier.get_option("snapshot_launches") == launches, "nothing was launched"
    # the offsets alone need no destination and launch nothing
    capi.check(capi.lib().suhmo_hier_snapshot(M.hier.h, 1, arr, 1, lo, bo, None, M.hier.stream))
    assert lo[M.hier.nlev] == sum((b[3] - b[1] + 3) * (b[2] - b[0] + 3) for bl in [[(0, 0, 63, 31)]] + M.hier.boxes for b in bl)
    assert M.hier.get_option("snapshot_launches") == launches
    assert M.timestep(DT) == T.timestep(DT)
    assert_same_state(M, T)
    M.close(); T.close()
