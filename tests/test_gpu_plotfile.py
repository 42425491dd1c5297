"""Plot files and packed checkpoints of a device-resident hierarchy (suhmo_amd/plotfile.py, checkpoint.write(packed=True)): what one snapshot
puts into a file against what the per-box calls read, and a restart from the packed checkpoint that continues bit for bit."""
import os

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import snapshot_ref as sr
from tests.test_gpu_checkpoint import UNION, MOULINS

pytestmark = pytest.mark.gpu
MODEL = dict(sy.A3_MODEL, diffFactor=1.0, use_impl_diff=1, use_moulin_source=1, distributed_input=7.93e-11)
DT = MODEL["dt"]


@pytest.fixture(scope="module")
def io():
    from suhmo_amd import checkpoint, plotfile
    if checkpoint.hdf5_prefix() is None and not os.path.exists(checkpoint.LIB_PATH):
        pytest.skip("no HDF5 C library on this box: the (optional) checkpoint / plot file library cannot be built")
    plotfile.build()
    return checkpoint, plotfile


def make():
    """the union hierarchy of tests/test_gpu_checkpoint.py"""
    from suhmo_amd import model
    sts = sy.shmip_amrm_states(64, 32, UNION, rough=0.5)
    M = model.HipHierModel(64, 32, sts[0][0]["dx"], sts[0][0]["dy"], sy.A3_BC, sy.A3_PHYS, MODEL, UNION, max_box=16)
    M.set_states(sts)
    M.moulin_source(**MOULINS)
    return M


def stepped(n=3):
    M = make()
    for _ in range(n):
        M.timestep(DT)
    return M


def test_plot_file_of_a_hierarchy(io, tmp_path):
    from suhmo_amd import level as lv
    _, plotfile = io
    M = stepped()
    path = str(tmp_path / "plot000003.2d.hdf5")
    plotfile.write(path, M, time=3 * DT)
    names, levels = plotfile.read_levels(path)
    assert names == ["head", "gapHeight", "bedelevation", "overburdenPress", "Pw", "Qw_x", "Qw_y", "Re", "meltRate", "GradHead_x", "GradHead_y",
                     "iceHeight", "iceMask"]
    boxes = [[(0, 0, 63, 31)]] + [list(bl) for bl in UNION]
    assert [v["boxes"] for v in levels] == boxes
    ids = [lv.F_PHI, lv.F_B, lv.F_ZB, lv.F_PI, lv.F_PW, lv.F_QWX, lv.F_QWY, lv.F_RE, lv.F_MR, lv.F_GRADX, lv.F_GRADY, lv.F_ZS, lv.F_MASK]
    comps = [(sr.FACE_TO_CELL if f in (lv.F_QWX, lv.F_QWY) else sr.FIELD, f, 0.0) for f in ids]
    # nobody loaded a surface height: iceHeight is 0 in the file (and the per-box get below would allocate it, so it is not asked)
    get = lambda l, k, f: None if f == lv.F_ZS else M.level[l][k].get(f, ghosted=f not in (lv.F_QWX, lv.F_QWY))
    lo, bo, flat = sr.pack(boxes, get, comps, 1)
    for l, v in enumerate(levels):
        assert v["ghost"] == 1 and v["time"] == 3 * DT and v["dt"] == 1.0 / 2 ** l and v["dx"] == M.level[l][0].dx and v["dy"] == M.level[l][0].dy
        assert v["domain"] == (0, 0, (64 << l) - 1, (32 << l) - 1) and v["vec_ref_ratio"] == ((2, 2) if l < 2 else (1, 1))
        assert np.array_equal(v["offsets"], bo[l])
        for k, b in enumerate(v["boxes"]):
            want = sr.box_of(lo, bo, flat, 13, 1, l, k, b)
            for q, nm in enumerate(names):
                assert want[q].tobytes() == v["fabs"][k][q].tobytes(), (nm, l, k)
            assert np.isfinite(v["fabs"][k]).all() and v["fabs"][k][5][1:-1, 1:-1].any() and not v["fabs"][k][11].any(), (l, k)
    M.close()


def test_plot_file_of_a_single_level(io, tmp_path):
    from suhmo_amd import level as lv, model
    _, plotfile = io
    m = sy.A3_MODEL
    st = sy.shmip_initial_state(64, 32, m["lx"], m["ly"])
    M = model.HipModel(64, 32, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=32)
    M.set_state(st)
    M.timestep(m["dt"])
    path = str(tmp_path / "plot000001.2d.hdf5")
    plotfile.write(path, M, time=m["dt"])
    names, levels = plotfile.read_levels(path)
    assert len(levels) == 1 and levels[0]["boxes"] == [(0, 0, 63, 31)] and levels[0]["vec_ref_ratio"] == (1, 1)
    fab = levels[0]["fabs"][0]
    assert fab[names.index("head")].tobytes() == M.level.get(lv.F_PHI, ghosted=True).tobytes()
    assert fab[names.index("iceMask")].tobytes() == M.level.get(lv.F_MASK, ghosted=True).tobytes()
    qx = M.level.get(lv.F_QWX)
    assert np.array_equal(fab[names.index("Qw_x")][1:-1, 1:-1], 0.5 * (qx[:, :-1] + qx[:, 1:]))
    M.close()


def test_packed_checkpoint_equals_the_per_box_one_and_restarts(io, tmp_path):
    checkpoint, _ = io
    A = stepped()
    packed, plain = str(tmp_path / "packed.2d.hdf5"), str(tmp_path / "plain.2d.hdf5")
    n = A.hier.get_option("snapshot_copies")
    checkpoint.write(packed, A, time=3 * DT, dt=DT, packed=True)
    assert A.hier.get_option("snapshot_copies") - n == A.hier.nlev, "one snapshot: a copy per level"
    checkpoint.write(plain, A, time=3 * DT, dt=DT)
    (ha, la), (hb, lb) = checkpoint.read_levels(packed), checkpoint.read_levels(plain)
    assert ha == hb and ha["current_step"] == 3 and len(la) == len(lb) == 3
    for a, b in zip(la, lb):
        assert {k: v for k, v in a.items() if k != "data"} == {k: v for k, v in b.items() if k != "data"}
        assert list(a["data"]) == list(b["data"]) == [name for name, _ in checkpoint.FIELDS]
        for name in a["data"]:
            for k, (x, y) in enumerate(zip(a["data"][name], b["data"][name])):
                assert x.tobytes() == y.tobytes(), (name, k)
    # a dataset given as arrays is filled on the host in either path
    extra = {"iceHeightData": [[np.full((bx[3] - bx[1] + 3, bx[2] - bx[0] + 3), 10.0 * l + k) for k, bx in enumerate(bl)]
                               for l, bl in enumerate([[(0, 0, 63, 31)]] + [list(q) for q in UNION])]}
    checkpoint.write(packed, A, time=3 * DT, dt=DT, packed=True, extra=extra)
    lv2 = checkpoint.read_levels(packed)[1]
    assert all((lv2[l]["data"]["iceHeightData"][k] == 10.0 * l + k).all() for l in range(3) for k in range(len(lv2[l]["boxes"])))
    assert all(lv2[l]["data"]["headData"][k].tobytes() == la[l]["data"]["headData"][k].tobytes() for l in range(3) for k in range(len(lv2[l]["boxes"])))
    checkpoint.write(packed, A, time=3 * DT, dt=DT, packed=True)
    # the restart from the packed file continues bit for bit
    counts = [A.timestep(DT) for _ in range(2)]
    B = make()
    hdr = checkpoint.restart(packed, B)
    assert hdr["current_step"] == 3 and B.cur_step == 3
    assert [B.timestep(DT) for _ in range(2)] == counts
    for l, bl in enumerate(A.level):
        for k in range(len(bl)):
            for nm in ("head", "B", "mR", "Pw", "qwx"):
                assert np.array_equal(A.get(l, k, nm), B.get(l, k, nm), equal_nan=True), (l, k, nm)
    A.close(); B.close()
