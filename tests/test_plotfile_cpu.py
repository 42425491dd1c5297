"""The plot file writer / reader (include/suhmo_plt.h; Chombo's layout of AmrHydro::writePlotFile, src/AmrHydro.cpp:5474-5667) on the host alone:
two levels of random data in the snapshot's order go through a file and come back bit for bit with names, attributes and offsets, and the
file has the groups and datasets Chombo's reader looks for."""
import os
import subprocess

import numpy as np
import pytest


@pytest.fixture(scope="module")
def plt():
    from suhmo_amd import checkpoint, plotfile
    if checkpoint.hdf5_prefix() is None and not os.path.exists(checkpoint.LIB_PATH):
        pytest.skip("no HDF5 C library on this box: the (optional) checkpoint / plot file library cannot be built")
    plotfile.build()
    return plotfile


BOXES = [[(0, 0, 31, 15)], [(8, 4, 23, 11), (24, 4, 39, 19), (40, 20, 47, 27)]]


def make_levels(rng, ncomp=13, ghost=1, dx=(100.0, 100.0)):
    levels = []
    for l, bl in enumerate(BOXES):
        sizes = [ncomp * (b[3] - b[1] + 1 + 2 * ghost) * (b[2] - b[0] + 1 + 2 * ghost) for b in bl]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        levels.append(dict(dx=dx[0] / 2 ** l, dy=dx[1] / 2 ** l, domain=(0, 0, (32 << l) - 1, (16 << l) - 1), boxes=bl, offsets=off,
                           data=rng.normal(size=int(off[-1]))))
    return levels


def test_round_trip(plt, tmp_path):
    levels = make_levels(np.random.default_rng(11))
    path = str(tmp_path / "plot000007.2d.hdf5")
    plt.write_levels(path, plt.NAMES, levels, time=25200.0, dt=1.0)
    names, back = plt.read_levels(path)
    assert names == plt.NAMES and len(names) == 13 and names[5] == "Qw_x" and names[-1] == "iceMask"
    assert len(back) == 2
    for l, (a, b) in enumerate(zip(levels, back)):
        assert a["boxes"] == b["boxes"] and a["domain"] == b["domain"]
        assert (b["dx"], b["dy"]) == (a["dx"], a["dy"]) and b["dx_attr"] == a["dx"], "vec_dx, and the scalar where the directions agree"
        assert b["dt"] == 1.0 / 2 ** l and b["time"] == 25200.0 and b["ghost"] == 1
        assert np.array_equal(a["offsets"], b["offsets"]) and b["offsets"][0] == 0
        sizes = [13 * (q[3] - q[1] + 3) * (q[2] - q[0] + 3) for q in a["boxes"]]
        assert np.array_equal(np.diff(b["offsets"]), sizes), "the offsets are the prefix sums of the boxes' sizes"
        assert a["data"].tobytes() == b["data"].tobytes()
        for k, q in enumerate(a["boxes"]):
            assert b["fabs"][k].shape == (13, q[3] - q[1] + 3, q[2] - q[0] + 3)
            assert np.array_equal(b["fabs"][k].reshape(-1), a["data"][a["offsets"][k]:a["offsets"][k + 1]])
    assert back[0]["vec_ref_ratio"] == (2, 2) and back[0]["ref_ratio"] == 2
    assert back[1]["vec_ref_ratio"] == (1, 1) and back[1]["ref_ratio"] == 1, "1 on the finest level"


def test_anisotropic_cells_have_no_scalar_dx(plt, tmp_path):
    levels = make_levels(np.random.default_rng(12), ncomp=2, ghost=0, dx=(100.0, 50.0))
    path = str(tmp_path / "plot.2d.hdf5")
    plt.write_levels(path, ["a", "b"], levels, time=0.0, dt=8.0, ghost=0)
    names, back = plt.read_levels(path)
    assert names == ["a", "b"]
    assert [(v["dx"], v["dy"], v["dx_attr"], v["dt"], v["ghost"]) for v in back] == [(100.0, 50.0, 0.0, 8.0, 0), (50.0, 25.0, 0.0, 4.0, 0)]
    assert all(a["data"].tobytes() == b["data"].tobytes() for a, b in zip(levels, back))


def test_a_level_whose_offsets_do_not_fit_its_boxes_is_refused(plt, tmp_path):
    levels = make_levels(np.random.default_rng(13))
    levels[1]["offsets"] = levels[1]["offsets"].copy()
    levels[1]["offsets"][1] += 1
    with pytest.raises(RuntimeError) as e:
        plt.write_levels(str(tmp_path / "bad.hdf5"), plt.NAMES, levels, time=0.0)
    assert "box 0" in str(e.value)


def test_file_layout_is_chombos(plt, tmp_path):
    from suhmo_amd import checkpoint
    h5ls = os.path.join(checkpoint.hdf5_prefix() or "", "bin", "h5ls")
    if not os.path.exists(h5ls):
        pytest.skip("no h5ls next to the HDF5 library")
    path = str(tmp_path / "plot.hdf5")
    plt.write_levels(path, plt.NAMES, make_levels(np.random.default_rng(14)), time=1.0)
    out = subprocess.run([h5ls, "-r", path], stdout=subprocess.PIPE, check=True).stdout.decode().replace("\\", "")
    for need in ("/Chombo_global", "/level_0/Processors", "/level_1/boxes", "/level_1/data:datatype=0", "/level_1/data:offsets=0", "/level_1/data_attributes"):
        assert need in out, (need, out)
