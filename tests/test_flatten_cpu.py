"""The rule of "FLATTEN" (include/suhmo_hip.h) on its numpy twin tests/flatten_ref.py: the arithmetic cases that can be written down, the
file name of the reference, the census of the sweep tests/test_gpu_flatten.py compares the device against, and the exported symbol."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import flatten_ref as fr
from tests import hierlayouts as hl
from tests import regrid_ref as rr

NX0, NY0 = hl.NX0, hl.NY0
TWO = [[(8, 4, 23, 15), (24, 4, 39, 15)]]


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def values_of(boxes, fn, nx0=NX0, ny0=NY0):
    """values[l][k] of flatten_ref.flatten from fn(l, global i (nx,), global j (ny,)) -> (ny, nx)"""
    return [[fn(l, np.arange(b[0], b[2] + 1), np.arange(b[1], b[3] + 1)) for b in bl] for l, bl in enumerate(fr.all_boxes(nx0, ny0, boxes))]


def random_values(boxes, seed, nx0=NX0, ny0=NY0):
    rng = np.random.default_rng(seed)
    return [[rng.uniform(-1.0, 3.0, size=(b[3] - b[1] + 1, b[2] - b[0] + 1)) for b in bl] for bl in fr.all_boxes(nx0, ny0, boxes)]


def test_a_constant_comes_back_bit_for_bit():
    for per in ((0, 0), (1, 1)):
        vals = values_of(TWO, lambda l, i, j: np.full((j.size, i.size), 0.1))
        out, _ = fr.flatten(NX0, NY0, per, TWO, vals, 3)
        assert out.shape == (NY0 << 3, NX0 << 3) and same_bits(out, np.full(out.shape, 0.1))


def test_ratio_one_is_a_copy():
    vals = random_values([], 3)
    out, census = fr.flatten(NX0, NY0, (0, 1), [], vals, 0)
    assert same_bits(out, vals[0][0]) and not any(census.values())
    # ... and the finest level of a hierarchy is copied over what level 0 wrote
    vals = random_values(TWO, 4)
    out, _ = fr.flatten(NX0, NY0, (0, 0), TWO, vals, 1)
    for b, v in zip(TWO[0], vals[1]):
        assert same_bits(out[b[1]:b[3] + 1, b[0]:b[2] + 1], v)


def test_ratio_two_is_the_regrid_interpolation():
    """max_level = 1 over level 0 alone: the same arithmetic as rule (a) of the regrid, whose offsets are written +-0.25"""
    for per in ((0, 0), (1, 0), (0, 1), (1, 1)):
        vals = random_values([], 5)
        out, _ = fr.flatten(NX0, NY0, per, [], vals, 1)
        for J in range(NY0):
            for I in range(NX0):
                v, _ = rr.interp_cell(vals[0][0], I, J, (NX0, NY0), per)
                assert same_bits(out[2 * J:2 * J + 2, 2 * I:2 * I + 2], np.array(v)), (per, I, J)


def test_block_means_of_an_exactly_representable_field():
    """8 x an integer plane at r = 4: away from the domain sides every slope is a multiple of 8 and the limiter inactive (the extrema of the
    block lie 40 from the cell, deltasum is 20), so every child is an integer and the 16 children of a cell average to the cell exactly.  (In a
    cell on a domain side the block lacks a row or a column, and on two of the sides eta = 0.8 cuts the tangential slope.)"""
    vals = values_of([], lambda l, i, j: 8.0 * (3.0 * i[None, :] - 2.0 * j[:, None] + 7.0))
    out, census = fr.flatten(NX0, NY0, (0, 0), [], vals, 2)
    assert census["one_sided"] == 2 * NX0 + 2 * NY0 - 4
    inner = out[4:-4, 4:-4]
    assert (inner == np.round(inner)).all()
    means = inner.reshape(NY0 - 2, 4, NX0 - 2, 4).sum(axis=(1, 3)) / 16.0
    assert same_bits(means, vals[0][0][1:-1, 1:-1])


# one 3 x 3 block, the middle cell at r = 4, by hand from the rule: c0 = 6; s0 = 0.5 (7 - 2) = 2.5, s1 = 0.5 (5 - 2) = 1.5; smax = 7, smin = 1;
# deltasum = 0.5 (2.5 + 1.5) = 2; etamax = (7 - 6) / 2 = 0.5, etamin = (6 - 1) / 2 = 2.5: eta = 0.5, s0 = 1.25, s1 = 0.75; the offsets are
# -0.375, -0.125, 0.125, 0.375: v(p, q) = 6 + 1.25 dx_p + 0.75 dy_q (every product and sum exact)
BLOCK = np.array([[1.0, 2.0, 3.0], [2.0, 6.0, 7.0], [3.0, 5.0, 6.5]])
BY_HAND = np.array([[5.25, 5.5625, 5.875, 6.1875], [5.4375, 5.75, 6.0625, 6.375], [5.625, 5.9375, 6.25, 6.5625], [5.8125, 6.125, 6.4375, 6.75]])


def test_typed_out_block_with_an_active_limiter():
    assert same_bits(fr.offsets(4), np.array([-0.375, -0.125, 0.125, 0.375]))
    out, census = fr.flatten(3, 3, (0, 0), [], [[BLOCK]], 2)
    assert same_bits(out[4:8, 4:8], BY_HAND)
    assert census["limited"] >= 1


def test_the_difference_is_formed_before_the_interpolation():
    other = np.array([[0.5, 4.0, 1.0], [3.0, 2.0, 0.0], [1.5, 2.5, 6.0]])
    of = lambda a: fr.flatten(3, 3, (0, 0), [], [[a]], 2)[0][4:8, 4:8]
    assert not np.array_equal(of(BLOCK - other), of(BLOCK) - of(other)), "the limiter is not linear"


def test_pp_name_is_the_reference_pattern():
    from suhmo_amd import plotfile
    # sprintf(iter_str, "%sCustom%06d", m_plot_prefix.c_str(), m_cur_step) + ".2d" + ".hdf5" (src/AmrHydro.cpp:5349-5361, :4823)
    assert plotfile.pp_name("plot", 1501) == "plotCustom001501.2d.hdf5"
    assert plotfile.pp_name("out/run_", 7) == "out/run_Custom000007.2d.hdf5"
    assert re.fullmatch(r"pCustom\d{6}\.2d\.hdf5", plotfile.pp_name("p", 0))


def test_the_sweep_meets_every_class_of_the_census():
    """the cases and the data of tests/test_gpu_flatten.py (component 0 of its list, the finest level + 1): every way a coarse cell can be
    treated occurs, and the limiter is active in a cell that reads the edge clause"""
    total = dict.fromkeys(fr.CLASSES, 0)
    for name, key in fr.CASES:
        bc, boxes = fr.case(key)
        assert hl.valid(NX0, NY0, bc["periodic"], boxes), name
        vals = [[fr.random_box(fr.DATA_SEED, key, l, k, 0, b)[1:-1, 1:-1] for k, b in enumerate(bl)] for l, bl in enumerate(fr.all_boxes(NX0, NY0, boxes))]
        _, census = fr.flatten(NX0, NY0, bc["periodic"], boxes, vals, len(boxes) + 1)
        for nm in fr.CLASSES:
            total[nm] += census[nm]
    assert all(total[nm] > 0 for nm in fr.CLASSES), total
    assert {len(fr.case(k)[1]) for _, k in fr.CASES} == {1, 2, 3}
    assert {tuple(fr.case(k)[0]["periodic"]) for _, k in fr.CASES} == {(0, 0), (1, 0), (0, 1), (1, 1)}


def test_the_library_exports_the_call():
    from suhmo_amd import capi
    capi.build()
    assert "suhmo_hier_flatten" in capi.SYMBOLS and hasattr(ctypes.CDLL(capi.LIB_PATH), "suhmo_hier_flatten")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "suhmo_hip.h")).read()
    assert "---- FLATTEN" in hdr
    assert ctypes.sizeof(capi.FlatComp) == 12 and (capi.FLAT_FIELD, capi.FLAT_DIFF) == (0, 1)


# ------------------------------------------------------------------ the interpolation kernel's own text, on the host
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/host_cpp/flatten_emu.cpp around the text of k_flat_interp as suhmo_flatten.hip holds it, with the sanitizers"""
    d = tmp_path_factory.mktemp("flatten_emu")
    src = open(os.path.join(ROOT, "suhmo_amd", "csrc", "suhmo_flatten.hip")).read()
    inc = d / "k_flat_interp.inc"
    inc.write_text(src[src.index("template <bool COPY> __global__"):src.index("int flat_comps(")])
    exe = str(d / "flatten_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                           '-DFLATTEN_KERNEL_INC="%s"' % inc, os.path.join(ROOT, "tests", "host_cpp", "flatten_emu.cpp"), "-o", exe])
    return exe, d


def _canvas(g, poison):
    """a ghosted box in a canvas of the library's shape: cell (i, j) at (j + 1) * P + 16 + i, P a multiple of 16, one spare row"""
    ny, nx = g.shape[0] - 2, g.shape[1] - 2
    P = ((16 + nx + 1 + 15) // 16) * 16
    c = np.full((ny + 3, P), poison)
    c[0:ny + 2, 15:15 + nx + 2] = g
    return P, c.reshape(-1)


@pytest.mark.parametrize("key", [k for _, k in fr.CASES], ids=[n for n, _ in fr.CASES])
def test_the_kernel_text_on_the_host_equals_the_twin(emu, key):
    """every layout of the GPU sweep at the finest level and one above it, with the cap on the grid at the library's 8192 workgroups and at 5 (rows
    taken in several passes).  The scratch rings are what step (ii) leaves (regrid_ref.regrid builds them: exchange, else the linear fill);
    every cell the kernel must not read -- across a non-periodic side, level 0's ring, the canvas beyond the ghosted box -- is poisoned, and the
    canvases are heap blocks of the library's size: a read or a store outside one ends the run"""
    exe, d = emu
    bc, boxes = fr.case(key)
    per = bc["periodic"]
    base = np.random.default_rng(5).uniform(-1.0, 3.0, size=(NY0 + 2, NX0 + 2))
    ghosted = [[base]] + rr.regrid(NX0, NY0, per, [], boxes, [], base, None)
    allb = fr.all_boxes(NX0, NY0, boxes)
    for l, bl in enumerate(allb):
        n = (NX0 << l, NY0 << l)
        for g, b in zip(ghosted[l], bl):
            for jj in range(g.shape[0]):
                for ii in range(g.shape[1]):
                    inside = 1 <= ii <= g.shape[1] - 2 and 1 <= jj <= g.shape[0] - 2
                    if not inside and (l == 0 or rr._wrapped(b[0] + ii - 1, b[1] + jj - 1, n, per) is None):
                        g[jj, ii] = 9.0e99
    vals = [[g[1:-1, 1:-1] for g in gl] for gl in ghosted]
    top = len(boxes)
    for ml in (top, top + 1):
        ref, _ = fr.flatten(NX0, NY0, per, boxes, vals, ml)
        with open(d / "in.bin", "wb") as f:
            f.write(struct.pack("7i", NX0, NY0, per[0], per[1], top + 1, ml, 1))
            for l, bl in enumerate(allb):
                f.write(struct.pack("i", len(bl)))
                for g, b in zip(ghosted[l], bl):
                    P, c = _canvas(g, 7.0e77)
                    f.write(struct.pack("7i", b[2] - b[0] + 1, b[3] - b[1] + 1, b[0], b[1], P, 1, c.size))
                    f.write(c.tobytes())
        for cap in ("8192", "5"):
            r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin"), cap], capture_output=True, text=True)
            assert r.returncode == 0, (key, ml, cap, r.stderr[-3000:])
            out = np.fromfile(d / "out.bin").reshape(ref.shape)
            assert same_bits(out, ref), (key, ml, cap, int((out.view(np.uint64) != ref.view(np.uint64)).sum()))
