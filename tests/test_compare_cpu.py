"""The rule of "COMPARE" (include/suhmo_hip.h) on its numpy twin tests/compare_ref.py: the cases that can be written down, the bound any order of
summation obeys, that the order of the block average can be told from numpy's, the exported symbol, and the per-cell header
suhmo_amd/csrc/suhmo_compare.h run on the host with the sanitizers over the layouts tests/test_gpu_compare.py compares the device on."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import compare_ref as cr
from tests import flatten_ref as fr
from tests import hierlayouts as hl
from tests import reduce_ref as rr

NX0, NY0 = hl.NX0, hl.NY0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO = [[(8, 4, 23, 15), (24, 4, 39, 15)]]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def random_values(boxes, seed, nx0=NX0, ny0=NY0):
    rng = np.random.default_rng(seed)
    return [[rng.uniform(-1.0, 3.0, size=(b[3] - b[1] + 1, b[2] - b[0] + 1)) for b in bl] for bl in fr.all_boxes(nx0, ny0, boxes)]


def test_identical_inputs_give_exactly_zero():
    v = random_values([], 3)
    norms, terms = cr.composite(NX0, NY0, 1.0, 0.5, [], v, v[0][0], 0)
    assert same_bits(norms, np.zeros(3)) and same_bits(terms, np.zeros((1, 3)))
    assert same_bits(cr.finest(v[0][0], v[0][0], 0.5), np.zeros(3))
    # ... and a field whose block sums are exact (0.75 everywhere) on two levels at r = 4 and 2
    v = [[np.full(x.shape, 0.75) for x in lv] for lv in random_values(TWO, 4)]
    norms, terms = cr.composite(NX0, NY0, 1.0, 1.0, TWO, v, np.full((NY0 << 2, NX0 << 2), 0.75), 2)
    assert same_bits(norms, np.zeros(3)) and same_bits(terms, np.zeros((2, 3)))


# a 2 x 1 level 0 whose cell (0, 0) is covered by the 2 x 2 box of level 1; dx0 = dy0 = 1, so w_0 = 1 and w_1 = 0.25.  Every value is a small
# multiple of a power of two: all sums are exact in any order.
#   exact_level 1 (r = 2 on level 0, 1 on level 1), exact = [[1 2 3 4] [5 6 7 9]]:
#     level 0, cell (1, 0): c = 5.5; block rows (3 + 4) = 7, (7 + 9) = 16; 7 + 16 = 23; avg = 23 / 4 = 5.75; e = -0.25: terms 0.25, 0.0625, 0.25
#     level 1: c = [[1.5 2] [5 5]] against [[1 2] [5 6]]: e = 0.5, 0, 0, -1: sum1 = 1.5 * 0.25 = 0.375, sum2 = 1.25 * 0.25 = 0.3125, max 1
#     norms: L1 = 0.625, L2 = sqrt(0.375), max = 1
#   exact_level 2 (r = 4 and 2), exact[j][i] = i + 8 j:
#     level 0, cell (1, 0): columns 4 .. 7, rows 0 .. 3: row sums (4 + 5) + (6 + 7) = 22, 54, 86, 118; 22 + 54 + 86 + 118 = 280; avg = 17.5; e = -12
#     level 1: blocks (0 + 1) + (8 + 9) = 18 -> 4.5, 26 -> 6.5, 82 -> 20.5, 90 -> 22.5; e = -3, -4.5, -15.5, -17.5:
#              sum1 = 40.5 * 0.25 = 10.125, sum2 = (9 + 20.25 + 240.25 + 306.25) * 0.25 = 143.9375, max 17.5
#     norms: L1 = 22.125, L2 = sqrt(144 + 143.9375), max = 17.5
HAND_BOXES = [[(0, 0, 1, 1)]]
HAND_VALUES = [[np.array([[100.0, 5.5]])], [np.array([[1.5, 2.0], [5.0, 5.0]])]]


def test_typed_out_by_hand():
    n, t = cr.composite(2, 1, 1.0, 1.0, HAND_BOXES, HAND_VALUES, np.array([[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 9.0]]), 1)
    assert same_bits(n, [0.625, math.sqrt(0.375), 1.0]) and same_bits(t, [[0.25, 0.0625, 0.25], [0.375, 0.3125, 1.0]])
    n, t = cr.composite(2, 1, 1.0, 1.0, HAND_BOXES, HAND_VALUES, np.arange(32.0).reshape(4, 8), 2)
    assert same_bits(n, [22.125, math.sqrt(287.9375), 17.5]) and same_bits(t, [[12.0, 144.0, 12.0], [10.125, 143.9375, 17.5]])
    assert same_bits(cr.block_average(np.arange(32.0).reshape(4, 8), 4), [[13.5, 17.5]])


def test_covered_cells_and_what_lies_under_them_do_not_count():
    bc, boxes = fr.case(6)
    top = len(boxes)
    vals = random_values(boxes, 6)
    rng = np.random.default_rng(7)
    exact = rng.uniform(-1.0, 3.0, size=(NY0 << (top + 1), NX0 << (top + 1)))
    want = cr.composite(NX0, NY0, 1.0, 1.0, boxes, vals, exact, top + 1)
    cov = cr.covers(NX0, NY0, boxes)
    assert sum(int(c.sum()) for lv in cov for c in lv) > 0
    # the covered cells of every level <- 1e300 and, seen from level 0 alone, the exact cells under its covered cells too
    for l in range(top):
        vals[l] = [np.where(c != 0, 1.0e300, v) for v, c in zip(vals[l], cov[l])]
    got = cr.composite(NX0, NY0, 1.0, 1.0, boxes, vals, exact, top + 1)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    r = 1 << (top + 1)
    poisoned = np.where(np.kron(cov[0][0], np.ones((r, r))) != 0, 1.0e300, exact)
    one = lambda x: cr.composite(NX0, NY0, 1.0, 1.0, [], [vals[0]], x, top + 1, cover=[cov[0]])
    assert same_bits(one(poisoned)[0], one(exact)[0]) and np.isfinite(one(poisoned)[0]).all()


def terms_of(boxes, vals, exact, el, dx0=1.0, dy0=1.0):
    """every term of a comparison as flat arrays (sum1's, sum2's, the |e|), covered cells left out"""
    cov = cr.covers(NX0, NY0, boxes)
    t = [[], [], []]
    for l, bl in enumerate(fr.all_boxes(NX0, NY0, boxes)):
        r = 1 << (el - l)
        for k, b in enumerate(bl):
            avg = cr.block_average(exact[b[1] * r:(b[3] + 1) * r, b[0] * r:(b[2] + 1) * r], r)
            keep = cov[l][k] == 0
            for m, x in enumerate(cr.cell_terms(vals[l][k], avg, (dx0 / 2 ** l) * (dy0 / 2 ** l))):
                t[m].append(x[keep])
    return [np.concatenate(x) for x in t]


@pytest.mark.parametrize("key", [1, 6, 11, "tiny-boxes"])
def test_the_max_is_exact_and_the_sums_lie_within_the_bound_of_any_order(key):
    bc, boxes = fr.case(key)
    top = len(boxes)
    vals = random_values(boxes, 8)
    exact = np.random.default_rng(9).uniform(-1.0, 3.0, size=(NY0 << (top + 1), NX0 << (top + 1)))
    norms, _ = cr.composite(NX0, NY0, 1.0, 1.0, boxes, vals, exact, top + 1)
    t1, t2, ae = terms_of(boxes, vals, exact, top + 1)
    assert norms[2] == np.max(ae)
    for got, t in ((norms[0], t1), (norms[1] ** 2, t2)):
        # (n - 1) 2^-53 sum |t| for the sum itself; sqrt and its square cost another 2 ulp of the sum
        bound = (t.size - 1) * 2.0 ** -53 * math.fsum(t) + (4 * 2.0 ** -53 * math.fsum(t) if t is t2 else 0.0)
        assert abs(got - math.fsum(t)) <= bound, (key, got, math.fsum(t), bound)
    flat = np.random.default_rng(10).uniform(-1.0, 3.0, size=exact.shape)
    n = cr.finest(flat, exact, 0.125)
    e = flat - exact
    assert n[2] == np.max(np.abs(e))
    t = (np.abs(e) * 0.125).reshape(-1)
    assert abs(n[0] - math.fsum(t)) <= (t.size - 1) * 2.0 ** -53 * math.fsum(t)


def test_the_order_of_the_block_average_can_be_told_from_numpys():
    """on data of reduce_ref.inputs' kind (both signs, magnitude 1 .. 2: the sums cancel and round) the rule's order, numpy's mean and a serial
    sum over the block disagree in some cells -- a kernel with another order cannot pass the bitwise tests"""
    x, _ = rr.inputs(256, 128)
    for r in (2, 4, 16):
        ours = cr.block_average(x, r)
        blocks = x.reshape(128 // r, r, 256 // r, r)
        mean = blocks.mean(axis=(1, 3))
        serial = np.zeros(ours.shape)
        for q in range(r):
            for p in range(r):
                serial = serial + blocks[:, q, :, p]
        serial = serial * (1.0 / (r * r))
        cols_first = cr.block_average(x.T, r).T                # the tree along y, the rows of it along x
        if r > 2:
            assert (ours != serial).any() and (ours != cols_first).any(), r
        if r > 4:
            assert (ours != mean).any(), r
        assert np.allclose(ours, mean, rtol=0, atol=16 * r * r * 2.0 ** -53)
    assert same_bits(cr.row_tree(np.array([1.0, 2.0 ** -53, 2.0 ** -53, 0.0])), 1.0)          # (1 + u) + (u + 0): 1 + u rounds to 1, twice
    assert cr.row_tree(np.array([2.0 ** -53, 2.0 ** -53, 1.0, 0.0])) == 1.0 + 2.0 ** -52           # (u + u) + (1 + 0)


def test_the_library_exports_the_call():
    from suhmo_amd import capi
    capi.build()
    assert "suhmo_hier_compare" in capi.SYMBOLS and hasattr(ctypes.CDLL(capi.LIB_PATH), "suhmo_hier_compare")
    hdr = open(os.path.join(ROOT, "include", "suhmo_hip.h")).read()
    assert "---- COMPARE" in hdr and hdr.index("---- FLATTEN") < hdr.index("---- COMPARE") < hdr.index("---- OUTPUT INSIDE THE RUN")
    assert (capi.CMP_COMPOSITE, capi.CMP_FINEST) == (0, 1)


# ------------------------------------------------------------------ the per-cell header on the host
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("compare_emu")
    exe = str(d / "compare_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                           os.path.join(ROOT, "tests", "host_cpp", "compare_emu.cpp"), "-o", exe])
    return exe, d


def _canvas(valid, poison):
    """the valid cells in a canvas of the library's shape: cell (i, j) at (j + 1) * P + 16 + i, P a multiple of 16, one ghost ring and one spare
    row; everything but the valid cells is poison"""
    ny, nx = valid.shape
    P = ((16 + nx + 1 + 15) // 16) * 16
    c = np.full((ny + 3, P), poison)
    c[1:ny + 1, 16:16 + nx] = valid
    return P, c.reshape(-1)


@pytest.mark.parametrize("key", [k for _, k in fr.CASES], ids=[n for n, _ in fr.CASES])
def test_the_header_on_the_host_equals_the_twin(emu, key):
    """every layout of the GPU sweep at the finest level and one above it, a FIELD and a DIFF.  Ghost rings and the canvas beyond them are
    poisoned, and so are the covered cells (every exact cell lies under exactly one cell that counts: none of them can be); the canvases are
    heap blocks of the library's size"""
    exe, d = emu
    bc, boxes = fr.case(key)
    allb = fr.all_boxes(NX0, NY0, boxes)
    cov = cr.covers(NX0, NY0, boxes)
    top = len(boxes)
    for el in (top, top + 1):
        for diff in (0, 1):
            a, b = random_values(boxes, [11, el]), random_values(boxes, [12, el])
            rng = np.random.default_rng([13, el])
            xa, xb = (rng.uniform(-1.0, 3.0, size=(NY0 << el, NX0 << el)) for _ in range(2))
            vals = [[cr.component(diff, p, q) for p, q in zip(la, lb)] for la, lb in zip(a, b)]
            ref, lt = cr.composite(NX0, NY0, 1.0, 0.5, boxes, vals, cr.component(diff, xa, xb), el)
            with open(d / "in.bin", "wb") as f:
                f.write(struct.pack("3i", top + 1, el, diff))
                P, c = _canvas(xa, 7.0e77)
                f.write(struct.pack("5i", NX0 << el, NY0 << el, P, 1, c.size))
                f.write(c.tobytes())
                if diff:
                    f.write(_canvas(xb, 7.0e77)[1].tobytes())
                for l, bl in enumerate(allb):
                    f.write(struct.pack("i", len(bl)))
                    f.write(struct.pack("d", (1.0 / 2 ** l) * (0.5 / 2 ** l)))
                    for k, bx in enumerate(bl):
                        P, c = _canvas(np.where(cov[l][k] != 0, 5.0e55, a[l][k]), 7.0e77)
                        f.write(struct.pack("7i", bx[2] - bx[0] + 1, bx[3] - bx[1] + 1, bx[0], bx[1], P, 1, c.size))
                        f.write(c.tobytes())
                        if diff:
                            f.write(_canvas(b[l][k], 7.0e77)[1].tobytes())
                        f.write(_canvas(cov[l][k], 7.0e77)[1].tobytes())
            r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
            assert r.returncode == 0, (key, el, diff, r.stderr[-3000:])
            out = np.fromfile(d / "out.bin")
            assert same_bits(out[:3], ref) and same_bits(out[3:].reshape(-1, 3), lt), (key, el, diff, out, ref, lt)
