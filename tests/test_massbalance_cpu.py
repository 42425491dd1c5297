"""The rule of "MASS BALANCE" (include/suhmo_hip.h) on its numpy twin tests/massbalance_ref.py: the answers that can be typed out by hand, a margin
face two boxes share, the bound any order of summation obeys, the census of the sweep's inputs as a condition, the declared and exported symbols,
the loud failure without a device, and the per-cell header suhmo_amd/csrc/suhmo_balance.h run on the host with the sanitizers over the layouts
tests/test_gpu_massbalance.py compares the device on."""
import ctypes as C
import math
import os
import struct
import subprocess
from collections import Counter

import numpy as np
import pytest

from tests import massbalance_ref as mb
from tests import reduce_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEU0 = dict(type=[[0, 0], [1, 1]], value=[[0.0, 8.0], [0.0, 0.0]], periodic=[0, 0])      # Dirichlet 0 and 8 in x, Neumann 0 in y


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def whole(nx, ny):
    return [(0, 0, nx - 1, ny - 1)]


# ------------------------------------------------------------------ answers typed out by hand
# 8 x 4 cells, dx = 0.5, dy = 0.25 (Lx = 4, Ly = 1); every number a small multiple of a power of two: all sums are exact in any order.
#   head = i + 0.5 (linear in x, slope 2 per unit length), Dirichlet 0 at x = 0 and 8 at x = 4: the ghosts 2 * 0 - 0.5 = -0.5 and 2 * 8 - 7.5 = 8.5
#   continue the line; Neumann 0 in y: the ghost is the cell.  Every x-face: gradphi = (1) * (-1) / 0.5 = -2, flux = -1 * -2 = 2, t = 2 * 0.25 = 0.5;
#   every y-face 0.  No mask (+1 everywhere): LO_X = HI_X = 4 rows * 0.5 = 2; the domain faces are the only ones with mec = 0, d = 0, mhi > 0:
#   DIR_X = +2 - 2 = 0 = LO_X - HI_X.  With K = 3 on the high domain face alone: HI_X = 6, DIR_X = 2 - 6 = -4.
#   B = 0.375 everywhere: VOLUME = 0.375 * 4 * 1 = 1.5
def linear_case(k_hi=1.0):
    nx, ny = 8, 4
    head = np.zeros((ny + 2, nx + 2)) + (np.arange(-1, nx + 1) + 0.5)[None, :]
    head[:, 0] = head[:, -1] = 1.0e300                       # the stored ghosts of a physical side are not read
    bx = np.ones((ny, nx + 1))
    bx[:, nx] = k_hi
    return dict(head=head, mask=np.ones((ny + 2, nx + 2)), B=np.full((ny, nx), 0.375), bx=bx, by=np.ones((ny + 1, nx)))


def test_a_head_linear_in_x_without_a_mask():
    out = mb.balance_of_level([linear_case()], whole(8, 4), (8, 4), NEU0, 0.5, 0.25)
    assert same_bits(out, [2.0, 2.0, 0.0, 0.0, 0.0, 0.0, 1.5]), out
    assert out[mb.LO_X] == out[mb.HI_X] and out[mb.DIR_X] == out[mb.LO_X] - out[mb.HI_X]
    out = mb.balance_of_level([linear_case(3.0)], whole(8, 4), (8, 4), NEU0, 0.5, 0.25)
    assert same_bits(out, [2.0, 6.0, 0.0, 0.0, -4.0, 0.0, 1.5]), out
    assert out[mb.DIR_X] == out[mb.LO_X] - out[mb.HI_X]


# the same grid; ice (+1) in the cells i = 2 .. 5, j = 1 .. 2, -1 elsewhere, ghost cells included.  K = 0 on every face between two ice-free cells
# (what bcoef_face leaves there with cutOffB), so nothing crosses the domain sides: LO = HI = 0.  head = c[i] + 16 j, c = 0 0 1 2 4 8 0 0.
#   left edge (face 2, rows 1 and 2): gradphi = (1 - 0) * -1 / 0.5 = -2, flux 2, t = 0.5; lower margin (d = +2): DIR_X += 0.5, twice
#   right edge (face 6): gradphi = (0 - 8) * -1 / 0.5 = 16, flux -16, t = -4; upper margin: DIR_X -= -4, twice          DIR_X = 1 + 8 = 9
#   bottom edge (face j = 1, columns 2 .. 5): gradphi = 16 * -1 / 0.25 = -64, flux 64 K; K = 1: t = 64 * 0.5 = 32; lower margin: += 32, four times
#   top edge (face j = 3): K = 0.5: t = 16; upper margin: -= 16, four times                                              DIR_Y = 128 - 64 = 64
#   the faces inside the ice carry K = 7 and do not count; B = 0.25 in the ice, 5 outside: VOLUME = 8 cells * 0.25 * 0.125 = 0.25
def rectangle_case():
    nx, ny = 8, 4
    mask = -np.ones((ny + 2, nx + 2))
    mask[2:4, 3:7] = 1.0
    c = np.array([0.0, 0.0, 0.0, 1.0, 2.0, 4.0, 8.0, 0.0, 0.0, 0.0])
    head = c[None, :] + 16.0 * np.arange(-1, ny + 1)[:, None]
    ice = mask[1:-1, 1:-1] > 0
    bx, by = np.zeros((ny, nx + 1)), np.zeros((ny + 1, nx))
    bx[1:3, 3:6] = 7.0; bx[1:3, 2] = 1.0; bx[1:3, 6] = 1.0
    by[2, 2:6] = 7.0; by[1, 2:6] = 1.0; by[3, 2:6] = 0.5
    return dict(head=head, mask=mask, B=np.where(ice, 0.25, 5.0), bx=bx, by=by)


def test_an_ice_rectangle_inside_the_domain():
    out = mb.balance_of_level([rectangle_case()], whole(8, 4), (8, 4), NEU0, 0.5, 0.25)
    assert same_bits(out, [0.0, 0.0, 0.0, 0.0, 9.0, 64.0, 0.25]), out


# ------------------------------------------------------------------ a margin face on a side two boxes share
def test_a_margin_face_two_boxes_share_counts_twice():
    """a level of 8 x 4 cells inside a 16 x 8 domain, ice for i < 8 and none beyond: the margin is the column of faces I = 8.  As one box (4, 2,
    11, 5) the level counts each of its four faces once; cut at the margin into (4, 2, 7, 5) and (8, 2, 11, 5) both boxes walk it -- the first as
    its high faces, the second as its low faces -- and DIR_X doubles exactly, as the reference's walk over every box's faces does"""
    dom = (16, 8)
    lvl = mb.synthetic_level(16, 8, (0, 0), 5)
    mask = np.ones((10, 18))
    mask[:, 9:] = -1.0                                       # ghosted column 9 = cell 8
    one, two = [(4, 2, 11, 5)], [(4, 2, 7, 5), (8, 2, 11, 5)]
    a = mb.balance_of_level([mb.cut_data(lvl, mask, b) for b in one], one, dom, mb.NEUMANN_BC, 0.5, 0.5, rr.CAP_BOX)
    b = mb.balance_of_level([mb.cut_data(lvl, mask, b) for b in two], two, dom, mb.NEUMANN_BC, 0.5, 0.5, rr.CAP_BOX)
    t = [-(-lvl["bx"][j, 8] * ((lvl["head"][j + 1, 9] - lvl["head"][j + 1, 8]) * -1.0 / 0.5)) * 0.5 for j in range(2, 6)]     # an upper margin: -= t
    assert a[mb.DIR_X] == math.fsum(t) and b[mb.DIR_X] == 2.0 * a[mb.DIR_X] and a[mb.DIR_X] != 0.0, (a, b, t)
    assert same_bits(a[mb.DIR_Y], 0.0) and same_bits(b[mb.DIR_Y], 0.0) and a[mb.VOLUME] == b[mb.VOLUME]
    assert same_bits(a[:4], np.zeros(4)) and same_bits(b[:4], np.zeros(4)), "no face of the level is a domain face"
    c = mb.census([mb.cut(mask, x) for x in two], two, dom, (0, 0))
    assert c["shared_margin"] == 8 and c["margin_upper_x"] == 8 and c["coarse_fine_side"] == 2 * (4 + 4) + 2 * 4


# ------------------------------------------------------------------ the sweep's inputs
def level_inputs(nx0, ny0, bc, boxes, masks, seed=3):
    """per level: (boxes, domain, dx, dy, data of every box) with synthetic fields"""
    out = []
    for l, bl in enumerate([whole(nx0, ny0)] + [list(b) for b in boxes]):
        nx, ny = nx0 << l, ny0 << l
        lvl = mb.synthetic_level(nx, ny, bc["periodic"], seed + l)
        out.append((bl, (nx, ny), 1.0 / 2 ** l, 0.5 / 2 ** l, [mb.cut_data(lvl, masks[l], b) for b in bl]))
    return out


SWEEP = list(mb.sweep_layouts())


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_every_sum_lies_within_the_bound_of_any_order(case):
    """|twin - fsum(terms)| <= (n - 1) 2^-53 sum |t| for each of the seven values of every level (n: the terms that are not 0)"""
    name, nx0, ny0, bc, boxes, masks = case
    for l, (bl, dom, dx, dy, data) in enumerate(level_inputs(nx0, ny0, bc, boxes, masks)):
        seqs = [mb.terms_of(d, b, dom, bc, dx, dy) for d, b in zip(data, bl)]
        got = mb.level_balance(seqs, rr.CAP_LEVEL if l == 0 else rr.CAP_BOX)
        for q, t in enumerate(mb.level_terms(seqs)):
            n = int(np.count_nonzero(t))
            exact = math.fsum(t.tolist())
            bound = max(n - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(t).tolist())
            assert abs(got[q] - exact) <= bound, (name, l, mb.NAMES[q], got[q], exact, bound)
        assert np.isfinite(got).all() and got[mb.VOLUME] > 0.0


def test_the_sweep_holds_every_class_of_face():
    total = Counter()
    for name, nx0, ny0, bc, boxes, masks in SWEEP:
        for l, bl in enumerate([whole(nx0, ny0)] + [list(b) for b in boxes]):
            total += mb.census([mb.cut(masks[l], b) for b in bl], bl, (nx0 << l, ny0 << l), bc["periodic"])
    print(dict(total))
    assert all(total[k] >= 1 for k in mb.CLASSES), {k: total[k] for k in mb.CLASSES if total[k] < 1}


# ------------------------------------------------------------------ symbols, loud failure
MB_SYMBOLS = ("suhmo_level_mass_balance", "suhmo_hier_mass_balance", "suhmo_batch_mass_balance")


def test_the_calls_are_declared_listed_and_exported():
    from suhmo_amd import capi
    capi.build()
    header = open(os.path.join(ROOT, "include", "suhmo_hip.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    for s in MB_SYMBOLS:
        assert ("int %s(" % s) in header and s in capi.SYMBOLS and hasattr(lib, s), s
    assert "MASS BALANCE" in header and "SUHMO_MB_COUNT" in header
    assert capi.MB_NAMES == mb.NAMES and len(capi.MB_NAMES) == 7


def test_the_calls_fail_loudly_without_a_device():
    from suhmo_amd import capi, model, synthetic as sy
    lib = capi.lib()
    out = (C.c_double * 7)()
    fake = C.c_void_p(8)                                     # never dereferenced: the argument check comes first
    assert lib.suhmo_level_mass_balance(None, out, None) == -1 and b"bad argument" in lib.suhmo_last_error()
    assert lib.suhmo_level_mass_balance(fake, None, None) == -1 and b"bad argument" in lib.suhmo_last_error()
    assert lib.suhmo_hier_mass_balance(None, out, None) == -1 and lib.suhmo_hier_mass_balance(fake, None, None) == -1
    assert lib.suhmo_batch_mass_balance(None, out, None, None) == -1 and lib.suhmo_batch_mass_balance(fake, None, None, None) == -1
    assert all(callable(f) for f in (model.HipModel.mass_balance, model.HipHierModel.mass_balance, model.HipBatchModel.mass_balance_all))
    if lib.suhmo_device_count() == 0:                        # no device, no fallback: the model cannot even be created
        with pytest.raises(capi.SuhmoError):
            model.HipModel(64, 4, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS, sy.A3_MODEL).mass_balance()


# ------------------------------------------------------------------ the per-cell header on the host
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("balance_emu")
    exe = str(d / "balance_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                           os.path.join(ROOT, "tests", "host_cpp", "balance_emu.cpp"), "-o", exe])
    return exe, d


POISON = float("nan")


def _canvas(nx, ny):
    """a canvas of the library's shape full of poison: cell (i, j) at (j + 1) * P + 16 + i, P a multiple of 16, one ghost ring and one spare row"""
    P = ((nx + 32 + 15) // 16) * 16
    return P, np.full((ny + 3, P), POISON)


def _box_record(d, box, dom, bc, dx, dy):
    """the view the library would hold of this box and its five canvases: the head with its stored ghosts on the sides where the device reads
    them and poison elsewhere, the mask with its four ghost sides (no corners), B's valid cells, the faces"""
    lo0, lo1, hi0, hi1 = box
    nx, ny = hi0 - lo0 + 1, hi1 - lo1 + 1
    modes = mb.side_modes(box, dom, bc["periodic"])
    P, head = _canvas(nx, ny)
    mask, B, bx, by = (head.copy() for _ in range(4))
    head[1:ny + 1, 16:16 + nx] = d["head"][1:-1, 1:-1]
    mask[1:ny + 1, 16:16 + nx] = d["mask"][1:-1, 1:-1]
    for a, src, every in ((head, d["head"], False), (mask, d["mask"], True)):
        if every or modes[(0, 0)] == "stored": a[1:ny + 1, 15] = src[1:-1, 0]
        if every or modes[(0, 1)] == "stored": a[1:ny + 1, 16 + nx] = src[1:-1, -1]
        if every or modes[(1, 0)] == "stored": a[0, 16:16 + nx] = src[0, 1:-1]
        if every or modes[(1, 1)] == "stored": a[ny + 1, 16:16 + nx] = src[-1, 1:-1]
    B[1:ny + 1, 16:16 + nx] = d["B"][1:-1, 1:-1] if d["B"].shape == (ny + 2, nx + 2) else d["B"]
    bx[1:ny + 1, 16:16 + nx + 1] = d["bx"]
    by[1:ny + 2, 16:16 + nx] = d["by"]
    st = lambda k: int(modes[k] == "stored")
    ints = [nx, ny, P, 1, lo0, lo1, dom[0], dom[1], int(bc["periodic"][0]), int(bc["periodic"][1]), st((0, 0)), st((0, 1)), st((1, 0)), st((1, 1))]
    ints += [int(bc["type"][dr][s]) for dr in range(2) for s in range(2)] + [head.size]
    h = (dx, dy)
    dbl = [dx, dy] + [2.0 * bc["value"][dr][s] for dr in range(2) for s in range(2)]
    dbl += [((-1.0 if s == 0 else 1.0) * h[dr]) * bc["value"][dr][s] for dr in range(2) for s in range(2)]
    return struct.pack("19i", *ints) + struct.pack("10d", *dbl) + b"".join(a.tobytes() for a in (head, mask, B, bx, by))


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_the_header_on_the_host_equals_the_twin(emu, case):
    """every layout of the GPU sweep: whatever the rule must not read is NaN, the canvases are heap blocks of the library's size; the serial form of
    the header equals the twin bit for bit and the sanitizers stay silent"""
    exe, d = emu
    name, nx0, ny0, bc, boxes, masks = case
    levels = level_inputs(nx0, ny0, bc, boxes, masks)
    blob = struct.pack("i", len(levels))
    want = []
    for l, (bl, dom, dx, dy, data) in enumerate(levels):
        cap = rr.CAP_LEVEL if l == 0 else rr.CAP_BOX
        blob += struct.pack("3i", len(bl), *cap) + b"".join(_box_record(x, b, dom, bc, dx, dy) for x, b in zip(data, bl))
        want.append(mb.balance_of_level(data, bl, dom, bc, dx, dy, cap))
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    with open(fin, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (name, r.returncode, r.stderr[-2000:])
    got = np.fromfile(fout).reshape(len(levels), 7)
    assert np.isfinite(got).all(), (name, got)
    assert same_bits(got, np.array(want)), (name, got, want)
