"""The inter-level transfer rules of suhmo_amd/csrc/suhmo_transfer.h, each stated once for every kernel that applies it, compiled on the HOST
(tests/host_cpp/transfer_rules.cpp: -ffp-contract=off, address and undefined-behaviour sanitizers, a child process) and compared bit for bit with
the numpy twins the tests hold: regrid_ref.limited_slopes / child, npref.restrict_sum4, and one-line expressions with the association spelled
out by parentheses.  Needs no device."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import npref
from tests import regrid_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4000                                                    # random operand sets per rule


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    d = tmp_path_factory.mktemp("transfer_rules")
    exe = str(d / "transfer_rules")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                           os.path.join(ROOT, "tests", "host_cpp", "transfer_rules.cpp"), "-o", exe])

    def run(rule, rows, nout):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        rows.tofile(d / "in.bin")
        r = subprocess.run([exe, rule, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (rule, r.returncode, r.stderr[-3000:])
        return np.fromfile(d / "out.bin").reshape(rows.shape[0], nout)
    return run


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def mismatches(a, b):
    return np.flatnonzero((np.asarray(a).view(np.uint64) != np.asarray(b, dtype=np.float64).view(np.uint64)).any(axis=1))[:5].tolist()


def operands(seed, n, k):
    """n rows of k operands: values of mixed sign and magnitude, then rows of +-0.0, rows with all operands equal, and small integers (ties)"""
    rng = np.random.default_rng(seed)
    q = n // 8
    a = rng.uniform(-3.0, 3.0, size=(n - 3 * q, k)) * 10.0 ** rng.integers(-3, 4, size=(n - 3 * q, 1))
    zeros = rng.choice([0.0, -0.0], size=(q, k))
    equal = np.repeat(rng.choice([0.0, -0.0, 1.0, -2.5, 0.1, 1.0e-300], size=(q, 1)), k, axis=1)
    ints = rng.integers(-2, 3, size=(q, k)).astype(np.float64)
    return np.concatenate([a, zeros, equal, ints])


# ------------------------------------------------------------------ PiecewiseLinearFillPatch / FineInterp
def slope_blocks():
    """3 x 3 blocks: random, +-0.0 only, all nine equal, small integers (ties in the extrema, eta exactly 0 or 1), and blocks whose central
    differences vanish while the extrema do not (deltasum == 0 with smax > c0 > smin)"""
    b = operands(11, 1600, 9)
    flat = operands(12, 200, 9)
    flat[:, 3] = flat[:, 5]
    flat[:, 1] = flat[:, 7]
    return np.concatenate([b, flat])


def test_limited_slopes_and_child_equal_the_regrid_twin(rules):
    """both values of tangential_only, every combination of missing neighbours (a missing cell holds NaN: it must not be read)"""
    blocks = slope_blocks()
    rows, want_s, want_v = [], [], []
    combos = list(itertools.product((0, 1), repeat=5))
    assert len(combos) == 32
    deltasum0 = limited = 0
    for n, blk in enumerate(blocks):
        xl, xh, yl, yh, tang = combos[n % 32]
        exx, eyy = (xl, True, xh), (yl, True, yh)
        ex = [[bool(exx[a] and eyy[b]) for a in range(3)] for b in range(3)]
        c = [[float(blk[3 * b + a]) if ex[b][a] else float("nan") for a in range(3)] for b in range(3)]
        s0, s1, eta, lim = rr.limited_slopes(c, ex, bool(tang))
        deltasum0 += eta is None
        limited += bool(lim)
        rows.append([c[b][a] for b in range(3) for a in range(3)] + [xl, xh, yl, yh, tang])
        want_s.append([s0, s1])
        want_v.append([rr.child(c[1][1], s0, s1, p, q) for q in range(2) for p in range(2)])
    assert deltasum0 > 100 and limited > 100                 # the branches a reordering would break first are met
    got = rules("limited_slopes", rows, 2)
    assert not np.isnan(got).any()
    assert same_bits(got, want_s), mismatches(got, want_s)
    kids = []
    for (s0, s1), r in zip(got, rows):
        kids += [[r[4], s0, s1, 0.25 if p else -0.25, 0.25 if q else -0.25] for q in range(2) for p in range(2)]
    got_v = rules("child_value", kids, 1).reshape(-1, 4)
    assert same_bits(got_v, want_v), mismatches(got_v, want_v)


def test_child_value_adds_x_then_y(rules):
    x = operands(13, N, 5)
    x[:, 3:] = np.random.default_rng(14).choice([-0.4375, -0.375, -0.25, -0.125, 0.125, 0.25, 0.375], size=(x.shape[0], 2))   # offsets -1/2 + (p + 1/2) / r
    c0, s0, s1, ox, oy = x.T
    assert same_bits(rules("child_value", x, 1)[:, 0], (c0 + (s0 * ox)) + (s1 * oy))


# ------------------------------------------------------------------ FORT_AVERAGE, CoarseAverageFace
def test_avg4_is_restrict_sum4_and_avg2_the_face_average(rules):
    x = operands(15, N, 4)
    fine = np.empty((2, 2 * x.shape[0]))
    fine[0, 0::2], fine[0, 1::2], fine[1, 0::2], fine[1, 1::2] = x.T     # (0,0) (1,0) (0,1) (1,1): i fastest
    got = rules("avg4", x, 1)[:, 0]
    # restrict_sum4 divides each term by 4 before it adds, avg4 multiplies the sum by 1/4: the same bits, both scalings being exact
    assert same_bits(got, npref.restrict_sum4(fine)[0])
    a, b, c, d = x.T
    assert same_bits(got, ((((0.0 + a) + b) + c) + d) * 0.25)
    y = operands(16, N, 2)
    assert same_bits(rules("avg2", y, 1)[:, 0], ((0.0 + y[:, 0]) + y[:, 1]) / 2.0)


# ------------------------------------------------------------------ QuadCFInterp
def test_cf_tangential_and_cf_ghost(rules):
    x = operands(17, N, 4)
    kind = np.arange(x.shape[0]) % 6
    x[:, 0] = kind
    _, a, b, c = x.T
    zero = np.zeros_like(a)
    c0 = np.where(kind == 0, b, a)
    d1 = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                   [0.5 * (c - a), 0.5 * (((-3.0 * a) + (4.0 * b)) - c), b - a, 0.5 * (((3.0 * a) - (4.0 * b)) + c), a - b], zero)
    d2 = np.select([kind == 0, (kind == 1) | (kind == 3)], [(c - (2.0 * b)) + a, (a - (2.0 * b)) + c], zero)
    want = np.stack([c0, d1, d2], axis=1)
    got = rules("cf_tangential", x, 3)
    assert same_bits(got, want), mismatches(got, want)
    g = operands(18, N, 6)
    g[:, 3] = np.where(np.arange(g.shape[0]) % 2, 0.25, -0.25)
    c0, d1, d2, xt, near, far = g.T
    phistar = (c0 + (xt * d1)) + (((0.5 * xt) * xt) * d2)
    assert same_bits(rules("cf_ghost", g, 1)[:, 0], (((8.0 / 15.0) * phistar) + ((2.0 / 3.0) * near)) + (-0.2 * far))


# ------------------------------------------------------------------ PROLONG_2_NL and its coarse copy's BC
def test_prolong2_nl_and_bc_ghost(rules):
    x = operands(19, N, 5)
    p, c, cx, cy, cd = x.T
    den = 1.0 / 16.0
    assert same_bits(rules("prolong2_nl", x, 1)[:, 0], ((p + ((9.0 * den) * c)) + ((1.0 * den) * cd)) + ((3.0 * den) * (cx + cy)))
    y = operands(20, N, 4)
    y[:, 0] = np.arange(y.shape[0]) % 2
    bct, two_v, neu, near = y.T
    assert same_bits(rules("bc_ghost", y, 1)[:, 0], np.where(bct == 0, two_v - near, near + neu))


# ------------------------------------------------------------------ LevelFluxRegister
def test_reflux_plain_and_residual(rules):
    x = operands(21, N, 16)
    x[:, 13] = np.where(np.arange(x.shape[0]) % 2, 1.0, -1.0)
    tsize, bc, phihi, philo, cs, bf0, hi0, lo0, bf1, hi1, lo1, fs, acc, sign, rscale, rhs = x.T
    reg = -(tsize * (-bc * ((phihi - philo) * cs)))
    reg = reg + ((tsize * (-bf0 * ((hi0 - lo0) * fs))) * 0.5)
    reg = reg + ((tsize * (-bf1 * ((hi1 - lo1) * fs))) * 0.5)
    plain = acc + ((sign * rscale) * reg)
    want = np.stack([plain, (-1.0 * plain) + (1.0 * rhs)], axis=1)
    got = rules("reflux", x, 2)
    assert same_bits(got, want), mismatches(got, want)
