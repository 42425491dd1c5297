"""The numpy twin of the device's two-stage sums (tests/reduce_ref.py) against a plain loop that follows the kernel text of
suhmo_amd/csrc/suhmo_reduce.h thread by thread, and the inputs of tests/test_gpu_reductions.py against wrong orders: a sum in another
order must give other bits on them, or the GPU test could not tell that the order changed."""
import numpy as np
import pytest

from tests import reduce_ref as rr

SMALL = [(63, 3), (64, 4), (65, 5), (130, 9)]            # several terms per sum, one or a few workgroups
LARGE = [(2050, 36), (66, 516)]                          # the walk wraps in x / in y; 288 / 256 partials


def tree_by_the_text(sm):
    sm = [float(v) for v in sm]
    s = 128
    while s > 0:
        for tid in range(s):
            sm[tid] = sm[tid] + sm[tid + s]
        s >>= 1
    return sm[0]


def sum_by_the_text(terms, cap_x, cap_y):
    """for_valid_cells, block_tree and k_norm_final as written, one thread after the other"""
    ny, nx = terms.shape
    gx, gy = rr.reduce_grid(nx, ny, cap_x, cap_y)
    partial = [0.0] * (gx * gy)
    for by in range(gy):
        for bx in range(gx):
            sm = [0.0] * 256
            for ty in range(4):
                for tx in range(64):
                    acc = 0.0
                    for j in range(by * 4 + ty, ny, gy * 4):
                        for i in range(bx * 64 + tx, nx, gx * 64):
                            acc += float(terms[j, i])
                    sm[ty * 64 + tx] = acc
            partial[by * gx + bx] = tree_by_the_text(sm)
    sm = [0.0] * 256
    for tid in range(256):
        acc = 0.0
        for k in range(tid, len(partial), 256):
            acc = acc + partial[k]
        sm[tid] = acc
    return tree_by_the_text(sm)


@pytest.mark.parametrize("nx,ny,cap", [(1, 1, rr.CAP_LEVEL), (65, 5, rr.CAP_LEVEL), (130, 9, rr.CAP_LEVEL),
                                       (130, 9, (1, 1)), (300, 70, rr.CAP_BOX)])
def test_twin_follows_the_kernel_text(nx, ny, cap):
    """(130 x 9 under a cap of 1 x 1 and 300 x 70 under the box cap: the walk wraps in both directions inside one thread)"""
    x, y = rr.inputs(nx, ny)
    for terms in (x * x, x * y):
        assert rr.two_stage_sum(terms, *cap) == sum_by_the_text(terms, *cap)


def test_tree_follows_the_kernel_text():
    v = np.random.default_rng(7).uniform(-1, 1, (3, 256))
    assert [float(t) for t in rr.block_tree(v)] == [tree_by_the_text(r) for r in v]


def adjacent_pair_tree(sm):
    sm = np.array(sm, dtype=np.float64)
    while sm.shape[-1] > 1:
        sm = sm[..., 0::2] + sm[..., 1::2]
    return sm[..., 0]


WRONG = {
    "adjacent-pair tree": lambda t: rr.two_stage_sum(t, tree=adjacent_pair_tree),
    "grid caps 16 x 64": lambda t: rr.two_stage_sum(t, 16, 64),
    "transposed walk": lambda t: rr.two_stage_sum(t.T),
    "np.sum": lambda t: float(np.sum(t)),
}


def differing(nx, ny):
    x, y = rr.inputs(nx, ny)
    right = rr.two_stage_sum(x * y)
    return [name for name, f in WRONG.items() if f(x * y) != right]


@pytest.mark.parametrize("nx,ny", LARGE)
def test_every_wrong_order_shows_in_the_dot_product_of_the_large_shapes(nx, ny):
    assert differing(nx, ny) == list(WRONG)


@pytest.mark.parametrize("nx,ny", SMALL)
def test_a_wrong_order_shows_in_the_dot_product_of_every_small_shape(nx, ny):
    assert differing(nx, ny)
