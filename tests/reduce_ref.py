"""The order of the device's two-stage sums (suhmo_amd/csrc/suhmo_reduce.h), restated in numpy: change one, change the other.

first stage   workgroups of 64 x 4 threads, at most cap_x x cap_y of them.  Thread (tx, ty) of workgroup (bx, by) takes the rows
              j = by * 4 + ty, + gy * 4, ... and in each the columns i = bx * 64 + tx, + gx * 64, ... and adds its terms in that
              order to 0.0; then the block tree over the 256 threads, tid = ty * 64 + tx; partial by * gx + bx
block tree    for s = 128, 64, ..., 1: sm[tid] = sm[tid] + sm[tid + s] for tid < s
second stage  thread t adds the partials t, t + 256, ... to 0.0; then the block tree

The terms are formed before the sum (x * x, x * y in numpy: the device is built with -ffp-contract=off and rounds the product, then the
sum, the same way).  Vectorised over the 256 thread slots (and the workgroups), with a loop over the stride steps: a term the device
never visits is a +0.0 added at the end of a thread's sum, which changes no bit (no thread's sum is -0.0: it starts from +0.0)."""
import numpy as np

CAP_LEVEL = (32, 128)        # CAP_LEVEL of suhmo_reduce.h: a level, a member of an ensemble
CAP_BOX = (4, 16)            # CAP_BOX: a box of a level of boxes


def reduce_grid(nx, ny, cap_x, cap_y):
    """workgroups (gx, gy) of the first stage over nx x ny cells (reduce_grid of suhmo_reduce.h)"""
    return min((nx + 63) // 64, cap_x), min((ny + 3) // 4, cap_y)


def block_tree(sm):
    """(..., 256) values at their thread slots -> (...): what the tree leaves in slot 0"""
    sm = np.array(sm, dtype=np.float64)
    s = 128
    while s > 0:
        sm[..., :s] = sm[..., :s] + sm[..., s:2 * s]
        s >>= 1
    return sm[..., 0]


def strided_sum(lists):
    """(steps, ...) -> (...): every slot adds its elements to 0.0 in the order of the steps"""
    acc = np.zeros(lists.shape[1:])
    for step in lists:
        acc = acc + step
    return acc


def first_stage(terms, cap_x, cap_y, tree=block_tree):
    """the partials of the first stage over the (ny, nx) array of per-cell terms, in the order the device stores them"""
    ny, nx = terms.shape
    gx, gy = reduce_grid(nx, ny, cap_x, cap_y)
    sx, sy = -(-nx // (gx * 64)), -(-ny // (gy * 4))                 # stride steps of the walk
    t = np.zeros((sy * gy * 4, sx * gx * 64))
    t[:ny, :nx] = terms
    t = t.reshape(sy, gy, 4, sx, gx, 64).transpose(0, 3, 1, 4, 2, 5)   # (step in y, step in x, by, bx, ty, tx): j outer, i inner
    acc = strided_sum(t.reshape(sy * sx, gy, gx, 256))
    return tree(acc).reshape(gy * gx)


def second_stage(partials, tree=block_tree):
    n = partials.size
    p = np.zeros(-(-n // 256) * 256)
    p[:n] = partials
    return float(tree(strided_sum(p.reshape(-1, 256))))


def two_stage_sum(terms, cap_x=CAP_LEVEL[0], cap_y=CAP_LEVEL[1], tree=block_tree):
    """the sum of the (ny, nx) array of per-cell terms, bit for bit as suhmo_level_norm(., 2) ** 2 and suhmo_level_dot leave it"""
    return second_stage(first_stage(np.asarray(terms, dtype=np.float64), cap_x, cap_y, tree), tree)


def inputs(nx, ny):
    """the fields of the order tests (tests/test_reduce_order_cpu.py shows that they tell orders apart): x of both signs, y positive, both
    of magnitude 1 .. 2, so that the products cancel and every partial sum rounds"""
    rng = np.random.default_rng([nx, ny, 1])
    x = rng.uniform(1, 2, (ny, nx)) * rng.choice([-1., 1.], (ny, nx))
    y = rng.uniform(1, 2, (ny, nx))
    return x, y
