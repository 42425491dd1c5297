"""numpy twin of "COMPARE" in include/suhmo_hip.h, of the per-cell rule suhmo_amd/csrc/suhmo_compare.h and -- through tests/reduce_ref.py -- of the
order of the sums suhmo_amd/csrc/suhmo_reduce.h, written from those texts: change one, change the other.  One array statement per statement of
the rule (numpy multiplies and adds separately), so that the device is compared bit for bit.

component     FIELD: a;  DIFF: a - b, per cell on each side before anything else
block         the r x r exact cells under a level cell: each row as a pairwise tree of neighbours, (x0 + x1) + (x2 + x3), ...; the r row sums in
              ascending row order starting from the first; times 1.0 / (r r).  r = 1: the value as it is
terms         e = c - avg;  |e| w,  (e e) w,  |e|;  a covered cell contributes nothing (+0.0: no bit of a sum that started from +0.0 changes)
sums          first stage per level: level 0 under CAP_LEVEL; every box of a level of boxes under CAP_BOX on the ONE grid of the level's
              largest box extents (a box smaller than that: the cells beyond it are +0.0 terms, a workgroup without cells leaves 0.0); the lists
              of partials per level, boxes ascending; second stage: thread t adds the partials t, t + 256, ... of each list in turn, then the
              tree.  The max is exact in any order: np.max"""
import numpy as np

from tests import reduce_ref as rr

FIELD, DIFF = 0, 1


def component(kind, a, b=None):
    return a - b if kind == DIFF else a


def row_tree(x):
    """(..., r) -> (...): the pairwise tree of neighbours over the last axis (r a power of two)"""
    x = np.asarray(x, dtype=np.float64)
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def block_average(x, r):
    """(ny r, nx r) exact values -> (ny, nx): the average over the r x r block under every level cell, in the order of the rule"""
    if r == 1:
        return np.array(x, dtype=np.float64)
    ny, nx = x.shape[0] // r, x.shape[1] // r
    with np.errstate(over="ignore", invalid="ignore"):
        rows = row_tree(np.asarray(x, dtype=np.float64).reshape(ny, r, nx, r))      # (ny, r, nx): the row sums
        acc = rows[:, 0]
        for q in range(1, r):
            acc = acc + rows[:, q]
        return acc * (1.0 / (r * r))


def cell_terms(c, avg, w, cover=None):
    """-> (|e| w, (e e) w, |e|), each of c's shape; 0.0 where cover != 0"""
    with np.errstate(over="ignore", invalid="ignore"):
        e = c - avg
    if cover is not None:
        e = np.where(cover != 0, 0.0, e)
    ae = np.abs(e)
    return ae * w, (e * e) * w, ae


def second_stage_lists(lists):
    """the second stage over several lists of partials: thread t adds t, t + 256, ... of each list in turn to 0.0; then the tree"""
    acc = np.zeros(256)
    for p in lists:
        n = p.size
        q = np.zeros(-(-n // 256) * 256)
        q[:n] = p
        for step in q.reshape(-1, 256):
            acc = acc + step
    return float(rr.block_tree(acc))


def level_partials(terms, cap):
    """terms[k]: the (ny_k, nx_k) per-cell terms of box k -> the level's list of partials, boxes ascending, every box on the grid of the largest
    extents (level 0: one box, its own)"""
    my, mx = max(t.shape[0] for t in terms), max(t.shape[1] for t in terms)
    out = []
    for t in terms:
        p = np.zeros((my, mx))
        p[:t.shape[0], :t.shape[1]] = t
        out.append(rr.first_stage(p, *cap))
    return np.concatenate(out)


def covers(nx0, ny0, boxes):
    """cover[l][k]: (ny, nx) of box k of level l, 1.0 under a box of level l + 1 (boxes[l - 1]: level l's, (lo0, lo1, hi0, hi1))"""
    allb = [[(0, 0, nx0 - 1, ny0 - 1)]] + [list(bl) for bl in boxes]
    out = []
    for l, bl in enumerate(allb):
        m = np.zeros((ny0 << l, nx0 << l))
        if l + 1 < len(allb):
            for lo0, lo1, hi0, hi1 in allb[l + 1]:
                m[lo1 // 2:hi1 // 2 + 1, lo0 // 2:hi0 // 2 + 1] = 1.0
        out.append([m[b[1]:b[3] + 1, b[0]:b[2] + 1] for b in bl])
    return out


def composite(nx0, ny0, dx0, dy0, boxes, values, exact, exact_level, cover=None):
    """one component.  values[l][k]: (ny, nx) valid cells of box k of level l (level 0: the one box); exact: (ny0 << exact_level,
    nx0 << exact_level); cover: as covers() gives it (None: from the boxes) -> (norms (3,): L1, L2, max; level_terms (nlev, 3): each level's
    own sum1, sum2, max)"""
    allb = [[(0, 0, nx0 - 1, ny0 - 1)]] + [list(bl) for bl in boxes]
    cover = covers(nx0, ny0, boxes) if cover is None else cover
    lists, level_terms = [[], []], []
    mx = 0.0
    for l, bl in enumerate(allb):
        r = 1 << (exact_level - l)
        w = (dx0 / 2 ** l) * (dy0 / 2 ** l)
        t = [[], [], []]
        for k, (lo0, lo1, hi0, hi1) in enumerate(bl):
            avg = block_average(exact[lo1 * r:(hi1 + 1) * r, lo0 * r:(hi0 + 1) * r], r)
            for m, x in enumerate(cell_terms(values[l][k], avg, w, cover[l][k])):
                t[m].append(x)
        cap = rr.CAP_LEVEL if l == 0 else rr.CAP_BOX
        p = [level_partials(t[0], cap), level_partials(t[1], cap)]
        lmax = max(float(x.max()) for x in t[2])
        level_terms.append([second_stage_lists([p[0]]), second_stage_lists([p[1]]), lmax])
        lists[0].append(p[0]); lists[1].append(p[1])
        mx = max(mx, lmax)
    s1, s2 = second_stage_lists(lists[0]), second_stage_lists(lists[1])
    return np.array([s1, np.sqrt(s2), mx]), np.array(level_terms)


def finest(flat, exact, w):
    """one component of a flattened hierarchy against the exact array of the same shape -> (3,): L1, L2, max"""
    t = cell_terms(flat, exact, w)
    s = [second_stage_lists([rr.first_stage(x, *rr.CAP_LEVEL)]) for x in t[:2]]
    return np.array([s[0], np.sqrt(s[1]), float(t[2].max())])
