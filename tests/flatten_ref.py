"""numpy twin of "FLATTEN" in include/suhmo_hip.h, written from that text: one component of a hierarchy interpolated onto the uniform grid of level
max_level.  Plain Python floats (IEEE doubles) for the slopes and the limiter, through regrid_ref.limited_slopes and regrid_ref.pwl_cell; the
r x r children of a cell in numpy, one array statement per statement of the header (numpy multiplies and adds separately), so that the
device is compared bit for bit.

flatten(nx0, ny0, periodic, boxes, values, max_level) -> (out (ny0 << max_level, nx0 << max_level), census)
    boxes[l - 1]    list of (lo0, lo1, hi0, hi1) in the index space of level l
    values[l][k]    (ny, nx) array: the component in the VALID cells of box k of level l (level 0: one box, the domain)
    census          how the coarse cells with r >= 2 were treated (CLASSES): a cell counts once per class it belongs to"""
import numpy as np

from tests import hierlayouts as hl
from tests import regrid_ref as rr

CLASSES = ("limited",        # the limiter was active: eta < 1
           "one_sided",      # a neighbour across a non-periodic domain side does not exist
           "wrap",           # a neighbour was read through a periodic wrap
           "other_box",      # a neighbour is a valid cell of another box of the level
           "edge",           # a neighbour is held by no box of the level: the linear fill from the level below (the edge clause)
           "edge_limited")   # ... and the limiter was active in that cell

# the sweep of tests/test_gpu_flatten.py: 2, 3 and 4 levels, all four periodicities; a box over the whole width; boxes 2 cells wide
CASES = [("seed-%d" % s, s) for s in range(12)] + [("span-x", "span-x"), ("tiny-boxes", "tiny-boxes")]
DATA_SEED = 11


def case(key):
    bc, boxes = hl.generate(key) if isinstance(key, int) else hl.FEATURES[key]
    return bc, [[tuple(int(v) for v in b) for b in bl] for bl in boxes]


def all_boxes(nx0, ny0, boxes):
    return [[(0, 0, nx0 - 1, ny0 - 1)]] + [list(bl) for bl in boxes]


def random_box(seed, key, l, k, q, b, kind="uniform"):
    """the ghosted (ny + 2, nx + 2) array test and twin agree on for component q of box k of level l: random valid cells, and a ghost ring of
    OTHER random values (far away from them: a ghost cell read by mistake shows)"""
    rng = np.random.default_rng([int(seed), 7717, sum(key.encode()) if isinstance(key, str) else int(key), l, k, q])
    shape = (b[3] - b[1] + 3, b[2] - b[0] + 3)
    a = np.where(rng.random(shape) < 0.3, -1.0, 1.0) if kind == "mask" else rng.uniform(-1.0, 3.0, size=shape)
    ring = rng.uniform(100.0, 200.0, size=shape)
    ring[1:-1, 1:-1] = a[1:-1, 1:-1]
    return ring


def offsets(r):
    """dx_p = -0.5 + (p + 0.5) / r, p = 0 .. r - 1"""
    return np.array([-0.5 + (p + 0.5) / r for p in range(r)])


def flatten(nx0, ny0, periodic, boxes, values, max_level):
    allb = all_boxes(nx0, ny0, boxes)
    nlev = len(allb)
    assert max_level >= nlev - 1 and len(values) == nlev
    full, owner = [], []
    for l, bl in enumerate(allb):
        f, o = np.full((ny0 << l, nx0 << l), np.nan), np.full((ny0 << l, nx0 << l), -1, dtype=np.int64)
        for k, (lo0, lo1, hi0, hi1) in enumerate(bl):
            f[lo1:hi1 + 1, lo0:hi0 + 1] = values[l][k]
            o[lo1:hi1 + 1, lo0:hi0 + 1] = k
        full.append(f); owner.append(o)
    out = np.full((ny0 << max_level, nx0 << max_level), np.nan)
    census = dict.fromkeys(CLASSES, 0)
    for l, bl in enumerate(allb):                             # ascending: a finer level overwrites
        r = 1 << (max_level - l)
        n = (nx0 << l, ny0 << l)
        if r == 1:                                            # a copy
            for lo0, lo1, hi0, hi1 in bl:
                out[lo1:hi1 + 1, lo0:hi0 + 1] = full[l][lo1:hi1 + 1, lo0:hi0 + 1]
            continue
        d = offsets(r)
        fills = {}                                            # the edge clause's values, each computed once
        for k, (lo0, lo1, hi0, hi1) in enumerate(bl):
            for J in range(lo1, hi1 + 1):
                for I in range(lo0, hi0 + 1):
                    c = [[0.0] * 3 for _ in range(3)]
                    ex = [[False] * 3 for _ in range(3)]
                    seen = set()
                    for b in range(3):
                        for a in range(3):
                            i, j = I + a - 1, J + b - 1
                            w = rr._wrapped(i, j, n, periodic)
                            if w is None:                     # across a non-periodic domain side: does not exist
                                seen.add("one_sided")
                                continue
                            ex[b][a] = True
                            if (w[0], w[1]) != (i, j):
                                seen.add("wrap")
                            x = full[l][w[1], w[0]]
                            if not np.isnan(x):               # a valid cell of the level, in whichever box
                                if owner[l][w[1], w[0]] != k:
                                    seen.add("other_box")
                                c[b][a] = float(x)
                                continue
                            seen.add("edge")                  # held by no box of the level: PiecewiseLinearFillPatch from level l - 1
                            if (w[0], w[1]) not in fills:
                                fills[(w[0], w[1])] = rr.pwl_cell(full[l - 1], w[0], w[1], (n[0] // 2, n[1] // 2))[0]
                            c[b][a] = fills[(w[0], w[1])]
                    s0, s1, eta, limited = rr.limited_slopes(c, ex, True)
                    if limited:
                        seen.add("limited")
                        if "edge" in seen:
                            seen.add("edge_limited")
                    for nm in seen:
                        census[nm] += 1
                    v = c[1][1] + s0 * d                      # v = c0; v = v + s0 * dx_p
                    out[r * J:r * J + r, r * I:r * I + r] = v[None, :] + (s1 * d)[:, None]      # v = v + s1 * dy_q
    return out, census
