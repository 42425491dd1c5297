"""numpy twin of the grid generation of include/suhmo_hip.h ("GRID GENERATION"): the tagging of suhmo_hier_tag_cells / suhmo_level_tag_cells and
the Berger-Rigoutsos clustering of suhmo_grids_generate.  Written from the rules as the header states them, not from the C++; the tests
(tests/test_gridgen_cpu.py, tests/test_gpu_tags.py) compare the library with it entry by entry and box by box, order included.  numpy only."""
import numpy as np


# ---------------------------------------------------------------- tagging
def tag_map(nx, ny, pieces, vmin, vmax, grow=0, grow_dir=(0, 0), g=1, into=None):
    """tag map of a level of nx x ny cells at granularity g.  pieces: (lo0, lo1, values) with values the VALID cells of a box, [j][i], whose
    lower corner is cell (lo0, lo1) of the level.  vmin < value < vmax, both strict (NaN: no); the tag reaches max(grow, grow_dir[d]) cells in
    direction d, clipped to the level's box (no periodic wrap); into: a map to accumulate into (the union of several calls)"""
    nbx, nby = -(-nx // g), -(-ny // g)
    m = np.zeros((nby, nbx), dtype=np.uint8) if into is None else into.copy()
    rx, ry = max(grow, grow_dir[0]), max(grow, grow_dir[1])
    for lo0, lo1, v in pieces:
        with np.errstate(invalid="ignore"):
            hit = (vmin < v) & (v < vmax)
        for j, i in zip(*np.nonzero(hit)):
            I, J = lo0 + int(i), lo1 + int(j)
            a0, a1 = max(I - rx, 0) // g, min(I + rx, nx - 1) // g
            b0, b1 = max(J - ry, 0) // g, min(J + ry, ny - 1) // g
            m[b0:b1 + 1, a0:a1 + 1] = 1
    return m


# ---------------------------------------------------------------- clustering
def _nearest_hole(S):
    """index of the zero of S nearest the centre of its range (a tie: the lower index); None without one"""
    n, best = len(S), None
    for k in range(n):
        if S[k] == 0:
            d = abs(2 * k - (n - 1))
            if best is None or d < best[0]:
                best = (d, k)
    return None if best is None else best[1]


def _best_inflection(S):
    """(strength, k): the cut between k and k + 1 with the largest |D[k] - D[k+1]| among those where the second difference D changes sign;
    ties: nearest the centre, then the lower index; None without one"""
    n, best = len(S), None
    D = {k: int(S[k - 1]) - 2 * int(S[k]) + int(S[k + 1]) for k in range(1, n - 1)}
    for k in range(1, n - 2):
        if D[k] * D[k + 1] < 0:
            key = (-abs(D[k] - D[k + 1]), abs(2 * k + 1 - (n - 1)), k)
            if best is None or key < best:
                best = key
    return None if best is None else (-best[0], best[2])


def cluster(T, fill_ratio, max_blocks):
    """make(R) on the whole of the block map T ([J][I], nonzero = tagged) -> rectangles (I0, J0, I1, J1) in emission order"""
    T = np.asarray(T) != 0
    out = []

    def make(i0, j0, i1, j1):
        sub = T[j0:j1 + 1, i0:i1 + 1]
        if not sub.any():
            return
        js, is_ = np.nonzero(sub)
        i0, i1, j0, j1 = i0 + int(is_.min()), i0 + int(is_.max()), j0 + int(js.min()), j0 + int(js.max())
        sub = T[j0:j1 + 1, i0:i1 + 1]
        w, h = i1 - i0 + 1, j1 - j0 + 1
        if int(sub.sum()) / (w * h) >= fill_ratio and w <= max_blocks and h <= max_blocks:
            out.append((i0, j0, i1, j1))
            return
        Sx, Sy = sub.sum(axis=0), sub.sum(axis=1)
        order = (0, 1) if w >= h else (1, 0)                  # the longer side first, a tie goes to x
        S = (Sx, Sy)
        split = None                                          # (direction, last index of the lower part, first of the upper), offsets
        for d in order:                                       # (a) hole
            k = _nearest_hole(S[d])
            if k is not None:
                split = (d, k - 1, k + 1)
                break
        if split is None:                                     # (b) inflection
            cand = []
            for rank, d in enumerate(order):
                r = _best_inflection(S[d])
                if r is not None:
                    cand.append((-r[0], rank, d, r[1]))
            if cand:
                _, _, d, k = min(cand)
                split = (d, k, k + 1)
        if split is None:                                     # (c) bisect the longer side
            d = order[0]
            half = (w if d == 0 else h) // 2
            split = (d, half - 1, half)
        d, a, b = split
        if d == 0:
            make(i0, j0, i0 + a, j1); make(i0 + b, j0, i1, j1)
        else:
            make(i0, j0, i1, j0 + a); make(i0, j0 + b, i1, j1)

    make(0, 0, T.shape[1] - 1, T.shape[0] - 1)
    return out


def nesting_tags(box, n_mid, periodic, g, nest):
    """entries (I, J) of the level two below `box` touched by coarsen(grow(coarsen(box), nest)); n_mid = (nx, ny) of the level in between, in
    whose cells the margin is counted: a cell beyond a periodic side wraps, one beyond a non-periodic side is dropped"""
    lo0, lo1, hi0, hi1 = box
    axes = []
    for d, (lo, hi) in enumerate(((lo0, hi0), (lo1, hi1))):
        e = set()
        for c in range(lo // 2 - nest, hi // 2 + nest + 1):
            if not 0 <= c < n_mid[d]:
                if not periodic[d]:
                    continue
                c %= n_mid[d]
            e.add((c // 2) // g)
        axes.append(sorted(e))
    return [(I, J) for J in axes[1] for I in axes[0]]


def generate(nx0, ny0, periodic, tags, fill_ratio, block_factor, max_box_size, nesting_radius=2):
    """the twin of suhmo_grids_generate: boxes[l - 1] = list of (lo0, lo1, hi0, hi1) of level l"""
    b = block_factor
    g, nest = b // 2, max(nesting_radius, 2)
    top = 0
    while top < len(tags) and np.asarray(tags[top]).any():    # levels above the first level without tags are dropped
        top += 1
    lev = {}
    for l in range(top - 1, -1, -1):
        T = (np.asarray(tags[l]) != 0).copy()
        assert T.shape == ((ny0 << l) // g, (nx0 << l) // g)
        for box in lev.get(l + 2, []):
            for I, J in nesting_tags(box, (nx0 << (l + 1), ny0 << (l + 1)), periodic, g, nest):
                T[J, I] = True
        lev[l + 1] = [(I0 * b, J0 * b, (I1 + 1) * b - 1, (J1 + 1) * b - 1) for I0, J0, I1, J1 in cluster(T, fill_ratio, max_box_size // b)]
    return [lev[l] for l in range(1, top + 1)]
