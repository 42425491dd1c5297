"""numpy twins of the tagSubset rules of include/suhmo_hip.h ("THE REST OF tagCells"), written from that text: restrict (levelTags &= tagSubset,
src/AmrHydro.cpp:4530-4533) on a tag map at granularity g, and the nesting of the per-level subsets (:1097-1108) as cell masks.  numpy only."""
import numpy as np


def restrict(tags, g, boxes):
    """the map after suhmo_hier_restrict_tags: entry (b, a) survives when its first cell (a g, b g) lies in one of the boxes; no boxes: unchanged"""
    out = np.array(tags, dtype=np.uint8, copy=True)
    if not boxes:
        return out
    nby, nbx = out.shape
    I, J = np.arange(nbx)[None, :] * g, np.arange(nby)[:, None] * g
    inside = np.zeros(out.shape, dtype=bool)
    for lo0, lo1, hi0, hi1 in boxes:
        inside |= (I >= lo0) & (I <= hi0) & (J >= lo1) & (J <= hi1)
    out[~inside] = 0
    return out


def aligned(g, boxes):
    return all(b[0] % g == 0 and b[1] % g == 0 and (b[2] + 1) % g == 0 and (b[3] + 1) % g == 0 for b in boxes)


def mask(nx, ny, boxes):
    m = np.zeros((ny, nx), dtype=bool)
    for lo0, lo1, hi0, hi1 in boxes:
        m[max(lo1, 0):hi1 + 1, max(lo0, 0):hi0 + 1] = True
    return m


def nest(nx0, ny0, subsets):
    """the nested subsets as cell masks of the levels (None: empty, constrains nothing)"""
    out, below = [], None
    for l, bl in enumerate(subsets):
        own = mask(nx0 << l, ny0 << l, bl) if bl else None
        if below is not None:
            crse = np.repeat(np.repeat(below, 2, axis=0), 2, axis=1)
            own = crse if own is None else own & crse
            if not own.any():
                own = None
        out.append(own)
        below = own
    return out
