"""numpy twin of the snapshot's layout (include/suhmo_hip.h, "SNAPSHOT"): the components of every box of every level in Chombo's on-disk
order.  Written from the header's text, not from the kernel."""
import numpy as np

FIELD, FACE_TO_CELL, CONST = 0, 1, 2
X_FACES = (7, 21, 27)                                       # SUHMO_F_BX, SUHMO_F_QWX, SUHMO_F_DCX; every other face field lies on y faces


def pack(boxes_per_level, get, comps, ghost):
    """boxes_per_level[l] = [(lo0, lo1, hi0, hi1), ...] (level 0: its single box); get(l, k, field) -> what the box holds of `field`: the
    ghosted (ny + 2, nx + 2) array of a cell field, the (ny, nx + 1) / (ny + 1, nx) array of a face field, None where the box does not hold
    it; comps = [(kind, field, value)]; ghost 0 or 1.  -> (level_offset (nlev + 1,), box_offset [per level (nbox + 1,)], flat)"""
    assert ghost in (0, 1) and 1 <= len(comps) <= 16
    level_offset, box_offset, parts = [0], [], []
    for l, bl in enumerate(boxes_per_level):
        off = [0]
        for k, (lo0, lo1, hi0, hi1) in enumerate(bl):
            nx, ny = hi0 - lo0 + 1, hi1 - lo1 + 1
            fab = np.zeros((len(comps), ny + 2 * ghost, nx + 2 * ghost))
            inner = (slice(ghost, ghost + ny), slice(ghost, ghost + nx))
            for q, (kind, field, value) in enumerate(comps):
                if kind == CONST:
                    fab[q] = value
                    continue
                a = get(l, k, field)
                if a is None:
                    continue                                 # a field the box does not hold: 0.0
                if kind == FIELD:
                    assert a.shape == (ny + 2, nx + 2)
                    fab[q] = a if ghost else a[1:-1, 1:-1]
                elif field in X_FACES:
                    assert a.shape == (ny, nx + 1)
                    fab[q][inner] = 0.5 * (a[:, :-1] + a[:, 1:])
                else:
                    assert a.shape == (ny + 1, nx)
                    fab[q][inner] = 0.5 * (a[:-1, :] + a[1:, :])
            parts.append(fab.reshape(-1))
            off.append(off[-1] + fab.size)
        box_offset.append(np.array(off, dtype=np.int64))
        level_offset.append(level_offset[-1] + off[-1])
    return np.array(level_offset, dtype=np.int64), box_offset, np.concatenate(parts)


def box_of(level_offset, box_offset, flat, ncomp, ghost, l, k, box):
    a = level_offset[l] + box_offset[l][k]
    return flat[a:a + box_offset[l][k + 1] - box_offset[l][k]].reshape(ncomp, box[3] - box[1] + 1 + 2 * ghost, box[2] - box[0] + 1 + 2 * ghost)
