"""numpy twin of "MASS BALANCE" in include/suhmo_hip.h, of the per-face and per-cell rule suhmo_amd/csrc/suhmo_balance.h and -- through
tests/reduce_ref.py -- of the order of the sums suhmo_amd/csrc/suhmo_reduce.h, written from those texts: change one, change the other.  One array
statement per statement of the rule (numpy multiplies, divides and adds separately), so that the device is compared bit for bit.

a box          head_g, mask_g: ghosted (ny + 2, nx + 2) as the canvases hold them; B: the valid cells; bx (ny, nx + 1), by (ny + 1, nx): the face
               coefficients; box = (lo0, lo1, hi0, hi1) in the cells of its level, domain = (nxg, nyg)
head beside    the neighbour inside the box; on a side the STORED ghost where the device reads it (a box or coarse-fine side; a periodic side of
a face         a box that does not span the domain), the wrap on a periodic side of a box that does, else mixBCValues: 2 value - near (Dirichlet),
               near + (sign d) value (Neumann) -- phiW / phiE / phiS / phiN of suhmo_common.h with homog = false
face           gradphi = (phihi - philo) * (-1.0) / h;  flux = -K * gradphi;  t = flux * area;  mec, up, down as mb_face has them
fold           per cell, in this order: low x-face, high x-face (last column), low y-face, high y-face (last row), the volume term; a term that
               is not there is +0.0 (no bit of a sum that started from +0.0 changes: such a sum is never -0.0)
sums           first stage per level: CAP_LEVEL for a level, CAP_BOX on the level's largest box extents for a level of boxes (a box smaller than
               that: +0.0 terms, a workgroup without cells leaves 0.0), boxes ascending; second stage per level: rr.second_stage"""
from collections import Counter

import numpy as np

from tests import ghostring as gr
from tests import reduce_ref as rr

NAMES = ("lo_x", "hi_x", "lo_y", "hi_y", "dir_x", "dir_y", "volume")
LO_X, HI_X, LO_Y, HI_Y, DIR_X, DIR_Y, VOLUME = range(7)


def side_modes(box, domain, periodic):
    """how the device finds the head across each side of a box: {(d, s): "stored" | "wrap" | "bc"} (make_dv of suhmo_level.hip: cfx / ext)"""
    lo0, lo1, hi0, hi1 = box
    nx, ny = hi0 - lo0 + 1, hi1 - lo1 + 1
    nxg, nyg = domain
    whole_y = lo1 == 0 and ny == nyg
    stored = {(0, 0): lo0 > 0 or (periodic[0] and nx < nxg), (0, 1): hi0 + 1 < nxg or (periodic[0] and nx < nxg),
              (1, 0): (not whole_y) and (lo1 > 0 or bool(periodic[1])), (1, 1): (not whole_y) and (hi1 + 1 < nyg or bool(periodic[1]))}
    return {k: "stored" if v else ("wrap" if periodic[k[0]] else "bc") for k, v in stored.items()}


def effective_head(head_g, box, domain, bc, dx, dy):
    """the ghosted head with the four sides as the device reads them (corners are never read)"""
    h = np.array(head_g, dtype=np.float64)
    v = h[1:-1, 1:-1]
    d = (dx, dy)
    for (dr, s), mode in side_modes(box, domain, bc["periodic"]).items():
        if mode == "stored":
            continue
        if dr == 0:
            near, wrap = (v[:, 0], v[:, -1]) if s == 0 else (v[:, -1], v[:, 0])
        else:
            near, wrap = (v[0, :], v[-1, :]) if s == 0 else (v[-1, :], v[0, :])
        if mode == "wrap":
            val = wrap
        elif bc["type"][dr][s] == 0:
            val = 2.0 * bc["value"][dr][s] - near
        else:
            val = near + ((-1.0 if s == 0 else 1.0) * d[dr]) * bc["value"][dr][s]
        if dr == 0:
            h[1:-1, 0 if s == 0 else -1] = val
        else:
            h[0 if s == 0 else -1, 1:-1] = val
    return h


def face_terms(phihi, philo, K, mhi, mlo, h, area, at_lo, at_hi):
    """mb_face over arrays -> (what it adds to lo, to hi, to dir), each of the faces' shape"""
    with np.errstate(over="ignore", invalid="ignore"):
        gradphi = (phihi - philo) * (-1.0) / h
        flux = -K * gradphi
        t = flux * area
        d = mhi - mlo
        mec = np.where(np.abs(d) < 1e-10, np.where(mhi > 0.0, 1.0, -1.0), 0.0)
    mec = np.where(at_lo | at_hi, 0.0, mec)
    on = np.abs(mec) < 1.0e-10
    pos = d > 0.0
    neg = ~pos & (d < 0.0)
    edge = ~pos & ~neg & (mhi > 0.0)
    up = on & (pos | (edge & at_lo))
    down = on & (neg | (edge & ~at_lo & at_hi))
    zero = np.zeros_like(t)
    return np.where(at_lo, t, zero), np.where(~at_lo & at_hi, t, zero), np.where(up, t, np.where(down, -t, zero))


def box_terms(head_g, mask_g, B, bx, by, box, domain, bc, dx, dy):
    """-> seq[q]: the (ny, nx) arrays the thread of a cell adds to value q, in the order it adds them"""
    lo0, lo1, hi0, hi1 = box
    nx, ny = hi0 - lo0 + 1, hi1 - lo1 + 1
    assert head_g.shape == mask_g.shape == (ny + 2, nx + 2) and B.shape == (ny, nx) and bx.shape == (ny, nx + 1) and by.shape == (ny + 1, nx)
    h = effective_head(head_g, box, domain, bc, dx, dy)
    m = np.asarray(mask_g, dtype=np.float64)
    seq = [[] for _ in NAMES]
    # x-faces 0 .. nx of every row: face i between cell i - 1 and cell i
    I = lo0 + np.arange(nx + 1)[None, :] + np.zeros((ny, 1), dtype=np.int64)
    lo, hi, dr = face_terms(h[1:-1, 1:], h[1:-1, :-1], bx, m[1:-1, 1:], m[1:-1, :-1], dx, dy, I == 0, I == domain[0])
    last = np.zeros((ny, nx))
    for q, a in ((LO_X, lo), (HI_X, hi), (DIR_X, dr)):
        high = last.copy()
        high[:, -1] = a[:, nx]
        seq[q] += [a[:, :nx], high]
    J = lo1 + np.arange(ny + 1)[:, None] + np.zeros((1, nx), dtype=np.int64)
    lo, hi, dr = face_terms(h[1:, 1:-1], h[:-1, 1:-1], by, m[1:, 1:-1], m[:-1, 1:-1], dy, dx, J == 0, J == domain[1])
    for q, a in ((LO_Y, lo), (HI_Y, hi), (DIR_Y, dr)):
        high = last.copy()
        high[-1, :] = a[ny, :]
        seq[q] += [a[:ny, :], high]
    with np.errstate(over="ignore", invalid="ignore"):
        seq[VOLUME] = [np.where(m[1:-1, 1:-1] > 0.0, B * dx * dy, 0.0)]
    return seq


def first_stage_seq(seq, grid_shape, cap):
    """the partials of one value over one box: seq = the arrays a cell's thread adds in turn, on the grid of an (ny, nx) = grid_shape level"""
    my, mx = grid_shape
    gx, gy = rr.reduce_grid(mx, my, *cap)
    sx, sy = -(-mx // (gx * 64)), -(-my // (gy * 4))
    steps = []
    for a in seq:
        t = np.zeros((sy * gy * 4, sx * gx * 64))
        t[:a.shape[0], :a.shape[1]] = a
        steps.append(t.reshape(sy, gy, 4, sx, gx, 64).transpose(0, 3, 1, 4, 2, 5).reshape(sy * sx, gy, gx, 256))
    walk = np.stack(steps, axis=1).reshape(sy * sx * len(seq), gy, gx, 256)      # j outer, i inner, within a cell the terms in their order
    return rr.block_tree(rr.strided_sum(walk)).reshape(gy * gx)


def level_balance(boxes_seq, cap):
    """boxes_seq[k]: box_terms of box k of the level -> (7,): the level's seven values"""
    my = max(s[VOLUME][0].shape[0] for s in boxes_seq)
    mx = max(s[VOLUME][0].shape[1] for s in boxes_seq)
    return np.array([rr.second_stage(np.concatenate([first_stage_seq(s[q], (my, mx), cap) for s in boxes_seq])) for q in range(len(NAMES))])


def level_terms(boxes_seq):
    """the terms of every value in the order of a serial walk (boxes, rows, columns, the cell's own order): for math.fsum and the bound"""
    out = []
    for q in range(len(NAMES)):
        out.append(np.concatenate([np.stack(s[q], axis=-1).reshape(-1) for s in boxes_seq]))
    return out


def balance_of_level(data, boxes, domain, bc, dx, dy, cap=None):
    """data[k] = dict(head=, mask= ghosted; B= valid or ghosted; bx=, by=) of box k -> (7,)"""
    cap = cap if cap is not None else (rr.CAP_LEVEL if len(boxes) == 1 and tuple(boxes[0]) == (0, 0, domain[0] - 1, domain[1] - 1) else rr.CAP_BOX)
    return level_balance([terms_of(d, b, domain, bc, dx, dy) for d, b in zip(data, boxes)], cap)


def terms_of(d, box, domain, bc, dx, dy):
    ny, nx = box[3] - box[1] + 1, box[2] - box[0] + 1
    B = d["B"] if d["B"].shape == (ny, nx) else d["B"][1:-1, 1:-1]
    return box_terms(d["head"], d["mask"], B, d["bx"], d["by"], box, domain, bc, dx, dy)


# ------------------------------------------------------------------ the census: which kinds of face an input holds
CLASSES = tuple(["margin_lower_x", "margin_upper_x", "margin_lower_y", "margin_upper_y"]
                + ["%s_%s" % (kind, side) for side in ("lo_x", "hi_x", "lo_y", "hi_y") for kind in ("ice_bearing", "ice_free")]
                + ["shared_margin", "periodic_side", "coarse_fine_side"])


def census(masks_g, boxes, domain, periodic):
    """faces per class over the boxes of ONE level (masks_g[k]: the ghosted mask of box k as stored):
    margin_lower / margin_upper_<d>   a face inside the domain with mhi - mlo > 0 / < 0
    ice_bearing / ice_free_<side>     a domain face with mhi == mlo and mhi > 0 / not
    shared_margin                     a margin face on a side two boxes share (each of them counts it)
    periodic_side                     a domain face on a periodic side
    coarse_fine_side                  a face on a box side inside the domain behind which no box of the level lies"""
    c = Counter({k: 0 for k in CLASSES})
    for m, box in zip(masks_g, boxes):
        lo0, lo1, hi0, hi1 = box
        nx, ny = hi0 - lo0 + 1, hi1 - lo1 + 1
        for d, n, ng, lo in ((0, nx, domain[0], lo0), (1, ny, domain[1], lo1)):
            for f in range(n + 1):
                G = lo + f
                if d == 0:
                    mhi, mlo = m[1:-1, f + 1], m[1:-1, f]
                    cells = [((G if f == n else G - 1), lo1 + t) for t in range(ny)]     # the cell outside the box where the face is on a side
                else:
                    mhi, mlo = m[f + 1, 1:-1], m[f, 1:-1]
                    cells = [(lo0 + t, (G if f == n else G - 1)) for t in range(nx)]
                dd = mhi - mlo
                nm = "xy"[d]
                if G == 0 or G == ng:
                    side = ("lo_" if G == 0 else "hi_") + nm
                    c["ice_bearing_" + side] += int(((dd == 0) & (mhi > 0)).sum())
                    c["ice_free_" + side] += int(((dd == 0) & ~(mhi > 0)).sum())
                    if periodic[d]:
                        c["periodic_side"] += dd.size
                    continue
                c["margin_lower_" + nm] += int((dd > 0).sum())
                c["margin_upper_" + nm] += int((dd < 0).sum())
                if f == 0 or f == n:
                    kinds = np.array([gr.cell_kind(i, j, domain, periodic, boxes) for i, j in cells])
                    c["shared_margin"] += int(((dd != 0) & (kinds == "fine-fine")).sum())
                    c["coarse_fine_side"] += int((kinds == "coarse-fine").sum())
    return c


# ------------------------------------------------------------------ the inputs of the sweeps (tests/test_massbalance_cpu.py, tests/test_gpu_massbalance.py)
SINGLE_SHAPES = ((70, 9), (64, 4), (16, 516), (2052, 4))
DIRICHLET_BC = dict(type=[[0, 0], [1, 1]], value=[[2.0, 900.0], [0.0, 0.0]], periodic=[0, 0])
NEUMANN_BC = dict(type=[[0, 1], [1, 1]], value=[[0.0, 0.0], [0.0, 0.0]], periodic=[0, 0])        # SHMIP's: Dirichlet on x-lo, Neumann elsewhere
MIXED_BC = dict(type=[[1, 0], [0, 1]], value=[[0.02, 40.0], [3.0, -0.01]], periodic=[0, 0])       # values that are not 0 on all four sides
X_PERIODIC_BC = dict(type=[[1, 1], [0, 1]], value=[[0.0, 0.0], [0.0, 0.0]], periodic=[1, 0])
SINGLE_BCS = (("dirichlet", DIRICHLET_BC), ("neumann", NEUMANN_BC), ("mixed", MIXED_BC), ("x-periodic", X_PERIODIC_BC))
HIER_KEYS = (0, 1, 2, 3, "span-x", "tiny-boxes")


def level_mask(nx, ny, periodic, seed):
    """an ice mask of +-1 over a level's whole ghosted domain, (ny + 2, nx + 2): patches of about three cells, a third of them ice-free, the
    ghost cells across a periodic side the periodic image; every box of the level is cut from it, so that two boxes agree on a shared face"""
    rng = np.random.default_rng([int(seed), 6151, nx, ny])
    coarse = np.where(rng.random(((ny + 2) // 3 + 1, (nx + 2) // 3 + 1)) < 0.33, -1.0, 1.0)
    m = np.ascontiguousarray(np.kron(coarse, np.ones((3, 3)))[:ny + 2, :nx + 2])
    if periodic[1]:
        m[0, :], m[-1, :] = m[-2, :].copy(), m[1, :].copy()
    if periodic[0]:
        m[:, 0], m[:, -1] = m[:, -2].copy(), m[:, 1].copy()
    return m


def cut(a, box):
    """the ghosted array of a box out of the ghosted array of its level"""
    lo0, lo1, hi0, hi1 = box
    return np.ascontiguousarray(a[lo1:hi1 + 3, lo0:hi0 + 3])


WALK_EDGE_LAYOUT = (160, 48, [[(0, 0, 7, 67), (16, 80, 275, 83)]])      # boxes of 8 x 68 and 260 x 4: the first extents beyond CAP_BOX in y and in x


def valley_mask(nx, ny):
    """the ghosted ice mask of synthetic.valley_initial_state (SHMIP E1's bed): an oblique margin"""
    from suhmo_amd import synthetic as sy
    return sy.valley_initial_state(nx, ny, 0.05)["mask"]


def sweep_layouts():
    """the inputs of the sweeps as far as the census needs them: (name, nx0, ny0, bc, boxes, masks) with masks[l] the ghosted mask of level l's
    whole domain -- the single levels with the valley's mask under every BC set, the hierarchies with level_mask"""
    from tests import flatten_ref as fr
    from tests import hierlayouts as hl
    for nx, ny in SINGLE_SHAPES:
        for nm, bc in SINGLE_BCS:
            yield "%dx%d-%s" % (nx, ny, nm), nx, ny, bc, [], [valley_mask(nx, ny)]
    for key in HIER_KEYS:
        bc, boxes = fr.case(key)
        yield "hier-%s" % key, hl.NX0, hl.NY0, bc, boxes, [level_mask(hl.NX0 << l, hl.NY0 << l, bc["periodic"], 7) for l in range(len(boxes) + 1)]
    nx0, ny0, boxes = WALK_EDGE_LAYOUT
    yield "walk-edges", nx0, ny0, hl._NP, boxes, [level_mask(nx0 << l, ny0 << l, (0, 0), 8) for l in range(2)]


def synthetic_level(nx, ny, periodic, seed):
    """random fields over a level's whole domain for the tests that need no device: head and B ghosted (the ghosts across a periodic side the
    periodic image, as an exchange leaves them), bx (ny, nx + 1), by (ny + 1, nx); every value a multiple of 2^-20 of magnitude 1 .. 4"""
    rng = np.random.default_rng([int(seed), 911, nx, ny])
    q = lambda shape: np.round(rng.uniform(1.0, 4.0, size=shape) * 2.0 ** 20) / 2.0 ** 20
    head, B = q((ny + 2, nx + 2)) * rng.choice([-1.0, 1.0], (ny + 2, nx + 2)), q((ny + 2, nx + 2))
    for a in (head, B):
        if periodic[1]:
            a[0, :], a[-1, :] = a[-2, :].copy(), a[1, :].copy()
        if periodic[0]:
            a[:, 0], a[:, -1] = a[:, -2].copy(), a[:, 1].copy()
    return dict(head=head, B=B, bx=q((ny, nx + 1)), by=q((ny + 1, nx)))


def cut_data(level, mask_g, box):
    """the data of a box (as balance_of_level takes them) out of synthetic_level's arrays and the level's ghosted mask"""
    lo0, lo1, hi0, hi1 = box
    return dict(head=cut(level["head"], box), B=cut(level["B"], box), mask=cut(mask_g, box),
                bx=np.ascontiguousarray(level["bx"][lo1:hi1 + 1, lo0:hi0 + 2]), by=np.ascontiguousarray(level["by"][lo1:hi1 + 2, lo0:hi0 + 1]))
