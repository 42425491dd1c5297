"""numpy twin of "INITIAL CONDITIONS" in include/suhmo_hip.h, written from that text: the three bodies of the four IBC kinds on a ghosted box,
and the ghost sequences of suhmo_level_ibc_init / suhmo_hier_ibc_init / suhmo_hier_ibc_reload.  The inter-level rules (PiecewiseLinearFillPatch,
the regrid's transfer) are tests/regrid_ref.py's, imported.

A box is given by geom = dict(i0, j0, nx, ny, dx, dy, nxg, nyg, periodic): its first cell in the level's index space, its size, the cell size
and the level's domain.  A state is a dict of ghosted (ny + 2, nx + 2) arrays under the names head, B, Pi, zb, mask, zs, Pw, mR.
p: dict(slope, ice_height, gap_init, rho_i, rho_w, gravity, G, L, gamma)."""
import numpy as np

from suhmo_amd import synthetic as sy
from tests import regrid_ref as rr

KINDS = ("basic", "sqrt", "valley", "dino")
DEFAULTS = dict(slope=0.0, ice_height=5000.0, gap_init=0.01, rho_i=sy.RHO_I, rho_w=sy.RHO_W, gravity=sy.GRAV, G=0.0, L=3.34e5, gamma=0.05)
NAMES = ("head", "B", "Pi", "zb", "mask", "zs", "Pw", "mR")
RELOAD_WRITES = dict(basic=("zb",), sqrt=("zb",), valley=("zb", "Pi", "zs"), dino=("Pi", "zs"))      # among zb, Pi, zs, in the order of the ghost fills
RULES = dict(zb="copy", Pi="extrap", zs="extrap", mask="copy")
# a regrid where the ORDER of reload and interpolation shows (tests/test_gpu_hier_run.py's OLD -> GEN lists on a 64 x 32 base): cell heights chosen so
# that the dino's ice margin y - x = 133333.3 m passes between the level-2 ghost cell (87, 62) of box 0 and its parent (43, 31) on level 1; B:
# the gap height loaded everywhere before the regrid; where: (level, box, row, column) of that ghost cell in the box's ghosted array
ORDER_CASE = dict(geo=(64, 32, 1000.0, 9900.0, (0, 0)), B=0.015, where=(2, 0, 31, 0),
                  old=[[(32, 16, 63, 47), (64, 16, 95, 31), (64, 32, 95, 47)], [(80, 44, 119, 83), (120, 44, 159, 83)]],
                  new=[[(40, 0, 55, 31), (40, 32, 55, 63)], [(88, 32, 103, 63), (88, 64, 103, 95)]])


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def geom(i0, j0, nx, ny, dx, dy, nxg=None, nyg=None, periodic=(0, 0)):
    return dict(i0=i0, j0=j0, nx=nx, ny=ny, dx=dx, dy=dy, nxg=nx if nxg is None else nxg, nyg=ny if nyg is None else nyg, periodic=tuple(periodic))


def positions(g):
    """X, Y of the ghosted box: a cell beyond a periodic side of the domain is its image inside"""
    gi = np.arange(g["i0"] - 1, g["i0"] + g["nx"] + 1)
    gj = np.arange(g["j0"] - 1, g["j0"] + g["ny"] + 1)
    if g["periodic"][0]:
        gi = np.where(gi < 0, gi + g["nxg"], np.where(gi >= g["nxg"], gi - g["nxg"], gi))
    if g["periodic"][1]:
        gj = np.where(gj < 0, gj + g["nyg"], np.where(gj >= g["nyg"], gj - g["nyg"], gj))
    return np.meshgrid((gi + 0.5) * g["dx"], (gj + 0.5) * g["dy"])


def _valley(p, X, Y):
    """S, zb, Pi of the valley (y already shifted by 750)"""
    P = np.power(2.0e10, 0.25)
    H6 = 100.0 * np.power(6000.0 + 200.0, 0.25) + 6000.0 / 60.0 - P + 1.0
    S = 100.0 * np.power(X + 200.0, 0.25) + X / 60.0 - P + 1.0
    gamma, gamma_b = p["gamma"], 0.05
    fx = (H6 - 6000.0 * gamma) * X * X / (6000.0 * 6000.0) + gamma * X
    fb = (H6 - 6000.0 * gamma_b) * X * X / (6000.0 * 6000.0) + gamma_b * X
    gy = 0.5e-6 * np.abs(Y * Y * Y)
    hx = (-4.5 * X / 6000.0 + 5.0) * (S - fx) / (S - fb + 1.0e-16)
    zb = fx + gy * hx
    Pi = p["rho_i"] * p["gravity"] * np.maximum(S - zb, 0.0)
    return S, zb, Pi


def _finger(X, Y, angle, x0, y0, a_max, s_gauss, sigma):
    ca, sa = np.cos(angle * 3.14159 / 180.0), np.sin(angle * 3.14159 / 180.0)
    xb, yb = X - x0, Y - y0
    xt = xb * ca + yb * sa
    yt = -xb * sa + yb * ca
    ag = a_max * np.exp(-0.5 / (s_gauss * s_gauss) * yt * yt)
    if sigma is None:
        sigma = 12000.0 - 3000.0 * np.minimum(1.0 - (50000.0 - yt) / 50000.0, 1.0)
    return ag * np.exp(-0.5 / (sigma * sigma) * xt * xt)


def _tilt(X, Y):
    return 1.5e-3 * X + -1.5e-3 * Y + 100.0


def mask_of(Pi):
    return np.where(Pi > 0.0, 1.0, -1.0)


def initial(kind, p, g):
    """initializeData + setup_iceMask on the ghosted box"""
    X, Y = positions(g)
    fact = 1.0 / (p["rho_w"] * p["gravity"])
    if kind == "basic":
        zb = p["slope"] * X
        B = np.full_like(X, p["gap_init"])
        zs = np.full_like(X, p["ice_height"])
        Pi = p["rho_i"] * p["gravity"] * zs
        Pw = Pi * 0.5
        head = Pw * fact + zb
    elif kind == "sqrt":
        zb = p["slope"] * X
        zs = np.maximum(6.0 * (np.sqrt(X + p["ice_height"]) - np.sqrt(p["ice_height"])) + 1.0, 0.0)
        Pi = np.maximum(p["rho_i"] * p["gravity"] * zs, 0.0)
        B = np.where(Pi < 2.0, 1.0e-16, p["gap_init"])
        Pw = np.full_like(X, 101325.0)
        head = Pw * fact + zb
    elif kind == "valley":
        S, zb, Pi = _valley(p, X, Y - 750.0)
        B = np.where(Pi < 1.0e-10, 1.0e-16, p["gap_init"])
        zs = np.maximum(S - zb, 0.0)
        Pw = Pi * 0.5
        head = Pw * fact + zb
        head = np.where(head < 0.0, 0.0, head)
    elif kind == "dino":
        t = _tilt(X, Y)
        zs = 2.0 * (t + 100.0)
        zb = (np.maximum(t, 0.0) + _finger(X, Y, 35.0, 100000.0, 0.0, 250.0, 50000.0, None) + _finger(X, Y, 90.0, 85000.0, 0.0, 250.0, 30000.0, 10000.0)
              + _finger(X, Y, 60.0, 55000.0, 0.0, 100.0, 20000.0, 5000.0) + _finger(X, Y, 2.0, 100000.0, 20000.0, 300.0, 35000.0, 6000.0))
        zb = np.maximum(zb, 0.0)
        Pi = p["rho_i"] * p["gravity"] * np.maximum(zs, 0.0)
        B = np.where(Pi == 0.0, 1.0e-16, p["gap_init"])
        Pw = Pi * 0.5
        head = Pw * fact + zb
        head = np.where(head < 0.0, 0.0, head)
    else:
        raise ValueError(kind)
    c = np.ascontiguousarray
    return dict(head=c(head), B=c(B), Pi=c(Pi), zb=c(zb), mask=c(mask_of(Pi)), zs=c(zs), Pw=c(Pw), mR=np.full_like(X, p["G"] / p["L"]))


def reload_body(kind, p, g, st):
    """initializeBed + initializePi: writes into the state what the kind writes there, ghost ring included"""
    X, Y = positions(g)
    if kind in ("basic", "sqrt"):
        st["zb"] = np.ascontiguousarray(p["slope"] * X)
    elif kind == "valley":
        S, zb, Pi = _valley(p, X, Y - 750.0)
        st["zs"], st["zb"], st["Pi"] = S, zb, Pi
    elif kind == "dino":
        zs = 2.0 * (_tilt(X, Y) + 100.0)
        Pi = p["rho_i"] * p["gravity"] * np.maximum(zs, 0.0)
        st["zs"], st["Pi"] = zs, Pi
        st["B"] = np.where(Pi == 0.0, 1.0e-16, st["B"])
    else:
        raise ValueError(kind)


def domain_ghosts(a, g, rule):
    """CopyGhostCells / ExtrapGhostCells of a box across the non-periodic domain sides it touches, side cells only"""
    ext = rule == "extrap"
    per = g["periodic"]
    if not per[0]:
        if g["i0"] == 0:
            a[1:-1, 0] = 2.0 * a[1:-1, 1] - a[1:-1, 2] if ext else a[1:-1, 1]
        if g["i0"] + g["nx"] == g["nxg"]:
            a[1:-1, -1] = 2.0 * a[1:-1, -2] - a[1:-1, -3] if ext else a[1:-1, -2]
    if not per[1]:
        if g["j0"] == 0:
            a[0, 1:-1] = 2.0 * a[1, 1:-1] - a[2, 1:-1] if ext else a[1, 1:-1]
        if g["j0"] + g["ny"] == g["nyg"]:
            a[-1, 1:-1] = 2.0 * a[-2, 1:-1] - a[-3, 1:-1] if ext else a[-2, 1:-1]


def level_init(kind, p, g):
    """suhmo_level_ibc_init on a whole level (or one member of an ensemble)"""
    st = initial(kind, p, g)
    domain_ghosts(st["zb"], g, "copy")
    domain_ghosts(st["mask"], g, "copy")
    return st


def box_geoms(nx0, ny0, dx0, dy0, periodic, l, boxes):
    s = 1 << l
    return [geom(lo0, lo1, hi0 - lo0 + 1, hi1 - lo1 + 1, dx0 / s, dy0 / s, nx0 * s, ny0 * s, periodic) for (lo0, lo1, hi0, hi1) in boxes]


def fill_ghosts(arrays, geoms, boxes, coarse, rule):
    """the ghost cells of a field of the boxes of level l: PiecewiseLinearFillPatch from `coarse` (the valid cells of level l - 1 on its whole
    domain, NaN where it has none), exchange with corners, then the domain-ghost rule -- steps (b), (d), (e) of the regrid's transfer"""
    g0 = geoms[0]
    nf, nc, per = (g0["nxg"], g0["nyg"]), (g0["nxg"] // 2, g0["nyg"] // 2), g0["periodic"]
    full = rr.level_array(nf[0], nf[1], boxes, arrays)
    for a, g in zip(arrays, geoms):
        for jj in range(g["ny"] + 2):
            for ii in range(g["nx"] + 2):
                if 1 <= ii <= g["nx"] and 1 <= jj <= g["ny"]:
                    continue
                w = rr._wrapped(g["i0"] + ii - 1, g["j0"] + jj - 1, nf, per)
                if w is None:
                    continue
                if not np.isnan(full[w[1], w[0]]):
                    a[jj, ii] = full[w[1], w[0]]
                else:
                    a[jj, ii] = rr.pwl_cell(coarse, w[0], w[1], nc)[0]
        domain_ghosts(a, g, rule)


def hier_init(kind, p, nx0, ny0, dx0, dy0, periodic, boxes):
    """suhmo_hier_ibc_init -> states[l][k]"""
    out = []
    for l in range(len(boxes) + 1):
        bl = [(0, 0, nx0 - 1, ny0 - 1)] if l == 0 else boxes[l - 1]
        gs = box_geoms(nx0, ny0, dx0, dy0, periodic, l, bl)
        out.append([level_init(kind, p, g) for g in gs])
    for l in range(1, len(boxes) + 1):
        bl_c = [(0, 0, nx0 - 1, ny0 - 1)] if l == 1 else boxes[l - 2]
        coarse = rr.level_array(nx0 << (l - 1), ny0 << (l - 1), bl_c, [s["mask"] for s in out[l - 1]])
        fill_ghosts([s["mask"] for s in out[l]], box_geoms(nx0, ny0, dx0, dy0, periodic, l, boxes[l - 1]), boxes[l - 1], coarse, "copy")
    return out


def hier_reload(kind, p, nx0, ny0, dx0, dy0, periodic, l, boxes_l, states_l, boxes_c, states_c):
    """suhmo_hier_ibc_reload of level l >= 1, in place on states_l; boxes_c / states_c: level l - 1 as it is now"""
    gs = box_geoms(nx0, ny0, dx0, dy0, periodic, l, boxes_l)
    nc = (nx0 << (l - 1), ny0 << (l - 1))
    for g, st in zip(gs, states_l):
        reload_body(kind, p, g, st)
    for f in RELOAD_WRITES[kind]:
        coarse = rr.level_array(nc[0], nc[1], boxes_c, [s[f] for s in states_c])
        fill_ghosts([s[f] for s in states_l], gs, boxes_l, coarse, RULES[f])
    for st in states_l:
        st["mask"] = mask_of(st["Pi"])
    coarse = rr.level_array(nc[0], nc[1], boxes_c, [s["mask"] for s in states_c])
    fill_ghosts([s["mask"] for s in states_l], gs, boxes_l, coarse, "copy")


def regrid_with_reload(kind, p, nx0, ny0, dx0, dy0, periodic, old_boxes, new_boxes, old_states, base_state, names=NAMES, reload_first=True):
    """suhmo_hier_regrid with an IBC on the handle: per new level, ascending, the transfer of every field (regrid_ref.regrid, one level at a
    time) and then the reload of that level, before the next level interpolates from it.  reload_first=False: the OTHER order -- every level
    transferred first, then reloaded -- which a test uses to show that the order matters.  -> states[l - 1][k] of the new levels"""
    out = []
    boxes_c, states_c = [(0, 0, nx0 - 1, ny0 - 1)], [base_state]
    pending = []
    for l, bl in enumerate(new_boxes, start=1):
        nc = (nx0 << (l - 1), ny0 << (l - 1))
        have_old = l <= len(old_boxes)
        states = [dict() for _ in bl]
        for f in names:
            coarse = np.pad(rr.level_array(nc[0], nc[1], boxes_c, [s[f] for s in states_c]), 1)
            new = rr.regrid(nc[0], nc[1], periodic, [old_boxes[l - 1]] if have_old else [], [bl], [[s[f] for s in old_states[l - 1]]] if have_old else [],
                            coarse, rr.RULES[f])[0]
            for st, a in zip(states, new):
                st[f] = a
        job = (l, bl, states, boxes_c, states_c)
        if reload_first:
            hier_reload(kind, p, nx0, ny0, dx0, dy0, periodic, *job)
        else:
            pending.append(job)
        out.append(states)
        boxes_c, states_c = bl, states
    for job in pending:
        hier_reload(kind, p, nx0, ny0, dx0, dy0, periodic, *job)
    return out
