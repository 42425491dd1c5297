"""numpy twin of "REGRID: FIELD TRANSFER" in include/suhmo_hip.h, written from that text: a hierarchy's field moved onto new box lists.
Plain Python floats (IEEE doubles), one statement per operation of the header, so that the device is compared bit for bit.

regrid(nx0, ny0, periodic, old_boxes, new_boxes, old_fields, base_field, rule) -> new ghosted per-box arrays
    old_boxes / new_boxes   boxes[l - 1] = list of (lo0, lo1, hi0, hi1) in the index space of level l
    old_fields[l - 1][k]    ghosted (ny + 2, nx + 2) array of old box k of level l (only its valid cells are read)
    base_field              ghosted (ny0 + 2, nx0 + 2) array of level 0 (only its valid cells are read)
    rule                    step (e): "copy" (CopyGhostCells), "extrap" (ExtrapGhostCells) or None (left alone); RULES maps field names
A ghost cell nobody writes holds 0, as in a freshly created box."""
import numpy as np

RULES = dict(head=None, B="copy", Pi="extrap", zb="copy", mask="copy", mR="extrap", Pw="extrap", zs="extrap")


def limited_slopes(c, ex, tangential_only):
    """c[b][a], ex[b][a]: the 3 x 3 block around the coarse cell (b: y, a: x; [1][1] the cell) and which of its cells exist.
    -> (s0, s1, eta or None, limited) with the slopes after the limiter.  tangential_only: the FineInterp rule (a); False:
    PiecewiseLinearFillPatch as or_pwl_fill states it (both slopes always)"""
    c0 = c[1][1]
    xl, xh, yl, yh = ex[1][0], ex[1][2], ex[0][1], ex[2][1]
    s0 = s1 = 0.0
    if xl and xh:
        s0 = 0.5 * (c[1][2] - c[1][0])
    elif xh:
        s0 = c[1][2] - c0
    elif xl:
        s0 = c0 - c[1][0]
    if yl and yh:
        s1 = 0.5 * (c[2][1] - c[0][1])
    elif yh:
        s1 = c[2][1] - c0
    elif yl:
        s1 = c0 - c[0][1]
    smax = smin = c0
    for b in range(3):
        for a in range(3):
            if ex[b][a]:
                smax = max(smax, c[b][a])
                smin = min(smin, c[b][a])
    deltasum = 0.5 * (abs(s0) + abs(s1))
    eta, limited = None, False
    if deltasum > 0.0:
        etamax = (smax - c0) / deltasum
        etamin = (c0 - smin) / deltasum
        eta = max(min(min(etamin, etamax), 1.0), 0.0)
        limited = eta < 1.0
        if not tangential_only or (xl and xh):
            s0 = eta * s0
        if not tangential_only or (yl and yh):
            s1 = eta * s1
    return s0, s1, eta, limited


def child(c0, s0, s1, p, q):
    v = c0
    v = v + s0 * (0.25 if p else -0.25)
    v = v + s1 * (0.25 if q else -0.25)
    return v


def _block(cf, I, J, n, periodic, wrap):
    """the 3 x 3 block around (I, J) of the full-domain array cf (n = (nx, ny)) and which cells exist; wrap: through periodic sides"""
    c = [[0.0] * 3 for _ in range(3)]
    ex = [[False] * 3 for _ in range(3)]
    for b in range(3):
        for a in range(3):
            i, j = I + a - 1, J + b - 1
            ok = True
            for d, (x, m) in enumerate(((i, n[0]), (j, n[1]))):
                if not 0 <= x < m:
                    ok = ok and bool(wrap and periodic[d])
            if ok:
                ex[b][a] = True
                c[b][a] = float(cf[j % n[1], i % n[0]])
    return c, ex


def interp_cell(cf, I, J, n, periodic):
    """the four children of coarse cell (I, J) by rule (a): [[v(p=0,q=0), v(1,0)], [v(0,1), v(1,1)]] (rows q), and the limiter's eta"""
    c, ex = _block(cf, I, J, n, periodic, True)
    s0, s1, eta, _ = limited_slopes(c, ex, True)
    return [[child(c[1][1], s0, s1, p, q) for p in range(2)] for q in range(2)], eta


def pwl_cell(cf, gi, gj, n):
    """fine cell (gi, gj) by PiecewiseLinearFillPatch from the full-domain coarse array cf (rule (b)); also (value, limited?)"""
    c, ex = _block(cf, gi >> 1, gj >> 1, n, (0, 0), False)
    s0, s1, _, lim = limited_slopes(c, ex, False)
    return child(c[1][1], s0, s1, gi & 1, gj & 1), lim


def level_array(nx, ny, boxes, arrays):
    """the valid cells of a level's ghosted box arrays on its whole domain, NaN where no box is"""
    out = np.full((ny, nx), np.nan)
    for (lo0, lo1, hi0, hi1), a in zip(boxes, arrays):
        out[lo1:hi1 + 1, lo0:hi0 + 1] = a[1:-1, 1:-1]
    return out


def _wrapped(i, j, n, periodic):
    c = [i, j]
    for d in range(2):
        if 0 <= c[d] < n[d]:
            continue
        if not periodic[d]:
            return None
        c[d] %= n[d]
    return c


def regrid(nx0, ny0, periodic, old_boxes, new_boxes, old_fields, base_field, rule=None):
    coarse = np.array(base_field[1:-1, 1:-1], dtype=np.float64)            # level l - 1 of the NEW hierarchy on its whole domain
    out = []
    for l, bl in enumerate(new_boxes, start=1):
        nc, nf = (nx0 << (l - 1), ny0 << (l - 1)), (nx0 << l, ny0 << l)
        full = np.full((nf[1], nf[0]), np.nan)
        # (a) interpolation of every valid cell
        for lo0, lo1, hi0, hi1 in bl:
            for J in range(lo1 // 2, hi1 // 2 + 1):
                for I in range(lo0 // 2, hi0 // 2 + 1):
                    v, _ = interp_cell(coarse, I, J, nc, periodic)
                    for q in range(2):
                        for p in range(2):
                            full[2 * J + q, 2 * I + p] = v[q][p]
        # (c) the old valid cells win
        if l <= len(old_boxes):
            for (lo0, lo1, hi0, hi1), a in zip(old_boxes[l - 1], old_fields[l - 1]):
                held = ~np.isnan(full[lo1:hi1 + 1, lo0:hi0 + 1])
                full[lo1:hi1 + 1, lo0:hi0 + 1][held] = np.asarray(a)[1:-1, 1:-1][held]
        arrays = []
        for lo0, lo1, hi0, hi1 in bl:
            nx, ny = hi0 - lo0 + 1, hi1 - lo1 + 1
            g = np.zeros((ny + 2, nx + 2))
            g[1:-1, 1:-1] = full[lo1:hi1 + 1, lo0:hi0 + 1]
            for jj in range(ny + 2):
                for ii in range(nx + 2):
                    if 1 <= ii <= nx and 1 <= jj <= ny:
                        continue
                    w = _wrapped(lo0 + ii - 1, lo1 + jj - 1, nf, periodic)
                    if w is None:
                        continue                                              # a domain ghost cell: (e), or nobody
                    if not np.isnan(full[w[1], w[0]]):
                        g[jj, ii] = full[w[1], w[0]]                          # (d) exchange, corners included
                    else:
                        g[jj, ii] = pwl_cell(coarse, w[0], w[1], nc)[0]       # (b) coarse-fine ghost cell
            # (e) domain ghost cells across a non-periodic side, side cells only
            if rule is not None:
                ext = rule == "extrap"
                if not periodic[0]:
                    if lo0 == 0:
                        g[1:-1, 0] = 2.0 * g[1:-1, 1] - g[1:-1, 2] if ext else g[1:-1, 1]
                    if hi0 == nf[0] - 1:
                        g[1:-1, -1] = 2.0 * g[1:-1, -2] - g[1:-1, -3] if ext else g[1:-1, -2]
                if not periodic[1]:
                    if lo1 == 0:
                        g[0, 1:-1] = 2.0 * g[1, 1:-1] - g[2, 1:-1] if ext else g[1, 1:-1]
                    if hi1 == nf[1] - 1:
                        g[-1, 1:-1] = 2.0 * g[-2, 1:-1] - g[-3, 1:-1] if ext else g[-2, 1:-1]
            arrays.append(g)
        out.append(arrays)
        coarse = full
    return out
