"""Plot files of the hydrology state in Chombo's HDF5 layout (include/suhmo_plt.h, suhmo_amd/csrc/suhmo_plt.cpp): AmrHydro::writePlotFile
(src/AmrHydro.cpp:5474-5667).  The thirteen components of every box of every level come off the device in ONE snapshot (suhmo_hier_snapshot:
a launch and a copy per level) and go into the file as they are, a multi-component dataset per level."""
import ctypes as C

import numpy as np

from . import capi, checkpoint, level as lv

LIB_PATH = checkpoint.LIB_PATH            # the library of the checkpoint files holds the plot files too
_LIB = None
SYMBOLS = ["suhmo_plt_last_error", "suhmo_plt_create", "suhmo_plt_write_level", "suhmo_plt_close", "suhmo_plt_open", "suhmo_plt_read_name",
           "suhmo_plt_read_level", "suhmo_plt_read_data"]
# plot component -> what the snapshot reads (src/AmrHydro.cpp:5484-5511, in that order); Qw is the water flux averaged from faces to cells
COMPONENTS = [("head", capi.SNAP_FIELD, lv.F_PHI), ("gapHeight", capi.SNAP_FIELD, lv.F_B), ("bedelevation", capi.SNAP_FIELD, lv.F_ZB),
              ("overburdenPress", capi.SNAP_FIELD, lv.F_PI), ("Pw", capi.SNAP_FIELD, lv.F_PW), ("Qw_x", capi.SNAP_FACE_TO_CELL, lv.F_QWX),
              ("Qw_y", capi.SNAP_FACE_TO_CELL, lv.F_QWY), ("Re", capi.SNAP_FIELD, lv.F_RE), ("meltRate", capi.SNAP_FIELD, lv.F_MR),
              ("GradHead_x", capi.SNAP_FIELD, lv.F_GRADX), ("GradHead_y", capi.SNAP_FIELD, lv.F_GRADY), ("iceHeight", capi.SNAP_FIELD, lv.F_ZS),
              ("iceMask", capi.SNAP_FIELD, lv.F_MASK)]
NAMES = [c[0] for c in COMPONENTS]
SNAP = [(kind, field) for _, kind, field in COMPONENTS]
GHOST = 1                                 # the reference plots with one ghost cell


def build(force=False):
    return checkpoint.build(force)


def lib():
    global _LIB
    if _LIB is None:
        checkpoint.lib()                  # (raises when the library is not built)
        L = C.CDLL(LIB_PATH)
        vp, ci, dp, ip, lp = C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_long)
        L.suhmo_plt_last_error.restype = C.c_char_p
        L.suhmo_plt_create.argtypes = [C.POINTER(vp), C.c_char_p, ci, ci, C.POINTER(C.c_char_p), C.c_double, C.c_double]
        L.suhmo_plt_write_level.argtypes = [vp, ci, C.c_double, C.c_double, ip, ci, ip, ci, lp, dp]
        L.suhmo_plt_close.argtypes = [vp]
        L.suhmo_plt_open.argtypes = [C.POINTER(vp), C.c_char_p, ip, ip]
        L.suhmo_plt_read_name.argtypes = [vp, ci, C.c_char_p, ci]
        L.suhmo_plt_read_level.argtypes = [vp, ci, dp, ip, dp, ip, dp, dp, ip, ip, ip, ci, ip, lp]
        L.suhmo_plt_read_data.argtypes = [vp, ci, lp, dp]
        _LIB = L
    return _LIB


def _check(rc):
    if rc:
        raise RuntimeError("libsuhmo_chk: " + lib().suhmo_plt_last_error().decode())


def write_levels(path, names, levels, time, dt=1.0, ghost=GHOST):
    """levels[l] = dict(dx, dy, domain=(lo0, lo1, hi0, hi1), boxes=[(lo0, lo1, hi0, hi1), ...], offsets=(nbox + 1,) prefix sums in doubles,
    data=flat float64 array: box after box, each [comp][j][i] over the box grown by `ghost` -- a level slice of a snapshot)"""
    h = C.c_void_p()
    cn = (C.c_char_p * len(names))(*[n.encode() for n in names])
    _check(lib().suhmo_plt_create(C.byref(h), str(path).encode(), len(levels), len(names), cn, float(time), float(dt)))
    try:
        for l, v in enumerate(levels):
            bx = np.ascontiguousarray(np.array(v["boxes"], dtype=np.int32).reshape(-1, 4))
            off = np.ascontiguousarray(v["offsets"], dtype=np.int64)
            data = v["data"]
            assert data.dtype == np.float64 and data.flags.c_contiguous and data.ndim == 1 and off.shape == (len(bx) + 1,) and data.size == off[-1]
            dom = (C.c_int * 4)(*[int(q) for q in v["domain"]])
            _check(lib().suhmo_plt_write_level(h, l, float(v["dx"]), float(v["dy"]), dom, len(bx), bx.ctypes.data_as(C.POINTER(C.c_int)), int(ghost),
                                               off.ctypes.data_as(C.POINTER(C.c_long)), data.ctypes.data_as(C.POINTER(C.c_double))))
    finally:
        lib().suhmo_plt_close(h)


def read_levels(path):
    """-> (names, levels): levels[l] = dict(dx, dy (vec_dx), vec_ref_ratio, dx_attr / ref_ratio (the scalar attributes; 0 where the file has
    none), dt, time, domain, boxes, ghost, offsets, data (flat) and fabs = per box the (ncomp, ny + 2 ghost, nx + 2 ghost) view of data)"""
    h, nlev, ncomp = C.c_void_p(), C.c_int(), C.c_int()
    _check(lib().suhmo_plt_open(C.byref(h), str(path).encode(), C.byref(nlev), C.byref(ncomp)))
    levels, names = [], []
    try:
        buf = C.create_string_buffer(256)
        for c in range(ncomp.value):
            _check(lib().suhmo_plt_read_name(h, c, buf, len(buf)))
            names.append(buf.value.decode())
        for l in range(nlev.value):
            vdx, vr, dom = (C.c_double * 2)(), (C.c_int * 2)(), (C.c_int * 4)()
            dx, ref, dt, time, nb, g, nd = C.c_double(), C.c_int(), C.c_double(), C.c_double(), C.c_int(), C.c_int(), C.c_long()
            _check(lib().suhmo_plt_read_level(h, l, vdx, vr, C.byref(dx), C.byref(ref), C.byref(dt), C.byref(time), dom, C.byref(nb), None, 0,
                                              C.byref(g), C.byref(nd)))
            bx = np.zeros((nb.value, 4), dtype=np.int32)
            _check(lib().suhmo_plt_read_level(h, l, None, None, None, None, None, None, None, C.byref(nb), bx.ctypes.data_as(C.POINTER(C.c_int)),
                                              nb.value, None, None))
            off, data = np.zeros(nb.value + 1, dtype=np.int64), np.zeros(nd.value)
            _check(lib().suhmo_plt_read_data(h, l, off.ctypes.data_as(C.POINTER(C.c_long)), data.ctypes.data_as(C.POINTER(C.c_double))))
            boxes = [tuple(int(q) for q in b) for b in bx]
            fabs = [data[off[k]:off[k + 1]].reshape(ncomp.value, b[3] - b[1] + 1 + 2 * g.value, b[2] - b[0] + 1 + 2 * g.value) for k, b in enumerate(boxes)]
            levels.append(dict(dx=vdx[0], dy=vdx[1], vec_ref_ratio=(vr[0], vr[1]), dx_attr=dx.value, ref_ratio=ref.value, dt=dt.value, time=time.value,
                               domain=tuple(dom), boxes=boxes, ghost=g.value, offsets=off, data=data, fabs=fabs))
    finally:
        lib().suhmo_plt_close(h)
    return names, levels


def levels_of_snapshot(model, level_offset, box_offset, flat):
    """the levels write_levels takes from a snapshot of a HipHierModel (boxes as checkpoint._boxes_of lists them)"""
    tree = checkpoint._boxes_of(model)
    nx0, ny0 = tree[0][0][1][2] + 1, tree[0][0][1][3] + 1
    return [dict(dx=bl[0][0].dx, dy=bl[0][0].dy, domain=(0, 0, (nx0 << l) - 1, (ny0 << l) - 1), boxes=[b for _, b in bl], offsets=box_offset[l],
                 data=flat[level_offset[l]:level_offset[l + 1]]) for l, bl in enumerate(tree)]


def write(path, model, time, dt=1.0):
    """AmrHydro::writePlotFile of a device-resident HipModel or HipHierModel: one snapshot of the thirteen components (each as the last step
    left it; a field no box holds yet is 0), one file.  dt: the reference passes 1."""
    from . import model as md
    if isinstance(model, md.HipHierModel):
        lo, bo, flat = model.hier.snapshot(SNAP, GHOST)
        levels = levels_of_snapshot(model, lo, bo, flat)
    elif isinstance(model, md.HipModel):
        L = model.level
        flat = L.snapshot(SNAP, GHOST).reshape(-1)
        levels = [dict(dx=L.dx, dy=L.dy, domain=(0, 0, L.nx - 1, L.ny - 1), boxes=[(0, 0, L.nx - 1, L.ny - 1)], offsets=np.array([0, flat.size]), data=flat)]
    else:
        raise TypeError("plotfile.write takes a HipModel or a HipHierModel, not %s" % type(model).__name__)
    write_levels(path, NAMES, levels, time, dt)


def pp_name(prefix, step):
    """the name AmrHydro::writePltPP gives its file (src/AmrHydro.cpp:5349-5361, namePlot = ".2d" at :4823)"""
    return "%sCustom%06d.2d.hdf5" % (prefix, int(step))


def write_pp(path, model, time, max_level=None):
    """AmrHydro::writePltPP (src/AmrHydro.cpp:5298-5389) of a HipHierModel: gap height and N = Pi - Pw of the whole hierarchy on the uniform grid
    of level max_level (HipHierModel.interp_finest: one flatten on the device, one copy), written as ONE level with ghost 0 and dx = level 0's
    dx / 2^max_level.  Deviations from the reference's file: the finest domain is one box (the reference cuts it with domainSplit); the
    ratio attribute is what write_levels writes for a finest level; the reference's third quantity tau (:4678) is not built.
    -> the (2, nyF, nxF) array that went into the file"""
    H = model.hier
    ml = H.nlev - 1 if max_level is None else int(max_level)
    a = H.flatten([c for _, c in model.PP_COMPONENTS], ml)
    nyF, nxF = a.shape[1:]
    L0 = model.level[0][0]
    lev = dict(dx=L0.dx / 2 ** ml, dy=L0.dy / 2 ** ml, domain=(0, 0, nxF - 1, nyF - 1), boxes=[(0, 0, nxF - 1, nyF - 1)], offsets=np.array([0, a.size]),
               data=a.reshape(-1))
    write_levels(path, [nm for nm, _ in model.PP_COMPONENTS], [lev], time, 1.0, ghost=0)
    return a
