"""Host-side handle on the hydrology time loop of one device-resident level: the single-level
subset of AmrHydro::timeStepFAS (src/AmrHydro.cpp:2254-3460) the C-ABI exposes as
suhmo_level_timestep.  Head = F_PHI and gap height = F_B stay in HBM from step to step."""
import ctypes as C

import numpy as np

from . import capi, level as lv
from . import synthetic as sy
from .capi import check


def model_params(m):
    ub = m.get("ub", (0.0, 0.0))
    return capi.ModelParams(m["rho_i"], m["rho_w"], m["gravity"], m["G"], m["L"], m["ct"], m["cw"], ub[0], ub[1],
                            m["br"], m["lr"], m.get("diffFactor", 0.0), m["distributed_input"], m["eps_picard"],
                            int(m.get("basal_friction", 1)), int(m.get("use_mask_rhs_b", 0)),
                            int(m.get("use_moulin_source", 0)), float(m.get("ramp", 1.0)), int(m.get("use_impl_diff", 0)),
                            int(m.get("head_melt_off", 0)), int(m.get("freeze_icefree_gap", 0)))


# the reference's tag variables (AmrHydro.tag_variables, src/AmrHydro.cpp:4539-4604) under the names of HipModel.FIELDS
TAG_VARIABLES = dict(meltingRate="mR", GapHeight="B", Pi="Pi", Qx="qwx")


def _tag_field(fields, name):
    if isinstance(name, int):
        return name
    return fields[TAG_VARIABLES.get(name, name)]


def _tag_reach(grow, grow_dir):
    return int(grow), int(grow_dir[0]), int(grow_dir[1])


def _tags_out(get, *handle):
    """the tag map behind get(*handle, host, nbx, nby) as a (nby, nbx) uint8 array; None when there is none"""
    nbx, nby = C.c_int(), C.c_int()
    check(get(*handle, None, C.byref(nbx), C.byref(nby)))
    if nbx.value == 0:
        return None
    out = np.zeros((nby.value, nbx.value), dtype=np.uint8)
    check(get(*handle, out.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(nbx), C.byref(nby)))
    return out


def _boxes_out(nlev, nbox, flat):
    boxes, q = [], 0
    for l in range(1, nlev):
        boxes.append([tuple(int(v) for v in flat[q + 4 * k:q + 4 * k + 4]) for k in range(nbox[l])])
        q += 4 * nbox[l]
    return boxes


def _generate(call, ntag):
    """run call(nlev, nbox, boxes, cap) -> rc with a box buffer that grows to the count the library reports"""
    nlev, nbox, cap = C.c_int(), (C.c_int * (ntag + 1))(), 256
    while True:
        flat = (C.c_int * (4 * cap))()
        rc = call(C.byref(nlev), nbox, flat, cap)
        if rc == -4 and sum(nbox) > cap:
            cap = sum(nbox)
            continue
        check(rc)
        return _boxes_out(nlev.value, list(nbox), list(flat))


def generate_grids(nx0, ny0, periodic, tags, fill_ratio, block_factor, max_box_size, nesting_radius=2):
    """suhmo_grids_generate, the host part alone (no device): tags[l] = the (ny0 << l) / g x (nx0 << l) / g map of level l at granularity
    g = block_factor / 2 -> boxes[l - 1] = list of (lo0, lo1, hi0, hi1) in the index space of level l, as HipHierModel takes them"""
    g = int(block_factor) // 2
    maps = []
    for l, t in enumerate(tags):
        a = np.ascontiguousarray(t, dtype=np.uint8)
        if g < 1 or a.shape != ((ny0 << l) // g, (nx0 << l) // g):
            raise ValueError("tags[%d] has shape %s, level %d at block_factor %d needs %s" % (l, a.shape, l, block_factor, ((ny0 << l) // max(g, 1), (nx0 << l) // max(g, 1))))
        maps.append(a)
    ucp = C.POINTER(C.c_ubyte)
    ptr = (ucp * max(len(maps), 1))(*[a.ctypes.data_as(ucp) for a in maps])
    per = (C.c_int * 2)(int(periodic[0]), int(periodic[1]))
    gp = capi.GridParams(float(fill_ratio), int(block_factor), int(max_box_size), int(nesting_radius))
    return _generate(lambda nlev, nbox, flat, cap: capi.lib().suhmo_grids_generate(int(nx0), int(ny0), per, C.byref(gp), len(maps), ptr, nlev, nbox, flat, cap),
                     len(maps))


def regrid_steps(first_cur_step, n_steps, interval, skip_first=False):
    """the cur_step values before whose step a run regrids (suhmo_hier_run, rule 1; src/AmrHydro.cpp:1317): c = first_cur_step + k with
    c - 1 != 0 and (c - 1) % interval == 0 -- c - 1 is the reference's m_cur_step before its increment -- except the run's first step when
    skip_first is set (m_cur_step != m_restart_step).  interval 0: never."""
    out = []
    for k in range(int(n_steps)):
        c = int(first_cur_step) + k
        if interval > 0 and c - 1 != 0 and (c - 1) % interval == 0 and not (k == 0 and skip_first):
            out.append(c)
    return out


PLOT, CHECKPOINT = 0, 1            # the `kind` of an output event (suhmo_hier_output_fn)


def output_steps(first_cur_step, n_steps, plot_interval, check_interval, restart_step=0, final=True):
    """the plot files and checkpoints a run writes (suhmo_hier_run_out; src/AmrHydro.cpp:1311, :1327, :1343-1358), in order:
    [(kind, cur_step, where)] with kind PLOT / CHECKPOINT, cur_step the reference's m_cur_step in the file name and where "before_regrid"
    (the plot before step c = cur_step + 1, taken before that step's regrid), "after_regrid" (the checkpoint before step c, taken after it) or
    "final" (after the last step; cur_step = the last c).  With b = c - 1: a plot when plot_interval > 0 and b % plot_interval == 0, b = 0
    included; a checkpoint when check_interval > 0, b % check_interval == 0 and b != restart_step; after the last step a plot when
    plot_interval >= 0 and a checkpoint when check_interval >= 0, unless final is False (a run that another run continues).  An interval
    of -1 switches that kind off."""
    out = []
    for k in range(int(n_steps)):
        b = int(first_cur_step) + k - 1
        if plot_interval > 0 and b % plot_interval == 0:
            out.append((PLOT, b, "before_regrid"))
        if check_interval > 0 and b % check_interval == 0 and b != restart_step:
            out.append((CHECKPOINT, b, "after_regrid"))
    if final and n_steps > 0:
        last = int(first_cur_step) + int(n_steps) - 1
        if plot_interval >= 0:
            out.append((PLOT, last, "final"))
        if check_interval >= 0:
            out.append((CHECKPOINT, last, "final"))
    return out


def _flat_boxes(levels):
    """[[(lo0, lo1, hi0, hi1), ...] per level] -> (counts, ints) as the C-ABI takes box lists"""
    nbox = (C.c_int * max(len(levels), 1))(*[len(bl) for bl in levels])
    flat = [int(v) for bl in levels for b in bl for v in b]
    return nbox, (C.c_int * max(len(flat), 1))(*flat)


def nest_tag_subsets(subsets):
    """suhmo_tag_subsets_nest (host only): the per-level tagSubset box lists, level 0 first, nested the way the reference does when it
    reads tagSubsetBoxesFile (src/AmrHydro.cpp:1097-1108): a level whose list is empty inherits the refined subset of the level below, a
    level with boxes is intersected with it, and an empty subset below constrains nothing.  -> the nested lists, as restrict_tags /
    tag_and_regrid / run take them"""
    subsets = [[tuple(int(v) for v in b) for b in bl] for bl in subsets]
    nbox, flat = _flat_boxes(subsets)
    out_n, cap = (C.c_int * max(len(subsets), 1))(), 64
    while True:
        out = (C.c_int * (4 * cap))()
        rc = capi.lib().suhmo_tag_subsets_nest(len(subsets), nbox, flat, out_n, out, cap)
        if rc == -4 and sum(out_n) > cap:
            cap = sum(out_n)
            continue
        check(rc)
        break
    res, q = [], 0
    for l in range(len(subsets)):
        res.append([tuple(int(v) for v in out[q + 4 * k:q + 4 * k + 4]) for k in range(out_n[l])])
        q += 4 * out_n[l]
    return res


def ibc(kind, **params):
    """suhmo_ibc_t for init_ibc / set_ibc: kind "basic", "sqrt", "valley" or "dino" (the reference's problem_type) and the values its formulas
    read -- slope, ice_height (m_H), gap_init, rho_i, rho_w, gravity, G, L, gamma (valley).  Defaults: synthetic's constants, suite A's G and L,
    slope 0, ice_height 5000, gap_init 0.01, gamma 0.05"""
    p = dict(slope=0.0, ice_height=5000.0, gap_init=0.01, rho_i=sy.RHO_I, rho_w=sy.RHO_W, gravity=sy.GRAV, G=sy.A3_MODEL["G"], L=sy.A3_MODEL["L"],
             gamma=0.05)
    unknown = set(params) - set(p)
    if unknown:
        raise ValueError("ibc: unknown parameter(s) %s" % sorted(unknown))
    p.update(params)
    k = capi.IBC_KINDS[kind] if isinstance(kind, str) else int(kind)
    return capi.Ibc(k, *[float(p[q]) for q in ("slope", "ice_height", "gap_init", "rho_i", "rho_w", "gravity", "G", "L", "gamma")])


ALL_LEVELS = 8          # max_level of a run or a tag_and_regrid that is given none: a hierarchy has at most 8 levels


def initial_grids(make_model, tag_specs, params, max_level):
    """The loop of AmrHydro::initGrids (src/AmrHydro.cpp:4835-4955): make_model(boxes) creates a model on the boxes so far and loads its
    initial state -- boxes = [] first: level 0 alone, a HipModel or a HipHierModel without boxes -- every level is tagged with tag_specs
    (dicts of tag_cells' arguments: name, vmin, vmax, grow, grow_dir), grids are generated with params (generate_grids' keywords), and the
    loop repeats while a new level appeared and max_level is not reached.  Returns (boxes, the model on them); the models in between are closed."""
    g = int(params["block_factor"]) // 2
    boxes = []
    m = make_model(boxes)
    while len(boxes) < max_level:
        if isinstance(m, HipModel):
            for sp in tag_specs:
                m.tag_cells(granularity=g, **sp)
            new = generate_grids(m.nx, m.ny, m.level._desc.bc.periodic, [m.tags()], **params)
        else:
            for l in range(len(boxes) + 1):
                for sp in tag_specs:
                    m.tag_cells(l, granularity=g, **sp)
            new, _ = m.generate_grids(**params)
        new = new[:max_level]
        if len(new) <= len(boxes):
            break
        m.close()
        boxes = new
        m = make_model(boxes)
    return boxes, m


class HipModel:
    FIELDS = dict(head=lv.F_PHI, B=lv.F_B, Pi=lv.F_PI, zb=lv.F_ZB, mask=lv.F_MASK, mR=lv.F_MR, Pw=lv.F_PW,
                  qwx=lv.F_QWX, qwy=lv.F_QWY, cd=lv.F_CD, rhs_h=lv.F_RHS, Re=lv.F_RE, msrc=lv.F_MSRC,
                  dcx=lv.F_DCX, dcy=lv.F_DCY, dterm=lv.F_DTERM)

    def __init__(self, nx, ny, dx, dy, bc, phys, model, max_box=64, device=0, j0=0, ny_global=None, halo_rows=1):
        """j0 / ny_global: this process holds rows j0 .. j0 + ny - 1 of a level of ny_global rows (one strip per GPU;
        couple the strips with suhmo_amd.multigpu.attach(model.level, ...) before the first step)"""
        self.level = lv.HipLevel(nx, ny, dx, dy, bc, phys, alpha=0.0, beta=-1.0, max_box=max_box, device=device,
                                 j0=j0, ny_global=ny_global, halo_rows=halo_rows)
        self.nx, self.ny, self.dx, self.dy = nx, ny, dx, dy
        self.model = dict(model)
        self._mp = model_params(model)
        self.cur_step = 0

    def set_state(self, f):
        """f: dict with ghosted (ny+2, nx+2) arrays head, B, Pi, zb, mask"""
        L = self.level
        L.set(lv.F_PHI, f["head"][1:-1, 1:-1])
        L.set(lv.F_ACOEF, np.zeros((self.ny, self.nx)))
        for k, fid in (("B", lv.F_B), ("Pi", lv.F_PI), ("zb", lv.F_ZB), ("mask", lv.F_MASK)):
            L.set(fid, f[k], ghosted=True)

    def init_ibc(self, ibc):
        """the initial state evaluated on the device (suhmo_level_ibc_init): initializeData and setup_iceMask of the reference's IBC class
        `ibc` (model.ibc(kind, ...)) in one launch -- head, B, Pi, zb, mask, zs, Pw, mR; nothing is loaded from the host"""
        check(capi.lib().suhmo_level_ibc_init(self.level.h, C.byref(ibc) if ibc is not None else None, self.level.stream))

    def moulin_source(self, positions, sigma, flux, time_factor=1.0):
        """Calc_moulin_integral + Calc_moulin_source_term_distributed (src/AmrHydro.cpp:1866-2066) -> F_MSRC; returns the integrals"""
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1)
        sg, fl = np.ascontiguousarray(sigma, dtype=np.float64), np.ascontiguousarray(flux, dtype=np.float64)
        integ = np.zeros(sg.size)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        check(capi.lib().suhmo_level_moulin_source(self.level.h, sg.size, dp(pos), dp(sg), dp(fl), float(time_factor), dp(integ),
                                                   self.level.stream))
        return integ

    def time_varying_recharge(self, zs, T_K, background):
        """suhmo.time_varying_input (src/AmrHydro.cpp:2849-2861): F_MSRC from the ghosted ice surface height zs"""
        self.level.set(lv.F_ZS, zs, ghosted=True)
        check(capi.lib().suhmo_level_time_varying_recharge(self.level.h, float(T_K), float(background), self.level.stream))

    def tag_cells(self, name, vmin, vmax, grow=0, grow_dir=(0, 0), granularity=1):
        """tagCellsLevel on this level (suhmo_level_tag_cells): cells with vmin < name < vmax, grown by `grow` cells (and to grow_dir in a
        direction where that is more), join the level's tag map, kept at `granularity` cells per entry"""
        check(capi.lib().suhmo_level_tag_cells(self.level.h, _tag_field(self.FIELDS, name), float(vmin), float(vmax), *_tag_reach(grow, grow_dir),
                                               int(granularity), self.level.stream))

    def clear_tags(self):
        check(capi.lib().suhmo_level_clear_tags(self.level.h))

    def tags(self):
        """the tag map, (nby, nbx) uint8; None before the first tag_cells and after clear_tags"""
        return _tags_out(capi.lib().suhmo_level_get_tags, self.level.h)

    def timestep(self, dt):
        self.cur_step += 1                                         # src/AmrHydro.cpp:2259
        pi, nv = C.c_int(), C.c_int()
        check(capi.lib().suhmo_level_timestep(self.level.h, C.byref(self._mp), float(dt), self.cur_step,
                                              C.byref(pi), C.byref(nv), self.level.stream))
        return pi.value, nv.value

    def get(self, name, ghosted=False):
        return self.level.get(self.FIELDS[name], ghosted=ghosted)

    def postproc_temporal(self):
        """the daily row of AmrHydro.post_proc_shmip_temporal (suhmo_level_postproc_temporal): avgN, N in the three bands, recharge, discharge"""
        out = np.zeros(6)
        check(capi.lib().suhmo_level_postproc_temporal(self.level.h, C.byref(self._mp), out.ctypes.data_as(C.POINTER(C.c_double)), self.level.stream))
        return out

    def postproc_temporal_device(self):
        """the same row finished on the device (suhmo_level_postproc_temporal_device): the column sums stay there"""
        out = np.zeros(6)
        check(capi.lib().suhmo_level_postproc_temporal_device(self.level.h, C.byref(self._mp), out.ctypes.data_as(C.POINTER(C.c_double)), self.level.stream))
        return out

    def postproc_table_device(self):
        """SHMIP cross-section table reduced on the device (suhmo_level_postproc_table)"""
        t = np.zeros((self.nx, 8))
        check(capi.lib().suhmo_level_postproc_table(self.level.h, C.byref(self._mp), t.ctypes.data_as(C.POINTER(C.c_double)),
                                                    self.level.stream))
        return t

    def postproc_partial(self):
        """column sums over this strip's rows (8 x nx); add them over the ranks, then postproc_finish"""
        t = np.zeros((8, self.nx))
        check(capi.lib().suhmo_level_postproc_partial(self.level.h, C.byref(self._mp), t.ctypes.data_as(C.POINTER(C.c_double)),
                                                      self.level.stream))
        return t

    def postproc_finish(self, sums):
        t, a = np.zeros((self.nx, 8)), np.ascontiguousarray(sums, dtype=np.float64)
        check(capi.lib().suhmo_postproc_finish(a.ctypes.data_as(C.POINTER(C.c_double)), self.nx, self.dx,
                                               t.ctypes.data_as(C.POINTER(C.c_double))))
        return t

    def postproc_temporal_host(self, sums):
        """the daily row from column sums already on the host (suhmo_postproc_temporal; the sums of rank strips added up, or one member's rows
        of HipBatchModel.postproc_partial_all)"""
        out, a = np.zeros(6), np.ascontiguousarray(sums, dtype=np.float64)
        check(capi.lib().suhmo_postproc_temporal(a.ctypes.data_as(C.POINTER(C.c_double)), self.nx, self.dx, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def mass_balance(self):
        """AmrHydro::check_fluxes reduced on the device (suhmo_level_mass_balance; include/suhmo_hip.h, "MASS BALANCE"): the discharge through
        the four domain sides (lo_x, hi_x, lo_y, hi_y), through the ice margin and the ice-bearing domain sides (dir_x, dir_y) and the water
        volume of the state as it is -> a dict of the seven names (capi.MB_NAMES).  Read-only"""
        out = np.zeros(len(capi.MB_NAMES))
        check(capi.lib().suhmo_level_mass_balance(self.level.h, out.ctypes.data_as(C.POINTER(C.c_double)), self.level.stream))
        return dict(zip(capi.MB_NAMES, out.tolist()))

    def water_budget(self):
        """the conservation record of a step (suhmo_level_water_budget; include/suhmo_hip.h, "WATER BUDGET"): the seven values of
        mass_balance, volume_old (the volume the last step with level option track_old_volume = 1 started from; NaN: none) and the two
        parts of the reference's rechargeTOT -> a dict of the ten names (capi.WB_NAMES).  Read-only"""
        out = np.zeros(len(capi.WB_NAMES))
        check(capi.lib().suhmo_level_water_budget(self.level.h, C.byref(self._mp), out.ctypes.data_as(C.POINTER(C.c_double)), self.level.stream))
        return dict(zip(capi.WB_NAMES, out.tolist()))

    def postproc_table(self):
        """SHMIP cross-section table (src/AmrHydro.cpp:3647-4102) from the device-resident state, reduced on the host"""
        mask = self.get("mask")
        src = np.where(mask > 0.0, self.model["distributed_input"], 0.0)
        return sy.shmip_postproc_table(self.dx, self.dy, self.get("qwx"), self.get("cd", ghosted=True), src,
                                       self.get("mR"), self.get("Pw"), self.get("Pi"), mask, self.model["rho_w"])

    def close(self):
        self.level.close()


class _MemberModel(HipModel):
    """Member k of a HipBatchModel as a HipModel: state, moulin source, recharge and post-processing through the member's level handle
    (stepping belongs to the batch)"""

    def __init__(self, level, model):
        self.level, self.nx, self.ny, self.dx, self.dy = level, level.nx, level.ny, level.dx, level.dy
        self.model = dict(model)
        self._mp = model_params(model)
        self.cur_step = 0

    def timestep(self, dt):
        raise capi.SuhmoError("a member of a batch is stepped by HipBatchModel.timestep")

    def close(self):
        pass


class HipBatchModel:
    """An ensemble of n models on one grid stepped together (suhmo_batch_timestep, suhmo_amd/csrc/suhmo_batch.hip): shared grid, BC types,
    dt and step number; per member every field, the BC values, the physics constants and the model parameters.  models: one dict per member
    (as HipModel's); phys / bc: one for all or a list per member.  Every member's results are those of a HipModel run alone, bit for bit.
    implicit_gap=True (batch option implicit_gap): members with use_impl_diff=1 are stepped too, their gap-height solves as one launch
    sequence; explicit and implicit members may share a batch.  Off, such a member is refused.
    bottom_solver=True: the head solves and the implicit gap-height solves end every V-cycle with RelaxSolver (HipBatch), as the reference does."""

    FIELDS = HipModel.FIELDS

    def __init__(self, nx, ny, dx, dy, bc, phys, models, max_box=64, device=0, implicit_gap=False, bottom_solver=False):
        n = len(models)
        bcs = list(bc) if isinstance(bc, (list, tuple)) else [bc] * n
        phs = list(phys) if isinstance(phys, (list, tuple)) else [phys] * n
        self.batch = lv.HipBatch(n, nx, ny, dx, dy, bcs[0], phs[0], alpha=0.0, beta=-1.0, max_box=max_box, device=device, bottom_solver=bottom_solver)
        self.n, self.nx, self.ny, self.dx, self.dy = n, nx, ny, dx, dy
        if implicit_gap:
            self.batch.set_option("implicit_gap", 1)
        for k in range(n):
            self.batch.set_bc(k, bcs[k])
            self.batch.set_phys(k, phs[k])
        self.members = [_MemberModel(self.batch.member(k), models[k]) for k in range(n)]
        self._mp = (capi.ModelParams * n)(*[m._mp for m in self.members])
        self.cur_step = 0

    def member(self, k):
        """member k with HipModel's methods: set_state, moulin_source, time_varying_recharge, get, postproc_*"""
        return self.members[k]

    def set_state(self, k, f):
        self.members[k].set_state(f)

    def init_ibc_all(self, ibcs, active=None):
        """the initial state of every (active) member on the device in one launch (suhmo_batch_ibc_init): ibcs = one model.ibc(...) per member
        -- the same kind, any parameters, e.g. SHMIP E's five gammas -- or one for all"""
        rows = list(ibcs) if isinstance(ibcs, (list, tuple)) else [ibcs] * self.n
        if len(rows) != self.n:
            raise ValueError("init_ibc_all: %d rows for %d members" % (len(rows), self.n))
        arr = (capi.Ibc * self.n)(*rows)
        check(capi.lib().suhmo_batch_ibc_init(self.batch.h, arr, self._active(active), self.batch.stream))

    def set_model(self, k, **changes):
        """change model parameters of member k between steps (e.g. ramp)"""
        m = self.members[k]
        m.model.update(changes)
        m._mp = model_params(m.model)
        self._mp[k] = m._mp

    def timestep(self, dt):
        """one step of every member; returns ([picard iterations], [V-cycles]) per member"""
        self.cur_step += 1
        pi, nv = (C.c_int * self.n)(), (C.c_int * self.n)()
        check(capi.lib().suhmo_batch_timestep(self.batch.h, self._mp, float(dt), self.cur_step, pi, nv, self.batch.stream))
        for m in self.members:
            m.cur_step = self.cur_step
        return list(pi), list(nv)

    def get(self, k, name, ghosted=False):
        return self.members[k].get(name, ghosted=ghosted)

    def postproc_table(self, k):
        return self.members[k].postproc_table()

    def postproc_table_device(self, k):
        return self.members[k].postproc_table_device()

    def postproc_temporal(self, k):
        return self.members[k].postproc_temporal()

    # ---- forcing and diagnostics of all members at once (suhmo_batch_time_varying_recharge / _moulin_source / _postproc_*): the launches of
    # one member whatever n, every member bit for bit what the per-k methods give
    def _active(self, active):
        return None if active is None else (C.c_int * self.n)(*[int(bool(x)) for x in active])

    def _per_member(self, x):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (self.n,)))

    def set_surface(self, k, zs):
        """the ghosted ice surface height of member k (F_ZS): loaded once, it stays on the device for time_varying_recharge"""
        self.members[k].level.set(lv.F_ZS, zs, ghosted=True)

    def time_varying_recharge(self, T_K, background, active=None):
        """F_MSRC of every member from its surface height (set_surface); T_K, background: one for all or one per member"""
        tk, bg = self._per_member(T_K), self._per_member(background)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        check(capi.lib().suhmo_batch_time_varying_recharge(self.batch.h, dp(tk), dp(bg), self._active(active), self.batch.stream))

    def moulin_source(self, lists, time_factor=1.0, active=None):
        """lists[k] = (positions, sigma, flux) of member k (None for a member that is not active); time_factor: one for all or one per member.
        Returns the integrals of every member's moulins (None for a member that is not active)"""
        on = [True] * self.n if active is None else [bool(x) for x in active]
        pos, sg, fl, cnt = [], [], [], []
        for k in range(self.n):
            if lists[k] is None:
                assert not on[k], "member %d is active and has no moulin list" % k
                cnt.append(0)
                continue
            s = np.asarray(lists[k][1], dtype=np.float64).reshape(-1)
            pos.append(np.asarray(lists[k][0], dtype=np.float64).reshape(-1)); sg.append(s); fl.append(np.asarray(lists[k][2], dtype=np.float64).reshape(-1))
            assert pos[-1].size == 2 * s.size and fl[-1].size == s.size
            cnt.append(s.size)
        cat = lambda a: np.ascontiguousarray(np.concatenate(a)) if a else np.zeros(1)
        pos, sg, fl = cat(pos), cat(sg), cat(fl)
        integ, tf = np.zeros(max(sum(cnt), 1)), self._per_member(time_factor)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        check(capi.lib().suhmo_batch_moulin_source(self.batch.h, (C.c_int * self.n)(*cnt), dp(pos), dp(sg), dp(fl), dp(tf), dp(integ), self._active(active),
                                                   self.batch.stream))
        off = np.concatenate([[0], np.cumsum(cnt)])
        return [integ[off[k]:off[k + 1]].copy() if on[k] else None for k in range(self.n)]

    def _postproc_all(self, fn, shape, active, out):
        t = np.zeros((self.n,) + shape) if out is None else out
        assert t.shape == (self.n,) + shape and t.dtype == np.float64 and t.flags.c_contiguous
        check(fn(self.batch.h, self._mp, t.ctypes.data_as(C.POINTER(C.c_double)), self._active(active), self.batch.stream))
        return t

    def postproc_partial_all(self, active=None, out=None):
        """column sums of every member, (n, 8, nx); out: an array whose rows of the members that are not active are kept"""
        return self._postproc_all(capi.lib().suhmo_batch_postproc_partial, (8, self.nx), active, out)

    def postproc_temporal_all(self, active=None, out=None):
        """the daily row of every member, (n, 6)"""
        return self._postproc_all(capi.lib().suhmo_batch_postproc_temporal, (6,), active, out)

    def postproc_table_device_all(self, active=None, out=None):
        """the SHMIP cross-section table of every member, (n, nx, 8)"""
        return self._postproc_all(capi.lib().suhmo_batch_postproc_table, (self.nx, 8), active, out)

    def mass_balance_all(self, active=None, out=None):
        """the mass balance of every member (suhmo_batch_mass_balance), (n, 7) in the order of capi.MB_NAMES: one first stage, one final launch
        and one read-back for all of them, every member bit for bit HipModel.mass_balance of the same model alone; out: an array whose rows of
        the members that are not active are kept.  Read-only"""
        t = np.zeros((self.n, len(capi.MB_NAMES))) if out is None else out
        assert t.shape == (self.n, len(capi.MB_NAMES)) and t.dtype == np.float64 and t.flags.c_contiguous
        check(capi.lib().suhmo_batch_mass_balance(self.batch.h, t.ctypes.data_as(C.POINTER(C.c_double)), self._active(active), self.batch.stream))
        return t

    def water_budget_all(self, active=None, out=None):
        """the water budget of every member (suhmo_batch_water_budget), (n, 10) in the order of capi.WB_NAMES, every member bit for bit
        HipModel.water_budget of the same model alone; volume_old: what the last step with batch option track_old_volume = 1 that served the
        member started from (NaN: none); out: an array whose rows of the members that are not active are kept.  Read-only"""
        t = np.zeros((self.n, len(capi.WB_NAMES))) if out is None else out
        assert t.shape == (self.n, len(capi.WB_NAMES)) and t.dtype == np.float64 and t.flags.c_contiguous
        check(capi.lib().suhmo_batch_water_budget(self.batch.h, self._mp, t.ctypes.data_as(C.POINTER(C.c_double)), self._active(active), self.batch.stream))
        return t

    def run(self, n_steps, dt, T_K=None, background=None, moulins=None, moulin_factor=None, ramp=None, diag_every=0, active=None, rows=None,
            balance_every=0, budget=None):
        """the time loop of the active members in ONE call (suhmo_batch_run): per step the forcing of the schedule, the time step and, after
        every diag_every-th step, the daily row finished on the device; the rows of the whole run come back in one copy.  Bit for bit what
        time_varying_recharge / moulin_source, timestep and postproc_temporal_all give step by step.
        T_K, background: (n_steps, n), or anything that broadcasts to it (a column per step, a scalar): the seasonal recharge, VALUES -- the
        caller evaluates the temperature.  moulins: lists[k] = (positions, sigma, flux) as moulin_source takes them, given once, with
        moulin_factor (n_steps, n).  ramp: (n_steps,), written into every member's ramp for that step.  rows: an (n_rows, n, 6) array whose
        entries of the members that are not active are kept.
        balance_every > 0 (suhmo_batch_run_bud): the water budget of the active members after every balance_every-th step, finished on the
        device, one more copy for the run -> self.last_run["budget"], (n_steps // balance_every, n, 10) prefilled with NaN (budget: an array
        of that shape to fill instead); self.last_run also holds steps_done and budget_rows.
        Returns (picard iterations (n_steps, n), V-cycles (n_steps, n), rows (n_steps // diag_every, n, 6))."""
        n = self.n
        n_steps, diag_every = int(n_steps), int(diag_every)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        keep = []                                              # the arrays the schedule points into

        def table(x, what):
            a = np.asarray(x, dtype=np.float64)
            if a.ndim == 2 and a.shape != (max(n_steps, 0), n):
                raise ValueError("%s has shape %s, the run needs (n_steps, n) = (%d, %d)" % (what, a.shape, n_steps, n))
            a = np.ascontiguousarray(np.broadcast_to(a, (max(n_steps, 0), n)))
            keep.append(a)
            return dp(a)

        sch = capi.BatchSchedule(n_steps=n_steps, dt=float(dt), first_cur_step=self.cur_step + 1, n_members=n, diag_every=diag_every)
        if (T_K is None) != (background is None):
            raise ValueError("the seasonal recharge needs T_K and background")
        if T_K is not None:
            sch.T_K, sch.background = table(T_K, "T_K"), table(background, "background")
        if (moulins is None) != (moulin_factor is None):
            raise ValueError("a moulin schedule needs moulins and moulin_factor")
        if moulins is not None:
            on = [True] * n if active is None else [bool(x) for x in active]
            if len(moulins) != n:
                raise ValueError("moulins has %d lists, the batch %d members" % (len(moulins), n))
            pos, sg, fl, cnt = [], [], [], []
            for k in range(n):
                if moulins[k] is None:
                    assert not on[k], "member %d is active and has no moulin list" % k
                    cnt.append(0)
                    continue
                sgk = np.asarray(moulins[k][1], dtype=np.float64).reshape(-1)
                pos.append(np.asarray(moulins[k][0], dtype=np.float64).reshape(-1)); sg.append(sgk); fl.append(np.asarray(moulins[k][2], dtype=np.float64).reshape(-1))
                assert pos[-1].size == 2 * sgk.size and fl[-1].size == sgk.size
                cnt.append(sgk.size)
            cat = lambda a: np.ascontiguousarray(np.concatenate(a)) if a and sum(x.size for x in a) else np.zeros(1)
            pos, sg, fl, cnt = cat(pos), cat(sg), cat(fl), (C.c_int * n)(*cnt)
            keep += [pos, sg, fl, cnt]
            sch.n_moulins, sch.positions, sch.sigma, sch.flux, sch.moulin_factor = cnt, dp(pos), dp(sg), dp(fl), table(moulin_factor, "moulin_factor")
        if ramp is not None:
            r = np.ascontiguousarray(ramp, dtype=np.float64)
            if r.shape != (max(n_steps, 0),):
                raise ValueError("ramp has shape %s, the run needs (n_steps,) = (%d,)" % (r.shape, n_steps))
            keep.append(r)
            sch.ramp = dp(r)
        n_rows = n_steps // diag_every if diag_every > 0 and n_steps > 0 else 0
        out = np.zeros((n_rows, n, 6)) if rows is None else rows
        assert out.shape == (n_rows, n, 6) and out.dtype == np.float64 and out.flags.c_contiguous
        pi, nv = np.zeros((max(n_steps, 0), n), dtype=np.intc), np.zeros((max(n_steps, 0), n), dtype=np.intc)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        res = capi.BatchRunResult(picard_iters=ip(pi), vcycles=ip(nv), rows=dp(out))
        balance_every = int(balance_every)
        if balance_every < 0:
            raise ValueError("balance_every = %d" % balance_every)
        if balance_every:
            wb_rows = n_steps // balance_every if n_steps > 0 else 0
            wb = np.full((wb_rows, n, len(capi.WB_NAMES)), np.nan) if budget is None else budget
            assert wb.shape == (wb_rows, n, len(capi.WB_NAMES)) and wb.dtype == np.float64 and wb.flags.c_contiguous
            bud = capi.RunBudget(every=balance_every, lev_cap=0, rows=dp(wb), nlev=None)
            rc = capi.lib().suhmo_batch_run_bud(self.batch.h, self._mp, C.byref(sch), self._active(active), C.byref(bud), C.byref(res), self.batch.stream)
            self.last_run = dict(steps_done=int(res.steps_done), budget=wb[:bud.n_rows], budget_rows=int(bud.n_rows))
        else:
            rc = capi.lib().suhmo_batch_run(self.batch.h, self._mp, C.byref(sch), self._active(active), C.byref(res), self.batch.stream)
            self.last_run = dict(steps_done=int(res.steps_done))
        self.cur_step += res.steps_done
        for m in self.members:
            m.cur_step = self.cur_step
        if ramp is not None and res.steps_done > 0:            # the members' ramp is the last step's, as a loop of set_model leaves it
            for k in range(n):
                self.set_model(k, ramp=float(r[res.steps_done - 1]))
        check(rc)
        return pi, nv, out

    def get_option(self, key):
        return self.batch.get_option(key)

    def set_option(self, key, value):
        self.batch.set_option(key, value)

    def close(self):
        self.batch.close()


class HipAmrModel:
    """The time loop on a hierarchy (base level + nested patches, patches[k] = box of level k+1 in the cells of level k):
    suhmo_amr_timestep over the array of level handles; head and gap height of every level stay in HBM."""

    FIELDS = HipModel.FIELDS

    def __init__(self, nx0, ny0, dx0, dy0, bc, phys, model, patches, max_box=64, device=0):
        self.amr = lv.HipAmr(nx0, ny0, dx0, dy0, bc, phys, patches, alpha=0.0, beta=-1.0, max_box=max_box, device=device)
        self.levels = self.amr.levels
        self.model = dict(model)
        self._mp = model_params(model)
        self.cur_step = 0

    def set_state(self, l, f):
        """f: dict with ghosted arrays head, B, Pi, zb, mask of level l (coarse-fine ghost cells: anything, they are interpolated)"""
        L = self.levels[l]
        L.set(lv.F_PHI, f["head"][1:-1, 1:-1])
        L.set(lv.F_ACOEF, np.zeros((L.ny, L.nx)))
        for k, fid in (("B", lv.F_B), ("Pi", lv.F_PI), ("zb", lv.F_ZB), ("mask", lv.F_MASK)):
            L.set(fid, f[k], ghosted=True)

    def timestep(self, dt):
        self.cur_step += 1
        pi, nv = C.c_int(), C.c_int()
        check(capi.lib().suhmo_amr_timestep(self.amr._arr, len(self.levels), C.byref(self._mp), float(dt), self.cur_step,
                                            C.byref(pi), C.byref(nv), self.amr.stream))
        return pi.value, nv.value

    def moulin_source(self, positions, sigma, flux, time_factor=1.0):
        """Calc_moulin_integral over the hierarchy + the source term of every level (suhmo_amr_moulin_source)"""
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1)
        sg, fl = np.ascontiguousarray(sigma, dtype=np.float64), np.ascontiguousarray(flux, dtype=np.float64)
        integ = np.zeros(sg.size)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        check(capi.lib().suhmo_amr_moulin_source(self.amr._arr, len(self.levels), None, sg.size, dp(pos), dp(sg), dp(fl), float(time_factor),
                                                 dp(integ), self.amr.stream))
        return integ

    def get(self, l, name, ghosted=False):
        return self.levels[l].get(self.FIELDS[name], ghosted=ghosted)

    def close(self):
        self.amr.close()


class HipHierModel:
    """The time loop on a hierarchy whose levels are unions of boxes (boxes[l-1] = list of (lo0, lo1, hi0, hi1) in the index
    space of level l): suhmo_hier_timestep / suhmo_hier_moulin_source; head and gap height of every box stay in HBM."""

    FIELDS = HipModel.FIELDS

    def __init__(self, nx0, ny0, dx0, dy0, bc, phys, model, boxes, max_box=64, device=0, j0=0, ny_global=None, halo_rows=1, options=None):
        self.hier = lv.HipHier(nx0, ny0, dx0, dy0, bc, phys, boxes, alpha=0.0, beta=-1.0, max_box=max_box, device=device,
                               j0=j0, ny_global=ny_global, halo_rows=halo_rows, options=options)
        self.level = self.hier.level
        self.model = dict(model)
        self._mp = model_params(model)
        self.cur_step = 0

    def set_state(self, l, k, f):
        """f: dict with ghosted arrays head, B, Pi, zb, mask of box k of level l (fine-fine / coarse-fine ghost cells: anything).  On a level dealt
        to the ranks a box this rank does not hold is skipped (its owner loads it); loading a mirror is harmless"""
        if not self.hier.held[l][k]:
            return
        L = self.level[l][k]
        L.set(lv.F_PHI, f["head"][1:-1, 1:-1])
        L.set(lv.F_ACOEF, np.zeros((L.ny, L.nx)))
        for key, fid in (("B", lv.F_B), ("Pi", lv.F_PI), ("zb", lv.F_ZB), ("mask", lv.F_MASK)):
            L.set(fid, f[key], ghosted=True)

    def set_states(self, sts):
        for l, bl in enumerate(sts):
            for k, st in enumerate(bl):
                self.set_state(l, k, st)

    def init_ibc(self, ibc):
        """the initial state of every box of every level evaluated on the device (suhmo_hier_ibc_init): one launch per level, then the
        ghost fills of initData; nothing is loaded from the host"""
        check(capi.lib().suhmo_hier_ibc_init(self.hier.h, C.byref(ibc) if ibc is not None else None, self.hier.stream))

    def set_ibc(self, ibc):
        """keep `ibc` on the hierarchy (suhmo_hier_set_ibc; None clears it): regrid, tag_and_regrid and run then evaluate initializeBed /
        initializePi / setup_iceMask on every new level on the device, inside the regrid, and `reload` may stay None"""
        check(capi.lib().suhmo_hier_set_ibc(self.hier.h, C.byref(ibc) if ibc is not None else None))

    def ibc_reload(self, level):
        """suhmo_hier_ibc_reload: the reload of one level >= 1 with the IBC set_ibc left (what regrid does per new level)"""
        check(capi.lib().suhmo_hier_ibc_reload(self.hier.h, int(level), self.hier.stream))

    def timestep(self, dt):
        self.cur_step += 1
        pi, nv = C.c_int(), C.c_int()
        check(capi.lib().suhmo_hier_timestep(self.hier.h, C.byref(self._mp), float(dt), self.cur_step, C.byref(pi), C.byref(nv),
                                             self.hier.stream))
        return pi.value, nv.value

    def moulin_source(self, positions, sigma, flux, time_factor=1.0):
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1)
        sg, fl = np.ascontiguousarray(sigma, dtype=np.float64), np.ascontiguousarray(flux, dtype=np.float64)
        integ = np.zeros(sg.size)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        check(capi.lib().suhmo_hier_moulin_source(self.hier.h, sg.size, dp(pos), dp(sg), dp(fl), float(time_factor), dp(integ), self.hier.stream))
        return integ

    def tag_cells(self, level, name, vmin, vmax, grow=0, grow_dir=(0, 0), granularity=1):
        """tagCellsLevel on every box of `level` (suhmo_hier_tag_cells) into the level's tag map; granularity = block_factor / 2 of the
        generate_grids call that is to read it"""
        check(capi.lib().suhmo_hier_tag_cells(self.hier.h, int(level), _tag_field(self.FIELDS, name), float(vmin), float(vmax),
                                              *_tag_reach(grow, grow_dir), int(granularity), self.hier.stream))

    def clear_tags(self, level=-1):
        """empty the tag map of `level` (default: of every level)"""
        check(capi.lib().suhmo_hier_clear_tags(self.hier.h, int(level)))

    def tags(self, level):
        """the tag map of `level`, (nby, nbx) uint8; None where there is none"""
        return _tags_out(capi.lib().suhmo_hier_get_tags, self.hier.h, int(level))

    def generate_grids(self, fill_ratio, block_factor, max_box_size, nesting_radius=2):
        """suhmo_hier_generate_grids: box lists from the tag maps of the levels 0, 1, ... that have one -> (boxes, same); boxes in the form the
        constructor takes, same: they are this hierarchy's own, level by level, in any order (the reference's gridsSame)"""
        gp = capi.GridParams(float(fill_ratio), int(block_factor), int(max_box_size), int(nesting_radius))
        same = C.c_int()
        boxes = _generate(lambda nlev, nbox, flat, cap: capi.lib().suhmo_hier_generate_grids(self.hier.h, C.byref(gp), nlev, nbox, flat, cap, C.byref(same)),
                          self.hier.nlev)
        return boxes, bool(same.value)

    def regrid(self, boxes, reload=None, fields=None):
        """AmrHydro::regrid's third step (destructiveRegrid, src/AmrHydro.cpp:4176-4223, 4363-4437) on the device, suhmo_hier_regrid: the
        hierarchy moves onto `boxes` (the form the constructor and generate_grids use; [] = level 0 alone) between two time steps.  Per new
        level, ascending: every cell interpolated from the new level below (FineInterp, limited slopes), then overwritten bit for bit where an
        old box of the level held it; ghost cells refilled.  fields: names of FIELDS (or ids); None = head, B, Pi, zb, mask, mR, Pw, zs.
        Every other field of the levels >= 1 starts as in a new hierarchy (the next moulin_source / timestep recomputes them); level 0, the
        model parameters and cur_step stay.  self.hier wraps the new handle afterwards and self.level holds the new boxes' views.
        reload(l, k, box) -> dict as set_state takes it, possibly partial (head, B, Pi, zb, mask: ghosted arrays of the box), or None: called
        for every new box after the transfer and loaded over the transferred values -- the place of initializeBed / initializePi /
        setup_iceMask (:4387-4437).  With an IBC on the hierarchy (set_ibc) that evaluation has already run on the device, inside the regrid; a reload that is given runs after it.
        THE MASK: a transferred ice mask is INTERPOLATED and therefore not +-1 along an ice margin.  The reference does not keep it either:
        it recomputes the mask from Pi after every regrid (setup_iceMask, :4436).  A caller whose domain has a margin must do the same in
        `reload` (return "mask" for every box); where the mask is +1 everywhere the transferred one is exact.
        A list that suhmo_hier_create would refuse (nesting, alignment) raises SuhmoError with its return code and leaves the model as it was."""
        ids = None if fields is None else [f if isinstance(f, int) else (lv.F_ZS if f == "zs" else self.FIELDS[f]) for f in fields]
        self.hier.regrid(boxes, ids)
        self.level = self.hier.level
        if reload is not None:
            for l, bl in enumerate(self.hier.boxes, start=1):
                for k, b in enumerate(bl):
                    f = reload(l, k, b)
                    if f:
                        self._load(l, k, f)

    def _load(self, l, k, f):
        L = self.level[l][k]
        if "head" in f:
            L.set(lv.F_PHI, f["head"][1:-1, 1:-1])
        for key, fid in (("B", lv.F_B), ("Pi", lv.F_PI), ("zb", lv.F_ZB), ("mask", lv.F_MASK), ("zs", lv.F_ZS)):
            if key in f:
                L.set(fid, f[key], ghosted=True)

    def tag_and_regrid(self, tag_specs, params, reload=None, subsets=None, max_level=None, fields=None):
        """The body of AmrHydro::regrid (src/AmrHydro.cpp:4227-4511): the tag maps are emptied, every tag variable of tag_specs (dicts of
        tag_cells' arguments without the level: name, vmin, vmax, grow, grow_dir; and min_level, cap_level: the levels it tags, default all)
        tags the levels max(min_level, 0) .. min(cap_level, max_level - 1, finest level) (tagCells, :4514-4536), each followed by
        restrict_tags with subsets[l] where that list is not empty (subsets: per level, level 0 first, nested: nest_tag_subsets); grids are
        generated with params (generate_grids' keywords) and, when they are not the hierarchy's own (gridsSame), the fields move onto them
        (regrid).  Returns (boxes, same); with same = True the handle is not touched."""
        g = int(params["block_factor"]) // 2
        self.clear_tags()
        for sp in tag_specs:
            sp = dict(sp)
            lo, cap = max(int(sp.pop("min_level", 0)), 0), sp.pop("cap_level", None)
            top = min(self.hier.nlev - 1, (ALL_LEVELS if max_level is None else int(max_level)) - 1)
            top = top if cap is None else min(top, int(cap))
            for l in range(lo, top + 1):
                self.tag_cells(l, granularity=g, **sp)
                if subsets is not None and l < len(subsets) and subsets[l]:
                    self.restrict_tags(l, subsets[l])
        boxes, same = self.generate_grids(**params)
        if not same:
            self.regrid(boxes, reload=reload, fields=fields)
        return boxes, same

    # the reference's two plotted components (src/AmrHydro.cpp:4672-4677): the gap height, and N = Pi - Pw formed BEFORE the interpolation
    PP_COMPONENTS = [("gapHeight", (capi.FLAT_FIELD, lv.F_B)), ("N", (capi.FLAT_DIFF, lv.F_PI, lv.F_PW))]

    def interp_finest(self, max_level=None):
        """AmrHydro::interpFinest (src/AmrHydro.cpp:4623-4829) on the device, suhmo_hier_flatten: gap height and effective pressure of the whole
        hierarchy on the uniform grid of level max_level (None: the finest level) -> dict(gapHeight=, N=), each (ny0 << max_level,
        nx0 << max_level).  Read-only."""
        a = self.hier.flatten([c for _, c in self.PP_COMPONENTS], max_level)
        return {nm: a[q] for q, (nm, _) in enumerate(self.PP_COMPONENTS)}

    # the fields of the reference's convergence tables (CONV_ANA/scripts/launch_comparaison*.py: head, gapHeight, Pw, Re, N)
    CMP_COMPONENTS = [("head", (capi.FLAT_FIELD, lv.F_PHI)), ("gapHeight", (capi.FLAT_FIELD, lv.F_B)), ("Pw", (capi.FLAT_FIELD, lv.F_PW)),
                      ("Re", (capi.FLAT_FIELD, lv.F_RE)), ("N", (capi.FLAT_DIFF, lv.F_PI, lv.F_PW))]

    def compare(self, exact_model, exact_level=None, mode="composite"):
        """suhmo_hier_compare against a single-level model (HipModel) on the uniform grid of level exact_level (None: the one its width gives):
        -> dict(head=, gapHeight=, Pw=, Re=, N=) of (L1, L2, max) arrays.  Read-only; nothing but the norms leaves the device"""
        if exact_level is None:
            exact_level = (exact_model.nx // self.level[0][0].nx).bit_length() - 1
        a = self.hier.compare(exact_model.level, [c for _, c in self.CMP_COMPONENTS], exact_level, mode)
        return {nm: a[q] for q, (nm, _) in enumerate(self.CMP_COMPONENTS)}

    def mass_balance(self):
        """AmrHydro::check_fluxes of every level, reduced on the device (suhmo_hier_mass_balance): a list of dicts of the seven names
        (capi.MB_NAMES), level 0 first; every level is summed whole, as the reference does.  A first stage per level, one final launch, one
        copy of 7 nlev doubles.  Read-only"""
        out = np.zeros((self.hier.nlev, len(capi.MB_NAMES)))
        check(capi.lib().suhmo_hier_mass_balance(self.hier.h, out.ctypes.data_as(C.POINTER(C.c_double)), self.hier.stream))
        return [dict(zip(capi.MB_NAMES, row.tolist())) for row in out]

    def water_budget(self):
        """the conservation record of a step, per level (suhmo_hier_water_budget; include/suhmo_hip.h, "WATER BUDGET"): a list of dicts of the
        ten names (capi.WB_NAMES), level 0 first -- the seven values of mass_balance, volume_old (the volume the last step with hierarchy
        option track_old_volume = 1 started from; NaN: none, as on every level after a regrid), the two parts of rechargeTOT.  A first
        stage per level, one final launch, one copy of 10 nlev doubles.  Read-only"""
        out = np.zeros((self.hier.nlev, len(capi.WB_NAMES)))
        check(capi.lib().suhmo_hier_water_budget(self.hier.h, C.byref(self._mp), out.ctypes.data_as(C.POINTER(C.c_double)), self.hier.stream))
        return [dict(zip(capi.WB_NAMES, row.tolist())) for row in out]

    def restrict_tags(self, level, boxes):
        """levelTags &= tagSubset (suhmo_hier_restrict_tags): every entry of the tag map of `level` that lies in none of `boxes`
        ((lo0, lo1, hi0, hi1) in cells of that level, aligned to the map's granularity) is cleared; an empty list is a no-op"""
        boxes = [tuple(int(v) for v in b) for b in boxes]
        _, flat = _flat_boxes([boxes])
        check(capi.lib().suhmo_hier_restrict_tags(self.hier.h, int(level), len(boxes), flat, self.hier.stream))

    def set_surface(self, l, k, zs):
        """the ghosted ice surface height of box k of level l (F_ZS): loaded once, it stays on the device for time_varying_recharge"""
        self.level[l][k].set(lv.F_ZS, zs, ghosted=True)

    def time_varying_recharge(self, T_K, background):
        """F_MSRC of every box from its surface height (suhmo_hier_time_varying_recharge): one launch per level"""
        check(capi.lib().suhmo_hier_time_varying_recharge(self.hier.h, float(T_K), float(background), self.hier.stream))

    def postproc_temporal(self):
        """the daily row (6 values) of the run: level 0's, as the reference evaluates it (suhmo_hier_postproc_temporal)"""
        out = np.zeros(6)
        check(capi.lib().suhmo_hier_postproc_temporal(self.hier.h, C.byref(self._mp), out.ctypes.data_as(C.POINTER(C.c_double)), self.hier.stream))
        return out

    def run(self, n_steps, dt, T_K=None, background=None, moulins=None, moulin_factor=None, ramp=None, diag_every=0, regrid_interval=0,
            tag_specs=None, params=None, subsets=None, max_level=None, reload=None, skip_first_regrid=False, fields=None,
            plot_interval=-1, check_interval=-1, plot_prefix="plot", check_prefix="chk", check_overwrite=True, restart_step=0,
            final_output=True, time0=0.0, periodic=(0, 0), balance_every=0):
        """AmrHydro::run in ONE call (suhmo_hier_run): per step the regrid the reference does before it (every regrid_interval steps:
        regrid_steps(self.cur_step + 1, n_steps, regrid_interval, skip_first_regrid) lists them; tag_and_regrid's arguments tag_specs, params,
        subsets, max_level, fields), the forcing, the time step and, after every diag_every-th step, the daily row finished on the device; the
        rows come back in one copy.  Bit for bit what tag_and_regrid, time_varying_recharge / moulin_source, timestep and postproc_temporal
        give step by step.
        T_K, background: (n_steps,) or scalars, VALUES: the seasonal recharge of every step.  moulins: dict or tuple of positions, sigma, flux,
        given once; moulin_factor (n_steps,) or None (1.0): the moulin source is formed at the first step, after a regrid that moved boxes
        and where the factor's bits differ from the step before.  ramp: (n_steps,).
        reload(l, k, box) -> dict as regrid's reload (and "zs": the ghosted surface height): called for every box of the new hierarchy after a
        regrid that moved boxes; an exception it raises ends the run and is raised again after the bookkeeping.
        With T_K the surface height (set_surface) must reach the new boxes of every such regrid: fields = None or a list with "zs" transfers
        it, or reload returns "zs" for EVERY box.  Otherwise the run ends at that regrid with SuhmoError rc -1 naming the box, before anything
        is launched on the new hierarchy; the steps before it are done, the model wraps the new hierarchy and goes on once the surface is loaded.
        OUTPUT (suhmo_hier_run_out; output_steps lists the events): plot_interval / check_interval as the reference's (-1: none of that kind, 0:
        only the file after the last step), restart_step, final_output=False for a run that another run continues.  Every event is one
        snapshot on the device and one file: plotfile's thirteen components into plot_prefix + "%06d.2d.hdf5" % cur_step, the checkpoint's
        datasets into check_prefix + ".2d.hdf5" (check_overwrite) or check_prefix + "%06d.2d.hdf5" (:5634, :5680-5691); the file's time is
        time0 + steps done x dt, `periodic` goes into the checkpoint's header.  An exception raised while writing ends the run and is raised
        again after the bookkeeping, as for reload.
        Returns (picard iterations (n_steps,), V-cycles (n_steps,), rows (n_steps // diag_every, 6), log) with log = one dict per regrid:
        cur_step, same, boxes_per_level.  self.last_run: steps_done, n_rows, moulin_steps (n_steps,), plots and checkpoints (the paths
        written, in order).  balance_every > 0 (suhmo_hier_run_bud): the water budget of every level after every balance_every-th step,
        finished on the device, one more copy for the run: self.last_run["budget"], (rows, lev_cap, 10) prefilled with NaN (lev_cap:
        max_level + 1 when the run regrids, else the levels it has), and ["budget_nlev"], the levels at each row.  cur_step advances by the steps done;
        after a regrid that moved boxes self.hier wraps the new handle and self.level holds the new boxes' views."""
        n_steps, diag_every = int(n_steps), int(diag_every)
        ns = max(n_steps, 0)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        keep = []

        def per_step(x, what):
            a = np.asarray(x, dtype=np.float64)
            if a.ndim == 1 and a.shape != (ns,):
                raise ValueError("%s has shape %s, the run needs (n_steps,) = (%d,)" % (what, a.shape, ns))
            a = np.ascontiguousarray(np.broadcast_to(a, (ns,)))
            keep.append(a)
            return dp(a)

        sch = capi.HierSchedule(n_steps=n_steps, dt=float(dt), first_cur_step=self.cur_step + 1, diag_every=diag_every,
                                regrid_interval=int(regrid_interval), skip_first_regrid=int(bool(skip_first_regrid)),
                                max_level=ALL_LEVELS if max_level is None else int(max_level))
        if (T_K is None) != (background is None):
            raise ValueError("the seasonal recharge needs T_K and background")
        if T_K is not None:
            sch.T_K, sch.background = per_step(T_K, "T_K"), per_step(background, "background")
        if moulins is None and moulin_factor is not None:
            raise ValueError("moulin_factor without moulins")
        if moulins is not None:
            pos, sg, fl = (moulins[q] for q in ("positions", "sigma", "flux")) if isinstance(moulins, dict) else moulins
            pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1)
            sg, fl = np.ascontiguousarray(sg, dtype=np.float64).reshape(-1), np.ascontiguousarray(fl, dtype=np.float64).reshape(-1)
            assert pos.size == 2 * sg.size and fl.size == sg.size
            keep += [pos, sg, fl]
            sch.n_moulins, sch.positions, sch.sigma, sch.flux = sg.size, dp(pos), dp(sg), dp(fl)
            if moulin_factor is not None:
                sch.moulin_factor = per_step(moulin_factor, "moulin_factor")
        if ramp is not None:
            r = np.ascontiguousarray(ramp, dtype=np.float64)
            if r.shape != (ns,):
                raise ValueError("ramp has shape %s, the run needs (n_steps,) = (%d,)" % (r.shape, ns))
            keep.append(r)
            sch.ramp = dp(r)
        if tag_specs:
            tg = (capi.TagSpec * len(tag_specs))()
            for q, sp in enumerate(tag_specs):
                cap = sp.get("cap_level")
                tg[q] = capi.TagSpec(_tag_field(self.FIELDS, sp["name"]), float(sp["vmin"]), float(sp["vmax"]),
                                     *_tag_reach(sp.get("grow", 0), sp.get("grow_dir", (0, 0))), int(sp.get("min_level", 0)),
                                     2 ** 30 if cap is None else int(cap))
            keep.append(tg)
            sch.n_tags, sch.tags = len(tag_specs), tg
        if params is not None:
            sch.grid = capi.GridParams(float(params["fill_ratio"]), int(params["block_factor"]), int(params["max_box_size"]),
                                       int(params.get("nesting_radius", 2)))
        if subsets is not None:
            per = [list(subsets[l]) if l < len(subsets) else [] for l in range(max(sch.max_level, 1))]
            nb, flat = _flat_boxes(per)
            keep += [nb, flat]
            sch.subset_nbox, sch.subset_boxes = nb, flat
        if fields is not None:
            ids = (C.c_int * max(len(fields), 1))(*[f if isinstance(f, int) else (lv.F_ZS if f == "zs" else self.FIELDS[f]) for f in fields])
            keep.append(ids)
            sch.n_fields, sch.fields = len(fields), ids
        raised = []

        def on_regrid(user, hnew, index, cur_step):
            try:
                self.hier._adopt(hnew)
                self.level = self.hier.level
                if reload is not None:
                    for l, bl in enumerate(self.hier.boxes, start=1):
                        for k, b in enumerate(bl):
                            f = reload(l, k, b)
                            if f:
                                self._load(l, k, f)
                return 0
            except BaseException as e:           # (an exception must not travel through the C frames)
                raised.append(e)
                return 1

        cb = capi.RELOAD_FN(on_regrid)
        sch.reload = cb
        out, written = None, ([], [])
        if plot_interval != -1 or check_interval != -1:
            from . import checkpoint, plotfile
            const = checkpoint.constants(self.model)
            chk_comps = checkpoint.snapshot_components(const)[0]
            first = self.cur_step

            def on_output(user, h, kind, cur_step, ncomp, level_offset, box_offset, data):
                try:
                    self.hier._adopt_if_new(h)
                    self.level = self.hier.level
                    nbox = [len(bl) for bl in self.level]
                    lo = np.array(level_offset[:self.hier.nlev + 1], dtype=np.int64)
                    bo = lv.split_box_offsets(box_offset, nbox)
                    flat = np.ctypeslib.as_array(data, shape=(int(lo[-1]),))           # the run's pinned buffer: valid during this call
                    time = float(time0) + (cur_step - first) * float(dt)
                    if kind == PLOT:
                        path = "%s%06d.2d.hdf5" % (plot_prefix, cur_step)
                        plotfile.write_levels(path, plotfile.NAMES, plotfile.levels_of_snapshot(self, lo, bo, flat), time)
                    else:
                        path = "%s.2d.hdf5" % check_prefix if check_overwrite else "%s%06d.2d.hdf5" % (check_prefix, cur_step)
                        checkpoint.write(path, self, time, float(dt), periodic, snapshot=(lo, bo, flat), step=cur_step)
                    written[kind].append(path)
                    return 0
                except BaseException as e:
                    raised.append(e)
                    return 1

            pc, cc = capi.snap_comps(plotfile.SNAP), capi.snap_comps(chk_comps)
            ocb = capi.OUTPUT_FN(on_output)
            keep += [pc, cc, ocb]
            out = capi.HierOutput(int(plot_interval), int(check_interval), int(restart_step), int(not final_output), len(plotfile.SNAP), pc,
                                  len(chk_comps), cc, ocb, None)
        n_rows = n_steps // diag_every if diag_every > 0 and n_steps > 0 else 0
        rows = np.zeros((n_rows, 6))
        pi, nv, ms = np.zeros(ns, dtype=np.intc), np.zeros(ns, dtype=np.intc), np.zeros(ns, dtype=np.intc)
        log = (capi.HierRegridLog * max(ns, 1))()
        res = capi.HierRunResult(picard_iters=ip(pi), vcycles=ip(nv), rows=dp(rows) if n_rows else None, moulin_steps=ip(ms), regrids_cap=max(ns, 1),
                                 regrids=log)
        balance_every, bud = int(balance_every), None
        if balance_every < 0:
            raise ValueError("balance_every = %d" % balance_every)
        if balance_every:
            wb_rows = n_steps // balance_every if n_steps > 0 else 0
            lev_cap = max(self.hier.nlev, min(sch.max_level + 1, 8) if regrid_interval > 0 else 0)      # (a hierarchy has at most 8 levels)
            wb, wb_nlev = np.full((wb_rows, lev_cap, len(capi.WB_NAMES)), np.nan), np.zeros(max(wb_rows, 1), dtype=np.intc)
            bud = capi.RunBudget(every=balance_every, lev_cap=lev_cap, rows=dp(wb), nlev=ip(wb_nlev))
        rc = self.hier.run(self._mp, sch, res, out, bud)
        self.level = self.hier.level
        self.cur_step += res.steps_done
        if ramp is not None and res.steps_done > 0:            # the model's ramp is the last step's, as a loop that sets it leaves it
            self._mp.ramp = float(r[res.steps_done - 1])
        self.last_run = dict(steps_done=int(res.steps_done), n_rows=int(res.n_rows), moulin_steps=ms, n_moved=int(res.n_moved),
                             plots=written[0], checkpoints=written[1])
        if bud is not None:
            self.last_run.update(budget=wb[:bud.n_rows], budget_nlev=wb_nlev[:bud.n_rows].astype(int))
        if raised:
            raise raised[0]
        check(rc)
        return pi, nv, rows[:res.n_rows], [dict(cur_step=int(e.cur_step), same=bool(e.same), boxes_per_level=[int(e.nbox[l]) for l in range(1, e.nlev)])
                                            for e in log[:res.n_regrids]]

    def get(self, l, k, name, ghosted=False):
        """a field of box k of level l; None where another rank owns the box (levels dealt to the ranks: hier.owns(l, k))"""
        if not self.hier.owns(l, k):
            return None
        return self.level[l][k].get(self.FIELDS[name], ghosted=ghosted)

    def postproc_table_device(self):
        """SHMIP cross-section table of a run with AMR levels: the reference evaluates it on LEVEL 0 ("POST PROC -- 1 LEVEL",
        m_amrGrids[0], src/AmrHydro.cpp:3643-3700; the finer levels enter through the averaged-down head, CoarseAverage :3138-3141) --
        suhmo_level_postproc_table on the base handle of the hierarchy (whole level 0; on rank strips: postproc_partial per rank)"""
        base = self.level[0][0]
        t = np.zeros((base.nx, 8))
        check(capi.lib().suhmo_level_postproc_table(base.h, C.byref(self._mp), t.ctypes.data_as(C.POINTER(C.c_double)), self.hier.stream))
        return t

    def close(self):
        self.hier.close()
