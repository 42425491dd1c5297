"""The time step swept over its data-dependent branches: cases, seeded inputs and a census of the branches, for tests/test_step_sweep_cpu.py (the
oracle alone) and tests/test_gpu_step_sweep.py (the device against the oracle, bitwise).  A plain helper module like tests/hierlayouts.py; numpy only,
nothing here touches the device library.

Single-level cases = SHAPES x BCS x ROWS; hierarchy cases = the layouts of tests/hierlayouts.py whose fine ghost cells across a periodic side are all
held by a box of their level (hierarchy_layouts) x HIER_MODELS.  plant() puts the values at which the per-cell kernels of suhmo_step.hip branch into a
few percent of the cells of a smooth state; census() restates the branch predicates in numpy, from the state entering a step and the fields the ORACLE
left after it, with the expressions of oracle/time_loop.c, and says per branch which cells (or faces) took which arm."""
import numpy as np

from suhmo_amd import synthetic as sy
from tests import hierlayouts as hl

# nx x ny of the single-level cases (the per-cell kernels run in workgroups of 64 x 4 threads)
SHAPES = (
    (12, 4),       # fewer cells than one workgroup: every launch is one partial workgroup, the Picard maxima come from a single block
    (40, 24),      # a partial workgroup in x (40 < 64), six rows of workgroups in y
    (72, 20),      # one full workgroup plus a partial one in x (72 = 64 + 8), an odd number (5) of workgroup rows in y
    (24, 36),      # the same transposed: partial in x, an odd number (9) of workgroup rows in y
)
DIRICHLET_BC = dict(type=[[0, 0], [1, 1]], value=[[2.0, 900.0], [0.0, 0.0]], periodic=[0, 0])     # tests/test_gpu_timestep.py "dirichlet-values"
X_PERIODIC_BC = dict(type=[[1, 1], [0, 1]], value=[[0.0, 0.0], [0.0, 0.0]], periodic=[1, 0])       # the margin (Dirichlet 0) on y-lo
XY_PERIODIC_BC = dict(type=[[0, 0], [0, 0]], value=[[0.0, 0.0], [0.0, 0.0]], periodic=[1, 1])
BCS = dict([("a3", sy.A3_BC), ("y-periodic", sy.CONV_BC), ("x-periodic", X_PERIODIC_BC), ("xy-periodic", XY_PERIODIC_BC), ("dirichlet", DIRICHLET_BC)])

DT = 60.0
PHYS = dict(sy.A3_PHYS, use_mask_gradients=1, cutOffB=1, cutOffbr=0.02, maxOffbr=0.08)
# dt: at SHMIP's 3600 s the creep closure A N^3 b dt under thick ice exceeds b, the forward Euler step leaves negative gap heights and the second
# step's head solves run into max_iter
_COMMON = dict(use_mask_rhs_b=1, G=0.05, dt=DT)
ROWS = dict([
    ("explicit", dict(_COMMON)),
    ("explicit-diffusion", dict(_COMMON, diffFactor=1.0)),
    ("implicit", dict(_COMMON, diffFactor=1.0, use_impl_diff=1)),
    ("implicit-half-freeze-nomelt", dict(_COMMON, diffFactor=0.5, use_impl_diff=1, freeze_icefree_gap=1, head_melt_off=1)),
    ("no-friction-unmasked-rhs", dict(basal_friction=0, use_mask_rhs_b=0, G=0.0, dt=DT)),
    ("moulin-ramped", dict(_COMMON, use_moulin_source=1, ramp=0.5, distributed_input=7.93e-11)),
    # a geothermal flux large enough (G / L = 0.15 m/s of melt) that gap height x melt rate / rho_i crosses the 5e-6 floor of the diffusion
    # coefficient: with the physical G the floor is taken on every face and its other arm on none.  Not a physical state: a short step keeps the gap
    # height in range, and without head_melt_off the melt's sink in RHS_h (0.15 m/s x (1/rho_w - 1/rho_i)) takes 12 x 4 past 20 Picard iterations
    ("hot-bed-diffusion", dict(_COMMON, G=5.0e4, diffFactor=1.0, dt=2.0, head_melt_off=1)),
])
MOULIN = dict(position=(0.37, 0.55), sigma=0.08, flux=4.0)        # in units of the domain's extent / its smaller extent; one moulin

# (bc, row) combinations left out of the sweep, with the reason; at most one in ten, no whole row, no whole BC (tests/test_step_sweep_cpu.py)
DROPPED = {}

N_STEPS = 2                                                       # the second at half the step size


def single_cases():
    """(case id, nx, ny, bc name, row name) of every single-level case"""
    return [("%dx%d-%s-%s" % (nx, ny, b, r), nx, ny, b, r) for nx, ny in SHAPES for b in BCS for r in ROWS if (b, r) not in DROPPED]


def model_of(row):
    return dict(sy.A3_MODEL, **ROWS[row])


def perturbed_state(nx, ny, seed, mask_holes=False, ly=2.0e4, base=None, head_amp=30.0):
    """a smooth state (default: SHMIP's sqrt ice sheet) with a multiplicative perturbation of the gap height on both sides of br = 0.1 and additive
    ones of head and bed"""
    st = sy.shmip_initial_state(nx, ny, ly=ly) if base is None else base
    rng = np.random.default_rng(seed)
    st["B"] = st["B"] * rng.uniform(0.5, 12.0, size=st["B"].shape)     # both sides of br = 0.1
    st["head"] = st["head"] + rng.uniform(0.0, head_amp, size=st["head"].shape)
    st["zb"] = st["zb"] + rng.uniform(0.0, 2.0, size=st["zb"].shape)
    if mask_holes:
        st["mask"][rng.uniform(size=st["mask"].shape) < 0.05] = -1.0
    return st


HEAD_AMP = 3.0
# Gap heights under the perturbation, tuned on the oracle alone until no head solve of the sweep ends on max_iter (tests/test_step_sweep_cpu.py).
# 0.005 (SHMIP: 0.01): at 72 x 20 the multigrid bottoms out at 9 x 5 cells and the smoothest mode falls by 0.967 per cycle; with b^3 eight times
# smaller its residual is under norm_thresh = 1e-7 within 100 cycles.  The doubly periodic head problem is singular (no Dirichlet side, aCoef = 0):
# its solves stop when the residual that is left sinks under norm_thresh, which happens within 100 cycles at 0.02 on three shapes and at 0.01 on
# 12 x 4 (and not the other way round); the branch-edge values come from plant() either way.
LX = 1.0e5          # extent along the ice sheet's profile; the other extent makes the cells square (at 24 x 36 on SHMIP's 100 km x 20 km the cells are
                    # 7.5 : 1 and the oracle's point relaxation runs most head solves into max_iter)


def base_state(nx, ny, bc):
    """the smooth state under the perturbation.  Not periodic in x: SHMIP's sqrt ice sheet along x (synthetic.shmip_initial_state).  Periodic in x:
    the sheet must not depend on x (wrapped, the sqrt profile jumps by the whole ice thickness across the wrap and the oracle goes to NaN in step
    1) -- x-periodic alone: the same sqrt profile along y, its margin on the Dirichlet side y-lo; doubly periodic: a slab of constant thickness,
    the value of the sqrt profile at mid-length"""
    px, py = bc["periodic"]
    GAP, GAPXY = 0.005, (0.01 if nx * ny < 256 else 0.02)
    if not px:
        return sy.shmip_initial_state(nx, ny, ly=LX * ny / nx, gap_init=GAP)
    if not py:
        with np.errstate(invalid="ignore"):
            t = sy.shmip_initial_state(ny, nx, lx=LX, ly=LX * nx / ny, gap_init=GAP)
        off = np.isnan(t["Pi"])                                  # 4 cells along the profile: the ghost row lies beyond the sqrt's origin -- no ice there
        t["Pi"], t["mask"], t["B"] = np.where(off, 0.0, t["Pi"]), np.where(off, -1.0, t["mask"]), np.where(off, 1.0e-16, t["B"])
        st = dict(nx=nx, ny=ny, dx=t["dy"], dy=t["dx"])
        for k in ("head", "B", "Pi", "zb", "mask"):
            st[k] = np.ascontiguousarray(t[k].T)
        return st
    st = sy.shmip_initial_state(nx, ny, ly=LX * ny / nx)
    with np.errstate(invalid="ignore"):
        mid = sy.shmip_initial_state(3, 1)["Pi"][1, 2]
    st["Pi"] = np.full_like(st["Pi"], mid)
    st["mask"] = np.ones_like(st["mask"])
    st["B"] = np.full_like(st["B"], GAPXY)
    return st


def ulp_set(phys, model):
    """the values at which the kernels branch on the gap height: far below and just below the 1e-6 of the melt rate's clamp, and cutOffbr, maxOffbr
    and br each with the doubles next to them"""
    out = [1.0e-16, 5.0e-7]
    for v in (phys["cutOffbr"], phys["maxOffbr"], model["br"]):
        out += [float(np.nextafter(v, 0.0)), float(v), float(np.nextafter(v, 1.0))]
    return np.array(out)


def plant(st, phys, model, bc, seed, share=0.04, mask_share=0.05, pairs=None):
    """branch-edge values in a few percent of the cells of state st, ghost ring included (drawn cell by cell; every cell drawn from the edge set
    sends every head solve into max_iter): B from ulp_set in `share` of the cells, the mask at -1 in `mask_share`, and `pairs` pairs of neighbouring
    cells of each of four kinds -- masks that differ / both -1, across a domain face (ghost cell and the cell next to it) / inside.  Then the ghost
    cells across periodic sides become the periodic image (synthetic.wrap_ghosts)."""
    rng = np.random.default_rng([int(seed), 7703])
    ny, nx = st["B"].shape[0] - 2, st["B"].shape[1] - 2
    edge = ulp_set(phys, model)
    pairs = (3 if nx * ny >= 256 else 1) if pairs is None else pairs
    hit = np.zeros(st["B"].shape, dtype=bool)
    inside = np.zeros_like(hit)
    inside[1:-1, 1:-1] = True
    for cells, least in ((np.flatnonzero(inside), 4), (np.flatnonzero(~inside), 2)):      # valid cells, then the ghost ring; 12 x 4 gets its few too
        hit.flat[rng.choice(cells, size=max(int(round(share * cells.size)), least), replace=False)] = True
    st["B"] = np.where(hit, edge[rng.integers(0, edge.size, size=st["B"].shape)], st["B"])
    st["mask"] = np.where(rng.random(st["mask"].shape) < mask_share, -1.0, st["mask"])
    two = lambda both, flip: (-1.0, -1.0) if both else ((1.0, -1.0) if flip else (-1.0, 1.0))
    for n in range(pairs):
        kinds = [(place, both) for place in range(4) for both in (False, True)]
        if nx * ny < 256:                                 # 12 x 4: half of the eight kinds, or the pairs alone would mask a third of its 48 cells
            kinds = [kinds[q] for q in sorted(rng.choice(8, size=4, replace=False))]
        for place, both in kinds:
            if place == 0:                                # across the domain face x-lo: ghost column 0 | column 1 of the ghosted array
                j = int(rng.integers(1, ny + 1))
                st["mask"][j, 0], st["mask"][j, 1] = two(both, n & 1)
            elif place == 1:                              # across y-hi
                i = int(rng.integers(1, nx + 1))
                st["mask"][ny + 1, i], st["mask"][ny, i] = two(both, n & 1)
            elif place == 2 and nx > 3 and ny > 3:        # inside, neighbours in x
                j, i = int(rng.integers(2, ny)), int(rng.integers(2, nx - 1))
                st["mask"][j, i], st["mask"][j, i + 1] = two(both, True)
            elif nx > 3 and ny > 3:                       # inside, neighbours in y
                j, i = int(rng.integers(2, ny - 1)), int(rng.integers(2, nx))
                st["mask"][j, i], st["mask"][j + 1, i] = two(both, False)
    for k in ("head", "B", "Pi", "zb", "mask"):
        st[k] = np.ascontiguousarray(st[k], dtype=np.float64)
    return sy.wrap_ghosts(st, bc)


def single_state(nx, ny, bcname, row, seed=11):
    """the state of a single-level case, deterministic in its arguments"""
    bc, m = BCS[bcname], model_of(row)
    st = perturbed_state(nx, ny, seed, base=base_state(nx, ny, bc), head_amp=HEAD_AMP)
    return plant(st, PHYS, m, bc, seed + 1000 * list(ROWS).index(row) + 17 * nx + ny)


def moulin_lists(st):
    """(positions, sigma, flux) of the one moulin of the moulin row on the extent of state st"""
    lx, ly = st["dx"] * st["nx"], st["dy"] * st["ny"]
    return (np.array([[MOULIN["position"][0] * lx, MOULIN["position"][1] * ly]]), np.array([MOULIN["sigma"] * min(lx, ly)]),
            np.array([MOULIN["flux"]]))


# ---- the census
CELL, XFACE, YFACE = "cell", "x-face", "y-face"


def _mac_grad(a, mask, dx, dy, masked):
    """Gradient::compGradientMAC as oracle/time_loop.c:mac_grad: (ny, nx + 1) and (ny + 1, nx) from a ghosted array"""
    gx = (1.0 / dx) * (a[1:-1, 1:] - a[1:-1, :-1])
    gy = (1.0 / dy) * (a[1:, 1:-1] - a[:-1, 1:-1])
    if masked:
        gx = np.where((mask[1:-1, 1:] < 1e-6) | (mask[1:-1, :-1] < 1e-6), 0.0, gx)
        gy = np.where((mask[1:, 1:-1] < 1e-6) | (mask[:-1, 1:-1] < 1e-6), 0.0, gy)
    return gx, gy


def census(state, after, phys, model, patch=None, periodic=(0, 0), cover=None):
    """{branch: {arm: boolean map}} of one step of one level (or one box of a hierarchy's level).

    state: what entered the step -- ghosted B (with the ghosts the step's first fill left: the oracle's OM_BOLD), Pi, zb, mask, and dx, dy.
    after: what the oracle left -- ghosted head, mR, Pw; qwx, qwy; with diffusion dcx, dcy.  patch = (i0, j0, nxg, nyg) of a box (default: the
    level spans its domain); cover: 1 where a finer level covers the cell.  Maps of cell branches are (ny, nx), of face branches (ny, nx + 1) /
    (ny + 1, nx); counts() sums them.  The melt rate's branches are those of its LAST evaluation in the step ([III], d_melt<1>): the heads of the
    Picard iterations before it are not kept by either side; the branches of d_melt<0> on b, the mask and the model options are taken by the
    same cells.  abs_QPw is recomputed from the oracle's QWX, QWY, head, zb and mask as oracle/time_loop.c:melting_rate does."""
    m, ph = model, phys
    B, Pi, zb, mask = state["B"], state["Pi"], state["zb"], state["mask"]
    h = after["head"]
    v = lambda a: a[1:-1, 1:-1]
    ny, nx = v(B).shape
    i0, j0, nxg, nyg = patch if patch is not None else (0, 0, nx, ny)
    hm = int(ph.get("use_mask_gradients", 0))
    b, im = v(B), v(mask)
    every, none = np.ones((ny, nx), dtype=bool), np.zeros((ny, nx), dtype=bool)
    flag = lambda on: {"on": every if on else none, "off": none if on else every}
    out = {}
    # melting_rate
    gx, gy = _mac_grad(h, mask, state["dx"], state["dy"], hm)
    zx, zy = _mac_grad(zb, mask, state["dx"], state["dy"], hm)
    qx, qy = after["qwx"], after["qwy"]
    t1x, t1y, t2x, t2y = qx * gx, qy * gy, qx * zx, qy * zy
    t0, t1 = 0.5 * (t1x[:, :-1] + t1x[:, 1:]), 0.5 * (t1y[:-1, :] + t1y[1:, :])
    u0, u1 = 0.5 * (t2x[:, :-1] + t2x[:, 1:]), 0.5 * (t2y[:-1, :] + t2y[1:, :])
    Pw = m["gravity"] * m["rho_w"] * (v(h) - v(zb))
    sca = 20. * 20. * m["ub"][0] * np.abs(v(Pi) - Pw) * m["ub"][0] if m["basal_friction"] else 0.0
    abs_QPw = t0 + t1 - (u0 + u1)
    clamp = (abs_QPw < 0) & (b < 1e-6)
    out["melt: abs_QPw < 0 && b < 1e-6"] = {"clamped to 0": clamp, "abs_QPw >= 0": ~(abs_QPw < 0), "abs_QPw < 0, b >= 1e-6": (abs_QPw < 0) & ~(b < 1e-6)}
    abs_QPw = np.where(clamp, 0.0, abs_QPw)
    mr = (m["G"] + sca - m["rho_w"] * m["gravity"] * (t0 + t1) + m["ct"] * m["cw"] * m["rho_w"] * m["rho_w"] * m["gravity"] * abs_QPw) / m["L"]
    out["melt: fmax(m, 0)"] = {"m < 0 clamped": mr < 0.0, "m >= 0": ~(mr < 0.0)}
    out["melt: im < 0"] = {"ice-free, m = 0": im < 0.0, "ice": ~(im < 0.0)}
    out["melt: b < br"] = {"b < br": b < m["br"], "b >= br": ~(b < m["br"])}
    for opt in ("basal_friction", "use_moulin_source", "head_melt_off"):
        out["melt: " + opt] = flag(int(m.get(opt, 0)) != 0)
    out["melt: diffFactor != 0"] = flag(m["diffFactor"] != 0.0)
    # gap-height right-hand side
    masked_arm = (im < 0.0) & bool(m.get("use_mask_rhs_b", 0))
    impl = bool(m.get("use_impl_diff", 0))
    out["gap rhs: (im < 0) && use_mask_rhs_b"] = {"masked, explicit": masked_arm & (not impl), "masked, use_impl_diff": masked_arm & impl, "not masked": ~masked_arm}
    lo, hi = ph["cutOffbr"] > b, ~(ph["cutOffbr"] > b) & (ph["maxOffbr"] < b)
    out["gap rhs: B clamps"] = {"cutOffbr > b": ~masked_arm & lo, "maxOffbr < b": ~masked_arm & hi, "between": ~masked_arm & ~lo & ~hi}
    ub_norm = np.sqrt(m["ub"][0] * m["ub"][0] + m["ub"][1] * m["ub"][1])
    RHS_A = v(after["mR"]) * (1.0 / m["rho_i"])
    RHS_B = np.where(b < m["br"], ub_norm * (m["br"] - b) / m["lr"], 0.0)
    zero = ~masked_arm & (RHS_A + RHS_B == 0.0)
    out["gap rhs: cd = 0/0"] = {"RHS_A + RHS_B == 0 (NaN)": zero, "finite": ~zero}
    freeze = impl and bool(m.get("freeze_icefree_gap", 0))
    out["keep_icefree"] = {"kept (mask < 0)": (im < 0.0) & freeze, "solved": ~(im < 0.0) & freeze}
    out["picard maxima: cover"] = {"skipped (covered)": none if cover is None else cover != 0, "counted": every if cover is None else cover == 0}
    # faces
    for name, d in ((XFACE, 0), (YFACE, 1)):
        if d == 0:
            mh, ml = mask[1:-1, 1:], mask[1:-1, :-1]
            f = np.arange(nx + 1)[None, :] + i0 + np.zeros((ny, 1), dtype=int)
            dom = (f == 0) | (f == nxg)
        else:
            mh, ml = mask[1:, 1:-1], mask[:-1, 1:-1]
            f = np.arange(ny + 1)[:, None] + j0 + np.zeros((1, nx), dtype=int)
            dom = (f == 0) | (f == nyg)
        H, L = (mh < 1e-6) & bool(hm), (ml < 1e-6) & bool(hm)
        out["face_grad (%s): masked side" % name] = {"high cell only": H & ~L, "low cell only": L & ~H, "both": H & L, "neither": ~H & ~L}
        if m["diffFactor"] != 0.0:
            same = np.abs(mh - ml) < 1e-10
            mec = np.where(same, np.where(mh > 0.0, 1.0, -1.0), 0.0)
            out["dcoef (%s): |m - mm1| < 1e-10" % name] = {"equal": same, "differ": ~same}
            out["dcoef (%s): domain face" % name] = {"domain face, mec = 0": dom, "inside": ~dom}
            mec = np.where(dom, 0.0, mec)
            cut = (mec < 0.0) & (ph.get("cutOffB", 0) > 0)
            out["dcoef (%s): mec < 0 && cutOffB" % name] = {"cut to 0": cut, "kept": ~cut}
            dc = after["dcx" if d == 0 else "dcy"]
            out["dcoef (%s): 5e-6 floor" % name] = {"floor": ~cut & (dc == 5.0e-6), "b mR / rho_i": ~cut & (dc > 5.0e-6)}
            # ghosts of mR the faces read (d_extrap_ghosts): the side cells of the ring, by kind
            side = np.zeros(dom.shape, dtype=bool)
            if d == 0:
                side[:, 0] = side[:, -1] = True
            else:
                side[0, :] = side[-1, :] = True
            out["extrap_ghosts (%s sides)" % name] = {"periodic": side & dom & bool(periodic[d]), "domain": side & dom & (not periodic[d]),
                                                     "coarse-fine or fine-fine": side & ~dom}
    return out


def where(branch):
    """CELL, XFACE or YFACE: what the maps of a branch are laid over"""
    return XFACE if "(x-face" in branch else YFACE if "(y-face" in branch else CELL


def counts(cen):
    return {br: {arm: int(np.count_nonzero(mp)) for arm, mp in arms.items()} for br, arms in cen.items()}


def add_counts(total, c):
    for br, arms in c.items():
        t = total.setdefault(br, {})
        for arm, n in arms.items():
            t[arm] = t.get(arm, 0) + n
    return total


def arms_at(cen, kind, j, i):
    """the arms the cell (or face) (j, i) took, as one string: what a failure message names"""
    got = []
    for br, arms in cen.items():
        if where(br) != kind:
            continue
        for arm, mp in arms.items():
            if mp.shape[0] > j and mp.shape[1] > i and mp[j, i]:
                got.append("%s -> %s" % (br, arm))
    return "; ".join(got)


def fold_faces(c):
    """counts with the x-face and y-face twins of a branch added up under one name"""
    out = {}
    for br, arms in c.items():
        add_counts(out, {br.replace(" (x-face)", "").replace(" (y-face)", "").replace(" (x-face sides)", "").replace(" (y-face sides)", ""): arms})
    return out


# arms that cannot be taken where the census looks, with the reason; every other arm of every branch must be (tests/test_step_sweep_cpu.py)
NOT_ON_ONE_LEVEL = {("picard maxima: cover", "skipped (covered)"): "a single level has no finer level; asserted on hierarchies",
                    ("extrap_ghosts", "coarse-fine or fine-fine"): "a single level has no such side; asserted on hierarchies"}


# ---- hierarchies
HIER_SEEDS = range(40)
HIER_DT = 60.0
HIER_MODELS = dict([
    ("explicit", dict(use_mask_rhs_b=1)),
    ("explicit-diffusion", dict(diffFactor=1.0)),
    ("implicit-freeze", dict(diffFactor=1.0, use_impl_diff=1, freeze_icefree_gap=1)),
])
# layouts dropped from the device comparison by name, with the reason (a difference only the reference's un-vendored Chombo could arbitrate)
HIER_DROPPED = {
    # not a difference: the oracle alone leaves the hierarchy non-finite in step 1.  The layout's drawn boundary condition (a Neumann gradient of 3.1
    # per cell width on x-lo) with the adversarial fields makes the head SOLVE diverge (oracle/amrm.c: residual 4e-6 -> 1e8 in five V-cycles on the
    # fields as hierlayouts hands them out, no time step involved); the solve sweep stops at seed 23 and never met it
    "seed-32": "the oracle's head solve diverges on this layout's drawn boundary condition",
}


# The device comparison runs every kept layout of FEATURES and these of the 13 kept generated ones: one of 2, 3 and 4 levels without periodicity,
# the x-periodic ones of 4 and 2 levels, the y-periodic one.  Thinned because the file took 12.2 s against the 3.5 s of tests/test_gpu_hier_layouts.py
# on the same MI355X machine (most of it the oracle's own steps on the CPU); the oracle-only test runs all of them.
DEVICE_SEEDS = (0, 4, 8, 9, 13, 30)


def device_layouts():
    """the layouts tests/test_gpu_step_sweep.py runs"""
    kept, _ = hierarchy_layouts()
    return [c for c in kept if c[0] not in HIER_DROPPED and (not c[0].startswith("seed-") or c[3] in DEVICE_SEEDS)]


def hierarchy_layouts(seeds=HIER_SEEDS):
    """(kept, left out): lists of (name, bc, boxes, seed of fields and recut) -- left out are the layouts with coarse-fine ghost cells across a
    periodic side (hierlayouts.cf_ghosts_across_periodic), and only those"""
    every = [(name, bc, boxes, 100 + n) for n, (name, (bc, boxes)) in enumerate(hl.FEATURES.items())]
    every += [("seed-%d" % s,) + hl.generate(s) + (s,) for s in seeds]
    kept, out = [], []
    for c in every:
        (out if hl.cf_ghosts_across_periodic(hl.NX0, hl.NY0, c[1]["periodic"], c[2]) else kept).append(c)
    return kept, out


def hier_model_of(name):
    return dict(sy.A3_MODEL, G=0.05, dt=HIER_DT, **HIER_MODELS[name])


def hier_states(bc, boxes, seed):
    """per level, per box: the state dicts OracleAmrMModel.set_states / HipHierModel.set_states take, from hierlayouts.adversarial_fields: B, Pi,
    zb, mask as they are; head = phi padded by one cell + an offset that keeps Pw = rho_w g (head - zb) positive"""
    fs = hl.adversarial_fields(hl.NX0, hl.NY0, boxes, bc, seed)
    flat = [fs[0]] + [f for lev in fs[1:] for f in lev]
    off = max(0.0, max(float(np.max(f["zb"][1:-1, 1:-1] - f["phi"])) for f in flat)) + 10.0
    def one(f):
        head = np.pad(f["phi"], 1, mode="edge") + off
        return dict(f, head=np.ascontiguousarray(head))
    return [[one(fs[0])]] + [[one(f) for f in lev] for lev in fs[1:]]


def cover_map(l, box, boxes):
    """1.0 where level l + 1 covers the cell of `box` of level l (boxes[l] = the boxes of level l + 1), else 0.0"""
    lo0, lo1, hi0, hi1 = box
    c = np.zeros((hi1 - lo1 + 1, hi0 - lo0 + 1))
    if l < len(boxes):
        for f0, f1, g0, g1 in boxes[l]:
            a0, a1, b0, b1 = max(f0 // 2, lo0), max(f1 // 2, lo1), min(g0 // 2, hi0), min(g1 // 2, hi1)
            if a0 <= b0 and a1 <= b1:
                c[a1 - lo1:b1 - lo1 + 1, a0 - lo0:b0 - lo0 + 1] = 1.0
    return c


# ---- running the oracle over the sweep (the `oracle` argument is oracle.pyoracle; the device test steps its model from on_step)
def compared_fields(oracle):
    """(name of HipModel.get, id of OracleModel.field) of the cell fields compared after every step; cd may be NaN (0/0), the others may not"""
    return (("head", oracle.OM_H), ("B", oracle.OM_B), ("mR", oracle.OM_MR), ("Pw", oracle.OM_PW), ("cd", oracle.OM_CD), ("rhs_h", oracle.OM_RHSH),
            ("Re", oracle.OM_RE))


def box_census(oracle, get, dx, dy, phys, model, patch=None, periodic=(0, 0), cover=None):
    """census() of one level or box from the oracle's own arrays after a step; get(fid) -> a copy of the field.  OM_BOLD is the gap height that
    entered the step, with the ghost cells its first fill left"""
    state = dict(B=get(oracle.OM_BOLD), Pi=get(oracle.OM_PI), zb=get(oracle.OM_ZB), mask=get(oracle.OM_MASK), dx=dx, dy=dy)
    after = dict(head=get(oracle.OM_H), mR=get(oracle.OM_MR), qwx=get(oracle.OM_QWX), qwy=get(oracle.OM_QWY))
    if model["diffFactor"] != 0.0:
        after.update(dcx=get(oracle.OM_DCX), dcy=get(oracle.OM_DCY))
    return census(state, after, phys, model, patch=patch, periodic=periodic, cover=cover)


def oracle_problems(oracle, get, cen, what):
    """what would hide a failure, as a list of messages: a compared field that is not finite on a valid cell (cd: NaN anywhere but where the census
    says RHS_A + RHS_B == 0, or not NaN there)"""
    out = []
    for nm, fid in compared_fields(oracle):
        a = get(fid)[1:-1, 1:-1]
        if nm == "cd":
            want = cen["gap rhs: cd = 0/0"]["RHS_A + RHS_B == 0 (NaN)"]
            if not np.array_equal(np.isnan(a), want):
                out.append("%s: cd is NaN on %d cells, the census says 0/0 on %d" % (what, int(np.isnan(a).sum()), int(want.sum())))
            if np.isinf(a).any():
                out.append("%s: cd is infinite" % (what,))
        elif not np.isfinite(a).all():
            out.append("%s: %s is not finite on %d valid cells" % (what, nm, int((~np.isfinite(a)).sum())))
    return out


def iteration_problems(p, v, what):
    out = []
    if p > 20:
        out.append("%s: %d Picard iterations" % (what, p))
    if not v < 100 * p:
        out.append("%s: a head solve ended on max_iter (%d V-cycles in %d Picard iterations)" % (what, v, p))
    return out


def run_single(oracle, case, on_start=None, on_step=None, dt=None):
    """two steps of a single-level case on the oracle -> dict(iters=[(picard, vcycles)], census=[per step], problems=[messages]).
    on_start(O, st, bc, model, src) and on_step(k, dt, O, census, (picard, vcycles)) let the device test run its model in lockstep;
    dt: a first step size other than the row's own (a batch steps all its members with one: tests/batchsweep.py)"""
    cid, nx, ny, b, r = case
    bc, m = BCS[b], model_of(r)
    if dt is not None:
        m = dict(m, dt=dt)
    st = single_state(nx, ny, b, r)
    O = oracle.OracleModel(nx, ny, st["dx"], st["dy"], bc, PHYS, m, max_box=16, nthreads=1)
    rec = dict(iters=[], census=[], problems=[])
    try:
        O.set_state(st)
        src = None
        if m.get("use_moulin_source"):
            src, _ = oracle.moulin_source(nx, ny, st["dx"], st["dy"], *moulin_lists(st))
            O.field(oracle.OM_MSRC)[1:-1, 1:-1] = src
        if on_start:
            on_start(O, st, bc, m, src)
        get = lambda fid: np.array(O.field(fid))
        for k in range(N_STEPS):
            dt = m["dt"] * (0.5 if k == 1 else 1.0)
            try:
                p, v = O.timestep(dt)
            except RuntimeError as e:
                rec["problems"].append("%s step %d: raised %r" % (cid, k, e))
                break
            cen = box_census(oracle, get, st["dx"], st["dy"], PHYS, m, periodic=bc["periodic"])
            rec["iters"].append((p, v)); rec["census"].append(cen)
            rec["problems"] += iteration_problems(p, v, "%s step %d" % (cid, k)) + oracle_problems(oracle, get, cen, "%s step %d" % (cid, k))
            if on_step:
                on_step(k, dt, O, cen, (p, v))
    finally:
        O.close()
    return rec


def run_hier(oracle, layout, model_name, on_start=None, on_step=None, boxes=None):
    """two steps of a hierarchy case on the oracle -> dict(iters, census=[per step {(level, box): census}], problems); `boxes`: another cutting of
    the layout's unions"""
    name, bc, lboxes, seed = layout
    boxes = lboxes if boxes is None else boxes
    m = hier_model_of(model_name)
    sts = hier_states(bc, boxes, seed)
    O = oracle.OracleAmrMModel(hl.NX0, hl.NY0, sts[0][0]["dx"], sts[0][0]["dy"], bc, hl.ADV_PHYS, m, boxes, max_box=16, nthreads=1)
    rec = dict(iters=[], census=[], problems=[])
    try:
        O.set_states(sts)
        if on_start:
            on_start(O, sts, bc, m)
        for k in range(N_STEPS):
            dt = m["dt"] * (0.5 if k == 1 else 1.0)
            what = "%s %s step %d" % (name, model_name, k)
            try:
                p, v = O.timestep(dt)
            except RuntimeError as e:
                rec["problems"].append("%s: raised %r" % (what, e))
                break
            cens = {}
            for l in range(O.nlev):
                for q, box in enumerate(O.boxes[l]):
                    get = lambda fid: np.array(O.field(l, q, fid))
                    cens[(l, q)] = box_census(oracle, get, sts[l][q]["dx"], sts[l][q]["dy"], hl.ADV_PHYS, m, patch=(box[0], box[1], hl.NX0 << l, hl.NY0 << l),
                                              periodic=bc["periodic"], cover=cover_map(l, box, boxes))
                    rec["problems"] += oracle_problems(oracle, get, cens[(l, q)], "%s level %d box %d" % (what, l, q))
            rec["iters"].append((p, v)); rec["census"].append(cens)
            rec["problems"] += iteration_problems(p, v, what)
            if on_step:
                on_step(k, dt, O, cens, (p, v))
    finally:
        O.close()
    return rec


# on a hierarchy these must each be taken on a level with both a coarser and a finer neighbour, in at least one layout
MIDDLE_LEVEL_ARMS = (("picard maxima: cover", "skipped (covered)"), ("face_grad: masked side", "high cell only"), ("face_grad: masked side", "low cell only"),
                     ("gap rhs: B clamps", "cutOffbr > b"), ("gap rhs: B clamps", "maxOffbr < b"), ("dcoef: mec < 0 && cutOffB", "cut to 0"),
                     ("extrap_ghosts", "coarse-fine or fine-fine"))


def sweep_census(oracle):
    """the oracle over the whole sweep -> dict(single={case id: record}, hier={(layout, model): record}, problems=[...], single_arms={(branch, arm):
    (cells, set of case ids, set of shapes)}, hier_arms={(branch, arm): (cells, set of layouts where taken on a middle level)})"""
    out = dict(single={}, hier={}, problems=[], single_arms={}, hier_arms={})
    for case in single_cases():
        rec = out["single"][case[0]] = run_single(oracle, case)
        out["problems"] += rec["problems"]
        for cen in rec["census"]:
            for br, arms in fold_faces(counts(cen)).items():
                for arm, n in arms.items():
                    t = out["single_arms"].setdefault((br, arm), [0, set(), set()])
                    t[0] += n
                    if n:
                        t[1].add(case[0]); t[2].add((case[1], case[2]))
    kept, _ = hierarchy_layouts()
    for layout in kept:
        if layout[0] in HIER_DROPPED:
            continue
        for mn in HIER_MODELS:
            rec = out["hier"][(layout[0], mn)] = run_hier(oracle, layout, mn)
            out["problems"] += rec["problems"]
            nlev = 1 + len(layout[2])
            for cens in rec["census"]:
                for (l, q), cen in cens.items():
                    for br, arms in fold_faces(counts(cen)).items():
                        for arm, n in arms.items():
                            t = out["hier_arms"].setdefault((br, arm), [0, set()])
                            t[0] += n
                            if n and 0 < l < nlev - 1:
                                t[1].add(layout[0])
    return out


def census_table(sw):
    """the census of sweep_census() as text: tests/golden/STEP_SWEEP_CENSUS.txt (tools/step_sweep_census.py writes it)"""
    lines = ["# census of the time-step sweep on the CPU oracle: tests/stepsweep.py, regenerated by tools/step_sweep_census.py",
             "# single level: %d cases x %d steps; cells or faces that took the arm, cases and shapes in which at least one did" % (len(sw["single"]), N_STEPS),
             "%-42s %-28s %9s %6s %6s" % ("branch", "arm", "cells", "cases", "shapes")]
    for (br, arm), (n, cs, shp) in sw["single_arms"].items():
        lines.append("%-42s %-28s %9d %6d %6d" % (br, arm, n, len(cs), len(shp)))
    lines += ["# hierarchies: %d layouts x %d models x %d steps; cells or faces of all levels, layouts in which a level between two others took the arm"
              % (len({k[0] for k in sw["hier"]}), len(HIER_MODELS), N_STEPS),
              "%-42s %-28s %9s %7s" % ("branch", "arm", "cells", "layouts")]
    for (br, arm), (n, lay) in sw["hier_arms"].items():
        lines.append("%-42s %-28s %9d %7d" % (br, arm, n, len(lay)))
    return "\n".join(lines) + "\n"
