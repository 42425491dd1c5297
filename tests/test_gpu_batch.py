"""An ensemble of levels on one grid (suhmo_batch_*): every member of a batched V-cycle / solve against the CPU oracle's run of that
member ALONE, bitwise (np.array_equal), none skipped -- head, residual, the coarse depths, the stored ghost rings (tests/ghostring.py),
cycle counts and residual norms -- plus the counters that show the batch path ran, the member handles, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import ghostring as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipmodel():
    from suhmo_amd import capi, model
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return model


@pytest.fixture(scope="module")
def hip():
    from suhmo_amd import capi, level
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return level


def member_inputs(kind, nx, ny, k):
    """fields, BC values and physics constants of member k: all different between members; the BC TYPES are the batch's"""
    rng = np.random.default_rng([91, k])
    if kind == "mixedbc":                                        # Dirichlet / Neumann mix, random coefficients with ice-free cells, alpha != 0
        f = sy.random_fields(nx, ny, seed=300 + k)
        bc = dict(sy.RANDOM_BC, value=[[3.0 + k, -0.02 * (k + 1)], [0.01 * (k + 1), 7.0 - k]])
        ph = dict(sy.RANDOM_PHYS, A=5e-25 * (1.0 + 0.3 * k), cutOffbr=0.01 + 0.002 * k, omega=1e-3 * (1.0 + 0.1 * k))
    else:                                                        # y periodic, SHMIP geometry
        f = sy.shmip_fields(nx, ny, seed=500 + k, source=5.79e-9 * (k + 1))
        f["phi"] = f["phi"] + rng.uniform(-0.5, 0.5, size=f["phi"].shape) * (k + 1)
        f["B"] = np.ascontiguousarray(f["B"] * (1.0 + 0.1 * k))
        bc = dict(sy.CONV_BC, value=[[0.5 * k, 1e-4 * k], [0.0, 0.0]])
        ph = dict(sy.A3_PHYS, A=5e-25 / (1.0 + 0.5 * k), nu=1.787e-6 * (1.0 + 0.05 * k))
    f.pop("bx", None); f.pop("by", None)
    return f, bc, ph


def load(B, O_cls, kind, nx, ny, bc0, alpha, max_box, members=None):
    """the batch's members and one oracle level per member, loaded with the same inputs"""
    Os = []
    for k in range(len(B)):
        f, bc, ph = member_inputs(kind, nx, ny, k if members is None else members[k])
        assert bc["type"] == bc0["type"] and bc["periodic"] == bc0["periodic"]
        m = B.member(k)
        B.set_bc(k, bc); B.set_phys(k, ph)
        m.set_inputs(f); m.build_mg_coefficients()
        O = O_cls(nx, ny, f["dx"], f["dy"], bc, ph, alpha, -1.0, max_box, 4)
        O.set_inputs(f); O.build_mg_coefficients()
        Os.append((O, f, bc))
    return Os


def same_member(oracle, hip, O, G, f, bc, what, relaxed_last):
    assert np.array_equal(G.get(hip.F_PHI), O.get(oracle.F_PHI)), (what, "head")
    go, gg = O.get(oracle.F_PHI, ghosted=True), G.get(hip.F_PHI, ghosted=True)
    gr.level_ring_equal(go, gg, (f["nx"], f["ny"]), bc["periodic"], what=what)
    if relaxed_last:
        gr.domain_bc_holds(gg, bc, f["dx"], f["dy"], (0, 0, f["nx"] - 1, f["ny"] - 1), (f["nx"], f["ny"]), what)
    for d in range(1, G.ndepth):
        assert np.array_equal(G.get(hip.F_PHI, depth=d), O.get(oracle.F_PHI, depth=d)), (what, "coarse head", d)
        assert np.array_equal(G.get(hip.F_RHS, depth=d), O.get(oracle.F_RHS, depth=d)), (what, "coarse right-hand side", d)
        assert np.array_equal(G.get(hip.F_RES, depth=d), O.get(oracle.F_RES, depth=d)), (what, "coarse residual", d)
    O.residual(); G.residual()
    assert np.array_equal(G.get(hip.F_RES), O.get(oracle.F_RES)), (what, "residual")


VCYCLE_CASES = [("mixedbc-128x64", "mixedbc", 128, 64, sy.RANDOM_BC, 0.6, 16, 4),
                ("yperiodic-320x64", "yperiodic", 320, 64, sy.CONV_BC, 0.0, 64, 6)]


@pytest.mark.parametrize("case", VCYCLE_CASES, ids=[c[0] for c in VCYCLE_CASES])
def test_batch_vcycle_every_member_is_the_oracles(oracle, hip, case):
    name, kind, nx, ny, bc0, alpha, max_box, ndepth = case
    f0 = member_inputs(kind, nx, ny, 0)[0]
    B = hip.HipBatch(5, nx, ny, f0["dx"], f0["dy"], bc0, sy.A3_PHYS, alpha=alpha, max_box=max_box)
    assert B.ndepth == ndepth
    Os = load(B, oracle.OracleLevel, kind, nx, ny, bc0, alpha, max_box)
    sp = dict(sy.SOLVER_DEFAULT)
    done = 0
    for upto in (1, 3):
        while done < upto:
            B.vcycle(sp)
            for O, _, _ in Os:
                O.vcycle(sp)
            done += 1
        for k, (O, f, bc) in enumerate(Os):
            assert O.ndepth == ndepth
            same_member(oracle, hip, O, B.member(k), f, bc, (name, "member", k, "cycles", upto), relaxed_last=True)
    assert B.get_option("batch_member_cycles") == 15 and B.get_option("batch_readbacks") == 0
    B.close()


def test_batch_vcycle_active_flags(oracle, hip):
    """only the flagged members advance; flags that select nobody are a no-op returning 0"""
    kind, nx, ny, bc0 = "yperiodic", 128, 64, sy.CONV_BC
    f0 = member_inputs(kind, nx, ny, 0)[0]
    B = hip.HipBatch(4, nx, ny, f0["dx"], f0["dy"], bc0, sy.A3_PHYS)
    Os = load(B, oracle.OracleLevel, kind, nx, ny, bc0, 0.0, 64)
    sp = dict(sy.SOLVER_DEFAULT)
    before = [B.member(k).get(hip.F_PHI, ghosted=True) for k in range(4)]
    n0 = B.get_option("batch_launches")
    B.vcycle(sp, active=[0, 0, 0, 0])
    assert B.get_option("batch_launches") == n0 and B.get_option("batch_member_cycles") == 0
    B.vcycle(sp, active=[0, 1, 0, 1])
    B.vcycle(sp, active=[0, 0, 0, 1])
    for k, cycles in enumerate((0, 1, 0, 2)):
        O, f, bc = Os[k]
        for _ in range(cycles):
            O.vcycle(sp)
        if cycles:
            same_member(oracle, hip, O, B.member(k), f, bc, ("active", k), relaxed_last=True)
        else:
            assert np.array_equal(B.member(k).get(hip.F_PHI, ghosted=True), before[k]), k
    assert B.get_option("batch_member_cycles") == 3
    B.close()


# members of one solve that stop at different cycles: (source term, amplitude of the head's perturbation, flow-law constant)
SOLVE_MEMBERS = [(5.79e-9, 1e-3, 5e-25), (5.79e-7, 1e-1, 5e-25), (2.5e-8, 1.0, 2.5e-25), (7.93e-11, 1e-5, 5e-25), (4.5e-8, 10.0, 1e-24)]
SOLVE_SP = dict(sy.SOLVER_DEFAULT, eps=1e-8, norm_thresh=1e-12, max_iter=30, imin=3, iter_min=1)


def solve_inputs(nx, ny, k):
    src, amp, A = SOLVE_MEMBERS[k]
    f = sy.shmip_fields(nx, ny, seed=100 + k, source=src)
    base = 101325.0 / (sy.RHO_W * sy.GRAV)
    f["phi"] = base + (f["phi"] - base) * (amp / 1e-3)
    return f, dict(sy.A3_PHYS, A=A)


def load_solve(B, hip, nx, ny, order):
    for pos, k in enumerate(order):
        f, ph = solve_inputs(nx, ny, k)
        B.set_phys(pos, ph)
        B.member(pos).set_inputs(f); B.member(pos).build_mg_coefficients()


def test_batch_solve_members_stop_at_their_own_cycle(oracle, hip):
    """cycle count, final residual norm, head, ring and residual of every member equal the oracle's solve of that member alone; the
    oracle's counts (16 ... 22 cycles when this test was written) differ between members, and the batch reads back once for the initial
    norms and once per cycle of the member that runs longest -- not once per member and cycle"""
    nx, ny = 128, 64
    f0 = solve_inputs(nx, ny, 0)[0]
    n = len(SOLVE_MEMBERS)
    B = hip.HipBatch(n, nx, ny, f0["dx"], f0["dy"], sy.A3_BC, sy.A3_PHYS)
    load_solve(B, hip, nx, ny, range(n))
    want = []
    for k in range(n):
        f, ph = solve_inputs(nx, ny, k)
        O = oracle.OracleLevel(nx, ny, f["dx"], f["dy"], sy.A3_BC, ph, 0.0, -1.0, 64, 4)
        O.set_inputs(f); O.build_mg_coefficients()
        it, hist = O.solve(SOLVE_SP)
        want.append((O, f, it, hist))
    counts = [w[2] for w in want]
    assert len(set(counts)) >= 3, ("the oracle's cycle counts must differ between members", counts)
    iters, res = B.solve(SOLVE_SP)
    print("cycles per member: oracle", counts, "batch", iters, "read-backs", B.get_option("batch_readbacks"))
    assert iters == counts
    for k, (O, f, it, hist) in enumerate(want):
        assert res[k] == hist[-1], (k, res[k], hist[-1])
        G = B.member(k)
        assert np.array_equal(G.get(hip.F_PHI), O.get(oracle.F_PHI)), k
        gr.level_ring_equal(O.get(oracle.F_PHI, ghosted=True), G.get(hip.F_PHI, ghosted=True), (nx, ny), sy.A3_BC["periodic"], what=("solve", k))
        assert np.array_equal(G.get(hip.F_RES), O.get(oracle.F_RES)), k
        for d in range(1, G.ndepth):
            assert np.array_equal(G.get(hip.F_PHI, depth=d), O.get(oracle.F_PHI, depth=d)), (k, d)
    assert B.get_option("batch_readbacks") == 1 + max(counts)          # (1: the norms of the initial residuals)
    assert B.get_option("batch_member_cycles") == sum(counts)
    B.close()


STEP_FIELDS = ("head", "B", "mR", "Re", "Pw", "qwx", "qwy", "cd", "rhs_h")


def step_member(k):
    """model parameters, physics constants and initial state of ensemble member k at 128 x 32 (all different; diffusion on for odd k)"""
    nx, ny = 128, 32
    rng = np.random.default_rng([77, k])
    st = sy.shmip_initial_state(nx, ny)
    st["B"] = st["B"] * rng.uniform(0.5, 12.0, size=st["B"].shape)
    st["head"] = st["head"] + rng.uniform(0.0, 30.0, size=st["head"].shape)
    m = dict(sy.A3_MODEL, distributed_input=list(sy.SHMIP_A_INPUT.values())[k % 6], diffFactor=1.0 if k % 2 else 0.0, eps_picard=1e-4 / (1 + k))
    return st, m, dict(sy.A3_PHYS, A=5e-25 * (1.0 + 0.2 * k))


def test_batch_timestep_independent_of_composition(hipmodel):
    """member X as a batch of 1, as member 0 of {X, Y, Z} and as member 2 of {Z, Y, X}, 5 time steps: X's fields, rings and counts identical"""
    nx, ny = 128, 32
    X, Y, Z = 3, 0, 4
    got = []
    for order, pos in (((X,), 0), ((X, Y, Z), 0), ((Z, Y, X), 2)):
        ins = [step_member(k) for k in order]
        G = hipmodel.HipBatchModel(nx, ny, ins[0][0]["dx"], ins[0][0]["dy"], sy.A3_BC, [i[2] for i in ins], [i[1] for i in ins], max_box=16)
        for q, i in enumerate(ins):
            G.set_state(q, i[0])
        counts = []
        for _ in range(5):
            pi, nv = G.timestep(3600.0)
            counts.append((pi[pos], nv[pos]))
        got.append((counts, [G.get(pos, nm) for nm in STEP_FIELDS], G.get(pos, "head", ghosted=True), G.get(pos, "B", ghosted=True)))
        G.close()
    for g in got[1:]:
        assert g[0] == got[0][0]
        for nm, a, b in zip(STEP_FIELDS, g[1], got[0][1]):
            assert np.array_equal(a, b, equal_nan=True), nm
        assert np.array_equal(g[2], got[0][2]) and np.array_equal(g[3], got[0][3])


def test_batch_member_handles(hip):
    """a member handle is an ordinary level: what is stored through it is what the batch solves, what the batch computed is read
    through it, and a batch of 1 equals suhmo_level_solve on an ordinary level with the same inputs"""
    nx, ny = 128, 64
    f, ph = solve_inputs(nx, ny, 1)
    B = hip.HipBatch(1, nx, ny, f["dx"], f["dy"], sy.A3_BC, sy.A3_PHYS)
    B.set_phys(0, ph)
    m = B.member(0)
    m.set_inputs(f)
    assert np.array_equal(m.get(hip.F_PHI), f["phi"]) and np.array_equal(m.get(hip.F_B, ghosted=True)[1:-1, 1:-1], f["B"][1:-1, 1:-1])
    m.build_mg_coefficients()
    L = hip.HipLevel(nx, ny, f["dx"], f["dy"], sy.A3_BC, ph)
    L.set_inputs(f); L.build_mg_coefficients()
    iters, res = B.solve(SOLVE_SP)
    n, hist = L.solve(SOLVE_SP)
    assert iters == [n] and res[0] == hist[-1]
    assert np.array_equal(m.get(hip.F_PHI, ghosted=True), L.get(hip.F_PHI, ghosted=True))
    assert np.array_equal(m.get(hip.F_RES), L.get(hip.F_RES))
    assert m.norm(hip.F_RES, 0) == res[0]
    # the member's own entry points keep working on the batch's state, and the batch on theirs (the head canvases trade places in both)
    sp = dict(sy.SOLVER_DEFAULT)
    m.vcycle(sp); L.vcycle(sp)
    B.vcycle(sp); L.vcycle(sp)
    m.gsrb(3); L.gsrb(3)
    B.vcycle(sp); L.vcycle(sp)
    assert np.array_equal(m.get(hip.F_PHI), L.get(hip.F_PHI))
    B.close(); L.close()


def test_batch_refusals_leave_it_usable(oracle, hip):
    from suhmo_amd import capi
    lib = capi.lib()
    kind, nx, ny, bc0 = "yperiodic", 128, 64, sy.CONV_BC
    f0 = member_inputs(kind, nx, ny, 0)[0]
    d = capi.LevelDesc()
    d.nx, d.ny, d.j0, d.ny_global, d.dx, d.dy = nx, ny, 0, ny, f0["dx"], f0["dy"]
    d.nbox, d.boxes, d.max_box, d.alpha, d.beta = 0, None, 64, 0.0, -1.0
    d.bc, d.phys, d.device, d.halo_rows = hip._bc(bc0), hip._phys(sy.A3_PHYS), 0, 1
    h = C.c_void_p()
    assert lib.suhmo_batch_create(C.byref(h), C.byref(d), 0) == -1 and b"n_members" in lib.suhmo_last_error()
    d.j0, d.ny_global = 64, 128                                  # a rank strip
    assert lib.suhmo_batch_create(C.byref(h), C.byref(d), 2) == -5 and b"whole levels" in lib.suhmo_last_error()
    d.j0, d.ny_global, d.i0, d.nx_global = 0, ny, 16, 512         # an AMR patch
    assert lib.suhmo_batch_create(C.byref(h), C.byref(d), 2) == -5 and b"whole levels" in lib.suhmo_last_error()
    B = hip.HipBatch(2, nx, ny, f0["dx"], f0["dy"], bc0, sy.A3_PHYS)
    Os = load(B, oracle.OracleLevel, kind, nx, ny, bc0, 0.0, 64)
    v = C.c_long()
    assert lib.suhmo_batch_set_option(B.h, b"no_such_option", 1) == -1 and b"unknown option" in lib.suhmo_last_error()
    assert lib.suhmo_batch_get_option(B.h, b"no_such_option", C.byref(v)) == -1
    assert lib.suhmo_batch_set_option(B.h, b"batch_launches", 0) == -1 and b"read-only" in lib.suhmo_last_error()
    assert lib.suhmo_batch_set_option(B.h, b"bottom_solver", 1) == -5 and b"bottom_solver" in lib.suhmo_last_error()
    assert lib.suhmo_level_destroy(B.member(0).h) == -1 and b"member of a batch" in lib.suhmo_last_error()
    assert lib.suhmo_batch_member(B.h, 2) is None
    sp = hip.solver_params(sy.SOLVER_DEFAULT)
    none = (C.c_int * 2)(0, 0)
    assert lib.suhmo_batch_vcycle(B.h, C.byref(sp), none, None) == 0
    B.member(1).set_option("bottom_solver", 1)                   # a member asking for the bottom solver: the batch call is refused, nothing ran
    assert lib.suhmo_batch_vcycle(B.h, C.byref(sp), None, None) == -5 and b"bottom_solver" in lib.suhmo_last_error()
    B.member(1).set_option("bottom_solver", 0)
    assert B.get_option("batch_launches") == 0
    B.vcycle(sy.SOLVER_DEFAULT)                                  # still usable, and still the oracle's
    for k, (O, f, bc) in enumerate(Os):
        O.vcycle(sy.SOLVER_DEFAULT)
        same_member(oracle, hip, O, B.member(k), f, bc, ("after refusals", k), relaxed_last=True)
    B.close()


def test_batch_launch_count_does_not_grow_with_members(hip):
    """a V-cycle of 6 members issues exactly the launches of a V-cycle of 1; a solve of n members reads back as often as its slowest one"""
    nx, ny = 320, 64
    f0 = sy.shmip_fields(nx, ny)
    counts = {}
    for n in (1, 6):
        B = hip.HipBatch(n, nx, ny, f0["dx"], f0["dy"], sy.A3_BC, sy.A3_PHYS)
        for k in range(n):
            B.member(k).set_inputs(sy.shmip_fields(nx, ny, seed=40 + k)); B.member(k).build_mg_coefficients()
        B.vcycle(sy.SOLVER_DEFAULT)
        counts[n] = B.get_option("batch_launches")
        assert B.get_option("batch_member_cycles") == n
        B.close()
    print("launches of one batched V-cycle at 320 x 64:", counts)
    assert counts[1] == counts[6] > 0


def same_step_fields(oracle, O, G, k, nx, ny, periodic, what):
    """member k of the batch model G against the oracle model O after a step: head, gap height, melt rate, Re, Pw (and the fluxes, cd, RHS_h),
    the head's stored ghost ring and the copied ghosts of the gap height"""
    v = lambda a: np.array(a)[1:-1, 1:-1]
    for nm, fid in (("head", oracle.OM_H), ("B", oracle.OM_B), ("mR", oracle.OM_MR), ("Re", oracle.OM_RE), ("Pw", oracle.OM_PW),
                    ("cd", oracle.OM_CD), ("rhs_h", oracle.OM_RHSH)):
        a, b = v(O.field(fid)), G.get(k, nm)
        assert np.array_equal(a, b, equal_nan=True), (what, nm, float(np.nanmax(np.abs(a - b))))
    for nm, fid in (("qwx", oracle.OM_QWX), ("qwy", oracle.OM_QWY)):
        assert np.array_equal(np.array(O.field(fid)), G.get(k, nm), equal_nan=True), (what, nm)
    gr.level_ring_equal(np.array(O.field(oracle.OM_H)), G.get(k, "head", ghosted=True), (nx, ny), periodic, what=(what, "head"))
    a, b = np.array(O.field(oracle.OM_B)), G.get(k, "B", ghosted=True)
    assert np.array_equal(a[1:-1, :], b[1:-1, :]) and np.array_equal(a[:, 1:-1], b[:, 1:-1]), (what, "ghosts of the gap height")


def test_batch_timestep_mixed_suite(oracle, hipmodel):
    """one batch of SHMIP A1-A6 and two moulin members (suite B's inputs B1 and B5 with the explicit gap update: use_moulin_source = 1, diffFactor = 1,
    the source array loaded through the member handle) at 320 x 64, steps 1-51 from the SHMIP initial state: cur_step crosses both
    solver-parameter thresholds (2 and 50).  Picard iterations and V-cycles of every member equal or_model_timestep's at EVERY step; at steps
    1, 2, 3, 49, 50, 51 so do head, gap height, melt rate, Re, Pw, fluxes and the stored ghost rings."""
    import json
    import os
    binp = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shmip_B_inputs.json")))
    nx, ny = 320, 64
    st = sy.shmip_initial_state(nx, ny)
    models, srcs = [], []
    for case in ("A1", "A2", "A3", "A4", "A5", "A6"):
        models.append(sy.shmip_a_model(case)); srcs.append(None)
    for case in ("B1", "B5"):
        models.append(dict(sy.shmip_b_model(case, binp[case]), use_impl_diff=0))
        srcs.append(oracle.moulin_source(nx, ny, st["dx"], st["dy"], np.array(binp[case]["positions"]).reshape(-1, 2), binp[case]["sigma"], binp[case]["flux"], 1.0)[0])
    n = len(models)
    G = hipmodel.HipBatchModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, models, max_box=64)
    Os = []
    from suhmo_amd import level as lv
    for k in range(n):
        O = oracle.OracleModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, models[k], max_box=64, nthreads=4)
        O.set_state(st); G.set_state(k, st)
        if srcs[k] is not None:
            O.field(oracle.OM_MSRC)[1:-1, 1:-1] = srcs[k]
            G.member(k).level.set(lv.F_MSRC, srcs[k])
        Os.append(O)
    seen = set()
    for step in range(1, 52):
        pi, nv = G.timestep(3600.0)
        want = [O.timestep(3600.0) for O in Os]
        assert list(zip(pi, nv)) == want, (step, list(zip(pi, nv)), want)
        seen.update(want)
        if step in (1, 2, 3, 49, 50, 51):
            for k in range(n):
                same_step_fields(oracle, Os[k], G, k, nx, ny, sy.A3_BC["periodic"], ("step", step, "member", k))
    print("distinct (picard iterations, V-cycles) per member and step:", sorted(seen))
    assert len(seen) > 1
    for O in Os:
        O.close()
    G.close()


def test_batch_timestep_member_interop_and_batch_of_one(hipmodel, hip):
    """postproc_table / set_field / get_field on a member handle see the batch's state; a batch of 1 equals suhmo_level_timestep on an ordinary
    level with the same inputs, step by step"""
    nx, ny = 128, 32
    st, m, ph = step_member(1)                                    # (diffusion on)
    G = hipmodel.HipBatchModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, ph, [m], max_box=16)
    L = hipmodel.HipModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, ph, m, max_box=16)
    G.set_state(0, st); L.set_state(st)
    assert np.array_equal(G.get(0, "head"), st["head"][1:-1, 1:-1])
    for step in range(4):
        pi, nv = G.timestep(3600.0)
        assert (pi[0], nv[0]) == L.timestep(3600.0), step
        for nm in STEP_FIELDS:
            assert np.array_equal(G.get(0, nm), L.get(nm), equal_nan=True), (step, nm)
        assert np.array_equal(G.get(0, "head", ghosted=True), L.get("head", ghosted=True))
        assert np.array_equal(G.postproc_table_device(0), L.postproc_table_device(), equal_nan=True)
        assert np.array_equal(G.postproc_table(0), L.postproc_table(), equal_nan=True)
    # a head stored through the member handle is the head the next batched step starts from
    h = L.get("head") + 1.0
    G.member(0).level.set(hip.F_PHI, h); L.level.set(hip.F_PHI, h)
    pi, nv = G.timestep(3600.0)
    assert (pi[0], nv[0]) == L.timestep(3600.0)
    assert np.array_equal(G.get(0, "head"), L.get("head")) and np.array_equal(G.get(0, "B"), L.get("B"))
    G.close(); L.close()


def test_batch_timestep_refusals(hipmodel):
    """use_impl_diff = 1 on any member: rc -5 with a message, nothing stepped; members whose BC types differ: rc -1; the batch stays usable"""
    from suhmo_amd import capi
    lib = capi.lib()
    nx, ny = 128, 32
    ins = [step_member(k) for k in range(2)]
    G = hipmodel.HipBatchModel(nx, ny, ins[0][0]["dx"], ins[0][0]["dy"], sy.A3_BC, [i[2] for i in ins], [i[1] for i in ins], max_box=16)
    S = hipmodel.HipBatchModel(nx, ny, ins[0][0]["dx"], ins[0][0]["dy"], sy.A3_BC, [i[2] for i in ins], [i[1] for i in ins], max_box=16)
    for q, i in enumerate(ins):
        G.set_state(q, i[0]); S.set_state(q, i[0])
    G.set_model(1, use_impl_diff=1)
    pi, nv = (C.c_int * 2)(), (C.c_int * 2)()
    assert lib.suhmo_batch_timestep(G.batch.h, G._mp, 3600.0, 1, pi, nv, None) == -5 and b"use_impl_diff" in lib.suhmo_last_error()
    assert G.get_option("batch_launches") == 0
    G.set_model(1, use_impl_diff=0)
    G.batch.set_bc(1, dict(sy.A3_BC, type=[[1, 1], [1, 0]]))
    assert lib.suhmo_batch_timestep(G.batch.h, G._mp, 3600.0, 1, pi, nv, None) == -1 and b"shared by all members" in lib.suhmo_last_error()
    G.batch.set_bc(1, sy.A3_BC)
    assert G.timestep(3600.0) == S.timestep(3600.0)
    for q in range(2):
        for nm in STEP_FIELDS:
            assert np.array_equal(G.get(q, nm), S.get(q, nm), equal_nan=True), (q, nm)
    G.close(); S.close()
