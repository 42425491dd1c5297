"""An ensemble with the reference's RelaxSolver as the bottom of every V-cycle (suhmo_batch_create_opts "bottom_solver=1"; HipBatch /
HipBatchModel bottom_solver=True): one workgroup per active member in one launch (suhmo_amd/csrc/suhmo_bottom.hip).  Every member against
the CPU oracle's run of that member ALONE under SUHMO_ORACLE_BOTTOM=1, with np.array_equal throughout, and against a level of its own
with level option bottom_solver = 1 (which pins the order of the l2 sums of RelaxSolver's break test: the oracle's is serial).  The batch
interface returns the final residual norm of a solve, not the history: that is what is compared with the last entry of the oracle's."""
import ctypes as C

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import ghostring as gr
from tests.test_gpu_batch import (SOLVE_MEMBERS, SOLVE_SP, VCYCLE_CASES, load, load_solve, member_inputs, same_member, same_step_fields,
                                  solve_inputs)

pytestmark = pytest.mark.gpu

SP = dict(sy.SOLVER_DEFAULT, num_bottom=2, eps=1e-10, norm_thresh=1e-13, max_iter=8, imin=10)


@pytest.fixture(scope="module")
def hip():
    from suhmo_amd import capi, level
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return level


@pytest.fixture(scope="module")
def hipmodel():
    from suhmo_amd import capi, model
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return model


@pytest.fixture(autouse=True)
def _oracle_runs_relaxsolver(monkeypatch):
    monkeypatch.setenv("SUHMO_ORACLE_BOTTOM", "1")


def batch(hip, n, case, bottom_solver=True):
    name, kind, nx, ny, bc0, alpha, max_box, ndepth = case
    f0 = member_inputs(kind, nx, ny, 0)[0]
    B = hip.HipBatch(n, nx, ny, f0["dx"], f0["dy"], bc0, sy.A3_PHYS, alpha=alpha, max_box=max_box, bottom_solver=bottom_solver)
    assert B.ndepth == ndepth
    return B


def load_members(B, kind, nx, ny, members=None):
    """the inputs of test_gpu_batch.load without the oracle levels"""
    for k in range(len(B)):
        f, bc, ph = member_inputs(kind, nx, ny, k if members is None else members[k])
        B.set_bc(k, bc); B.set_phys(k, ph)
        B.member(k).set_inputs(f); B.member(k).build_mg_coefficients()


@pytest.mark.parametrize("case", VCYCLE_CASES, ids=[c[0] for c in VCYCLE_CASES])
def test_vcycle_and_solve_every_member_is_the_oracles(oracle, hip, case):
    """5 members, bottoms of 16 x 8 (mixedbc: alpha, Dirichlet / Neumann, ice-free cells) and 10 x 2 (yperiodic: less than one wave): after 1 and
    3 V-cycles and after a solve, head, ring, PHI / RHS / RES of every coarse depth, the depth-0 residual, cycle counts and final norms are the
    oracle's; a twin batch without the option shows that the option changed every member"""
    name, kind, nx, ny, bc0, alpha, max_box, ndepth = case
    B, T = batch(hip, 5, case), batch(hip, 5, case, bottom_solver=False)
    assert B.get_option("bottom_solver") == 1 and T.get_option("bottom_solver") == 0
    Os = load(B, oracle.OracleLevel, kind, nx, ny, bc0, alpha, max_box)
    load_members(T, kind, nx, ny)
    done = 0
    for upto in (1, 3):
        while done < upto:
            B.vcycle(SP); T.vcycle(SP)
            for O, _, _ in Os:
                O.vcycle(SP)
            done += 1
        for k, (O, f, bc) in enumerate(Os):
            same_member(oracle, hip, O, B.member(k), f, bc, (name, "member", k, "cycles", upto), relaxed_last=True)
            if upto == 1 and kind == "yperiodic":
                assert not np.array_equal(B.member(k).get(hip.F_PHI), T.member(k).get(hip.F_PHI)), (name, k, "one cycle: same head as without the option")
    assert B.get_option("batch_member_cycles") == 15 and B.get_option("batch_readbacks") == 0
    iters, res = B.solve(SP)
    T.solve(SP)
    total = 0
    for k, (O, f, bc) in enumerate(Os):
        it, hist = O.solve(SP)
        print(name, "member", k, "cycles: oracle", it, "batch", iters[k], "final norm", hist[-1], res[k])
        assert iters[k] == it and res[k] == hist[-1], (name, k, iters[k], it, res[k], hist[-1])
        same_member(oracle, hip, O, B.member(k), f, bc, (name, "member", k, "solve"), relaxed_last=False)
        assert not np.array_equal(B.member(k).get(hip.F_PHI), T.member(k).get(hip.F_PHI)), (name, k, "solve: same head as without the option")
        assert B.member(k).get_option("bottom_solver_iterations") > 0, (name, k)
        assert B.member(k).get_option("bottom_solves_one_launch") == 3 + it, (name, k)
        assert B.member(k).get_option("bottom_solves_host_loop") == 0
        total += 3 + it
    assert B.get_option("bottom_solves_one_launch") == total
    assert B.get_option("bottom_solver_iterations") == sum(B.member(k).get_option("bottom_solver_iterations") for k in range(5))
    assert T.get_option("bottom_solves_one_launch") == 0 and T.get_option("bottom_solver_iterations") == 0
    B.close(); T.close()


@pytest.mark.parametrize("case", VCYCLE_CASES, ids=[c[0] for c in VCYCLE_CASES])
def test_batch_equals_solo_bit_for_bit(hip, case):
    """every member against a HipLevel of its own with bottom_solver = 1 on the same inputs: head, ring, counts, norms and RelaxSolver's iteration
    count (the l2 sums of its break test are summed in the same order: 1024 thread-strided partial sums, the butterfly, the waves in order)"""
    name, kind, nx, ny, bc0, alpha, max_box, ndepth = case
    B = batch(hip, 5, case)
    load_members(B, kind, nx, ny)
    for _ in range(3):
        B.vcycle(SP)
    iters, res = B.solve(SP)
    for k in range(5):
        f, bc, ph = member_inputs(kind, nx, ny, k)
        L = hip.HipLevel(nx, ny, f["dx"], f["dy"], bc, ph, alpha, -1.0, max_box)
        L.set_option("bottom_solver", 1)
        L.set_inputs(f); L.build_mg_coefficients()
        for _ in range(3):
            L.vcycle(SP)
        n, hist = L.solve(SP)
        assert iters[k] == n and res[k] == hist[-1], (name, k)
        assert np.array_equal(B.member(k).get(hip.F_PHI, ghosted=True), L.get(hip.F_PHI, ghosted=True)), (name, k, "head and ring")
        assert B.member(k).get_option("bottom_solver_iterations") == L.get_option("bottom_solver_iterations") > 0, (name, k)
        assert B.member(k).get_option("bottom_solves_one_launch") == L.get_option("bottom_solves_one_launch") == 3 + n
        L.close()
    B.close()


def test_solve_members_leave_at_their_own_cycle(oracle, hip):
    """the solve inputs of test_gpu_batch with num_bottom = 2: the members stop after different cycle counts, each with the oracle's count,
    norm and fields; one read-back for the initial norms and one per cycle of the slowest member"""
    nx, ny = 128, 64
    sp = dict(SOLVE_SP, num_bottom=2)
    f0 = solve_inputs(nx, ny, 0)[0]
    n = len(SOLVE_MEMBERS)
    B = hip.HipBatch(n, nx, ny, f0["dx"], f0["dy"], sy.A3_BC, sy.A3_PHYS, bottom_solver=True)
    load_solve(B, hip, nx, ny, range(n))
    want = []
    for k in range(n):
        f, ph = solve_inputs(nx, ny, k)
        O = oracle.OracleLevel(nx, ny, f["dx"], f["dy"], sy.A3_BC, ph, 0.0, -1.0, 64, 4)
        O.set_inputs(f); O.build_mg_coefficients()
        it, hist = O.solve(sp)
        want.append((O, it, hist))
    counts = [w[1] for w in want]
    assert len(set(counts)) >= 3, ("the oracle's cycle counts must differ between members", counts)
    iters, res = B.solve(sp)
    print("cycles per member: oracle", counts, "batch", iters, "read-backs", B.get_option("batch_readbacks"))
    assert iters == counts
    for k, (O, it, hist) in enumerate(want):
        assert res[k] == hist[-1], (k, res[k], hist[-1])
        G = B.member(k)
        assert np.array_equal(G.get(hip.F_PHI), O.get(oracle.F_PHI)), k
        gr.level_ring_equal(O.get(oracle.F_PHI, ghosted=True), G.get(hip.F_PHI, ghosted=True), (nx, ny), sy.A3_BC["periodic"], what=("solve", k))
        assert np.array_equal(G.get(hip.F_RES), O.get(oracle.F_RES)), k
        for d in range(1, G.ndepth):
            assert np.array_equal(G.get(hip.F_PHI, depth=d), O.get(oracle.F_PHI, depth=d)), (k, d)
        assert G.get_option("bottom_solves_one_launch") == it and G.get_option("bottom_solver_iterations") > 0, k
    assert B.get_option("batch_readbacks") == 1 + max(counts)
    assert B.get_option("batch_member_cycles") == sum(counts) == B.get_option("bottom_solves_one_launch")
    B.close()


def test_active_flags_and_composition(oracle, hip):
    """members 0, 2, 4 of the five: flagged in a batch of 5 and as a batch of 3, two V-cycles and a solve -- the same bits, the oracle's; the
    members not flagged keep their state and their counters"""
    case = VCYCLE_CASES[0]
    name, kind, nx, ny, bc0, alpha, max_box, ndepth = case
    pick = [0, 2, 4]
    B5, B3 = batch(hip, 5, case), batch(hip, 3, case)
    load_members(B5, kind, nx, ny)
    Os = load(B3, oracle.OracleLevel, kind, nx, ny, bc0, alpha, max_box, members=pick)
    before = {k: B5.member(k).get(hip.F_PHI, ghosted=True) for k in (1, 3)}
    for _ in range(2):
        B5.vcycle(SP, active=[1, 0, 1, 0, 1]); B3.vcycle(SP)
        for O, _, _ in Os:
            O.vcycle(SP)
    for q, k in enumerate(pick):
        O, f, bc = Os[q]
        same_member(oracle, hip, O, B3.member(q), f, bc, ("batch of 3", k), relaxed_last=True)
        assert np.array_equal(B5.member(k).get(hip.F_PHI, ghosted=True), B3.member(q).get(hip.F_PHI, ghosted=True)), k
        for d in range(1, ndepth):
            for fld in (hip.F_PHI, hip.F_RHS, hip.F_RES):
                assert np.array_equal(B5.member(k).get(fld, depth=d), B3.member(q).get(fld, depth=d)), (k, d, fld)
        assert B5.member(k).get_option("bottom_solver_iterations") == B3.member(q).get_option("bottom_solver_iterations") > 0
        assert B5.member(k).get_option("bottom_solves_one_launch") == 2
    for k in (1, 3):
        assert np.array_equal(B5.member(k).get(hip.F_PHI, ghosted=True), before[k]), k
        assert B5.member(k).get_option("bottom_solves_one_launch") == 0 and B5.member(k).get_option("bottom_solver_iterations") == 0
    assert B5.get_option("batch_member_cycles") == 6 == B5.get_option("bottom_solves_one_launch")
    B5.close(); B3.close()


def test_depth_0_as_the_bottom(oracle, hip):
    """max_depth = 0 at 32 x 16: the cycle is the bottom relaxes and RelaxSolver on depth 0, and the ghost ring it leaves is the inhomogeneous
    fill of RelaxSolver's last residual evaluation"""
    kind, nx, ny, bc0, alpha = "mixedbc", 32, 16, sy.RANDOM_BC, 0.6
    sp = dict(SP, max_depth=0)
    f0 = member_inputs(kind, nx, ny, 0)[0]
    B = hip.HipBatch(3, nx, ny, f0["dx"], f0["dy"], bc0, sy.A3_PHYS, alpha=alpha, max_box=16, bottom_solver=True)
    T = hip.HipBatch(3, nx, ny, f0["dx"], f0["dy"], bc0, sy.A3_PHYS, alpha=alpha, max_box=16)
    Os = load(B, oracle.OracleLevel, kind, nx, ny, bc0, alpha, 16)
    load_members(T, kind, nx, ny)
    B.vcycle(sp); T.vcycle(sp)
    for k, (O, f, bc) in enumerate(Os):
        O.vcycle(sp)
        G = B.member(k)
        assert np.array_equal(G.get(hip.F_PHI), O.get(oracle.F_PHI)), k
        gr.level_ring_equal(O.get(oracle.F_PHI, ghosted=True), G.get(hip.F_PHI, ghosted=True), (nx, ny), bc["periodic"], what=("depth-0 bottom", k))
        assert np.array_equal(G.get(hip.F_RES), O.get(oracle.F_RES)), (k, "the residual RelaxSolver ended on")
        assert not np.array_equal(G.get(hip.F_PHI), T.member(k).get(hip.F_PHI)), k
        assert G.get_option("bottom_solves_one_launch") == 1 and G.get_option("bottom_solver_iterations") > 0
    iters, res = B.solve(sp)
    for k, (O, f, bc) in enumerate(Os):
        it, hist = O.solve(sp)
        assert iters[k] == it and res[k] == hist[-1], k
        assert np.array_equal(B.member(k).get(hip.F_PHI), O.get(oracle.F_PHI)), k
        gr.level_ring_equal(O.get(oracle.F_PHI, ghosted=True), B.member(k).get(hip.F_PHI, ghosted=True), (nx, ny), bc["periodic"], what=("depth-0 bottom, solve", k))
    B.close(); T.close()


def test_timesteps_with_the_implicit_gap_solve(oracle, hipmodel):
    """A3 (explicit), B1 and B5 as the reference runs them (implicit gap solve) and B5 with the explicit update in one batch at 320 x 64, steps 1-51
    (cur_step = 50: numBottom of the head solve and imin of the gap solve change): Picard iterations and V-cycles of every member are
    or_model_timestep's at every step, fields and rings at steps 1, 2, 3, 49, 50, 51; head solves and gap solves both ran RelaxSolver"""
    import json
    import os
    binp = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shmip_B_inputs.json")))
    from suhmo_amd import level as lv
    nx, ny = 320, 64
    st = sy.shmip_initial_state(nx, ny)

    def b_member(case, **changes):
        b = binp[case]
        src = oracle.moulin_source(nx, ny, st["dx"], st["dy"], np.array(b["positions"]).reshape(-1, 2), b["sigma"], b["flux"], 1.0)[0]
        return dict(sy.shmip_b_model(case, b), **changes), src

    members = [(sy.shmip_a_model("A3"), None), b_member("B1"), b_member("B5"), b_member("B5", use_impl_diff=0)]
    assert [m.get("use_impl_diff", 0) for m, _ in members] == [0, 1, 1, 0]
    n = len(members)
    G = hipmodel.HipBatchModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, [m for m, _ in members], max_box=64, implicit_gap=True, bottom_solver=True)
    assert G.get_option("bottom_solver") == 1
    Os = []
    for k, (m, src) in enumerate(members):
        O = oracle.OracleModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=64, nthreads=4)
        O.set_state(st); G.set_state(k, st)
        if src is not None:
            O.field(oracle.OM_MSRC)[1:-1, 1:-1] = src
            G.member(k).level.set(lv.F_MSRC, src)
        Os.append(O)
    seen, gap_cycles, solves, iterations = set(), 0, 0, 0
    for step in range(1, 52):
        pi, nv = G.timestep(3600.0)
        want = [O.timestep(3600.0) for O in Os]
        assert list(zip(pi, nv)) == want, (step, list(zip(pi, nv)), want)
        seen.update(want)
        if step in (1, 2, 3, 49, 50, 51):
            for k in range(n):
                same_step_fields(oracle, Os[k], G, k, nx, ny, sy.A3_BC["periodic"], ("step", step, "member", k))
            now = (G.get_option("batch_gap_member_cycles"), G.get_option("bottom_solves_one_launch"), G.get_option("bottom_solver_iterations"))
            assert now[0] > gap_cycles and now[1] > solves and now[2] > iterations, (step, now, gap_cycles, solves, iterations)
            gap_cycles, solves, iterations = now
    # every V-cycle of a head solve and of a gap solve ended with one RelaxSolver solve of each of its members
    assert solves == G.get_option("batch_member_cycles") + gap_cycles
    heads = sum(G.member(k).level.get_option("bottom_solves_one_launch") for k in range(n))
    assert heads == G.get_option("batch_member_cycles") and solves > heads
    print("distinct (picard iterations, V-cycles):", sorted(seen), "head / gap member cycles:", heads, gap_cycles, "RelaxSolver iterations:", iterations)
    for O in Os:
        O.close()
    G.close()


def test_launch_count_grows_by_one_and_not_with_members(hip):
    """one V-cycle at 320 x 64 takes the launches of the default batch's + 1 (the RelaxSolver launch), for 1 member and for 6"""
    nx, ny = 320, 64
    f0 = sy.shmip_fields(nx, ny)
    counts = {}
    for n in (1, 6):
        for bottom in (False, True):
            B = hip.HipBatch(n, nx, ny, f0["dx"], f0["dy"], sy.A3_BC, sy.A3_PHYS, bottom_solver=bottom)
            for k in range(n):
                B.member(k).set_inputs(sy.shmip_fields(nx, ny, seed=40 + k)); B.member(k).build_mg_coefficients()
            B.vcycle(sy.SOLVER_DEFAULT)
            counts[n, bottom] = B.get_option("batch_launches")
            assert B.get_option("bottom_solves_one_launch") == (n if bottom else 0)
            B.close()
    print("launches of one batched V-cycle at 320 x 64 (members, bottom_solver):", counts)
    assert counts[1, True] == counts[6, True] == counts[1, False] + 1 == counts[6, False] + 1


def test_interface(oracle, hip):
    from suhmo_amd import capi
    lib = capi.lib()
    case = VCYCLE_CASES[1]
    name, kind, nx, ny, bc0, alpha, max_box, ndepth = case
    f0 = member_inputs(kind, nx, ny, 0)[0]
    d = capi.LevelDesc()
    d.nx, d.ny, d.j0, d.ny_global, d.dx, d.dy = nx, ny, 0, ny, f0["dx"], f0["dy"]
    d.nbox, d.boxes, d.max_box, d.alpha, d.beta = 0, None, max_box, alpha, -1.0
    d.bc, d.phys, d.device, d.halo_rows = hip._bc(bc0), hip._phys(sy.A3_PHYS), 0, 1
    v = C.c_long(-1)
    # NULL and "": suhmo_batch_create
    for opts in (None, b""):
        h = C.c_void_p()
        assert lib.suhmo_batch_create_opts(C.byref(h), C.byref(d), 2, opts) == 0
        assert lib.suhmo_batch_get_option(h, b"bottom_solver", C.byref(v)) == 0 and v.value == 0
        assert lib.suhmo_batch_set_option(h, b"bottom_solver", 0) == 0
        assert lib.suhmo_batch_set_option(h, b"bottom_solver", 1) == -5
        msg = lib.suhmo_last_error()
        assert b"bottom_solver" in msg and b"fixed at creation" in msg, msg
        assert lib.suhmo_batch_size(h) == 2 and lib.suhmo_batch_destroy(h) == 0
    # unknown keys, a value that is no flag
    h = C.c_void_p()
    assert lib.suhmo_batch_create_opts(C.byref(h), C.byref(d), 2, b"no_such_option=1") == -1 and b"no_such_option" in lib.suhmo_last_error()
    assert lib.suhmo_batch_create_opts(C.byref(h), C.byref(d), 2, b"bottom_solver=1,other=2") == -1 and b"other" in lib.suhmo_last_error()
    assert lib.suhmo_batch_create_opts(C.byref(h), C.byref(d), 2, b"bottom_solver=2") == -1
    assert not h.value
    # a bottom the one launch cannot take: 1024 x 1024 with max_box = 8 is 256 x 256 at the bottom (creation only)
    big = capi.LevelDesc()
    C.memmove(C.byref(big), C.byref(d), C.sizeof(d))
    big.nx, big.ny, big.ny_global, big.max_box = 1024, 1024, 1024, 8
    assert lib.suhmo_batch_create_opts(C.byref(h), C.byref(big), 2, b"bottom_solver=1") == -5
    msg = lib.suhmo_last_error()
    assert b"bottom_solver" in msg and b"256 x 256" in msg and b"65536" in msg, msg
    assert not h.value
    # the option on: the creation value is reported, only that value can be "set"
    B = batch(hip, 2, case)
    T = batch(hip, 2, case, bottom_solver=False)
    Os = load(B, oracle.OracleLevel, kind, nx, ny, bc0, alpha, max_box)
    load_members(T, kind, nx, ny)
    assert B.get_option("bottom_solver") == 1 and all(B.member(k).get_option("bottom_solver") == 1 for k in range(2))
    assert lib.suhmo_batch_set_option(B.h, b"bottom_solver", 1) == 0
    assert lib.suhmo_batch_set_option(B.h, b"bottom_solver", 0) == -5
    msg = lib.suhmo_last_error()
    assert b"bottom_solver" in msg and b"fixed at creation" in msg, msg
    for key in (b"bottom_solver_iterations", b"bottom_solves_one_launch"):
        assert lib.suhmo_batch_set_option(B.h, key, 0) == -1 and b"read-only" in lib.suhmo_last_error()
        assert lib.suhmo_batch_get_option(B.h, key, C.byref(v)) == 0 and v.value == 0
    # a member toggled to the other value, in both directions: rc -5 before anything is launched
    sp = hip.solver_params(SP)
    for X, other in ((B, 0), (T, 1)):
        X.member(1).set_option("bottom_solver", other)
        assert lib.suhmo_batch_vcycle(X.h, C.byref(sp), None, None) == -5 and b"bottom_solver" in lib.suhmo_last_error()
        assert lib.suhmo_batch_solve(X.h, C.byref(sp), None, None, None) == -5 and b"bottom_solver" in lib.suhmo_last_error()
        assert X.get_option("batch_launches") == 0 and X.get_option("batch_readbacks") == 0
        X.member(1).set_option("bottom_solver", 1 - other)
    B.vcycle(SP); T.vcycle(SP)                                   # still usable, and still the oracle's
    for k, (O, f, bc) in enumerate(Os):
        O.vcycle(SP)
        same_member(oracle, hip, O, B.member(k), f, bc, ("after refusals", k), relaxed_last=True)
        assert not np.array_equal(B.member(k).get(hip.F_PHI), T.member(k).get(hip.F_PHI)), k
    assert B.get_option("bottom_solves_one_launch") == 2 and T.get_option("bottom_solves_one_launch") == 0
    B.close(); T.close()
