"""The implicit gap-height solve of a batch (batch option implicit_gap: members with use_impl_diff = 1, SolveForGap_nl as one launch sequence for
all of them).  Every member against a run of that member ALONE -- the CPU oracle's time loop, or suhmo_level_timestep on a level of its own --
with np.array_equal throughout: the arithmetic is the solo path's, there is no tolerance to choose.  SHMIP suites B and E as the reference runs
them (solver.use_ImplDiff = true), mixed with forward-Euler members, changing step sizes, and the whole suite-B run against the reference's table."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests.test_gpu_batch import same_step_fields

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEP_FIELDS = ("head", "B", "mR", "Re", "Pw", "qwx", "qwy", "cd", "rhs_h")


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


@pytest.fixture(scope="module")
def binp():
    return json.load(open(os.path.join(GOLD, "shmip_B_inputs.json")))


def b_member(oracle, binp, case, nx=320, ny=64, **changes):
    """(model, moulin source array) of suite B's case as the reference runs it: implicit gap-height solve, the oracle's source array"""
    st = sy.shmip_initial_state(nx, ny)
    b = binp[case]
    src = oracle.moulin_source(nx, ny, st["dx"], st["dy"], np.array(b["positions"]).reshape(-1, 2), b["sigma"], b["flux"], 1.0)[0]
    return dict(sy.shmip_b_model(case, b), **changes), src


def b_batch(hipmodel, members, nx=320, ny=64, phys=sy.A3_PHYS, implicit_gap=True, state=None):
    """a batch of (model, source) members on the SHMIP initial state"""
    from suhmo_amd import level as lv
    st = state or sy.shmip_initial_state(nx, ny)
    G = hipmodel.HipBatchModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, phys, [m for m, _ in members], max_box=64, implicit_gap=implicit_gap)
    for k, (_, src) in enumerate(members):
        G.set_state(k, st)
        if src is not None:
            G.member(k).level.set(lv.F_MSRC, src)
    return G


def solo(hipmodel, member, nx=320, ny=64, phys=sy.A3_PHYS, state=None):
    from suhmo_amd import level as lv
    st = state or sy.shmip_initial_state(nx, ny)
    L = hipmodel.HipModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, phys, member[0], max_box=64)
    L.set_state(st)
    if member[1] is not None:
        L.level.set(lv.F_MSRC, member[1])
    return L


def same_as_solo(G, k, L, what):
    for nm in STEP_FIELDS:
        assert np.array_equal(G.get(k, nm), L.get(nm), equal_nan=True), (what, nm)
    assert np.array_equal(G.get(k, "head", ghosted=True), L.get("head", ghosted=True)), (what, "ghosted head")
    a, b = L.get("B", ghosted=True), G.get(k, "B", ghosted=True)
    assert np.array_equal(a[1:-1, :], b[1:-1, :]) and np.array_equal(a[:, 1:-1], b[:, 1:-1]), (what, "ghosts of the gap height")


def test_suite_b_as_the_reference_runs_it_mixed_with_the_rest(oracle, hipmodel, binp):
    """one batch at 320 x 64: B1-B5 (implicit), A3 (explicit, no diffusion), B5 with the explicit update, B3 with diffFactor 0.5 (another beta of
    the gap operator).  Steps 1-51: (Picard iterations, V-cycles) of every member equal the oracle's at every step; at steps 1, 2, 3, 49, 50, 51
    (50: imin of the gap solve changes) so do all fields and rings.  The gap solve ran, batched: batch_gap_member_cycles grows every step."""
    nx, ny = 320, 64
    st = sy.shmip_initial_state(nx, ny)
    members = [b_member(oracle, binp, c) for c in ("B1", "B2", "B3", "B4", "B5")]
    members.append((sy.shmip_a_model("A3"), None))
    members.append(b_member(oracle, binp, "B5", use_impl_diff=0))
    members.append(b_member(oracle, binp, "B3", diffFactor=0.5))
    n = len(members)
    G = b_batch(hipmodel, members)
    Os = []
    for m, src in members:
        O = oracle.OracleModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=64, nthreads=4)
        O.set_state(st)
        if src is not None:
            O.field(oracle.OM_MSRC)[1:-1, 1:-1] = src
        Os.append(O)
    seen, gap_cycles = set(), 0
    for step in range(1, 52):
        pi, nv = G.timestep(3600.0)
        want = [O.timestep(3600.0) for O in Os]
        assert list(zip(pi, nv)) == want, (step, list(zip(pi, nv)), want)
        seen.update(want)
        now = G.get_option("batch_gap_member_cycles")
        assert now >= gap_cycles + 2 * 6, (step, now, gap_cycles)          # iter_min = 2 cycles of each of the 6 implicit members at least
        gap_cycles = now
        if step in (1, 2, 3, 49, 50, 51):
            for k in range(n):
                same_step_fields(oracle, Os[k], G, k, nx, ny, sy.A3_BC["periodic"], ("step", step, "member", k))
    print("distinct (picard iterations, V-cycles):", sorted(seen), "gap member cycles:", gap_cycles)
    assert len(seen) > 1
    for O in Os:
        O.close()
    G.close()


def test_suite_e_in_one_batch(oracle, hipmodel):
    """E1-E5 at 256 x 64 (valley glacier, ice margin, masked gradients and right-hand side, diffusion + implicit gap solve), the ice-free gap
    height frozen on E1, E3, E5 and evolving on E2, E4: 30 steps, counts every step and the fields at the end against the oracle per member"""
    from suhmo_amd import level as lv
    cases = ("E1", "E2", "E3", "E4", "E5")
    models = [dict(sy.shmip_e_model(c), freeze_icefree_gap=1 if c in ("E1", "E3", "E5") else 0) for c in cases]
    m0 = models[0]
    nx, ny = m0["nx"], m0["ny"]
    states = [sy.valley_initial_state(nx, ny, sy.E_GAMMA[c], m0["lx"], m0["ly"]) for c in cases]
    phys = [dict(sy.E_PHYS, cutOffB=sy.E_CUTOFFB[c]) for c in cases]
    G = hipmodel.HipBatchModel(nx, ny, states[0]["dx"], states[0]["dy"], sy.A3_BC, phys, models, max_box=64, implicit_gap=True)
    Os = []
    v = lambda a: np.array(a)[1:-1, 1:-1]
    for k, c in enumerate(cases):
        O = oracle.OracleModel(nx, ny, states[k]["dx"], states[k]["dy"], sy.A3_BC, phys[k], models[k], max_box=64, nthreads=4)
        O.set_state(states[k]); G.set_state(k, states[k])
        O.field(oracle.OM_MR)[:] = models[k]["G"] / models[k]["L"]
        G.member(k).level.set(lv.F_MR, np.full((ny, nx), models[k]["G"] / models[k]["L"]))
        mask = v(O.field(oracle.OM_MASK))
        assert (mask < 0).sum() > 1000 and (mask > 0).sum() > 1000, (c, int((mask < 0).sum()), int((mask > 0).sum()))
        Os.append(O)
    for step in range(30):
        pi, nv = G.timestep(m0["dt"])
        want = [O.timestep(m0["dt"]) for O in Os]
        assert list(zip(pi, nv)) == want, (step, list(zip(pi, nv)), want)
    for k, c in enumerate(cases):
        same_step_fields(oracle, Os[k], G, k, nx, ny, sy.A3_BC["periodic"], ("suite E", c))
        icefree = states[k]["mask"][1:-1, 1:-1] < 0
        kept = np.array_equal(G.get(k, "B")[icefree], states[k]["B"][1:-1, 1:-1][icefree])
        assert kept == bool(models[k]["freeze_icefree_gap"]), (c, kept)
    assert G.get_option("batch_gap_member_cycles") >= 30 * 5 * 2
    for O in Os:
        O.close()
    G.close()


def test_step_size_changes(oracle, hipmodel, binp):
    """dt = 3600, 3600, 7200, 7200, 3600: the gap operators take the new beta (no rebuild), the tables follow; against three models stepped alone"""
    members = [b_member(oracle, binp, "B2"), b_member(oracle, binp, "B4", diffFactor=0.25), b_member(oracle, binp, "B5")]
    G = b_batch(hipmodel, members)
    Ls = [solo(hipmodel, m) for m in members]
    for step, dt in enumerate((3600.0, 3600.0, 7200.0, 7200.0, 3600.0)):
        pi, nv = G.timestep(dt)
        assert list(zip(pi, nv)) == [L.timestep(dt) for L in Ls], (step, dt)
        for k, L in enumerate(Ls):
            same_as_solo(G, k, L, ("step", step, "dt", dt, "member", k))
    for L in Ls:
        L.close()
    G.close()


def test_batch_of_one_and_member_interop(oracle, hipmodel, hip, binp):
    """an implicit batch of 1 equals HipModel.timestep (fields, ghosted head, both post-processing tables); a gap height stored through the
    member handle is what the next step's solve starts from"""
    member = b_member(oracle, binp, "B3")
    G, L = b_batch(hipmodel, [member]), solo(hipmodel, member)
    for step in range(4):
        pi, nv = G.timestep(3600.0)
        assert (pi[0], nv[0]) == L.timestep(3600.0), step
        same_as_solo(G, 0, L, ("step", step))
        assert np.array_equal(G.postproc_table_device(0), L.postproc_table_device(), equal_nan=True)
        assert np.array_equal(G.postproc_table(0), L.postproc_table(), equal_nan=True)
    assert G.get_option("batch_gap_member_cycles") > 0
    b = L.get("B", ghosted=True) * 1.5
    G.member(0).level.set(hip.F_B, b, ghosted=True); L.level.set(hip.F_B, b, ghosted=True)
    before = L.get("B")
    pi, nv = G.timestep(3600.0)
    assert (pi[0], nv[0]) == L.timestep(3600.0)
    same_as_solo(G, 0, L, "after a stored gap height")
    assert not np.array_equal(L.get("B"), before)
    G.close(); L.close()


def test_composition_independence(oracle, hipmodel, binp):
    """member B2's fields after 5 steps do not depend on who else is in the batch, nor on its place in it"""
    mem = {c: b_member(oracle, binp, c) for c in ("B1", "B2", "B4", "B5")}
    mem["A3"] = (sy.shmip_a_model("A3"), None)
    got = []
    for names in (("B2",), ("B1", "B2", "A3"), ("B5", "B4", "B2", "B1")):
        G = b_batch(hipmodel, [mem[c] for c in names])
        k = names.index("B2")
        counts = [G.timestep(3600.0) for _ in range(5)]
        got.append(([(pi[k], nv[k]) for pi, nv in counts], {nm: G.get(k, nm, ghosted=(nm in ("head", "B"))) for nm in STEP_FIELDS}))
        G.close()
    for other in got[1:]:
        assert other[0] == got[0][0]
        for nm in STEP_FIELDS:
            assert np.array_equal(other[1][nm], got[0][1][nm], equal_nan=True), nm


def test_launches_do_not_grow_with_members(oracle, hipmodel, binp):
    """an implicit step of 6 identical members issues exactly the launches and read-backs of a step of 1"""
    member = b_member(oracle, binp, "B3")
    counts = {}
    for n in (1, 6):
        G = b_batch(hipmodel, [member] * n)
        G.timestep(3600.0)
        counts[n] = (G.get_option("batch_launches"), G.get_option("batch_readbacks"), G.get_option("batch_gap_member_cycles") // n)
        G.close()
    print("(launches, read-backs, gap V-cycles per member) of the first implicit step at 320 x 64:", counts)
    assert counts[1] == counts[6] and counts[1][0] > 0 and counts[1][2] > 0


def test_nothing_moves_when_it_is_off_or_unused(oracle, hipmodel, binp):
    """the option is off on a new batch; on, with explicit members only, it changes neither a field nor the number of launches"""
    members = [(sy.shmip_a_model("A3"), None), b_member(oracle, binp, "B5", use_impl_diff=0), b_member(oracle, binp, "B1", use_impl_diff=0)]
    on, off = b_batch(hipmodel, members, implicit_gap=True), b_batch(hipmodel, members, implicit_gap=False)
    assert off.get_option("implicit_gap") == 0 and on.get_option("implicit_gap") == 1
    for step in range(3):
        assert on.timestep(3600.0) == off.timestep(3600.0)
    for k in range(len(members)):
        for nm in STEP_FIELDS:
            assert np.array_equal(on.get(k, nm, ghosted=(nm in ("head", "B"))), off.get(k, nm, ghosted=(nm in ("head", "B"))), equal_nan=True), (k, nm)
    assert on.get_option("batch_launches") == off.get_option("batch_launches") > 0
    assert on.get_option("batch_readbacks") == off.get_option("batch_readbacks")
    assert on.get_option("batch_gap_member_cycles") == 0
    on.close(); off.close()


def test_refusals(oracle, hipmodel, binp):
    """option on, a member with use_impl_diff = 1 and diffFactor = 0: rc -1, nothing launched, the batch usable afterwards; the counter is read-only"""
    from suhmo_amd import capi
    lib = capi.lib()
    members = [b_member(oracle, binp, "B1"), b_member(oracle, binp, "B4")]
    G, S = b_batch(hipmodel, members), b_batch(hipmodel, members)
    G.set_model(1, diffFactor=0.0)
    pi, nv = (C.c_int * 2)(), (C.c_int * 2)()
    assert lib.suhmo_batch_timestep(G.batch.h, G._mp, 3600.0, 1, pi, nv, None) == -1 and b"diffFactor" in lib.suhmo_last_error()
    assert G.get_option("batch_launches") == 0 and G.get_option("batch_gap_member_cycles") == 0
    assert lib.suhmo_batch_set_option(G.batch.h, b"batch_gap_member_cycles", 0) == -1 and b"read-only" in lib.suhmo_last_error()
    assert lib.suhmo_batch_set_option(G.batch.h, b"implicit_gap", 2) == -1
    G.set_model(1, diffFactor=members[1][0]["diffFactor"])
    for step in range(2):
        assert G.timestep(3600.0) == S.timestep(3600.0)
    for k in range(2):
        for nm in STEP_FIELDS:
            assert np.array_equal(G.get(k, nm), S.get(k, nm), equal_nan=True), (k, nm)
    G.close(); S.close()


def test_the_whole_suite_b_run_in_one_batch(oracle, hipmodel, binp):
    """exec/B_SHMIP/B1 ... B5, 10002 steps each, as ONE batch with the run-state settings of the reference's tables (head_melt_off,
    use_mask_gradients, melt rate preloaded: test_gpu_timestep.test_device_reproduces_the_reference_table).  Per member: the reference's
    committed results/postproc.dat to the pin tolerances, the Picard / V-cycle totals of the oracle's committed pin run, its table to 1e-9"""
    from suhmo_amd import level as lv
    from test_oracle_timeloop import check_against_reference
    cases = ("B1", "B2", "B3", "B4", "B5")
    members = [b_member(oracle, binp, c, head_melt_off=1, freeze_icefree_gap=0) for c in cases]
    m0 = members[0][0]
    nx, ny = m0["nx"], m0["ny"]
    st = sy.shmip_initial_state(nx, ny, m0["lx"], m0["ly"])
    G = b_batch(hipmodel, members, nx, ny, phys=dict(sy.A3_PHYS, use_mask_gradients=1), state=st)
    for k in range(len(cases)):
        G.member(k).level.set(lv.F_MR, np.full((ny, nx), members[k][0]["G"] / members[k][0]["L"]))
    tot = np.zeros((len(cases), 2), dtype=np.int64)
    for step in range(m0["max_step"] + 2):
        pi, nv = G.timestep(m0["dt"])
        tot[:, 0] += pi
        tot[:, 1] += nv
    tables = []
    for k, (m, src) in enumerate(members):
        mask = G.get(k, "mask")
        tables.append(sy.shmip_postproc_table(st["dx"], st["dy"], G.get(k, "qwx"), G.get(k, "cd", ghosted=True),
                                              np.where(mask > 0.0, src * m["ramp"] + m["distributed_input"], 0.0),
                                              G.get(k, "mR"), G.get(k, "Pw"), G.get(k, "Pi"), mask, m["rho_w"]))
    print("gap member cycles of the run:", G.get_option("batch_gap_member_cycles"), "totals:", tot.tolist())
    G.close()
    for k, case in enumerate(cases):
        check_against_reference(tables[k], case, "pin")
        orc = np.loadtxt(os.path.join(GOLD, "shmip_%s_oracle_pin_table.dat" % case))
        run = json.load(open(os.path.join(GOLD, "shmip_%s_oracle_pin.json" % case)))
        assert (int(tot[k, 0]), int(tot[k, 1])) == (run["picard_total"], run["vcycles_total"]), case
        scale = np.max(np.abs(orc), axis=0)
        assert np.all(np.abs(tables[k] - orc) <= 1e-9 * scale), (case, np.max(np.abs(tables[k] - orc) / scale, axis=0))
