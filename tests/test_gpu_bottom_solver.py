"""The bottom solver of the FAS V-cycle (level option bottom_solver = 1): Chombo's RelaxSolver after the bottom relaxes, as every head
solve and the implicit gap solve of the reference configure it (src/AmrHydro.cpp:623,628,726,733-735).  The oracle runs the same loop
under SUHMO_ORACLE_BOTTOM=1 (oracle/level_shim.c, fas_cycle).  Bar: bitwise, as in test_gpu_parity; the l2 norms of the loop's break
test are summed in another order on the device (one-launch kernel: a fixed tree in LDS; host loop: suhmo_level_norm), which only a
near-tie at a break test could show."""
import os

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import ghostring as gr
from test_gpu_parity import same_ring

pytestmark = pytest.mark.gpu

PARITY_CASES = [
    ("random-mixedbc", lambda: sy.random_fields(48, 32), sy.RANDOM_BC, sy.RANDOM_PHYS, 0.7, -1.0, 16),
    ("random-yperiodic", lambda: sy.random_fields(64, 32, seed=3), sy.CONV_BC, sy.RANDOM_PHYS, 0.0, -1.0, 16),
    ("random-allperiodic", lambda: sy.random_fields(32, 32, seed=5),
     dict(type=[[0, 0], [0, 0]], value=[[0, 0], [0, 0]], periodic=[1, 1]), sy.RANDOM_PHYS, 0.25, -1.0, 8),
    ("ragged-odd", lambda: sy.random_fields(50, 34, seed=9), sy.RANDOM_BC, sy.RANDOM_PHYS, 0.0, -1.0, 64),
    ("shmip-a3", lambda: sy.shmip_fields(128, 64), sy.A3_BC, sy.A3_PHYS, 0.0, -1.0, 64),
    ("no-nl", lambda: sy.random_fields(32, 16, seed=2), sy.A3_BC, dict(sy.RANDOM_PHYS, use_NL=0), 0.0, -1.0, 16),
]


@pytest.fixture(scope="module")
def hip():
    from suhmo_amd import capi, level
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return level


def pair(oracle, hip, case, bottom=1, need_b=True, max_box=None):
    _, mk, bc, ph, alpha, beta, mb = case
    f = mk()
    mb = max_box or mb
    O = oracle.OracleLevel(f["nx"], f["ny"], f["dx"], f["dy"], bc, ph, alpha, beta, mb, 2)
    G = hip.HipLevel(f["nx"], f["ny"], f["dx"], f["dy"], bc, ph, alpha, beta, mb)
    if bottom:
        G.set_option("bottom_solver", 1)
    O.set_inputs(f); G.set_inputs(f)
    if need_b and "bx" not in f:
        O.update_operator(); G.update_operator()
    O.build_mg_coefficients(); G.build_mg_coefficients()
    return f, O, G


def test_options_and_defaults(hip):
    f = sy.random_fields(32, 16, seed=2)
    G = hip.HipLevel(f["nx"], f["ny"], f["dx"], f["dy"], sy.A3_BC, sy.RANDOM_PHYS, 0.0, -1.0, 16)
    assert G.get_option("bottom_solver") == 0
    assert G.get_option("bottom_one_launch_max_cells") == 16384
    G.set_option("bottom_solver", 1)
    assert G.get_option("bottom_solver") == 1
    for k in ("bottom_solver_iterations", "bottom_solves_one_launch", "bottom_solves_host_loop"):
        assert G.get_option(k) == 0
    with pytest.raises(Exception):
        G.set_option("bottom_solver", 2)
    G.close()


@pytest.mark.parametrize("case", PARITY_CASES, ids=[c[0] for c in PARITY_CASES])
def test_vcycle_and_solve_bitwise(oracle, hip, case, monkeypatch):
    """V-cycle and solve with the bottom solver against the oracle's SUHMO_ORACLE_BOTTOM=1: head, depth-0 residual, cycle count and
    residual history bit for bit; the result is not the plain cycle's (two bottom relaxes: sixteen solve these few-cell bottoms to rounding
    already, and RelaxSolver then stops after one iteration that changes no bit)"""
    monkeypatch.setenv("SUHMO_ORACLE_BOTTOM", "1")
    sp = dict(sy.SOLVER_DEFAULT, num_bottom=2, eps=1e-10, norm_thresh=1e-13, max_iter=8, imin=10)
    f, O, G = pair(oracle, hip, case)
    _, _, G0 = pair(oracle, hip, case, bottom=0)
    O.vcycle(sp); G.vcycle(sp); G0.vcycle(sp)
    a, b = G.get(hip.F_PHI), O.get(oracle.F_PHI)
    assert np.array_equal(a, b), float(np.max(np.abs(a - b)))
    # (a level of one depth ends its cycle on RelaxSolver's residual evaluation, not on a relaxation)
    same_ring(O, G, oracle, hip, f, case[2], (case[0], "vcycle"), relaxed_last=G.ndepth > 1)
    assert not np.array_equal(a, G0.get(hip.F_PHI))
    assert G.get_option("bottom_solver_iterations") > 0
    assert G.get_option("bottom_solves_one_launch") == 1 and G.get_option("bottom_solves_host_loop") == 0
    no, ho = O.solve(sp)
    ng, hg = G.solve(sp)
    assert no == ng and np.array_equal(ho, hg), (ho, hg)
    assert np.array_equal(G.get(hip.F_PHI), O.get(oracle.F_PHI))
    same_ring(O, G, oracle, hip, f, case[2], (case[0], "solve"))
    O.residual(); G.residual()
    assert np.array_equal(G.get(hip.F_RES), O.get(oracle.F_RES))
    O.close(); G.close(); G0.close()


def solve_1024(oracle, hip, max_box, host_loop=False, with_oracle=True):
    n = 1024
    f = sy.shmip_fields(n, n, ly=1.0e5)
    f.pop("bx", None); f.pop("by", None)
    G = hip.HipLevel(n, n, f["dx"], f["dy"], sy.A3_BC, sy.A3_PHYS, max_box=max_box)
    G.set_option("bottom_solver", 1)
    if host_loop:
        G.set_option("bottom_one_launch_max_cells", 0)
    G.set_inputs(f); G.build_mg_coefficients()
    sp = dict(sy.SOLVER_DEFAULT)
    ng, hg = G.solve(sp)
    out = dict(n=ng, hist=hg, phi=G.get(hip.F_PHI), ghosted=G.get(hip.F_PHI, ghosted=True), iters=G.get_option("bottom_solver_iterations"),
               one=G.get_option("bottom_solves_one_launch"), host=G.get_option("bottom_solves_host_loop"), ndepth=G.ndepth)
    G.close()
    if with_oracle:
        O = oracle.OracleLevel(n, n, f["dx"], f["dy"], sy.A3_BC, sy.A3_PHYS, max_box=max_box, nthreads=min(16, os.cpu_count() or 1))
        O.set_inputs(f); O.build_mg_coefficients()
        no, ho = O.solve(sp)
        out["oracle"] = (no, ho, O.get(oracle.F_PHI), O.get(oracle.F_PHI, ghosted=True))
        O.close()
    return out


@pytest.mark.parametrize("max_box,bottom_cells,one_launch", [(64, 32 * 32, True), (16, 128 * 128, True), (8, 256 * 256, False)])
def test_both_paths_at_1024(oracle, hip, max_box, bottom_cells, one_launch, monkeypatch):
    """the step >= 50 solve of bench.py's converged_solve at 1024^2 with bottoms of 32^2 and 128^2 (one launch) and 256^2 (host loop),
    against the oracle; the one-launch sizes forced onto the host loop give the same bits"""
    monkeypatch.setenv("SUHMO_ORACLE_BOTTOM", "1")
    r = solve_1024(oracle, hip, max_box)
    assert (1024 >> (r["ndepth"] - 1)) ** 2 == bottom_cells
    no, ho, po, pgo = r["oracle"]
    assert no == r["n"] and np.array_equal(ho, r["hist"]), (no, r["n"], ho[-3:], r["hist"][-3:])
    assert np.array_equal(r["phi"], po)
    gr.level_ring_equal(pgo, r["ghosted"], (1024, 1024), sy.A3_BC["periodic"], what=("solve", max_box))
    assert r["iters"] > 0
    if one_launch:
        assert r["one"] == r["n"] and r["host"] == 0
        h = solve_1024(oracle, hip, max_box, host_loop=True, with_oracle=False)
        assert h["host"] == h["n"] and h["one"] == 0
        assert h["n"] == r["n"] and np.array_equal(h["hist"], r["hist"]) and np.array_equal(h["phi"], r["phi"])
        gr.level_ring_equal(pgo, h["ghosted"], (1024, 1024), sy.A3_BC["periodic"], what=("solve, host loop", max_box))
        assert h["iters"] == r["iters"]
    else:
        assert r["host"] == r["n"] and r["one"] == 0


@pytest.mark.parametrize("max_depth", [0, 2])
def test_max_depth_bitwise(oracle, hip, max_depth, monkeypatch):
    """a shallow cycle at 256^2 (depth 0 as the bottom: the ghost fill and the residual the cycle leaves for the solve loop)"""
    monkeypatch.setenv("SUHMO_ORACLE_BOTTOM", "1")
    n = 256
    f = sy.shmip_fields(n, n, ly=1.0e5)
    O = oracle.OracleLevel(n, n, f["dx"], f["dy"], sy.A3_BC, sy.A3_PHYS, max_box=64, nthreads=min(16, os.cpu_count() or 1))
    G = hip.HipLevel(n, n, f["dx"], f["dy"], sy.A3_BC, sy.A3_PHYS, max_box=64)
    G.set_option("bottom_solver", 1)
    O.set_inputs(f); G.set_inputs(f)
    O.build_mg_coefficients(); G.build_mg_coefficients()
    sp = dict(sy.SOLVER_DEFAULT, max_depth=max_depth, max_iter=6, imin=10)
    O.vcycle(sp); G.vcycle(sp)
    assert np.array_equal(G.get(hip.F_PHI), O.get(oracle.F_PHI))
    no, ho = O.solve(sp)
    ng, hg = G.solve(sp)
    assert no == ng and np.array_equal(ho, hg), (ho, hg)
    assert np.array_equal(G.get(hip.F_PHI), O.get(oracle.F_PHI))
    O.residual(); G.residual()
    assert np.array_equal(G.get(hip.F_RES), O.get(oracle.F_RES))
    host = max_depth == 0            # the 256^2 bottom does not fit the LDS
    assert (G.get_option("bottom_solves_host_loop") > 0) == host and (G.get_option("bottom_solves_one_launch") > 0) == (not host)
    O.close(); G.close()


def test_graph_replay(hip):
    """three solves at 1024^2 replayed as graphs (default) and eager (graph_max_cells = 0): the same histories, head and iteration count"""
    n = 1024
    f = sy.shmip_fields(n, n, ly=1.0e5)
    f.pop("bx", None); f.pop("by", None)
    sp = dict(sy.SOLVER_DEFAULT)
    res = []
    for graphs in (True, False):
        G = hip.HipLevel(n, n, f["dx"], f["dy"], sy.A3_BC, sy.A3_PHYS, max_box=64)
        G.set_option("bottom_solver", 1)
        if not graphs:
            G.set_option("graph_max_cells", 0)
        G.set_inputs(f); G.build_mg_coefficients()
        hs = []
        for _ in range(3):
            n_, h = G.solve(sp)
            hs.append(h.copy())
        res.append((hs, G.get(hip.F_PHI, ghosted=True), G.get_option("bottom_solver_iterations"), G.get_option("bottom_solves_one_launch")))
        G.close()
    (ha, pa, ia, oa), (hb, pb, ib, ob) = res
    assert all(np.array_equal(x, y) for x, y in zip(ha, hb))
    assert np.array_equal(pa[1:-1, 1:-1], pb[1:-1, 1:-1])
    gr.level_ring_equal(pb, pa, (n, n), sy.A3_BC["periodic"], what="graph replay against eager")
    assert ia == ib > 0 and oa == ob > 0


TS_CASES = [
    ("a3-32x16", 32, 16, sy.A3_BC, sy.A3_PHYS, dict(), 3),
    ("a3-128x32-perturbed", 128, 32, sy.A3_BC, sy.A3_PHYS, dict(), 3),
    ("yperiodic-mask", 64, 32, sy.CONV_BC, dict(sy.A3_PHYS, use_mask_gradients=1, cutOffbr=0.02, maxOffbr=0.08, cutOffB=1),
     dict(use_mask_rhs_b=1, G=0.05), 2),
    ("implicit-gap-changing-dt", 64, 32, sy.A3_BC, sy.A3_PHYS, dict(diffFactor=1.0, use_impl_diff=1), 3),
]


@pytest.mark.parametrize("name,nx,ny,bc,ph,mpo,nsteps", TS_CASES, ids=[c[0] for c in TS_CASES])
def test_timestep_bitwise(oracle, name, nx, ny, bc, ph, mpo, nsteps, monkeypatch):
    """time steps (steps 0..2: cur_step < 50, numBottom = 10) with the bottom solver on the head solve and the implicit gap solve"""
    from suhmo_amd import model
    from test_gpu_timestep import perturbed_state
    monkeypatch.setenv("SUHMO_ORACLE_BOTTOM", "1")
    m = dict(sy.A3_MODEL, **mpo)
    st = sy.shmip_initial_state(nx, ny) if name == "a3-32x16" else perturbed_state(nx, ny, 11, name == "yperiodic-mask")
    O = oracle.OracleModel(nx, ny, st["dx"], st["dy"], bc, ph, m, max_box=16, nthreads=2)
    G = model.HipModel(nx, ny, st["dx"], st["dy"], bc, ph, m, max_box=16)
    G.level.set_option("bottom_solver", 1)
    O.set_state(st); G.set_state(st)
    v = lambda a: np.array(a)[1:-1, 1:-1]
    for k in range(nsteps):
        dt = m["dt"] * (0.5 if k == 1 else 1.0)
        assert O.timestep(dt) == G.timestep(dt), k
        for nm, fid in (("head", oracle.OM_H), ("B", oracle.OM_B), ("mR", oracle.OM_MR), ("Pw", oracle.OM_PW)):
            a, b = v(O.field(fid)), G.get(nm)
            assert np.array_equal(a, b, equal_nan=True), (name, k, nm, float(np.nanmax(np.abs(a - b))))
    it = G.level.get_option("bottom_solver_iterations")
    assert it > 0
    O.close(); G.close()


def test_tutorial_run_first_steps(oracle, monkeypatch):
    """the tutorial run (32 x 8) with the bottom solver: per-step Picard / V-cycle counts equal the oracle's over the first 100 steps; the
    first step takes 4 Picard iterations and 26 V-cycles (profiles/r04_stopping_rule_sweep.txt, row 0 0 0 1)"""
    import ctypes as C
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))
    import convergence_channelized as cc
    from oracle import pyoracle as po
    from suhmo_amd import model
    monkeypatch.setenv("SUHMO_ORACLE_BOTTOM", "1")
    nx, ny = 32, 8
    counts = {}
    for which in ("oracle", "hip"):
        st, m = cc.basic_state(nx, ny), dict(cc.MODEL)
        src, _ = po.moulin_source(nx, ny, st["dx"], st["dy"], cc.MOULIN[0], cc.MOULIN[1], cc.MOULIN[2], 1.0)
        if which == "oracle":
            M = po.OracleModel(nx, ny, st["dx"], st["dy"], cc.BC, cc.PHYS, m, max_box=8, nthreads=1)
            M.set_state(st)
            M.field(po.OM_MR)[:] = m["G"] / m["L"]
            M.field(po.OM_MSRC)[1:-1, 1:-1] = src
        else:
            M = model.HipModel(nx, ny, st["dx"], st["dy"], cc.BC, cc.PHYS, m, max_box=8)
            M.level.set_option("bottom_solver", 1)
            M.set_state(st)
            M.level.set(model.lv.F_MR, np.full((ny, nx), m["G"] / m["L"]))
            M.level.set(model.lv.F_MSRC, src)
        pv = []
        for k in range(100):
            M._mp.ramp = float(cc.ramp(k * m["dt"]))
            if which == "oracle":
                po.lib().or_model_set_ramp(M.h, C.c_double(M._mp.ramp))
            pv.append(M.timestep(m["dt"]))
        M.close()
        counts[which] = np.array(pv)
    assert np.array_equal(counts["hip"], counts["oracle"]), np.where(np.any(counts["hip"] != counts["oracle"], axis=1))[0][:5]
    assert tuple(counts["hip"][0]) == (4, 26), counts["hip"][:3]


def test_hier_vcycle_and_solve_bitwise(oracle, monkeypatch):
    """a hierarchy of box unions: the option set through HipHier.set_option reaches level 0's cycle (the bottom of every AMR V-cycle)"""
    from suhmo_amd.level import F_PHI
    from test_gpu_hier import pair as hpair, same_levels, same_rings, UNION, BC_NP
    monkeypatch.setenv("SUHMO_ORACLE_BOTTOM", "1")
    sp = dict(sy.SOLVER_DEFAULT, eps=1e-9, norm_thresh=1e-14, max_iter=6, imin=30)
    O, G, fs = hpair(oracle, UNION, BC_NP, sy.CFG3_PHYS)
    G.set_option("bottom_solver", 1)
    assert G.get_option("bottom_solver") == 1
    O.vcycle(sp); G.vcycle(sp)
    same_levels(O, G, oracle, ((oracle.F_PHI, F_PHI),), "vcycle")
    same_rings(O, G, oracle, BC_NP, fs, "vcycle", relaxed_last=True)
    no, ho = O.solve(sp)
    ng, hg = G.solve(sp)
    assert no == ng and np.array_equal(ho, hg), (ho, hg)
    same_levels(O, G, oracle, ((oracle.F_PHI, F_PHI),), "solve")
    assert G.get_option("bottom_solver_iterations") > 0
    same_rings(O, G, oracle, BC_NP, fs, "solve", exchange=True)
    O.close(); G.close()


def test_hier_timestep_bitwise(oracle, monkeypatch):
    """time steps on a hierarchy with the implicit gap solve: the hierarchy's gap operator takes the option too"""
    from test_gpu_hier_timestep import make, UNION, B5ISH
    monkeypatch.setenv("SUHMO_ORACLE_BOTTOM", "1")
    m = dict(sy.A3_MODEL, **B5ISH)
    m["use_moulin_source"] = 0
    O, G, sts = make(oracle, UNION, m)
    G.hier.set_option("bottom_solver", 1)
    v = lambda a: np.array(a)[1:-1, 1:-1]
    for step in range(2):
        dt = m["dt"] * (0.5 if step == 1 else 1.0)
        co, cg = O.timestep(dt), G.timestep(dt)
        assert co == cg, (step, co, cg)
        for l in range(O.nlev):
            for k in range(len(O.boxes[l])):
                for nm, fid in (("head", oracle.OM_H), ("B", oracle.OM_B)):
                    a, b = v(O.field(l, k, fid)), G.get(l, k, nm)
                    assert np.array_equal(a, b, equal_nan=True), (step, l, k, nm)
    assert G.hier.get_option("bottom_solver_iterations") > 0
    O.close(); G.close()


def test_strips_agglomerated_bottom_equals_single_canvas(monkeypatch):
    """thread ranks whose coarse depths are agglomerated: the bottom runs in one launch on the whole-level copy, bit for bit the single
    canvas"""
    from suhmo_amd import level as lv
    from test_gpu_strips import run_strips, single, wrap_ghosts
    monkeypatch.setenv("SUHMO_AGG_MIN_CELLS", "2000")
    n, world = 256, 4
    f = wrap_ghosts(sy.shmip_fields(n, n, ly=1.0e5), sy.A3_BC)
    sp = dict(sy.SOLVER_DEFAULT, eps=1e-10, norm_thresh=1e-13, max_iter=4, imin=5)

    def body(G, rank):
        G.set_option("bottom_solver", 1)
        G.build_mg_coefficients()
        n_, hist = G.solve(sp)
        return G.get(lv.F_PHI), n_, hist, G.get_option("bottom_solves_one_launch"), G.get_option("bottom_solves_host_loop")

    parts = run_strips(world, f, sy.A3_BC, sy.A3_PHYS, 0.0, -1.0, body, halo=24, max_box=64)
    s = single(f, sy.A3_BC, sy.A3_PHYS, 0.0, -1.0, body, max_box=64)
    assert np.array_equal(np.vstack([p[0] for p in parts]), s[0])
    assert all(p[1] == s[1] and np.array_equal(p[2], s[2]) for p in parts)
    assert all(p[3] == s[1] and p[4] == 0 for p in parts), [(p[3], p[4]) for p in parts]


def test_strips_host_loop_against_the_oracle(oracle, monkeypatch):
    """thread ranks without agglomeration: the bottom solve runs as the host loop over the strips (halo exchanges, l2 norms reduced over
    the ranks), against the oracle's whole level"""
    from suhmo_amd import level as lv
    from test_gpu_strips import run_strips, wrap_ghosts
    monkeypatch.setenv("SUHMO_AGG_MIN_CELLS", "0")
    monkeypatch.setenv("SUHMO_ORACLE_BOTTOM", "1")
    n, world = 256, 2
    f = wrap_ghosts(sy.shmip_fields(n, n, ly=1.0e5), sy.A3_BC)
    sp = dict(sy.SOLVER_DEFAULT, eps=1e-10, norm_thresh=1e-13, max_iter=4, imin=5)

    def body(G, rank):
        G.set_option("bottom_solver", 1)
        G.build_mg_coefficients()
        n_, hist = G.solve(sp)
        return G.get(lv.F_PHI), n_, hist, G.get_option("bottom_solves_one_launch"), G.get_option("bottom_solves_host_loop")

    parts = run_strips(world, f, sy.A3_BC, sy.A3_PHYS, 0.0, -1.0, body, halo=24, max_box=64)
    O = oracle.OracleLevel(n, n, f["dx"], f["dy"], sy.A3_BC, sy.A3_PHYS, 0.0, -1.0, 64, 4)
    O.set_inputs(f); O.build_mg_coefficients()
    no, ho = O.solve(sp)
    assert np.array_equal(np.vstack([p[0] for p in parts]), O.get(oracle.F_PHI))
    assert all(p[1] == no and np.array_equal(p[2], ho) for p in parts)
    assert all(p[4] == no and p[3] == 0 for p in parts)
    O.close()
