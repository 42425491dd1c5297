"""setAlphaAndBeta / setBC of a whole level (HipLevel.set_alpha_beta, set_bc) between V-cycles that run as replayed HIP graphs.

On one GPU a V-cycle of a small level is, from its second use, a launch of a captured graph, and a captured launch carries the operator's
view (alpha, beta, BC types and values) by value: a setter has to drop the graphs, and the new values have to reach every depth, every
relaxation kernel layout and the one-launch bottom solver.  A stale replay would give a plausible, wrong head.

Bar: bitwise against the oracle, as in test_gpu_parity.  The oracle has no setters: after every setter the reference is a fresh
OracleLevel created with the then-current alpha, beta and BC and handed the old oracle level's state (head, inputs, face coefficients).
Two conditions keep the comparison from passing vacuously: the read-only option vcycle_graph_replays grows in every phase (and stays 0 in
a control run with graph_max_cells = 0, whose bits are the graph run's), and the first cycle after a setter differs from the same cycle
of a twin level that was not given the setter."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from test_gpu_parity import CASES, FUSED_VCYCLE_CASES, same_ring

pytestmark = pytest.mark.gpu

# mixed non-periodic BCs with alpha != 0 (48 x 32 and 256 x 64) and a y-periodic level with alpha = 0: all far below graph_max_cells
SETTER_CASES = [c for c in CASES if c[0] in ("random-mixedbc", "random-yperiodic")] + [c for c in FUSED_VCYCLE_CASES if c[0] == "mixedbc-helmholtz"]
LAYOUTS = [
    ("tile", {}),
    ("colour-passes", dict(gsrb_tile=0, gsrb_variant=0)),
    ("streaming", dict(gsrb_variant=2, fused_min_cells=0)),
    ("bottom-solver", dict(bottom_solver=1)),
]


@pytest.fixture(scope="module")
def hip():
    from suhmo_amd import capi, level
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return level


def other_bc(bc):
    """other types (the two sides of every direction swapped) and other values, the same periodicity"""
    t = [[bc["type"][d][1], bc["type"][d][0]] for d in range(2)]
    v = [[(4.0 + d) if t[d][s] == 0 else 0.015 * (1 + s) for s in range(2)] for d in range(2)]
    return dict(type=t, value=v, periodic=list(bc["periodic"]))


def other_alpha_beta(alpha, beta):
    """both changed, and alpha across zero (the kernels' alpha != 0 arm)"""
    return (0.0 if alpha != 0.0 else 0.7), 2.0 * beta


def make_hip(hip, f, bc, ph, alpha, beta, mb, opts, graphs=True):
    G = hip.HipLevel(f["nx"], f["ny"], f["dx"], f["dy"], bc, ph, alpha, beta, mb)
    for k, v in opts.items():
        G.set_option(k, v)
    if not graphs:
        G.set_option("graph_max_cells", 0)
    return G


def oracle_with(oracle, O, f, bc, ph, alpha, beta, mb):
    """a fresh oracle level with these operator constants, in the state of O (which is closed)"""
    N = oracle.OracleLevel(f["nx"], f["ny"], f["dx"], f["dy"], bc, ph, alpha, beta, mb, 2)
    N.set_inputs(dict(f, phi=O.get(oracle.F_PHI)))
    N.build_mg_coefficients()
    for fid in (oracle.F_BX, oracle.F_BY):
        N.set(fid, O.get(fid))
    O.close()
    return N


def twin_of(hip, G, f, bc, ph, alpha, beta, mb, opts):
    """a second device level in the state of G, with the operator constants G has now"""
    T = make_hip(hip, f, bc, ph, alpha, beta, mb, opts)
    T.set_inputs(dict(f, phi=G.get(hip.F_PHI)))
    T.build_mg_coefficients()
    for fid in (hip.F_BX, hip.F_BY):
        T.set(fid, G.get(fid))
    return T


COARSE = ("F_PHI", "F_RES", "F_RHS")


def compare(O, G, oracle, hip, f, bc, what, relaxed_last=True):
    a, b = G.get(hip.F_PHI), O.get(oracle.F_PHI)
    assert np.array_equal(a, b), (what, "head", float(np.max(np.abs(a - b))))
    same_ring(O, G, oracle, hip, f, bc, what, relaxed_last=relaxed_last)
    for d in range(1, G.ndepth):
        for name in COARSE:
            assert np.array_equal(G.get(getattr(hip, name), depth=d), O.get(getattr(oracle, name), depth=d)), (what, name, "depth", d)


def snapshot(G, hip):
    return [G.get(hip.F_PHI, ghosted=True)] + [G.get(getattr(hip, name), depth=d) for d in range(1, G.ndepth) for name in COARSE]


def run_sequence(oracle, hip, case, opts, sp, graphs, with_oracle):
    """three V-cycles, set_alpha_beta, three V-cycles, set_bc, three V-cycles, everything back, three V-cycles and a solve; returns
    (what the device held after every cycle and the solve, the growth of vcycle_graph_replays in every phase)"""
    _, mk, bc0, ph, a0, b0, mb = case
    f = mk()
    f.pop("bx", None); f.pop("by", None)
    a1, b1 = other_alpha_beta(a0, b0)
    bc1 = other_bc(bc0)
    G = make_hip(hip, f, bc0, ph, a0, b0, mb, opts, graphs)
    G.set_inputs(f); G.build_mg_coefficients()
    O = None
    if with_oracle:
        O = oracle.OracleLevel(f["nx"], f["ny"], f["dx"], f["dy"], bc0, ph, a0, b0, mb, 2)
        O.set_inputs(f); O.build_mg_coefficients()
    assert G.ndepth > 1 and (O is None or O.ndepth == G.ndepth)
    phases = [("start", (a0, b0, bc0)), ("set_alpha_beta", (a1, b1, bc0)), ("set_bc", (a1, b1, bc1)), ("back", (a0, b0, bc0))]
    cur = phases[0][1]
    snaps, grown = [], []
    for name, new in phases:
        T = None
        if name != "start":
            T = twin_of(hip, G, f, cur[2], ph, cur[0], cur[1], mb, opts)        # ... does not get the setter
            if (new[0], new[1]) != (cur[0], cur[1]):
                G.set_alpha_beta(new[0], new[1])
            if new[2] is not cur[2]:
                G.set_bc(new[2])
            cur = new
            if O is not None:
                O = oracle_with(oracle, O, f, cur[2], ph, cur[0], cur[1], mb)
        r0 = G.get_option("vcycle_graph_replays")
        for k in range(3):                                                      # (at the start: eager, captured, replayed)
            G.vcycle(sp)
            if O is not None:
                O.vcycle(sp)
                compare(O, G, oracle, hip, f, cur[2], (case[0], name, "cycle", k))
            if T is not None and k == 0:
                T.vcycle(sp)
                assert not np.array_equal(G.get(hip.F_PHI), T.get(hip.F_PHI)), (case[0], name, "the cycle after the setter is the cycle without it")
                T.close()
            snaps.append(snapshot(G, hip))
        grown.append(G.get_option("vcycle_graph_replays") - r0)
    ng, hg = G.solve(sp)
    if O is not None:
        no, ho = O.solve(sp)
        assert ng == no and np.array_equal(hg, ho), (case[0], "solve", hg, ho)
        compare(O, G, oracle, hip, f, cur[2], (case[0], "solve"), relaxed_last=False)
        O.close()
    snaps.append([np.array([float(ng)]), hg] + snapshot(G, hip))
    if opts.get("bottom_solver"):                                               # (inside the captured cycle: the one-launch solver)
        assert G.get_option("bottom_solves_one_launch") > 0 and G.get_option("bottom_solves_host_loop") == 0
    G.close()
    return snaps, grown


def solver(layout_opts):
    sp = dict(sy.SOLVER_DEFAULT, eps=1e-10, norm_thresh=1e-13, max_iter=3, imin=6)
    if layout_opts.get("bottom_solver"):
        sp["num_bottom"] = 2                     # (sixteen bottom relaxes leave RelaxSolver nothing to do on these few-cell bottoms)
    return sp


@pytest.mark.parametrize("case", SETTER_CASES, ids=[c[0] for c in SETTER_CASES])
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_setters_between_replayed_cycles(oracle, hip, case, layout, monkeypatch):
    """head, ghost ring and the coarse PHI / RES / RHS of every depth equal the oracle's after every cycle of the sequence, on every
    kernel layout; the cycles after a setter are graph launches again and are not the cycles without the setter; with graphs off the
    same bits"""
    opts = layout[1]
    if opts.get("bottom_solver"):
        monkeypatch.setenv("SUHMO_ORACLE_BOTTOM", "1")
    sp = solver(opts)
    snaps, grown = run_sequence(oracle, hip, case, opts, sp, graphs=True, with_oracle=True)
    print("vcycle_graph_replays grew by", grown)
    assert len(grown) == 4 and all(g > 0 for g in grown), grown
    csnaps, cgrown = run_sequence(oracle, hip, case, opts, sp, graphs=False, with_oracle=False)
    assert cgrown == [0, 0, 0, 0], cgrown
    assert len(csnaps) == len(snaps) == 13
    for k, (a, b) in enumerate(zip(snaps, csnaps)):
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), ("graph run and eager run differ at step", k)


def test_set_bc_that_changes_the_periodicity_is_refused(hip):
    from suhmo_amd import capi
    _, mk, bc, ph, alpha, beta, mb = SETTER_CASES[1]                 # y-periodic
    f = mk()
    G = hip.HipLevel(f["nx"], f["ny"], f["dx"], f["dy"], bc, ph, alpha, beta, mb)
    for periodic in ([0, 0], [1, 1], [1, 0]):
        with pytest.raises(capi.SuhmoError, match="periodicity"):
            G.set_bc(dict(other_bc(bc), periodic=periodic))
    G.set_bc(other_bc(bc))                                           # the same periodicity: taken
    G.close()


@pytest.mark.parametrize("case", SETTER_CASES, ids=[c[0] for c in SETTER_CASES])
def test_setters_between_solves_change_the_residual_history_as_the_oracles(oracle, hip, case):
    _, mk, bc0, ph, a0, b0, mb = case
    f = mk()
    f.pop("bx", None); f.pop("by", None)
    sp = solver({})
    G = make_hip(hip, f, bc0, ph, a0, b0, mb, {})
    O = oracle.OracleLevel(f["nx"], f["ny"], f["dx"], f["dy"], bc0, ph, a0, b0, mb, 2)
    for L in (G, O):
        L.set_inputs(f); L.build_mg_coefficients()
    ng, hg = G.solve(sp)
    no, ho = O.solve(sp)
    assert ng == no and np.array_equal(hg, ho), (hg, ho)
    cur = (a0, b0, bc0)
    for name, new in (("set_alpha_beta", other_alpha_beta(a0, b0) + (bc0,)), ("set_bc", other_alpha_beta(a0, b0) + (other_bc(bc0),)), ("back", (a0, b0, bc0))):
        T = twin_of(hip, G, f, cur[2], ph, cur[0], cur[1], mb, {})
        G.set_alpha_beta(new[0], new[1])
        G.set_bc(new[2])
        cur = new
        O = oracle_with(oracle, O, f, cur[2], ph, cur[0], cur[1], mb)
        ng, hg = G.solve(sp)
        no, ho = O.solve(sp)
        nt, ht = T.solve(sp)
        assert ng == no and np.array_equal(hg, ho), (name, hg, ho)
        assert not np.array_equal(hg, ht), (name, "the history is the one without the setter", hg)
        compare(O, G, oracle, hip, f, cur[2], (case[0], name, "solve"), relaxed_last=False)
        T.close()
    G.close(); O.close()
