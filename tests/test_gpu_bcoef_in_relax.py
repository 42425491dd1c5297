"""UpdateOperator of the V-cycle inside the first pre-smoothing launch of depth 0 (level option bcoef_in_relax, default 1; suhmo_gsrb.hip,
k_gsrb_fused<.., BCF>): the launch forms depth 0's face coefficients from the head as loaded and stores them, AverageOperator follows it.
Every case bitwise against the oracle's V-cycle and against the option-off run -- the faces of depth 0 with the level's last face column and
row, the averaged faces of every coarse depth, the head and its ghost ring -- with every depth on the streaming kernel; the counter
bcoef_in_relax_launches says which path ran.  The mode needs a mask that is KNOWN clean: the first cycle of a level scans it (on
k_bcoef_fused), so every case runs one such cycle first and then two in the new mode (the head's two canvases have traded places an odd
number of times in between or not, depending on the depth: the second cycle starts from the other ping-pong state where they have)."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import ghostring as gr

pytestmark = pytest.mark.gpu

PER_BC = dict(type=[[0, 0], [0, 0]], value=[[0, 0], [0, 0]], periodic=[1, 1])
SP = dict(sy.SOLVER_DEFAULT, eps=1e-10, norm_thresh=1e-13, max_iter=3, imin=6)
# name: (fields, boundary conditions, physics, max_box)
CASES = {
    "wide-strips-physical-x": (lambda: sy.random_fields(1100, 48, seed=21), sy.RANDOM_BC, sy.RANDOM_PHYS, 16),   # several strips, physical x sides at both ends
    "allperiodic": (lambda: sy.random_fields(128, 96, seed=22), PER_BC, sy.RANDOM_PHYS, 32),                     # images and stored ghost B on all four sides
    "yperiodic-tall": (lambda: sy.random_fields(64, 200, seed=23), sy.CONV_BC, sy.RANDOM_PHYS, 8),              # many chunks, the periodic seam in y
    "shmip-physical-y": (lambda: sy.shmip_fields(128, 64), sy.A3_BC, sy.A3_PHYS, 64),                           # one strip, top and bottom ghost rows, chunk seams
}
NCYC = 3      # the scanning cycle, then two in the new mode


@pytest.fixture(scope="module")
def hip():
    from suhmo_amd import capi, level
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return level


def streaming_everywhere(monkeypatch, hc, graphs=True):
    monkeypatch.setenv("SUHMO_FUSED_MIN_CELLS", "1")
    monkeypatch.setenv("SUHMO_GSRB_TILE", "0")
    monkeypatch.setenv("SUHMO_FUSED_HC", str(hc))
    if not graphs:
        monkeypatch.setenv("SUHMO_GRAPH_MAX_CELLS", "0")


def clean_fields(mk):
    f = mk()
    f.pop("bx", None); f.pop("by", None)
    f["mask"][:] = 1.0
    return f


def snapshot(L, mod):
    return dict(phi=L.get(mod.F_PHI, ghosted=True),
                bx=[L.get(mod.F_BX, depth=d) for d in range(L.ndepth)], by=[L.get(mod.F_BY, depth=d) for d in range(L.ndepth)])


def make(mod, f, bc, ph, mb, alpha=0.0, oracle_side=False):
    if oracle_side:
        L = mod.OracleLevel(f["nx"], f["ny"], f["dx"], f["dy"], bc, ph, alpha, -1.0, mb, 2)
    else:
        L = mod.HipLevel(f["nx"], f["ny"], f["dx"], f["dy"], bc, ph, alpha, -1.0, mb)
    L.set_inputs(f)
    L.build_mg_coefficients()
    return L


_REF = {}


def reference(oracle, name):
    """the oracle's state after each of NCYC V-cycles of a case: computed once, shared by every chunk height and both graph settings"""
    if name not in _REF:
        mk, bc, ph, mb = CASES[name]
        O = make(oracle, clean_fields(mk), bc, ph, mb, oracle_side=True)
        snaps = []
        for _ in range(NCYC):
            O.vcycle(SP)
            snaps.append(snapshot(O, oracle))
        _REF[name] = snaps
    return _REF[name]


def same(got, want, f, bc, what):
    nx, ny = f["nx"], f["ny"]
    assert got["bx"][0].shape == (ny, nx + 1) and got["by"][0].shape == (ny + 1, nx)       # the level's last face column and row are in
    for d in range(len(want["bx"])):
        for k in ("bx", "by"):
            bad = np.argwhere(got[k][d] != want[k][d])
            assert bad.size == 0, (what, k, "depth", d, "first at (row, column)", tuple(bad[0]), "of", len(bad))
    assert np.array_equal(got["phi"][1:-1, 1:-1], want["phi"][1:-1, 1:-1]), (what, "head", float(np.max(np.abs(got["phi"][1:-1, 1:-1] - want["phi"][1:-1, 1:-1]))))
    gr.level_ring_equal(want["phi"], got["phi"], (nx, ny), bc["periodic"], what=what)
    gr.domain_bc_holds(got["phi"], bc, f["dx"], f["dy"], (0, 0, nx - 1, ny - 1), (nx, ny), what)


def run(hip, f, bc, ph, mb, on, sp=SP, alpha=0.0, ncyc=NCYC):
    """ncyc V-cycles of a device level: (snapshot, counter) after each"""
    G = make(hip, f, bc, ph, mb, alpha=alpha)
    G.set_option("bcoef_in_relax", on)
    assert G.get_option("bcoef_in_relax") == on and G.get_option("bcoef_in_relax_launches") == 0
    out = []
    for _ in range(ncyc):
        G.vcycle(sp)
        G.synchronize()                   # (the scan's answer has arrived when the next cycle asks)
        out.append((snapshot(G, hip), G.get_option("bcoef_in_relax_launches")))
    return G, out


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("hc", [0, 6, 10])
@pytest.mark.parametrize("name", list(CASES))
def test_faces_formed_by_the_first_presmoothing_launch(oracle, hip, name, hc, graphs, monkeypatch):
    streaming_everywhere(monkeypatch, hc, graphs)
    mk, bc, ph, mb = CASES[name]
    f = clean_fields(mk)
    ref = reference(oracle, name)
    G, on = run(hip, f, bc, ph, mb, 1)
    _, off = run(hip, f, bc, ph, mb, 0)
    assert G.get_option("mask_state") == 1 and G.get_option("mask_scans") == 1       # known clean after the first cycle's scan
    for k in range(NCYC):
        same(on[k][0], ref[k], f, bc, (name, hc, "cycle", k, "option on"))
        same(off[k][0], ref[k], f, bc, (name, hc, "cycle", k, "option off"))
        same(on[k][0], off[k][0], f, bc, (name, hc, "cycle", k, "on against off"))
        assert on[k][1] == k, ("one launch per cycle once the mask is known clean", [c for _, c in on])
        assert off[k][1] == 0
    # the launch stands for the cycle's unmasked UpdateOperator: that counter moves as it did
    assert G.get_option("bcoef_unmasked_launches") == NCYC - 1


FALLBACKS = ["two-sweeps", "mask-below-1e-6", "alpha"]


@pytest.mark.parametrize("which", FALLBACKS)
def test_cases_that_keep_the_separate_pass(oracle, hip, which, monkeypatch):
    """the mode does not arm: a pre-smoothing that is one restricting launch, a mask that is not clean, an operator with alpha != 0"""
    streaming_everywhere(monkeypatch, 6)
    mk, bc, ph, mb = CASES["allperiodic"]
    f = clean_fields(mk)
    sp, alpha = SP, 0.0
    if which == "two-sweeps": sp = dict(SP, num_smooth=2)
    elif which == "mask-below-1e-6": f["mask"][40, 70] = 5e-7
    else: alpha = 0.6
    O = make(oracle, f, bc, ph, mb, alpha=alpha, oracle_side=True)
    G, got = run(hip, f, bc, ph, mb, 1, sp=sp, alpha=alpha)
    for k in range(NCYC):
        O.vcycle(sp)
        same(got[k][0], snapshot(O, oracle), f, bc, (which, "cycle", k))
        assert got[k][1] == 0, (which, [c for _, c in got])
    assert G.get_option("mask_state") == (2 if which == "mask-below-1e-6" else 1)


def test_solve_with_the_faces_formed_in_the_relaxation(oracle, hip, monkeypatch):
    streaming_everywhere(monkeypatch, 6)
    mk, bc, ph, mb = CASES["shmip-physical-y"]
    f = clean_fields(mk)
    O = make(oracle, f, bc, ph, mb, oracle_side=True)
    G = make(hip, f, bc, ph, mb)
    for k in range(2):                    # (the second solve starts with the mask known)
        no, ho = O.solve(SP); ng, hg = G.solve(SP)
        assert ng == no and np.array_equal(hg, ho), (k, ng, no, hg, ho)
        go, gg = O.get(oracle.F_PHI, ghosted=True), G.get(hip.F_PHI, ghosted=True)
        assert np.array_equal(gg[1:-1, 1:-1], go[1:-1, 1:-1]), (k, "head")
        gr.level_ring_equal(go, gg, (f["nx"], f["ny"]), bc["periodic"], what=("solve", k))
    assert ng > 0 and G.get_option("bcoef_in_relax_launches") >= ng      # every cycle of the second solve at least
