"""The streaming relaxation kernel's row loop (suhmo_gsrb.hip, k_gsrb_fused) at the shapes where a change of its control flow or of where it
reads its uniform operands can go wrong: workgroups that touch no side of the level next to ones that do.  The launch that forms the faces reads what
only a workgroup at a side needs (boundary types and values) from its arguments inside the rare branch, and every instantiation forms a
boundary ghost through one helper; nothing about an update changes, so every case is bitwise against the oracle's V-cycle and, for the faces, against the run with
bcoef_in_relax = 0: the head and its ghost ring, depth 0's faces with the last face column and row, the averaged faces of every depth, and
what the restricting launch and the launch that forms the FAS right-hand side leave on the coarse depths (R phi relaxed, right-hand side,
restricted residual); `solve` adds the residual its last launch leaves behind.  Every depth that can runs on the streaming kernel.  The
shapes are the smallest with
  - three to four strips, so that strips without a side of the level lie between the two that have one: 384 columns (strips of 96 / 128) and
    348 columns (strips 116 wide: an LDS row is full, its first and last lanes are halo lanes);
  - chunks of 6 rows in 48: a chunk has fill, middle and drain steps, and chunks without a side lie between the first and the last;
  - one strip (128 x 64): no workgroup without a side;
  - 16 rows in chunks of 6: the last chunk is 4 rows, shorter than the 2K + 1 rows a half-sweep pipeline holds;
  - an odd chunk height (7) that the restricting launch rounds up while the other launches keep it.
Three cycles per case: the first scans the mask, the second and third enter with the head's two canvases in either order."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import ghostring as gr
from tests.test_gpu_bcoef_in_relax import PER_BC, SP, NCYC, streaming_everywhere, clean_fields, snapshot, make, same

pytestmark = pytest.mark.gpu

# name: (nx, ny, seed, boundary conditions)
SHAPES = {
    "384x48-physical": (384, 48, 31, sy.RANDOM_BC),
    "384x48-periodic": (384, 48, 32, PER_BC),
    "348x48-physical": (348, 48, 33, sy.RANDOM_BC),
    "348x48-periodic": (348, 48, 34, PER_BC),
    "128x64-one-strip": (128, 64, 35, sy.RANDOM_BC),
    "384x16-physical": (384, 16, 36, sy.RANDOM_BC),
    "384x16-periodic": (384, 16, 37, PER_BC),
}
MAX_BOX = 16


@pytest.fixture(scope="module")
def hip():
    from suhmo_amd import capi, level
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return level


def fields(name):
    nx, ny, seed, bc = SHAPES[name]
    return clean_fields(lambda: sy.random_fields(nx, ny, seed=seed)), bc


def coarse(L, mod):
    return {d: {k: L.get(fld, depth=d) for k, fld in (("R phi relaxed", mod.F_PHI), ("right-hand side", mod.F_RHS), ("restricted residual", mod.F_RES))}
            for d in range(1, L.ndepth)}


_REF = {}


def reference(oracle, name):
    """the oracle's state after each of NCYC V-cycles: computed once per shape"""
    if name not in _REF:
        f, bc = fields(name)
        O = make(oracle, f, bc, sy.RANDOM_PHYS, MAX_BOX, oracle_side=True)
        out = []
        for _ in range(NCYC):
            O.vcycle(SP)
            out.append((snapshot(O, oracle), coarse(O, oracle)))
        _REF[name] = out
    return _REF[name]


def cycles(hip, f, bc, on):
    G = make(hip, f, bc, sy.RANDOM_PHYS, MAX_BOX)
    G.set_option("bcoef_in_relax", on)
    out = []
    for _ in range(NCYC):
        G.vcycle(SP)
        G.synchronize()
        out.append((snapshot(G, hip), coarse(G, hip), G.get_option("bcoef_in_relax_launches")))
    return G, out


def check(oracle, hip, name, what):
    f, bc = fields(name)
    ref = reference(oracle, name)
    G, on = cycles(hip, f, bc, 1)
    _, off = cycles(hip, f, bc, 0)
    assert G.get_option("mask_state") == 1
    for k in range(NCYC):
        for label, got in (("option on", on[k]), ("option off", off[k])):
            same(got[0], ref[k][0], f, bc, (what, "cycle", k, label))
            for d, want in ref[k][1].items():
                for key, arr in want.items():
                    bad = np.argwhere(got[1][d][key] != arr)
                    assert bad.size == 0, (what, "cycle", k, label, key, "depth", d, "first at (row, column)", tuple(bad[0]), "of", len(bad))
        same(on[k][0], off[k][0], f, bc, (what, "cycle", k, "on against off"))
        assert on[k][2] == k and off[k][2] == 0, (what, [c for _, _, c in on])


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("hc", [6, 10, 0])
@pytest.mark.parametrize("name", ["384x48-physical", "384x48-periodic", "348x48-physical", "348x48-periodic"])
def test_strips_and_chunks_without_a_side_next_to_ones_with(oracle, hip, name, hc, graphs, monkeypatch):
    streaming_everywhere(monkeypatch, hc, graphs)
    check(oracle, hip, name, (name, hc, graphs))


@pytest.mark.parametrize("name", ["128x64-one-strip", "384x16-physical", "384x16-periodic"])
def test_one_strip_and_a_chunk_shorter_than_the_pipeline(oracle, hip, name, monkeypatch):
    streaming_everywhere(monkeypatch, 6)
    check(oracle, hip, name, (name, 6))


@pytest.mark.parametrize("name", ["384x48-physical", "348x48-periodic"])
def test_odd_chunk_height_that_the_restricting_launch_rounds(oracle, hip, name, monkeypatch):
    streaming_everywhere(monkeypatch, 7)
    check(oracle, hip, name, (name, 7))


@pytest.mark.parametrize("name", ["384x48-physical", "348x48-periodic"])
def test_solve_leaves_the_residual_of_its_last_launch(oracle, hip, name, monkeypatch):
    """the launch that ends a cycle of `solve` stores the residual of the final head and its norm: iteration count, every norm of the
    history, the head with its ring and the residual field are the oracle's"""
    streaming_everywhere(monkeypatch, 6)
    f, bc = fields(name)
    O = make(oracle, f, bc, sy.RANDOM_PHYS, MAX_BOX, oracle_side=True)
    G = make(hip, f, bc, sy.RANDOM_PHYS, MAX_BOX)
    for k in range(2):                    # (the second solve starts with the mask known)
        no, ho = O.solve(SP); ng, hg = G.solve(SP)
        assert ng == no and np.array_equal(hg, ho), (name, k, ng, no, hg, ho)
        go, gg = O.get(oracle.F_PHI, ghosted=True), G.get(hip.F_PHI, ghosted=True)
        assert np.array_equal(gg[1:-1, 1:-1], go[1:-1, 1:-1]), (name, k, "head")
        gr.level_ring_equal(go, gg, (f["nx"], f["ny"]), bc["periodic"], what=(name, "solve", k))
        assert np.array_equal(G.get(hip.F_RES), O.get(oracle.F_RES)), (name, k, "residual of the final head")
    assert ng > 0 and G.get_option("residual_in_relax_launches") > 0 and G.get_option("bcoef_in_relax_launches") >= ng
