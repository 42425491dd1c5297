"""What is known about the bed elevation across V-cycles (level option zb_known): the first V-cycle after a write to zb scans every
depth's array, bit pattern against bit pattern; later cycles of a clean-mask alpha = 0 level relax the depths whose bed is ONE pattern with
the instantiations of k_gsrb_fused that take it as a scalar (ZBU) and load no zb.  The operand of COMPUTENONLINEARTERMS is the same value,
so every case is bitwise against the oracle's V-cycle -- the head with its ghost ring, the faces of every depth -- and against the same run
with zb_known = 0, three cycles each (the first scans mask and bed on the parent's kernels, the second and third enter with the head's two
canvases in either order); the counters relax_zb_uniform_launches_d<depth> say which depths took the path.  The shapes are the ones on which
tests/test_gpu_relax_steady.py forces the streaming kernel: strips and chunks that touch no side of the level between ones that do (384 and
348 columns, chunks of 6 and 10 rows in 48 and the automatic height), physical and all-periodic sides, one strip (64 x 48), as graph
replays and eagerly."""
import ctypes as C

import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import ghostring as gr

pytestmark = pytest.mark.gpu

PER_BC = dict(type=[[0, 0], [0, 0]], value=[[0, 0], [0, 0]], periodic=[1, 1])
SP = dict(sy.SOLVER_DEFAULT, eps=1e-10, norm_thresh=1e-13, max_iter=3, imin=6)
NCYC = 3
MAX_BOX = 16
UNKNOWN, UNIFORM, VARYING = 0, 1, 2
# name: (nx, ny, seed, boundary conditions)
SHAPES = {
    "384x48-physical": (384, 48, 31, sy.RANDOM_BC),
    "384x48-periodic": (384, 48, 32, PER_BC),
    "348x48-physical": (348, 48, 33, sy.RANDOM_BC),
    "348x48-periodic": (348, 48, 34, PER_BC),
    "64x48-one-strip": (64, 48, 35, sy.RANDOM_BC),
}


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


def streams(nx, ny, d):
    """depth d relaxes with two-sweep launches of the streaming kernel: fused_ok(K = 2) of suhmo_gsrb.hip on a whole level"""
    return (nx >> d) % 2 == 0 and (nx >> d) >= 64 and (ny >> d) >= 12


def launches_per_cycle(d, ndepth):
    """pre- and post-smoothing of four sweeps; the bottom depth relaxes num_bottom = 16 sweeps: two per launch"""
    return SP["num_bottom"] // 2 if d == ndepth - 1 else SP["num_smooth"]


def fields(name, zb):
    """clean mask, no faces; zb: a value for every cell (ghost ring included) or a function that edits the ghosted array"""
    nx, ny, seed, bc = SHAPES[name]
    f = sy.random_fields(nx, ny, seed=seed)
    f.pop("bx", None); f.pop("by", None)
    f["mask"][:] = 1.0
    if callable(zb): zb(f["zb"])
    else: f["zb"][:] = zb
    return f, bc


def make(mod, f, bc, ph=sy.RANDOM_PHYS, alpha=0.0, oracle_side=False, zb_known=1):
    if oracle_side:
        L = mod.OracleLevel(f["nx"], f["ny"], f["dx"], f["dy"], bc, ph, alpha, -1.0, MAX_BOX, 2)
    else:
        L = mod.HipLevel(f["nx"], f["ny"], f["dx"], f["dy"], bc, ph, alpha, -1.0, MAX_BOX)
        L.set_option("zb_known", zb_known)
        assert L.get_option("zb_known") == zb_known and L.get_option("relax_zb_uniform_launches") == 0
    L.set_inputs(f)
    L.build_mg_coefficients()
    return L


def snapshot(L, mod):
    return dict(phi=L.get(mod.F_PHI, ghosted=True),
                bx=[L.get(mod.F_BX, depth=d) for d in range(L.ndepth)], by=[L.get(mod.F_BY, depth=d) for d in range(L.ndepth)])


def same(got, want, f, bc, what):
    nx, ny = f["nx"], f["ny"]
    for d in range(len(want["bx"])):
        for k in ("bx", "by"):
            bad = np.argwhere(got[k][d] != want[k][d])
            assert bad.size == 0, (what, k, "depth", d, "first at (row, column)", tuple(bad[0]), "of", len(bad))
    bad = np.argwhere(got["phi"][1:-1, 1:-1] != want["phi"][1:-1, 1:-1])
    assert bad.size == 0, (what, "head", "first at (row, column)", tuple(bad[0]), "of", len(bad))
    gr.level_ring_equal(want["phi"], got["phi"], (nx, ny), bc["periodic"], what=what)


def per_depth(G):
    return [G.get_option("relax_zb_uniform_launches_d%d" % d) for d in range(G.ndepth)]


def cycles(G, hip, ncyc=NCYC):
    """ncyc V-cycles: (snapshot, per-depth counters) after each; the scans' answers have arrived when the next cycle asks"""
    out = []
    for _ in range(ncyc):
        G.vcycle(SP)
        G.synchronize()
        out.append((snapshot(G, hip), per_depth(G)))
    return out


_REF = {}


def reference(oracle, key, f, bc, ph=sy.RANDOM_PHYS, alpha=0.0):
    """the oracle's state after each of NCYC V-cycles: computed once per (shape, bed) and shared by every chunk height and graph setting"""
    if key not in _REF:
        O = make(oracle, f, bc, ph, alpha, oracle_side=True)
        out = []
        for _ in range(NCYC):
            O.vcycle(SP)
            out.append(snapshot(O, oracle))
        _REF[key] = out
    return _REF[key]


def check(oracle, hip, key, f, bc, what, ph=sy.RANDOM_PHYS, alpha=0.0):
    """three cycles with the option on and off against the oracle; returns the level with the option on and its counters after each cycle"""
    ref = reference(oracle, key, f, bc, ph, alpha)
    G = make(hip, f, bc, ph, alpha)
    on = cycles(G, hip)
    G0 = make(hip, f, bc, ph, alpha, zb_known=0)
    off = cycles(G0, hip)
    for k in range(NCYC):
        same(on[k][0], ref[k], f, bc, (what, "cycle", k, "zb_known = 1"))
        same(off[k][0], ref[k], f, bc, (what, "cycle", k, "zb_known = 0"))
        same(on[k][0], off[k][0], f, bc, (what, "cycle", k, "on against off"))
    assert sum(off[-1][1]) == 0 and G0.get_option("zb_scans") == 0 and G0.get_option("zb_state") == UNKNOWN, (what, off[-1][1])
    assert sum(on[0][1]) == 0, (what, "the first cycle runs while nothing is known", on[0][1])
    return G, [c for _, c in on]


def bits_uniform(a):
    b = np.ascontiguousarray(a).view(np.uint64)
    return bool(np.all(b == b.flat[0]))


def counters_follow_the_arrays(G, hip, f, counts, what):
    """on every depth that streams the counter moved exactly when that depth's bed, read back, is one bit pattern"""
    for d in range(G.ndepth):
        uni = bits_uniform(G.get(hip.F_ZB, depth=d))
        if streams(f["nx"], f["ny"], d):
            assert (counts[-1][d] > 0) == uni, (what, "depth", d, uni, counts)
            assert G.get_option("zb_state_d%d" % d) == (UNIFORM if uni else VARYING), (what, d)
        elif (f["nx"] >> d) < 64:
            assert counts[-1][d] == 0, (what, "depth", d, "cannot stream", counts)


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("hc", [6, 10, 0])
@pytest.mark.parametrize("zb", [0.0, 37.5])
@pytest.mark.parametrize("name", ["384x48-physical", "384x48-periodic", "348x48-physical", "348x48-periodic"])
def test_uniform_bed_runs_as_a_scalar_on_every_streaming_depth(oracle, hip, name, zb, hc, graphs, monkeypatch):
    """the face-forming launch, the plain and the restricting launch of depth 0 and depth 1's launches (the first forms the FAS right-hand
    side) all take the scalar from the second cycle on"""
    streaming_everywhere(monkeypatch, hc, graphs)
    f, bc = fields(name, zb)
    G, counts = check(oracle, hip, (name, zb), f, bc, (name, zb, hc, graphs))
    assert G.get_option("zb_scans") == 1 and G.get_option("zb_state") == UNIFORM
    nstream = 0
    for d in range(G.ndepth):
        if streams(f["nx"], f["ny"], d):
            nstream += 1
            n = launches_per_cycle(d, G.ndepth)                # every launch of the depth, in cycles two and three
            assert counts[1][d] == n and counts[2][d] == 2 * n, (name, zb, hc, graphs, "depth", d, counts)
    assert nstream >= 2, (name, nstream)
    assert G.get_option("bcoef_in_relax_launches") == 2 and G.get_option("rhs_in_streaming_launches") >= 2
    assert G.get_option("relax_zb_uniform_launches") == sum(counts[2])
    counters_follow_the_arrays(G, hip, f, counts, (name, zb))


@pytest.mark.parametrize("zb", [0.0, 37.5])
def test_one_strip(oracle, hip, zb, monkeypatch):
    streaming_everywhere(monkeypatch, 6)
    f, bc = fields("64x48-one-strip", zb)
    G, counts = check(oracle, hip, ("64x48-one-strip", zb), f, bc, ("one strip", zb))
    assert counts[2][0] == 8, counts


@pytest.mark.parametrize("zb", [0.0, 37.5])
@pytest.mark.parametrize("name", ["384x48-physical", "348x48-periodic"])
def test_solve_leaves_the_residual_behind_with_the_bed_as_a_scalar(oracle, hip, name, zb, monkeypatch):
    """the launch that ends a cycle of `solve` (RM = 2) stores the residual of the final head and its norm: iteration count, history, head
    with its ring and residual field are the oracle's, with the option on and off"""
    streaming_everywhere(monkeypatch, 6)
    f, bc = fields(name, zb)
    O = make(oracle, f, bc, oracle_side=True)
    G, G0 = make(hip, f, bc), make(hip, f, bc, zb_known=0)
    ncyc = 0
    for k in range(2):
        no, ho = O.solve(SP)
        ncyc += no
        go = O.get(oracle.F_PHI, ghosted=True)
        for L in (G, G0):
            ng, hg = L.solve(SP)
            assert ng == no and np.array_equal(hg, ho), (name, zb, k, ng, no, hg, ho)
            gg = L.get(hip.F_PHI, ghosted=True)
            assert np.array_equal(gg[1:-1, 1:-1], go[1:-1, 1:-1]), (name, zb, k, "head")
            gr.level_ring_equal(go, gg, (f["nx"], f["ny"]), bc["periodic"], what=(name, zb, "solve", k))
            assert np.array_equal(L.get(hip.F_RES), O.get(oracle.F_RES)), (name, zb, k, "residual of the final head")
    assert no > 0 and G.get_option("residual_in_relax_launches") > 0
    # every cycle from the second on: all four launches of depth 0, the residual-leaving one among them
    assert ncyc > 2 and per_depth(G)[0] == 4 * (ncyc - 1), (per_depth(G), ncyc)
    assert sum(per_depth(G0)) == 0


@pytest.mark.parametrize("name", ["384x48-physical", "348x48-periodic"])
def test_a_value_whose_averages_are_computed(oracle, hip, name, monkeypatch):
    """0.1: the coarse depths hold ((c + c) + c + c) / 4, whatever that rounds to -- each depth is scanned on its own and carries its own value"""
    streaming_everywhere(monkeypatch, 6)
    f, bc = fields(name, 0.1)
    G, counts = check(oracle, hip, (name, 0.1), f, bc, (name, 0.1))
    assert counts[2][0] == 8, counts
    counters_follow_the_arrays(G, hip, f, counts, (name, 0.1))


def _deviate(where):
    def edit(zb):                          # ghosted: zb[j + 1, i + 1] is cell (i, j)
        ny, nx = zb.shape[0] - 2, zb.shape[1] - 2
        zb[:] = 37.5
        j, i = {"first-cell": (0, 0), "last-cell-of-the-last-row": (ny - 1, nx - 1), "middle-strip-and-chunk": (ny // 2 + 1, nx // 2 + 3)}[where]
        zb[j + 1, i + 1] = np.nextafter(37.5, 38.0)
    return edit


@pytest.mark.parametrize("where", ["first-cell", "last-cell-of-the-last-row", "middle-strip-and-chunk"])
def test_one_deviating_cell_keeps_the_loads(oracle, hip, where, monkeypatch):
    streaming_everywhere(monkeypatch, 6)
    f, bc = fields("384x48-physical", _deviate(where))
    G, counts = check(oracle, hip, ("384x48-physical", where), f, bc, where)
    assert counts[2][0] == 0 and G.get_option("zb_state") == VARYING and G.get_option("zb_scans") == 1, counts
    counters_follow_the_arrays(G, hip, f, counts, where)


def _zeros(kind):
    def edit(zb):
        zb[:] = -0.0 if kind == "all-negative-zero" else 0.0
        if kind == "one-negative-zero": zb[20, 200] = -0.0
    return edit


@pytest.mark.parametrize("kind", ["one-negative-zero", "all-negative-zero"])
def test_zeros_are_compared_as_bit_patterns(oracle, hip, kind, monkeypatch):
    """+0.0 everywhere but one -0.0: equal as values, not as bits -- depth 0 keeps loading (its averages are +0.0 again: the coarse depths
    do not); -0.0 everywhere is one pattern"""
    streaming_everywhere(monkeypatch, 6)
    f, bc = fields("384x48-physical", _zeros(kind))
    assert np.signbit(f["zb"]).sum() == (1 if kind == "one-negative-zero" else f["zb"].size)
    G, counts = check(oracle, hip, ("384x48-physical", kind), f, bc, kind)
    if kind == "one-negative-zero":
        assert counts[2][0] == 0 and G.get_option("zb_state") == VARYING and counts[2][1] == 2 * launches_per_cycle(1, G.ndepth), counts
    else:
        assert counts[2][0] == 8 and G.get_option("zb_state") == UNIFORM, counts
    counters_follow_the_arrays(G, hip, f, counts, kind)


def test_the_counter_follows_rewrites_of_the_bed(oracle, hip, monkeypatch):
    """uniform -> varying -> another uniform value (replayed graphs carry the value: the old ones must go) -> a writable pointer handed
    out: from then on nothing is known, whatever is written"""
    from suhmo_amd import capi
    streaming_everywhere(monkeypatch, 6)
    f, bc = fields("384x48-physical", 37.5)
    O, G = make(oracle, f, bc, oracle_side=True), make(hip, f, bc)

    def step(what, n=3):
        before = per_depth(G)[0]
        for k in range(n):
            O.vcycle(SP); G.vcycle(SP); G.synchronize()
            same(snapshot(G, hip), snapshot(O, oracle), f, bc, (what, k))
        return per_depth(G)[0] - before

    def rewrite(zb):
        O.set(oracle.F_ZB, zb, ghosted=True); G.set(hip.F_ZB, zb, ghosted=True)
        assert G.get_option("zb_state") == UNKNOWN
        O.build_mg_coefficients(); G.build_mg_coefficients()

    assert step("uniform 37.5") == 8 and G.get_option("zb_state") == UNIFORM
    rng = np.random.default_rng(5)
    rewrite(37.5 + rng.uniform(-1.0, 1.0, size=f["zb"].shape))
    assert step("varying") == 0 and G.get_option("zb_state") == VARYING and G.get_option("zb_scans") == 2
    rewrite(np.full(f["zb"].shape, 12.25))
    assert step("uniform 12.25") == 8 and G.get_option("zb_state") == UNIFORM and G.get_option("zb_scans") == 3
    rewrite(np.full(f["zb"].shape, -3.0))
    assert step("uniform -3.0") == 8 and G.get_option("zb_scans") == 4
    base = C.c_void_p(); pitch = C.c_long(); origin = C.c_long()
    capi.check(capi.lib().suhmo_level_field_view(G.h, 0, hip.F_ZB, C.byref(base), C.byref(pitch), C.byref(origin)))
    assert base.value and pitch.value > 384 and G.get_option("zb_state") == UNKNOWN
    assert step("after the view, same bed") == 0 and G.get_option("zb_state") == UNKNOWN
    rewrite(np.full(f["zb"].shape, 5.0))
    assert step("after the view, new bed") == 0 and G.get_option("zb_state") == UNKNOWN and G.get_option("zb_scans") == 4


def test_a_masked_level_keeps_the_parents_kernels(oracle, hip, monkeypatch):
    streaming_everywhere(monkeypatch, 6)
    f, bc = fields("384x48-physical", 37.5)
    f["mask"][20, 100] = -1.0
    G, counts = check(oracle, hip, ("384x48-physical", "one negative mask cell"), f, bc, "masked")
    assert sum(counts[2]) == 0 and G.get_option("mask_state") == 2, counts


def test_an_operator_with_alpha_keeps_the_parents_kernels(oracle, hip, monkeypatch):
    streaming_everywhere(monkeypatch, 6)
    f, bc = fields("384x48-physical", 37.5)
    G, counts = check(oracle, hip, ("384x48-physical", "alpha 0.7"), f, bc, "alpha = 0.7", alpha=0.7)
    assert sum(counts[2]) == 0, counts


def test_rank_strips_keep_the_parents_kernels(oracle, monkeypatch):
    from suhmo_amd import level as lv
    from test_gpu_strips import run_strips
    streaming_everywhere(monkeypatch, 6)
    f = sy.random_fields(128, 128, seed=41, with_mask_holes=False)
    f.pop("bx"); f.pop("by")
    f["mask"][:] = 1.0; f["zb"][:] = 37.5
    bc, ph = sy.RANDOM_BC, sy.RANDOM_PHYS

    def body(known):
        def run(G, rank):
            G.set_option("zb_known", known)
            G.build_mg_coefficients()
            for k in range(NCYC):
                G.vcycle(SP); G.synchronize()
            return G.get(lv.F_PHI), G.get_option("relax_zb_uniform_launches"), G.get_option("strip_streaming_launches"), G.get_option("zb_scans")
        return run

    on = run_strips(2, f, bc, ph, 0.0, -1.0, body(1), halo=16, max_box=32)
    off = run_strips(2, f, bc, ph, 0.0, -1.0, body(0), halo=16, max_box=32)
    O = oracle.OracleLevel(128, 128, f["dx"], f["dy"], bc, ph, 0.0, -1.0, 32, 2)
    O.set_inputs(f); O.build_mg_coefficients()
    for k in range(NCYC):
        O.vcycle(SP)
    want = O.get(oracle.F_PHI)
    assert np.array_equal(np.vstack([p[0] for p in on]), want) and np.array_equal(np.vstack([p[0] for p in off]), want)
    assert all(p[1] == 0 and p[2] > 0 and p[3] == 0 for p in on + off), [p[1:] for p in on + off]


def test_a_hierarchys_base_keeps_the_parents_kernels(oracle, monkeypatch):
    """two levels, the base (64 x 16, a whole level) on the streaming kernel with a uniform bed: it serves a hierarchy and keeps loading"""
    from suhmo_amd import level as lv
    streaming_everywhere(monkeypatch, 0)
    boxes = ([(16, 8, 47, 23)],)
    bc = dict(type=[[0, 1], [1, 0]], value=[[0.0, 0.0], [0.0, 0.0]], periodic=[0, 0])
    fs = sy.amrm_fields(64, 16, boxes, slope=0.0)
    fs[0]["zb"][:] = 37.5
    for b in fs[1]: b["zb"][:] = 37.5
    O = oracle.OracleAmrM(64, 16, fs[0]["dx"], fs[0]["dy"], bc, sy.CFG3_PHYS, boxes, max_box=32, nthreads=2)
    O.set_inputs(fs)
    runs = []
    for known in ("1", "0"):
        monkeypatch.setenv("SUHMO_ZB_KNOWN", known)
        G = lv.HipHier(64, 16, fs[0]["dx"], fs[0]["dy"], bc, sy.CFG3_PHYS, boxes, max_box=32)
        G.set_inputs(fs)
        runs.append(G)
    for k in range(NCYC):
        O.vcycle(SP)
        for G in runs:
            G.vcycle(SP)
            assert np.array_equal(G.coarse.get(lv.F_PHI), O.coarse.get(oracle.F_PHI)), ("base", k)
            assert np.array_equal(G.level[1][0].get(lv.F_PHI), O.box_get(1, 0, oracle.F_PHI)), ("level 1", k)
    for G in runs:
        assert G.coarse.get_option("relax_zb_uniform_launches") == 0 and G.coarse.get_option("zb_scans") == 0
        assert G.coarse.get_option("relax_unmasked_launches") > 0      # (the base streams: those launches are the streaming kernel's)
        G.close()
