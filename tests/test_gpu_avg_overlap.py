"""AverageOperator beside the restricting launch of depth 0 (level option avg_overlap, default 1; suhmo_gsrb.hip, avg_fork / suhmo_avg_join):
in a cycle whose first pre-smoothing launch forms depth 0's faces, the averages of every coarse depth run on the level's side stream while the
cycle's stream goes on with the launch that restricts; the cycle's stream waits for them before it first reads a coarse face and before the
cycle returns.  Nothing about any kernel's arithmetic changes, so every case is bitwise: against the option-off run and against the oracle's
V-cycle -- the faces of every depth, the head with its ghost ring.  The counter avg_overlap_launches says which path ran.

The shapes are the small levels that the tests of the face-forming launch force onto the streaming kernel (tests/test_gpu_relax_steady.py): 384
columns in chunks of 6, 10 and the automatic height, 348 columns with physical and with periodic sides.  The mode needs a mask known clean, so
every run starts with one cycle that scans it (and a synchronize, so that the answer is there); the cycles that follow are the ones counted.
The cycles run eagerly (graph_max_cells = 0) except where a case says otherwise: a level whose cycles are captured keeps the averages on the
cycle's stream, in the capture and in the eager first use before it."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests.test_gpu_bcoef_in_relax import SP, streaming_everywhere, snapshot, make, same
from tests.test_gpu_relax_steady import MAX_BOX, fields

pytestmark = pytest.mark.gpu

NCYC = 3                                  # counted cycles, after the one that scans the mask
CASES = [("384x48-physical", 6), ("384x48-physical", 10), ("384x48-physical", 0), ("348x48-physical", 6), ("348x48-periodic", 6)]


@pytest.fixture(scope="module")
def hip():
    from suhmo_amd import capi, level
    assert capi.lib().suhmo_device_count() > 0, "no GPU visible: the product path has no fallback"
    return level


_REF = {}


def reference(oracle, name, sp=SP):
    """the oracle's state after the scanning cycle and each of the NCYC cycles behind it: once per shape and smoothing count"""
    key = (name, sp["num_smooth"])
    if key not in _REF:
        f, bc = fields(name)
        O = make(oracle, f, bc, sy.RANDOM_PHYS, MAX_BOX, oracle_side=True)
        O.vcycle(sp)
        out = []
        for _ in range(NCYC):
            O.vcycle(sp)
            out.append(snapshot(O, oracle))
        _REF[key] = out
    return _REF[key]


def counters(G):
    return {k: G.get_option(k) for k in ("avg_overlap_launches", "bcoef_in_relax_launches", "vcycle_graph_replays")}


def start(hip, name, overlap, sp=SP, graph_max_cells=None, profile=False):
    """a level behind its scanning cycle"""
    f, bc = fields(name)
    G = make(hip, f, bc, sy.RANDOM_PHYS, MAX_BOX)
    G.set_option("avg_overlap", overlap)
    if graph_max_cells is not None: G.set_option("graph_max_cells", graph_max_cells)
    if profile: G.profile(True)
    assert G.get_option("avg_overlap") == overlap and G.get_option("avg_overlap_launches") == 0
    G.vcycle(sp)
    G.synchronize()                       # (the scan's answer has arrived when the next cycle asks)
    return G


def cycles(hip, name, overlap, sp=SP, **kw):
    """NCYC cycles behind the scanning one, each read straight after the call returns: (snapshot, counters) after each"""
    G = start(hip, name, overlap, sp, **kw)
    base = counters(G)
    out = []
    for _ in range(NCYC):
        G.vcycle(sp)
        out.append((snapshot(G, hip), {k: v - base[k] for k, v in counters(G).items()}))
    return G, out


@pytest.mark.parametrize("name,hc", CASES)
def test_averages_beside_the_restricting_launch(oracle, hip, name, hc, monkeypatch):
    streaming_everywhere(monkeypatch, hc, graphs=False)
    f, bc = fields(name)
    ref = reference(oracle, name)
    _, on = cycles(hip, name, 1)
    _, off = cycles(hip, name, 0)
    for k in range(NCYC):
        same(on[k][0], ref[k], f, bc, (name, hc, "cycle", k, "option on"))
        same(off[k][0], ref[k], f, bc, (name, hc, "cycle", k, "option off"))
        same(on[k][0], off[k][0], f, bc, (name, hc, "cycle", k, "on against off"))
        assert on[k][1]["avg_overlap_launches"] == k + 1 and on[k][1]["bcoef_in_relax_launches"] == k + 1, (name, hc, [c for _, c in on])
        assert off[k][1]["avg_overlap_launches"] == 0 and off[k][1]["bcoef_in_relax_launches"] == k + 1, (name, hc, [c for _, c in off])
        assert on[k][1]["vcycle_graph_replays"] == 0


@pytest.mark.parametrize("name", ["384x48-physical", "348x48-periodic"])
def test_solve_with_the_averages_on_the_side_stream(hip, name, monkeypatch):
    streaming_everywhere(monkeypatch, 6, graphs=False)
    f, bc = fields(name)
    got = {}
    for overlap in (1, 0):
        G = make(hip, f, bc, sy.RANDOM_PHYS, MAX_BOX)
        G.set_option("avg_overlap", overlap)
        runs = []
        for k in range(2):                # (the second solve starts with the mask known)
            n, hist = G.solve(SP)
            runs.append((n, hist, G.get(hip.F_PHI, ghosted=True)))
        got[overlap] = (runs, G.get_option("avg_overlap_launches"), G.get_option("bcoef_in_relax_launches"))
    for k in range(2):
        (n1, h1, p1), (n0, h0, p0) = got[1][0][k], got[0][0][k]
        assert n1 == n0 and np.array_equal(h1, h0), (name, k, n1, n0, h1, h0)
        assert np.array_equal(p1, p0), (name, k, "head and ring")
    assert got[1][0][1][0] > 0 and got[1][1] == got[1][2] >= got[1][0][1][0]      # every cycle that formed the faces forked, the second solve's at least
    assert got[0][1] == 0 and got[0][2] == got[1][2]


@pytest.mark.parametrize("which", ["graphs", "profiling"])
def test_cases_that_keep_the_averages_on_the_cycle_stream(oracle, hip, which, monkeypatch):
    """a level whose cycles are captured, and a level that is being profiled: no fork, same results"""
    name = "384x48-physical"
    streaming_everywhere(monkeypatch, 6, graphs=(which == "graphs"))
    f, bc = fields(name)
    ref = reference(oracle, name)
    kw = dict(graph_max_cells=1000000) if which == "graphs" else dict(profile=True)
    G, got = cycles(hip, name, 1, **kw)
    for k in range(NCYC):
        same(got[k][0], ref[k], f, bc, (which, "cycle", k))
        assert got[k][1]["avg_overlap_launches"] == 0 and got[k][1]["bcoef_in_relax_launches"] == k + 1, (which, [c for _, c in got])
    replays = [c["vcycle_graph_replays"] for _, c in got]
    if which == "graphs": assert replays[0] >= 1 and replays[1] > replays[0] and replays[2] > replays[1], replays
    else: assert replays == [0] * NCYC, replays
    assert G.get_option("avg_overlap_launches") == 0


def test_join_when_the_presmoothing_is_one_launch(oracle, hip, monkeypatch):
    """two pre-smoothing sweeps are the restricting launch alone: the faces come from the separate pass and its averages, nothing forks, and what
    the caller reads straight after the call is what it reads after a synchronize"""
    name = "348x48-physical"
    streaming_everywhere(monkeypatch, 6, graphs=False)
    sp = dict(SP, num_smooth=2)
    f, bc = fields(name)
    ref = reference(oracle, name, sp)
    G = start(hip, name, 1, sp)
    for k in range(NCYC):
        G.vcycle(sp)
        first = snapshot(G, hip)
        G.synchronize()
        again = snapshot(G, hip)
        same(first, again, f, bc, ("num_smooth 2", "cycle", k, "straight after the call against after a synchronize"))
        same(first, ref[k], f, bc, ("num_smooth 2", "cycle", k))
    assert G.get_option("avg_overlap_launches") == 0 and G.get_option("bcoef_in_relax_launches") == 0


def test_two_levels_with_interleaved_cycles(hip, monkeypatch):
    """each level owns its side stream and events, and no cycle returns with its fork open: interleaved, both are what they are alone"""
    names = ["384x48-physical", "348x48-periodic"]
    streaming_everywhere(monkeypatch, 6, graphs=False)
    solo = {}
    for name in names:
        _, out = cycles(hip, name, 1)
        solo[name] = out[-1][0]
    Gs = [start(hip, name, 1) for name in names]
    for _ in range(NCYC):
        for G in Gs: G.vcycle(SP)
    for G in Gs: G.synchronize()
    for name, G in zip(names, Gs):
        f, bc = fields(name)
        same(snapshot(G, hip), solo[name], f, bc, (name, "interleaved against alone"))
        assert G.get_option("avg_overlap_launches") == NCYC
