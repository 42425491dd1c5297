"""The device reductions (suhmo_amd/csrc/suhmo_reduce.h) at the edges of their launches, bit for bit: the sums against the numpy twin of
their order (tests/reduce_ref.py; tests/test_reduce_order_cpu.py shows that these inputs tell orders apart), the maxima against numpy.

Shapes of whole levels: 63 x 3, 64 x 4 and 65 x 5 (either side of one workgroup), 130 x 9, 2050 x 36 (33 columns of workgroups wanted, 32
given: the walk wraps in x; 288 partials: the second stage strides past 256) and 66 x 516 (129 rows of workgroups wanted, 128 given: the
walk wraps in y; exactly 256 partials).  The smallest level suhmo_level_create accepts is 2 x 2 (nx >= 2 and ny >= 2, and no coarser depth
of it exists), so that stands for the single cell; the twin's 1 x 1 is held to the kernel text on the CPU.

The moulin integrals contain the device's exp and have no twin: tests/test_gpu_moulin.py, test_gpu_timestep_strips.py, test_gpu_hier_strips.py
and test_gpu_amr_timestep.py hold them equal across entry points, layouts and ranks.

The hierarchy's level 1 is ONE box of 272 x 72 cells: HipHier accepts it.  Under the box cap of 4 x 16 workgroups (256 x 64 cells a round) the
walk wraps in both directions inside it."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import reduce_ref as rr

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2), (63, 3), (64, 4), (65, 5), (130, 9), (2050, 36), (66, 516)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d" % s)
def lev(request):
    from suhmo_amd import level
    nx, ny = request.param
    G = level.HipLevel(nx, ny, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS)
    x, y = rr.inputs(nx, ny)
    G.set(level.F_RES, x); G.set(level.F_LPHI, y)
    yield G, x, y
    G.close()


def test_sums_equal_the_twin(lev):
    from suhmo_amd.level import F_RES, F_LPHI
    G, x, y = lev
    n2, d = G.norm(F_RES, 2), G.dot(F_RES, F_LPHI)
    t2, td = rr.two_stage_sum(x * x), rr.two_stage_sum(x * y)
    print("%d x %d: norm2 %s twin %s   dot %s twin %s" % (G.nx, G.ny, n2.hex(), float(np.sqrt(t2)).hex(), d.hex(), td.hex()))
    assert n2 == float(np.sqrt(t2))                 # (the host's sqrt on both sides: correctly rounded, both)
    assert d == td
    assert G.dot(F_LPHI, F_RES) == td               # a product commutes; the order of the sum is the same


def test_max_norm_finds_the_planted_extreme(lev):
    """in the last column, in the last row, and in the last cell a thread that wrapped around visits (the last cell of the level)"""
    from suhmo_amd.level import F_RES, F_CORR
    G, x, _ = lev
    assert G.norm(F_RES, 0) == np.max(np.abs(x))
    ny, nx = x.shape
    for j, i in ((ny // 2, nx - 1), (ny - 1, nx // 2), (ny - 1, nx - 1)):
        z = x.copy()
        z[j, i] = -3.5
        G.set(F_CORR, z)
        assert G.norm(F_CORR, 0) == 3.5 == np.max(np.abs(z)), (j, i)
    z = x.copy()
    z[0, 0] = np.nextafter(2.0, 3.0)               # ... and a maximum that exceeds the rest by one bit
    G.set(F_CORR, z)
    assert G.norm(F_CORR, 0) == z[0, 0]


def test_picard_pair_through_the_time_step(oracle):
    """max h and max |h_lagged - h| decide when the Picard loop of a time step ends: on a level of more than one workgroup the iteration
    counts and the head are the oracle's"""
    from suhmo_amd import model
    nx, ny = 160, 32
    m = sy.A3_MODEL
    st = sy.shmip_initial_state(nx, ny)
    O = oracle.OracleModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=32, nthreads=2)
    G = model.HipModel(nx, ny, st["dx"], st["dy"], sy.A3_BC, sy.A3_PHYS, m, max_box=32)
    O.set_state(st); G.set_state(st)
    for k in range(3):
        po, pg = O.timestep(m["dt"]), G.timestep(m["dt"])
        assert po == pg and po[0] >= 1, (k, po, pg)
        assert np.array_equal(np.array(O.field(oracle.OM_H))[1:-1, 1:-1], G.get("head")), k
    O.close(); G.close()


@pytest.mark.parametrize("options", [None, "merged_launches=0"], ids=["merged", "per-level"])
def test_composite_max_norm_of_a_box_beyond_one_round_of_its_grid(options):
    """the composite residual norm equals numpy's over the uncovered cells of what the device left in RES, with the maximum planted in the
    level-1 box beyond column 256 and row 64, in turn with it planted on level 0 under the box (covered: it must not count)"""
    from suhmo_amd import level
    nx0, ny0, box = 192, 48, (32, 8, 303, 79)
    bc = dict(type=[[0, 1], [1, 0]], value=[[0.0, 0.0], [0.0, 0.0]], periodic=[0, 0])
    fs = sy.amrm_fields(nx0, ny0, ([box],), lx=192.0, ly=48.0)
    G = level.HipHier(nx0, ny0, fs[0]["dx"], fs[0]["dy"], bc, sy.CFG3_PHYS, [[box]], max_box=32, options=options)
    G.set_inputs(fs)
    G.update_operator(1); G.coarse.update_operator()
    B = G.level[1][0]
    assert (B.nx, B.ny) == (272, 72)
    covered = np.zeros((ny0, nx0), dtype=bool)
    covered[box[1] // 2:box[3] // 2 + 1, box[0] // 2:box[2] // 2 + 1] = True

    def composite():
        r = G.residual()
        r0, r1 = G.coarse.get(level.F_RES), B.get(level.F_RES)
        assert np.all(r0[covered] == 0.0)
        return r, max(np.max(np.abs(r0[~covered])), np.max(np.abs(r1))), r1

    r, ref, _ = composite()
    assert r == ref and r > 0.0
    rhs = B.get(level.F_RHS)
    rhs[70, 270] += 1.0e6 * r
    B.set(level.F_RHS, rhs)
    r, ref, r1 = composite()
    assert r == ref == abs(r1[70, 270])
    c = G.coarse.get(level.F_RHS)
    c[20, 60] += 1.0e9 * r                          # under the box
    G.coarse.set(level.F_RHS, c)
    r2, ref2, _ = composite()
    assert r2 == ref2 == r
    G.close()
