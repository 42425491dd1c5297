"""The host rules of a hierarchy's run (include/suhmo_hip.h, "THE RUN OF A HIERARCHY" and "THE REST OF tagCells"), without a device: the steps
before which a run regrids against hand cases of src/AmrHydro.cpp:1317, the nesting of the tagSubset lists against hand cases of :1097-1108,
and the numpy twin of the restrict rule (tests/tagsubset_ref.py, which the GPU tests compare the kernel with) on hand-made maps."""
import numpy as np

from suhmo_amd import model
from tests import tagsubset_ref as ts


# ---- the reference regrids before the step that makes m_cur_step = c when m_cur_step = c - 1 is neither 0 nor the restart step and is a
# multiple of the interval
def test_interval_10_from_step_1():
    assert model.regrid_steps(1, 35, 10) == [11, 21, 31]
    assert model.regrid_steps(1, 10, 10) == []                 # c - 1 = 0 .. 9: only 0 is a multiple, and it is the first step


def test_a_second_run_from_11_regrids_unless_it_is_a_restart():
    assert model.regrid_steps(11, 5, 10) == [11]
    assert model.regrid_steps(11, 5, 10, skip_first=True) == []
    assert model.regrid_steps(11, 15, 10, skip_first=True) == [21]           # only the run's first step is the restart step
    assert model.regrid_steps(12, 15, 10, skip_first=True) == [21]


def test_interval_0_never_and_interval_1_skips_only_the_first_step():
    assert model.regrid_steps(1, 50, 0) == []
    assert model.regrid_steps(1, 5, 1) == [2, 3, 4, 5]
    assert model.regrid_steps(3, 3, 1) == [3, 4, 5]
    assert model.regrid_steps(3, 3, 1, skip_first=True) == [4, 5]
    assert model.regrid_steps(1, 7, 2) == [3, 5, 7]


# ---- nesting of the subsets
def as_masks(nx0, ny0, nested):
    return [ts.mask(nx0 << l, ny0 << l, bl) if bl else None for l, bl in enumerate(nested)]


def same_sets(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)) for x, y in zip(a, b))


def test_an_empty_level_inherits_the_refined_subset_below():
    got = model.nest_tag_subsets([[(2, 2, 9, 5)], [], []])
    assert got == [[(2, 2, 9, 5)], [(4, 4, 19, 11)], [(8, 8, 39, 23)]]


def test_a_level_with_boxes_is_intersected():
    got = model.nest_tag_subsets([[(2, 2, 9, 5), (12, 0, 15, 7)], [(0, 0, 9, 31), (16, 6, 27, 9), (60, 0, 63, 3)]])
    assert got[0] == [(2, 2, 9, 5), (12, 0, 15, 7)]
    # own x refined: (0,0,9,31) x (4,4,19,11) = (4,4,9,11); (16,6,27,9) x (4,4,19,11) = (16,6,19,9), x (24,0,31,15) = (24,6,27,9); (60..63) meets nothing
    assert got[1] == [(4, 4, 9, 11), (16, 6, 19, 9), (24, 6, 27, 9)]
    assert same_sets(as_masks(32, 16, got), ts.nest(32, 16, [[(2, 2, 9, 5), (12, 0, 15, 7)], [(0, 0, 9, 31), (16, 6, 27, 9), (60, 0, 63, 3)]]))


def test_an_empty_coarser_level_constrains_nothing():
    assert model.nest_tag_subsets([[], [(1, 1, 4, 4)], []]) == [[], [(1, 1, 4, 4)], [(2, 2, 9, 9)]]
    # a level whose boxes miss the refined subset below ends up empty, and an empty subset constrains nothing above it
    assert model.nest_tag_subsets([[(0, 0, 1, 1)], [(10, 10, 11, 11)], [(40, 40, 41, 41)]]) == [[(0, 0, 1, 1)], [], [(40, 40, 41, 41)]]


def test_nesting_agrees_with_the_mask_twin_on_drawn_lists():
    rng = np.random.default_rng(11)
    for _ in range(30):
        subs = []
        for l in range(3):
            bl = []
            for _ in range(int(rng.integers(0, 4))):
                lo0, lo1 = int(rng.integers(0, 30 << l)), int(rng.integers(0, 14 << l))
                bl.append((lo0, lo1, min(lo0 + int(rng.integers(0, 12 << l)), (32 << l) - 1), min(lo1 + int(rng.integers(0, 8 << l)), (16 << l) - 1)))
            subs.append(bl)
        assert same_sets(as_masks(32, 16, model.nest_tag_subsets(subs)), ts.nest(32, 16, subs)), subs


# ---- the restrict rule
def test_restrict_twin_at_granularity_1():
    t = np.ones((4, 6), dtype=np.uint8)
    t[0, 0] = 0
    got = ts.restrict(t, 1, [(1, 1, 3, 2), (3, 2, 5, 3)])
    want = np.array([[0, 0, 0, 0, 0, 0], [0, 1, 1, 1, 0, 0], [0, 1, 1, 1, 1, 1], [0, 0, 0, 1, 1, 1]], dtype=np.uint8)
    assert np.array_equal(got, want)
    assert np.array_equal(ts.restrict(t, 1, []), t)            # an empty subset is skipped
    assert not ts.restrict(t, 1, [(0, 0, 0, 0)]).any()         # the one entry inside was not tagged: nothing is set by a restrict


def test_restrict_twin_at_granularity_2():
    t = np.ones((3, 4), dtype=np.uint8)                        # a level of 8 x 6 cells
    got = ts.restrict(t, 2, [(2, 0, 5, 3), (6, 4, 9, 5)])      # the second box reaches beyond the domain
    assert np.array_equal(got, np.array([[0, 1, 1, 0], [0, 1, 1, 0], [0, 0, 0, 1]], dtype=np.uint8))
    assert ts.aligned(2, [(2, 0, 5, 3)]) and not ts.aligned(2, [(2, 0, 4, 3)]) and not ts.aligned(2, [(1, 0, 4, 3)])


# ---- the grids of tests/test_gpu_hier_run.py's runs: what the host generator makes of the tags its two variables and its subset leave
def test_the_run_tests_set_up_generates_the_grids_it_names():
    from suhmo_amd import synthetic as sy
    from tests import hierlayouts as hl
    dx0 = 1.0e5 / 64
    pi = lambda x: sy.RHO_I * sy.GRAV * (6.0 * (np.sqrt(x + 5000.0) - np.sqrt(5000.0)) + 1.0)
    p0 = sy.shmip_amrm_states(64, 32, [], rough=0.5)[0][0]["Pi"][1:-1, 1:-1]
    t0 = ((p0 > pi(20 * dx0)) & (p0 < pi(28 * dx0))).astype(np.uint8)
    assert list(np.nonzero(t0.any(axis=0))[0]) == list(range(20, 28)) and t0[:, 20:28].all()
    p1 = pi((np.arange(128) + 0.5) * dx0 / 2)
    t1 = np.zeros((64, 128), dtype=np.uint8)
    t1[:, (p1 > pi(44 * dx0 / 2)) & (p1 < pi(52 * dx0 / 2))] = 1
    t1 = ts.restrict(t1, 1, [(0, 16, 127, 47)])
    assert t1[16:48, 44:52].all() and t1.sum() == 32 * 8
    params = dict(fill_ratio=0.7, block_factor=2, max_box_size=32, nesting_radius=2)
    gen = model.generate_grids(64, 32, (0, 0), [t0, t1], **params)
    assert gen == [[(40, 0, 55, 31), (40, 32, 55, 63)], [(88, 32, 103, 63), (88, 64, 103, 95)]] and hl.valid(64, 32, [0, 0], gen)
    assert model.generate_grids(64, 32, (0, 0), [t0], **params) == gen[:1]
