"""Cell tagging on the device (suhmo_hier_tag_cells / suhmo_level_tag_cells, suhmo_amd/csrc/suhmo_tags.hip) against the numpy twin of
tests/gridgen_ref.py, entry by entry, on the 32 x 16 base over hierarchies of tests/hierlayouts.py; then tagging and box generation together
(suhmo_hier_generate_grids, model.initial_grids) up to a hierarchy that is created from generated boxes and solves."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import gridgen_ref as gr
from tests import hierlayouts as hl

pytestmark = pytest.mark.gpu
NX0, NY0 = hl.NX0, hl.NY0
SEEDS = range(12)                       # seed % 4: the periodicity, (seed // 4) % 3: 2, 3, 4 levels
VMIN, VMAX = 0.95, 0.98
# (grow, grow_dir, granularity): no growth, the square, beyond it in one direction; entries of 1, 2 and 4 cells
REACH = ((0, (0, 0), 1), (1, (0, 0), 2), (3, (0, 0), 4), (1, (4, 0), 1), (0, (0, 2), 2), (2, (1, 5), 4), (3, (0, 0), 1))


def hier_model(bc, boxes, ph=sy.CFG3_PHYS):
    from suhmo_amd import model
    return model.HipHierModel(NX0, NY0, 1.0, 1.0, bc, ph, sy.A3_MODEL, boxes, max_box=16)


def level_boxes(boxes, l):
    return [(0, 0, NX0 - 1, NY0 - 1)] if l == 0 else boxes[l - 1]


def draw(rng, box):
    """valid cells of a box: 3 % inside (VMIN, VMAX), values exactly at either bound, NaN and both infinities sprinkled in, and the four corner
    cells inside -- their grown squares reach the neighbouring box, cells of no box and, for boxes on a domain side, beyond the domain"""
    nx, ny = box[2] - box[0] + 1, box[3] - box[1] + 1
    u = rng.random((ny, nx))
    v = np.where(u < 0.03, rng.uniform(0.951, 0.979, size=(ny, nx)), rng.uniform(0.0, 0.9, size=(ny, nx)))
    for special in (VMIN, VMAX, np.nan, np.inf, -np.inf):
        v[int(rng.integers(0, ny)), int(rng.integers(0, nx))] = special
    v[0, 0] = v[0, -1] = v[-1, 0] = v[-1, -1] = 0.96
    return v


def load(M, l, name, vals, ghost=None):
    """vals[k]: valid cells of box k of level l; ghost: the value of the whole ghost ring (a ghosted load), else valid cells only"""
    fid = M.FIELDS[name]
    for k, v in enumerate(vals):
        if ghost is None:
            M.level[l][k].set(fid, v)
        else:
            M.level[l][k].set(fid, np.pad(v, 1, constant_values=ghost), ghosted=True)


def pieces(bl, vals):
    return [(b[0], b[1], v) for b, v in zip(bl, vals)]


@pytest.mark.parametrize("seed", SEEDS)
def test_hier_tags_equal_the_twin(seed):
    from suhmo_amd import capi
    bc, boxes = hl.generate(seed)
    rng = np.random.default_rng([seed, 8803])
    M = hier_model(bc, boxes)
    for l in range(len(boxes) + 1):
        nx, ny, bl = NX0 << l, NY0 << l, level_boxes(boxes, l)
        assert M.tags(l) is None
        a, b = [draw(rng, bx) for bx in bl], [draw(rng, bx) for bx in bl]
        load(M, l, "mR", a)
        load(M, l, "Pw", b)
        for grow, gd, g in REACH:
            M.clear_tags(l)
            M.tag_cells(l, "mR", VMIN, VMAX, grow=grow, grow_dir=gd, granularity=g)
            want = gr.tag_map(nx, ny, pieces(bl, a), VMIN, VMAX, grow, gd, g)
            assert want.any()
            assert np.array_equal(M.tags(l), want), (seed, l, grow, gd, g)
        # everything finite: NaN and the infinities stay out
        M.clear_tags(l)
        M.tag_cells(l, "mR", -np.inf, np.inf)
        want = gr.tag_map(nx, ny, pieces(bl, a), -np.inf, np.inf)
        got = M.tags(l)
        assert np.array_equal(got, want)
        assert got.sum() == sum(np.isfinite(v).sum() for v in a)
        # two calls form the union; a map keeps its granularity; clear
        M.clear_tags(l)
        M.tag_cells(l, "mR", VMIN, VMAX, grow=1, granularity=2)
        M.tag_cells(l, "Pw", VMIN, VMAX, grow=0, grow_dir=(2, 0), granularity=2)
        want = gr.tag_map(nx, ny, pieces(bl, a), VMIN, VMAX, 1, (0, 0), 2)
        want = gr.tag_map(nx, ny, pieces(bl, b), VMIN, VMAX, 0, (2, 0), 2, into=want)
        assert np.array_equal(M.tags(l), want)
        with pytest.raises(capi.SuhmoError):
            M.tag_cells(l, "mR", VMIN, VMAX, granularity=4)
        assert np.array_equal(M.tags(l), want)
        # a ghost ring full of in-range values tags nothing; with a few valid cells in range: exactly those
        M.clear_tags(l)
        quiet = [np.zeros_like(v) for v in a]
        load(M, l, "B", quiet, ghost=0.96)
        M.tag_cells(l, "B", VMIN, VMAX, grow=1)
        assert not M.tags(l).any()
        load(M, l, "B", a, ghost=0.96)
        M.tag_cells(l, "B", VMIN, VMAX, grow=1)
        assert np.array_equal(M.tags(l), gr.tag_map(nx, ny, pieces(bl, a), VMIN, VMAX, 1))
    M.clear_tags()
    assert all(M.tags(l) is None for l in range(len(boxes) + 1))
    M.close()


@pytest.mark.parametrize("nx,ny", [(4, 4), (136, 8)])
def test_level_tags_equal_the_twin(nx, ny):
    """suhmo_level_tag_cells, the OnLevel instantiation: the smallest level, and a width that leaves the third workgroup of a row partly filled"""
    from suhmo_amd import model
    rng = np.random.default_rng([nx, ny, 8804])
    M = model.HipModel(nx, ny, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS, sy.A3_MODEL, max_box=4 if nx == 4 else 8)
    assert M.tags() is None
    v = draw(rng, (0, 0, nx - 1, ny - 1))
    M.level.set(M.FIELDS["mR"], v)
    for grow, gd, g in REACH:
        M.clear_tags()
        M.tag_cells("mR", VMIN, VMAX, grow=grow, grow_dir=gd, granularity=g)
        assert np.array_equal(M.tags(), gr.tag_map(nx, ny, [(0, 0, v)], VMIN, VMAX, grow, gd, g)), (grow, gd, g)
    M.clear_tags()
    assert M.tags() is None
    M.close()


TAG_LEVELS = dict(fill_ratio=0.7, block_factor=4, max_box_size=16)


@pytest.mark.parametrize("seed", (1, 6, 11))
def test_generate_on_a_hierarchy_equals_the_host_call_on_its_maps(seed):
    from suhmo_amd import model
    bc, boxes = hl.generate(seed)
    rng = np.random.default_rng([seed, 8805])
    M = hier_model(bc, boxes)
    for l in range(len(boxes) + 1):
        load(M, l, "mR", [draw(rng, bx) for bx in level_boxes(boxes, l)])
        M.tag_cells(l, "mR", VMIN, VMAX, grow=1, granularity=2)
    got, same = M.generate_grids(**TAG_LEVELS)
    maps = [M.tags(l) for l in range(len(boxes) + 1)]
    assert got == model.generate_grids(NX0, NY0, bc["periodic"], maps, **TAG_LEVELS)
    assert got == gr.generate(NX0, NY0, bc["periodic"], maps, **TAG_LEVELS)
    assert len(got) == len(boxes) + 1 and not same and hl.valid(NX0, NY0, bc["periodic"], got)
    M.close()


OWN = dict(fill_ratio=0.6, block_factor=2, max_box_size=16)


def _own_tags():
    """tag cells per level, each inside the level the tags below it generate"""
    t0, t1 = np.zeros((NY0, NX0), dtype=np.uint8), np.zeros((2 * NY0, 2 * NX0), dtype=np.uint8)
    t0[5:9, 9:14] = 1; t0[6, 14] = 1; t0[10:12, 20:23] = 1
    t1[12:15, 20:25] = 1
    return [t0, t1]


def _load_tags(M, boxes, tags):
    """a melt rate that is 1 on the tagged cells and 0 elsewhere, on every box"""
    for l, t in enumerate(tags):
        bl = level_boxes(boxes, l)
        load(M, l, "mR", [t[b[1]:b[3] + 1, b[0]:b[2] + 1].astype(float) for b in bl])
        assert sum(t[b[1]:b[3] + 1, b[0]:b[2] + 1].sum() for b in bl) == t.sum()          # every tag lies in a box of its level


def test_same_a_generated_hierarchy_solves():
    from suhmo_amd import model
    bc = hl._NP
    tags = _own_tags()
    boxes = model.generate_grids(NX0, NY0, bc["periodic"], tags, **OWN)
    assert len(boxes) == 2 and hl.valid(NX0, NY0, bc["periodic"], boxes)
    M = hier_model(bc, boxes)
    # the tags that made the boxes, found again on the device: the hierarchy's own grids, in the order given or another
    _load_tags(M, boxes, tags)
    for l in range(2):
        M.tag_cells(l, "mR", 0.5, 2.0)
    got, same = M.generate_grids(**OWN)
    assert got == boxes and same
    M.close()
    M = hier_model(bc, [bl[::-1] for bl in boxes])
    _load_tags(M, [bl[::-1] for bl in boxes], tags)
    for l in range(2):
        M.tag_cells(l, "mR", 0.5, 2.0)
    got, same = M.generate_grids(**OWN)
    assert got == boxes and same
    # one more tag: other grids
    one = np.zeros((NY0, NX0)); one[2, 28] = 1.0
    M.level[0][0].set(M.FIELDS["Pw"], one)
    M.tag_cells(0, "Pw", 0.5, 2.0)
    got, same = M.generate_grids(**OWN)
    assert not same and got == model.generate_grids(NX0, NY0, bc["periodic"], [np.maximum(tags[0], one.astype(np.uint8)), tags[1]], **OWN)
    M.close()
    # created from generated boxes, a V-cycle, a finite head on every box
    from suhmo_amd.level import F_PHI
    fs = hl.analytic_fields(NX0, NY0, boxes, bc)
    M = hier_model(bc, boxes)
    M.hier.set_inputs(fs)
    r0 = M.hier.residual()
    M.hier.vcycle(dict(sy.SOLVER_DEFAULT))
    r1 = M.hier.residual()
    assert np.isfinite(r0) and np.isfinite(r1)
    for l in range(3):
        for L in M.level[l]:
            assert np.isfinite(L.get(F_PHI)).all()
    M.close()


def _bump(l, box, everywhere=True):
    """a melt-rate bump around (10.3, 7.6) base cells, sampled at the cell centres of a box of level l"""
    if l > 0 and not everywhere:
        return np.zeros((box[3] - box[1] + 1, box[2] - box[0] + 1))
    h = 1.0 / (1 << l)
    x, y = (np.arange(box[0], box[2] + 1) + 0.5) * h, (np.arange(box[1], box[3] + 1) + 0.5) * h
    return np.exp(-((x[None, :] - 10.3) ** 2 + (y[:, None] - 7.6) ** 2) / 6.0)


@pytest.mark.parametrize("everywhere,levels", [(True, 2), (False, 1)])
def test_initial_grids(everywhere, levels):
    """the loop of initGrids from a melt-rate bump: level 0 alone, then one more level per pass up to max_level = 2; with the bump loaded on level 0
    only, level 1 tags nothing and the loop stops with one refined level"""
    from suhmo_amd import model
    bc, made = hl._PY, []

    def make_model(boxes):
        made.append(boxes)
        if not boxes:
            M = model.HipModel(NX0, NY0, 1.0, 1.0, bc, sy.CFG3_PHYS, sy.A3_MODEL, max_box=16)
            M.level.set(M.FIELDS["mR"], _bump(0, (0, 0, NX0 - 1, NY0 - 1)))
            return M
        M = hier_model(bc, boxes)
        for l in range(len(boxes) + 1):
            load(M, l, "mR", [_bump(l, b, everywhere) for b in level_boxes(boxes, l)])
        return M

    params = dict(fill_ratio=0.7, block_factor=4, max_box_size=32, nesting_radius=2)
    boxes, M = model.initial_grids(make_model, [dict(name="meltingRate", vmin=0.6, vmax=1e30, grow=1)], params, max_level=2)
    assert len(boxes) == levels and hl.valid(NX0, NY0, bc["periodic"], boxes)
    assert [len(b) for b in made] == list(range(levels + 1)) and made[-1] == boxes
    # the grids are the twin's from the twin's tags (the bump's tags lie inside level 1 whichever pass made it)
    t = [gr.tag_map(NX0 << l, NY0 << l, [(b[0], b[1], _bump(l, b, everywhere)) for b in level_boxes(boxes, l)], 0.6, 1e30, 1, (0, 0), 2)
         for l in range(len(boxes))]
    assert boxes == gr.generate(NX0, NY0, bc["periodic"], t, **params)
    if everywhere:                                            # level 2's margin widened level 1 beyond what level 0's own tags ask for
        assert boxes[:1] != gr.generate(NX0, NY0, bc["periodic"], t[:1], **params)
    M.close()
