"""suhmo_grids_generate (include/suhmo_hip.h, "GRID GENERATION"; suhmo_amd/csrc/suhmo_tags.hip): the host step from tag maps to the box lists
suhmo_hier_create takes.  No device: hand cases with the lists worked out on paper from the rules of the header, a seeded sweep against the numpy
twin (tests/gridgen_ref.py, written from the same text) and against the properties the rules promise, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import gridgen_ref as gr
from tests import hierlayouts as hl

NX0, NY0 = hl.NX0, hl.NY0                 # 32 x 16
HAND = dict(fill_ratio=0.7, block_factor=2, max_box_size=16)      # blocks of 2 cells, at most 8 blocks a side; the map of level 0 is 16 x 32


@pytest.fixture(scope="module")
def model():
    from suhmo_amd import capi, model
    capi.build()
    capi.lib()
    return model


def tags0(*rects):
    """level-0 map at granularity 1 with the rectangles (i0, j0, i1, j1) of entries set"""
    t = np.zeros((NY0, NX0), dtype=np.uint8)
    for i0, j0, i1, j1 in rects:
        t[j0:j1 + 1, i0:i1 + 1] = 1
    return t


def blocks(*rects):
    """rectangles in blocks -> boxes in cells of the generated level (block_factor 2)"""
    return [(2 * a, 2 * b, 2 * c + 1, 2 * d + 1) for a, b, c, d in rects]


def test_one_tag_one_block(model):
    assert model.generate_grids(NX0, NY0, (0, 0), [tags0((7, 5, 7, 5))], **HAND) == [blocks((7, 5, 7, 5))]


def test_solid_rectangle_is_bisected_to_max_box_size(model):
    """20 x 6 blocks, efficiency 1, 20 > 8: no hole, a constant signature has no inflection, so rule (c): 10 + 10, then 5 + 5"""
    assert model.generate_grids(NX0, NY0, (0, 0), [tags0((3, 4, 22, 9))], **HAND) == [blocks((3, 4, 7, 9), (8, 4, 12, 9), (13, 4, 17, 9), (18, 4, 22, 9))]


def test_two_clusters_split_at_the_hole(model):
    """columns 2-4 and 9-11 over rows 2-5: efficiency 24 / 40 < 0.7; holes 5 .. 8, the centre of [2, 11] is 6.5: 6 and 7 tie, the lower wins;
    [2, 5] and [7, 11] shrink to the clusters"""
    assert model.generate_grids(NX0, NY0, (0, 0), [tags0((2, 2, 4, 5), (9, 2, 11, 5))], **HAND) == [blocks((2, 2, 4, 5), (9, 2, 11, 5))]


def test_l_shape_split_at_its_inflection(model):
    """an L of columns 2-4 x rows 2-11 and rows 2-4 x columns 2-13: 57 of 120, no hole.  Sx = 10 10 10 3 ...: D = 0 -7 7 0 ..., strength 14;
    Sy = 12 12 12 3 ...: D = 0 -9 9 0 ..., strength 18: the cut is in y between rows 4 and 5.  The lower arm (12 x 3, full) is too long: bisected;
    the upper arm is one box"""
    assert model.generate_grids(NX0, NY0, (0, 0), [tags0((2, 2, 4, 11), (2, 2, 13, 4))], **HAND) == [blocks((2, 2, 7, 4), (8, 2, 13, 4), (2, 5, 4, 11))]


def test_full_domain(model):
    """32 x 16 blocks: x is bisected twice (16, then 8), then each 8 x 16 piece in y; the lower part first"""
    want = blocks(*[(8 * a, 8 * b, 8 * a + 7, 8 * b + 7) for a in range(4) for b in range(2)])
    assert model.generate_grids(NX0, NY0, (0, 0), [np.ones((NY0, NX0), dtype=np.uint8)], **HAND) == [want]


def test_a_tag_in_each_corner(model):
    """holes in x first (the longer side): 15 and 16 tie around 15.5, the lower wins; either half is a column that splits at its hole in y"""
    t = tags0((0, 0, 0, 0), (31, 0, 31, 0), (0, 15, 0, 15), (31, 15, 31, 15))
    assert model.generate_grids(NX0, NY0, (0, 0), [t], **HAND) == [blocks((0, 0, 0, 0), (0, 15, 0, 15), (31, 0, 31, 0), (31, 15, 31, 15))]


def _three_levels():
    t0, t1, t2 = tags0((1, 8, 1, 8)), np.zeros((2 * NY0, 2 * NX0), dtype=np.uint8), np.zeros((4 * NY0, 4 * NX0), dtype=np.uint8)
    t1[16, 2] = 1
    t2[32, 0] = 1
    return [t0, t1, t2]


def test_nesting_forces_tags_across_a_periodic_side(model):
    """level 3's box (0, 64, 1, 65) is cell (0, 32) of level 2; grown by 2 it is columns -2 .. 2 -> 126, 127, 0, 1, 2 of 128, rows 30 .. 34: entries
    {63, 0, 1} x {15, 16, 17} of level 1, which with the level's own tag (2, 16) make a 3 x 3 box of 7 tags (0.78) and a column across the wrap.
    Their margins in turn tag {31, 0, 1, 2} x {6 .. 9} and {30, 31, 0} x {6 .. 9} of level 0"""
    got = model.generate_grids(NX0, NY0, (1, 0), _three_levels(), **HAND)
    assert got == [[(0, 12, 5, 19), (60, 12, 63, 19)], [(0, 30, 5, 35), (126, 30, 127, 35)], [(0, 64, 1, 65)]]
    assert hl.valid(NX0, NY0, (1, 0), got)


def test_nesting_margin_is_dropped_at_a_non_periodic_side(model):
    got = model.generate_grids(NX0, NY0, (0, 0), _three_levels(), **HAND)
    assert got == [[(0, 12, 5, 19)], [(0, 30, 5, 35)], [(0, 64, 1, 65)]]
    assert hl.valid(NX0, NY0, (0, 0), got)


def test_nesting_radius_below_two_is_raised(model):
    a = model.generate_grids(NX0, NY0, (0, 0), _three_levels(), nesting_radius=0, **HAND)
    assert a == model.generate_grids(NX0, NY0, (0, 0), _three_levels(), nesting_radius=2, **HAND)
    b = model.generate_grids(NX0, NY0, (0, 0), _three_levels(), nesting_radius=4, **HAND)
    assert b == gr.generate(NX0, NY0, (0, 0), _three_levels(), nesting_radius=4, **HAND) and b != a


def test_levels_above_an_empty_one_are_dropped(model):
    t = _three_levels()
    t[1][:] = 0
    assert model.generate_grids(NX0, NY0, (0, 0), t, **HAND) == [blocks((1, 8, 1, 8))]
    t[0][:] = 0
    assert model.generate_grids(NX0, NY0, (0, 0), t, **HAND) == []


def _cloud(rng, shape):
    """a random tag cloud: a few blobs of random extent and density, and a few lone tags"""
    ny, nx = shape
    t = np.zeros(shape, dtype=np.uint8)
    for _ in range(int(rng.integers(1, 5))):
        w, h = int(rng.integers(1, max(2, nx // 2))), int(rng.integers(1, max(2, ny // 2)))
        i, j = int(rng.integers(0, nx - w + 1)), int(rng.integers(0, ny - h + 1))
        t[j:j + h, i:i + w] |= (rng.random((h, w)) < rng.uniform(0.3, 1.0)).astype(np.uint8)
    for _ in range(int(rng.integers(0, 4))):
        t[int(rng.integers(0, ny)), int(rng.integers(0, nx))] = 1
    if not t.any():
        t[int(rng.integers(0, ny)), int(rng.integers(0, nx))] = 1
    return t


def _sweep_case(seed):
    rng = np.random.default_rng([seed, 7411])
    periodic = (seed % 4 & 1, seed % 4 >> 1)
    p = dict(fill_ratio=(0.5, 0.7, 0.9)[(seed // 4) % 3], block_factor=(2, 4, 8)[(seed // 12) % 3], max_box_size=(8, 16, 32)[int(rng.integers(0, 3))])
    ntag, g = 1 + seed % 3, p["block_factor"] // 2
    return periodic, p, [_cloud(rng, ((NY0 << l) // g, (NX0 << l) // g)) for l in range(ntag)]


def test_seeded_sweep(model):
    """200 tag clouds over the four periodicities, three fill ratios, three block factors, three box sizes and one to three tag levels: the twin's
    list, order included; a hierarchy suhmo_hier_create accepts; every tag (the nesting tags of the levels above included) covered; every box the
    bounding box of its tags, efficient, small enough and block-aligned; the same answer twice"""
    seen = set()
    for seed in range(200):
        periodic, p, tags = _sweep_case(seed)
        seen.add((periodic, p["fill_ratio"], p["block_factor"], p["max_box_size"], len(tags)))
        got = model.generate_grids(NX0, NY0, periodic, tags, **p)
        assert got == gr.generate(NX0, NY0, periodic, tags, **p), seed
        assert got == model.generate_grids(NX0, NY0, periodic, tags, **p), seed
        assert len(got) == len(tags), seed                      # every cloud has a tag, so no level is dropped
        assert hl.valid(NX0, NY0, periodic, got), seed
        b, g = p["block_factor"], p["block_factor"] // 2
        for l in range(len(tags) - 1, -1, -1):
            T = tags[l] != 0
            if l + 2 <= len(got):                               # what the level above forces into this map
                for box in got[l + 1]:
                    for I, J in gr.nesting_tags(box, (NX0 << (l + 1), NY0 << (l + 1)), periodic, g, 2):
                        T[J, I] = True
            covered = np.zeros_like(T)
            for lo0, lo1, hi0, hi1 in got[l]:
                assert lo0 % b == 0 and lo1 % b == 0 and (hi0 + 1) % b == 0 and (hi1 + 1) % b == 0, (seed, l)
                I0, J0, I1, J1 = lo0 // b, lo1 // b, hi0 // b, hi1 // b
                assert I1 - I0 + 1 <= p["max_box_size"] // b and J1 - J0 + 1 <= p["max_box_size"] // b, (seed, l)
                sub = T[J0:J1 + 1, I0:I1 + 1]
                assert sub.sum() / sub.size >= p["fill_ratio"], (seed, l)
                assert sub[0].any() and sub[-1].any() and sub[:, 0].any() and sub[:, -1].any(), (seed, l)       # the bounding box of its tags
                assert not covered[J0:J1 + 1, I0:I1 + 1].any(), (seed, l)
                covered[J0:J1 + 1, I0:I1 + 1] = True
            assert not (T & ~covered).any(), (seed, l)
    assert len({s[0] for s in seen}) == 4 and {s[1] for s in seen} == {0.5, 0.7, 0.9} and {s[2] for s in seen} == {2, 4, 8}
    assert {s[3] for s in seen} == {8, 16, 32} and {s[4] for s in seen} == {1, 2, 3}


def _raw(model, tags, cap, **p):
    from suhmo_amd import capi
    ucp = C.POINTER(C.c_ubyte)
    ptr = (ucp * max(len(tags), 1))(*[t.ctypes.data_as(ucp) for t in tags])
    gp = capi.GridParams(p["fill_ratio"], p["block_factor"], p["max_box_size"], 2)
    nlev, nbox, flat = C.c_int(-7), (C.c_int * 8)(), (C.c_int * (4 * max(cap, 1)))()
    rc = capi.lib().suhmo_grids_generate(NX0, NY0, (C.c_int * 2)(0, 0), C.byref(gp), len(tags), ptr, C.byref(nlev), nbox, flat, cap)
    return rc, nlev.value, list(nbox), capi.lib().suhmo_last_error().decode()


def test_refusals(model):
    t = [tags0((3, 4, 22, 9))]
    rc, _, _, msg = _raw(model, t, 16, fill_ratio=0.7, block_factor=3, max_box_size=12)
    assert rc == -1 and "block_factor" in msg
    rc, _, _, msg = _raw(model, t, 16, fill_ratio=0.7, block_factor=4, max_box_size=18)
    assert rc == -1 and "max_box_size" in msg
    rc, nlev, nbox, msg = _raw(model, t, 3, **HAND)             # four boxes, room for three: the needed count comes back
    assert rc < 0 and nlev == 2 and nbox[1] == 4 and "4" in msg
    rc, nlev, nbox, _ = _raw(model, t, 4, **HAND)
    assert rc == 0 and nlev == 2 and nbox[1] == 4
    rc, _, _, _ = _raw(model, [], 16, **HAND)                   # ntag = 0
    assert rc == -1
    from suhmo_amd import capi
    with pytest.raises(capi.SuhmoError):
        model.generate_grids(NX0, NY0, (0, 0), t, fill_ratio=0.7, block_factor=3, max_box_size=12)
