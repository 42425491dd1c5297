"""The numpy twin of the device IBCs (tests/ibc_ref.py) against the states every other test is pinned by (suhmo_amd/synthetic.py), bit for bit,
so that the twin cannot drift from them; the ghost sequences on a case small enough to state by hand; the C-ABI's table.  No device."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import hierlayouts as hl
from tests import ibc_ref as ir

KEYS = ("head", "B", "Pi", "zb", "mask")


def same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("nx,ny,slope", [(64, 16, 0.0), (62, 2, 0.02), (130, 9, 1.0e-3)])
def test_sqrt_twin_equals_shmip_initial_state(nx, ny, slope):
    want = sy.shmip_initial_state(nx, ny, slope=slope)
    got = ir.initial("sqrt", ir.params(slope=slope), ir.geom(0, 0, nx, ny, want["dx"], want["dy"]))
    same(got, want, (nx, ny))
    assert (got["B"] == 1.0e-16).any() and (got["B"] == 0.01).any(), "both sides of the gap threshold"


@pytest.mark.parametrize("seed", [0, 5])
def test_sqrt_twin_equals_shmip_amrm_states_on_boxes(seed):
    _, boxes = hl.generate(seed)
    sts = sy.shmip_amrm_states(hl.NX0, hl.NY0, boxes, rough=0)
    dx0, dy0 = sts[0][0]["dx"], sts[0][0]["dy"]
    for l in range(len(boxes) + 1):
        bl = [(0, 0, hl.NX0 - 1, hl.NY0 - 1)] if l == 0 else boxes[l - 1]
        for g, want in zip(ir.box_geoms(hl.NX0, hl.NY0, dx0, dy0, (0, 0), l, bl), sts[l]):
            same(ir.initial("sqrt", ir.params(), g), want, (seed, l, g["i0"], g["j0"]))


@pytest.mark.parametrize("case", sorted(sy.E_GAMMA))
@pytest.mark.parametrize("nx,ny", [(64, 16), (128, 32)])
def test_valley_twin_equals_valley_initial_state(case, nx, ny):
    want = sy.valley_initial_state(nx, ny, sy.E_GAMMA[case])
    p = ir.params(gamma=sy.E_GAMMA[case])
    g = ir.geom(0, 0, nx, ny, want["dx"], want["dy"])
    got = ir.initial("valley", p, g)
    same(got, want, (case, nx, ny))
    # what lets the device's mask and gap pattern be compared exactly although its pow differs in the last bits: no cell near the margin
    X, Y = ir.positions(g)
    S, zb, _ = ir._valley(p, X, Y - 750.0)
    assert np.abs(S - zb).min() >= 0.03 and got["head"].min() >= 0.0
    assert (got["mask"] < 0).any() and (got["mask"] > 0).any()


def valley_margin(p, g):
    """(least |surface - bed|, least |head before resetCovered|) over the ghosted box"""
    X, Y = ir.positions(g)
    S, zb, Pi = ir._valley(p, X, Y - 750.0)
    head = Pi * 0.5 * (1.0 / (p["rho_w"] * p["gravity"])) + zb
    return float(np.abs(S - zb).min()), float(np.abs(head).min())


def test_every_valley_input_of_the_gpu_tests_keeps_its_cells_away_from_the_margin():
    """tests/test_gpu_ibc.py compares the valley's mask, its pattern b == 1e-16 and the clamp of its head EXACTLY although the device's pow differs
    from numpy's in the last bits (relative 1e-13 at most, i.e. below 1e-9 m here).  That holds when no cell has |surface - bed| or |head| near 0:
    here every geometry and gamma those tests use -- the odd single levels under all three periodicities, every box of the twelve generated
    layouts, the ensemble's and the end-to-end grids, the regrid and run cases -- keeps 0.03 m of ice and 1e-3 m of head away from it"""
    from tests import test_gpu_hier_run as hr
    lx, ly = 6000.0, 1500.0
    cases = []
    for nx, ny in [(62, 2), (70, 5), (130, 9), (64, 16)]:
        for per in [(0, 0), (0, 1), (1, 1)]:
            for gamma in sorted(set(sy.E_GAMMA.values()) | {0.05, -0.5}):
                cases.append((ir.params(gamma=gamma), ir.geom(0, 0, nx, ny, lx / nx, ly / ny, periodic=per)))
    for seed in range(12):
        bc, boxes = hl.generate(seed)
        for l in range(len(boxes) + 1):
            bl = [(0, 0, hl.NX0 - 1, hl.NY0 - 1)] if l == 0 else boxes[l - 1]
            for g in ir.box_geoms(hl.NX0, hl.NY0, lx / hl.NX0, ly / hl.NY0, tuple(bc["periodic"]), l, bl):
                cases += [(ir.params(gamma=gamma), g) for gamma in (0.05, -0.5)]
    for lists, gamma in ((hr.OLD, -0.1), (hr.GEN, -0.1), ([[(32, 16, 63, 47)]], 0.05)):          # the regrid case; the seasonal run's first grids
        for l in range(len(lists) + 1):
            bl = [(0, 0, 63, 31)] if l == 0 else lists[l - 1]
            cases += [(ir.params(gamma=gamma), g) for g in ir.box_geoms(64, 32, lx / 64, ly / 32, (0, 0), l, bl)]
    assert len(cases) > 250
    for p, g in cases:
        ice, head = valley_margin(p, g)
        assert ice >= 0.03 and head >= 1.0e-3, (p["gamma"], g, ice, head)
    # the regrid case: the mask is made from the STORED Pi, whose ghost cells are interpolated or extrapolated -- each is 0 or far from 0
    p, geo = ir.params(gamma=-0.1), (64, 32, lx / 64, ly / 32, (0, 0))
    old = ir.hier_init("valley", p, *geo, hr.OLD)
    for bl in ir.regrid_with_reload("valley", p, *geo, hr.OLD, hr.GEN, old[1:], old[0][0]):
        for st in bl:
            assert ((st["Pi"] == 0.0) | (np.abs(st["Pi"]) >= 1.0)).all()


def test_dino_twin_equals_mountain_state():
    for (nx, ny, i0, j0, nxg, nyg) in [(32, 32, 0, 0, 32, 32), (16, 24, 40, 8, 64, 64), (30, 10, 98, 118, 128, 128)]:
        want = sy.mountain_state(nx, ny, i0, j0, nxg, nyg)
        got = ir.initial("dino", ir.params(), ir.geom(i0, j0, nx, ny, want["dx"], want["dy"], nxg, nyg))
        same(got, want, (nx, ny, i0, j0))


def test_periodic_images_are_what_wrap_ghosts_demands():
    bc = dict(sy.CONV_BC, periodic=[1, 1])
    for kind in ir.KINDS:
        g = ir.geom(0, 0, 12, 6, 500.0, 250.0, periodic=(1, 1))
        st = ir.level_init(kind, ir.params(slope=0.01, gamma=-0.1), g)
        want = sy.wrap_ghosts({k: st[k].copy() for k in ("B", "Pi", "zb", "mask")}, bc)
        for k in ("B", "Pi", "zb", "mask"):
            assert np.array_equal(st[k], want[k]), (kind, k)


def test_level_init_copies_bed_and_mask_into_the_side_ghosts_only():
    g = ir.geom(0, 0, 10, 4, 1000.0, 1000.0)
    raw, st = ir.initial("sqrt", ir.params(slope=0.02), g), ir.level_init("sqrt", ir.params(slope=0.02), g)
    assert np.array_equal(st["zb"][1:-1, 0], st["zb"][1:-1, 1]) and not np.array_equal(raw["zb"][1:-1, 0], raw["zb"][1:-1, 1])
    for k in ("zb", "mask"):
        for c in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            assert st[k][c] == raw[k][c], "corner ghosts are written by nobody"
    for k in ("Pi", "B", "head", "zs", "Pw", "mR"):
        assert np.array_equal(st[k], raw[k])


def test_reload_order_matters_where_the_dino_margin_meets_a_coarse_fine_side():
    """ibc_ref.ORDER_CASE: at ghost cell (87, 62) of level 2 the formula gives ice, at its parent (43, 31) on level 1 none.  The level-1 reload sets the parent's gap
    height to 1e-16 and the limiter leaves the ghost cell the parent's value: 1e-16 when level 1 is reloaded BEFORE level 2 interpolates
    (the reference's loop), the transferred gap height otherwise"""
    c = ir.ORDER_CASE
    old = ir.hier_init("dino", ir.params(), *c["geo"], c["old"])
    for bl in old:
        for st in bl:
            st["B"] = np.full_like(st["B"], c["B"])
    a = ir.regrid_with_reload("dino", ir.params(), *c["geo"], c["old"], c["new"], old[1:], old[0][0])
    b = ir.regrid_with_reload("dino", ir.params(), *c["geo"], c["old"], c["new"], old[1:], old[0][0], reload_first=False)
    l, k, jj, ii = c["where"]
    assert a[l - 1][k]["B"][jj, ii] == 1.0e-16 and b[l - 1][k]["B"][jj, ii] == c["B"]
    for f in ir.NAMES:
        if f != "B":
            assert all(np.array_equal(x[f], y[f]) for la, lb in zip(a, b) for x, y in zip(la, lb)), f


def test_the_new_symbols_are_in_the_table():
    from suhmo_amd import capi
    for s in ("suhmo_level_ibc_init", "suhmo_hier_ibc_init", "suhmo_batch_ibc_init", "suhmo_hier_set_ibc", "suhmo_hier_ibc_reload"):
        assert s in capi.SYMBOLS
    assert [n for n, _ in capi.Ibc._fields_] == ["kind", "slope", "ice_height", "gap_init", "rho_i", "rho_w", "gravity", "G", "L", "gamma"]
    assert capi.IBC_KINDS == dict(basic=0, sqrt=1, valley=2, dino=3)
