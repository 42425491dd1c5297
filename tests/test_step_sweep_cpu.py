"""The time-step sweep of tests/stepsweep.py on the CPU oracle alone (oracle/time_loop.c, oracle/amr_step_m.c): nothing in it hides a failure (every
compared field finite, cd NaN exactly where the census says 0/0, no step raises, no Picard loop past 20 iterations, no head solve ending on
max_iter), every arm of every branch the sweep is after is taken (the census, printed and pinned by tests/golden/STEP_SWEEP_CENSUS.txt), and the
sweep contains the cases it claims.  tests/test_gpu_step_sweep.py compares the device with the oracle on the same cases, bitwise."""
import os

import pytest

from tests import hierlayouts as hl
from tests import stepsweep as sw

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "STEP_SWEEP_CENSUS.txt")


@pytest.fixture(scope="module")
def sweep(oracle):
    """two steps of every case on the oracle, once for the module"""
    return sw.sweep_census(oracle)


def test_the_tables_hold_what_the_sweep_claims():
    assert sw.SHAPES == ((12, 4), (40, 24), (72, 20), (24, 36))
    per = {tuple(bc["periodic"]) for bc in sw.BCS.values()}
    assert per == {(0, 0), (0, 1), (1, 0), (1, 1)} and sw.BCS["dirichlet"]["value"][0] == [2.0, 900.0]
    rows = {r: sw.model_of(r) for r in sw.ROWS}
    for r, m in rows.items():
        if r != "no-friction-unmasked-rhs":
            assert m["use_mask_rhs_b"] == 1 and m["G"] != 0.0, r
    assert all(sw.PHYS[k] == v for k, v in dict(use_mask_gradients=1, cutOffB=1, cutOffbr=0.02, maxOffbr=0.08).items())
    has = lambda **kw: any(all(m.get(k, 0) == v for k, v in kw.items()) for m in rows.values())
    assert has(diffFactor=0.0, use_impl_diff=0) and has(diffFactor=1.0, use_impl_diff=0) and has(diffFactor=1.0, use_impl_diff=1)
    assert has(diffFactor=0.5, use_impl_diff=1, freeze_icefree_gap=1, head_melt_off=1) and has(basal_friction=0, use_mask_rhs_b=0, G=0.0)
    assert any(m.get("use_moulin_source") and m.get("ramp", 1.0) != 1.0 for m in rows.values())
    # at most one (BC, row) combination in ten dropped, no whole row, no whole BC
    combos = len(sw.BCS) * len(sw.ROWS)
    assert 10 * len(sw.DROPPED) <= combos and all(reason for reason in sw.DROPPED.values())
    kept = {(c[3], c[4]) for c in sw.single_cases()}
    assert {b for b, _ in kept} == set(sw.BCS) and {r for _, r in kept} == set(sw.ROWS)
    assert len(sw.single_cases()) == len(sw.SHAPES) * (combos - len(sw.DROPPED))


def test_planted_values_sit_on_the_branch_edges():
    import numpy as np
    m = sw.model_of("explicit")
    e = sw.ulp_set(sw.PHYS, m)
    for v in (sw.PHYS["cutOffbr"], sw.PHYS["maxOffbr"], m["br"]):
        assert v in e and np.nextafter(v, 0.0) in e and np.nextafter(v, 1.0) in e
    assert 1.0e-16 in e and 5.0e-7 in e
    for nx, ny in sw.SHAPES:
        for b, bc in sw.BCS.items():
            st = sw.single_state(nx, ny, b, "explicit")
            planted = np.isin(st["B"], e)
            assert 0.02 < planted[1:-1, 1:-1].mean() < 0.10, (nx, ny, b)                  # a few percent: 4 cells of the 48 of 12 x 4
            if not (bc["periodic"][0] and bc["periodic"][1]):                             # (doubly periodic: the whole ring is an image)
                assert np.concatenate([planted[0, :], planted[-1, :], planted[:, 0], planted[:, -1]]).any(), (nx, ny, b)
            assert 0.03 < (st["mask"][1:-1, 1:-1] < 0).mean() < 0.35, (nx, ny, b)
            # periodic sides: the ghost cells are the periodic image
            for k in ("B", "Pi", "zb", "mask"):
                if bc["periodic"][0]:
                    assert np.array_equal(st[k][:, 0], st[k][:, -2]) and np.array_equal(st[k][:, -1], st[k][:, 1]), (nx, ny, b, k)
                if bc["periodic"][1]:
                    assert np.array_equal(st[k][0, :], st[k][-2, :]) and np.array_equal(st[k][-1, :], st[k][1, :]), (nx, ny, b, k)
            assert sw.single_state(nx, ny, b, "explicit")["B"].tobytes() == st["B"].tobytes()


def test_layouts_kept_and_left_out():
    """hierarchies take a time step where no fine ghost cell across a periodic side is coarse-fine (hierlayouts.cf_ghosts_across_periodic); the
    counts are asserted so that a change to the generator cannot silently empty the sweep"""
    cf = lambda name: hl.cf_ghosts_across_periodic(hl.NX0, hl.NY0, hl.FEATURES[name][0]["periodic"], hl.FEATURES[name][1])
    assert {n: cf(n) for n in hl.FEATURES if cf(n)} == {"x-wrap-self": 12, "xy-wrap-corner": 24, "x-wrap-two-faces": 4}
    kept, out = sw.hierarchy_layouts()
    assert len([c for c in kept if not c[0].startswith("seed-")]) == 9 and len(hl.FEATURES) == 12
    per = lambda cs: sorted(tuple(c[1]["periodic"]) for c in cs if c[0].startswith("seed-"))
    count = lambda cs, p: per(cs).count(p)
    assert [count(kept, p) for p in ((0, 0), (1, 0), (0, 1), (1, 1))] == [10, 3, 1, 0]
    assert [count(kept + out, p) for p in ((0, 0), (1, 0), (0, 1), (1, 1))] == [10, 10, 10, 10]
    for name, bc, boxes, seed in kept:
        assert hl.cf_ghosts_across_periodic(hl.NX0, hl.NY0, bc["periodic"], boxes) == 0 and hl.valid(hl.NX0, hl.NY0, bc["periodic"], boxes), name
    assert set(sw.HIER_DROPPED) <= {c[0] for c in kept} and len(sw.HIER_DROPPED) <= 1
    # what the device comparison runs: at least two layouts of every periodicity the sweep covers
    run = sw.device_layouts()
    assert {c[0] for c in run} >= {c[0] for c in kept if not c[0].startswith("seed-")} and not set(sw.HIER_DROPPED) & {c[0] for c in run}
    for p in ((0, 0), (1, 0), (0, 1)):
        assert sum(tuple(c[1]["periodic"]) == p for c in run) >= 2, p
    assert {1 + len(c[2]) for c in run if c[0].startswith("seed-")} == {2, 3, 4}


def test_nothing_hides_a_failure(sweep):
    assert len(sweep["single"]) == len(sw.single_cases()) and all(len(r["iters"]) == sw.N_STEPS for r in sweep["single"].values())
    assert all(len(r["iters"]) == sw.N_STEPS for r in sweep["hier"].values())
    assert not sweep["problems"], "\n".join(sweep["problems"][:20])


def test_every_arm_is_taken(sweep):
    print("\n" + sw.census_table(sweep))
    missing = []
    for (br, arm), (n, cases, shapes) in sweep["single_arms"].items():
        if (br, arm) in sw.NOT_ON_ONE_LEVEL:
            assert n == 0, (br, arm)
            continue
        if len(cases) < 4 or len(shapes) < 2:
            missing.append((br, arm, n, len(cases), len(shapes)))
    assert not missing, missing
    assert len(sweep["single_arms"]) >= 40
    for key in sw.MIDDLE_LEVEL_ARMS + tuple(sw.NOT_ON_ONE_LEVEL):
        n, layouts = sweep["hier_arms"][key]
        assert n > 0 and len(layouts) >= 1, key


def test_census_table_is_the_committed_one(sweep):
    """tests/golden/STEP_SWEEP_CENSUS.txt is what tools/step_sweep_census.py writes: recorded results, regenerated when the sweep changes"""
    with open(GOLD) as f:
        assert f.read() == sw.census_table(sweep)
