"""The ensemble sweep of tests/batchsweep.py on the CPU oracle alone: the tables hold the shapes, rows and rotation they claim, the oracle's fields are
finite in every batch (a condition of the bitwise comparison on the device: no batch is filtered), every arm of the ensemble's own code the sweep
is after is taken (the census, printed and pinned by tests/golden/BATCH_SWEEP_CENSUS.txt), the members of a solve leave at different cycles, the
spikes put each member's residual maximum into its chosen partial, and the time-step batches take every arm the census of tests/stepsweep.py can
take on one level.  tests/test_gpu_batch_sweep.py compares the device with the oracle on the same batches, bitwise."""
import os

import pytest

from tests import batchsweep as bw
from tests import stepsweep as sw

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "BATCH_SWEEP_CENSUS.txt")


@pytest.fixture(scope="module")
def sweep(oracle):
    """the protocol of every V-cycle / solve batch on the oracle, once for the module"""
    return bw.sweep_census(oracle)


@pytest.fixture(scope="module")
def steps(oracle):
    """two steps of every member of every time-step batch on the oracle, once for the module"""
    return bw.step_census(oracle)


def test_the_tables_hold_what_the_sweep_claims():
    bs = bw.batches()
    assert len(bw.SHAPES) == 16 and len(bw.ROWS) == 8 and len({b[0] for b in bs}) == len(bs)
    # the rotation: every (shape, row) pair and every (BC, row) pair.  16 shapes x 8 rows are 128 pairs, so 128 batches is the least that holds them
    assert len({(b[1], b[3]) for b in bs}) == len(bw.SHAPES) * len(bw.ROWS) - len(bw.DROPPED)
    assert {(b[2], b[3]) for b in bs} == {(b, r) for b in bw.BCS for r in bw.ROWS}
    assert len(bs) + len(bw.DROPPED) == len(bw.SHAPES) * len(bw.ROWS) and 10 * len(bw.DROPPED) <= len(bs) and all(bw.DROPPED.values())
    assert {b[1] for b in bs} == set(bw.SHAPES) and {b[3] for b in bs} == set(bw.ROWS)
    # odd ny skips the y-periodic rows and nothing else does; 4 x 4 is doubly periodic
    for shape in bw.SHAPES:
        mine = bw.bcs_of(shape)
        if shape[:2] == (4, 4):
            assert mine == ("xy-periodic",)
        elif shape[1] & 1:
            assert set(mine) == {"a3", "x-periodic", "dirichlet"}
        else:
            assert set(mine) == set(bw.BCS)
    assert bw.ROWS[0] == (4, 16, -1, 0, 0.0, 0) and (3, 9, -1, 0, 0.6, 1) in bw.ROWS and (0, 3, -1, 0, 0.0, 0) in bw.ROWS
    assert {r[2] for r in bw.ROWS} == {-1, 0, 1} and {r[3] for r in bw.ROWS} == {0, 1} and {r[5] for r in bw.ROWS} == {0, 1, 2}
    assert bw.PALETTES.count("dirty") == 2 and set(bw.PALETTES) == {"dirty", "clean", "one-cell", "plus-minus"} and len(bw.PALETTES) == bw.N_MEMBERS
    # members with 2, 1, 3, 2, 2 cycles before the solve (the num_smooth = 0 row: 2, 1, 2, 1, 2 and a solve of at most 2)
    assert [bw.cycles_of_member(bw.ROWS[0], k) for k in range(5)] == [2, 1, 3, 2, 2] and bw.protocol(bw.ROWS[0])[1] == 6
    assert [bw.cycles_of_member(bw.ROWS[5], k) for k in range(5)] == [2, 1, 2, 1, 2] and bw.protocol(bw.ROWS[5])[1] == 2
    # time-step batches: every (shape, BC) of the step sweep with the six rows at dt = 60, the hot-bed row with two others at dt = 2 on two shapes
    sb = bw.step_batches()
    assert {(b[1], b[2]) for b in sb} == set(sw.SHAPES) and {b[3] for b in sb} == set(sw.BCS)
    assert all(len(b[5]) == 6 and "hot-bed-diffusion" not in b[5] for b in sb if b[4] == 60.0)
    assert {(b[1], b[2]) for b in sb if b[4] == 2.0} == {(12, 4), (72, 20)} and all(b[5] == ("hot-bed-diffusion", "explicit-diffusion", "implicit") for b in sb if b[4] == 2.0)
    for nx, ny in sw.SHAPES:
        have = {b[3] for b in sb if (b[1], b[2]) == (nx, ny) and b[4] == 60.0}
        assert len(have) >= (3 if (nx, ny) in ((72, 20), (24, 36)) else 5), (nx, ny, have)
    assert bw.BATCH_MAX == 64 and len(bw.big_active_lists()) == 4 and sum(bw.big_active_lists()[0]) == 1 and bw.big_active_lists()[0][63] == 1
    assert sum(bw.big_active_lists()[2]) == 32 and bw.big_active_lists()[2][63] == 1 and bw.big_active_lists()[1][0] == 1


def test_the_geometry_restated():
    """suhmo_batch_tile_ok, single_tile_of and the 4 / 2 / 1 decomposition of batch_relax, at the values the issue's depth tables name"""
    assert bw.single_tile_of(16, 16) == 16 and bw.single_tile_of(32, 28) == 32 and bw.single_tile_of(32, 30) == 0 and bw.single_tile_of(20, 12) == 32
    assert not bw.tile_ok(13, 9, (0, 0)) and not bw.tile_ok(70, 51, (0, 1)) and bw.tile_ok(70, 51, (1, 0))
    assert bw.sequence(bw.relax_launches(40, 24, (0, 0), 7)) == "4+2+1" and bw.sequence(bw.relax_launches(40, 24, (0, 0), 3)) == "2+1"
    assert bw.sequence(bw.relax_launches(40, 24, (0, 0), 9)) == "4+4+1" and bw.relax_launches(10, 6, (0, 0), 9) == [(4, 2, 16), (1, 1, 16)]
    assert bw.relax_launches(20, 12, (0, 0), 16) == [(4, 4, 32)] and bw.relax_launches(20, 12, (0, 0), 7) == [(4, 1, 16), (2, 1, 16), (1, 1, 16)]
    assert bw.relax_launches(13, 9, (0, 0), 4) == [("colour", 1, 0)] * 8 and bw.relax_launches(12, 4, (0, 0), 0) == []
    assert [bw.norm_partials(64, ny) for ny in (252, 256, 260)] == [63, 64, 65] and bw.norm_partials(12, 4) == 1
    # a default cycle of 40 x 24 / 8: bcoef, averages, 4 | restrict | 4 | restrict | 4x4 | 4 | 4 + closing fill
    c = bw.cycle_census([(40, 24), (20, 12), (10, 6)], (0, 0), bw.ROWS[0])
    assert c["launches"] == 2 + 1 + 1 + 1 + 1 + 1 + 1 + 2 and c["paths"] == {0: "tile", 1: "tile", 2: "T16 chunked"}
    assert set(c["rhs"].values()) == {"fused"} and set(c["prolong"].values()) == {"fused"}


def test_depth_tables_are_the_oracles(sweep):
    want = {(4, 4): [(4, 4), (2, 2)], (12, 4): [(12, 4), (6, 2)], (16, 16): [(16, 16), (8, 8), (4, 4), (2, 2)], (20, 12): [(20, 12), (10, 6)],
            (32, 28): [(32, 28), (16, 14)], (32, 30): [(32, 30)], (40, 24): [(40, 24), (20, 12), (10, 6)], (72, 20): [(72, 20), (36, 10)],
            (80, 48): [(80, 48), (40, 24), (20, 12), (10, 6)], (48, 48): [(48, 48), (24, 24), (12, 12), (6, 6)], (70, 51): [(70, 51)], (13, 9): [(13, 9)]}
    for bid, shape, b, row in bw.batches():
        rec = sweep["batches"][bid]
        if shape == (40, 24, 4):
            assert rec["depths"] == [(40, 24), (20, 12)], bid
        elif shape[:2] in want:
            assert rec["depths"] == want[shape[:2]], bid
        assert rec["depths"][0] == shape[:2] and rec["np"] == bw.norm_partials(*shape[:2])
    # coarse depths are even in both directions: the separate arms are reachable through sweep counts of 0 alone, colour passes on one depth alone
    for rec in sweep["batches"].values():
        assert all(nx % 2 == 0 and ny % 2 == 0 for nx, ny in rec["depths"][1:])


def test_the_oracle_is_finite_in_every_batch(sweep):
    assert len(sweep["batches"]) == len(bw.batches()) == 128 - len(bw.DROPPED)
    assert not sweep["problems"], "\n".join(sweep["problems"][:20])
    assert all(len(r["counts"]) == bw.N_MEMBERS for r in sweep["batches"].values())


def test_every_arm_is_taken(sweep, steps):
    print("\n" + bw.census_table(sweep, steps))
    for arm in bw.REQUIRED_ARMS:
        assert len(sweep["arms"].get(arm, ())) >= (2 if arm == "path: colour" else 3), (arm, sorted(sweep["arms"].get(arm, ())))
    # the colour passes over members: the odd nx of 13 x 9 alone
    assert all(b.startswith("13x9b16-") for b in sweep["arms"]["path: colour"])
    # dirty palettes through launch_bcoef_fused(OnMembers): every arm of bcoefsweep's census that depends on the mask, in at least 3 batches
    for (br, arm), (n, ids) in sweep["palette"].items():
        if (br, arm) in bw.PALETTE_NOT_TAKEN:
            assert n == 0, (br, arm)
            continue
        assert n > 0 and len(ids) >= 3, (br, arm, n, len(ids))
    assert len(sweep["palette"]) >= 30


def test_members_leave_the_solve_at_different_cycles(sweep):
    uneq = [bid for bid, r in sweep["batches"].items() if len(set(r["counts"])) > 1]
    print("solves whose members' cycle counts differ: %d of %d" % (len(uneq), len(sweep["batches"])))
    assert 3 * len(uneq) >= len(sweep["batches"])


def test_spikes_put_every_maximum_into_its_partial(sweep):
    """the three 64-wide shapes: the residual that enters the solve has its maximum in the partial spike_partial() names, per member"""
    n = 0
    for bid, shape, b, row in bw.batches():
        if shape[:2] in bw.TALL:
            rec = sweep["batches"][bid]
            last = rec["np"] - 1
            want = [bw.spike_partial(shape[1], k) for k in range(bw.N_MEMBERS)]
            assert want == [0, last, last // 2, last - 1, 1] and [p[0] for p in rec["max_partial"]] == want, (bid, rec["max_partial"], want)
            n += 1
    assert n == 24 - sum(1 for d in bw.DROPPED if d.startswith("64x2"))


def test_time_step_batches_take_every_arm(steps):
    assert not steps["problems"], "\n".join(steps["problems"][:20])
    assert steps["runs"] == sum(len(b[5]) for b in bw.step_batches())
    missing = []
    for (br, arm), (n, members, shapes) in steps["arms"].items():
        if (br, arm) in sw.NOT_ON_ONE_LEVEL:
            assert n == 0, (br, arm)
        elif len(members) < 4 or len(shapes) < 2:
            missing.append((br, arm, n, len(members), len(shapes)))
    assert not missing, missing
    assert len(steps["arms"]) >= 40


def test_census_table_is_the_committed_one(sweep, steps):
    """tests/golden/BATCH_SWEEP_CENSUS.txt is what tools/batch_sweep_census.py writes: recorded results, regenerated when the sweep changes"""
    with open(GOLD) as f:
        assert f.read() == bw.census_table(sweep, steps)
