"""The oracle's own ghost rings, pinned on the CPU before the device is judged against them: after a call whose last step is a
relaxation (levelGSRB ends with the homogeneous ghost fill, src/VCAMRNonLinearPoissonOp.cpp:757-759) the domain sides of the
head's ring are npref's homogeneous boundary condition of the array's own valid cells, bit for bit, on a single level and on
every box of every level of a hierarchy; a periodic side of a whole level holds the wrapped valid cells."""
import numpy as np
import pytest

from suhmo_amd import synthetic as sy
from tests import ghostring as gr
from tests.test_gpu_hier import BC, BC_NP, BC_V, UNION, WRAP, WRAP_SIDE      # the layouts the device tests judge

SP = dict(sy.SOLVER_DEFAULT, eps=1e-9, norm_thresh=1e-14, max_iter=6, imin=30)

LEVEL_CASES = {"shmip-a3": (lambda: sy.shmip_fields(64, 32), sy.A3_BC, sy.A3_PHYS),
               "random-values": (lambda: sy.random_fields(48, 40), sy.RANDOM_BC, sy.RANDOM_PHYS),
               "periodic-y": (lambda: sy.shmip_fields(64, 32), sy.CONV_BC, sy.A3_PHYS)}


@pytest.mark.parametrize("call", ["gsrb", "vcycle"])
@pytest.mark.parametrize("case", list(LEVEL_CASES))
def test_oracle_level_ring_is_the_homogeneous_bc(oracle, case, call):
    make, bc, ph = LEVEL_CASES[case]
    f = make()
    ny, nx = f["phi"].shape
    O = oracle.OracleLevel(nx, ny, f["dx"], f["dy"], bc, ph, max_box=16, nthreads=2)
    O.set_inputs(f); O.build_mg_coefficients()
    O.gsrb(4) if call == "gsrb" else O.vcycle(dict(sy.SOLVER_DEFAULT))
    a = O.get(oracle.F_PHI, ghosted=True)
    n = gr.domain_bc_holds(a, bc, f["dx"], f["dy"], (0, 0, nx - 1, ny - 1), (nx, ny), (case, call))
    assert n == 2 * (ny * (1 - bc["periodic"][0]) + nx * (1 - bc["periodic"][1])) and n > 0
    if bc["periodic"][1]:                                  # the periodic sides of the ghosted read-back: the other end's valid row
        assert np.array_equal(a[0, 1:-1], a[-2, 1:-1]) and np.array_equal(a[-1, 1:-1], a[1, 1:-1]), (case, call)
    O.close()


@pytest.mark.parametrize("call", ["gsrb", "vcycle"])
@pytest.mark.parametrize("name,boxes,bc", [("union", UNION, BC_NP), ("union-values", UNION, BC_V), ("wrap-periodic", WRAP, BC),
                                            ("wrap-side-self-neighbour", WRAP_SIDE, BC)],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_oracle_amrm_ring_is_the_homogeneous_bc(oracle, name, boxes, bc, call):
    fs = sy.amrm_fields(64, 16, boxes)
    O = oracle.OracleAmrM(64, 16, fs[0]["dx"], fs[0]["dy"], bc, sy.CFG3_PHYS, boxes, max_box=32, nthreads=2)
    O.set_inputs(fs)
    if call == "gsrb":
        for l in range(1, O.nlev):
            O.cf_interp_phi(l); O.gsrb(l, 4)
    else:
        O.vcycle(SP)
    n = 0
    for l in range(1, O.nlev):
        for k, b in enumerate(O.boxes[l - 1]):
            n += gr.domain_bc_holds(O.box_get(l, k, oracle.F_PHI, ghosted=True), bc, fs[l][k]["dx"], fs[l][k]["dy"], b,
                                    (64 << l, 16 << l), (name, call, l, k))
    if call == "vcycle":                                   # the base relaxed last in the upward leg too
        n += gr.domain_bc_holds(O.coarse.get(oracle.F_PHI, ghosted=True), bc, fs[0]["dx"], fs[0]["dy"], (0, 0, 63, 15), (64, 16),
                                (name, call, "base"))
    assert n > 0 or (name == "wrap-periodic" and call == "gsrb")     # (WRAP: no box of a finer level on a non-periodic side)
    O.close()


def test_ring_kinds_of_the_test_layouts():
    """the classification the device tests rely on: every kind occurs where the layouts say it does"""
    kinds = lambda boxes, l, k, per: gr.ring_kinds(boxes[l - 1][k], (64 << l, 16 << l), per, boxes[l - 1])
    u = kinds(UNION, 1, 2, [0, 0])                         # the disjoint box on the x-lo domain side
    assert set(u["x-lo"]) == {"domain"} and set(u["x-hi"]) == {"coarse-fine"}
    u = kinds(UNION, 1, 0, [0, 0])                         # the L: its x-hi side is partly the abutting box
    assert set(u["x-hi"]) == {"fine-fine", "coarse-fine"}
    w = kinds(WRAP, 1, 2, [0, 1])                          # the box that spans the period is its own neighbour
    assert set(w["y-lo"]) == {"periodic"} and set(w["y-hi"]) == {"periodic"}
    w = kinds(WRAP, 1, 0, [0, 1])                          # neighbours through the wrap
    assert set(w["y-lo"]) == {"periodic"} and set(w["y-hi"]) == {"coarse-fine"}
    for l in (1, 2):                                       # WRAP_SIDE: its own periodic neighbour and on the x-lo domain side
        w = kinds(WRAP_SIDE, l, 0, [0, 1])
        assert set(w["x-lo"]) == {"domain"} and set(w["y-lo"]) == set(w["y-hi"]) == {"periodic"}
    a, b = np.zeros((5, 6)), np.zeros((5, 6))
    b[2, -1] = 1.0                                         # a differing cell on the x-hi side: named with its side, kind and index
    with pytest.raises(AssertionError, match=r"side x-hi \(domain\), first at cell \(i, j\) = \(4, 1\)"):
        gr.ring_equal(a, b, (0, 0, 3, 2), (4, 3), (0, 0), what="t")
    assert gr.ring_equal(a, b, (0, 0, 3, 2), (4, 3), (0, 0), kinds=("periodic",)) == {"periodic": 0}
