"""What can be said about a run's output without a device: the numpy twin of the snapshot's layout (tests/snapshot_ref.py) against a case typed
out by hand, model.output_steps against the reference's rule (src/AmrHydro.cpp:1311, :1327, :1343-1358), and the symbols of include/suhmo_plt.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import snapshot_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_twin_against_a_hand_written_case():
    """one level of two boxes, 2 x 1 and 1 x 2 cells; component 0 a cell field, component 1 the x-face field averaged to cells.
    Ghosted cell arrays are numbered 10 j + i over the grown box; the face arrays are typed out."""
    boxes = [[(0, 0, 1, 0), (4, 2, 4, 3)]]
    cell = {0: np.array([[0., 1, 2, 3], [10, 11, 12, 13], [20, 21, 22, 23]]), 1: np.array([[0., 1, 2], [10, 11, 12], [20, 21, 22], [30, 31, 32]])}
    face = {0: np.array([[1., 3, 7]]), 1: np.array([[2., 4], [6, 16]])}
    get = lambda l, k, field: cell[k] if field == 3 else face[k]
    comps = [(sr.FIELD, 3, 0.0), (sr.FACE_TO_CELL, 21, 0.0)]
    lo, bo, flat = sr.pack(boxes, get, comps, 1)
    want = [0, 1, 2, 3, 10, 11, 12, 13, 20, 21, 22, 23,                 # box 0, component 0: 3 rows of 4
            0, 0, 0, 0, 0, 2, 5, 0, 0, 0, 0, 0,                         # box 0, component 1: (1 + 3) / 2, (3 + 7) / 2 inside a ring of zeros
            0, 1, 2, 10, 11, 12, 20, 21, 22, 30, 31, 32,                # box 1, component 0: 4 rows of 3
            0, 0, 0, 0, 3, 0, 0, 11, 0, 0, 0, 0]                        # box 1, component 1: (2 + 4) / 2, (6 + 16) / 2
    assert flat.tolist() == want
    assert lo.tolist() == [0, 48] and [b.tolist() for b in bo] == [[0, 24, 48]]
    lo, bo, flat = sr.pack(boxes, get, comps, 0)
    assert flat.tolist() == [11, 12, 2, 5, 11, 21, 3, 11]
    assert lo.tolist() == [0, 8] and [b.tolist() for b in bo] == [[0, 4, 8]]
    # a constant, a field nobody holds, a y-face field, two levels
    yface = np.array([[1., 2], [3, 6]])
    lo, bo, flat = sr.pack([[(0, 0, 1, 0)], [(0, 0, 1, 0)]], lambda l, k, f: None if f == 9 else yface, [(sr.CONST, 0, 3.5), (sr.FIELD, 9, 0.0), (sr.FACE_TO_CELL, 22, 0.0)], 0)
    assert flat.tolist() == [3.5, 3.5, 0, 0, 2, 4] * 2 and lo.tolist() == [0, 6, 12] and [b.tolist() for b in bo] == [[0, 6], [0, 6]]


def test_output_steps_against_hand_cases():
    from suhmo_amd.model import output_steps, PLOT as P, CHECKPOINT as K
    b, a, f = "before_regrid", "after_regrid", "final"
    # :1311 with b = 0 included; :1327 skips b = restart_step = 0; both after the last step
    assert output_steps(1, 7, 3, 3) == [(P, 0, b), (P, 3, b), (K, 3, a), (P, 6, b), (K, 6, a), (P, 7, f), (K, 7, f)]
    assert output_steps(1, 7, 2, 3) == [(P, 0, b), (P, 2, b), (K, 3, a), (P, 4, b), (P, 6, b), (K, 6, a), (P, 7, f), (K, 7, f)]
    # -1: none of that kind; 0: only the file after the last step
    assert output_steps(1, 4, -1, -1) == []
    assert output_steps(1, 4, 0, -1) == [(P, 4, f)]
    assert output_steps(1, 4, -1, 0) == [(K, 4, f)]
    assert output_steps(1, 4, 0, 0) == [(P, 4, f), (K, 4, f)]
    # a checkpoint whose step is the last one is written in the loop never (b < last c) and once after it
    assert output_steps(1, 4, -1, 4) == [(K, 4, f)]
    assert output_steps(1, 5, -1, 4) == [(K, 4, a), (K, 5, f)]
    # a restarted run does not rewrite the checkpoint it started from, but plots its first state
    assert output_steps(5, 2, 4, 4, restart_step=4) == [(P, 4, b), (P, 6, f), (K, 6, f)]
    assert output_steps(5, 2, 4, 4, restart_step=0) == [(P, 4, b), (K, 4, a), (P, 6, f), (K, 6, f)]
    # a run split in two with final=False on the first part gives the events of one run, minus none, plus none
    for split in (1, 3, 4, 6):
        assert output_steps(1, split, 3, 2, final=False) + output_steps(1 + split, 7 - split, 3, 2) == output_steps(1, 7, 3, 2), split
    # plot, regrid and checkpoint at the same b: the plot comes first (old boxes), the checkpoint after the regrid (new boxes)
    ev = output_steps(1, 4, 3, 3, final=False)
    assert ev == [(P, 0, b), (P, 3, b), (K, 3, a)]
    assert output_steps(1, 0, 1, 1) == []


def test_plot_header_symbols_are_exported():
    from suhmo_amd import checkpoint, plotfile
    hdr = open(os.path.join(ROOT, "include", "suhmo_plt.h")).read()
    declared = sorted(set(re.findall(r"\b(suhmo_plt_[a-z_]+)\s*\(", hdr)))
    assert declared == sorted(plotfile.SYMBOLS)
    if checkpoint.hdf5_prefix() is None and not os.path.exists(checkpoint.LIB_PATH):
        pytest.skip("no HDF5 C library on this box: the (optional) checkpoint / plot file library cannot be built")
    plotfile.build()
    L = C.CDLL(plotfile.LIB_PATH)
    for s in declared:
        assert hasattr(L, s), s
    names = (C.c_char_p * 13).in_dll(L, "suhmo_plt_component_names")
    assert [n.decode() for n in names] == plotfile.NAMES
