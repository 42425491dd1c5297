"""bench.py's options and its output dump without a GPU: the --full figures are refused in a plain run, and --dump-outputs writes a
level larger than its budget as the same seeded sample of cells on every call."""
import os
import subprocess
import sys

import numpy as np

import bench
from suhmo_amd import level

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweeps_only_needs_full():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sweeps-only", "4"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert p.returncode == 2 and b"--full" in p.stderr


class _Head:
    """stands in for a HipLevel: get(F_PHI) returns a fixed head"""
    def __init__(self, phi):
        self.phi = phi

    def get(self, field):
        assert field == level.F_PHI
        return self.phi.copy()


def test_dump_outputs_sample(tmp_path, monkeypatch):
    phi = np.random.default_rng(1).uniform(size=(96, 80))
    bench.dump_outputs(str(tmp_path / "whole"), _Head(phi), level, 0, 1)
    assert np.array_equal(np.load(str(tmp_path / "whole" / "phi.npy")), phi)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), _Head(phi), level, 0, 1)
    s1, s2 = (np.load(str(tmp_path / d / "phi.npy")) for d in ("s1", "s2"))
    assert s1.dtype == np.float64 and s1.shape == (1000,)
    assert np.array_equal(s1, s2)
    assert np.all(np.isin(s1, phi))
    bench.dump_outputs(str(tmp_path / "ranks"), _Head(phi), level, 1, 2)       # two ranks share the budget, one file each
    assert np.load(str(tmp_path / "ranks" / "phi_rank1.npy")).shape == (500,)
