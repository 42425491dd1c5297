"""bench.py on one GPU: a plain run prints the headline line and nothing it has to measure besides, --steps sets the timed V-cycles, and
--dump-outputs writes the head the last timed V-cycle left -- the same on every run with the same arguments, the same in a --full run,
and bit for bit the oracle's after as many V-cycles from the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from suhmo_amd import synthetic as sy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, WARMUP, STEPS = 256, 1, 3


def run_bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cells", str(N), "--steps", str(STEPS),
                        "--warmup", str(WARMUP)] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("{")][-1])


def test_plain_line_and_dumped_head(oracle, tmp_path):
    a = run_bench("--dump-outputs", str(tmp_path / "a"))
    assert a["unit"] == "V-cycles/s" and a["higher_is_better"] is True and a["dtype"] == "f64" and a["metric"]
    assert a["steps"] == STEPS and a["warmup"] == WARMUP and a["ms_per_step"] > 0
    assert abs(a["value"] * a["ms_per_step"] - 1e3) < 1e-6                  # one step = one V-cycle on one GPU
    for k in ("roofline", "residual_max_norm", "cpu_baseline", "parity_at_bench_size", "other_configs", "converged_solve"):
        assert k not in a, k
    b = run_bench("--dump-outputs", str(tmp_path / "b"))
    c = run_bench("--full", "--no-cpu", "--no-side", "--dump-outputs", str(tmp_path / "c"))
    assert c["roofline"]["launches_timed"] > 0
    assert c["residual_max_norm"]["after_timed_cycles"] < c["residual_max_norm"]["before_warmup"]
    ha, hb, hc = (np.load(str(tmp_path / d / "phi.npy")) for d in "abc")
    assert ha.dtype == np.float64 and ha.shape == (N, N)
    assert np.array_equal(ha, hb) and np.array_equal(ha, hc)
    # the timed path's head against the oracle's after warm-up + timed V-cycles from bench.py's inputs
    f = sy.shmip_fields(N, N, ly=1.0e5)
    O = oracle.OracleLevel(N, N, f["dx"], f["dy"], sy.A3_BC, sy.A3_PHYS, max_box=64, nthreads=min(16, os.cpu_count() or 1))
    O.set_inputs(f)
    O.build_mg_coefficients()
    sp = dict(sy.SOLVER_DEFAULT)
    for _ in range(WARMUP + STEPS):
        O.vcycle(sp)
    ref = O.get(oracle.F_PHI)
    O.close()
    assert np.array_equal(ha, ref), float(np.max(np.abs(ha - ref)))
