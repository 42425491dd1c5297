"""suhmo_batch_run as far as a machine without a GPU can check it: the ctypes layout of the schedule and the result against what the C
compiler lays out (sizeof / offsetof printed by a small host program built from include/suhmo_hip.h), the symbols declared, listed and
exported, the argument check before any device is touched, and HipBatchModel.run failing loudly where there is no GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULE = ("n_steps", "dt", "first_cur_step", "n_members", "T_K", "background", "n_moulins", "positions", "sigma", "flux", "moulin_factor", "ramp",
            "diag_every")
RESULT = ("steps_done", "n_rows", "picard_iters", "vcycles", "rows")


@pytest.fixture(scope="module")
def lib():
    from suhmo_amd import capi
    capi.build()
    return capi.lib()


def test_struct_layout_is_the_c_compilers(tmp_path):
    from suhmo_amd import capi
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler (the oracle is built with one)"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "suhmo_hip.h"', 'int main(void) {',
             '  printf("schedule %zu\\n", sizeof(suhmo_batch_schedule_t));', '  printf("result %zu\\n", sizeof(suhmo_batch_run_result_t));']
    lines += ['  printf("schedule.%s %%zu\\n", offsetof(suhmo_batch_schedule_t, %s));' % (f, f) for f in SCHEDULE]
    lines += ['  printf("result.%s %%zu\\n", offsetof(suhmo_batch_run_result_t, %s));' % (f, f) for f in RESULT]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert [f for f, _ in capi.BatchSchedule._fields_] == list(SCHEDULE) and [f for f, _ in capi.BatchRunResult._fields_] == list(RESULT)
    assert C.sizeof(capi.BatchSchedule) == int(want["schedule"]) and C.sizeof(capi.BatchRunResult) == int(want["result"])
    for f in SCHEDULE:
        assert getattr(capi.BatchSchedule, f).offset == int(want["schedule." + f]), f
    for f in RESULT:
        assert getattr(capi.BatchRunResult, f).offset == int(want["result." + f]), f


def test_run_symbols_declared_listed_and_exported(lib):
    from suhmo_amd import capi
    hdr = open(os.path.join(ROOT, "include", "suhmo_hip.h")).read()
    declared = set(re.findall(r"^int\s+(suhmo_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    for name in ("suhmo_batch_run", "suhmo_level_postproc_temporal_device"):
        assert name in declared and name in capi.SYMBOLS and getattr(lib, name).argtypes, name


def test_missing_arguments_are_refused_without_a_device(lib):
    from suhmo_amd import capi
    mp, sch, res = (capi.ModelParams * 2)(), capi.BatchSchedule(), capi.BatchRunResult()
    fake = C.c_void_p(8)          # never dereferenced: the argument check comes first
    for hole in range(4):
        args = [fake, mp, C.byref(sch), None, C.byref(res), None]
        args[hole if hole < 3 else 4] = None
        assert lib.suhmo_batch_run(*args) == -1 and b"bad argument" in lib.suhmo_last_error(), hole
    out = (C.c_double * 6)()
    assert lib.suhmo_level_postproc_temporal_device(None, mp, out, None) == -1 and b"bad argument" in lib.suhmo_last_error()


def test_run_fails_loudly_without_a_gpu(lib):
    """like every other entry point: no device, no fallback -- the ensemble cannot even be created"""
    from suhmo_amd import capi, model, synthetic as sy
    assert callable(model.HipBatchModel.run) and callable(model.HipModel.postproc_temporal_device)
    if lib.suhmo_device_count() > 0:
        pytest.skip("a GPU is visible: tests/test_gpu_batch_run.py runs the call")
    with pytest.raises(capi.SuhmoError):
        G = model.HipBatchModel(40, 24, 150.0, 62.5, sy.A3_BC, sy.A3_PHYS, [dict(sy.A3_MODEL)] * 2, max_box=8)
        G.run(2, 3600.0, T_K=np.zeros((2, 2)), background=np.zeros((2, 2)))
