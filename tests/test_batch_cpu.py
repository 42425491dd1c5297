"""The ensemble interface (suhmo_batch_*) as far as a machine without a GPU can check it: the library exports every entry point the
header declares and the ctypes table lists, creation fails loudly where there is no device, and the Python mirror stays clear of the
test oracle."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from suhmo_amd import capi
    capi.build()
    return capi.lib()


def test_batch_symbols_exported(lib):
    from suhmo_amd import capi
    hdr = open(os.path.join(ROOT, "include", "suhmo_hip.h")).read()
    declared = set(re.findall(r"\b(suhmo_batch_[a-z_0-9]+)\s*\(", hdr))
    assert {"suhmo_batch_create", "suhmo_batch_destroy", "suhmo_batch_size", "suhmo_batch_member", "suhmo_batch_set_phys",
            "suhmo_batch_vcycle", "suhmo_batch_solve", "suhmo_batch_timestep", "suhmo_batch_set_option", "suhmo_batch_get_option"} <= declared
    assert declared <= set(capi.SYMBOLS)
    for name in sorted(declared):
        assert hasattr(lib, name), name


def test_batch_create_fails_loudly_without_gpu(lib):
    if lib.suhmo_device_count() > 0:
        pytest.skip("a GPU is present")
    from suhmo_amd import capi, level, synthetic as sy
    d = capi.LevelDesc()
    d.nx, d.ny, d.j0, d.ny_global, d.dx, d.dy = 64, 64, 0, 64, 1.0, 1.0
    d.nbox, d.boxes, d.max_box, d.alpha, d.beta = 0, None, 64, 0.0, -1.0
    d.bc, d.phys, d.device, d.halo_rows = level._bc(sy.A3_BC), level._phys(sy.A3_PHYS), 0, 1
    h = C.c_void_p()
    assert lib.suhmo_batch_create(C.byref(h), C.byref(d), 4) == -3
    assert not h.value
    assert b"no HIP device" in lib.suhmo_last_error()
    with pytest.raises(capi.SuhmoError):
        level.HipBatch(4, 64, 64, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS)


def test_batch_arguments_are_checked_before_the_device(lib):
    """n_members out of range and a descriptor that is not a whole level are refused with their own codes, GPU or not"""
    from suhmo_amd import capi, level, synthetic as sy
    d = capi.LevelDesc()
    d.nx, d.ny, d.j0, d.ny_global, d.dx, d.dy = 64, 32, 0, 32, 1.0, 1.0
    d.nbox, d.boxes, d.max_box, d.alpha, d.beta = 0, None, 64, 0.0, -1.0
    d.bc, d.phys, d.device, d.halo_rows = level._bc(sy.A3_BC), level._phys(sy.A3_PHYS), 0, 1
    h = C.c_void_p()
    assert lib.suhmo_batch_create(C.byref(h), C.byref(d), 0) == -1 and b"n_members" in lib.suhmo_last_error()
    assert lib.suhmo_batch_create(C.byref(h), C.byref(d), 65) == -1
    d.j0, d.ny_global = 32, 64                                   # a rank strip
    assert lib.suhmo_batch_create(C.byref(h), C.byref(d), 2) == -5 and b"whole levels" in lib.suhmo_last_error()
    d.j0, d.ny_global, d.i0, d.nx_global = 0, 32, 8, 256          # an AMR patch
    assert lib.suhmo_batch_create(C.byref(h), C.byref(d), 2) == -5
    assert not h.value


def test_batch_model_imports_nothing_from_oracle():
    """HipBatchModel and what it stands on: the check tests/test_capi_cpu.py makes for the whole package, on the ensemble's files, and
    importing the class loads no oracle module"""
    import subprocess
    import sys
    pat = re.compile(r"import\s+oracle|from\s+oracle|from\s+\.+oracle|liboracle|pyoracle|level_shim|suhmo_oracle")
    for rel in ("suhmo_amd/model.py", "suhmo_amd/level.py", "suhmo_amd/capi.py", "suhmo_amd/csrc/suhmo_batch.hip", "suhmo_amd/csrc/suhmo_batch.h",
                "tools/batch_bench.py"):
        assert not pat.search(open(os.path.join(ROOT, rel)).read()), rel
    code = ("import sys; sys.path.insert(0, %r); from suhmo_amd.model import HipBatchModel; "
            "assert HipBatchModel.timestep and not [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.')]" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])
