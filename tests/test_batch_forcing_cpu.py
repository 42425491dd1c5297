"""Forcing and diagnostics of an ensemble in one launch (suhmo_batch_time_varying_recharge, suhmo_batch_moulin_source, suhmo_batch_postproc_*)
as far as a machine without a GPU can check them: declared in the header, listed in the ctypes table, exported by the library, and a call
without its required arguments returns -1 before any device is touched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("suhmo_batch_time_varying_recharge", "suhmo_batch_moulin_source", "suhmo_batch_postproc_partial", "suhmo_batch_postproc_temporal",
       "suhmo_batch_postproc_table")


@pytest.fixture(scope="module")
def lib():
    from suhmo_amd import capi
    capi.build()
    return capi.lib()


def test_forcing_symbols_declared_listed_and_exported(lib):
    from suhmo_amd import capi
    hdr = open(os.path.join(ROOT, "include", "suhmo_hip.h")).read()
    declared = set(re.findall(r"^int\s+(suhmo_batch_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert getattr(lib, name).argtypes, name
    # the sentence that sent callers to the member handle names both ways now
    assert "suhmo_level_time_varying_recharge on the" in hdr and "or the calls below for all members at once" in hdr


def test_missing_arguments_are_refused_without_a_device(lib):
    n = 3
    d, i = (C.c_double * n)(), (C.c_int * n)(1, 1, 1)
    from suhmo_amd import capi
    mp = (capi.ModelParams * n)()
    fake = C.c_void_p(8)          # never dereferenced: the argument check comes first
    assert lib.suhmo_batch_time_varying_recharge(None, d, d, None, None) == -1 and b"bad argument" in lib.suhmo_last_error()
    assert lib.suhmo_batch_time_varying_recharge(fake, None, d, None, None) == -1
    assert lib.suhmo_batch_time_varying_recharge(fake, d, None, None, None) == -1
    assert lib.suhmo_batch_moulin_source(None, i, d, d, d, d, None, None, None) == -1 and b"bad argument" in lib.suhmo_last_error()
    for hole in range(1, 6):
        args = [fake, i, d, d, d, d]
        args[hole] = None
        assert lib.suhmo_batch_moulin_source(*args, None, None, None) == -1, hole
    for fn in (lib.suhmo_batch_postproc_partial, lib.suhmo_batch_postproc_temporal, lib.suhmo_batch_postproc_table):
        assert fn(None, mp, d, None, None) == -1 and b"bad argument" in lib.suhmo_last_error()
        assert fn(fake, None, d, None, None) == -1
        assert fn(fake, mp, None, None, None) == -1


def test_batch_model_has_the_ensemble_methods():
    from suhmo_amd.model import HipBatchModel
    for name in ("set_surface", "time_varying_recharge", "moulin_source", "postproc_partial_all", "postproc_temporal_all", "postproc_table_device_all"):
        assert callable(getattr(HipBatchModel, name)), name
