"""The water budget ("WATER BUDGET", include/suhmo_hip.h) as far as a machine without a GPU can check it: the ctypes layout of suhmo_run_budget_t
against the C compiler's, the symbols declared, listed and exported, the argument refusals that come before any device is touched, the loud
failure without a device, and the numpy twin tests/budget_ref.py on the inputs of the mass-balance sweep -- its volume-only reduction is its
VOLUME on the same data, its recharge sums are a plain math.fsum of the cells it should count, to 1e-12 relative (the GPU tests are bitwise
against the twin: this only checks that the twin sums the right cells)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import budget_ref as br
from tests import massbalance_ref as mb
from tests import reduce_ref as rr
from tests.test_massbalance_cpu import SWEEP, level_inputs, same_bits, whole

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = ("every", "lev_cap", "rows", "nlev", "n_rows")
WB_SYMBOLS = ("suhmo_level_water_budget", "suhmo_hier_water_budget", "suhmo_batch_water_budget", "suhmo_hier_run_bud", "suhmo_batch_run_bud")
MP = dict(use_moulin_source=0, ramp=1.0, distributed_input=2.0 ** -7, rho_w=1000.0)
MP_SRC = dict(use_moulin_source=1, ramp=0.625, distributed_input=2.0 ** -7, rho_w=1000.0)


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
             '  printf("budget %zu\\n", sizeof(suhmo_run_budget_t));', '  printf("count %d\\n", (int)SUHMO_WB_COUNT);',
             '  printf("old %d\\n", (int)SUHMO_WB_VOLUME_OLD);', '  printf("mb %d\\n", (int)SUHMO_MB_COUNT);']
    lines += ['  printf("budget.%s %%zu\\n", offsetof(suhmo_run_budget_t, %s));' % (f, f) for f in BUDGET]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert [f for f, _ in capi.RunBudget._fields_] == list(BUDGET)
    assert C.sizeof(capi.RunBudget) == int(want["budget"])
    for f in BUDGET:
        assert getattr(capi.RunBudget, f).offset == int(want["budget." + f]), f
    assert int(want["count"]) == len(capi.WB_NAMES) == len(br.NAMES) == 10 and int(want["mb"]) == 7, "SUHMO_MB_COUNT stays"
    assert int(want["old"]) == br.VOLUME_OLD == capi.WB_NAMES.index("volume_old")


def test_the_calls_are_declared_listed_and_exported(lib):
    from suhmo_amd import capi, model
    hdr = open(os.path.join(ROOT, "include", "suhmo_hip.h")).read()
    declared = set(re.findall(r"^int\s+(suhmo_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    raw = C.CDLL(capi.LIB_PATH)
    for name in WB_SYMBOLS:
        assert name in declared and name in capi.SYMBOLS and hasattr(raw, name) and getattr(lib, name).argtypes, name
    assert "WATER BUDGET" in hdr and "SUHMO_WB_COUNT" in hdr and "track_old_volume" in hdr
    assert capi.WB_NAMES == br.NAMES and capi.WB_NAMES[:7] == capi.MB_NAMES
    assert all(callable(f) for f in (model.HipModel.water_budget, model.HipHierModel.water_budget, model.HipBatchModel.water_budget_all))


def test_missing_arguments_are_refused_without_a_device(lib):
    """the argument check comes before the handle is read: the fake handle is never dereferenced"""
    from suhmo_amd import capi
    fake, out = C.c_void_p(8), (C.c_double * 80)(*([-77.0] * 80))
    mp, mps = capi.ModelParams(), (capi.ModelParams * 2)()
    bad = lambda rc: rc == -1 and b"bad argument" in lib.suhmo_last_error()
    for fn in (lib.suhmo_level_water_budget, lib.suhmo_hier_water_budget):
        assert bad(fn(None, C.byref(mp), out, None)) and bad(fn(fake, None, out, None)) and bad(fn(fake, C.byref(mp), None, None)), fn
    fn = lib.suhmo_batch_water_budget
    assert bad(fn(None, mps, out, None, None)) and bad(fn(fake, None, out, None, None)) and bad(fn(fake, mps, None, None, None))
    assert all(v == -77.0 for v in out)
    # the runs with a budget: the same four holes as the runs without
    bud = capi.RunBudget(every=1, lev_cap=8, rows=out, nlev=(C.c_int * 8)())
    hp, hnull = C.c_void_p(8), C.c_void_p(None)
    hs, hr = capi.HierSchedule(), capi.HierRunResult()
    for hole in range(5):
        args = [C.byref(hp), C.byref(mp), C.byref(hs), None, C.byref(bud), C.byref(hr), None]
        if hole == 4:
            args[0] = C.byref(hnull)
        else:
            args[(0, 1, 2, 5)[hole]] = None
        assert bad(lib.suhmo_hier_run_bud(*args)), hole
    bs, brr = capi.BatchSchedule(), capi.BatchRunResult()
    for hole in range(4):
        args = [fake, mps, C.byref(bs), None, C.byref(bud), C.byref(brr), None]
        args[(0, 1, 2, 5)[hole]] = None
        assert bad(lib.suhmo_batch_run_bud(*args)), hole
    assert bud.n_rows == 0 and all(v == -77.0 for v in out)


def test_the_calls_fail_loudly_without_a_device(lib):
    from suhmo_amd import capi, model, synthetic as sy
    if lib.suhmo_device_count() > 0:
        return                                               # a GPU is visible: tests/test_gpu_budget.py runs the calls
    with pytest.raises(capi.SuhmoError):
        model.HipModel(64, 4, 1.0, 1.0, sy.A3_BC, sy.A3_PHYS, sy.A3_MODEL).water_budget()
    with pytest.raises(capi.SuhmoError):
        G = model.HipBatchModel(40, 24, 150.0, 62.5, sy.A3_BC, sy.A3_PHYS, [dict(sy.A3_MODEL)] * 2, max_box=8)
        G.run(2, 3600.0, balance_every=1)


# ------------------------------------------------------------------ the twin
def with_recharge(data, bl, dom, seed):
    mr, ms = br.synthetic_recharge(dom[0], dom[1], seed)
    return [dict(d, mr=br.cut_valid(mr, b), msrc=br.cut_valid(ms, b)) for d, b in zip(data, bl)]


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_the_twins_old_volume_is_its_volume_and_its_first_seven_are_the_mass_balance(case):
    name, nx0, ny0, bc, boxes, masks = case
    for l, (bl, dom, dx, dy, data) in enumerate(level_inputs(nx0, ny0, bc, boxes, masks)):
        cap = rr.CAP_LEVEL if l == 0 else rr.CAP_BOX
        data = with_recharge(data, bl, dom, 11 + l)
        seven = mb.balance_of_level(data, bl, dom, bc, dx, dy, cap)
        old = br.volume_of_level(data, bl, dom, bc, dx, dy, cap)
        assert same_bits(old, seven[mb.VOLUME]) and old > 0.0, (name, l, old, seven)
        ten = br.budget_of_level(data, bl, dom, bc, dx, dy, MP, cap, volume_old=old)
        assert same_bits(ten[:7], seven) and same_bits(ten[br.VOLUME_OLD], old), (name, l, ten, seven)
        assert np.isnan(br.budget_of_level(data, bl, dom, bc, dx, dy, MP, cap)[br.VOLUME_OLD])
        assert br.default_cap(bl, dom) == cap


@pytest.mark.parametrize("mp", [MP, MP_SRC], ids=["distributed", "moulin-source"])
@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_the_twins_recharge_sums_are_the_plain_sums_of_the_ice_cells(case, mp):
    name, nx0, ny0, bc, boxes, masks = case
    for l, (bl, dom, dx, dy, data) in enumerate(level_inputs(nx0, ny0, bc, boxes, masks)):
        cap = rr.CAP_LEVEL if l == 0 else rr.CAP_BOX
        data = with_recharge(data, bl, dom, 11 + l)
        got = br.budget_of_level(data, bl, dom, bc, dx, dy, mp, cap)
        ext, melt, n = [], [], 0
        for d in data:                                        # a serial walk that owes the twin nothing: cell by cell, in Python
            m = d["mask"][1:-1, 1:-1]
            for j in range(m.shape[0]):
                for i in range(m.shape[1]):
                    if m[j, i] > 0.0:
                        src = d["msrc"][j, i] * mp["ramp"] + mp["distributed_input"] if mp["use_moulin_source"] else mp["distributed_input"]
                        ext.append(src * dy * dx); melt.append(d["mr"][j, i] / mp["rho_w"] * dy * dx); n += 1
        e, m = math.fsum(ext), math.fsum(melt)
        assert n > 0 and e > 0.0 and m > 0.0
        assert abs(got[br.RECH_EXT] - e) <= 1e-12 * e and abs(got[br.RECH_MELT] - m) <= 1e-12 * m, (name, l, got, e, m)


def test_recharge_typed_out_by_hand():
    """8 x 4 cells, dx = 0.5, dy = 0.25, ice in the 8 cells i = 2 .. 5, j = 1 .. 2 (test_massbalance_cpu.rectangle_case): cell area 0.125.
    distributed input 0.5 on ice: ext = 8 * 0.5 * 0.125 = 0.5; MR = 16, rho_w = 4: melt = 8 * 4 * 0.125 = 4.  With a source of 3 everywhere and
    ramp 0.5: src = 3 * 0.5 + 0.5 = 2 on the ice cells (the cells without ice do not count whatever their source): ext = 8 * 2 * 0.125 = 2"""
    from tests.test_massbalance_cpu import NEU0, rectangle_case
    d = dict(rectangle_case(), mr=np.full((4, 8), 16.0), msrc=np.full((4, 8), 3.0))
    mp = dict(use_moulin_source=0, ramp=0.5, distributed_input=0.5, rho_w=4.0)
    out = br.budget_of_level([d], whole(8, 4), (8, 4), NEU0, 0.5, 0.25, mp)
    assert same_bits(out[:7], [0.0, 0.0, 0.0, 0.0, 9.0, 64.0, 0.25]) and np.isnan(out[7]) and same_bits(out[8:], [0.5, 4.0]), out
    out = br.budget_of_level([d], whole(8, 4), (8, 4), NEU0, 0.5, 0.25, dict(mp, use_moulin_source=1), volume_old=0.25)
    assert same_bits(out[7:], [0.25, 2.0, 4.0]), out
