"""The C++ host mirror of the reference's operator interface (suhmo_amd/host) driven like
Chombo's multigrid drives VCAMRNonLinearPoissonOp, checked bitwise against the oracle."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host_cpp", "test_mirror")


def build_exe():
    from suhmo_amd import capi
    capi.build()
    csrc = os.path.join(ROOT, "suhmo_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "host_cpp", "test_mirror.cpp"),
            os.path.join(ROOT, "suhmo_amd", "host", "VCAMRNonLinearPoissonOpHIP.cpp")]
    objs = []
    for c in ("suhmo_oracle.c", "level_shim.c", "amrm.c"):
        o = os.path.join(ROOT, "tests", "host_cpp", c.replace(".c", ".o"))
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fopenmp", "-c", os.path.join(ROOT, "oracle", c), "-o", o])
        objs.append(o)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + srcs + objs +
                          ["-L" + csrc, "-lsuhmo_hip", "-Wl,-rpath," + csrc, "-fopenmp", "-lm", "-o", EXE])


def test_host_mirror_compiles_cpu():
    """the mirror is plain C++ over the C-ABI: it must build without a GPU"""
    build_exe()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_host_mirror_matches_oracle():
    build_exe()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0 and "RESULT: PASS" in out, out


EXE_B2 = os.path.join(ROOT, "tests", "host_cpp", "test_b2")


def build_b2():
    from suhmo_amd import capi
    capi.build()
    csrc = os.path.join(ROOT, "suhmo_amd", "csrc")
    o = os.path.join(ROOT, "tests", "host_cpp", "suhmo_oracle.o")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-c", os.path.join(ROOT, "oracle", "suhmo_oracle.c"), "-o", o])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "host_cpp", "test_b2.cpp"), o,
                           "-L" + csrc, "-lsuhmo_hip", "-Wl,-rpath," + csrc, "-lm", "-o", EXE_B2])


def b2_names():
    """the per-box symbols of include/suhmo_chf.h"""
    hdr = open(os.path.join(ROOT, "include", "suhmo_chf.h")).read()
    return set(re.findall(r"^void ([a-z_0-9]+_)\(", hdr, flags=re.M))


def test_b2_symbols_exported_cpu():
    """every per-box Fortran-ABI symbol of include/suhmo_chf.h is exported (link check, no GPU)"""
    build_b2()
    names = b2_names()
    assert len(names) == 23, names          # 18 on the solve path + 5 of the time step (src/AmrHydroF.ChF)
    out = subprocess.check_output(["nm", "-D", os.path.join(ROOT, "suhmo_amd", "csrc", "libsuhmo_hip.so")]).decode()
    for n in names:
        assert re.search(r" T %s$" % n, out, flags=re.M), n


# what the driver's table has to cover (tests/host_cpp/test_b2.cpp prints one line per check: symbol, direction, ncomp, geometry)
B2_DIRECTIONAL = ("sumfacesnl_", "newgetfluxnl_", "divergence_", "newmacgrad_", "computebcoeff_", "computeqw_", "computescaprod_",
                  "computedcoeff_", "simpleextrapbc_", "simplecopybc_", "nullbc_")
B2_BC_FILLS = ("simpleextrapbc_", "simplecopybc_", "nullbc_")
B2_NCOMP_GENERAL = ("gsrbhelmholtzvcnl2d_", "vcnlcomputeop2d_", "vcnlcomputeres2d_", "restrictvcnl_", "restrictnl_", "restrictresvcnl2d_",
                    "sumfacesnl_", "prolongnl_", "prolong_2_nl_", "newgetfluxnl_", "simpleextrapbc_", "simplecopybc_", "nullbc_", "divergence_")
B2_GEOMETRIES = ("1x1@", "1x7@", "7x1@", "64x4@", "65x5@", "130x9@", "300x200@")


def b2_checks(out, prefix):
    """(labels of the check lines that start with prefix, the check count of the RESULT line)"""
    labels = [ln[len(prefix):].strip() for ln in out.splitlines() if ln.startswith(prefix)]
    m = re.search(r"^RESULT: PASS \((\d+) checks\)$", out, flags=re.M)
    assert m, out[-2000:]
    return labels, int(m.group(1))


def b2_table_covers(labels):
    """every symbol, every direction, ncomp = 2, every geometry: a symbol the table leaves out is a failure"""
    def has(name, *words):
        return any(ln.split()[0] == name and all(" %s " % w in ln + " " for w in words) for ln in labels)
    names = b2_names()
    assert len(names) == 23
    for n in sorted(names):
        assert has(n), "no check of %s" % n
        for geo in B2_GEOMETRIES:
            assert any(ln.split()[0] == n and geo in ln for ln in labels), "%s never runs on a %s region" % (n, geo)
    for n in B2_DIRECTIONAL:
        for d in (0, 1):
            assert has(n, "dir=%d" % d), "%s never runs with dir = %d" % (n, d)
    for n in B2_BC_FILLS:
        for d in (0, 1):
            for side in ("lo", "hi"):
                assert has(n, "dir=%d" % d, "side=%s" % side, "nc=2"), "%s never fills side (%d, %s) with ncomp = 2" % (n, d, side)
    for n in B2_NCOMP_GENERAL:
        assert has(n, "nc=1") and has(n, "nc=2"), "%s never runs with ncomp = 1 and 2" % n
    for n in ("restrictvcnl_", "restrictnl_", "restrictresvcnl2d_", "prolongnl_", "prolong_2_nl_"):
        for reg in ("full", "even", "odd"):
            assert has(n, "reg=%s" % reg), "%s never runs on the %s sub-region" % (n, reg)
    for hm in (0, 1):
        for d in (0, 1):
            assert has("newmacgrad_", "dir=%d" % d, "hasMask=%d" % hm)
    assert any("handler called once (ncomp)" in ln for ln in labels) and any("handler called once (dir != edgeDir)" in ln for ln in labels)
    assert sum("empty region" in ln or "empty bcbox" in ln for ln in labels) >= 4


EXE_B2_SAN = os.path.join(ROOT, "tests", "host_cpp", "test_b2_oracle_san")


def test_b2_table_stays_inside_its_fabs_cpu():
    """the driver's own table, oracle side only (--oracle-only: no call into the library, no GPU), built with the host's address and
    undefined-behaviour sanitizers: no geometry of the sweep indexes outside a fab -- an out-of-range access in the GPU run would be the
    library's -- and the table covers every symbol, direction, ncomp and geometry with the count it reports"""
    from suhmo_amd import capi
    capi.build()
    csrc = os.path.join(ROOT, "suhmo_amd", "csrc")
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    o = os.path.join(ROOT, "tests", "host_cpp", "suhmo_oracle_san.o")
    subprocess.check_call(["gcc", "-std=c99"] + san + ["-c", os.path.join(ROOT, "oracle", "suhmo_oracle.c"), "-o", o])
    # (the sanitizer runtimes linked statically: they then do not depend on their place in the list of loaded libraries)
    subprocess.check_call(["g++", "-std=c++17"] + san + ["-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "host_cpp", "test_b2.cpp"),
                           o, "-L" + csrc, "-lsuhmo_hip", "-Wl,-rpath," + csrc, "-lm", "-o", EXE_B2_SAN])
    p = subprocess.run([EXE_B2_SAN, "--oracle-only"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    for word in ("Sanitizer", "runtime error", "FAIL:", "ok:"):          # (no report; and no line that claims a comparison was made)
        assert word not in out, out[-4000:]
    labels, n = b2_checks(out, "ref:")
    assert n == len(labels) and len(set(labels)) == n, (n, len(labels), len(set(labels)))
    b2_table_covers(labels)


@pytest.mark.gpu
def test_b2_per_box_kernels_match_oracle():
    build_b2()
    p = subprocess.run([EXE_B2], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0 and "RESULT: PASS" in out, out
    assert "FAIL:" not in out and "MAYDAYERROR" not in out, out
    labels, n = b2_checks(out, "ok:")
    assert n == len(labels), (n, len(labels))                            # the driver's count = the lines it printed
    b2_table_covers(labels)
    ref = subprocess.run([EXE_B2, "--oracle-only"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300).stdout.decode()
    assert b2_checks(ref, "ref:") == (labels, n)                         # ... = the table the sanitized host run went through
