"""The OH chemistry (module_oh_chem, src/mptrac.c:5351-5434) in the host layer and the C library's log10 it needs:
SPECIES presets of OH_CHEM_REACTION / OH_CHEM (mptrac.c:7291-7383) and their overrides as trac prints them, the
refusals, the quantity mloss_oh; mphip_libm_log10 against the running libm on the CPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libm_args
import refchem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mptrac_amd", "csrc")


@pytest.fixture(scope="module")
def trac():
    from mptrac_amd import build
    return build.build_host()[1]


def _run(trac, tmp, keys):
    import hostfiles as hf
    open(os.path.join(tmp, "dirlist"), "w").write(tmp + "\n")
    open(os.path.join(tmp, "atm.tab"), "w").write("0 10 0 0 1\n")
    hf.write_ctl(os.path.join(tmp, "trac.ctl"), dict({"MET_TYPE": 1, "METBASE": os.path.join(tmp, "nothing")}, **keys))
    r = subprocess.run([trac, os.path.join(tmp, "dirlist"), "trac.ctl", "atm.tab"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    return r.returncode, r.stdout.decode()


def _printed(out, key):
    for line in out.splitlines():
        if line.startswith(key + " = "):
            return float(line.split("=")[1])
    raise AssertionError(f"{key} not printed")


@pytest.mark.parametrize("species", sorted(refchem.PRESETS))
def test_species_presets_and_overrides(trac, tmp_path, species):
    reaction, c = refchem.PRESETS[species]
    rc, out = _run(trac, str(tmp_path), {"NQ": 1, "QNT_NAME[0]": "m", "SPECIES": species,
                                         "CLIM_OH_FILENAME": os.path.join(str(tmp_path), "no_oh.nc")})
    assert _printed(out, "OH_CHEM_REACTION") == reaction
    for k in range(4):
        assert _printed(out, f"OH_CHEM[{k}]") == pytest.approx(c[k], rel=1e-5, abs=0)
    # switched on, but the table is missing: the run stops naming the chemistry and the file
    assert rc != 0 and "OH chemistry" in out and "no_oh.nc" in out
    rc, out = _run(trac, str(tmp_path), {"NQ": 1, "QNT_NAME[0]": "m", "SPECIES": species, "OH_CHEM_REACTION": 1,
                                         "OH_CHEM[0]": 4.5e-13, "OH_CHEM[3]": 0.7})
    assert _printed(out, "OH_CHEM_REACTION") == 1 and _printed(out, "OH_CHEM[0]") == 4.5e-13
    assert _printed(out, "OH_CHEM[3]") == 0.7 and _printed(out, "OH_CHEM[1]") == pytest.approx(c[1], rel=1e-5, abs=0)
    rc, out = _run(trac, str(tmp_path), {"NQ": 1, "QNT_NAME[0]": "m", "SPECIES": species, "OH_CHEM_REACTION": 0})
    assert "OH chemistry" not in out


def test_refusals(trac, tmp_path):
    tmp = str(tmp_path)
    for r in (-1, 4):
        rc, out = _run(trac, tmp, {"NQ": 1, "QNT_NAME[0]": "m", "OH_CHEM_REACTION": r})
        assert rc != 0 and "Set OH_CHEM_REACTION to 0, 1, 2, or 3!" in out
    rc, out = _run(trac, tmp, {"NQ": 1, "QNT_NAME[0]": "loss_rate", "SPECIES": "SO2"})
    assert rc != 0 and "Module needs quantity mass or volume mixing ratio!" in out
    rc, out = _run(trac, tmp, {"NQ": 2, "QNT_NAME[0]": "m", "QNT_NAME[1]": "mloss_oh", "OH_CHEM_REACTION": 0})
    assert "mloss_oh" in out and "does not provide" not in out
    rc, out = _run(trac, tmp, {"NQ": 2, "QNT_NAME[0]": "m", "QNT_NAME[1]": "Cx", "OH_CHEM_REACTION": 0})
    assert rc != 0 and "does not provide" in out


@pytest.fixture(scope="module")
def log10_lib():
    out = os.path.join(ROOT, "tests", "c", "build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "log10_cpu.so")
    cmd = ["gcc", "-O2", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC", "-std=gnu99", "-Wall", "-Wextra", "-I", CSRC,
           "-o", so, os.path.join(ROOT, "tests", "c", "log10_cpu.c"), "-lm"]
    if " fma " in open("/proc/cpuinfo").read():
        cmd.insert(1, "-mfma")
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    L.cmp_log10.restype = C.c_size_t
    return L


def test_restated_log10_has_the_librarys_bits(log10_lib):
    """glibc's log10 (__ieee754_log10 on top of log) over 1.2e8 arguments: the argument sets of log, and the
    arguments module_oh_chem hands it (k0 M / ki of the presets, 1e-3 ... 1e3)."""
    flags = open("/proc/cpuinfo").read()
    if not (" fma " in flags and " avx2 " in flags):
        pytest.skip("host CPU without FMA + AVX2: glibc selects other variants of log here")
    rng = np.random.default_rng(20261015)
    total = 0
    for rnd in range(3):
        sets = list(libm_args.log_sets(rng, 5_000_000)) + [("oh_chem", 10.0 ** rng.uniform(-3.0, 3.0, 10_000_000))]
        for name, x in sets:
            x = np.ascontiguousarray(x, dtype=np.float64)
            first = C.c_size_t(2 ** 63)
            bad = log10_lib.cmp_log10(x.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(len(x)), C.byref(first))
            assert bad == 0, (name, bad, float(x[first.value]).hex())
            total += len(x)
    assert total >= 10 ** 8
