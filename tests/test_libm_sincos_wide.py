"""cos / sin of geo2cart's longitudes: mphip_libm_cos_wide / mphip_libm_sin_wide (mptrac_amd/csrc/mphip_libm.h) restate the
branch 2.426265 <= |x| < 105414350 of the C library's s_sin.c (reduce_sincos + do_sincos) and fall through to
mphip_libm_cos / _sin below it.  The same header is compiled for the CPU (tests/c/libm_wide_cpu.c) and compared bit by bit
with the running libm -- the one write_sample / write_station of the host call; the condition is 0 differences, since
the membership tests of the device's sample and station kernels rest on these bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mptrac_amd", "csrc")
_dp = C.POINTER(C.c_double)
LOW = float.fromhex("0x1.368fdp+1")        # first argument of the wide branch (high word 0x400368fd)
HIGH = float.fromhex("0x1.921fbp+26")      # first argument beyond it (high word 0x419921fb)


def _has(flag):
    try:
        return " %s " % flag in open("/proc/cpuinfo").read()
    except OSError:
        return False


@pytest.fixture(scope="module")
def lib():
    if not (_has("fma") and _has("avx2")):
        pytest.skip("host CPU without FMA + AVX2: glibc selects other variants of cos / sin here")
    out = os.path.join(ROOT, "tests", "c", "build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libm_wide_cpu.so")
    cmd = ["gcc", "-mfma", "-O2", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC", "-std=gnu99", "-Wall", "-Wextra", "-I", CSRC,
           "-o", so, os.path.join(ROOT, "tests", "c", "libm_wide_cpu.c"), "-lm"]
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    L.cmp_wide.restype = C.c_size_t
    return L


def _check(L, name, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    for which, fn in ((0, "cos"), (1, "sin")):
        first = C.c_size_t(2 ** 63)
        bad = L.cmp_wide(which, x.ctypes.data_as(_dp), C.c_size_t(len(x)), C.byref(first))
        assert bad == 0, (fn, name, bad, float(x[first.value]).hex())
    return len(x)


def test_reduction_constants_are_the_generated_ones(lib):
    assert lib.check_wide_constants() == 0


def test_wide_cos_sin_over_the_longitudes_of_geo2cart(lib):
    """10^8 arguments with 2.42 <= |x| <= 7 (a longitude of up to 360 degrees is 6.2832 rad), both signs."""
    rng = np.random.default_rng(20261017)
    total = 0
    for _ in range(10):
        x = rng.uniform(2.42, 7.0, 10_000_000) * rng.choice([-1.0, 1.0], 10_000_000)
        total += _check(lib, "2.42 <= |x| <= 7", x)
    assert total >= 10 ** 8


def test_wide_cos_sin_sweep_to_1e5(lib):
    rng = np.random.default_rng(20261018)
    n = 4_000_000
    _check(lib, "uniform to 1e5", rng.uniform(-1e5, 1e5, n))
    _check(lib, "log-uniform 2.4 .. 1e5", 10.0 ** rng.uniform(np.log10(2.4), 5.0, n) * rng.choice([-1.0, 1.0], n))
    _check(lib, "log-uniform to the end of the branch", 10.0 ** rng.uniform(0.0, np.log10(HIGH), n))
    _check(lib, "regular sweep", np.arange(-1e5, 1e5, 0.0371))
    # next to the multiples of pi / 2, where the reduced argument is tiny and its low part carries the result
    m = rng.integers(1, 63662, n).astype(np.float64)
    _check(lib, "next to multiples of pi / 2", m * (np.pi / 2) + rng.uniform(-1e-6, 1e-6, n) * rng.choice([0.0, 1.0, 1e-6], n))
    _check(lib, "below the branch (falls through)", rng.uniform(-2.43, 2.43, n))


def test_wide_cos_sin_at_the_branch_boundaries(lib):
    edges = []
    for b in (LOW, HIGH, 0.126, 0.855469, np.pi / 2, np.pi, 1.5 * np.pi, 2 * np.pi, 7.0):
        for s in (1.0, -1.0):
            for v in (np.nextafter(b, 0.0), b, np.nextafter(b, np.inf)):
                if abs(v) < HIGH:
                    edges.append(s * v)
    _check(lib, "edges", np.array(edges))
    # the first argument beyond the branch is reported as not handled, never answered
    x = np.array([HIGH, -HIGH, 1e300, np.inf, np.nan])
    out = np.empty_like(x)
    handled = np.ones(len(x), dtype=np.int32)
    for which in (0, 1):
        lib.rst_wide(which, x.ctypes.data_as(_dp), C.c_size_t(len(x)), out.ctypes.data_as(_dp),
                     handled.ctypes.data_as(C.POINTER(C.c_int)))
        assert not handled.any() and np.isnan(out).all()


def test_wide_cos_sin_of_every_quarter_degree(lib):
    """DEG2RAD of every multiple of 0.25 degrees in [-180, 360], as geo2cart forms it (x * pi / 180)."""
    deg = np.arange(-720, 1441) * 0.25
    assert deg[0] == -180.0 and deg[-1] == 360.0
    _check(lib, "quarter degrees", deg * (np.pi / 180.0))


def test_the_check_has_teeth(lib):
    """The same header with every fused multiply-add replaced by a multiplication and an addition (-DLIBM_WIDE_UNFUSED)
    is not the library's cos / sin in some last bits: cmp_wide, the counter of every test above, finds them -- and
    finds none in the same arguments with the header as it is."""
    out = os.path.join(ROOT, "tests", "c", "build", "libm_wide_cpu_unfused.so")
    subprocess.check_call(["gcc", "-DLIBM_WIDE_UNFUSED", "-O2", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC", "-std=gnu99",
                           "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "c", "libm_wide_cpu.c"), "-lm"])
    U = C.CDLL(out)
    U.cmp_wide.restype = C.c_size_t
    x = np.random.default_rng(5).uniform(2.5, 7.0, 200000)
    for which in (0, 1):
        first = C.c_size_t(2 ** 63)
        bad = U.cmp_wide(which, x.ctypes.data_as(_dp), C.c_size_t(len(x)), C.byref(first))
        assert 10 <= bad < len(x) // 100 and first.value < len(x), (which, bad)
    _check(lib, "the arguments of the unfused comparison", x)
