"""MET_DETREND through the drop-in boundary: `met_conv` and `trac` on the netCDF world of
tests/test_gpu_pv_tropo_driver.py (three hourly files, 37 x 19 x 20, 3000 particles, two hours) with HIP_MET_PREP 2.

The reader detrends last: t, u, v, w of the converted file are mphip_detrend_met of the file converted without the key,
bit for bit, and every other plane -- the derived ones among them -- is the same byte for byte.  The read-ahead thread of
HIP_MET_PREFETCH 1 reads the same, and without the key nothing changes.  (A run from the converted MET_TYPE 1 files is
not compared: the reader of that format limits t to >= 0 as the reference's does, and a perturbation temperature has both
signs -- docs/host_layer_and_transfers.md.)"""
import os

import numpy as np
import pytest

import hostfiles as hf
from mptrac_amd import build
from mptrac_amd.synth import Met
from test_gpu_pv_tropo_driver import HOURS, T0, _atm_files, _run, _same_files, _trac, world      # noqa: F401

pytestmark = pytest.mark.gpu

SCALE = "3000"       # km: half-widths 3 rows and 3 ... 18 columns on the 10 degree grid
DETRENDED = ("t", "u", "v", "w")


def _convert(world, base, k, *args):
    tmp = world["tmp"]
    src = hf.met_filename(os.path.join(tmp, "met"), T0 + 3600.0 * k)[:-4] + ".nc"
    dst = hf.met_filename(os.path.join(tmp, base), T0 + 3600.0 * k)
    rc, out = _run([build.MET_CONV_BIN, os.path.join(tmp, "old.ctl"), src, "0", dst, "1", "HIP_MET_PREP", "2", *args])
    assert rc == 0, out[-2000:]
    return dst, out


@pytest.fixture(scope="module")
def converted(world):
    """The three files converted to MET_TYPE 1 without and with MET_DETREND."""
    plain, det = [], []
    for k in range(HOURS + 1):
        plain.append(_convert(world, "plain", k)[0])
        dst, out = _convert(world, "det", k, "MET_DETREND", SCALE)
        assert "Detrended on the device" in out
        det.append(dst)
    return plain, det


@pytest.fixture(scope="module")
def detrended_run(world):
    rc, out, d = _trac(world, "det_run", "old", "HIP_MET_PREP", "2", "MET_DETREND", SCALE)
    assert rc == 0, out[-3000:]
    assert "Detrended on the device" in out
    return d


@pytest.fixture(scope="module")
def plain_run(world):
    rc, out, d = _trac(world, "plain_run", "old", "HIP_MET_PREP", "2")
    assert rc == 0, out[-3000:]
    assert "Detrended on the device" not in out
    return d


def test_met_conv_writes_what_detrend_met_returns_and_nothing_else_changes(converted):
    from test_gpu_metprep import bare_context
    from test_gpu_metprep_driver import read_met_bin
    sim = bare_context()
    try:
        for k, (a, b) in enumerate(zip(*converted)):
            time, (lon, lat, p), f2, f3 = read_met_bin(a)
            time2, axes2, g2, g3 = read_met_bin(b)
            assert time == time2 and all(np.array_equal(x, y) for x, y in zip((lon, lat, p), axes2))
            got = sim.detrend_met(Met(time, lon, lat, p, {n: f3[n] for n in DETRENDED}, {}), float(SCALE))
            for n in DETRENDED:
                assert np.array_equal(got[n].view(np.uint32), g3[n].view(np.uint32)), (k, n)
            assert not np.array_equal(f3["t"], g3["t"]) and not np.array_equal(f3["u"], g3["u"])
            for n in f3:
                if n not in DETRENDED:
                    assert f3[n].tobytes() == g3[n].tobytes(), (k, n)
            for n in f2:
                assert f2[n].tobytes() == g2[n].tobytes(), (k, n)
            # perturbations: every temperature is smaller than the smallest full temperature
            assert np.abs(g3["t"]).max() < np.abs(f3["t"]).min()
    finally:
        sim.close()


def test_read_ahead_thread_detrends_the_same(world, detrended_run, plain_run):
    rc, out, d = _trac(world, "det_prefetch", "old", "HIP_MET_PREP", "2", "MET_DETREND", SCALE, "HIP_MET_PREFETCH", "1")
    assert rc == 0, out[-3000:]
    assert "Meteo data from the read-ahead" in out and "Detrended on the device" in out
    _same_files(detrended_run, d)
    # (and the detrended winds are not the full winds)
    a, b = (hf.read_atm_bin(_atm_files(x)[-1], 8) for x in (detrended_run, plain_run))
    assert not np.array_equal(a["lon"], b["lon"])


def test_without_the_key_nothing_changes(world, plain_run):
    rc, out, d = _trac(world, "off_run", "old", "HIP_MET_PREP", "2", "MET_DETREND", "-999")
    assert rc == 0, out[-3000:]
    assert "Detrended on the device" not in out
    _same_files(plain_run, d)
