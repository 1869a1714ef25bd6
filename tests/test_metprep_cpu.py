"""tests/refmetprep.py -- the restatement of the derived meteo fields the GPU tests compare mphip_derive_met with --
against closed forms, and the condition under which that comparison leaves nothing out: on every seeded input of the
GPU tests no comparison between computed values is decided by less than 1e-9 (relative), so that the default library,
whose doubles differ from the reference's by an ulp, takes the same branches everywhere."""
import math

import numpy as np
import pytest

import refmetprep as R

# the inputs of tests/test_gpu_metprep.py: (nx, ny, np, seed, latitudes descending)
GPU_INPUTS = [(9, 7, 20, 2024, False), (9, 7, 20, 2024, True), (37, 19, 20, 2024, False), (37, 19, 20, 2024, True),
              (5, 4, 137, 2024, False), (5, 4, 137, 2024, True)]
SMOOTHING = [(-1, -1), (0, 0), (2, 1)]


def test_geopotential_of_an_isothermal_dry_column():
    """z = zs + RI / MA / G0 T log(ps / p) with T the virtual temperature of a column at the dry floor of TVIRT."""
    p = [1000. * math.exp(-0.3 * k) for k in range(12)]
    T, ps, zs = 250., 912.5, 0.8
    tv = R.TVIRT(T, 0.)
    z = R.geopot_column(p, [T] * 12, [0.] * 12, ps, zs)
    for k in range(12):
        assert z[k] == pytest.approx(zs + R.RI / R.MA / R.G0 * tv * math.log(ps / p[k]), rel=1e-13, abs=1e-12)
    assert z[0] < zs < z[1]         # the surface lies between the two lowest levels: one below, the rest above


def test_ozone_column_of_a_constant_mixing_ratio():
    """Constant o3 above the surface: the trapezoids add up to o3 MO3 / MA (p[k0] - p[np-1]) 100 / G0 / 2.1415e-5, k0 the
    first level of the first layer whose lower level is at or above the surface."""
    p = [1000. - 60. * k for k in range(15)]
    x, ps = 3e-6, 905.
    k0 = next(k for k in range(15) if p[k] <= ps)
    want = x * R.MO3 / R.MA * (p[k0] - p[-1]) * 100. / R.G0 / 2.1415e-5
    assert R.o3c_column(p, [x] * 15, ps) == pytest.approx(want, rel=1e-13)
    assert 200. < R.o3c_column(p, [x] * 15, ps) < 2000.         # Dobson units of a plausible size


def _column(met, name):
    c = R.SPECIAL[name]
    return c // met.ny, c % met.ny


@pytest.mark.parametrize("key", GPU_INPUTS[::2], ids=lambda k: "x".join(map(str, k[:3])))
def test_marked_columns(key):
    met = R.atmosphere(*key)
    out, _ = R.reference(key)
    ix, iy = _column(met, "dry")
    assert all(np.isnan(out[k][ix, iy]) for k in ("plcl", "plfc", "pel", "cape", "cin"))
    ix, iy = _column(met, "cloud_free")
    assert np.isnan(out["pct"][ix, iy]) and np.isnan(out["pcb"][ix, iy]) and out["cl"][ix, iy] == 0
    ix, iy = _column(met, "cloud_top_only")
    p20 = R.P(20.)
    khi = max(k for k in range(met.np - 1) if met.p[k] >= p20 and met.p[k] <= met.f2["ps"][ix, iy])
    assert out["pct"][ix, iy] == np.float32(0.5 * (met.p[khi] + met.p[khi + 1]))
    assert out["pcb"][ix, iy] == np.float32(0.5 * (met.p[khi] + met.p[khi - 1])) and out["cl"][ix, iy] > 0


@pytest.mark.parametrize("key", GPU_INPUTS[::2], ids=lambda k: "x".join(map(str, k[:3])))
def test_the_input_covers_the_cases(key):
    """Surfaces below the lowest level, between levels and above many; columns with CAPE and an equilibrium level and
    columns without; clouds in some columns; the periodic column repeats the first."""
    met = R.atmosphere(*key)
    out, _ = R.reference(key)
    ps = met.f2["ps"]
    assert (ps > met.p[0]).any() and (ps < met.p[0]).any()
    assert (met.p > ps.min()).sum() >= max(2, met.np // 12)          # a mountain: the surface above that many levels
    assert 600. <= ps.min() and ps.max() == 1040.
    free = (out["cape"] > 0) & np.isfinite(out["pel"]) & np.isfinite(out["plfc"])
    none = np.isnan(out["plfc"]) & (out["cape"] == 0) & np.isnan(out["cin"])
    assert free.any() and none.any()
    # (twenty levels leave gaps of more than 50 hPa: only where a level lies within 50 hPa above the surface is there a parcel)
    assert np.isfinite(out["pct"]).any() and np.isfinite(out["plcl"]).sum() >= ps.size // 5
    assert (out["pbl"] < ps).all() and (out["pbl"] >= np.float32(ps * math.exp(-5. / 7.)) * (1 - 1e-6)).all()
    assert np.all(np.diff(out["z"], axis=2) > 0) and 100. < out["o3c"].min() and out["o3c"].max() < 800.
    for name, a in out.items():
        assert np.array_equal(a[-1], a[0], equal_nan=True) or name == "z", name
    p20 = R.P(20.)
    assert min(abs(pk - p20) / p20 for pk in met.p) > 1e-9          # the cloud search's upper bound lies between levels


def test_smoothing_weights_and_wrap():
    """A constant field stays constant to float rounding; a NaN is skipped, and a point whose neighbours are all NaN gives NaN."""
    z = np.full((6, 5, 2), 3.25, dtype=np.float32)
    lon = np.arange(6) * 60.
    assert np.allclose(R.smooth(z, lon, -1, -1), 3.25, rtol=3e-7)
    z[2, 2, 0] = np.nan
    s = R.smooth(z, lon, 2, 1)
    assert np.isfinite(s).all() and np.allclose(s, 3.25, rtol=3e-7)
    z[:, :, 1] = np.nan
    assert np.isnan(R.smooth(z, lon, 2, 2)[:, :, 1]).all()
    # the wrap: with a half-width of 2 the first column sees the last one
    z = np.zeros((6, 5, 1), dtype=np.float32)
    z[5] = 4.
    assert R.smooth(z, lon, 2, 1)[0, 2, 0] == np.float32(0.5 * 4. / 2.)
    assert np.array_equal(R.smooth(z, lon, 0, 3), z)


@pytest.mark.parametrize("key", GPU_INPUTS, ids=lambda k: "x".join(map(str, k[:3])) + ("desc" if k[4] else ""))
def test_no_comparison_is_decided_by_rounding(key):
    """The condition of the GPU comparison.  (If it fails: change the seed, not the bound.)"""
    for met_pbl in (3, 2):
        for sx, sy in (SMOOTHING if met_pbl == 2 else SMOOTHING[:1]):
            _, margin = R.reference(key, met_pbl, sx, sy)
            worst = np.unravel_index(np.argmin(margin), margin.shape)
            assert margin.min() >= 1e-9, (met_pbl, sx, sy, worst, margin.min())
