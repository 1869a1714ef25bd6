"""The restatement of the detrending (tests/refdetrend.py) against properties that need no device, the size of
mphip_detrend_t, and the control keys of MET_DETREND in mptrac_read_ctl (the control file is read before any device is
touched: the tool goes on to the input file, which is absent)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import detrend_cases as K                      # noqa: E402
import refdetrend as R                         # noqa: E402
from test_regrid_ctl_cpu import _met_conv      # noqa: E402


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32)))


def test_constant_field():
    """A power of two times the weights is exact and scaling by it commutes with every rounding of the two sums, so b =
    256 ws exactly and the result is +0: within one float ulp of the constant as stated, in fact exact.  A constant
    with a full mantissa rounds every product: its result is bounded like any other field's, by (taps + 1) 2^-24 c."""
    met, scale = K.case("poles")
    for c in (256.0, 287.6251):
        for f in met.f3:
            met.f3[f][...] = c
        res = R.detrend(met, scale)
        taps = np.array(R.taps(met.lon, met.lat, scale), dtype=np.float64)[None, :, None]
        for f, (out, bg) in res.items():
            worst = float(np.abs(out).max())
            print(f"constant {c}: field {f}: largest |out| {worst:.3e} = {worst / float(_ulp(np.float32(c))):.2f} ulp")
            if c == 256.0:
                assert (np.abs(out) <= _ulp(np.float32(c))).all() and (out == 0).all()
            assert (np.abs(out) <= (taps + 1) * 2.0 ** -24 * c).all()


def test_against_a_float64_evaluation():
    """Case `widest` (up to 13 x 7 taps): float sums in the stated order against double sums of the same terms."""
    met, scale = K.case("widest")
    ref = K.reference("widest")
    taps = np.array(R.taps(met.lon, met.lat, scale), dtype=np.float64)[None, :, None]
    assert taps.max() == 13 * 7
    for f in R.FIELDS:
        dense, mag = R.dense64(met, scale, f)
        err = np.abs(ref[f][0].astype(np.float64) - dense)
        bound = (taps + 1) * 2.0 ** -24 * mag
        print(f"{f}: largest error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), f


def test_half_widths_of_the_cases():
    """The cases reach what they are meant to reach: both limits of either half-width and a value between."""
    met, scale = K.case("widest")
    sy, sx = R.half_widths(met.lon, met.lat, scale)
    assert sy == met.ny // 2 and sx == [met.nx // 2] * met.ny
    met, scale = K.case("poles")
    sy, sx = R.half_widths(met.lon, met.lat, scale)
    assert sx[0] == 1 and sx[-1] == 1                                   # the DX2DEG zero at the poles
    assert sx[1] == met.nx // 2 and sx[-2] == met.nx // 2                # next to them: the upper limit
    assert 1 < sx[met.ny // 2] < met.nx // 2 and 1 < sy < met.ny // 2    # the equator: strictly between
    met, scale = K.case("narrowest")
    sy, sx = R.half_widths(met.lon, met.lat, scale)
    assert sy == 1 and sx == [1] * met.ny
    met, scale = K.case("regional")
    sy, sx = R.half_widths(met.lon, met.lat, scale)
    assert 1 < sy < met.ny // 2 and all(1 < s < met.nx // 2 for s in sx)


def test_a_nan_and_an_infinity_spread_over_their_windows():
    met, scale = K.case("nonfinite")
    ref = K.reference("nonfinite")
    sy, sx = R.half_widths(met.lon, met.lat, scale)
    t, u = ref["t"][0], ref["u"][0]
    for iy in range(met.ny):
        for ix in range(met.nx):
            d = min(abs(ix - 5), met.nx - abs(ix - 5))
            hit = abs(iy - 6) <= sy and d <= sx[iy]
            assert np.isnan(t[ix, iy, 2]) == hit, (ix, iy)
    assert np.isfinite(t[:, :, [0, 1, 3, 4]]).all() and np.isfinite(ref["v"][0]).all()
    # +inf: the background is +inf (or NaN where a weight underflowed to 0), the result -inf or NaN: never finite
    d = np.minimum(np.abs(np.arange(met.nx) - 20), met.nx - np.abs(np.arange(met.nx) - 20))
    for iy in range(met.ny):
        hit = (abs(iy - 1) <= sy) & (d <= sx[iy])
        assert (~np.isfinite(u[hit, iy, 0])).all() and np.isfinite(u[~hit, iy, 0]).all(), iy


def test_sizeof_detrend_matches_the_python_mirror():
    from mptrac_amd import hip
    L = hip.load()
    assert L.mphip_sizeof_detrend() == C.sizeof(hip.MphipDetrend)


def test_met_detrend_is_accepted_with_hip_met_prep_2(tmp_path):
    rc, out = _met_conv(str(tmp_path), "MET_DETREND", "5", model_levels=False, prep=2)
    assert "Cannot open file" in out and "not part of this build" not in out, out[-1500:]


@pytest.mark.parametrize("value", ["0", "-1", "-999"])
def test_met_detrend_off_is_accepted_without_hip_met_prep(tmp_path, value):
    rc, out = _met_conv(str(tmp_path), "MET_DETREND", value, model_levels=False, prep=0)
    assert "Cannot open file" in out and "not part of this build" not in out, out[-1500:]


@pytest.mark.parametrize("prep", [0, 1])
def test_met_detrend_without_hip_met_prep_2_is_refused_and_the_message_names_it(tmp_path, prep):
    rc, out = _met_conv(str(tmp_path), "MET_DETREND", "5", model_levels=False, prep=prep)
    assert rc != 0 and "Error" in out and all(w in out for w in ("MET_DETREND", "not part of this build", "HIP_MET_PREP 2")), out[-1500:]


@pytest.mark.parametrize("value", ["nan", "inf"])
def test_met_detrend_not_finite_is_refused(tmp_path, value):
    rc, out = _met_conv(str(tmp_path), "MET_DETREND", value, model_levels=False, prep=2)
    assert rc != 0 and "Error" in out and "MET_DETREND" in out, out[-1500:]


def test_met_detrend_with_model_level_advection_is_refused(tmp_path):
    rc, out = _met_conv(str(tmp_path), "MET_DETREND", "5", "ADVECT_VERT_COORD", "2", model_levels=True, prep=2)
    assert rc != 0 and "Error" in out and "MET_DETREND" in out and "ADVECT_VERT_COORD" in out, out[-1500:]
