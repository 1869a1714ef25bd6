"""tests/refregrid.py, the restatement the device's regridding is compared with, against independent statements, and
what of mphip_regrid_met needs no device: mphip_sizeof_regrid and mphip_regrid_shape.

ML2PL: on strictly monotone columns with targets inside the column np.interp on the reversed axis is the same piecewise
linear function, evaluated with other roundings (its slope form or its weights): the two agree within one float ulp of
the larger neighbouring value -- both are within a few double roundings of the exact interpolant, a value between the
two neighbours, and each is rounded to float once.  SAMPLE: a constant field, the identity, plain striding."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import refregrid as R        # noqa: E402
import regrid_cases as K     # noqa: E402


def _inside_targets(met, met_np):
    pl = met.f3["pl"].astype(np.float64)
    lo, hi = pl.min(axis=2).max(), pl.max(axis=2).min()      # inside every column
    return np.exp(np.linspace(np.log(hi), np.log(lo), met_np + 2))[1:-1]


@pytest.mark.parametrize("ascending", [False, True])
@pytest.mark.parametrize("npl,met_np", [(7, 5), (137, 60), (7, 60)])
def test_ml2pl_is_np_interp_on_monotone_columns(npl, met_np, ascending):
    met = K.ml_atmosphere(9, 8, npl, ascending=ascending)
    q = _inside_targets(met, met_np)
    ref = R.ml2pl(met, q)
    pl = met.f3["pl"].astype(np.float64)
    for name in R.ML_FIELDS:
        f = met.f3[name].astype(np.float64)
        k, _ = R.brackets(pl, q)
        for ix in range(met.nx):
            for iy in range(met.ny):
                x, y = (pl[ix, iy], f[ix, iy]) if ascending else (pl[ix, iy, ::-1], f[ix, iy, ::-1])
                want = np.interp(q, x, y)
                kk = k[ix, iy]
                bound = R.ulp32(np.maximum(np.abs(f[ix, iy][kk]), np.abs(f[ix, iy][kk + 1])))
                assert (np.abs(ref.f3[name][ix, iy].astype(np.float64) - want) <= bound).all(), (name, ix, iy)


def test_ml2pl_reproduces_a_field_linear_in_pressure():
    met = K.ml_atmosphere(5, 3, 137)
    pl = met.f3["pl"].astype(np.float64)
    met.f3["t"] = (200.0 + 0.0625 * pl).astype(np.float32)      # exact products; the sum is rounded to float
    q = _inside_targets(met, 60)
    ref = R.ml2pl(met, q)
    k, _ = R.brackets(pl, q)
    f = met.f3["t"].astype(np.float64)
    want = 200.0 + 0.0625 * q[None, None, :]
    # the nodes themselves are off the line by half a float ulp each: within one float ulp of the larger neighbour
    bound = R.ulp32(np.maximum(np.take_along_axis(f, k, 2), np.take_along_axis(f, k + 1, 2)))
    assert (np.abs(ref.f3["t"].astype(np.float64) - want) <= bound).all()


@pytest.mark.parametrize("ascending", [False, True])
def test_ml2pl_targets_beyond_either_end_return_the_end_value(ascending):
    met = K.ml_atmosphere(5, 3, 7, ascending=ascending)
    ref = R.ml2pl(met, [1100.0, 1080.0, 0.9, 0.5])
    bottom, top = (-1, 0) if ascending else (0, -1)
    for name in R.ML_FIELDS:
        f = met.f3[name]
        assert np.array_equal(ref.f3[name][:, :, 0], f[:, :, bottom]) and np.array_equal(ref.f3[name][:, :, 1], f[:, :, bottom])
        assert np.array_equal(ref.f3[name][:, :, 2], f[:, :, top]) and np.array_equal(ref.f3[name][:, :, 3], f[:, :, top])
    assert np.array_equal(ref.p, [1100.0, 1080.0, 0.9, 0.5])
    assert all(np.array_equal(ref.f2[n], met.f2[n]) for n in met.f2)


def test_locate_irr_on_a_descending_column():
    pl = [900.0, 700.0, 500.0, 300.0, 100.0]
    for q, k in ((950.0, 0), (900.0, 0), (899.0, 0), (700.0, 0), (699.0, 1), (300.0, 2), (299.0, 3), (100.0, 3), (50.0, 3)):
        assert R.locate_irr(pl, q) == k, q
    up = pl[::-1]
    for q, k in ((50.0, 0), (100.0, 0), (299.0, 0), (300.0, 1), (899.0, 3), (900.0, 3), (950.0, 3)):
        assert R.locate_irr(up, q) == k, q


@pytest.mark.parametrize("s,exact", [((2, 2, 2), True), ((3, 2, 2), False), ((3, 3, 1), False), ((2, 1, 2), True)])
def test_sample_of_a_constant_field(s, exact):
    """The constant is 287.625 = 2301 / 8, twelve significant bits.  Half-widths 2 (or 1): every weight is a multiple of
    1/8 and ws a sum of such, so every product and partial sum is exact and a / ws is the constant -- what "exactly"
    presupposes: with a full mantissa (287.65) the partial sums c k / 8 are rounded, and so is the quotient.  Other
    half-widths round their weights: within one float ulp.  The full-mantissa constant is reported, not asserted: its
    partial sums carry up to one rounding per term (measured: 1 ulp with half-widths 2, 2 ulp with 3 2 2 at clamped
    corners)."""
    c = np.float32(287.625)
    f = np.full((9, 7, 6), c)
    out = R.sample_field(f, (2, 1, 1), s)
    out2 = R.sample_field(f[:, :, 0], (2, 1), s[:2])
    assert out.shape == (5, 7, 6) and out2.shape == (5, 7)
    for o in (out, out2):
        assert (R.ulp_distance(o, np.full_like(o, c)) <= (0 if exact else 1)).all()
    full = np.full((9, 7, 6), np.float32(287.65))
    print(s, "full mantissa: largest distance", int(R.ulp_distance(R.sample_field(full, (2, 1, 1), s), full[::2]).max()))


def test_sample_identity_and_plain_striding():
    met = K.pl_atmosphere(9, 7, 6)
    met.f3["t"][1, 2, 3] = -0.0
    same = R.sample(met)
    for n, a in met.f3.items():
        assert np.array_equal(same.f3[n].view(np.int32), a.view(np.int32)), n
    for n, a in met.f2.items():
        assert np.array_equal(same.f2[n].view(np.int32), a.view(np.int32)), n
    assert np.array_equal(same.lon, met.lon) and np.array_equal(same.p, met.p)
    strided = R.sample(met, (2, 3, 2))
    assert (strided.nx, strided.ny, strided.np) == (5, 3, 3)
    for n, a in met.f3.items():
        assert np.array_equal(strided.f3[n].view(np.int32), a[::2, ::3, ::2].view(np.int32)), n
    assert np.array_equal(strided.f2["ps"], met.f2["ps"][::2, ::3])
    assert np.array_equal(strided.lon, met.lon[::2]) and np.array_equal(strided.lat, met.lat[::3])
    assert np.array_equal(strided.p, met.p[::2])


def test_sample_wraps_in_longitude_and_clamps_elsewhere():
    """One point by hand: the corner (0, 0, 0) with half-widths 2, 2, 2 reads columns nx-1, 0, 1, rows 0, 1, levels 0, 1."""
    met = K.pl_atmosphere(9, 7, 6)
    f = met.f3["t"]
    a = ws = np.float32(0)
    for ix2, wx in ((-1, 0.5), (0, 1.0), (1, 0.5)):
        for iy2, wy in ((0, 1.0), (1, 0.5)):
            for ip2, wp in ((0, 1.0), (1, 0.5)):
                w = np.float32(np.float32(np.float32(wx) * np.float32(wy)) * np.float32(wp))
                a = np.float32(a + np.float32(w * f[ix2 % 9, iy2, ip2]))
                ws = np.float32(ws + w)
    assert R.sample_field(f, (1, 1, 1), (2, 2, 2))[0, 0, 0] == np.float32(a / ws)


def test_sample_spreads_a_nan():
    met = K.with_nan(K.pl_atmosphere(9, 7, 6))
    out = R.sample_field(met.f3["t"], (1, 1, 1), (2, 2, 2))
    want = np.zeros((9, 7, 6), dtype=bool)
    want[3:6, 2:5, 1:4] = True
    assert np.array_equal(np.isnan(out), want)


# ---- the library, without a device ----------------------------------------------------------------------------------------

def _met_struct(nx, ny, n, npl=0):
    from mptrac_amd import hip
    m = hip.MphipMet()
    m.nx, m.ny, m.np, m.npl = nx, ny, n, npl
    m.sx, m.sy, m.sx2 = ny * n, n, ny
    return m


def _shape(m, what, **kw):
    from mptrac_amd import hip
    L = hip.load()
    met_p = np.ascontiguousarray(kw.pop("met_p", ()), dtype=np.float64)
    o = hip.MphipRegrid(len(met_p), hip._ptr(met_p, hip._dp) if len(met_p) else None,
                        *(kw.pop(k, 1) for k in ("met_dx", "met_dy", "met_dp", "met_sx", "met_sy", "met_sp")))
    n = [C.c_int(-1) for _ in range(3)]
    rc = L.mphip_regrid_shape(C.byref(m), what, C.byref(o), *(C.byref(k) for k in n))
    return rc, tuple(k.value for k in n)


def test_sizeof_regrid_matches_the_python_mirror():
    from mptrac_amd import hip
    L = hip.load()
    assert L.mphip_sizeof_regrid() == C.sizeof(hip.MphipRegrid)


@pytest.mark.parametrize("n,d", [((9, 7, 6), (2, 3, 2)), ((19, 11, 20), (4, 5, 6)), ((721, 361, 60), (2, 2, 1)),
                                 ((10, 10, 10), (3, 7, 9)), ((9, 7, 6), (1, 1, 1))])
def test_regrid_shape_is_the_restatements(n, d):
    rc, got = _shape(_met_struct(*n), 2, met_dx=d[0], met_dy=d[1], met_dp=d[2])
    assert rc == 0 and got == R.shape(n, d)


def test_regrid_shape_of_ml2pl_and_of_both():
    q = K.targets(60)
    assert _shape(_met_struct(9, 8, 137, 137), 1, met_p=q) == (0, (9, 8, 60))
    assert _shape(_met_struct(9, 8, 137, 137), 3, met_p=q, met_dx=2, met_dy=3, met_dp=7) == (0, (5, 3, 9))


def test_regrid_shape_refuses_what_the_call_refuses():
    q = K.targets(5)
    untouched = (-1, -1, -1)
    for m, what, kw in [
            (_met_struct(9, 8, 7, 7), 0, {}), (_met_struct(9, 8, 7, 7), 4, {}),
            (_met_struct(9, 8, 1, 1), 1, dict(met_p=q)), (_met_struct(9, 8, 7, 6), 1, dict(met_p=q)),
            (_met_struct(9, 8, 7, 7), 1, dict(met_p=q[:1])), (_met_struct(9, 8, 7, 7), 1, dict(met_p=q[::-1])),
            (_met_struct(9, 8, 7, 7), 1, dict(met_p=[500.0, 500.0])), (_met_struct(9, 8, 7, 7), 1, dict(met_p=[500.0, -1.0])),
            (_met_struct(9, 8, 7, 7), 1, dict(met_p=[np.inf, 500.0])), (_met_struct(9, 8, 7, 7), 1, dict(met_p=[500.0, np.nan])),
            (_met_struct(9, 8, 20000, 20000), 1, dict(met_p=q)),
            (_met_struct(9, 7, 6), 2, dict(met_dx=0)), (_met_struct(9, 7, 6), 2, dict(met_sp=0)), (_met_struct(9, 7, 6), 2, dict(met_dy=-1)),
            (_met_struct(9, 7, 6), 2, dict(met_sx=11)), (_met_struct(9, 7, 6), 2, dict(met_dx=9)),
            (_met_struct(9, 7, 6), 2, dict(met_dy=7)), (_met_struct(9, 7, 6), 2, dict(met_dp=6)),
            (_met_struct(12, 12, 8), 2, dict(met_sx=11, met_sy=11, met_sp=4))]:
        assert _shape(m, what, **kw) == (1, untouched), (what, kw)
    assert _shape(_met_struct(9, 7, 6), 2, met_sx=10)[0] == 0
    assert _shape(_met_struct(12, 12, 8), 2, met_sx=10, met_sy=11, met_sp=4)[0] == 0
    assert R.tile_floats((1, 1, 1), (10, 11, 4)) * 4 <= 65536 < R.tile_floats((1, 1, 1), (11, 11, 4)) * 4
