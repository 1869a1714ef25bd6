"""The edge snapshots of tests/metprep_cases.py on the CPU: that the cases they are made for occur in the restatement (ties
between inputs by a counter, both end branches of the spline, smoothing points without a finite neighbour, options and the
Cartesian latitude changing outputs), the condition of the device comparison (no comparison between COMPUTED values on a
finite edge input is decided by less than 1e-9; comparisons between inputs are exact in any arithmetic and exempt -- the
named ties of refmetprep.Ties and reftropo's "coldpoint_end", nothing else), that the restatement ends on every
non-finite input with the values IEEE arithmetic gives, and the natural spline through three points in closed form."""
import math

import numpy as np
import pytest

import metprep_cases as C
import refmetprep as R
import reftropo as T

TIES = ("loc", "o3c", "cloud_ps", "cloud_min", "pbl3_ps", "pbl3_300", "cape_pbot", "cape_50")


def _at(columns, name):
    c = columns[name]
    return c // 7, c % 7


def test_every_tie_between_inputs_occurs():
    (cols, _), ties = C.columns("levels_era5", cloud_min=C.CLOUD_MIN)
    print(dict(ties.count))
    for name in TIES:
        assert ties.count[name] > 0, name
    assert set(ties.count) <= set(TIES)
    met = C.levels_era5()
    ps = met.f2["ps"]
    at = lambda name: _at(C.ERA5_COLUMNS, name)      # noqa: E731
    assert ps[at("ps_lowest")] == met.p[0] and ps[at("ps_interior")] == met.p[4] and ps[at("mountain")] == 600. == met.p[13]
    assert float(ps[at("ps_lowest")]) - 50. == met.p[2] and float(ps[at("ps_interior")]) - 50. == met.p[6]
    assert ps[at("above_lowest")] > 1000. > ps[at("below_lowest")] and ps[at("above_interior")] > 900. > ps[at("below_interior")]
    assert ps[at("above_lowest")] - ps[at("below_lowest")] < 2e-4 and ps[at("ps_below_axis")] > met.p[0]
    assert all(c // 7 not in (0, 8) for c in C.ERA5_COLUMNS.values())           # not the periodic column or its source
    # the surface ON a level: the level counts as above the surface -- z there is zs, its layer is in the ozone column
    ix, iy = at("ps_interior")
    assert cols["z"][ix, iy, 4] == met.f2["zs"][ix, iy]
    assert cols["o3c"][ix, iy] > R.o3c_column(met.p.tolist(), R._f64(met, "o3")[ix][iy], float(down32(900.)))
    # PBL 3: the 300 hPa level ends the search, and the result is no clamp
    ix, iy = at("stop_300")
    pbl, psc = float(cols["pbl3"][ix, iy]), float(ps[ix, iy])
    assert psc * math.exp(-5. / 7.) < pbl < 300. and pbl < psc * math.exp(-0.1 / 7.)
    # PBL 3 on the cold surfaces: the search passes the level ON the surface and ends below it -> the lower clamp
    for name in ("ps_interior", "mountain"):
        ix, iy = at(name)
        assert cols["pbl3"][ix, iy] == np.float32(float(ps[ix, iy]) * math.exp(-0.1 / 7.))
    # cloud water AT met_cloud_min is no cloud, one float ulp above it is one
    ix, iy = at("cloud_at_min")
    assert np.isnan(cols["pct"][ix, iy]) and cols["cl"][ix, iy] > 0
    ix, iy = at("cloud_above_min")
    assert cols["pct"][ix, iy] == np.float32(0.5 * (875. + 850.)) and cols["pcb"][ix, iy] == np.float32(0.5 * (875. + 900.))
    # the parcel of ps = 1000 holds the three levels 1000, 975, 950; one ulp below, two
    p, t, h = met.p.tolist(), R._f64(met, "t"), R._f64(met, "h2o")
    ix, iy = at("ps_lowest")
    three = R.cape_column(p, t[ix][iy], h[ix][iy], 1000., 200., R.Margin())
    two = R.cape_column(p, t[ix][iy], h[ix][iy], float(down32(1000.)), 200., R.Margin())
    assert np.float32(three[0]) != np.float32(two[0])


def down32(x):
    return C.down(x)


@pytest.mark.parametrize("name,low,high", [("np3", True, True), ("np4", True, True), ("high_start", True, False),
                                           ("low_top", False, True)])
def test_both_spline_ends_are_taken(name, low, high):
    """np3: zc = 4.9 ... 21.1 km; np4: ... 22.6 km (the WMO modes look up to 24.5 km); high_start begins at 6.5 km; low_top ends
    at 14.9 km.  The fine grid runs from 4.5 km to 21.5 (24.5) km."""
    zc = [T.Z(x) for x in C.SHORT_AXES[name]]
    for mode in (2, 3, 4, 5):
        for method in (0, 1):
            _, ties = C.tropo("short_" + name, mode, method)
            top = T.Z2[-1] if mode in (3, 4) else T.Z2[T.TOP]          # np4 ends between 21.5 and 24.5 km
            assert (ties.count["spline_low"] > 0) == low, (mode, method, ties.count)
            assert (ties.count["spline_high"] > 0) == (top >= zc[-1]), (mode, method, ties.count)
    assert (T.Z2[0] < zc[0]) == low and (T.Z2[-1] > zc[-1]) == high


def test_short_axes_give_tropopauses_and_none():
    n_finite = 0
    for name in C.SHORT_AXES:
        for mode in (2, 3, 4, 5):
            (ref, _), _ = C.tropo("short_" + name, mode, 1)
            n_finite += int(np.isfinite(ref["pt"]).sum())
    assert n_finite > 0


@pytest.mark.parametrize("shape", C.SMOOTH_SHAPES, ids=lambda s: "%dx%dx%d" % s[:3])
def test_smoothing_cases_have_points_without_a_finite_neighbour_and_wraps(shape):
    nx, ny, n, widths, dlon = shape
    name = "smooth_%dx%dx%d" % (nx, ny, n)
    met = C.snapshot(name)
    raw = C.columns(name)[0][0]["z"]
    assert np.isnan(raw[:, :, n - 2:]).all() and np.isnan(raw[2, 2]).all() and np.isfinite(raw[:, :, :n - 2]).sum() == (nx * ny - 1) * (n - 2)
    for sx, sy in widths:
        out = C.five(name, 3, sx, sy)[0]["z"]
        if sx < 0:
            assert abs(met.lon[1] - met.lon[0]) < 0.5
            sx, sy = 3, 2
            assert np.array_equal(out, R.smooth(raw, met.lon, 3, 2), equal_nan=True)
        assert np.isnan(out[:, :, n - 2:]).all()                       # no finite neighbour on those levels
        assert np.isfinite(out[:, :, :n - 2]).all()                    # ... and the NaN column is skipped and filled
        assert sx - 1 <= nx
        if sx > 1:
            # the halo wraps: raising the last column alone raises the smoothed first column
            bumped = raw.copy()
            bumped[nx - 1, :, 0] += np.float32(1.)
            assert (R.smooth(bumped, met.lon, sx, sy)[0, :, 0] > out[0, :, 0]).all()
    if (nx, ny, n) == (12, 5, 17):
        assert (13, 13) in widths and 13 - 1 == nx and 13 - 1 > ny
        assert (8 + 2 * 12) * (8 + 2 * 12) * 16 * 4 == 64 * 1024 < (8 + 2 * 12) * (8 + 2 * 13) * 16 * 4


def test_options_change_outputs():
    for met_pbl in (3, 2):
        dflt = C.five("levels_era5", met_pbl, cloud_min=C.CLOUD_MIN)[0]
        opt = C.five("levels_era5", met_pbl, pbl_min=C.PBL_MIN, pbl_max=C.PBL_MAX, cloud_min=C.CLOUD_MIN)[0]
        ps = C.levels_era5().f2["ps"].astype(np.float64)
        lower = opt["pbl"] == (ps * math.exp(-C.PBL_MIN / 7.)).astype(np.float32)
        upper = opt["pbl"] == (ps * math.exp(-C.PBL_MAX / 7.)).astype(np.float32)
        changed = opt["pbl"] != dflt["pbl"]
        print(met_pbl, int((lower & changed).sum()), int((upper & changed).sum()))
        assert (lower & changed).any() and (upper & changed).any(), met_pbl
    zero = C.five("levels_era5", 3, cloud_min=0.0)[0]
    some = C.five("levels_era5", 3, cloud_min=C.CLOUD_MIN)[0]
    assert (np.isnan(some["pct"]) != np.isnan(zero["pct"])).any()
    assert np.array_equal(zero["cl"], some["cl"])


def test_the_cartesian_latitude_changes_outputs():
    here = C.five("cartesian", lat=C.REF_LAT)[0]
    rows = C.five("cartesian")[0]
    differ = ~((here["pel"] == rows["pel"]) | (np.isnan(here["pel"]) & np.isnan(rows["pel"])))
    pt_here = C.tropo("cartesian", 1, 1, C.REF_LAT)[0][0]["pt"]
    pt_rows = C.tropo("cartesian", 1, 1)[0][0]["pt"]
    print(int(differ.sum()), int((pt_here != pt_rows).sum()))
    assert differ.any() and (here["cape"] != rows["cape"]).any()
    assert abs(C.snapshot("cartesian").lat[3]) < 1e-12 and differ[_at(C.ERA5_COLUMNS, "deep")]
    assert (pt_here != pt_rows).all() and (pt_here == pt_here[0, 0]).all()


@pytest.mark.parametrize("call", [c for c in C.calls("finite") if not c["refused"]], ids=lambda c: c["id"])
def test_no_comparison_between_computed_values_is_decided_by_rounding(call):
    """The condition of the device comparison.  (If it fails: change the seed or the column, not the bound.)"""
    assert C.margin(call) >= 1e-9, C.margin(call)


def test_every_axis_keeps_the_cloud_searchs_upper_bound_between_levels():
    p20 = R.P(20.)
    for name in C.SNAPSHOTS:
        if name == "tall_beyond":
            continue
        met = C.snapshot(name)
        assert min(abs(pk - p20) / p20 for pk in met.p) > 1e-9 and np.all(np.diff(met.p) < 0), name
    assert all(float(np.float32(x)) == x for x in C.ERA5) and len(C.ERA5) == 37


def test_the_level_limit_follows_the_formula():
    n = C.level_limit()
    assert 16 * n + 20 * (n | 1) <= 65536 < 16 * (n + 1) + 20 * ((n + 1) | 1) and n == 1819
    # 600 levels: 4, 8 and 16 columns per workgroup
    def cpb(nf):
        return max(c for c in (1, 2, 4, 8, 16, 32, 64) if 16 * 600 + 4 * nf * c * 601 <= 65536)
    assert {cpb(nf) for nf in (1, 2, 3, 4, 5)} == {4, 8, 16}


def test_the_restatement_ends_on_every_nonfinite_input():
    """Within its caps (a cap raises), with the values the arithmetic gives."""
    for call in C.calls("nonfinite"):
        if not call["refused"]:
            C.expected(call)
    met = C.nonfinite()
    at = lambda name: _at(C.NONFINITE_COLUMNS, name)      # noqa: E731
    for met_pbl in (3, 2):
        ref = C.five("nonfinite", met_pbl, 0, 0)[0]
        base = C.five("levels_era5", met_pbl, 0, 0)[0]
        same = ~C.nonfinite_touched()
        same[8] = same[0]
        for f in ref:
            assert np.array_equal(ref[f][same], base[f][same], equal_nan=True), f      # the other columns are untouched
        assert np.isnan(ref["z"][at("ps_nan")]).all() and np.isnan(ref["z"][at("ps_pinf")]).all()
        assert np.isnan(ref["z"][at("ps_minf")]).all() and np.isnan(ref["z"][at("ps_negative")]).all()
        assert (ref["z"][at("ps_zero")] == -np.inf).all()
        assert ref["o3c"][at("ps_nan")] == 0 and ref["o3c"][at("ps_zero")] == 0 and ref["o3c"][at("ps_pinf")] > 100.
        assert np.isnan(ref["pct"][at("ps_minf")]) and ref["cl"][at("ps_minf")] == 0
        for name in ("ps_nan", "ps_pinf", "ps_minf"):       # a parcel from p[0]; the three loops end in their first pass
            assert ref["cape"][at(name)] == 0 and np.isnan(ref["plcl"][at(name)]) and np.isnan(ref["cin"][at(name)]), name
        for name in ("ps_zero", "ps_negative"):             # no level at or below the surface: no parcel
            assert np.isnan(ref["cape"][at(name)]), name
        # a NaN ts makes pbl NaN (PBL 3) or never meets the Richardson criterion (PBL 2): the lower clamp either way
        assert np.isnan(ref["pbl"][at("ps_nan")])
        assert ref["pbl"][at("ts_nan")] == np.float32(float(met.f2["ps"][at("ts_nan")]) * math.exp(-0.1 / 7.))
        assert np.isnan(ref["z"][at("zs_nan")]).all() and np.isnan(ref["z"][at("t_all_nan")]).all()
        # max(h, 1e-7) = h > 1e-7 ? h : 1e-7 takes a NaN water vapour for the dry floor: z is that of the dry column
        ix, iy = at("h2o_nan")
        dry = R.geopot_column(met.p.tolist(), R._f64(met, "t")[ix][iy], [0.] * met.np, float(met.f2["ps"][ix, iy]),
                              float(met.f2["zs"][ix, iy]))
        assert np.array_equal(ref["z"][ix, iy], np.array(dry, dtype=np.float32)) and np.isfinite(ref["plcl"][ix, iy])
        assert np.isnan(ref["z"][at("h2o_inf")]).all()          # Tv is infinite on every level: the surface's LIN is inf - inf
        # ps ON level 4 with t NaN on level 3: the surface temperature comes from levels 4 and 5
        ix, iy = at("t_nan_below_tie")
        z = ref["z"][ix, iy]
        assert z[4] == met.f2["zs"][ix, iy] and np.isfinite(z[4:]).all() and np.isnan(z[:4]).all()
    sm = C.five("nonfinite", 3, 2, 1)[0]["z"]
    assert np.isnan(sm[6, 5]).all() and np.isfinite(sm[7, 5]).all()      # (7, 5) is NaN itself, (8, 5) is not


def test_natural_spline_through_three_points():
    """np = 3: the system is 2 (h0 + h1) c1 = 3 ((y2 - y1) / h1 - (y1 - y0) / h0), c0 = c2 = 0."""
    zc, y = [5., 11.5, 21.], [250., 212., 221.]
    h0, h1 = zc[1] - zc[0], zc[2] - zc[1]
    c1 = 3 * ((y[2] - y[1]) / h1 - (y[1] - y[0]) / h0) / (2 * (h0 + h1))
    assert T.spline_coeffs(zc, y) == [0., c1, 0.]
    xs = [4.5, 5., 7.25, 11.5, 16., 21., 21.4]
    got = T.spline(zc, y, xs, 1)

    def hand(x):
        if x <= zc[0]:
            return y[0]
        if x >= zc[2]:
            return y[2]
        if x < zc[1]:
            d = x - zc[0]
            return y[0] + d * ((y[1] - y[0]) / h0 - h0 * c1 / 3 + d * d * c1 / (3 * h0))
        d = x - zc[1]
        return y[1] + d * ((y[2] - y[1]) / h1 - 2 * h1 * c1 / 3 + d * (c1 - d * c1 / (3 * h1)))
    for x, g in zip(xs, got):
        assert g == pytest.approx(hand(x), rel=1e-14), x
    assert got[0] == y[0] and got[1] == y[0] and got[-2] == y[2] and got[-1] == y[2] and got[3] == pytest.approx(y[1], rel=1e-15)
    # four points: the back substitution runs once
    zc4, y4 = [5., 9., 14., 22.], [250., 225., 210., 220.]
    c = T.spline_coeffs(zc4, y4)
    h = [4., 5., 8.]
    g0 = 3 * ((y4[2] - y4[1]) / h[1] - (y4[1] - y4[0]) / h[0])
    g1 = 3 * ((y4[3] - y4[2]) / h[2] - (y4[2] - y4[1]) / h[1])
    assert 2 * (h[0] + h[1]) * c[1] + h[1] * c[2] == pytest.approx(g0, rel=1e-13)
    assert h[1] * c[1] + 2 * (h[1] + h[2]) * c[2] == pytest.approx(g1, rel=1e-13)


def test_ieee_helpers():
    inf = math.inf
    assert R._log(0.) == -inf and math.isnan(R._log(-5.)) and R._log(inf) == inf and math.isnan(R._log(-inf)) and math.isnan(R._log(R.NAN))
    assert R._exp(1e4) == inf and R._exp(-inf) == 0. and math.isnan(R._exp(R.NAN))
    assert R._pow(inf, 0.286) == inf and math.isnan(R._pow(-200., 0.286)) and R._pow(-0., 0.286) == 0. and R._pow(1e300, 2.) == inf
    assert R._div(1., 0.) == inf and R._div(-1., 0.) == -inf and R._div(1., -0.) == -inf and math.isnan(R._div(0., 0.))
    assert math.isnan(R._div(R.NAN, 0.)) and R._div(6., 3.) == 2.
    assert R.THETA(0., 280.) == inf and math.isnan(R.THETA(-5., 280.)) and R.THETA(-inf, 280.) == 0.
