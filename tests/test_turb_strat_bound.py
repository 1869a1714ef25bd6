"""The pressure bound of module_diff_turb's short path (DevMet::strat_skip in mptrac_amd/csrc/mphip_api.hip, restated in
tests/turbstrat.py) against a dense scan of the reference's clim_tropo (tests/refmodules.py): over every second-of-year
and every latitude in [-90, 90] the upper edge of the tropopause weight, 0.866877899 x pt, is never below the bound --
and beyond the poles it can be, which is why the path asks for a latitude in [-90, 90]."""
import numpy as np

import refmodules
import turbstrat as TS
from mptrac_amd.clim import load_clim_tropo

CLIM = load_clim_tropo()
REF = refmodules.Ref(None, CLIM, None, None)


def _seconds():
    time = np.asarray(CLIM[0], dtype=np.float64)
    dense = np.linspace(0.0, TS.YEAR, 2931)
    ends = [0.0, np.nextafter(0.0, 1.0), np.nextafter(TS.YEAR, 0.0), TS.YEAR - 1.0, 1.0]
    nodes = np.concatenate([time, np.nextafter(time, -np.inf), np.nextafter(time, np.inf)])
    sec = np.unique(np.concatenate([dense[:-1], ends, nodes]))
    assert sec[0] == 0.0 and sec[-1] < TS.YEAR
    return sec


def _latitudes():
    lat = np.asarray(CLIM[1], dtype=np.float64)
    nodes = np.concatenate([lat, np.nextafter(lat, -np.inf), np.nextafter(lat, np.inf)])
    out = np.unique(np.concatenate([np.linspace(-90.0, 90.0, 1441), nodes]))
    return out[(out >= -90.0) & (out <= 90.0)]


def _edge(sec, lat):
    return TS.EDGE * REF.clim_tropo(sec[:, None], lat[None, :])


def test_the_table_is_the_one_the_bound_was_sized_for():
    time, lat, tropo = CLIM[:3]
    assert len(time) == 12 and len(lat) == 73 and lat[0] == -90.0 and lat[-1] == 90.0
    assert 0.0 < time[0] < 15 * 86400.0 and 348 * 86400.0 < time[-1] < TS.YEAR     # (day 14 ... day 349: both ends extrapolate)
    assert abs(float(np.min(tropo)) - 98.07) < 0.01
    b = TS.strat_bound(CLIM)
    assert 80.0 < b < TS.EDGE * float(np.min(tropo))      # (about 84 hPa: the extrapolated ends lie below the smallest node)


def test_the_edge_of_the_tropopause_weight_is_never_below_the_bound():
    sec, lat = _seconds(), _latitudes()
    assert np.isin(np.asarray(CLIM[0]), sec).all() and np.isin(np.asarray(CLIM[1]), lat).all()
    edge = _edge(sec, lat)
    assert edge.shape == (len(sec), len(lat)) and np.all(np.isfinite(edge))
    bound = TS.strat_bound(CLIM)
    lowest = float(edge.min())
    assert lowest >= bound, (lowest, bound)
    # ... and the bound is no lower than its guard band asks for: the scan contains the place of the minimum (a
    # latitude node at an end of the year), so its smallest value is the unguarded bound up to rounding
    assert abs(lowest - TS.EDGE * TS.tropo_min(CLIM)) <= 1e-12 * lowest, (lowest, TS.EDGE * TS.tropo_min(CLIM))
    # what a particle that passes the device's test `1.01 p < bound` gets: tropopause weight 0 everywhere
    p = np.nextafter(bound / 1.01, 0.0)
    assert p * 1.01 < bound
    assert np.all(REF.tropo_weight(sec[:, None], lat[None, :], p * 1.01) == 0.0)


def test_beyond_the_poles_the_edge_can_be_below_the_bound():
    """locate_reg clamps the latitude index and the interpolation continues the end cell's slope beyond +-90 degrees,
    so "the value lies between the nodes of its interval", which the bound rests on, does not hold there.

    On the shipped table that shows at 91 degrees as a value below both nodes of the end cell at the same second -- not
    as a value below the global bound: the polar cells are nearly flat and far above the tropical minimum (over the year
    the smallest edge is 143.76 hPa at -91 degrees, 143.93 at -90; 232.04 hPa at 91 degrees, 232.28 at 90; the bound is
    84.59 hPa).  Whether the continued slope reaches the bound is a property of the table, and mphip_update_clim takes
    any table: with steep end cells (turbstrat.steep_pole_clim, the table of the device test of the latitude clause)
    the edge at 91 degrees is below the bound at every second, and already 0.05 degrees beyond the pole -- one step of
    the advection -- while inside [-90, 90] it keeps above it."""
    sec, lat = _seconds(), _latitudes()
    for clim, reaches_bound in ((CLIM, False), (TS.steep_pole_clim(CLIM), True)):
        ref = refmodules.Ref(None, clim, None, None)
        bound = TS.strat_bound(clim)
        assert float((TS.EDGE * ref.clim_tropo(sec[:, None], lat[None, :])).min()) >= bound
        for pole, inner in ((-90.0, -87.5), (90.0, 87.5)):
            at = {x: TS.EDGE * ref.clim_tropo(sec, np.full_like(sec, x)) for x in (pole, inner, pole / 90.0 * 91.0, pole / 90.0 * 90.05)}
            beyond = at[pole / 90.0 * 91.0]
            # below both nodes of its interval at some second: the argument behind the bound does not cover 91 degrees
            assert np.any(beyond < np.minimum(at[pole], at[inner])), pole
            print("pole", pole, "smallest edge at 91 degrees", float(beyond.min()), "bound", bound)
            if reaches_bound:
                assert float(beyond.max()) < bound and float(at[pole / 90.0 * 90.05].max()) < bound, pole
    # the shipped table's figures, so that a new table which does reach the bound at 91 degrees is noticed here
    ref = refmodules.Ref(None, CLIM, None, None)
    lowest = [float((TS.EDGE * ref.clim_tropo(sec, np.full_like(sec, x))).min()) for x in (-91.0, 91.0)]
    assert abs(lowest[0] - 143.76) < 0.01 and abs(lowest[1] - 232.04) < 0.01, lowest
