"""module_diff_turb's short path above every tropopause (DevMet::strat_skip, diff_turb_strat): the bound restated in
numpy, for tests/test_turb_strat_bound.py and tests/test_gpu_turb_strat.py."""
import numpy as np

YEAR = 365.25 * 86400.0
EDGE = 0.866877899          # tropo_weight's upper edge: weight 0 for p < EDGE * pt (mptrac.c:12748-12770)


def tropo_min(clim):
    """The smallest pressure clim_tropo can return at a latitude in [-90, 90] and a second of the year in [0, YEAR]:
    inside a latitude interval the value lies between the interval's nodes, and in time it is A + s (B - A), linear in
    s -- s in [0, 1] inside the month axis, beyond that where the first and the last interval are continued to the ends
    of the year.  So the minimum sits at a latitude node and at an end of s of some month interval."""
    time, lat, tropo = (np.asarray(a, dtype=np.float64) for a in clim[:3])
    assert lat[0] <= -90.0 and lat[-1] >= 90.0 and np.all(np.diff(time) > 0) and np.all(np.diff(lat) > 0)
    lo = np.inf
    last = len(time) - 2
    for i in range(last + 1):
        w = time[i + 1] - time[i]
        s0 = min(0.0, (0.0 - time[0]) / w) if i == 0 else 0.0
        s1 = max(1.0, (YEAR - time[i]) / w) if i == last else 1.0
        for s in (s0, s1):
            lo = min(lo, float(np.min(tropo[i] + s * (tropo[i + 1] - tropo[i]))))
    return lo


def guard(b):
    """the band every bound of DevMet is lowered by"""
    return b - 1e-6 * abs(b) - 1e-6


def strat_bound(clim):
    """DevMet::strat_skip where the path is on: a particle with 1.01 p below it and a latitude in [-90, 90] has
    tropopause weight 0 at any time"""
    return guard(EDGE * tropo_min(clim))


def steep_pole_clim(clim):
    """The table with steep end cells: the pole nodes at the table's smallest value, their neighbours at 600 hPa.  The
    slope of -200 hPa per degree continues beyond +-90 degrees (locate_reg clamps the index), so a latitude 0.05 degrees
    past a pole -- what one step of the advection can do -- sees a tropopause 10 % below every value inside."""
    time, lat, tropo = (np.array(a, dtype=np.float64) for a in clim[:3])
    lo = float(np.min(tropo))
    tropo[:, 0] = tropo[:, -1] = lo
    tropo[:, 1] = tropo[:, -2] = 600.0
    return (time, lat, tropo) + tuple(clim[3:])
