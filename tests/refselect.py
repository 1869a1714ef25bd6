"""Reference of mphip_select_atm: the definition of include/mptrac_hip.h, stated in Python.

A candidate is an external index e with first <= e <= last (last < 0 or last >= np: np - 1) and (e - first) % stride == 0;
it is selected when no given criterion rejects it.  Every test is the negated-or form of the host loops (write_atm_asc,
inside() of output.c) -- a NaN passes:

  time  rejected when time < t0 or time > t1
  z     rejected when Z(p) < z0 or Z(p) > z1
  lon   rejected when lon < lon0 or lon > lon1 (as stored)
  lat   rejected when lat < lat0 or lat > lat1
  near  rejected when dist2(geo2cart(0, near_lon, near_lat), geo2cart(0, lon, lat)) > near_r^2

Z and geo2cart are refanalysis's: per value through Python's math module, that is the C library's log, cos and sin, one
IEEE operation after the other in the order of the host's code -- the decisions are the host loop's."""
import numpy as np

import refanalysis as RA


def candidates(n, stride=1, first=0, last=-1):
    end = n - 1 if last < 0 or last >= n else last
    return range(first, end + 1, stride)


def select(atm, stride=1, first=0, last=-1, time=None, z=None, lon=None, lat=None, near=None):
    """the external indices selected, ascending (int32)"""
    tt, pp, ll, bb = atm["time"].tolist(), atm["p"].tolist(), atm["lon"].tolist(), atm["lat"].tolist()
    centre = RA.geo2cart(0.0, float(near[0]), float(near[1])) if near is not None else None
    out = []
    for e in candidates(len(tt), stride, first, last):
        if time is not None and (tt[e] < time[0] or tt[e] > time[1]):
            continue
        if lon is not None and (ll[e] < lon[0] or ll[e] > lon[1]):
            continue
        if lat is not None and (bb[e] < lat[0] or bb[e] > lat[1]):
            continue
        if z is not None:
            height = RA.Z(pp[e])
            if height < z[0] or height > z[1]:
                continue
        if near is not None:
            x = RA.geo2cart(0.0, ll[e], bb[e])
            s = 0.0
            for k in range(3):      # dist2 of output.c
                s += (centre[k] - x[k]) * (centre[k] - x[k])
            if s > near[2] * near[2]:
                continue
        out.append(e)
    return np.array(out, dtype=np.int32)


def rows(atm, index):
    """what mphip_get_atm has at those indices"""
    out = {k: atm[k][index] for k in ("time", "p", "lon", "lat")}
    out["q"] = atm["q"][:, index]
    return out
