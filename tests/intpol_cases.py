"""Cases of mphip_intpol_met (Simulation.intpol_met), shared by tests/test_intpol_cpu.py and tests/test_gpu_intpol*.py.

A case is a dict: name, m0 / m1 (synth.Met), time / p / lon / lat (float64 [n]) and `nan` (bool [n]: points the call's
not-finite rule answers with NaN -- the oracle is not asked there, its FMOD is undefined for them).

  (a) axis_edges      the edge grids of tests/axis_cases.py: 36 x 19 x 40 (and the periodic column) at lon0 -180 and 0, the
                      even / ladder axes and the first four WARPS; the points are the particles' positions (every node of
                      every axis +- 1 ulp, both ends and beyond, +- 360 degrees); the times cycle through TIME_CYCLE
  (b) nonfinite       surface fields with NaN at 1, 2, 3 and 4 corners of a cell and +inf at one; points in each quadrant
                      and on wx == 0.5, wy == 0.5 exactly; one whole snapshot NaN with times on wt == 0.5 exactly and one
                      ulp either side; a NaN corner in a pressure-level field
  (c) other grids     a regional longitude axis 10 ... 40 with points 0.5 and 20 degrees beyond either end, its Cartesian
                      twin, and the 2 x 2 x 2 grid
  (d) bad_points      NaN / +-inf in each coordinate in turn and |lon| = 2e9: NaN is expected

expected(case, fields) is the oracle's scalar orc_intpol_met_time_3d / _2d per point and field (NaN where `nan`), computed
once per (case, fields) and shared."""
import ctypes as C

import numpy as np

import axis_cases as AX
from mptrac_amd.synth import FIELDS_2D, FIELDS_3D, FIELDS_ML, Met, synthetic_met
from oracle import binding as ob

F3 = tuple(f for f in FIELDS_3D if f not in FIELDS_ML)
F2 = FIELDS_2D
T0, T1 = 0.0, 3600.0
N_AXIS = 4096


def _ulps(x):
    return [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]


def time_cycle(t0=T0, t1=T1):
    """time0, time1, the exact midpoint, one ulp either side of each, and 600 s outside either end"""
    return np.array(_ulps(t0) + _ulps(t1) + _ulps(0.5 * (t0 + t1)) + [min(t0, t1) - 600.0, max(t0, t1) + 600.0])


def cycle(values, n):
    return np.resize(np.asarray(values, dtype=np.float64), n)


def case(name, m0, m1, time, p, lon, lat, nan=None):
    time, p, lon, lat = (np.ascontiguousarray(a, dtype=np.float64) for a in (time, p, lon, lat))
    assert len(time) == len(p) == len(lon) == len(lat)
    return dict(name=name, m0=m0, m1=m1, time=time, p=p, lon=lon, lat=lat,
                nan=np.zeros(len(lon), dtype=bool) if nan is None else np.asarray(nan, dtype=bool))


def fields_of(c):
    """every pressure-level and surface field both snapshots carry: (3-D names, 2-D names)"""
    return (tuple(f for f in F3 if f in c["m0"].f3 and f in c["m1"].f3),
            tuple(f for f in F2 if f in c["m0"].f2 and f in c["m1"].f2))


# ---- (a) ---------------------------------------------------------------------------------------------------------------
AXIS_SETS = [("even", "ladder")] + AX.WARPS[:4]
AXIS_GRIDS = [(lon0, lat, p) for lon0 in AX.LON0 for lat, p in AXIS_SETS]

_cache = {}


def _complete(met, lon0, lat, p, amp):
    """a field the `meteo` case lacks: synth's analytic field on the same (warped) axes"""
    missing = [f for f in F3 + F2 if f not in met.f3 and f not in met.f2]
    if missing:
        full = AX.warp_met(synthetic_met(AX.GRIDS[0], met.time, amp, fields=missing, lon0=lon0), lat, p)
        met.f3.update(full.f3)
        met.f2.update(full.f2)
    return met


def axis_edges(lon0, lat, p):
    key = ("axis", lon0, lat, p)
    if key not in _cache:
        ctl, clim, m0, m1, atm, placed = AX.setup("meteo", AX.GRIDS[0], lon0, lat, p, n=N_AXIS)
        m0, m1 = _complete(m0, lon0, lat, p, 1.0), _complete(m1, lon0, lat, p, 1.25)
        c = case("axis-%g-%s-%s" % (lon0, lat, p), m0, m1, cycle(time_cycle(m0.time, m1.time), N_AXIS), atm["p"], atm["lon"],
                 atm["lat"])
        c["placed"] = placed
        _cache[key] = c
    return _cache[key]


# ---- (b) ---------------------------------------------------------------------------------------------------------------
# cells (ix, iy) of field `ps` of met0 and the corners (dx, dy) that are not finite there
BAD_CELLS = [((4, 4), [(0, 0)], np.nan), ((8, 4), [(0, 0), (1, 1)], np.nan), ((12, 4), [(0, 1), (1, 0), (1, 1)], np.nan),
             ((16, 4), [(0, 0), (0, 1), (1, 0), (1, 1)], np.nan), ((20, 4), [(1, 0)], np.inf)]
BAD_3D = (24, 9, 5)       # node of `t` of met0 that is a NaN
FRACTIONS = [(0.25, 0.25), (0.25, 0.75), (0.75, 0.25), (0.75, 0.75), (0.5, 0.25), (0.5, 0.75), (0.25, 0.5), (0.75, 0.5), (0.5, 0.5)]


def nonfinite():
    if "nonfinite" not in _cache:
        names = ("t", "u", "ps", "pbl", "ts", "zs")
        m0, m1 = synthetic_met("tiny", T0, 1.0, fields=names), synthetic_met("tiny", T1, 1.25, fields=names)
        for (ix, iy), corners, bad in BAD_CELLS:
            for dx, dy in corners:
                m0.f2["ps"][ix + dx, iy + dy] = bad
        m1.f2["pbl"][:] = np.nan          # one whole snapshot NaN: met1 of pbl, met0 of ts
        m0.f2["ts"][:] = np.nan
        m0.f3["t"][BAD_3D] = np.nan
        lon, lat, p = [], [], []
        cells = [cell for cell, _, _ in BAD_CELLS] + [BAD_3D[:2], (BAD_3D[0] - 1, BAD_3D[1] - 1)]
        for ix, iy in cells:
            for fx, fy in FRACTIONS:      # the tiny grid's nodes are whole tens of degrees: the fractions are exact
                lon.append(m0.lon[ix] + fx * (m0.lon[ix + 1] - m0.lon[ix]))
                lat.append(m0.lat[iy] + fy * (m0.lat[iy + 1] - m0.lat[iy]))
                p.append(0.5 * (m0.p[BAD_3D[2]] + m0.p[BAD_3D[2] - (len(p) & 1)]))
        n = len(lon)
        times = _ulps(0.5 * (T0 + T1)) + [T0, T1, 900.0, 2700.0]
        reps = len(times)
        c = case("nonfinite", m0, m1, np.repeat(times, n), np.tile(p, reps), np.tile(lon, reps), np.tile(lat, reps))
        _cache["nonfinite"] = c
    return _cache["nonfinite"]


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def _analytic(time, lon, lat, p, coord_type, amp):
    i = np.arange(len(lon), dtype=np.float64)[:, None, None]
    j = np.arange(len(lat), dtype=np.float64)[None, :, None]
    k = np.arange(len(p), dtype=np.float64)[None, None, :]
    f3 = {"t": 250.0 + amp * (1.5 * i - 0.75 * j + 3.25 * k + 0.125 * i * j), "u": amp * (10.0 + np.sin(i + 2.0 * j) * (k + 1.0))}
    f2 = {"ps": 1000.0 + amp * (i[:, :, 0] - 2.0 * j[:, :, 0]), "pbl": 900.0 - amp * (i[:, :, 0] * j[:, :, 0]) / 7.0}
    return Met(time, lon, lat, p, {a: np.broadcast_to(v, (len(lon), len(lat), len(p))) for a, v in f3.items()},
               {a: np.broadcast_to(v, (len(lon), len(lat))) for a, v in f2.items()}, coord_type)


def regional(coord_type):
    key = ("regional", coord_type)
    if key not in _cache:
        lon_ax, lat_ax = np.arange(10.0, 40.5, 1.0), np.arange(50.0, 19.5, -1.5)
        p_ax = np.array([1000.0, 850.0, 700.0, 500.0, 300.0, 200.0, 100.0, 50.0])
        m0, m1 = (_analytic(t, lon_ax, lat_ax, p_ax, coord_type, a) for t, a in ((T0, 1.0), (T1, 1.5)))
        lon = [9.5, -10.0, 40.5, 60.0, 10.0, 40.0, 25.25, 369.5, 400.5, -349.75] + _ulps(17.0) + list(np.linspace(10.1, 39.9, 41))
        n = len(lon)
        lat = cycle([19.0, 20.0, 50.0, 51.0, 33.3, 47.75, 21.125], n)
        p = cycle([1000.0, 1100.0, 50.0, 20.0, 600.0, 850.0, 123.0], n)
        _cache[key] = case("regional-%d" % coord_type, m0, m1, cycle(time_cycle(), n), p, lon, lat)
    return _cache[key]


def two_cubed():
    if "two" not in _cache:
        lon_ax, lat_ax, p_ax = np.array([0.0, 10.0]), np.array([0.0, 10.0]), np.array([1000.0, 500.0])
        m0, m1 = (_analytic(t, lon_ax, lat_ax, p_ax, 0, a) for t, a in ((T0, 1.0), (T1, 1.5)))
        lon = [0.0, 10.0, 5.0, 2.5, -1.0, 11.0, 361.0, 7.5] + _ulps(10.0)
        n = len(lon)
        _cache["two"] = case("two-cubed", m0, m1, cycle(time_cycle(), n), cycle([1000.0, 500.0, 750.0, 1200.0, 300.0], n), lon,
                             cycle([0.0, 10.0, 5.0, -3.0, 12.0, 7.5], n))
    return _cache["two"]


# ---- (d) ---------------------------------------------------------------------------------------------------------------
def bad_points():
    if "bad" not in _cache:
        names = ("t", "u", "ps", "pbl")
        m0, m1 = synthetic_met("tiny", T0, 1.0, fields=names), synthetic_met("tiny", T1, 1.25, fields=names)
        rows = [(1800.0, 500.0, 10.0, 20.0)]       # (a good point first and last: the lanes beside a refused one)
        for k in range(4):
            for bad in (np.nan, np.inf, -np.inf):
                row = list(rows[0])
                row[k] = bad
                rows.append(tuple(row))
        rows += [(1800.0, 500.0, 2e9, 20.0), (1800.0, 500.0, -2e9, 20.0), (900.0, 300.0, -75.0, -33.0)]
        a = np.array(rows)
        nan = np.ones(len(rows), dtype=bool)
        nan[0] = nan[-1] = False
        _cache["bad"] = case("bad-points", m0, m1, a[:, 0], a[:, 1], a[:, 2], a[:, 3], nan)
    return _cache["bad"]


def small_cases():
    return [nonfinite(), regional(0), regional(1), two_cubed(), bad_points()]


# ---- the oracle's scalar calls -------------------------------------------------------------------------------------------
def orc_met(met):
    m = ob.OrcMet()
    m.time, m.coord_type, m.nx, m.ny, m.np, m.npl = met.time, met.coord_type, met.nx, met.ny, met.np, met.npl
    m.lon, m.lat, m.p = (a.ctypes.data_as(ob._dp) for a in (met.lon, met.lat, met.p))
    for i, k in enumerate(FIELDS_3D):
        m.f3[i] = met.f3[k].ctypes.data_as(ob._fp) if k in met.f3 else None
    for i, k in enumerate(FIELDS_2D):
        m.f2[i] = met.f2[k].ctypes.data_as(ob._fp) if k in met.f2 else None
    return m


def oracle_rows(m0, m1, fields, time, p, lon, lat, nan=None):
    """[nfield][n] of orc_intpol_met_time_3d / _2d, one scalar call per point and field; NaN where `nan`"""
    L = ob.lib()
    o0, o1 = C.byref(orc_met(m0)), C.byref(orc_met(m1))
    n = len(lon)
    time = np.broadcast_to(np.asarray(time, dtype=np.float64), (n,))
    out = np.full((len(fields), n), np.nan)
    v = C.c_double()
    ref = C.byref(v)
    good = np.flatnonzero(~nan) if nan is not None else range(n)
    for k, name in enumerate(fields):
        if name in FIELDS_2D:
            f = FIELDS_2D.index(name)
            for i in good:
                L.orc_intpol_met_time_2d(o0, o1, f, time[i], lon[i], lat[i], ref)
                out[k, i] = v.value
        else:
            f = FIELDS_3D.index(name)
            for i in good:
                L.orc_intpol_met_time_3d(o0, o1, f, time[i], p[i], lon[i], lat[i], ref)
                out[k, i] = v.value
    return out


def expected(c, fields):
    key = ("expected", c["name"], tuple(fields))
    if key not in _cache:
        _cache[key] = oracle_rows(c["m0"], c["m1"], fields, c["time"], c["p"], c["lon"], c["lat"], c["nan"])
    return _cache[key]


def same_bits(a, b):
    """equal as 64-bit patterns, with NaNs in the same places (a NaN's sign and payload are not compared)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def first_difference(got, want, fields):
    na, nb = np.isnan(got), np.isnan(want)
    bad = (na != nb) | (~na & ~nb & (got.view(np.uint64) != want.view(np.uint64)))
    k, i = np.argwhere(bad)[0]
    return "%d values differ; first: field %s point %d: %r != %r" % (np.count_nonzero(bad), fields[k], i, got[k, i], want[k, i])
