"""Edge snapshots for mphip_derive_met and what the restatement (tests/refmetprep.py, tests/reftropo.py) makes of them:
the inputs of tests/test_metprep_edges_cpu.py and tests/test_gpu_metprep_edges.py.

tests/refmetprep.atmosphere avoids every tie by construction (levels that are no floats, a uniform log-pressure axis from
13 m to 42 km, finite values, default options, a longitude / latitude grid).  The snapshots here keep its physical shape
(shape()) and put it on axes of their own:

  levels_era5  the 37 standard levels (exact floats, uneven), 9 x 7, with ps ON levels, one float ulp beside them, 50 hPa
               above them, below the lowest level, a mountain, the 300 hPa stop of PBL 3, cloud water AT met_cloud_min;
  short_axes   3, 4, 12 ("high start") and 14 ("low top") levels, 5 x 5: both end branches of the spline, its shortest systems;
  tall_axes    600 levels (4, 8 and 16 columns per workgroup) and the level limit of the five older kernels;
  pv_shapes    level counts around the tile of 32, two columns, rows at +-90 degrees, uneven spacing;
  smooth_shapes  the largest tile, half-widths beyond the grid, tile-aligned extents, the automatic fine setting, with
               levels and a column that are NaN;
  cartesian    levels_era5 with coord_type 1 and met_utm_ref_lat = 47.5;
  options      levels_era5 with met_pbl_min / _max = 0.3 / 2.0 and met_cloud_min;
  nonfinite    levels_era5 with ps NaN, +-inf, 0, -5 and NaN / inf in t, h2o, ts, zs, in single columns.

calls(step) lists every library call of the GPU test (step "finite": all inputs finite; step "nonfinite": smooth_shapes
and nonfinite, run last and on its own); expected(call) is the restatement of one call, margin(call) the smallest
distance of a comparison between computed values from equality.
"""
import functools
import math

import numpy as np

import refmetprep as R
import reftropo as T
from mptrac_amd.synth import Met

ERA5 = [1000., 975., 950., 925., 900., 875., 850., 825., 800., 775., 750., 700., 650., 600., 550., 500., 450., 400., 350.,
        300., 250., 225., 200., 175., 150., 125., 100., 70., 50., 30., 20., 10., 7., 5., 3., 2., 1.]
# met_cloud_min of the cases: the float nearest 1e-6, so that a float cloud water can EQUAL it (1e-6 itself is no float)
CLOUD_MIN = float(np.float32(1e-6))
REF_LAT = 47.5
PBL_MIN, PBL_MAX = 0.3, 2.0
FIVE = ("geopot", "o3c", "pbl", "cloud", "cape")
BIT_FIELDS = {"geopot": ("z",), "o3c": ("o3c",), "pbl": ("pbl",), "cloud": ("pct", "pcb", "cl"),
              "cape": ("plcl", "plfc", "pel", "cape", "cin"), "pv": ("pv",), "tropo": ("pt", "tt", "zt", "h2ot")}


def up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def geometric(p0, p1, n):
    return [p0 * (p1 / p0) ** (k / (n - 1)) for k in range(n)]


def shape(nx, ny, p, seed, lon=None, lat=None):
    """The recipe of refmetprep.atmosphere on the pressure axis p (writable float32 fields): 6.5 K/km to a tropopause and
    isothermal above, surface temperature and boundary-layer humidity by column, ps from 1040 to 600 hPa, an ozone layer,
    cloud water in a few layers of some columns, sheared winds."""
    n = len(p)
    rng = np.random.default_rng(seed + 1000003 * nx + 1009 * ny + n)
    lon = -180. + 360. / (nx - 1) * np.arange(nx) if lon is None else np.asarray(lon, dtype=np.float64)
    lat = np.linspace(-80., 80., ny) if lat is None else np.asarray(lat, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    zlev = 7. * np.log(1013.25 / p)
    shape2 = (nx, ny)
    ps = rng.uniform(700., 1040., shape2)
    ps.flat[4::5] = rng.uniform(600., 700., ps.flat[4::5].shape)
    ps.flat[5::7] = rng.uniform(1015., 1040., ps.flat[5::7].shape)
    zs = np.maximum(7. * np.log(1013.25 / ps), 0.)
    tsfc = rng.uniform(270., 306., shape2)
    ztrop = rng.uniform(10., 16., shape2)
    q0 = rng.uniform(5e-4, 3e-2, shape2) * (tsfc > 285.) + 3e-4
    t = tsfc[:, :, None] - 6.5 * np.minimum(zlev[None, None, :], ztrop[:, :, None]) + rng.normal(0., 0.3, shape2 + (n,))
    h2o = np.maximum(q0[:, :, None] * np.exp(-zlev[None, None, :] / 2.), 3e-6) * rng.uniform(0.9, 1.1, shape2 + (n,))
    ts = tsfc - 6.5 * zs + rng.uniform(-1., 3., shape2)
    shear = rng.uniform(0.5, 3., shape2)
    u = 3. + shear[:, :, None] * zlev[None, None, :] + rng.normal(0., 1., shape2 + (n,))
    v = rng.normal(0., 2., shape2 + (n,))
    o3 = 2e-8 + 8e-6 * np.exp(-((zlev[None, None, :] - 25.) / 6.) ** 2) * rng.uniform(0.8, 1.2, shape2)[:, :, None]
    layers = rng.uniform(0., 1., shape2 + (n,)) < 0.15
    cloudy = (rng.uniform(0., 1., shape2) < 0.6)[:, :, None]
    lwc = np.where(layers & cloudy & (zlev < 6.)[None, None, :], rng.uniform(2e-6, 3e-4, shape2 + (n,)), 0.)
    iwc = np.where(layers & cloudy & (zlev > 4.)[None, None, :] & (zlev < 14.)[None, None, :],
                   rng.uniform(1e-7, 5e-5, shape2 + (n,)), 0.)
    rwc = np.where(lwc > 1e-4, 0.3 * lwc, 0.)
    f3 = dict(t=t, h2o=h2o, u=u, v=v, o3=o3, lwc=lwc, iwc=iwc, rwc=rwc)
    f2 = dict(ps=ps, zs=zs, ts=ts, us=rng.normal(2., 1., shape2), vs=rng.normal(0., 1., shape2))
    f3 = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in f3.items()}
    f2 = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in f2.items()}
    return lon, lat, p, f3, f2


def finish(lon, lat, p, f3, f2, periodic=True, coord_type=0, time=1.3e7):
    if periodic:
        for d in (f3, f2):
            for a in d.values():
                a[-1] = a[0]
    met = Met(time, lon, lat, p, f3, f2, coord_type)
    for d in (met.f3, met.f2):
        for a in d.values():
            a.setflags(write=False)
    return met


# ---- levels_era5 -----------------------------------------------------------------------------------------------------------

# flat column indices (ix * 7 + iy; all in ix = 1 ... 3, `deep` on the equator row iy = 3: none is the periodic column or its source)
ERA5_COLUMNS = dict(ps_lowest=8, ps_interior=9, above_lowest=10, below_lowest=11, above_interior=12, below_interior=13,
                    ps_below_axis=15, mountain=16, stop_300=18, cloud_at_min=20, cloud_above_min=21, deep=24)
ERA5_SEED = 2025


def _era5_fields(seed=ERA5_SEED):
    lon, lat, p, f3, f2 = shape(9, 7, ERA5, seed)
    ps, ts = f2["ps"], f2["ts"]

    def at(name):
        c = ERA5_COLUMNS[name]
        return c // 7, c % 7
    ps[at("ps_lowest")] = 1000.          # == p[0]; ps - 50 == p[2]
    ps[at("ps_interior")] = 900.         # == p[4]; ps - 50 == p[6]
    ps[at("above_lowest")] = up(1000.)
    ps[at("below_lowest")] = down(1000.)
    ps[at("above_interior")] = up(900.)
    ps[at("below_interior")] = down(900.)
    ps[at("ps_below_axis")] = 1040.
    ps[at("mountain")] = 600.            # == p[13]; ps - 50 == p[14]
    # PBL 3 walks down from the top; a cold ts keeps THETA(p[k], t[k]) <= th0 + 2 false all the way, so that the level ON
    # the surface is visited and only `p[k] > ps` (one level further down) ends the search
    ts[at("ps_interior")] = 200.
    ts[at("mountain")] = 200.
    # ... and a surface whose th0 + 2 lies 0.25 K above THETA of the 300 hPa level, the first level the search admits: it
    # ends there, and above the clamp at ps exp(-5/7) = 274 hPa
    ix, iy = at("stop_300")
    ps[ix, iy] = 560.
    k300 = ERA5.index(300.)
    ts[ix, iy] = (R.THETA(300., float(f3["t"][ix, iy, k300])) - 1.75) / math.pow(1000. / 560., R.KAPPA)
    # cloud water AT the threshold in one layer (no cloud), one float ulp above it in another column (a cloud)
    for name, w in (("cloud_at_min", np.float32(CLOUD_MIN)), ("cloud_above_min", up(CLOUD_MIN))):
        ix, iy = at(name)
        for f in ("lwc", "iwc", "rwc"):
            f3[f][ix, iy] = 0.
        ps[ix, iy] = 990.5
        f3["lwc"][ix, iy, 5] = w
    # a hot, moist column on the equator row, unstable to 16 km: its parcel is still buoyant at three quarters of the
    # tropopause pressure of 47.5 degrees, so that cape and pel depend on the latitude the tropopause is taken at
    ix, iy = at("deep")
    zlev = 7. * np.log(1013.25 / p)
    ps[ix, iy] = 1005.
    f3["t"][ix, iy] = 303. - 7.5 * np.minimum(zlev, 16.)
    f3["h2o"][ix, iy] = np.maximum(0.03 * np.exp(-zlev / 2.), 3e-6)
    ts[ix, iy] = 304.
    f2["zs"][:] = np.maximum(7. * np.log(1013.25 / ps.astype(np.float64)), 0.)
    return lon, lat, p, f3, f2


@functools.lru_cache(maxsize=None)
def levels_era5(coord_type=0):
    return finish(*_era5_fields(), coord_type=coord_type)


# ---- nonfinite ---------------------------------------------------------------------------------------------------------------

NONFINITE_COLUMNS = dict(ps_nan=28, ps_pinf=29, ps_minf=30, ps_zero=31, ps_negative=32, t_nan_below_tie=33, t_nan_mid=34,
                         t_all_nan=35, h2o_nan=36, h2o_inf=37, ts_nan=38, zs_nan=42)
NONFINITE_BLOCK = [(ix, iy) for ix in (5, 6, 7) for iy in (4, 5, 6)]      # ps NaN: (6, 5) has no finite neighbour with sy = 1


@functools.lru_cache(maxsize=None)
def nonfinite():
    lon, lat, p, f3, f2 = _era5_fields()
    nan, inf = np.float32(np.nan), np.float32(np.inf)

    def at(name):
        c = NONFINITE_COLUMNS[name]
        return c // 7, c % 7
    for name, v in (("ps_nan", nan), ("ps_pinf", inf), ("ps_minf", -inf), ("ps_zero", 0.), ("ps_negative", -5.)):
        f2["ps"][at(name)] = v
    # ps ON the level p[4] and a NaN in t one level below: loc(ps) = 4 keeps the NaN out of the surface temperature (LIN
    # over levels 4 and 5), loc = 3 would take it in
    ix, iy = at("t_nan_below_tie")
    f2["ps"][ix, iy] = 900.
    f3["t"][ix, iy, 3] = nan
    ix, iy = at("t_nan_mid")
    f3["t"][ix, iy, 15] = nan
    f3["t"][at("t_all_nan")] = nan
    f3["h2o"][at("h2o_nan")] = nan
    f3["h2o"][at("h2o_inf")] = inf
    f2["ts"][at("ts_nan")] = nan
    f2["zs"][at("zs_nan")] = nan
    for ix, iy in NONFINITE_BLOCK:
        f2["ps"][ix, iy] = nan
    assert not {ix * 7 + iy for ix, iy in NONFINITE_BLOCK} & (set(NONFINITE_COLUMNS.values()) | set(ERA5_COLUMNS.values()))
    assert not set(NONFINITE_COLUMNS.values()) & set(ERA5_COLUMNS.values())
    return finish(lon, lat, p, f3, f2)


def nonfinite_touched():
    """[nx][ny] bool: the columns nonfinite() changes against levels_era5()."""
    m = np.zeros((9, 7), dtype=bool)
    for c in NONFINITE_COLUMNS.values():
        m[c // 7, c % 7] = True
    for ix, iy in NONFINITE_BLOCK:
        m[ix, iy] = True
    return m


# ---- short, tall, pv and smoothing shapes --------------------------------------------------------------------------------

SHORT_AXES = {"np3": [500., 200., 50.], "np4": [500., 250., 120., 40.], "high_start": geometric(400., 30., 12),
              "low_top": geometric(1000., 120., 14)}


@functools.lru_cache(maxsize=None)
def short_axis(name, seed=7):
    return finish(*shape(5, 5, SHORT_AXES[name], seed))


def level_limit(nf=5):
    """The largest np with 16 np + 4 nf (np | 1) <= 65536: two doubles per level and nf float planes of one column at a
    pitch of np | 1 within 64 KB (columns_per_workgroup as mphip_derive_met calls it; nf = 5: met_pbl 2, the most any of
    the five older kernels stages)."""
    n = 2
    while 16 * (n + 1) + 4 * nf * ((n + 1) | 1) <= 65536:
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def tall_axis(nx, ny, n, seed=11):
    return finish(*shape(nx, ny, geometric(1000., 1., n), seed))


PV_SHAPES = [(2, 5, 2), (3, 5, 3), (9, 6, 32), (8, 8, 33), (16, 9, 64)]


@functools.lru_cache(maxsize=None)
def pv_shape(nx, ny, n, descending=False, uneven=False, seed=13):
    lat = np.linspace(-90., 90., ny)
    lon = -180. + 360. / (nx - 1) * np.arange(nx)
    if uneven:
        rng = np.random.default_rng(seed)
        lon = -170. + np.cumsum(rng.uniform(5., 60., nx))
        lat = -85. + np.cumsum(rng.uniform(8., 24., ny))
        assert lat[-1] < 90. and np.all(np.diff(lon) > 0) and np.all(np.diff(lat) > 0)
    if descending:
        lat = lat[::-1].copy()
    p = geometric(1000., 10., n) if n > 3 else [900., 500., 200.][:n]
    return finish(*shape(nx, ny, p, seed, lon, lat), periodic=False)


# (nx, ny, np, [(sx, sy) ...], lon spacing or None)
SMOOTH_SHAPES = [(12, 5, 17, [(13, 13), (13, 1), (1, 13)], None), (8, 8, 16, [(3, 2)], None), (16, 8, 17, [(3, 2)], None),
                 (9, 7, 20, [(-1, -1)], 0.25)]
SMOOTH_REFUSED = [(12, 5, 17, 13, 14), (12, 5, 17, 14, 1)]      # a tile beyond 64 KB; sx - 1 > nx


@functools.lru_cache(maxsize=None)
def smooth_shape(nx, ny, n, dlon=None, seed=17):
    """t is NaN on the level below the top in every column -- z is NaN from there up, so those levels have no finite
    neighbour anywhere -- and ps is NaN in column (2, 2), which the finite levels of its neighbours skip."""
    lon = None if dlon is None else 10. + dlon * np.arange(nx)
    lon, lat, p, f3, f2 = shape(nx, ny, geometric(1000., 5., n), seed, lon)
    f3["t"][:, :, n - 2] = np.nan
    f2["ps"][2, 2] = np.nan
    return finish(lon, lat, p, f3, f2, periodic=False)


SNAPSHOTS = {"levels_era5": levels_era5, "cartesian": lambda: levels_era5(1), "nonfinite": nonfinite}
for _name in SHORT_AXES:
    SNAPSHOTS["short_" + _name] = functools.partial(short_axis, _name)
SNAPSHOTS["tall_600"] = functools.partial(tall_axis, 7, 3, 600)
SNAPSHOTS["tall_limit"] = lambda: tall_axis(3, 2, level_limit())
SNAPSHOTS["tall_beyond"] = lambda: tall_axis(3, 2, level_limit() + 1)
for _g in PV_SHAPES:
    SNAPSHOTS["pv_%dx%dx%d" % _g] = functools.partial(pv_shape, *_g)
    SNAPSHOTS["pv_%dx%dx%d_desc" % _g] = functools.partial(pv_shape, *_g, descending=True)
SNAPSHOTS["pv_uneven"] = functools.partial(pv_shape, 9, 7, 20, uneven=True)
for _nx, _ny, _n, _, _dlon in SMOOTH_SHAPES:
    SNAPSHOTS["smooth_%dx%dx%d" % (_nx, _ny, _n)] = functools.partial(smooth_shape, _nx, _ny, _n, _dlon)


def snapshot(name):
    return SNAPSHOTS[name]()


# ---- the restatement of a snapshot ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def columns(name, pbl_min=0.1, pbl_max=5.0, cloud_min=0.0, lat=None):
    """(refmetprep.columns_of, the Ties it counted)"""
    ties = R.Ties()
    return R.columns_of(snapshot(name), pbl_min, pbl_max, cloud_min, lat, ties), ties


@functools.lru_cache(maxsize=None)
def five(name, met_pbl=3, sx=-1, sy=-1, pbl_min=0.1, pbl_max=5.0, cloud_min=0.0, lat=None):
    return R.reference_of(snapshot(name), met_pbl, sx, sy, pbl_min, pbl_max, cloud_min, lat,
                          cols=columns(name, pbl_min, pbl_max, cloud_min, lat)[0])


@functools.lru_cache(maxsize=None)
def z_given(name):
    """The restatement's float geopotential height (smoothing automatic): what TROPO is given as z."""
    z = five(name)[0]["z"].copy()
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def pv_given(name):
    """(pv float32, S) of the restatement."""
    met = snapshot(name)
    with np.errstate(invalid="ignore", over="ignore"):
        pv, S = T.pv_field(met.lon.tolist(), met.lat.tolist(), met.p.tolist(), R._f64(met, "t"), R._f64(met, "u"), R._f64(met, "v"))
    pv.setflags(write=False)
    return pv, S


@functools.lru_cache(maxsize=None)
def tropo(name, mode, method=1, lat=None):
    """((fields, margin), the Ties of the spline's end branches)"""
    ties = R.Ties()
    met = snapshot(name)
    pv = pv_given(name)[0] if mode == 5 else None
    with np.errstate(invalid="ignore", over="ignore"):
        return T.tropo_of(met, z_given(name), pv, mode, method, lat=lat, ties=ties), ties


def given(name, pv=True):
    """The snapshot with the restatement's z and pv as input fields."""
    met = snapshot(name)
    view = Met.__new__(Met)
    view.__dict__.update(met.__dict__)
    view.f3 = dict(met.f3, z=z_given(name))
    if pv:
        view.f3["pv"] = pv_given(name)[0]
    return view


# ---- the calls of the GPU test -------------------------------------------------------------------------------------------------

def _call(family, met, what, strided=False, given=False, ref_lat=None, refused=None, **opts):
    what = (what,) if isinstance(what, str) else tuple(what)
    tag = "_".join("%s%s" % (k.replace("met_", ""), v) for k, v in sorted(opts.items()))
    cid = "|".join((family, met, "+".join(what), tag, "strided" if strided else "compact"))
    return dict(id=cid, family=family, met=met, what=what, strided=strided, given=given, ref_lat=ref_lat, refused=refused,
                opts=opts)


def calls(step):
    out = []
    if step == "finite":
        for strided in (False, True):
            for met_pbl in (3, 2):
                out.append(_call("levels_era5", "levels_era5", FIVE, strided, met_pbl=met_pbl, met_cloud_min=CLOUD_MIN))
            out.append(_call("levels_era5", "levels_era5", "pv", strided, given=True))
            for mode in (2, 3, 4, 5):
                out.append(_call("levels_era5", "levels_era5", "tropo", strided, given=True, met_tropo=mode))
        for name in SHORT_AXES:
            for mode in (2, 3, 4, 5):
                for method in (0, 1):
                    out.append(_call("short_axes", "short_" + name, "tropo", given=True, met_tropo=mode, met_tropo_spline=method))
        for met_pbl in (3, 2):
            out.append(_call("tall_axes", "tall_600", FIVE, met_pbl=met_pbl))
        # (three columns: the automatic half-width of 6 does not fit)
        out.append(_call("tall_axes", "tall_limit", FIVE, met_pbl=2, met_geopot_sx=2, met_geopot_sy=1))
        out.append(_call("tall_axes", "tall_beyond", FIVE, met_pbl=2, met_geopot_sx=2, met_geopot_sy=1,
                         refused="too many pressure levels"))
        for name in SNAPSHOTS:
            if name.startswith("pv_"):
                for strided in (False, True):
                    out.append(_call("pv_shapes", name, "pv", strided))
        out.append(_call("cartesian", "cartesian", ("cape", "tropo"), given=True, ref_lat=REF_LAT, met_tropo=1))
        for met_pbl in (3, 2):
            out.append(_call("options", "levels_era5", FIVE, met_pbl=met_pbl, met_pbl_min=PBL_MIN, met_pbl_max=PBL_MAX,
                             met_cloud_min=CLOUD_MIN))
    elif step == "nonfinite":
        for nx, ny, n, widths, _ in SMOOTH_SHAPES:
            for sx, sy in widths:
                out.append(_call("smooth_shapes", "smooth_%dx%dx%d" % (nx, ny, n), "geopot", met_geopot_sx=sx, met_geopot_sy=sy))
        for nx, ny, n, sx, sy in SMOOTH_REFUSED:
            out.append(_call("smooth_shapes", "smooth_%dx%dx%d" % (nx, ny, n), "geopot", met_geopot_sx=sx, met_geopot_sy=sy,
                             refused="smoothing half-widths too large"))
        for met_pbl in (3, 2):
            for sx, sy in ((2, 1), (0, 0)):
                out.append(_call("nonfinite", "nonfinite", FIVE, met_pbl=met_pbl, met_geopot_sx=sx, met_geopot_sy=sy))
        out.append(_call("nonfinite", "nonfinite", "pv", given=True))
        for mode in (2, 3, 4, 5):
            out.append(_call("nonfinite", "nonfinite", "tropo", given=True, met_tropo=mode))
    else:
        raise ValueError(step)
    assert len({c["id"] for c in out}) == len(out)
    return out


def _five_args(call):
    o = call["opts"]
    return (call["met"], o.get("met_pbl", 3), o.get("met_geopot_sx", -1), o.get("met_geopot_sy", -1), o.get("met_pbl_min", 0.1),
            o.get("met_pbl_max", 5.0), o.get("met_cloud_min", 0.0), call["ref_lat"])


def expected(call):
    """{field: float32 array} of the call's outputs (and "S", the size of pv's terms, with PV)."""
    out = {}
    bits = [b for b in call["what"] if b in FIVE]
    if bits:
        ref, _ = five(*_five_args(call))
        for b in bits:
            for f in BIT_FIELDS[b]:
                out[f] = ref[f]
    if "pv" in call["what"]:
        out["pv"], out["S"] = pv_given(call["met"])
    if "tropo" in call["what"]:
        o = call["opts"]
        (ref, _), _ = tropo(call["met"], o.get("met_tropo", 3), o.get("met_tropo_spline", 1), call["ref_lat"])
        out.update(ref)
    return out


def margin(call):
    """The smallest distance from equality of a comparison between computed values, over all columns of the call."""
    worst = math.inf
    if any(b in FIVE for b in call["what"]):
        worst = min(worst, float(five(*_five_args(call))[1].min()))
    if "tropo" in call["what"]:
        o = call["opts"]
        worst = min(worst, float(tropo(call["met"], o.get("met_tropo", 3), o.get("met_tropo_spline", 1), call["ref_lat"])[0][1].min()))
    return worst
