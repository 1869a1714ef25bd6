"""The derived meteo fields of mphip_derive_met, restated per column in plain Python from the definitions of
include/mptrac_hip.h (this project's own statement of the reference's preprocessing) -- not from the kernels.  The
`math` module is glibc's exp / log / pow, which the device library reproduces bit for bit, and Python has no fused
multiply-add: what is computed here is what libmptrac_hip_exact.so has to return, bit for bit.

It also builds the input (atmosphere) and, for every column, the smallest relative distance of any comparison between
COMPUTED values from its threshold (Margin): a comparison decided by less than a few ulp may go the other way in the
default library, whose divisions and contractions move a double by an ulp, and the GPU test would then compare different
branches.  Comparisons between input values alone (a level against the surface pressure, a water content against the
cloud threshold, an exact zero) come out the same in any arithmetic and are not recorded in the Margin; where such a
comparison is an EQUALITY -- a tie -- a Ties recorder counts it by name, so that a test can show that its inputs reach it.

Where Python would raise -- the logarithm of a number that is not positive, a division by zero, an exp or pow that
overflows -- the restatement returns what IEEE arithmetic and the C library return (_log, _exp, _pow, _div), so that it is
defined on every float input, a NaN, an infinity or a surface pressure <= 0 included.  Every loop whose end depends on
the arithmetic has a cap (CAP passes) and raises beyond it.
"""
import bisect
import collections
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mptrac_amd.clim import load_clim_tropo     # noqa: E402
from mptrac_amd.synth import Met                # noqa: E402

RI, MA, G0, MO3 = 8.3144598, 28.9644, 9.80665, 48.00
EPS = 18.01528 / MA
RA = 1e3 * RI / MA
CPD, LV, KAPPA, T0 = 1003.5, 2501000., 0.286, 273.15
PFAC = 1.01439
NAN = float("nan")
OUTPUTS_2D = ("o3c", "pbl", "pct", "pcb", "cl", "plcl", "plfc", "pel", "cape", "cin")
DEFAULTS = dict(met_pbl_min=0.1, met_pbl_max=5.0, met_cloud_min=0.0)


CAP = 20000       # passes of a bisection or an ascent: three orders above what any finite input takes


def _log(x):
    if x > 0:
        return math.log(x)
    return -math.inf if x == 0 else NAN


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _pow(x, y):
    try:
        return math.pow(x, y)
    except OverflowError:
        return math.inf
    except ValueError:          # a zero to a negative power; a negative number to a power that is no integer
        return math.inf if x == 0 else NAN


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1., b)


class Ties:
    """Counts, by name, the comparisons between input values that were equalities."""

    def __init__(self):
        self.count = collections.Counter()

    def see(self, name, a, b):
        if a == b:
            self.count[name] += 1


def _tie(ties, name, a, b):
    if ties is not None:
        ties.see(name, a, b)


class Margin:
    """Smallest relative distance of a recorded comparison from equality."""

    def __init__(self):
        self.value = math.inf

    def see(self, a, b):
        if math.isfinite(a) and math.isfinite(b):
            scale = max(abs(a), abs(b))
            self.value = min(self.value, abs(a - b) / scale if scale > 0 else 0.0)


def LIN(x0, y0, x1, y1, x):
    return y0 + _div(y1 - y0, x1 - x0) * (x - x0)


def P(z):
    return 1013.25 * _exp(-z / 7.)


def fmax(a, b):
    return a if a > b else b


def fmin(a, b):
    return a if a < b else b


def THETA(p, t):
    return t * _pow(_div(1000., p), KAPPA)


def TVIRT(t, h):
    return t * (1. + (1. - EPS) * fmax(h, 0.1e-6))


def PSAT(t):
    return 6.112 * _exp(_div(17.62 * (t - T0), 243.12 + t - T0))


def PW(p, h):
    return _div(p * fmax(h, 0.1e-6), 1. + (1. - EPS) * fmax(h, 0.1e-6))


def SH(h):
    return EPS * fmax(h, 0.1e-6)


def lapse_rate(t, h):
    a = RA * (t * t)
    r = _div(SH(h), 1. - SH(h))
    return _div(1e3 * G0 * (a + LV * r * t), CPD * a + LV * LV * r * EPS)


_NEGATED = {}


def loc(p, q):
    """The largest k in [0, np - 2] with p[k] >= q, else 0 (p descending: a bisection in the negated axis)."""
    neg = _NEGATED.get(id(p))
    if neg is None or len(neg) != len(p) - 1 or neg[0] != -p[0]:
        neg = _NEGATED[id(p)] = [-x for x in p[:-1]]
    if q != q:
        return 0
    return max(bisect.bisect_right(neg, -q) - 1, 0)


def loc_computed(p, q, m):
    """loc for a computed q: the nodes next to q decide."""
    k = loc(p, q)
    m.see(p[k], q)
    m.see(p[k + 1], q)
    return k


def env(p, f, q, m):
    k = loc_computed(p, q, m)
    return LIN(p[k], f[k], p[k + 1], f[k + 1], q)


def clim_tropo(clim, t, lat):
    """The climatological tropopause pressure (mphip_update_clim's table): bilinear in the second of the year and latitude."""
    time, lats, tropo = clim[:3]
    year = 365.25 * 86400.
    sec = t - int(t / year) * year
    for _ in range(CAP):
        if not sec < 0:
            break
        sec += year
    else:
        raise RuntimeError("the second of the year does not become positive")
    lo, hi = 0, len(time) - 1
    while hi > lo + 1:
        mid = (hi + lo) >> 1
        if time[mid] > sec:
            hi = mid
        else:
            lo = mid
    il = min(max(int((lat - lats[0]) / (lats[1] - lats[0])), 0), len(lats) - 2)
    pa = LIN(lats[il], tropo[lo][il], lats[il + 1], tropo[lo][il + 1], lat)
    pb = LIN(lats[il], tropo[lo + 1][il], lats[il + 1], tropo[lo + 1][il + 1], lat)
    return LIN(time[lo], pa, time[lo + 1], pb, sec)


# ---- the columns ---------------------------------------------------------------------------------------------------------

def geopot_column(p, t, h2o, ps, zs, ties=None):
    """z[np] in km as doubles (the caller rounds to float once).  An infinite ps is taken as NaN."""
    n = len(p)
    if math.isinf(ps):
        ps = NAN
    tv = [TVIRT(t[k], h2o[k]) for k in range(n)]
    lp = [_log(p[k]) for k in range(n)]
    c = RI / MA / G0

    def ZD(a, ta, b, tb):
        return c * (0.5 * (ta + tb)) * (a - b)
    k0 = loc(p, ps)
    _tie(ties, "loc", p[k0], ps)
    tsurf = LIN(p[k0], tv[k0], p[k0 + 1], tv[k0 + 1], ps)
    lps = _log(ps)
    z = [NAN] * n
    z[k0 + 1] = zs + ZD(lps, tsurf, lp[k0 + 1], tv[k0 + 1])
    for k in range(k0 + 2, n):
        z[k] = z[k - 1] + ZD(lp[k - 1], tv[k - 1], lp[k], tv[k])
    z[k0] = zs + ZD(lps, tsurf, lp[k0], tv[k0])
    for k in range(k0 - 1, -1, -1):
        z[k] = z[k + 1] + ZD(lp[k + 1], tv[k + 1], lp[k], tv[k])
    return z


def smooth(z, lon, sx, sy):
    """Horizontal smoothing of the float field z[nx][ny][np]; all points at once, every point in the order of the
    definition: ix2 outer, iy2 inner, float weights and float sums, one operation at a time."""
    if sx < 0 or sy < 0:
        sx, sy = (3, 2) if abs(lon[1] - lon[0]) < 0.5 else (6, 4)
    if sx == 0 or sy == 0:
        return z.copy()
    nx, ny, _ = z.shape
    f32 = np.float32
    wz = np.zeros(z.shape, dtype=f32)
    ws = np.zeros(z.shape, dtype=f32)
    ix = np.arange(nx)
    iy = np.arange(ny)
    for dx in range(-sx + 1, sx):
        ix2 = ix + dx
        ix2 = np.where(ix2 < 0, ix2 + nx, np.where(ix2 >= nx, ix2 - nx, ix2))
        assert ix2.min() >= 0 and ix2.max() < nx
        wx = f32(1) - f32(abs(dx)) / f32(sx)
        for dy in range(-sy + 1, sy):
            iy2 = iy + dy
            rows = (iy2 >= 0) & (iy2 < ny)
            w = f32(wx * (f32(1) - f32(abs(dy)) / f32(sy)))
            v = z[ix2][:, np.clip(iy2, 0, ny - 1)]
            use = np.isfinite(v) & rows[None, :, None]
            with np.errstate(invalid="ignore", over="ignore"):
                prod = (w * v).astype(f32)
                wz = np.where(use, (wz + prod).astype(f32), wz)
                ws = np.where(use, (ws + w).astype(f32), ws)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ws > 0, (wz / ws).astype(f32), f32(NAN)).astype(f32)


def o3c_column(p, o3, ps, ties=None):
    cd = 0.
    for k in range(1, len(p)):
        _tie(ties, "o3c", p[k - 1], ps)
        if p[k - 1] <= ps:
            cd += 0.5 * (o3[k - 1] + o3[k]) * MO3 / MA * (p[k - 1] - p[k]) * 100. / G0
    return cd / 2.1415e-5


def cloud_column(p, lwc, rwc, iwc, swc, ps, cloud_min, ties=None):
    pct = pcb = NAN
    cl = 0.
    p20 = P(20.)
    for k in range(len(p) - 1):
        _tie(ties, "cloud_ps", p[k], ps)
        if p[k] > ps or p[k] < p20:     # (P(20) lies between levels by construction of the axes: checked by the CPU test)
            continue
        for w in (lwc[k], rwc[k], iwc[k], swc[k]):
            _tie(ties, "cloud_min", w, cloud_min)
        if lwc[k] > cloud_min or rwc[k] > cloud_min or iwc[k] > cloud_min or swc[k] > cloud_min:
            pct = 0.5 * (p[k] + p[k + 1])
            if pcb != pcb:
                pcb = 0.5 * (p[k] + p[max(k - 1, 0)])
        s = ((lwc[k] + lwc[k + 1]) + (rwc[k] + rwc[k + 1])) + (iwc[k] + iwc[k + 1]) + (swc[k] + swc[k + 1])
        cl += 0.5 * s * 100. * (p[k] - p[k + 1]) / G0
    return pct, pcb, cl


def pbl_clamp(ps, pbl, below, pbl_min, pbl_max, m):
    pmin = ps * _exp(-pbl_min / 7.)
    pmax = ps * _exp(-pbl_max / 7.)
    m.see(pbl, pmin)
    if not math.isfinite(pbl) or pbl > pmin or below:
        pbl = pmin
    m.see(pbl, pmax)
    if pbl < pmax:
        pbl = pmax
    return pbl


def pbl3_column(p, t, ps, ts, pbl_min, pbl_max, m, ties=None):
    th0 = THETA(ps, ts)
    k = len(p) - 2
    while k > 0:
        if p[k] >= 300.:
            _tie(ties, "pbl3_ps", p[k], ps)
            if p[k] > ps:
                break
            th = THETA(p[k], t[k])
            m.see(th, th0 + 2.)
            if th <= th0 + 2.:
                _tie(ties, "pbl3_300", p[k], 300.)      # the 300 hPa level itself ends the search
                break
        k -= 1
    pbl = LIN(THETA(p[k + 1], t[k + 1]), p[k + 1], THETA(p[k], t[k]), p[k], th0 + 2.)
    return pbl_clamp(ps, pbl, p[k] > ps, pbl_min, pbl_max, m)


def pbl2_column(p, t, h2o, u, v, z, ps, ts, zs, us, vs, pbl_min, pbl_max, m):
    n = len(p)
    pb = ps * _exp(-0.05 / 7.)
    k = 1
    while k < n - 1:
        m.see(p[k], pb)
        if p[k] < pb:
            break
        k += 1
    h2os = LIN(p[k - 1], h2o[k - 1], p[k], h2o[k], pb)
    tvs = TVIRT(THETA(pb, ts), h2os)
    pbl = pb
    rib_old = 0.
    while k < n:
        du, dv = u[k] - us, v[k] - vs
        vh2 = fmax(du * du + dv * dv, 25.)
        m.see(du * du + dv * dv, 25.)
        rib = _div(_div(G0 * 1e3 * (z[k] - zs), tvs) * (TVIRT(THETA(p[k], t[k]), h2o[k]) - tvs), vh2)
        m.see(rib, 0.25)
        if rib >= 0.25:
            cand = LIN(rib_old, p[k - 1], rib, p[k], 0.25)
            m.see(cand, pb)
            pbl = fmin(cand, pb)
            break
        rib_old = rib
        k += 1
    return pbl_clamp(ps, pbl, False, pbl_min, pbl_max, m)


def cape_column(p, t, h2o, ps, ptropo, m, ties=None):
    """(plcl, plfc, pel, cape, cin).  An infinite ps is taken as NaN."""
    n = len(p)
    if math.isinf(ps):
        ps = NAN
    pbot = fmin(ps, p[0])
    th = h = 0.
    cnt = 0
    for k in range(n):
        _tie(ties, "cape_pbot", p[k], pbot)
        _tie(ties, "cape_50", p[k], pbot - 50.)
        if pbot >= p[k] >= pbot - 50.:
            th += THETA(p[k], t[k])
            h += h2o[k]
            cnt += 1
        elif cnt > 0 and p[k] < pbot - 50.:
            break
    plcl = plfc = pel = cape = cin = NAN
    if cnt == 0:
        return plcl, plfc, pel, cape, cin
    th /= cnt
    h /= cnt
    if h != 0:
        m.see(h, 0.)
    if h <= 0:
        return plcl, plfc, pel, cape, cin
    ptop = P(20.)
    pbot = ps
    for passes in range(CAP + 1):
        if passes == CAP:
            raise RuntimeError("the bisection of the lifted condensation level does not end")
        plcl = 0.5 * (pbot + ptop)
        tp = _div(th, _pow(_div(1000., plcl), KAPPA))
        rh = _div(100. * PW(plcl, h), PSAT(tp))
        m.see(rh, 100.)
        if rh > 100.:
            ptop = plcl
        else:
            pbot = plcl
        m.see(pbot - ptop, 0.1)
        if not pbot - ptop > 0.1:
            break
    dz0 = RI / MA / G0 * math.log(PFAC)
    cape = cin = 0.
    pp = ps
    TV = TVIRT

    def buoyancy(tp, hp, q, dz):
        te, he = env(p, t, q, m), env(p, h2o, q, m)
        m.see(TVIRT(tp, hp), TVIRT(te, he))       # the sign of d
        return _div(1e3 * G0 * (TV(tp, hp) - TV(te, he)), TV(te, he)) * dz
    for passes in range(CAP + 1):
        if passes == CAP:
            raise RuntimeError("the dry ascent does not end")
        dz = dz0 * TVIRT(tp, h)
        pp /= PFAC
        tp = _div(th, _pow(_div(1000., pp), KAPPA))
        d = buoyancy(tp, h, pp, dz)
        if d < 0:
            cin += abs(d)
        m.see(pp, plcl)
        if not pp > plcl:
            break
    d = 0.
    pp = plcl
    tp = _div(th, _pow(_div(1000., pp), KAPPA))
    ptop = 0.75 * ptropo
    for passes in range(CAP + 1):
        if passes == CAP:
            raise RuntimeError("the moist ascent does not end")
        dz = dz0 * TVIRT(tp, h)
        pp /= PFAC
        tp -= lapse_rate(tp, h) * dz
        e = PSAT(tp)
        h = _div(e, pp - (1. - EPS) * e)
        d_old = d
        d = buoyancy(tp, h, pp, dz)
        if d > 0:
            cape += d
            if plfc != plfc:
                plfc = pp
        elif d_old > 0:
            pel = pp
        if d < 0 and plfc != plfc:
            cin += abs(d)
        m.see(pp, ptop)
        if not pp > ptop:
            break
    if plfc != plfc:
        cin = NAN
    return plcl, plfc, pel, cape, cin


# ---- a whole snapshot ------------------------------------------------------------------------------------------------------

def _f64(met, name, three=True):
    src = met.f3 if three else met.f2
    return src[name].astype(np.float64).tolist() if name in src else None


def columns_of(met, met_pbl_min=DEFAULTS["met_pbl_min"], met_pbl_max=DEFAULTS["met_pbl_max"],
               met_cloud_min=DEFAULTS["met_cloud_min"], lat=None, ties=None):
    """Everything but the smoothing and PBL 2 of a snapshot: {name: float32 [nx][ny]}, z raw, margins.  `lat`: the latitude
    of the climatological tropopause in every column (met_utm_ref_lat on a Cartesian grid) instead of the row's."""
    clim = load_clim_tropo()
    p = met.p.tolist()
    nx, ny, n = met.nx, met.ny, met.np
    f = {k: _f64(met, k) for k in ("t", "h2o", "o3", "lwc", "rwc", "iwc", "swc")}
    g = {k: _f64(met, k, False) for k in ("ps", "ts", "zs")}
    zero = [0.] * n
    out = {k: np.empty((nx, ny), dtype=np.float32) for k in OUTPUTS_2D if k != "pbl"}
    out["pbl3"] = np.empty((nx, ny), dtype=np.float32)
    out["z"] = np.empty((nx, ny, n), dtype=np.float32)
    margin = np.empty((nx, ny))
    with np.errstate(over="ignore", invalid="ignore"):
        for ix in range(nx):
            for iy in range(ny):
                m = Margin()
                t, h2o, ps = f["t"][ix][iy], f["h2o"][ix][iy], g["ps"][ix][iy]
                out["z"][ix, iy] = geopot_column(p, t, h2o, ps, g["zs"][ix][iy], ties)
                out["o3c"][ix, iy] = o3c_column(p, f["o3"][ix][iy], ps, ties)
                out["pct"][ix, iy], out["pcb"][ix, iy], out["cl"][ix, iy] = cloud_column(
                    p, f["lwc"][ix][iy], f["rwc"][ix][iy] if f["rwc"] else zero, f["iwc"][ix][iy],
                    f["swc"][ix][iy] if f["swc"] else zero, ps, met_cloud_min, ties)
                out["pbl3"][ix, iy] = pbl3_column(p, t, ps, g["ts"][ix][iy], met_pbl_min, met_pbl_max, m, ties)
                five = cape_column(p, t, h2o, ps, clim_tropo(clim, met.time, met.lat[iy] if lat is None else lat), m, ties)
                for name, val in zip(("plcl", "plfc", "pel", "cape", "cin"), five):
                    out[name][ix, iy] = val
                margin[ix, iy] = m.value
    return out, margin


def reference_of(met, met_pbl=3, sx=-1, sy=-1, met_pbl_min=DEFAULTS["met_pbl_min"], met_pbl_max=DEFAULTS["met_pbl_max"],
                 met_cloud_min=DEFAULTS["met_cloud_min"], lat=None, ties=None, cols=None):
    """({name: float32 array} of all eleven outputs, margin [nx][ny]) of a snapshot; `cols`: columns_of, if at hand."""
    cols, margin = cols or columns_of(met, met_pbl_min, met_pbl_max, met_cloud_min, lat, ties)
    out = {k: v for k, v in cols.items() if k not in ("pbl3", "z")}
    out["z"] = smooth(cols["z"], met.lon, sx, sy)
    if met_pbl == 3:
        out["pbl"] = cols["pbl3"]
        return out, margin
    margin = margin.copy()
    p = met.p.tolist()
    f = {k: _f64(met, k) for k in ("t", "h2o", "u", "v")}
    g = {k: _f64(met, k, False) for k in ("ps", "ts", "zs", "us", "vs")}
    z = out["z"].astype(np.float64).tolist()
    out["pbl"] = np.empty((met.nx, met.ny), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for ix in range(met.nx):
            for iy in range(met.ny):
                m = Margin()
                out["pbl"][ix, iy] = pbl2_column(p, f["t"][ix][iy], f["h2o"][ix][iy], f["u"][ix][iy], f["v"][ix][iy], z[ix][iy],
                                                 g["ps"][ix][iy], g["ts"][ix][iy], g["zs"][ix][iy], g["us"][ix][iy],
                                                 g["vs"][ix][iy], met_pbl_min, met_pbl_max, m)
                margin[ix, iy] = min(margin[ix, iy], m.value)
    return out, margin


@functools.lru_cache(maxsize=None)
def _columns(key, met_pbl_min=DEFAULTS["met_pbl_min"], met_pbl_max=DEFAULTS["met_pbl_max"],
             met_cloud_min=DEFAULTS["met_cloud_min"], lat=None):
    return columns_of(atmosphere(*key), met_pbl_min, met_pbl_max, met_cloud_min, lat)


@functools.lru_cache(maxsize=None)
def reference(key, met_pbl=3, sx=-1, sy=-1, met_pbl_min=DEFAULTS["met_pbl_min"], met_pbl_max=DEFAULTS["met_pbl_max"],
              met_cloud_min=DEFAULTS["met_cloud_min"], lat=None):
    """reference_of for the snapshot atmosphere(*key); the columns are computed once per set of options."""
    return reference_of(atmosphere(*key), met_pbl, sx, sy, met_pbl_min, met_pbl_max, met_cloud_min, lat,
                        cols=_columns(key, met_pbl_min, met_pbl_max, met_cloud_min, lat))


# ---- the input --------------------------------------------------------------------------------------------------------------

SPECIAL = {"dry": 1, "cloud_free": 2, "cloud_top_only": 3}      # flat column indices (ix * ny + iy) of the marked columns


@functools.lru_cache(maxsize=None)
def atmosphere(nx, ny, n, seed=2024, lat_descending=False, time=1.3e7):
    """A physically shaped, seeded snapshot on nx x ny x n nodes (the last longitude column repeats the first, as the
    periodic column of a global file): 6.5 K/km to a tropopause and isothermal above; surface temperature and
    boundary-layer humidity by column, so that some columns have CAPE and an equilibrium level and some have none; ps
    from 1040 hPa (below p[0]) to 600 hPa (mountains, above many levels); an ozone layer; cloud water in a few layers of
    some columns; column 1 without water vapour, column 2 without cloud, column 3 with cloud only in the highest layer the
    cloud search admits."""
    rng = np.random.default_rng(seed + 1000003 * nx + 1009 * ny + n)
    lon = -180. + 360. / (nx - 1) * np.arange(nx)
    lat = np.linspace(-80., 80., ny)
    if lat_descending:
        lat = lat[::-1].copy()
    zlev = 0.013 + (42. / (n - 1)) * np.arange(n)         # km; p[0] = 1011.4 hPa, top near 2.5 hPa; P(20) between levels
    p = 1013.25 * np.exp(-zlev / 7.)
    shape2 = (nx, ny)
    ps = rng.uniform(700., 1040., shape2)
    ps.flat[0] = 1040.
    ps.flat[4::5] = rng.uniform(600., 700., ps.flat[4::5].shape)       # mountains
    ps.flat[5::7] = rng.uniform(1015., 1040., ps.flat[5::7].shape)     # the surface below the lowest level
    zs = np.maximum(7. * np.log(1013.25 / ps), 0.)
    tsfc = rng.uniform(270., 306., shape2)                              # sea-level temperature of the column
    ztrop = rng.uniform(10., 16., shape2)
    q0 = rng.uniform(5e-4, 3e-2, shape2) * (tsfc > 285.) + 3e-4         # warm columns may be moist
    t = tsfc[:, :, None] - 6.5 * np.minimum(zlev[None, None, :], ztrop[:, :, None]) + rng.normal(0., 0.3, shape2 + (n,))
    h2o = np.maximum(q0[:, :, None] * np.exp(-zlev[None, None, :] / 2.), 3e-6) * rng.uniform(0.9, 1.1, shape2 + (n,))
    ts = tsfc - 6.5 * zs + rng.uniform(-1., 3., shape2)
    shear = rng.uniform(0.5, 3., shape2)
    u = 3. + shear[:, :, None] * zlev[None, None, :] + rng.normal(0., 1., shape2 + (n,))
    v = rng.normal(0., 2., shape2 + (n,))
    o3 = 2e-8 + 8e-6 * np.exp(-((zlev[None, None, :] - 25.) / 6.) ** 2) * rng.uniform(0.8, 1.2, shape2)[:, :, None]
    layers = rng.uniform(0., 1., shape2 + (n,)) < 0.15
    cloudy = (rng.uniform(0., 1., shape2) < 0.6)[:, :, None]
    lwc = np.where(layers & cloudy & (zlev < 6.)[None, None, :], rng.uniform(1e-6, 3e-4, shape2 + (n,)), 0.)
    iwc = np.where(layers & cloudy & (zlev > 4.)[None, None, :] & (zlev < 14.)[None, None, :], rng.uniform(1e-7, 5e-5, shape2 + (n,)), 0.)
    rwc = np.where(lwc > 1e-4, 0.3 * lwc, 0.)
    f3 = dict(t=t, h2o=h2o, u=u, v=v, o3=o3, lwc=lwc, iwc=iwc, rwc=rwc)
    f2 = dict(ps=ps, zs=zs, ts=ts, us=rng.normal(2., 1., shape2), vs=rng.normal(0., 1., shape2))
    f3 = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in f3.items()}
    f2 = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in f2.items()}

    def column(c):
        return c // ny, c % ny
    ix, iy = column(SPECIAL["dry"])
    f3["h2o"][ix, iy] = 0.
    ix, iy = column(SPECIAL["cloud_free"])
    for k in ("lwc", "iwc", "rwc"):
        f3[k][ix, iy] = 0.
    ix, iy = column(SPECIAL["cloud_top_only"])
    for k in ("lwc", "iwc", "rwc"):
        f3[k][ix, iy] = 0.
    p20 = P(20.)
    khi = max(k for k in range(n - 1) if p[k] >= p20 and p[k] <= float(f2["ps"][ix, iy]))
    f3["iwc"][ix, iy, khi] = 2e-6
    for d in (f3, f2):
        for a in d.values():
            a[-1] = a[0]
    met = Met(time, lon, lat, p, f3, f2)
    for d in (met.f3, met.f2):
        for a in d.values():
            a.setflags(write=False)
    return met


def strided(met, pad_y=3, pad_p=5):
    """The same snapshot as views into arrays of larger extents: sy = np + 5, sx = (ny + 3) sy, sx2 = ny + 3."""
    sy = met.np + pad_p
    ey = met.ny + pad_y
    f3, f2 = {}, {}
    for k, a in met.f3.items():
        big = np.full((met.nx, ey, sy), -7777., dtype=np.float32)
        big[:, :met.ny, :met.np] = a
        f3[k] = big[:, :met.ny, :met.np]
    for k, a in met.f2.items():
        big = np.full((met.nx, ey), -7777., dtype=np.float32)
        big[:, :met.ny] = a
        f2[k] = big[:, :met.ny]
    view = Met.__new__(Met)
    view.__dict__.update(met.__dict__)
    view.f3, view.f2 = f3, f2
    view.strides = (ey * sy, sy, ey)
    return view
