"""NumPy restatement of mphip_detrend_met, written from the definition in include/mptrac_hip.h (not from the kernel):
the half-widths and the weights in double with the C library's functions (math.cos / sin / exp), the stencil as plain loops
over the taps in np.float32 arithmetic in the stated order -- the loops run over the taps, every point of a row takes the
same tap at the same time (the points are independent of each other)."""
import math

import numpy as np

RE = 6367.421
FIELDS = ("t", "u", "v", "w")


def RAD(x):
    return x * (math.pi / 180.0)


def DX2DEG(dx, lat):
    if lat < -89.999 or lat > 89.999:
        return 0.0
    return dx * 180. / (math.pi * RE * math.cos(RAD(lat)))


def DY2DEG(dy):
    return dy * 180. / (math.pi * RE)


def geo2cart(z, lon, lat):
    r = RE + z
    return (r * math.cos(RAD(lat)) * math.cos(RAD(lon)), r * math.cos(RAD(lat)) * math.sin(RAD(lon)), r * math.sin(RAD(lat)))


def DIST2(a, b):
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2])


def _limited(v, hi):
    s = hi if not (v < hi) else int(v)
    return max(s, 1)


def half_widths(lon, lat, met_detrend):
    """sy and the list sx(iy)."""
    nx, ny = len(lon), len(lat)
    sigma = met_detrend / 2.355
    dlon, dlat = abs(float(lon[1]) - float(lon[0])), abs(float(lat[1]) - float(lat[0]))
    sy = _limited(3. * DY2DEG(sigma) / dlat, ny // 2)
    sx = [_limited(3. * DX2DEG(sigma, float(lat[iy])) / dlon, nx // 2) for iy in range(ny)]
    return sy, sx


def weight(lat, dlon, tssq, iy, iy2, d):
    """w(iy, iy2, d) as a float64 (the stencil takes np.float32 of it)."""
    d2 = DIST2(geo2cart(0.0, 0.0, float(lat[iy])), geo2cart(0.0, d * dlon, float(lat[iy2])))
    return math.exp(-d2 / tssq)


def taps(lon, lat, met_detrend):
    """Number of taps of a point of each row."""
    sy, sx = half_widths(lon, lat, met_detrend)
    ny = len(lat)
    return [(2 * sx[iy] + 1) * (min(iy + sy, ny - 1) - max(iy - sy, 0) + 1) for iy in range(ny)]


def detrend(met, met_detrend, fields=None):
    """{name: (out, background)} for the fields of t, u, v, w the snapshot has (or `fields`): float32 arrays."""
    lon, lat = met.lon, met.lat
    nx, ny = len(lon), len(lat)
    sigma = met_detrend / 2.355
    tssq = 2. * sigma * sigma
    dlon = abs(float(lon[1]) - float(lon[0]))
    sy, sx = half_widths(lon, lat, met_detrend)
    names = [f for f in (FIELDS if fields is None else fields) if f in met.f3]
    res = {f: (np.empty((nx, ny, met.f3[f].shape[2]), dtype=np.float32), np.empty((nx, ny, met.f3[f].shape[2]), dtype=np.float32))
           for f in names}
    ix = np.arange(nx)
    with np.errstate(all="ignore"):
        for iy in range(ny):
            lo, hi = max(iy - sy, 0), min(iy + sy, ny - 1)
            w = {(iy2, d): np.float32(weight(lat, dlon, tssq, iy, iy2, d)) for iy2 in range(lo, hi + 1) for d in range(sx[iy] + 1)}
            b = {f: np.zeros((nx, met.f3[f].shape[2]), dtype=np.float32) for f in names}
            ws = np.float32(0.0)
            for off in range(-sx[iy], sx[iy] + 1):            # ix2 = ix + off, the outer loop
                ix3 = ix + off
                ix3 = np.where(ix3 < 0, ix3 + nx, np.where(ix3 >= nx, ix3 - nx, ix3))
                for iy2 in range(lo, hi + 1):                 # the inner loop
                    wt = w[(iy2, abs(off))]
                    ws = np.float32(ws + wt)
                    for f in names:
                        prod = (wt * met.f3[f][ix3, iy2, :]).astype(np.float32)
                        b[f] = (b[f] + prod).astype(np.float32)
            for f in names:
                bg = (b[f] / ws).astype(np.float32)
                res[f][1][:, iy, :] = bg
                res[f][0][:, iy, :] = (met.f3[f][:, iy, :] - bg).astype(np.float32)
    return res


def dense64(met, met_detrend, field):
    """The same formula in float64 throughout (weights not rounded to float): (out, sum of w |f| / ws) per point."""
    lon, lat = met.lon, met.lat
    nx, ny = len(lon), len(lat)
    sigma = met_detrend / 2.355
    tssq = 2. * sigma * sigma
    dlon = abs(float(lon[1]) - float(lon[0]))
    sy, sx = half_widths(lon, lat, met_detrend)
    f = met.f3[field].astype(np.float64)
    out, mag = np.empty_like(f), np.empty_like(f)
    ix = np.arange(nx)
    for iy in range(ny):
        lo, hi = max(iy - sy, 0), min(iy + sy, ny - 1)
        b = np.zeros((nx, f.shape[2]))
        a = np.zeros((nx, f.shape[2]))
        ws = 0.0
        for off in range(-sx[iy], sx[iy] + 1):
            ix3 = (ix + off) % nx               # (|off| <= nx / 2: the single wrap)
            for iy2 in range(lo, hi + 1):
                wt = float(np.float32(weight(lat, dlon, tssq, iy, iy2, abs(off))))
                ws += wt
                b += wt * f[ix3, iy2, :]
                a += wt * np.abs(f[ix3, iy2, :])
        out[:, iy, :] = f[:, iy, :] - b / ws
        mag[:, iy, :] = a / ws
    return out, mag
