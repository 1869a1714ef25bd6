"""A plain numpy / Python restatement of the definitions of mphip_ingest_met (include/mptrac_hip.h): decoding of the values a
netCDF file stores (packed shorts or floats, the fill / missing-value mask, the unit scale, the surface pressure from its
logarithm), the re-ordering from the file's [level][y][x] to met_t's [x][y][level], the extrapolation below the lowest valid
level, the pole rows of the winds and the periodic longitude column.

The float steps are float32 operations (numpy's, one IEEE operation each); the double steps are Python floats; exp, cos
and sin are math.exp / math.cos / math.sin, the C library's, as in tests/refdetrend.py.  tests/test_ingest_cpu.py pins
this restatement to the host loops of read_met_nc that are the definition."""
import math

import numpy as np

F32 = np.float32
NAN = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]
ELEVEN = ("t", "u", "v", "w", "h2o", "o3", "lwc", "rwc", "iwc", "swc", "cc")
DECODE, EXTRAPOLATE, POLAR, PERIODIC = 1, 2, 4, 8
ALL = 15


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def decode(a, scale_factor=1.0, add_offset=0.0, fill=0, miss=0, scl=1.0, lnsp=0):
    """One field in file order ([nlev][ny][nx] or [ny][nx], int16 or float32) -> met order ([nx][ny][nlev] or [nx][ny])."""
    with np.errstate(all="ignore"):
        if a.dtype == np.int16:
            prod = a.astype(F32) * F32(scale_factor)
            v = prod + F32(add_offset)
            keep = np.ones(a.shape, dtype=bool)
            if int(fill) != 0:
                keep &= a != np.int16(fill)
            if int(miss) != 0:
                keep &= a != np.int16(miss)
        else:
            assert a.dtype == np.float32
            v = a
            keep = np.ones(a.shape, dtype=bool)
            for special in (F32(fill), F32(miss)):
                if not special == 0:        # (a NaN is not 0, and then differs from every value: it masks nothing)
                    keep &= v != special
        keep &= np.abs(v) < F32(1e14)
        out = np.where(keep, F32(scl) * v, NAN).astype(F32)
    if lnsp:
        flat = out.reshape(-1)
        for i in range(flat.size):
            x = float(flat[i])
            try:
                e = math.exp(x)
            except OverflowError:
                e = math.inf
            with np.errstate(all="ignore"):
                flat[i] = F32(e / 100.)
    return np.ascontiguousarray(out.transpose(*range(out.ndim - 1, -1, -1)))


def extrapolate(f3, np_):
    """In place on the [nx][ny][np] arrays of f3 (a dict by name)."""
    first = next(iter(f3.values()))
    bad = np.zeros(first.shape, dtype=bool)
    for name in ("t", "u", "v", "w"):
        if name in f3:
            bad |= ~np.isfinite(f3[name])
    views = [f3[name].view(np.uint32) for name in ELEVEN if name in f3]
    for i, j in zip(*np.nonzero(bad.any(axis=2))):
        low = int(np.nonzero(bad[i, j])[0].max())
        for u in views:
            u[i, j, :low + 1] = u[i, j, low + 1] if low + 1 < np_ else np.uint32(0)


def polar_acts(lat, coord_type):
    return coord_type == 0 and abs(float(lat[0])) >= 89.999 and abs(float(lat[-1])) >= 89.999


def polar(u, v, lon, lat, nx):
    """In place on u, v [>= nx][ny][np]; nx: the extent without the periodic column."""
    ny, np_ = u.shape[1], u.shape[2]
    for pole, nxt in ((0, 1), (ny - 1, ny - 2)):
        turn = -1.0 if float(lat[pole]) < 0 else 1.0
        c = [math.cos(turn * (float(lon[ix]) * (math.pi / 180.0))) for ix in range(nx)]
        s = [math.sin(turn * (float(lon[ix]) * (math.pi / 180.0))) for ix in range(nx)]
        for k in range(np_):
            mx = my = 0.0
            for ix in range(nx):
                uu, vv = float(u[ix, nxt, k]), float(v[ix, nxt, k])
                mx += (uu * c[ix] - vv * s[ix]) / nx
                my += (uu * s[ix] + vv * c[ix]) / nx
            with np.errstate(all="ignore"):
                for ix in range(nx):
                    u[ix, pole, k] = F32(mx * c[ix] + my * s[ix])
                    v[ix, pole, k] = F32(my * c[ix] - mx * s[ix])


def periodic_acts(lon, coord_type):
    lon = [float(x) for x in lon]
    return coord_type == 0 and abs(lon[-1] - lon[0] + lon[1] - lon[0] - 360) < 0.01


def ingest(raw, lon, lat, p, coord_type, what, f3=None, f2=None):
    """The whole call: raw = {name: (array, options)} (read with DECODE only), f3 / f2 further fields in met order.
    Returns (lon2, f3, f2) with new arrays."""
    o3 = {k: np.array(a, dtype=np.float32) for k, a in (f3 or {}).items()}
    o2 = {k: np.array(a, dtype=np.float32) for k, a in (f2 or {}).items()}
    if what & DECODE:
        for name, (a, opt) in raw.items():
            opt = {k: v for k, v in opt.items() if k != "type"}
            (o3 if a.ndim == 3 else o2)[name] = decode(a, **opt)
    nx, np_ = len(lon), len(p)
    if what & EXTRAPOLATE and any(k in o3 for k in ELEVEN):
        extrapolate({k: a for k, a in o3.items() if k in ELEVEN}, np_)
    if what & POLAR and polar_acts(lat, coord_type) and "u" in o3 and "v" in o3:
        polar(o3["u"], o3["v"], lon, lat, nx)
    lon2 = np.array(lon, dtype=np.float64)
    if what & PERIODIC and periodic_acts(lon, coord_type):
        lon2 = np.append(lon2, float(lon[-1]) + float(lon[1]) - float(lon[0]))
        for d in (o3, o2):
            for k in d:
                d[k] = np.concatenate([d[k], d[k][:1]], axis=0)
    return lon2, o3, o2
