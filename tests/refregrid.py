"""Restatement in NumPy of the definitions of mphip_regrid_met (include/mptrac_hip.h): model levels to pressure levels
(ML2PL) and smoothing with down-sampling (SAMPLE).  Written from the definitions alone, with the operations in the
order they name: ML2PL in float64 with one rounding to float32 per value, SAMPLE in float32 throughout (NumPy rounds
every float32 operation on its own, so nothing is contracted).  The bisection is scalar Python per (column, target);
the arithmetic is done on arrays."""
import numpy as np

ML_FIELDS = ("t", "u", "v", "w", "h2o", "o3", "lwc", "rwc", "iwc", "swc", "cc")
PL_FIELDS = ML_FIELDS + ("z", "pv")
TILE = (8, 8, 16)       # kept points per workgroup of the SAMPLE kernel (the refusal for LDS is stated with them)


class Snap:
    """A snapshot: axes (float64) and float32 fields [nx][ny][np] / [nx][ny]; for ML2PL f3["pl"] and np == npl."""

    def __init__(self, lon, lat, p, f3, f2, time=0.0, coord_type=0):
        self.time, self.coord_type = float(time), int(coord_type)
        self.lon, self.lat, self.p = (np.ascontiguousarray(a, dtype=np.float64) for a in (lon, lat, p))
        self.nx, self.ny, self.np = len(self.lon), len(self.lat), len(self.p)
        self.npl = self.np
        self.f3, self.f2 = dict(f3), dict(f2)


# ---- ML2PL ----------------------------------------------------------------------------------------------------------------

def clamp(pl, q):
    n = len(pl)
    if pl[0] > pl[1]:
        if q > pl[0]:
            q = pl[0]
        elif q < pl[n - 1]:
            q = pl[n - 1]
    else:
        if q < pl[0]:
            q = pl[0]
        elif q > pl[n - 1]:
            q = pl[n - 1]
    return q


def locate_irr(pl, q):
    n = len(pl)
    ilo, ihi = 0, n - 1
    i = (ihi + ilo) >> 1
    if pl[i] < pl[i + 1]:
        while ihi > ilo + 1:
            i = (ihi + ilo) >> 1
            if pl[i] > q:
                ihi = i
            else:
                ilo = i
    else:
        while ihi > ilo + 1:
            i = (ihi + ilo) >> 1
            if pl[i] <= q:
                ihi = i
            else:
                ilo = i
    return ilo


def brackets(pl3, met_p):
    """k[nx][ny][met_np] and the clamped q of every (column, target)."""
    nx, ny, n = pl3.shape
    k = np.zeros((nx, ny, len(met_p)), dtype=np.int64)
    q = np.zeros((nx, ny, len(met_p)), dtype=np.float64)
    for ix in range(nx):
        for iy in range(ny):
            pl = [float(v) for v in pl3[ix, iy]]
            for j, target in enumerate(met_p):
                q[ix, iy, j] = clamp(pl, float(target))
                k[ix, iy, j] = locate_irr(pl, q[ix, iy, j])
    return k, q


def ml2pl(met, met_p):
    """The snapshot on the pressure levels met_p; fields that are not among the eleven are left out, the 2-D fields and
    the horizontal axes pass through."""
    met_p = np.asarray(met_p, dtype=np.float64)
    pl = met.f3["pl"].astype(np.float64)
    k, q = brackets(pl, met_p)
    x0, x1 = np.take_along_axis(pl, k, 2), np.take_along_axis(pl, k + 1, 2)
    f3 = {}
    with np.errstate(all="ignore"):
        for name in ML_FIELDS:
            if name in met.f3:
                f = met.f3[name].astype(np.float64)
                y0, y1 = np.take_along_axis(f, k, 2), np.take_along_axis(f, k + 1, 2)
                f3[name] = (y0 + (y1 - y0) / (x1 - x0) * (q - x0)).astype(np.float32)
    return Snap(met.lon, met.lat, met_p, f3, {n: a.copy() for n, a in met.f2.items()}, met.time, met.coord_type)


# ---- SAMPLE ---------------------------------------------------------------------------------------------------------------

def shape(n, d):
    return tuple((a + b - 1) // b for a, b in zip(n, d))


def tile_floats(d, s):
    """Floats of LDS the tile of the SAMPLE kernel takes (the definition's refusal: beyond 64 KB)."""
    h = [(t - 1) * min(dd, 2 * ss - 1) + 2 * ss - 1 for t, dd, ss in zip(TILE, d, s)]
    return h[0] * h[1] * h[2]


def _weight(off, s):
    return np.float32(1) - np.float32(abs(off)) / np.float32(s)


def sample_field(f, d, s):
    """One field, 3-D or 2-D (then d and s have two entries)."""
    f = np.asarray(f, dtype=np.float32)
    two = f.ndim == 2
    if two:
        f, d, s = f[:, :, None], tuple(d) + (1,), tuple(s) + (1,)
    nx, ny, n = f.shape
    ix, iy, ip = (np.arange(0, m, dd) for m, dd in zip(f.shape, d))
    if tuple(s) == (1, 1, 1):
        out = f[np.ix_(ix, iy, ip)].copy()
        return out[:, :, 0] if two else out
    a = np.zeros((len(ix), len(iy), len(ip)), dtype=np.float32)
    ws = np.zeros_like(a)
    with np.errstate(all="ignore"):
        for ox in range(-s[0] + 1, s[0]):
            ix3 = ix + ox
            ix3 = np.where(ix3 < 0, ix3 + nx, np.where(ix3 >= nx, ix3 - nx, ix3))
            wx = _weight(ox, s[0])
            for oy in range(-s[1] + 1, s[1]):
                iy2 = iy + oy
                oky = (iy2 >= 0) & (iy2 <= ny - 1)
                wxy = np.float32(wx * _weight(oy, s[1]))
                for op in range(-s[2] + 1, s[2]):
                    ip2 = ip + op
                    okp = (ip2 >= 0) & (ip2 <= n - 1)
                    w = np.float32(wxy * _weight(op, s[2]))
                    v = f[np.ix_(ix3, np.clip(iy2, 0, ny - 1), np.clip(ip2, 0, n - 1))]
                    ok = oky[None, :, None] & okp[None, None, :] & np.ones((len(ix), 1, 1), dtype=bool)
                    prod = (w * v).astype(np.float32)
                    a = np.where(ok, (a + prod).astype(np.float32), a)
                    ws = np.where(ok, (ws + w).astype(np.float32), ws)
        out = (a / ws).astype(np.float32)
    return out[:, :, 0] if two else out


def sample(met, d=(1, 1, 1), s=(1, 1, 1)):
    f3 = {n: sample_field(a, d, s) for n, a in met.f3.items() if n in PL_FIELDS}
    f2 = {n: sample_field(a, d[:2], s[:2]) for n, a in met.f2.items()}
    return Snap(met.lon[::d[0]], met.lat[::d[1]], met.p[::d[2]], f3, f2, met.time, met.coord_type)


# ---- the distances of the tests ----------------------------------------------------------------------------------------------

def ulp32(x):
    """Spacing of float32 at |x| (elementwise; of the float32 nearest to x)."""
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def ulp_distance(a, b):
    """Distance in float32 steps between finite values (elementwise)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def ml2pl_bound(met, met_p, ref):
    """Per value |got - ref| may reach in libmptrac_hip.so: one float rounding boundary and the forward bound of LIN's
    four double roundings with a fast division and a contracted final sum."""
    pl = met.f3["pl"].astype(np.float64)
    k, _ = brackets(pl, np.asarray(met_p, dtype=np.float64))
    out = {}
    for name, r in ref.f3.items():
        f = np.abs(met.f3[name].astype(np.float64))
        out[name] = ulp32(r) + 16 * 2.0 ** -53 * (np.take_along_axis(f, k, 2) + np.take_along_axis(f, k + 1, 2))
    return out
