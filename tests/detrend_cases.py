"""Shapes and inputs of the detrending tests (tests/test_detrend_cpu.py, tests/test_gpu_detrend.py).  Everything is
seeded and small: the largest case has 40 x 21 x 20 points with nine taps each, the largest window 13 x 7 taps.  The
restatement's result of a case is computed once (reference()) and shared."""
import functools

import numpy as np

import refdetrend as R
from refregrid import Snap


def atmosphere(lon, lat, n, seed, fields=R.FIELDS):
    """t near 220 K plus structure, winds of both signs, on the given axes and n levels."""
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    rng = np.random.default_rng(seed)
    x, y = np.deg2rad(lon)[:, None, None], np.deg2rad(lat)[None, :, None]
    k = np.arange(n)[None, None, :]
    shape = (len(lon), len(lat), n)
    base = dict(t=220.0 + 25.0 * np.cos(y) * np.cos(2 * x) - 2.0 * k + 3.0 * rng.standard_normal(shape),
                u=30.0 * np.sin(2 * y) * np.cos(x + 0.3 * k) + 5.0 * rng.standard_normal(shape),
                v=-12.0 * np.sin(3 * x) * np.cos(y) + 4.0 * rng.standard_normal(shape),
                w=0.2 * np.sin(x - y) + 0.05 * rng.standard_normal(shape))
    p = 1000.0 * np.exp(-np.arange(n) * (6.0 / max(n - 1, 1)))
    return Snap(lon, lat, p, {f: np.ascontiguousarray(base[f], dtype=np.float32) for f in fields}, {}, time=3600.0)


def _global15(n, seed, fields=R.FIELDS):
    return atmosphere(np.arange(24) * 15.0, np.linspace(-90.0, 90.0, 13), n, seed, fields)


def _levels(n):
    return lambda: (atmosphere(np.arange(16) * 22.5, np.linspace(-80.0, 80.0, 9), n, 40 + n), 3000.0)


def _nonfinite():
    met = _global15(5, 7)
    met.f3["t"][5, 6, 2] = np.nan
    met.f3["u"][20, 1, 0] = np.inf
    return met, 5200.0


# name: a function that returns (snapshot, met_detrend [km])
CASES = {
    # (a) sy = ny / 2 and sx = nx / 2 in every row (no row next to a pole: there sx is 1)
    "widest": lambda: (atmosphere(np.arange(12) * 30.0, np.linspace(-75.0, 75.0, 7), 3, 1), 20000.0),
    # (b) both poles: sx is 1 at the poles (the DX2DEG zero), nx / 2 next to them, 3 at the equator
    "poles": lambda: (_global15(5, 2), 5200.0),
    # (c) sx = sy = 1 everywhere (the lower limit)
    "narrowest": lambda: (atmosphere(np.arange(40) * 9.0, np.linspace(-90.0, 90.0, 21), 20, 3), 10.0),
    # (d) level counts around the wave size: the lanes of a row are (longitude group, level) pairs, 4 ... 130 of them
    "levels_2": _levels(2), "levels_17": _levels(17), "levels_33": _levels(33), "levels_65": _levels(65),
    # ... and more lanes per row than one workgroup has (5 groups x 65 levels)
    "two_workgroups": lambda: (atmosphere(np.arange(40) * 9.0, np.linspace(-60.0, 60.0, 5), 65, 4), 1500.0),
    # (e) descending latitudes; a longitude axis 0 ... 360 with the periodic extra column
    "descending": lambda: (atmosphere(np.arange(24) * 15.0, np.linspace(90.0, -90.0, 13), 5, 5), 5200.0),
    "extra_column": lambda: (atmosphere(np.arange(25) * 15.0, np.linspace(-90.0, 90.0, 13), 4, 6), 5200.0),
    # (f) a regional grid: the wrap by +-nx applies all the same
    "regional": lambda: (atmosphere(np.linspace(10.0, 30.0, 21), np.linspace(40.0, 50.0, 11), 4, 8), 300.0),
    # (g) one NaN and one +inf cell
    "nonfinite": _nonfinite,
    # (k) the smallest
    "smallest": lambda: (atmosphere(np.arange(9) * 40.0, np.linspace(-80.0, 80.0, 5), 2, 9), 4000.0),
}


def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """{field: (out, background)} of the restatement; computed once, not to be written to."""
    met, scale = case(name)
    res = R.detrend(met, scale)
    for pair in res.values():
        for a in pair:
            a.setflags(write=False)
    return res


def strided(met, pad_y=3, pad_p=5, sentinel=-5555.0):
    """The same snapshot as views into arrays of larger extents (the reference's [EX][EY][EP])."""
    sy = met.np + pad_p
    sx = (met.ny + pad_y) * sy
    f3 = {}
    for k, v in met.f3.items():
        big = np.full((met.nx, met.ny + pad_y, sy), sentinel, dtype=np.float32)
        big[:, :met.ny, :met.np] = v
        f3[k] = big[:, :met.ny, :met.np]
    out = Snap(met.lon, met.lat, met.p, f3, {}, met.time, met.coord_type)
    out.strides = (sx, sy, met.ny + pad_y)
    return out
