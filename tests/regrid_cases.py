"""Shapes and inputs of the regridding tests (tests/test_regrid_cpu.py, tests/test_gpu_regrid.py): model-level
snapshots for ML2PL, pressure-level snapshots for SAMPLE, target axes, and the lists of cases.  Everything is seeded and
small: the largest ML2PL case has 72 columns of 137 levels, the largest SAMPLE case 19 x 11 x 20 points."""
import numpy as np

import refregrid as R

ML_GRIDS = [(5, 3), (9, 8)]                 # less than one workgroup's columns; 72 columns: a full block and a partial one
ML_LEVELS = [2, 7, 137]
ML_TARGETS = [2, 5, 60]
SURFACE = ("ps", "zs", "ts")


def ml_atmosphere(nx, ny, npl, seed=11, ascending=False, fields=R.ML_FIELDS):
    """Model levels from the surface (k = 0) to ~1 hPa over a smooth surface pressure; strictly monotone in float32."""
    rng = np.random.default_rng(seed + 1000 * nx + 10 * ny + npl)
    lon = np.linspace(-20.0, 20.0, nx)
    lat = np.linspace(30.0, 60.0, ny)
    ps = 990.0 + 40.0 * np.sin(np.deg2rad(9 * lon))[:, None] * np.cos(np.deg2rad(3 * lat))[None, :] \
        - 150.0 * np.exp(-((lon[:, None] - 5) ** 2 + (lat[None, :] - 45) ** 2) / 60.0)
    eta = np.arange(npl) / (npl - 1)
    pl = (1.0 + (ps[:, :, None] - 1.0) * (1.0 - eta)[None, None, :] ** 2).astype(np.float32)
    rel = pl.astype(np.float64) / ps[:, :, None]
    base = dict(t=210.0 + 80.0 * rel, u=30.0 * np.sin(6 * rel), v=-20.0 * np.cos(5 * rel), w=0.3 * np.sin(9 * rel),
                h2o=1e-2 * rel ** 3, o3=1e-5 * (1 - rel), lwc=1e-4 * rel, rwc=5e-5 * rel ** 2, iwc=2e-5 * (1 - rel),
                swc=1e-5 * rel * (1 - rel), cc=0.5 + 0.5 * np.sin(4 * rel))
    f3 = {"pl": pl}
    for name in fields:
        f3[name] = (base[name] * (1.0 + 0.05 * rng.standard_normal(pl.shape))).astype(np.float32)
    if ascending:
        f3 = {k: np.ascontiguousarray(v[:, :, ::-1]) for k, v in f3.items()}
    f2 = dict(ps=ps.astype(np.float32), zs=(0.01 * (1013.25 - ps)).astype(np.float32),
              ts=(288.0 + rng.standard_normal(ps.shape)).astype(np.float32))
    return R.Snap(lon, lat, np.arange(npl, dtype=np.float64), f3, f2, time=3600.0)


def targets(met_np):
    """Descending, from below every surface (1050 hPa) to above every top (0.5 hPa): both clamps are taken."""
    return np.exp(np.linspace(np.log(1050.0), np.log(0.5), met_np))


def targets_on_levels(met, ix=2, iy=1):
    """Targets exactly on model levels of one column, one double ulp either side, at and beyond both column ends."""
    pl = np.sort(met.f3["pl"][ix, iy].astype(np.float64))[::-1]
    n = len(pl)
    q = [pl[0] + 10.0, np.nextafter(pl[0], np.inf), pl[0], np.nextafter(pl[0], -np.inf)]
    for k in sorted({n // 3, n // 2, n - 2} - {0, n - 1}):
        q += [np.nextafter(pl[k], np.inf), pl[k], np.nextafter(pl[k], -np.inf)]
    q += [np.nextafter(pl[n - 1], np.inf), pl[n - 1], np.nextafter(pl[n - 1], -np.inf), 0.5 * pl[n - 1]]
    q = np.array(q)
    assert (np.diff(q) < 0).all()
    return q


def degenerate(kind):
    """Columns whose result is what IEEE arithmetic and the bisection as written give (compared in the exact library)."""
    met = ml_atmosphere(5, 3, 7, seed=5)
    pl = met.f3["pl"]
    if kind == "nan_pl":
        pl[1, 1, 3] = np.nan
        pl[4, 2, 0] = np.nan
        pl[0, 0, 6] = np.nan
    elif kind == "nan_field":
        met.f3["t"][2, 2, 4] = np.nan
        met.f3["u"][0, 1, 0] = np.nan
    elif kind == "equal_pressures":
        pl[3, 1, 4] = pl[3, 1, 3]
        pl[1, 0, 1] = pl[1, 0, 0]
    elif kind == "non_monotone":
        pl[2, 0, 2], pl[2, 0, 4] = pl[2, 0, 4], pl[2, 0, 2]
        pl[4, 1, 5] = pl[4, 1, 1]
    else:
        raise KeyError(kind)
    return met


DEGENERATE = ("nan_pl", "nan_field", "equal_pressures", "non_monotone")


def strided(met, pad_y=3, pad_p=5, pad_ml=2):
    """The same snapshot as views into arrays of larger extents (the reference's [EX][EY][EP]); the model-level pressure
    has strides of its own."""
    sy, sy_ml = met.np + pad_p, met.np + pad_ml
    sx, sx_ml, sx2 = (met.ny + pad_y) * sy, (met.ny + pad_y + 1) * sy_ml, met.ny + pad_y

    def view3(a, rows, lev):
        big = np.full((met.nx, rows, lev), -5555.0, dtype=np.float32)
        big[:, :met.ny, :met.np] = a
        return big[:, :met.ny, :met.np]

    f3 = {k: view3(v, sx_ml // sy_ml, sy_ml) if k == "pl" else view3(v, sx // sy, sy) for k, v in met.f3.items()}
    f2 = {}
    for k, v in met.f2.items():
        big = np.full((met.nx, sx2), -5555.0, dtype=np.float32)
        big[:, :met.ny] = v
        f2[k] = big[:, :met.ny]
    out = R.Snap(met.lon, met.lat, met.p, f3, f2, met.time, met.coord_type)
    out.strides, out.strides_ml = (sx, sy, sx2), (sx_ml, sy_ml)
    return out


# ---- SAMPLE ---------------------------------------------------------------------------------------------------------------

def pl_atmosphere(nx, ny, n, seed=3, periodic=True, fields=("t", "u", "w", "h2o", "z", "pv")):
    rng = np.random.default_rng(seed + 1000 * nx + 10 * ny + n)
    lon = np.linspace(-180.0, 180.0, nx) if periodic else np.linspace(0.0, 40.0, nx)
    lat = np.linspace(-90.0, 90.0, ny)
    p = 1000.0 * np.exp(-np.arange(n) * (6.0 / max(n - 1, 1)))
    scale = dict(t=250.0, u=20.0, v=15.0, w=0.2, h2o=1e-3, o3=1e-6, lwc=1e-5, rwc=1e-5, iwc=1e-5, swc=1e-5, cc=0.5, z=10.0, pv=2.0)
    f3 = {k: (scale[k] * (1.0 + 0.3 * rng.standard_normal((nx, ny, n)))).astype(np.float32) for k in fields}
    f2 = dict(ps=(1000.0 + 20.0 * rng.standard_normal((nx, ny))).astype(np.float32),
              zs=(0.5 * rng.standard_normal((nx, ny))).astype(np.float32))
    return R.Snap(lon, lat, p, f3, f2, time=7200.0)


# name: (nx, ny, np, periodic, strides, half-widths)
SAMPLE_CASES = {
    "strides_not_dividing": (9, 7, 6, True, (2, 3, 2), (1, 1, 1)),         # -> 5 x 3 x 3, plain striding
    "strides_and_smoothing": (9, 7, 6, True, (2, 3, 2), (2, 2, 2)),
    "half_widths_3_2_2": (9, 7, 6, True, (1, 1, 1), (3, 2, 2)),
    "regional_wrap": (9, 7, 6, False, (1, 1, 1), (3, 2, 2)),
    "sx_minus_1_is_nx": (3, 4, 3, True, (1, 1, 1), (4, 1, 1)),
    "tiles_end_inside": (19, 11, 20, True, (1, 1, 1), (2, 2, 2)),
    "tiles_end_inside_strided": (19, 11, 20, True, (2, 1, 3), (2, 3, 2)),
    "windows_apart": (19, 11, 20, True, (4, 5, 6), (2, 1, 2)),             # strides beyond the windows: packed in LDS
    "largest_tile": (12, 12, 8, True, (1, 1, 1), (10, 11, 4)),              # 26 x 28 x 22 floats = 64064 bytes
    "identity": (9, 7, 6, True, (1, 1, 1), (1, 1, 1)),
}
TOO_LARGE_TILE = (12, 12, 8, True, (1, 1, 1), (11, 11, 4))                  # 28 x 28 x 22 floats: beyond 64 KB


def sample_input(name):
    nx, ny, n, periodic, d, s = SAMPLE_CASES[name] if isinstance(name, str) else name
    return pl_atmosphere(nx, ny, n, periodic=periodic), d, s


def with_nan(met):
    met.f3["t"][4, 3, 2] = np.nan
    met.f2["ps"][0, 0] = np.nan
    return met
