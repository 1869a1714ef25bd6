"""The cases of mphip_ingest_met (tests/test_gpu_ingest.py, tests/test_ingest_cpu.py), all small: at most ~40 000 values per
field.  A case is a dict: the axes (lon, lat, p, coord_type), `raw` = {name: (array in file order, options)} as
Simulation.ingest_met takes it, and `tag`.

Extents: nx and np each from {2, 31, 32, 33, 63, 64, 65, 129} -- below, at and above the 64 x 64 tile of the decode kernel
and its multiples, and the smallest grid --, ny from {2, 3, 5}.  Every (nx, np) pair appears once (SHAPES) with the winds,
the temperature and a surface field; the FEATURES carry what the definitions decide on: both storage types; fill and missing
values absent, hit and NaN; |v| at 1e14f and one float ulp either side; stored NaN and infinities; the unit scales of the reader (0.01f, MA / MH2O, 1 among them);
lnsp; columns with low = -1, 0, np - 2, np - 1, columns where only one of t, u, v, w is invalid, and a snapshot without w;
latitudes north-first and south-first, with and without poles, |lat| = 89.999 exactly and the double below it, ny == 2 with
both poles; a longitude axis that meets the periodic condition, one that misses it by 0.02 and a regional one."""
import numpy as np

F32 = np.float32
EXTENTS = (2, 31, 32, 33, 63, 64, 65, 129)
NYS = (2, 3, 5)
MOST = 40000
MA, MH2O = 28.9644, 18.01528
MO3 = 48.00
# the unit scales of the host layer's reader (read_met_nc), as floats: 0.01f, MA / MH2O and 1 among them
SCL = {"w": float(F32(0.01)), "h2o": float(F32(MA / MH2O)), "o3": float(F32(MA / MO3)), "ps": float(F32(0.01)),
       "zs": float(F32(1. / (1000. * 9.80665))), "pbl": float(F32(0.01))}
LEVEL_FIELDS = ("t", "u", "v", "w", "h2o", "o3", "lwc", "rwc", "iwc", "swc", "cc")
SURFACE_FIELDS = ("ps", "zs", "ts", "us", "vs", "ess", "nss", "shf", "lsm", "sst", "pbl", "cape", "cin")
FILL_S, MISS_S = -32767, 12345
FILL_F, MISS_F = float(F32(-9.99e8)), float(F32(7777.5))
BIG = F32(1e14)


def lon_axis(nx, mode):
    i = np.arange(nx, dtype=np.float64)
    if mode == "periodic":
        return -180.0 + i * (360.0 / nx)
    if mode == "miss":                      # misses the condition by 0.02
        return -180.0 + i * ((360.0 - 0.02) / nx)
    return 5.0 + 0.5 * i                    # regional


def lat_axis(ny, mode):
    if mode in ("north", "south"):
        lat = np.linspace(90.0, -90.0, ny)
    elif mode in ("edge", "below"):
        lat = np.linspace(89.999, -89.999, ny)
        lat[0], lat[-1] = 89.999, -89.999
        if mode == "below":
            lat[-1] = np.nextafter(-89.999, 0.0)
    else:                                   # no poles
        lat = np.linspace(60.0, -60.0, ny)
    return np.ascontiguousarray(lat[::-1] if mode == "south" else lat)


def p_axis(np_):
    return 1000.0 * np.exp(-np.arange(np_, dtype=np.float64) * (9.0 / max(np_ - 1, 1)))


def raw_field(rng, shape, short, fill, miss, scl, offset=0.0, spread=30.0):
    """Random stored values and their options; fill / miss: "absent", "hit" or "nan" (floats only)."""
    opt = dict(scl=scl)
    if short:
        a = rng.integers(-32000, 32000, size=shape).astype(np.int16)
        opt.update(scale_factor=float(F32(spread / 32000.0)), add_offset=float(F32(offset)))
        if fill == "hit":
            opt["fill"] = FILL_S
        if miss == "hit":
            opt["miss"] = MISS_S
    else:
        a = (offset + spread * rng.standard_normal(shape)).astype(np.float32)
        if fill != "absent":
            opt["fill"] = FILL_F if fill == "hit" else float("nan")
        if miss != "absent":
            opt["miss"] = MISS_F if miss == "hit" else float("nan")
    flat = a.reshape(-1)
    hits = rng.choice(flat.size, size=max(1, flat.size // 50), replace=False)
    if fill == "hit":
        flat[hits[::2]] = FILL_S if short else F32(FILL_F)
    if miss == "hit":
        flat[hits[1::2]] = MISS_S if short else F32(MISS_F)
    return a, opt


def make(tag, nx, ny, np_, short, lon="periodic", lat="north", coord_type=0, fill="hit", miss="absent", seed=0,
         level=LEVEL_FIELDS, surface=("ps",), lnsp=False, clean=("t", "u", "v", "w")):
    """`clean`: the level fields that get no fill / missing value from the random draw (so that `low` is what the case
    sets by hand)."""
    rng = np.random.default_rng(1000 + seed)
    raw = {}
    for n, name in enumerate(level):
        f, m = ("absent", "absent") if name in clean else (fill, miss)
        raw[name] = raw_field(rng, (np_, ny, nx), short, f, m, SCL.get(name, 1.0), offset=250.0 if name == "t" else 0.0)
    for n, name in enumerate(surface):
        if name == "ps" and lnsp:
            a = (11.5 + 0.2 * rng.standard_normal((ny, nx))).astype(np.float32)
            if short:
                a = np.round((a - 11.5) / 1e-4).astype(np.int16)
                raw[name] = (a, dict(scale_factor=float(F32(1e-4)), add_offset=float(F32(11.5)), fill=FILL_S, scl=1.0, lnsp=1))
                a[0, 0] = FILL_S
            else:
                raw[name] = (a, dict(fill=FILL_F, scl=1.0, lnsp=1))
                a[0, 0] = F32(FILL_F)
                a[-1, -1] = F32(800.0)          # exp overflows the double: +inf
                a[-1, 0] = F32(-800.0)          # ... and underflows it: 0
        else:
            raw[name] = raw_field(rng, (ny, nx), short, fill, miss, SCL.get(name, 1.0), offset=1000.0)
    return dict(tag=tag, nx=nx, ny=ny, np=np_, lon=lon_axis(nx, lon), lat=lat_axis(ny, lat), p=p_axis(np_), coord_type=coord_type,
                raw=raw)


def invalidate(case, name, i, j, k):
    """Make the stored value of field `name` at column (i, j), level k one that decodes to NaN."""
    a, opt = case["raw"][name]
    if a.dtype == np.int16:
        opt.setdefault("fill", FILL_S)
        a[k, j, i] = opt["fill"]
    else:
        a[k, j, i] = np.nan


def set_lows(case):
    """Columns with low = 0, np - 2, np - 1 (and -1 everywhere else), and columns where only one of t, u, v, w is invalid."""
    nx, ny, np_ = case["nx"], case["ny"], case["np"]
    cols = [(i, j) for j in range(ny) for i in range(nx)]
    rng = np.random.default_rng(7)
    rng.shuffle(cols)
    present = [n for n in ("t", "u", "v", "w") if n in case["raw"]]
    plan = [(present[0], 0), (present[1 % len(present)], np_ - 2), (present[2 % len(present)], np_ - 1)]
    plan += [(n, np_ // 2) for n in present]
    for (i, j), (name, k) in zip(cols, plan):
        invalidate(case, name, i, j, k)
    # (two invalid levels in one column: the larger one decides)
    if len(cols) > len(plan) and np_ > 2:
        i, j = cols[len(plan)]
        invalidate(case, present[0], i, j, 0)
        invalidate(case, present[-1], i, j, np_ - 2)
    return case


def shapes():
    out = []
    n = 0
    for nx in EXTENTS:
        for np_ in EXTENTS:
            ny = NYS[n % 3]
            while nx * ny * np_ > MOST:
                ny = NYS[NYS.index(ny) - 1]
            short = n % 2 == 0
            c = make(f"shape_{nx}x{ny}x{np_}_{'short' if short else 'float'}", nx, ny, np_, short, seed=n,
                     lon=("periodic", "regional", "miss")[n % 3], lat=("north", "south", "none")[(n // 3) % 3],
                     level=("t", "u", "v", "w", "h2o"), surface=("ps", "zs"))
            out.append(set_lows(c))
            n += 1
    return out


def features():
    out = []
    # every field, both storage types, the fill / missing-value combinations
    for n, (short, fill, miss) in enumerate([(True, "hit", "hit"), (True, "absent", "hit"), (True, "absent", "absent"),
                                             (False, "hit", "hit"), (False, "nan", "hit"), (False, "hit", "nan"),
                                             (False, "absent", "absent")]):
        c = make(f"all_{'short' if short else 'float'}_fill_{fill}_miss_{miss}", 33, 5, 65, short, fill=fill, miss=miss, seed=100 + n,
                 surface=SURFACE_FIELDS, lnsp=n % 2 == 0)
        out.append(set_lows(c))
    # |v| at 1e14f and one ulp either side, stored NaN and infinities (floats); the same threshold through the short decode
    c = make("threshold_float", 31, 3, 32, False, fill="absent", seed=200, lat="none", lon="regional")
    edge = np.array([BIG, np.nextafter(BIG, F32(0)), np.nextafter(BIG, F32(np.inf)), -BIG, -np.nextafter(BIG, F32(0)),
                     -np.nextafter(BIG, F32(np.inf)), np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    nanp = np.array([0x7fc12345, 0xffc00001], dtype=np.uint32).view(np.float32)      # NaNs with payloads
    for name in ("h2o", "o3", "t"):
        a = c["raw"][name][0]
        a[5, 1, :edge.size] = edge
        a[6, 2, :2] = nanp
    out.append(c)
    c = make("threshold_short", 32, 3, 31, True, fill="absent", seed=201, lat="none", lon="miss")
    for name in ("h2o", "o3"):
        a, opt = c["raw"][name]
        opt.update(scale_factor=float(F32(1e10)), add_offset=0.0)
        a[3, 1, :6] = (10000, 9999, 10001, -10000, -9999, -10001)
    a, opt = c["raw"]["lwc"]
    opt.update(scale_factor=float(BIG / F32(3)), add_offset=float(np.nextafter(BIG, F32(0)) - BIG))
    a[3, 1, :4] = (3, -3, 2, 4)
    out.append(c)
    # the poles: |lat| = 89.999 exactly, the double below it, south first, ny == 2, a Cartesian grid
    for n, (lat, ny, coord) in enumerate([("edge", 5, 0), ("below", 5, 0), ("south", 3, 0), ("north", 2, 0), ("south", 2, 0),
                                          ("north", 3, 1)]):
        for short in (True, False):
            c = make(f"poles_{lat}_ny{ny}_coord{coord}_{'short' if short else 'float'}", 63, ny, 33, short, lat=lat,
                     coord_type=coord, seed=300 + n, level=("t", "u", "v", "w", "cc"), surface=("ps", "lsm"))
            out.append(set_lows(c))
    # no w in the file: it counts as finite, and is not filled
    c = make("without_w", 64, 3, 64, True, seed=400, level=("t", "u", "v", "h2o", "o3"))
    out.append(set_lows(c))
    c = make("winds_and_t", 65, 2, 63, False, seed=401, level=("t", "u", "v"))
    out.append(set_lows(c))
    return out


SHAPES = shapes()
FEATURES = features()
CASES = {c["tag"]: c for c in SHAPES + FEATURES}
assert len(CASES) == len(SHAPES) + len(FEATURES)
