"""Inputs for the edge tests of the radix sort and of the order repair, placed by key.

On a latitude/longitude grid the key of module_sort is (ix * ny + iy) * np + iz, (ix, iy, iz) being the cell the
interpolation stencil starts in.  A particle at the centre of a cell with ix <= nx - 2, iy <= ny - 2, iz <= np - 2 (a
"usable" cell) is strictly inside it in all three axes, so a case is a list of keys by slot (place()); the searches
themselves, on and beside grid lines, are the subject of tests/test_gpu_axis_edges.py.  Every particle carries its
index + 1 in the quantity m.

One grid per pass plan of radix_passes (mptrac_amd/csrc/mphip_api.hip), restated in plan():

    grid tuple       kmax      key bits  digit      passes  result pair
    (6, 6, 6)        252       8         8          1       1
    (7, 8, 7)        448       9         9 (auto)   1       1
    (9, 10, 10)      1000      10        10 (auto)  1       1
    (36, 19, 20)     14060     14        8          2       0
    (72, 37, 40)     108040    17        9 (auto)   2       0
    (120, 61, 100)   738100    20        10 (auto)  2       0
    C1               3920460   22        8          3       1

Left out: 25 to 27 key bits (three 9-bit passes without forcing) need the C3 grid, and four passes need more than 2^30
cells.  The forced digit widths (option sort_bits) bring every kernel instantiation to one, two and three passes.

What arithmetic rules out: in a one-pass plan the digit is at least as wide as the key, and the largest usable key is
below kmax - 1 <= radix - 1, so no valid key has the digit radix - 1 there; the pattern "low_radix_1" (valid keys that
share the digit of the padding lanes, whose key is 0xffffffff) runs on the plans with two and three passes.  On the
(36, 19, 20) grid the high digit never exceeds 54, so only the first pass of its sorts has counters behind the border of
the scan's first chunk (digit 240 at 17 and 18 tiles); on (9, 10, 10) the single pass has (digit 819 at 5 tiles).

The repair cases (REPAIR) decide who moves: the case `advect` without diffusion, winds u constant per latitude row and
v = w = 0 in both snapshots.  The cell rows iy = 0, 2, 4 ... have the same u on their two latitude rows, +1.2 cell widths
per step where iy % 4 == 0 and -1.2 where iy % 4 == 2 (a particle is then never closer than 0.1 cell widths to a grid
line), and only these rows hold particles.  A particle moves in a step if the slot it is stored in got a time step:
module_timesteps runs before module_sort and cache->dt stays with the slot (as in the reference), so the movers of a
step are the slots whose particle BEFORE that step's sort had been released (time < t).  Particles that are never
released carry time = t_stop.  model_run() restates this; tests/test_sort_edges_cpu.py holds it against the oracle."""
import functools

import numpy as np

from mptrac_amd.ctl import ctl_from_quantities
from mptrac_amd.clim import load_clim_tropo
from mptrac_amd.synth import GRIDS as NAMED, make_axes, synthetic_met

# ---- the launch arithmetic, restated (tests/test_sort_edges_cpu.py pins the constants to the source text) ---------------
SORT_THREADS, SORT_ROUNDS = 256, 16
SORT_TILE = SORT_THREADS * SORT_ROUNDS          # keys per workgroup
WAVE_SHARE = SORT_TILE // 4                     # keys of a tile that one wave ranks
SCAN_THREADS, SCAN_PER_SMALL, SCAN_PER_LARGE = 1024, 4, 16
REPAIR_TILE, MERGE_TILE = 1024, 2048
RADIX_MAX_BITS = 10

GRIDS = {"p1b8": (6, 6, 6), "p1b9": (7, 8, 7), "p1b10": (9, 10, 10),
         "p2b8": NAMED["tiny"], "p2b9": (72, 37, 40), "p2b10": (120, 61, 100), "p3b8": NAMED["C1"]}
# (key bits, automatic digit width, passes, buffer pair of the result)
PLANS = {"p1b8": (8, 8, 1, 1), "p1b9": (9, 9, 1, 1), "p1b10": (10, 10, 1, 1),
         "p2b8": (14, 8, 2, 0), "p2b9": (17, 9, 2, 0), "p2b10": (20, 10, 2, 0), "p3b8": (22, 8, 3, 1)}


def dims(grid):
    nx0, ny, npl = GRIDS[grid]
    return nx0 + 1, ny, npl


def bits_for(kmax):
    b = 1
    while b < 32 and (kmax >> b) != 0:
        b += 1
    return b


def plan(grid, n, sort_bits=0):
    """radix_passes for n pairs with the keys of `grid`"""
    nx, ny, npl = dims(grid)
    key_bits = bits_for(nx * ny * npl)
    bits = sort_bits
    if bits == 0:
        bits = 8
        for b in range(9, RADIX_MAX_BITS + 1):
            if -(-key_bits // b) < -(-key_bits // bits):
                bits = b
    passes = -(-key_bits // bits)
    ntiles = -(-n // SORT_TILE)
    m = (1 << bits) * ntiles
    small = -(-m // (SCAN_THREADS * SCAN_PER_SMALL)) <= SCAN_THREADS
    chunk = SCAN_THREADS * (SCAN_PER_SMALL if small else SCAN_PER_LARGE)
    return dict(key_bits=key_bits, bits=bits, passes=passes, pair=passes & 1, ntiles=ntiles, m=m, chunk=chunk,
                nchunks=-(-m // chunk), last_tile=n - (ntiles - 1) * SORT_TILE)


def repair_plan(n):
    tiles = -(-n // REPAIR_TILE)
    return dict(tiles=tiles, per=-(-tiles // 1024), merge_tiles=-(-n // MERGE_TILE))


# ---- keys and positions --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def usable(grid):
    """the keys of the cells a centred particle is strictly inside of, ascending"""
    nx, ny, npl = dims(grid)
    ix, iy, iz = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(npl - 1), indexing="ij")
    k = ((ix * ny + iy) * npl + iz).ravel().astype(np.int64)
    k.setflags(write=False)
    return k


def cell_of(grid, keys):
    _, ny, npl = dims(grid)
    keys = np.asarray(keys, dtype=np.int64)
    return keys // (ny * npl), keys // npl % ny, keys % npl


def axes(grid):
    return make_axes(*GRIDS[grid])


def place(grid, keys, time=0.0):
    """atm: particle i at the centre of the cell of keys[i]; q[m] = i + 1"""
    lon, lat, p = axes(grid)
    ix, iy, iz = cell_of(grid, keys)
    nx, ny, npl = dims(grid)
    assert ix.max(initial=0) <= nx - 2 and iy.max(initial=0) <= ny - 2 and iz.max(initial=0) <= npl - 2
    n = len(ix)
    t = np.empty(n)
    t[:] = time
    return {"time": t, "lon": 0.5 * (lon[ix] + lon[ix + 1]), "lat": 0.5 * (lat[iy] + lat[iy + 1]),
            "p": np.sqrt(p[iz] * p[iz + 1]), "q": np.arange(1.0, n + 1.0).reshape(1, n)}


def keys_of(grid, lon, lat, p):
    """module_sort's key of positions that are on no grid line (numpy restatement)"""
    glon, glat, gp = axes(grid)
    nx, ny, npl = dims(grid)
    ix = np.clip(np.floor((lon - glon[0]) / (glon[1] - glon[0])).astype(np.int64), 0, nx - 2)
    iy = np.clip(np.floor((lat - glat[0]) / (glat[1] - glat[0])).astype(np.int64), 0, ny - 2)
    iz = np.clip(np.searchsorted(-gp, -np.asarray(p), side="right") - 1, 0, npl - 2)
    return (ix * ny + iy) * npl + iz


CTL = dict(advect=4, dt_mod=180.0, t_stop=3600.0, dt_met=3600.0, rng_type=1, **ctl_from_quantities(("m",)))
FIELDS = ("u", "v", "w", "ps")


@functools.lru_cache(maxsize=2)
def mets(grid):
    return synthetic_met(GRIDS[grid], 0.0, 1.0, fields=FIELDS), synthetic_met(GRIDS[grid], 3600.0, 1.25, fields=FIELDS)


def clim():
    return load_clim_tropo()


# ---- key patterns --------------------------------------------------------------------------------------------------------

def _spread(pool, n):
    """n keys of the ascending pool, ascending, with the fewest repeats"""
    return pool[np.arange(n, dtype=np.int64) * len(pool) // n]


def _cycle(pool, n, step=7):
    """n keys of the pool in a scrambled, repeating order"""
    step = next(s for s in range(step, step + len(pool) + 1) if np.gcd(s, len(pool)) == 1)
    return pool[(np.arange(n, dtype=np.int64) * step + 3) % len(pool)]


def _most(values):
    v, c = np.unique(values, return_counts=True)
    return v[np.argmax(c)]


def pattern_keys(grid, pattern, n, bits=0):
    """the keys of a from-scratch case, by slot; `bits`: the digit width of the sort (0: the automatic one)"""
    U = usable(grid)
    P = plan(grid, n, bits)
    radix, top = 1 << P["bits"], P["bits"] * (P["passes"] - 1)
    if pattern == "equal_first":
        return np.full(n, U[0])
    if pattern == "equal_last":
        return np.full(n, U[-1])
    if pattern == "sorted":
        return np.sort(_spread(U, n))
    if pattern == "descending":
        return np.sort(_spread(U, n))[::-1].copy()
    if pattern.startswith("alternate"):          # the smallest and the largest usable key, `period` slots each
        period = int(pattern[9:])
        return np.where((np.arange(n) // period) % 2 == 0, U[0], U[-1])
    if pattern == "low_radix_1":                 # the digit of the padding lanes in the first pass
        return _cycle(U[(U & (radix - 1)) == radix - 1], n)
    if pattern == "top_only":                    # one value of all digits below the top one
        low = U & ((1 << top) - 1)
        return _cycle(U[low == _most(low)], n)
    if pattern == "bottom_only":                 # one value of all digits above the bottom one
        return _cycle(U[(U >> P["bits"]) == _most(U >> P["bits"])], n)
    if pattern == "tied":                        # a few hundred distinct keys, one of them holds half the particles
        rng = np.random.default_rng(n + 31 * P["bits"])
        distinct = rng.choice(U, size=min(300, len(U)), replace=False)
        k = distinct[rng.integers(0, len(distinct), n)]
        k[rng.permutation(n)[:n // 2]] = distinct[0]
        return k
    if pattern == "uniform":                     # every usable key about equally often, in random order
        return np.random.default_rng(n).choice(U, size=n)
    raise KeyError(pattern)


# (grid, pattern, n): the automatic digit width
SCRATCH = (
    [("p1b8", "equal_first", n) for n in (1, 2, 63, 64, 65)]
    + [("p2b8", "equal_first", 4096), ("p2b8", "equal_first", 8193), ("p1b10", "equal_first", 1025),
       ("p1b9", "equal_last", 4097), ("p2b9", "equal_last", 8192), ("p3b8", "equal_last", 1024),
       ("p1b8", "sorted", 1023), ("p1b8", "sorted", 1024), ("p2b8", "sorted", 4095), ("p2b10", "sorted", 8193),
       ("p1b9", "descending", 1025), ("p2b8", "descending", 4096), ("p2b8", "descending", 4097),
       ("p2b9", "descending", 65), ("p3b8", "descending", 8193)]
    + [("p1b8", "alternate%d" % k, 8193) for k in (1, 64, 1024, 4096)]
    + [("p2b8", "alternate64", 8192), ("p2b8", "alternate1024", 8192), ("p2b10", "alternate1", 8193),
       ("p2b10", "alternate4096", 8193),
       ("p2b8", "low_radix_1", 63), ("p2b8", "low_radix_1", 1025), ("p2b8", "low_radix_1", 4097),
       ("p2b9", "low_radix_1", 1023), ("p2b10", "low_radix_1", 65), ("p3b8", "low_radix_1", 4097),
       ("p1b8", "top_only", 1024), ("p2b8", "top_only", 4097), ("p2b10", "top_only", 1025),
       ("p1b10", "bottom_only", 4097), ("p2b8", "bottom_only", 4097), ("p2b9", "bottom_only", 8193),
       ("p1b8", "tied", 4097), ("p1b9", "tied", 20011), ("p2b8", "tied", 20011), ("p2b10", "tied", 8193),
       ("p3b8", "tied", 4097),
       # the two-level scan: 16, 17 and 18 tiles of 256 counters (1 chunk, then 2, the border inside digit 240's row);
       # 5 and 6 tiles of 1024 counters (2 chunks)
       ("p2b8", "uniform", 65536), ("p2b8", "uniform", 65537), ("p2b8", "uniform", 69633),
       ("p1b10", "uniform", 16385), ("p1b10", "uniform", 20481)])
# (grid, pattern, n, sort_bits): every instantiation at one, two and three passes
FORCED = ([(g, "tied", 4097, b) for g in GRIDS for b in (8, 9, 10)]
          + [("p1b9", "low_radix_1", 1025, 8), ("p2b9", "low_radix_1", 1025, 8), ("p2b10", "low_radix_1", 4097, 9)])


def case_id(case):
    return "-".join(str(c) for c in case)


# ---- the repair: who moves -----------------------------------------------------------------------------------------------

STEP_CELLS = 1.2          # cell widths per time step in a moving row
NEVER = CTL["t_stop"]     # time of a particle that is never released


def row_sign(iy):
    return np.where(iy % 4 == 0, 1.0, -1.0)


def repair_mets(grid, still=False):
    """both snapshots: u carries a centred particle of the cell rows 0, 2, 4 ... by 1.2 cells per step along its row
    (still: no wind at all), v = w = 0, the surface below every particle"""
    out = []
    lon, lat, _ = axes(grid)
    nx, ny, npl = dims(grid)
    re = 6367.421          # the reference's mean radius of the Earth [km]
    for time in (0.0, 3600.0):
        m = synthetic_met(GRIDS[grid], time, 1.0, fields=FIELDS)
        u = np.zeros((nx, ny, npl), dtype=np.float32)
        for iy in range(0, ny - 1, 2):
            latc = 0.5 * (lat[iy] + lat[iy + 1])
            assert abs(latc) < 89.0
            km = STEP_CELLS * (lon[1] - lon[0]) * np.pi * re / 180.0 * np.cos(np.deg2rad(latc))
            u[:, iy:iy + 2, :] = 0.0 if still else row_sign(iy) * km * 1000.0 / CTL["dt_mod"]
        assert np.all(np.isfinite(u))
        m.f3["u"] = u
        m.f3["v"] = np.zeros_like(u)
        m.f3["w"] = np.zeros_like(u)
        m.f2["ps"] = np.full((nx, ny), 1013.25, dtype=np.float32)
        out.append(m)
    return out


def moving_cells(grid, band):
    """keys (ascending) of the cells that hold particles: band -- every ix of one level and of one row of either
    direction (crowded: movers arrive among stayers, from lower and from higher slots); all -- every usable cell of the
    rows 0, 2, 4 ..."""
    U = usable(grid)
    ix, iy, iz = cell_of(grid, U)
    rows = sorted(set(iy[iy % 2 == 0].tolist()))
    if band:
        plus, minus = [r for r in rows if r % 4 == 0], [r for r in rows if r % 4 == 2]
        keep = np.isin(iy, [plus[len(plus) // 2], minus[len(minus) // 2]]) & (iz == 1)
    else:
        keep = np.isin(iy, rows)
    return U[keep]


def _mask(n, slots):
    m = np.zeros(n, dtype=bool)
    m[np.asarray(slots, dtype=np.int64)] = True
    return m


def repair_case(name):
    """dict(grid, keys, time, still, steps, movers): keys by slot (ascending: the first sort is the identity), release
    times, and the slots of the previous sort that have moved at each module_sort -- what the case claims"""
    grid, band, still, steps = "p2b8", True, False, 4
    late = None
    if name[1:].isdigit():                                # about 15 % movers at the sizes around the tiles
        n = int(name[1:])
        rng = np.random.default_rng(n)
        first = rng.random(n) < 0.15
        late = (rng.random(n) < 0.02) & ~first
    elif name == "none":
        n, still = 4097, True
        first = np.ones(n, dtype=bool)                    # (everybody gets a time step; there is no wind)
    elif name == "all":
        n = 4097
        first = np.ones(n, dtype=bool)
    elif name == "one_first":
        n = 4097
        first = _mask(n, [0])
    elif name == "one_last":
        n = 4097
        first = _mask(n, [n - 1])
    elif name == "one_stayer":
        n = 4097
        first = ~_mask(n, [n // 2])
    elif name == "tiles":                                 # tile 1: movers only, tiles 0 and 2: none, tile 3: one, tile 4: 1023
        n = 20011
        first = _mask(n, np.r_[1024:2048, 3072 + 5, 4096:4096 + 400, 4096 + 401:5120])
    elif name == "cross4096":                                 # 4096 movers, then 4097
        n = 20011
        first = _mask(n, np.arange(4096) * 4 + 1)
        late = _mask(n, [19999])
    elif name == "runs":                                  # whole merge tiles from one side, stayers and movers
        n = 20011
        first = _mask(n, np.r_[9000:9000 + 4200])
    elif name == "mixed":
        n, band = 20011, False
        rng = np.random.default_rng(5)
        first = rng.random(n) < 0.15
        late = (rng.random(n) < 0.02) & ~first
    elif name == "one_pass":                              # the movers' radix sort in a single digit pass
        grid, n = "p1b8", 4097
        rng = np.random.default_rng(7)
        first = rng.random(n) < 0.15
    elif name == "big":                                   # 1026 repair tiles: repair_scan_kernel with per = 2
        n, band, steps = 1049601, False, 3
        rng = np.random.default_rng(11)
        first = rng.random(n) < 0.15
    else:
        raise KeyError(name)
    cells = moving_cells(grid, band)
    keys = np.sort(_spread(cells, n))
    if name == "runs":          # the 4200 movers share one cell: they arrive as one run of the merged sequence
        crowded = keys[9000]
        keys[9000:9000 + 4200] = crowded
        keys = np.sort(keys)
        first = keys == crowded
        assert 4200 <= first.sum() < 4500
    time = np.where(first, 0.0, NEVER)
    if late is not None:
        time[late] = CTL["dt_mod"]
    return dict(name=name, grid=grid, keys=keys, time=time, still=still, steps=steps, n=n)


REPAIR = ["none", "all", "one_first", "one_last", "one_stayer", "tiles", "cross4096", "runs", "mixed", "one_pass",
          "n1023", "n1024", "n1025", "n2047", "n2048", "n2049", "n4097"]
BIG = "big"


def repair_inputs(case):
    """(ctl, clim, met0, met1, atm) of a repair case"""
    m0, m1 = repair_mets(case["grid"], case["still"])
    atm = place(case["grid"], case["keys"], case["time"])
    return dict(CTL, sort_dt=CTL["dt_mod"]), clim(), m0, m1, atm


def step_times(case):
    return [k * CTL["dt_mod"] for k in range(case["steps"])]


def model_run(case):
    """The run restated: for every step the keys by slot before module_sort, the stable permutation, and the slots (of
    the previous sort's order) whose key has changed since that sort -- the movers of the repair."""
    grid = case["grid"]
    lon, lat, p = (place(grid, case["keys"])[k] for k in ("lon", "lat", "p"))
    time = case["time"].copy()
    dlon = axes(grid)[0][1] - axes(grid)[0][0]
    out, prev_sorted = [], None
    for t in step_times(case):
        dt = np.where((time >= 0.0) & (time <= CTL["t_stop"]) & (time < t), t - time, 0.0)      # by slot, before the sort
        keys = keys_of(grid, lon, lat, p)
        perm = np.argsort(keys, kind="stable")
        movers = np.zeros(len(keys), dtype=bool) if prev_sorted is None else keys != prev_sorted
        out.append(dict(t=t, keys=keys, perm=perm, movers=movers))
        lon, lat, p, time = lon[perm], lat[perm], p[perm], time[perm]
        prev_sorted = keys[perm]
        if not case["still"]:
            iy = cell_of(grid, prev_sorted)[1]
            moved = dt != 0.0
            lon = np.where(moved, lon + row_sign(iy) * STEP_CELLS * dlon * dt / CTL["dt_mod"], lon)
            lon = np.where(moved, (lon + 180.0) % 360.0 - 180.0, lon)
        time = time + dt
    return out


def merge_sides(step):
    """per merge tile of 2048 results of a step of model_run / oracle_run: (results from the stayers, from the movers)"""
    f = step["movers"][step["perm"]]
    return [(int(np.count_nonzero(~f[a:a + MERGE_TILE])), int(np.count_nonzero(f[a:a + MERGE_TILE])))
            for a in range(0, len(f), MERGE_TILE)]


def scratch_inputs(grid, keys):
    m0, m1 = mets(grid)
    return dict(CTL), clim(), m0, m1, place(grid, keys)


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The steps of a repair case on the oracle: per step the keys by slot before module_sort, its permutation, the
    movers (as model_run) and the state and random-number counter behind the step.  Computed once per case."""
    from oracle import binding as B
    case = repair_case(name)
    o = B.Oracle(*repair_inputs(case))
    o.timesteps_init()
    out, prev_sorted = [], None
    for t in step_times(case):
        saved = {k: getattr(o, k).copy() for k in ("time", "lon", "lat", "p", "q")}
        keys, perm = o.sort()                       # (module_sort for its keys and permutation, then undone: inside the
        for k, v in saved.items():                  #  step module_timesteps runs before module_sort)
            getattr(o, k)[...] = v
        keys = keys.astype(np.int64)
        movers = np.zeros(len(keys), dtype=bool) if prev_sorted is None else keys != prev_sorted
        prev_sorted = keys[perm]
        o.run_timestep(t)
        state = o.state()
        for v in state.values():
            v.setflags(write=False)
        out.append(dict(t=t, keys=keys, perm=perm, movers=movers, state=state, ctr=int(o.cache.rng_ctr)))
    return out
