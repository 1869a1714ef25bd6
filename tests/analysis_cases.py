"""Edge inputs of the sample and station outputs (mphip_sample_obs, mphip_station_hits; sample_hits_kernel, sample_sum_kernel,
station_mark_kernel / _rows_kernel / _restore_kernel in mptrac_amd/csrc/mphip_kernels.hpp; the host loops: write_sample and
write_station of mptrac_amd/host/output.c, transcribed in tests/refanalysis.py).

Every decision of the two loops is a negated strict comparison -- equality is inside, a NaN is inside:

  sample  : !(time < t0 || time > t1), !(fabs(ob_lat - lat) > reach_lat), !(dist2 > dx^2), dz > 0 && !(p > p_bottom || p < p_top)
  station : !(time < t0 || time > t1 || time < s0 || time > s1), !(int) flag, !(dist2 > r^2)
  weight  : z < kz[0], z > kz[nk - 1], the bisection kz[mid] > z

  sites       observations / stations with longitudes in [180, 360) and beyond 360, the same place given as 370 and as 10,
              both poles, latitude 89.5 with particles across the pole, the equator
  distance    per (site, direction) the two adjacent doubles of the particle's longitude or latitude between which
              dist2 > dx^2 changes (bisection on the reference), and a dx with dx * dx == dist2 of a placed pair
  band        per site the adjacent doubles either side of fabs(ob_lat - lat) > reach_lat, north and south; particles in
              the sliver beyond the band where the chord is still <= dx; fabs(...) == reach_lat where it exists
  depth       p equal to the host's 1013.25 exp(-(z +- dz) / 7) and one double either side; dz = 0, -999, 5e-324, normal
  time        the ends of the step window and of the station windows with their neighbours; s0 > s1, s0 == s1 == time
  weighting   nk = 0, 1, 2, 5, nodes that are Z of placed pressures, particles below / above all nodes, repeated nodes
  lists       clusters that give observations exactly 0, 1, 63, 64, 65, 128 and 129 hits, masses over 16 decades with
              both signs, identical observations, a particle inside five cylinders
  tiles       0, 1, 255, 256, 257, 513 and 1025 observations per call, crowded ones at 0, 255, 256, 257, 511, 512, nobs - 1
  counts      1, 255, 256, 257 and 16390 particles; hits either side of the scan's chunk border at 16384; a block of 256
              whose last lane alone is in the time window, blocks without any
  not finite  NaN and +-inf in time, lon, lat and p, one at a time
  flags       0.5, -0.5, 1e-300 ... truncate to 0 (listed, set to 1, restored bit for bit); 1.5, 2, -1 are skipped

The placed particles come first, in front of a random background.  What the inputs do is computed from the reference
arithmetic alone (facts, asserted in tests/test_analysis_edges_cpu.py); the expected results of every call are computed
once per process (reference) and shared by the GPU tests."""
import functools
import math

import numpy as np

import refanalysis as RA
from box_cases import heights

NAMES = ("m", "stat")
QM, QSTAT = 0, 1
T, DT_MOD = 360.0, 180.0                  # the window [270, 450]: its ends and its middle are exact
T0, T1 = T - 0.5 * DT_MOD, T + 0.5 * DT_MOD
T_OUT = T - DT_MOD                        # outside the window; the earliest particle time (a time step there moves nobody)
DX, DZ, Z_OBS = 800.0, 6.0, 10.0
MET_GRID = (36, 19, 40)
EVER = (-1e100, 1e100)
N_BACKGROUND = 1200
SLIVER = (1e-9, 1e-4, 6e-4)               # |dlat| = (1 + f) reach_lat: beyond the band, the chord still <= dx
VARIANTS = ("uploaded", "locality", "interval0")
NOBS = (0, 1, 255, 256, 257, 513, 1025)
TILE_SLOTS = (0, 255, 256, 257, 511, 512)     # ... and nobs - 1
COUNTS = (1, 255, 256, 257, 16390)
BORDER = (0, 16382, 16383, 16384, 16385, 16389)
FLAGS = (0.0, 0.5, -0.5, 1.5, 2.0, -1.0, 1e-300, 1.0, -0.0, 0.999999, -1e-300)
LENGTHS = (129, 0, 128, 65, 65, 64, 63, 1)    # an empty observation between two crowded ones, two identical ones
BOX = (-180.0, 180.0, 6, -90.0, 90.0, 5, 0.0, 30.0, 4)

SITES = {   # name: (lon, lat)
    "mid": (12.3, 41.7), "wide": (200.0, -30.0), "w370": (370.0, 10.0), "w10": (10.0, 10.0), "npole": (33.0, 90.0),
    "spole": (-120.0, -90.0), "cap": (75.0, 89.5), "equator": (300.0, 0.0), "depth": (-60.0, 25.0), "time": (150.0, -10.0),
    "wfn": (100.0, 45.0), "flags": (-100.0, 35.0),
}
EDGE_SITES = ("mid", "wide", "w370", "w10", "npole", "spole", "cap", "equator")
STATION_WINDOWS = {"ever": EVER, "inside": (300.0, 400.0), "reversed": (400.0, 300.0), "point": (T, T),
                   "cuts_above": (-1e100, 360.5), "cuts_below": (350.25, 1e100), "over_t0": (100.0, 300.0),
                   "over_t1": (400.0, 1000.0)}


def up(x):
    return math.nextafter(x, math.inf)


def down(x):
    return math.nextafter(x, -math.inf)


def setup():
    """(ctl, clim, met0, met1): no module is due in a time step at the earliest particle time, which only stores the
    particles in the order asked for"""
    import cases
    from mptrac_amd.ctl import ctl_from_quantities
    from mptrac_amd.synth import synthetic_met
    ctl = dict(cases.BASE, **ctl_from_quantities(NAMES))
    m0 = synthetic_met(MET_GRID, 0.0, 1.0, fields=cases.PRESSURE_LEVEL_FIELDS)
    m1 = synthetic_met(MET_GRID, 3600.0, 1.25, fields=cases.PRESSURE_LEVEL_FIELDS)
    return ctl, cases.load_clim_tropo(), m0, m1


def reach_lat(dx):
    return dx * 180. / (math.pi * RA.RE)


def dist2(lon_a, lat_a, lon_b, lat_b):
    """dist2(geo2cart(a), geo2cart(b)) of output.c"""
    a, b = RA.geo2cart(0.0, lon_a, lat_a), RA.geo2cart(0.0, lon_b, lat_b)
    s = 0.0
    for k in range(3):
        s += (a[k] - b[k]) * (a[k] - b[k])
    return s


def bisect(pred, lo, hi):
    """two adjacent doubles lo < hi between the arguments with pred(lo) != pred(hi)"""
    at_lo = pred(lo)
    assert lo < hi and at_lo != pred(hi), (lo, hi)
    while True:
        mid = lo + 0.5 * (hi - lo)
        if not lo < mid < hi:
            break
        if pred(mid) == at_lo:
            lo = mid
        else:
            hi = mid
    assert up(lo) == hi
    return lo, hi


def around(x):
    return ((x, "on"), (down(x), "below"), (up(x), "above"))


# ---------------------------------------------------------------------------
# weighting functions
# ---------------------------------------------------------------------------

NODE_HEIGHTS = (4.0, 8.0, 12.0, 16.0, 22.0)


@functools.lru_cache(maxsize=None)
def nodes():
    """[(kz, exact pressure, pressure below, pressure above)]: kz is Z of a pressure, to the bit"""
    out = []
    for z in NODE_HEIGHTS:
        kz = RA.Z(RA.P(z))
        exact, below, above = heights(kz)
        assert exact and below is not None and above is not None and RA.Z(below) < kz < RA.Z(above)
        out.append((kz, exact[0], below, above))
    return out


def kernels():
    kz = [n[0] for n in nodes()]
    return {
        "nk0": ((), ()),
        "nk1": ((5.0,), (0.7,)),
        "nk2": ((kz[0], kz[4]), (0.2, 1.0)),
        "nk5": (tuple(kz), (0.2, 1.0, 0.6, 0.1, 0.4)),
        "rep4": ((kz[0], kz[2], kz[2], kz[4]), (0.2, 1.0, 0.5, 0.1)),      # a repeated inner node: never divided by
        "rep3": ((kz[0], kz[2], kz[2]), (0.2, 1.0, 0.5)),                  # ... a repeated last node: 0.5 / 0 * 0 on it
    }


# ---------------------------------------------------------------------------
# the main particle set
# ---------------------------------------------------------------------------

def _distance_pairs(site):
    """[(direction, lon, lat, side)]: the adjacent doubles either side of dist2 > DX^2.  east / west: along the site's
    parallel; ne: 5 degrees east, northwards (inside the band); across: over the pole; north / south: along the meridian
    (beyond the band: the station output alone decides on the distance there)."""
    lon0, lat0 = SITES[site]
    out = []

    def far(lon, lat):
        return dist2(lon0, lat0, lon, lat) > DX * DX

    def along_lon(name, lo, hi, lat):
        a, b = bisect(lambda x: far(x, lat), lo, hi)
        out.extend([(name, a, lat, "lo"), (name, b, lat, "hi")])

    def along_lat(name, lo, hi, lon):
        a, b = bisect(lambda y: far(lon, y), lo, hi)
        out.extend([(name, lon, a, "lo"), (name, lon, b, "hi")])

    if site in ("npole", "spole"):
        sign = -1.0 if site == "npole" else 1.0
        lo, hi = sorted((lat0 + sign * 7.0, lat0 + sign * 7.4))
        along_lat("south" if site == "npole" else "north", lo, hi, lon0)
        along_lat("south2" if site == "npole" else "north2", lo, hi, lon0 + 90.0)
    elif site == "cap":
        along_lat("across", 80.0, 89.0, lon0 + 180.0)
        along_lat("across2", 80.0, 89.0, lon0 + 170.0)
        along_lat("south", lat0 - 7.4, lat0 - 7.0, lon0)
    else:
        along_lon("east", lon0 + 1.0, lon0 + 40.0, lat0)
        along_lon("west", lon0 - 40.0, lon0 - 1.0, lat0)
        along_lat("ne", lat0 + 1.0, lat0 + 7.15, lon0 + 5.0)
        along_lat("sw", lat0 - 7.15, lat0 - 1.0, lon0 - 5.0)
        along_lat("north", lat0 + 7.0, lat0 + 7.4, lon0)
        along_lat("south", lat0 - 7.4, lat0 - 7.0, lon0)
    return out


def _band_points(site):
    """[(kind, lat)] on the site's meridian: the adjacent doubles either side of fabs(ob_lat - lat) > reach_lat, the
    sliver beyond, and ob_lat +- reach_lat where the difference is reach_lat to the bit"""
    _, lat0 = SITES[site]
    reach = reach_lat(DX)
    out = []
    for name, sign in (("north", 1.0), ("south", -1.0)):
        if (site in ("npole", "cap") and sign > 0) or (site == "spole" and sign < 0):
            continue         # (no latitudes beyond a pole)
        lo, hi = sorted((lat0 + sign * 7.19, lat0 + sign * 7.21))
        a, b = bisect(lambda y: math.fabs(lat0 - y) > reach, lo, hi)
        out.extend([("band/%s/lo" % name, a), ("band/%s/hi" % name, b)])
        for f in SLIVER:
            out.append(("sliver/%s/%g" % (name, f), lat0 + sign * ((1.0 + f) * reach)))
        lat = lat0 + sign * reach
        if math.fabs(lat0 - lat) == reach:
            out.append(("band_eq/%s" % name, lat))
    return out


def clusters(rng):
    """observations along 50 S, 30 degrees apart, with exactly LENGTHS particles around them, and five overlapping ones
    around one particle"""
    obs, rows = [], []
    lon = -170.0
    centres = []
    for k, n in enumerate(LENGTHS):
        if k > 0 and LENGTHS[k - 1] == n:        # the identical observation: the same place
            centres.append(centres[-1])
        else:
            centres.append(lon)
            lon += 30.0
        obs.append(("list/%d%s" % (n, "b" if centres[-1] in centres[:-1] else ""), centres[-1], -50.0, Z_OBS))
    seen = set()
    for (tag, olon, olat, _), n in zip(obs, LENGTHS):
        if olon in seen:
            continue
        seen.add(olon)
        for j in range(n):
            mass = (-1.0) ** int(rng.integers(2)) * 10.0 ** rng.uniform(-8.0, 8.0)
            rows.append((olon + rng.uniform(-0.5, 0.5), olat + rng.uniform(-0.4, 0.4), RA.P(Z_OBS + rng.uniform(-3.0, 3.0)), T,
                         mass, 0.0, "cluster/%d/%d" % (n, j)))
    for k in range(5):
        obs.append(("five/%d" % k, lon + 0.1 * k, -50.0 + 0.05 * k, Z_OBS))
    rows.append((lon + 0.2, -49.9, RA.P(Z_OBS), T, 3.25, 0.0, "five"))
    order = rng.permutation(len(rows))            # the clusters' particles interleaved
    return obs, [rows[i] for i in order]


@functools.lru_cache(maxsize=None)
def main():
    """(atm, tags of the placed particles, observations [(tag, lon, lat, z)]) of the main case"""
    rng = np.random.default_rng(20260)
    p_mid = RA.P(Z_OBS)
    rows = []      # (lon, lat, p, time, mass or None, flag, tag)

    def put(lon, lat, tag, p=p_mid, time=T, flag=0.0):
        rows.append((lon, lat, p, time, None, flag, tag))

    for site in EDGE_SITES:
        for name, lon, lat, side in _distance_pairs(site):
            put(lon, lat, "dist/%s/%s/%s" % (site, name, side))
        for kind, lat in _band_points(site):
            put(SITES[site][0], lat, kind.replace("/", "/%s/" % site, 1))
        put(*SITES[site], "centre/%s" % site)
    for site in ("depth", "time", "wfn"):
        put(*SITES[site], "centre/%s" % site)
    # depth: at the site, p on the host's bounds of the layer and either side
    lon, lat = SITES["depth"]
    for dz in (1.5, DZ, 5e-324):
        for name, sign in (("top", 1.0), ("bottom", -1.0)):
            for p, side in around(RA.P(Z_OBS + sign * dz)):
                put(lon, lat, "depth/%g/%s/%s" % (dz, name, side), p=p)
    # time: the ends of the step window and of the station windows
    lon, lat = SITES["time"]
    stamps = sorted({T0, T1} | {v for w in STATION_WINDOWS.values() for v in w if abs(v) < 1e99})
    for v in stamps:
        for t, side in around(v):
            put(lon, lat, "time/%g/%s" % (v, side), time=t)
    # weighting function: on, below and above every node, below the first and above the last node
    lon, lat = SITES["wfn"]
    for k, (kz, exact, below, above) in enumerate(nodes()):
        for p, side in ((exact, "on"), (below, "below"), (above, "above")):
            put(lon, lat, "node/%d/%s" % (k, side), p=p)
    put(lon, lat, "node/under", p=RA.P(1.0))
    put(lon, lat, "node/over", p=RA.P(28.0))
    # station flags
    lon, lat = SITES["flags"]
    for rep in range(2):
        for f in FLAGS:
            put(lon + 0.01 * rep, lat, "flag/%r/%d" % (f, rep), flag=f)
    cluster_obs, cluster_rows = clusters(rng)
    rows += cluster_rows
    tags = [r[6] for r in rows]
    npl = len(rows)
    n = npl + N_BACKGROUND
    # the background: between 58 N and 76 N, out of reach of every site; a tenth of it outside the time window
    atm = {"lon": np.concatenate([[r[0] for r in rows], rng.uniform(-180.0, 180.0, N_BACKGROUND)]),
           "lat": np.concatenate([[r[1] for r in rows], rng.uniform(58.0, 76.0, N_BACKGROUND)]),
           "p": np.concatenate([[r[2] for r in rows], RA.P0 * np.exp(-rng.uniform(2.0, 25.0, N_BACKGROUND) / RA.H0)])}
    tb = np.full(N_BACKGROUND, T)
    tb[::10] = T_OUT
    atm["time"] = np.concatenate([[r[3] for r in rows], tb])
    q = np.zeros((len(NAMES), n))
    q[QM] = 0.5 + rng.random(n)
    for i, r in enumerate(rows):
        if r[4] is not None:
            q[QM][i] = r[4]
        q[QSTAT][i] = r[5]
    atm["q"] = q
    for k in ("lon", "lat", "p", "time"):
        atm[k] = np.ascontiguousarray(atm[k], dtype=np.float64)
    obs = [("site/" + s, SITES[s][0], SITES[s][1], Z_OBS) for s in SITES] + cluster_obs
    wild = np.random.default_rng(99)
    for k in range(6):      # among the background
        obs.append(("wild/%d" % k, float(wild.uniform(-180.0, 180.0)), float(wild.uniform(60.0, 74.0)), float(wild.uniform(5.0, 20.0))))
    return atm, tags, obs


def obs_arrays(obs):
    return tuple(np.array([o[k] for o in obs], dtype=np.float64) for k in (1, 2, 3))


def tiled(nobs):
    """nobs observations [(tag, lon, lat, z)]: crowded and edge observations at TILE_SLOTS and nobs - 1, the other
    special ones from index 1, fillers without a particle in reach everywhere else (odd indices: 66 S, the band rejects;
    even: on the clusters' parallel, 15 degrees east of one, the distance rejects)"""
    _, _, obs = main()
    by = {o[0]: o for o in obs}
    keys = ["list/65", "list/129", "list/128", "site/mid", "list/64", "list/63"]
    out = [None] * nobs
    for slot, key in zip(TILE_SLOTS, keys):
        if slot < nobs:
            out[slot] = by[key]
    if nobs > 1:
        out[nobs - 1] = by["list/65b"]
    rest = [o for o in obs if o[0] not in keys + ["list/65b"]]
    at = 1
    for o in rest:
        while at < nobs and out[at] is not None:
            at += 1
        if at >= nobs or nobs - at < 200:       # (only where the call has room for them in front of slot 255)
            break
        out[at] = o
        at += 1
    for i in range(nobs):
        if out[i] is None:
            out[i] = ("filler/%d" % i, -180.0 + (0.37 * i) % 360.0, -66.0, Z_OBS) if i % 2 else \
                     ("filler/%d" % i, -155.0 + 30.0 * ((i // 2) % 6), -50.0, Z_OBS)
    return out


def sample_calls():
    """{name: (t0, t1, observations, dx, dz, kernel name)} of the main case"""
    _, _, obs = main()
    calls = {"main": (T0, T1, obs, DX, DZ, "nk5")}
    for dz in (0.0, -999.0, 5e-324, 1.5):
        calls["dz/%g" % dz] = (T0, T1, obs, DX, dz, "nk0")
    for name in kernels():
        calls["kernel/" + name] = (T0, T1, obs, DX, -999.0, name)
    calls["kernel/rep3/dz"] = (T0, T1, obs, DX, DZ, "rep3")
    dx, _, _ = equal_radius()
    for name, v in (("below", down(dx)), ("on", dx), ("above", up(dx))):
        calls["dx_eq/" + name] = (T0, T1, obs, v, DZ, "nk2")
    calls["t_point"] = (T, T, obs, DX, DZ, "nk2")
    calls["t_reversed"] = (T1, T0, obs, DX, DZ, "nk2")
    for nobs in NOBS:
        calls["nobs/%d" % nobs] = (T0, T1, tiled(nobs), DX, DZ, "nk5")
    return calls


def station_calls():
    """{name: (site, lon, lat, r, s0, s1)} of the main case, all without a flag quantity (nothing changes)"""
    calls = {}
    for site in EDGE_SITES:
        calls["dist/" + site] = (site,) + SITES[site] + (DX,) + EVER
    for name, (s0, s1) in STATION_WINDOWS.items():
        calls["window/" + name] = ("time",) + SITES["time"] + (DX, s0, s1)
    r, site, _ = equal_radius()
    for name, v in (("below", down(r)), ("on", r), ("above", up(r))):
        calls["r_eq/" + name] = (site,) + SITES[site] + (v,) + EVER
    return calls


@functools.lru_cache(maxsize=None)
def equal_radius():
    """(dx, site, index of the placed particle) with dx * dx == dist2(site, particle) to the bit: sqrt(dist2) of a placed
    pair's inner particle, or a double next to it"""
    atm, tags, _ = main()
    for i, tag in enumerate(tags):
        part = tag.split("/")
        if part[0] != "dist" or part[2] not in ("east", "west", "ne", "sw", "across"):
            continue
        lon0, lat0 = SITES[part[1]]
        s = dist2(lon0, lat0, float(atm["lon"][i]), float(atm["lat"][i]))
        if s > DX * DX:
            continue
        dx = math.sqrt(s)
        for v in (dx, down(dx), up(dx)):
            if v * v == s and down(v) * down(v) < s < up(v) * up(v):
                return v, part[1], i
    raise AssertionError("no placed pair has a radius with dx * dx == dist2")


# ---------------------------------------------------------------------------
# particle counts, not-finite particles
# ---------------------------------------------------------------------------

COUNT_OBS = [("hits", 20.0, 30.0, Z_OBS), ("some", -150.0, -20.0, Z_OBS), ("none", 90.0, 60.0, Z_OBS)]


@functools.lru_cache(maxsize=None)
def count_case(n):
    """(atm, indices placed at the first observation): n particles, all but the placed ones far from every observation
    (60 S to 70 S) or around the second one; in the large case BORDER are placed, block 2 (512 .. 767) is outside the
    time window except for its last particle, blocks 3 and 4 entirely -- and all three lie at the first observation."""
    rng = np.random.default_rng(1000 + n)
    lon, lat = rng.uniform(-180.0, 180.0, n), rng.uniform(-70.0, -60.0, n)
    p = RA.P0 * np.exp(-rng.uniform(6.0, 14.0, n) / RA.H0)
    time = np.full(n, T)
    time[rng.random(n) < 0.1] = T_OUT
    near = rng.random(n) < 0.02
    lon[near], lat[near] = -150.0 + rng.uniform(-6.0, 6.0, int(near.sum())), -20.0 + rng.uniform(-6.0, 6.0, int(near.sum()))
    placed = sorted({0, n - 1} | {i for i in (254, 255) if i < n} | ({i for i in BORDER} if n > 16385 else set()))
    if n > 1280:
        blocks = np.arange(512, 1280)
        lon[blocks], lat[blocks], time[blocks] = 20.0, 30.0, T_OUT
        placed = sorted(set(placed) | {767})
    for i in placed:
        lon[i], lat[i], p[i], time[i] = 20.0 + 0.001 * (i % 7), 30.0, RA.P(Z_OBS), T
    q = np.zeros((len(NAMES), n))
    q[QM] = (-1.0) ** rng.integers(2, size=n) * 10.0 ** rng.uniform(-8.0, 8.0, n)
    atm = {"lon": lon, "lat": lat, "p": p, "time": time, "q": q}
    return atm, placed


@functools.lru_cache(maxsize=None)
def not_finite():
    """(atm, tags): 40 good particles around the first of COUNT_OBS, then NaN, +inf and -inf in time, lon, lat and p, one
    at a time in a particle that is otherwise at the observation, then a background.  No NaN in the flag quantity."""
    rng = np.random.default_rng(77)
    rows, tags = [], []
    for j in range(40):
        rows.append([20.0 + rng.uniform(-2.0, 2.0), 30.0 + rng.uniform(-2.0, 2.0), RA.P(Z_OBS + rng.uniform(-8.0, 8.0)), T])
        tags.append("good/%d" % j)
    for k, field in enumerate(("lon", "lat", "p", "time")):
        for v in (math.nan, math.inf, -math.inf):
            row = [20.0, 30.0, RA.P(Z_OBS), T]
            row[k] = v
            rows.append(row)
            tags.append("%s/%r" % (field, v))
    for j in range(100):
        rows.append([rng.uniform(-180.0, 180.0), rng.uniform(-70.0, -60.0), RA.P(rng.uniform(2.0, 20.0)), T if j % 5 else T_OUT])
        tags.append("background/%d" % j)
    order = np.concatenate([rng.permutation(52), np.arange(52, len(rows))])      # bad particles among the good ones
    a = np.array(rows)[order]
    n = len(a)
    q = np.zeros((len(NAMES), n))
    q[QM] = 0.5 + rng.random(n)
    atm = {"lon": a[:, 0].copy(), "lat": a[:, 1].copy(), "p": a[:, 2].copy(), "time": a[:, 3].copy(), "q": q}
    return atm, [tags[i] for i in order]


# ---------------------------------------------------------------------------
# the reference's results, once per process
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def xyz_of(case):
    return RA.cartesian(particles(case))


def particles(case):
    if case == "main":
        return main()[0]
    if case == "not_finite":
        return not_finite()[0]
    return count_case(int(case))[0]


@functools.lru_cache(maxsize=None)
def sample_reference(case, name):
    """(count, mass, stages, hits) of refanalysis.sample_obs for a call of a case"""
    if case == "main":
        t0, t1, obs, dx, dz, kernel = sample_calls()[name]
    else:
        t0, t1, obs, dx, dz, kernel = T0, T1, COUNT_OBS, DX, (DZ if name == "layer" else -999.0), ("nk5" if name == "layer" else "nk0")
    lon, lat, z = obs_arrays(obs)
    if len(obs) == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0), [], []
    return RA.sample_obs(particles(case), t0, t1, lon, lat, z, dx, dz, QM, kernels()[kernel], xyz_of(case))


def sample_arguments(case, name):
    """what Simulation.sample_obs is called with"""
    if case == "main":
        t0, t1, obs, dx, dz, kernel = sample_calls()[name]
    else:
        t0, t1, obs, dx, dz, kernel = T0, T1, COUNT_OBS, DX, (DZ if name == "layer" else -999.0), ("nk5" if name == "layer" else "nk0")
    return (t0, t1) + obs_arrays(obs) + (dx, dz, kernels()[kernel]), [o[0] for o in obs]


@functools.lru_cache(maxsize=None)
def station_reference(case, lon, lat, r, s0, s1, qnt_stat):
    """(listed, rows, q afterwards, skipped) of refanalysis.station_hits"""
    return RA.station_hits(particles(case), T, DT_MOD, lon, lat, r, s0, s1, qnt_stat, xyz_of(case))


def deciders(case, name, i, limit=4):
    """The placed particles on which a wrong decision about observation i of a call would show, by the decision, from
    the reference arithmetic: {"band alone": in the time window and the layer, chord <= dx, beyond the band; "distance
    alone": ... in the band, chord > dx, by less than 1 %; "layer alone"; "on an equality": hits with dist2 == dx^2,
    fabs(ob_lat - lat) == reach_lat, p on a bound of the layer or time on an end of the window}"""
    args, _ = sample_arguments(case, name)
    t0, t1, lon, lat, z, dx, dz = args[:7]
    atm = particles(case)
    tags = main()[1] if case == "main" else (not_finite()[1] if case == "not_finite" else [])
    lon0, lat0, reach = float(lon[i]), float(lat[i]), reach_lat(dx)
    p_top, p_bottom = RA.P(float(z[i]) + dz), RA.P(float(z[i]) - dz)
    out = {"band alone": [], "distance alone": [], "layer alone": [], "on an equality": []}
    for j, tag in enumerate(tags):
        tp, plon, plat, p = (float(atm[k][j]) for k in ("time", "lon", "lat", "p"))
        if tp < t0 or tp > t1:
            continue
        s, dlat = dist2(lon0, lat0, plon, plat), math.fabs(lat0 - plat)
        band, near, layer = not dlat > reach, not s > dx * dx, not (dz > 0 and (p > p_bottom or p < p_top))
        if near and layer and not band:
            out["band alone"].append(tag)
        if band and layer and not near and not s > 1.01 * dx * 1.01 * dx:
            out["distance alone"].append(tag)
        if band and near and not layer:
            out["layer alone"].append(tag)
        if band and near and layer and (s == dx * dx or dlat == reach or tp in (t0, t1) or (dz > 0 and p in (p_top, p_bottom))):
            out["on an equality"].append(tag)
    return {k: v[:limit] for k, v in out.items() if v}


# ---------------------------------------------------------------------------
# facts: what the inputs do, from the reference arithmetic alone
# ---------------------------------------------------------------------------

def member(site, i, dx=DX, dz=DZ, z=Z_OBS, t0=T0, t1=T1):
    """(in the time window, in the band, chord <= dx, in the layer) of particle i of the main case for an observation at
    `site`, each decision on its own"""
    atm = main()[0]
    lon0, lat0 = SITES[site]
    tp, lon, lat, p = (float(atm[k][i]) for k in ("time", "lon", "lat", "p"))
    return (not (tp < t0 or tp > t1), not math.fabs(lat0 - lat) > reach_lat(dx), not dist2(lon0, lat0, lon, lat) > dx * dx,
            not (dz > 0 and (p > RA.P(z - dz) or p < RA.P(z + dz))))


def facts_main():
    atm, tags, obs = main()
    f = {"case": "main", "particles": len(atm["time"]), "placed": len(tags), "observations": len(obs)}
    where = {tag: i for i, tag in enumerate(tags)}
    # distance: per (site, direction) two adjacent doubles, the decision differs
    pairs = 0
    for tag, i in where.items():
        part = tag.split("/")
        if part[0] == "dist" and part[3] == "lo":
            j = where["/".join(part[:3] + ["hi"])]
            k = "lat" if atm["lon"][i] == atm["lon"][j] else "lon"
            assert up(float(atm[k][i])) == float(atm[k][j]), tag
            assert member(part[1], i)[2] != member(part[1], j)[2], tag
            pairs += 1
    f["distance_pairs"] = pairs
    dx, site, i = equal_radius()
    s = dist2(*SITES[site], float(atm["lon"][i]), float(atm["lat"][i]))
    f["dx_equal"] = {"dx": dx, "site": site, "particle": tags[i], "equal": dx * dx == s, "below": down(dx) * down(dx) < s,
                     "above": up(dx) * up(dx) > s}
    # band: adjacent doubles either side, the sliver, equality
    band, sliver, equal = 0, {}, []
    for tag, i in where.items():
        part = tag.split("/")
        if part[0] == "band" and part[3] == "lo":
            j = where["/".join(part[:3] + ["hi"])]
            assert up(float(atm["lat"][i])) == float(atm["lat"][j]), tag
            assert member(part[1], i)[1] != member(part[1], j)[1], tag
            band += 1
        if part[0] == "sliver":
            m = member(part[1], i)
            if m[0] and not m[1] and m[2] and m[3]:
                sliver[part[1]] = sliver.get(part[1], 0) + 1
        if part[0] == "band_eq":
            assert math.fabs(SITES[part[1]][1] - float(atm["lat"][i])) == reach_lat(DX) and member(part[1], i)[1]
            equal.append(part[1] + "/" + part[2])
    f["band_pairs"], f["band_rejects_what_the_chord_accepts"], f["band_equal"] = band, sliver, equal
    # depth
    depth = {}
    for dz in (1.5, DZ, 5e-324):
        for name in ("top", "bottom"):
            got = tuple(member("depth", where["depth/%g/%s/%s" % (dz, name, side)], dz=dz)[3] for side in ("below", "on", "above"))
            depth["%g/%s" % (dz, name)] = got
    f["depth_below_on_above"] = depth
    # time
    f["time_below_on_above"] = {"%g" % v: tuple(member("time", where["time/%g/%s" % (v, side)])[0] for side in ("below", "on", "above"))
                                for v in (T0, T1)}
    # weighting function
    zs = {tag: RA.Z(float(atm["p"][i])) for tag, i in where.items() if tag.startswith("node/")}
    kz = [n[0] for n in nodes()]
    f["nodes_below_on_above"] = [(zs["node/%d/below" % k] < kz[k], zs["node/%d/on" % k] == kz[k],
                                  zs["node/%d/above" % k] > kz[k]) for k in range(len(kz))]
    f["under_first_node"], f["over_last_node"] = zs["node/under"] < kz[0], zs["node/over"] > kz[-1]
    return f


def facts_lists():
    """counts of the clusters' observations, the order of addition, the particle in five cylinders (the call `main`)"""
    atm, tags, obs = main()
    count, mass, stages, hits = sample_reference("main", "main")
    names = [o[0] for o in obs]
    f = {"counts": {n: int(count[names.index(n)]) for n in names if n.startswith(("list/", "five/"))}}
    order = {}
    for n, idx in zip(names, hits):
        if len(idx) >= 63:
            kz, kw = kernels()["nk5"]
            vals = [RA.kernel_weight(list(kz), list(kw), float(atm["p"][i])) * float(atm["q"][QM][i]) for i in idx.tolist()]
            fwd = bwd = 0.0
            for v in vals:
                fwd += v
            for v in reversed(vals):
                bwd += v
            order[n] = fwd != bwd
    f["order_of_addition_shows"] = order
    seen = np.zeros(len(atm["time"]), dtype=int)
    for idx in hits:
        seen[idx] += 1
    f["most_cylinders_around_a_particle"] = int(seen.max())
    f["stages_remove"] = [bool(any(s[k] > s[k + 1] for s in stages)) for k in range(3)]
    return f
