"""Edge inputs of the axis searches: warped meteo axes and particles on grid lines.

The lean kernels set up a stencil from a first guess per axis (lon_fast, lat_fast, p_fast, raw_cell_fast in
mptrac_amd/csrc/mphip_device.hpp) and check it once; a lane whose check fails takes the general code, which corrects a
guess of its own (lat_guess / p_guess + locate_from).  On the evenly spaced axes of synth.make_axes with scattered
particles none of these corrections ever runs.  Here:

  warp_met         the analytic fields of synthetic_met on uneven latitudes (either direction) and on a pressure ladder
                   whose lowest levels share bins of the pressure table (either direction)
  edge_particles   particles on every node of every axis, one ulp beside it, on the ends of the axes, beyond them, on
                   the pressure table's bin edges, and on nodes of two and three axes at once
  preconditions    what these inputs do to the first guesses, restated in numpy from upload_axes / lat_guess / p_guess,
                   so that a test can assert that its inputs reach the branches it is about
"""
import numpy as np

import cases
import refmodules as R
from mptrac_amd.synth import FIELDS_ML, Met

GRIDS = [(36, 19, 40), "C1"]
LON0 = [-180.0, 0.0]
LAT_AXES = ("even", "uneven", "reversed_uneven")
P_AXES = ("ladder", "crowded", "crowded_ascending")
# every warped pair (latitude axis, pressure axis) the tests run: both warps in both directions, and each warp alone
WARPS = [("uneven", "crowded"), ("reversed_uneven", "crowded_ascending"), ("reversed_uneven", "crowded"),
         ("uneven", "crowded_ascending"), ("uneven", "ladder"), ("even", "crowded")]
N_CROWDED = 12          # levels at the bottom of the crowded ladder ...
CROWDED_STEP = 0.0015   # ... 0.15 % apart (ERA5's lowest L137 levels: 0.2-0.3 %; a bin of the pressure table: 0.4-0.8 %)
BIN_EDGES = (512.0, 256.0, 128.0)      # powers of two: edges of table bins, and nodes of the crowded ladder
LAT_AMP = 0.9           # degrees


def uneven_lat(ny, amp=LAT_AMP):
    """-90 + 180 s + amp sin(6 pi s), s = j / (ny - 1), the ends pinned to the poles.  Monotonic for amp < 30 / pi."""
    s = np.arange(ny, dtype=np.float64) / (ny - 1)
    lat = -90.0 + 180.0 * s + amp * np.sin(6.0 * np.pi * s)
    lat[0], lat[-1] = -90.0, 90.0
    assert np.all(np.diff(lat) > 0)
    return lat


def crowded_p(p):
    """From a descending ladder: the N_CROWDED lowest levels CROWDED_STEP apart, the rest evenly spaced in log p up to
    the old top, and the nodes nearest to 512, 256 and 128 hPa moved onto them."""
    n = len(p)
    q = np.array(p, dtype=np.float64)
    q[:N_CROWDED] = p[0] * (1.0 - CROWDED_STEP) ** np.arange(N_CROWDED)
    q[N_CROWDED:] = np.exp(np.linspace(np.log(q[N_CROWDED - 1]), np.log(p[-1]), n - N_CROWDED + 1)[1:])
    for edge in BIN_EDGES:
        j = int(np.argmin(np.abs(np.log(q / edge))))
        assert j >= N_CROWDED
        q[j] = edge
    assert np.all(np.diff(q) < 0)
    return q


def warp_met(met, lat="even", p="ladder", lat_amp=LAT_AMP):
    """A synth.Met with the fields of `met` (analytic in the node indices, so a wrong index reads another value) on other
    axes.  lat: "even", "uneven" (uneven_lat) or "reversed_uneven" (north to south, fields flipped with it);
    p: "ladder", "crowded" (crowded_p) or "crowded_ascending" (top first, pressure-level fields flipped with it)."""
    assert lat in LAT_AXES and p in P_AXES and met.lat[0] < met.lat[-1] and met.p[0] > met.p[-1]
    f3, f2 = dict(met.f3), dict(met.f2)
    lat_axis = met.lat if lat == "even" else uneven_lat(met.ny, lat_amp)
    if lat == "reversed_uneven":
        lat_axis = lat_axis[::-1]
        f3 = {k: v[:, ::-1, :] for k, v in f3.items()}
        f2 = {k: v[:, ::-1] for k, v in f2.items()}
    p_axis = met.p if p == "ladder" else crowded_p(met.p)
    if p == "crowded_ascending":
        p_axis = p_axis[::-1]
        f3 = {k: (v if k in FIELDS_ML else v[:, :, ::-1]) for k, v in f3.items()}
    out = Met(met.time, met.lon, lat_axis, p_axis, f3, f2, met.coord_type)
    for d in (out.f3, out.f2):
        for a in d.values():
            assert np.array_equal(a[-1], a[0], equal_nan=True)      # the periodic column is still a copy of column 0
    return out


def _both_sides(x):
    return [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]


def edge_particles(atm, met):
    """Overwrites the first particles of `atm` (in place) with positions on and beside the grid lines of `met`; a
    coordinate that is not named keeps the scattered value the particle had.  Returns the number placed."""
    lon_ax, lat_ax, p_ax = met.lon, met.lat, met.p
    lon_first, lon_last = lon_ax[0], lon_ax[-1]
    p_max, p_min = p_ax.max(), p_ax.min()
    lon, lat, p = [], [], []
    for x in lon_ax:                                # every node and its two neighbours among the doubles
        lon += _both_sides(x)
    lon += [lon_first, lon_last, lon_last - 360.0, lon_first + 360.0, 360.0, -360.0, 720.25]
    for y in lat_ax:
        lat += [v for v in _both_sides(y) if abs(v) <= 90.0]
    lat += [lat_ax[0], lat_ax[-1], 90.0, -90.0, np.nextafter(90.0, 0.0), np.nextafter(-90.0, 0.0)]
    for z in p_ax:
        p += _both_sides(z)
    p += [p_max, np.nextafter(p_max, -np.inf), np.nextafter(p_max, np.inf), 1.1 * p_max,
          p_min, np.nextafter(p_min, -np.inf), np.nextafter(p_min, np.inf), 0.5 * p_min]
    for edge in BIN_EDGES:
        p += _both_sides(edge)
    lo, hi = p_ax[:-1], p_ax[1:]                    # inside every interval: the crowded ones hold no scattered particle
    for f in (0.25, 0.5, 0.75):
        p += list(lo + f * (hi - lo))
    triples = [(x, None, None) for x in lon] + [(None, y, None) for y in lat] + [(None, None, z) for z in p]
    # nodes of two axes and of all three at once; the last ones three times each: ties of module_sort's keys
    nx, ny, npl = len(lon_ax), len(lat_ax), len(p_ax)
    for k in range(24):
        i, j, l = (5 * k + 1) % nx, (7 * k + 2) % ny, (3 * k) % npl
        triples += [(lon_ax[i], lat_ax[j], None), (lon_ax[i], None, p_ax[l]), (None, lat_ax[j], p_ax[l])]
        triples += [(lon_ax[i], lat_ax[j], p_ax[l])] * 3
    for j in (0, ny - 1):                           # corners of the grid
        for l in (0, npl - 1):
            triples += [(lon_ax[i], lat_ax[j], p_ax[l]) for i in (0, nx - 1)]
    placed = len(triples)
    assert placed < len(atm["lon"]), (placed, len(atm["lon"]))
    for k, (x, y, z) in enumerate(triples):
        if x is not None:
            atm["lon"][k] = x
        if y is not None:
            atm["lat"][k] = y
        if z is not None:
            atm["p"][k] = z
    for k in ("lon", "lat", "p"):
        assert np.all(np.isfinite(atm[k]))
    return placed


def _bisect(xx, x):
    """locate_irr (mptrac.c:3495-3521), the bisection as written: tests/refmodules.py"""
    return R.locate_irr(xx, x)


def p_table(p_ax):
    """upload_axes: one entry per value of (bits of p) >> 45 between the smallest and the largest node -- the bisection's
    index of the bin's lower edge.  Returns (first bin, table)."""
    bins = np.sort(np.asarray(p_ax, dtype=np.float64)).view(np.int64) >> 45
    edges = (np.arange(bins[0], bins[-1] + 1, dtype=np.int64) << 45).view(np.float64)
    return int(bins[0]), _bisect(p_ax, edges)


def preconditions(met, atm, first=0):
    """What the inputs do to the first guesses, over the particles from index `first` on (the scattered ones)."""
    bins = met.p.view(np.int64) >> 45
    lat = np.clip(atm["lat"][first:], met.lat.min(), met.lat.max())
    guess = np.clip(np.trunc((lat - met.lat[0]) * ((met.ny - 1) / (met.lat[-1] - met.lat[0]))).astype(np.int64), 0, met.ny - 2)
    miss = np.abs(guess - _bisect(met.lat, lat))
    base, table = p_table(met.p)
    pp = np.clip(atm["p"], met.p.min(), met.p.max())
    p_miss = np.abs(table[(pp.view(np.int64) >> 45) - base] - _bisect(met.p, pp))
    return {"nodes_in_one_bin": int(np.bincount(bins - bins.min()).max()),
            "bins_with_two_nodes": int(np.count_nonzero(np.bincount(bins - bins.min()) >= 2)),
            "node_on_bin_edge": bool(np.any((met.p.view(np.int64) & ((1 << 45) - 1)) == 0)),
            "lat_guess_wrong": int(np.count_nonzero(miss)), "lat_guess_wrong_fraction": float(np.mean(miss > 0)),
            "lat_guess_off_by_two_fraction": float(np.mean(miss >= 2)), "lat_guess_max_miss": int(miss.max()),
            "p_guess_wrong": int(np.count_nonzero(p_miss)), "p_guess_max_miss": int(p_miss.max())}


def assert_preconditions(met, atm, placed, lat, p):
    """The inputs reach the corrections (conditions on the inputs, not on the code under test).

    Pressure: three nodes in one bin of the table and a node on a bin edge, hence a table guess that is two intervals
    off for some particle -- locate_from walks more than one step.
    Latitude: node j of uneven_lat lies amp sin(6 pi s) degrees from the evenly spaced one, at most LAT_AMP = 0.9 degrees,
    which is less than one interval on every grid used here (1 and 10 degrees).  So the guess from the mean spacing
    misses by one interval at most, never by two, and it misses for a fraction f = 2 amp / (pi dlat) of evenly scattered
    particles (the mean of |sin|): 57 % on the one-degree grid, 5.7 % on the ten-degree grid.  Asserted: a miss for at
    least f / 2 of the scattered particles (29 % and 2.9 %; with the few hundred scattered particles of the small grid
    the count is 25 +- 5, so 5 % is not a bound the sample keeps), and that the largest miss is exactly one interval."""
    pre = preconditions(met, atm, placed)
    if p != "ladder":
        assert pre["nodes_in_one_bin"] >= 3 and pre["bins_with_two_nodes"] >= 2, pre
        assert pre["node_on_bin_edge"], pre
        assert pre["p_guess_max_miss"] >= 2, pre
    if lat != "even":
        expected = 2.0 * LAT_AMP / (np.pi * 180.0 / (met.ny - 1))
        assert pre["lat_guess_wrong_fraction"] >= 0.5 * expected and pre["lat_guess_max_miss"] == 1, (pre, expected)
    return pre


def setup(case, grid, lon0, lat, p, n=4096, seed=12345, over=None, **kw):
    """make_case on a warped grid with the edge particles: (ctl, clim, met0, met1, atm, placed)."""
    ctl, clim, m0, m1, atm = cases.make_case(case, n=n, grid=grid, lon0=lon0, seed=seed, **kw)
    ctl.update(over or {})
    m0, m1 = warp_met(m0, lat, p), warp_met(m1, lat, p)
    placed = edge_particles(atm, m0)
    assert_preconditions(m0, atm, placed, lat, p)
    return ctl, clim, m0, m1, atm, placed
