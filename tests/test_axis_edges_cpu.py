"""The reference side of the axis-search edge tests (tests/axis_cases.py): the oracle against the numpy restatement
tests/refmodules.py on every warped grid, with particles on the grid lines, one ulp beside them, on and beyond the ends
of the axes -- ADVECT 1, 2 and 4, module_sort's keys and order, module_meteo's fields, module_diff_meso's raw cell.
Two independent statements of the tie rules agree before the device is held to them (tests/test_gpu_axis_edges.py):
a coordinate on a node belongs to the interval whose lower value it is, the last node to the last interval, and
module_sort / module_diff_meso search the longitude as it is, not wrapped.  Bars as in
tests/test_oracle_second_opinion.py: 1e-13 relative, indices and single-precision values equal."""
import ctypes as C
import functools

import numpy as np
import pytest

import axis_cases as A
import cases
import refmodules as R
from oracle import binding as B

TOL = 1e-13
# (grid, lon0, latitude axis, pressure axis): every warp on the small grid, both full warps on the one-degree grid
COMBOS = [(g, lon0, lat, p) for g in A.GRIDS for lon0 in A.LON0 for lat, p in (A.WARPS if g != "C1" else A.WARPS[:2])]
IDS = ["%s-lon%d-%s-%s" % (g if isinstance(g, str) else "x".join(map(str, g)), lon0, lat, p) for g, lon0, lat, p in COMBOS]
combos = pytest.mark.parametrize("combo", COMBOS, ids=IDS)


@functools.lru_cache(maxsize=None)
def _inputs(combo):
    grid, lon0, lat, p = combo
    return A.setup("meteo", grid, lon0, lat, p, n=4096 if grid == "C1" else 1024, seed=4711)


def _oracle(combo, **over):
    ctl, clim, m0, m1, atm, placed = _inputs(combo)
    o = B.Oracle(dict(ctl, **over), clim, m0, m1, atm)
    o.timesteps_init()
    t = cases.step_times(o.ctl)[1]          # (the first call of the time loop has dt = 0)
    o.module("timesteps", t)
    return o, R.Ref(o.ctl, clim, m0, m1), placed


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))


@combos
def test_inputs_reach_the_corrections(combo):
    """axis_cases.setup asserts the preconditions; here also that the edge particles are where they should be."""
    _, _, m0, m1, atm, placed = _inputs(combo)
    pre = A.preconditions(m0, atm, placed)
    assert np.array_equal(m0.lat, m1.lat) and np.array_equal(m0.p, m1.p)
    assert set(m0.lon) <= set(atm["lon"]) and set(m0.lat) <= set(atm["lat"]) and set(m0.p) <= set(atm["p"])
    on = np.isin(atm["lon"], m0.lon) & np.isin(atm["lat"], m0.lat) & np.isin(atm["p"], m0.p)
    assert np.count_nonzero(on) >= 24 * 3
    assert pre["lat_guess_max_miss"] <= 1
    for f in m0.f3.values():
        assert np.array_equal(f[-1], f[0])


@pytest.mark.parametrize("axis", ["lat", "p"])
@combos
def test_a_node_belongs_to_the_interval_it_opens(combo, axis):
    """locate_irr on the nodes themselves and one ulp beside them, restatement and oracle: on an ascending axis node k
    gives k, on a descending axis k - 1 (either way the interval whose lower VALUE the node is), the ends clamp to
    0 and n - 2, and the neighbours among the doubles fall on either side."""
    m0 = _inputs(combo)[2]
    xx = getattr(m0, axis)
    n = len(xx)
    k = np.arange(n)
    asc = xx[0] < xx[-1]
    on = R.locate_irr(xx, xx)
    below, above = R.locate_irr(xx, np.nextafter(xx, -np.inf)), R.locate_irr(xx, np.nextafter(xx, np.inf))
    if asc:
        assert np.array_equal(on, np.minimum(k, n - 2)) and np.array_equal(above, on)
        assert np.array_equal(below, np.clip(k - 1, 0, n - 2))
    else:
        assert np.array_equal(on, np.clip(k - 1, 0, n - 2)) and np.array_equal(above, on)
        assert np.array_equal(below, np.minimum(k, n - 2))
    L = B.lib()
    ptr = xx.ctypes.data_as(C.POINTER(C.c_double))
    for x, want in ((xx, on), (np.nextafter(xx, -np.inf), below), (np.nextafter(xx, np.inf), above)):
        assert [L.orc_locate_irr(ptr, n, float(v)) for v in x] == list(want)


@pytest.mark.parametrize("advect", [4, 2, 1])
@combos
def test_advect(combo, advect):
    o, ref, _ = _oracle(combo, advect=advect)
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    o.module("advect")
    time, lon, lat, p = ref.advect(*s0, o.dt.copy())
    assert np.array_equal(time, o.time)
    assert np.all(np.isfinite(o.lon)) and np.all(np.isfinite(o.lat)) and np.all(np.isfinite(o.p))
    assert _rel(lon, o.lon) <= TOL and _rel(lat, o.lat) <= TOL and _rel(p, o.p) <= TOL
    assert np.max(np.abs(lon - s0[1])) > 1e-3


@combos
def test_sort_keys_and_a_stable_order(combo):
    o, ref, placed = _oracle(combo)
    lon, lat, p, q0 = o.lon.copy(), o.lat.copy(), o.p.copy(), o.q.copy()
    keys, perm = o.sort()
    want = ref.sort_keys(lon, lat, p)
    assert np.array_equal(keys, want)
    order = np.argsort(want, kind="stable")
    assert np.array_equal(perm, order)
    assert np.array_equal(o.lon, lon[order]) and np.array_equal(o.p, p[order]) and np.array_equal(o.q, q0[:, order])
    assert len(np.unique(want[:placed])) <= placed - 48                   # (the ties among the on-node particles are there)


@combos
def test_meteo_fields(combo):
    o, ref, _ = _oracle(combo)
    names = cases.CASE_QUANTITIES["meteo"]
    o.module("meteo")
    want = ref.meteo(o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    checked = 0
    for row, name in enumerate(names):
        if name in ("m", "rp", "rhop"):
            continue
        got = o.q[row]
        fin = np.isfinite(got)                      # (sst is NaN over land: the nearest-corner rule on both sides)
        assert np.array_equal(fin, np.isfinite(want[name])), name
        scale = max(float(np.max(np.abs(got[fin]))), 1e-300)
        assert float(np.max(np.abs(want[name][fin] - got[fin]))) <= TOL * scale, name
        assert np.ptp(got[fin]) > 0, name
        checked += 1
    assert checked == len(names) - sum(n in ("m", "rp", "rhop") for n in names)


@combos
def test_diff_meso_raw_cell(combo):
    """module_diff_meso's cell (locate_reg on the raw longitude, locate_irr on latitude and pressure) index by index
    against the oracle's own searches, and through the module: the single-precision perturbations are equal only if
    both sides took the statistics over the same sixteen corner values."""
    o, ref, _ = _oracle(combo)
    lon, lat, p = o.lon.copy(), o.lat.copy(), o.p.copy()
    o.module("diff_meso")
    rs = o.rs[:3 * o.n].copy()
    (ix, iy, iz), uvwp, new_lon, new_lat, new_p = ref.diff_meso(lon, lat, p, o.dt.copy(), np.zeros((o.n, 3), np.float32), rs)
    L = B.lib()
    m0 = _inputs(combo)[2]
    ptr = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in (m0.lon, m0.lat, m0.p)]
    assert [L.orc_locate_reg(ptr[0], m0.nx, float(v)) for v in lon] == list(ix)
    assert [L.orc_locate_irr(ptr[1], m0.ny, float(v)) for v in lat] == list(iy)
    assert [L.orc_locate_irr(ptr[2], m0.np, float(v)) for v in p] == list(iz)
    assert np.array_equal(uvwp, o.uvwp) and np.count_nonzero(o.uvwp) > o.n
    assert _rel(new_lon, o.lon) <= TOL and _rel(new_lat, o.lat) <= TOL and _rel(new_p, o.p) <= TOL
