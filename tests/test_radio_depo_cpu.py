"""tests/refradiodepo.py, the restatement of module_radio_depo, on the CPU: the cell arithmetic on the grid's edges, the bin
outside the grid, the ground decay over two unequal intervals, which nuclides deposit, and conservation."""
import math

import numpy as np

import refradio
import refradiodepo as RD

GRID = (-170.0, 175.0, 69, -80.0, 85.0, 33)       # 5 x 5 degree cells, not the whole globe
NCELL = 69 * 33
IDX = {n: k for k, n in enumerate(RD.NAMES)}


def test_cells_on_the_edges():
    lon = np.array([-170.0, -165.0, np.nextafter(-165.0, -180.0), np.nextafter(175.0, 0.0), 175.0, -170.0, 0.0, 0.0, 0.0,
                    np.nextafter(-170.0, -180.0), 180.0])
    lat = np.array([-80.0, -80.0, -80.0, np.nextafter(85.0, 0.0), 0.0, 85.0, -80.0, np.nextafter(-80.0, -90.0), -75.0,
                    0.0, 0.0])
    c = RD.ground_cell(GRID, lon, lat)
    assert c[0] == 0                                   # lower bounds inclusive
    assert c[1] == 33 and c[2] == 0                    # a cell border belongs to the upper cell
    # one ulp inside the upper bounds the quotient rounds to nx: the guard `ix >= nx` of the box arithmetic -> outside
    assert c[3] == NCELL and (lon[3] - GRID[0]) / ((GRID[1] - GRID[0]) / GRID[2]) == 69.0
    assert RD.ground_cell(GRID, [174.999], [84.999])[0] == NCELL - 1      # the last cell
    assert c[4] == NCELL and c[5] == NCELL             # upper bounds exclusive
    assert c[6] == 34 * 33 and c[7] == NCELL and c[8] == 34 * 33 + 1
    assert c[9] == NCELL and c[10] == NCELL
    # a grid whose cell width is not exact in binary: every cell's lower edge computed as the kernel would lies in a cell
    g = (0.0, 1.0, 10, 0.0, 0.7, 7)
    cc = RD.ground_cell(g, np.arange(10) * ((1.0 - 0.0) / 10), np.zeros(10))
    assert np.all((cc >= 0) & (cc < 70)) and np.all(np.diff(cc) >= 0)


def _particles(n=4000, seed=5):
    rng = np.random.default_rng(seed)
    lon, lat = rng.uniform(-180.0, 180.0, n), rng.uniform(-90.0, 90.0, n)
    q = 10.0 ** rng.uniform(1.0, 5.0, (6, n))
    dt = np.where(np.arange(n) % 7 == 0, 0.0, 180.0)
    aux_w, aux_d = rng.uniform(0.5, 1.0, n), rng.uniform(0.9, 1.0, n)
    acts_w, acts_d = rng.uniform(size=n) < 0.4, rng.uniform(size=n) < 0.3
    return lon, lat, q, dt, aux_w, acts_w, aux_d, acts_d


def test_the_bin_outside_and_who_deposits():
    lon, lat, q, dt, aux_w, acts_w, aux_d, acts_d = _particles()
    q0 = q.copy()
    inv = RD.Inventory(GRID).step(0.0, q, IDX, lon, lat, dt, aux_w, acts_w, aux_d, acts_d)
    cell = RD.ground_cell(GRID, lon, lat)
    live = dt != 0
    outside = (cell == NCELL) & live
    assert (outside & acts_w).sum() > 20 and (outside & acts_d).sum() > 20
    for name in RD.DEPOSITING:
        k = IDX[name]
        w = np.where(acts_w & live, q0[k] - q0[k] * aux_w, 0.0)
        assert inv.wet[k][NCELL] > 0 and inv.dry[k][NCELL] > 0
        assert inv.wet[k][NCELL] == RD.serial_cell_sums(w, np.where(outside & acts_w, NCELL, -1), NCELL)[NCELL]
        assert np.array_equal(q[k][~live], q0[k][~live])                        # dt == 0: untouched
        assert np.array_equal(q[k][live & ~acts_w & ~acts_d], q0[k][live & ~acts_w & ~acts_d])
        assert np.all(q[k][live & (acts_w | acts_d)] < q0[k][live & (acts_w | acts_d)])
    for name in RD.NOBLE:
        k = IDX[name]
        assert np.array_equal(q[k], q0[k]) and not inv.wet[k].any() and not inv.dry[k].any()
    assert np.array_equal(inv.cells >= 0, live & (acts_w | acts_d))
    # an absent activity: its plane stays zero, the others do not change
    q1 = q0.copy()
    idx = dict(IDX, Acs137=-1)
    inv1 = RD.Inventory(GRID).step(0.0, q1, idx, lon, lat, dt, aux_w, acts_w, aux_d, acts_d)
    assert not inv1.wet[IDX["Acs137"]].any() and np.array_equal(q1[IDX["Acs137"]], q0[IDX["Acs137"]])
    assert np.array_equal(inv1.wet[IDX["Ai131"]], inv.wet[IDX["Ai131"]])


def test_ground_decay_over_two_unequal_intervals():
    lon, lat, q, dt, aux_w, acts_w, aux_d, acts_d = _particles(n=500)
    nothing = np.zeros(len(dt), dtype=bool)
    inv = RD.Inventory(GRID).step(100.0, q, IDX, lon, lat, dt, aux_w, acts_w, aux_d, acts_d)
    first = {k: (inv.wet[k].copy(), inv.dry[k].copy()) for k in range(6)}
    t1, t2 = 100.0 + 3.0 * 86400.0, 100.0 + 11.5 * 86400.0
    inv.step(t1, q, IDX, lon, lat, dt, aux_w, nothing, aux_d, nothing)
    inv.step(t2, q, IDX, lon, lat, dt, aux_w, nothing, aux_d, nothing)
    assert inv.t_inv == t2
    for name in RD.DEPOSITING:
        k = IDX[name]
        f1 = math.exp(-refradio.LAMBDA[k] * (t1 - 100.0))
        f2 = math.exp(-refradio.LAMBDA[k] * (t2 - t1))
        assert np.array_equal(inv.wet[k], first[k][0] * f1 * f2)            # each interval its own factor, in order
        assert np.array_equal(inv.dry[k], first[k][1] * f1 * f2)
        whole = math.exp(-refradio.LAMBDA[k] * (t2 - 100.0))
        assert np.allclose(inv.wet[k], first[k][0] * whole, rtol=1e-14, atol=0.0)
    k = IDX["Ai131"]                                                        # 11.5 days of an 8.0252-day half-life
    assert np.allclose(inv.wet[k].sum() / first[k][0].sum(), 0.5 ** (11.5 / 8.0252), rtol=1e-12)
    # decay_to alone does the same
    other = RD.Inventory(GRID)
    other.wet[k], other.t_inv = first[k][0].copy(), 100.0
    other.decay_to(t1)
    other.decay_to(t2)
    assert np.array_equal(other.wet[k], inv.wet[k])


def test_conservation():
    """without decay in between, what left the air is on the ground: 1e-12 of the initial activity"""
    lon, lat, q, dt, aux_w, acts_w, aux_d, acts_d = _particles(n=3000, seed=9)
    q0 = q.copy()
    inv = RD.Inventory(GRID)
    for _ in range(5):
        inv.step(50.0, q, IDX, lon, lat, dt, aux_w, acts_w, aux_d, acts_d)       # (the same time: no ground decay)
    for name in RD.DEPOSITING:
        k = IDX[name]
        total = math.fsum(q[k]) + math.fsum(inv.wet[k]) + math.fsum(inv.dry[k])
        assert abs(total - math.fsum(q0[k])) <= 1e-12 * math.fsum(q0[k]), name
        assert math.fsum(inv.wet[k]) > 0.05 * math.fsum(q0[k])
