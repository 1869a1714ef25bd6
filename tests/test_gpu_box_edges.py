"""The box a particle belongs to, on the device, for particles on cell faces, on the borders the arithmetic itself draws,
on the bounds of the box and on the ends of the time window (tests/box_cases.py; what these inputs reach is asserted on
the reference in tests/test_box_edges_cpu.py).

box_cell (mphip_kernels.hpp) through box_index_kernel (module_mixing, the chemistry grid, the gridded output's group
path), cell_slot_pairs_kernel with use_box (the gridded output's chain path), sort_key_kernel with BoxArgs and the step
kernel's EmitKeys; box_cell_of_height through mphip_box_sums.  A wrong cell is a discrete error: the placed particles
carry 1000 times the background's values, the ordered sums are compared with array_equal, and where a bar is a tolerance
(atomic sums, the weighting function of the gridded output, the chemistry grid, a time step) the test first shows on the
reference that one placed particle in the neighbouring cell moves a result by far more than the bar.

The particles are used as uploaded (no time step moves them), in the caller's order and in the locality order (a time
step at the earliest particle time, in which nobody has a time step yet, only stores them).  Each comparison prints one
"BOX_EDGE {json}" line before it asserts.  tests/test_gpu_box_edges_exact.py runs the functions of this file in the
reference-rounding build."""
import functools
import json

import numpy as np
import pytest

import box_cases as BC
import cases
import refanalysis as RA
import refmodules as RM
from mptrac_amd import hip
from oracle import binding as B

pytestmark = pytest.mark.gpu

T, DT = BC.T, BC.DT_MOD
MIXED = (BC.QM, BC.QVMR, BC.QAOA)
ORDERS = ("external", "locality")


def report(**row):
    print("BOX_EDGE " + json.dumps(row))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    atm, npl, tags = BC.particles(name, T, DT)
    return atm, npl, tags


def _simulation(name, nens, order, **over):
    """the particles of grid `name` on the device, bit for bit, in the order asked for"""
    atm, _, _ = _inputs(name)
    ctl, clim, m0, m1 = BC.setup(name, nens, **over)
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.set_option("locality_sort_interval", 1 if order == "locality" else 0)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    if order == "locality":
        s.run_timestep(float(atm["time"].min()))      # dt = 0 for everybody; module_mixing is not due (box_cases.setup)
    g = s.get_atm()
    for k in ("time", "lon", "lat", "p", "q"):
        assert np.array_equal(g[k], atm[k]), k         # the placed bits are what the kernels see
    return s, ctl, clim, m0, m1, atm


def _oracle(ctl, clim, m0, m1, atm):
    return B.Oracle(ctl, clim, m0, m1, atm)


def _mixparam(o, clim, m0, m1, atm):
    w = RM.Ref(o.ctl, clim, m0, m1).tropo_weight(atm["time"], atm["lat"], atm["p"])
    return w * o.ctl.mixing_trop + (1.0 - w) * o.ctl.mixing_strat


# ---------------------------------------------------------------------------
# module_mixing
# ---------------------------------------------------------------------------

def mixing_ordered(name, nens):
    """deterministic_sums 1, both ordered-sum algorithms, both particle orders: the oracle's bits"""
    for order in ORDERS:
        s, ctl, clim, m0, m1, atm = _simulation(name, nens, order)
        o = _oracle(ctl, clim, m0, m1, atm)
        o.module("mixing", T)
        want = o.state()["q"]
        npl = _inputs(name)[1]
        assert np.count_nonzero(want[BC.QM][:npl] != atm["q"][BC.QM][:npl]) > npl // 4      # placed particles were mixed
        s.set_option("deterministic_sums", 1)
        for path in (1, 2):
            for k in MIXED:
                s.update_quantity(k, atm["q"][k])
            s.set_option("sum_path", path)
            s.module("mixing", T)
            got = s.get_atm()
            differing = int(np.count_nonzero(got["q"] != want))
            report(test="mixing", grid=name, nens=nens, order=order, sum_path=path, differing=differing)
            assert differing == 0 and np.array_equal(got["q"], want)
            for k in ("time", "lon", "lat", "p"):
                assert np.array_equal(got[k], atm[k])
        s.close()


@pytest.mark.parametrize("nens", [0, BC.NMEMBER])
@pytest.mark.parametrize("name", list(BC.GRIDS))
def test_module_mixing_with_ordered_sums(name, nens):
    mixing_ordered(name, nens)


def mixing_atomics(name, nens):
    """deterministic_sums 0: floating-point atomics, order of arrival -- the existing bar 1e-12 per quantity row, after
    the reference has shown that one placed particle in the cell across its face changes a value by more than 1e-6"""
    s, ctl, clim, m0, m1, atm = _simulation(name, nens, "external")
    o = _oracle(ctl, clim, m0, m1, atm)
    npl, tags = _inputs(name)[1:]
    cell = BC.cells(BC.GRIDS[name], atm, T, DT)
    margin, n = BC.flip_effects(BC.GRIDS[name], cell, atm["q"][BC.QM], _mixparam(o, clim, m0, m1, atm), tags, nens,
                                atm["q"][BC.QENS])
    o.module("mixing", T)
    s.set_option("deterministic_sums", 0)
    s.module("mixing", T)
    err, row = cases.q_rows_err(o.ctl, s.get_atm()["q"], o.state()["q"])
    report(test="mixing_atomics", grid=name, nens=nens, err=err, row=row, flip_margin=margin, flips=n)
    assert n > npl // 4 and margin > 1e-6
    assert err <= 1e-12, (row, err)
    s.close()


@pytest.mark.parametrize("nens", [0, BC.NMEMBER])
@pytest.mark.parametrize("name", list(BC.GRIDS))
def test_module_mixing_with_atomic_sums(name, nens):
    mixing_atomics(name, nens)


# ---------------------------------------------------------------------------
# gridded output
# ---------------------------------------------------------------------------

def gridded(name, exact=False):
    """counts, sums and squares of mphip_grid_sums against Oracle.grid_sums: through box_index_kernel (sum_path 1) and
    cell_slot_pairs_kernel (sum_path 2), values from records and from the arrays; then with the vertical weighting
    function, whose weight goes through the device's logarithm in the default build (the bar of
    test_gpu_parity.py::test_gridded_sums_with_a_vertical_weighting_function: counts equal, sums within 1e-12 of the
    largest); `exact`: the reference-rounding build returns the oracle's bits there too."""
    atm, npl, tags = _inputs(name)
    kernel, _ = BC.weighting(name, atm, tags)
    for order in ORDERS:
        s, ctl, clim, m0, m1, atm = _simulation(name, 0, order)
        o = _oracle(ctl, clim, m0, m1, atm)
        plain, weighted = o.grid_sums(T), o.grid_sums(T, kernel=kernel)
        cell = BC.cells(BC.GRIDS[name], atm, T, DT)
        assert np.array_equal(plain[0], np.bincount(cell[cell >= 0], minlength=len(plain[0])))
        assert np.abs(weighted[1] - plain[1]).max() > 0.1 * np.abs(plain[1]).max()
        for path in (1, 2):
            s.set_option("sum_path", path)
            for records in (0, 1):
                s.set_option("grid_records", records)
                s.set_grid_kernel()
                got = s.grid_sums(T)
                same = [bool(np.array_equal(a, b)) for a, b in zip(got, plain)]
                report(test="gridded", grid=name, order=order, sum_path=path, records=records, equal=same)
                assert all(same)
                s.set_grid_kernel(*kernel)
                cnt, mean, sigma = s.grid_sums(T)
                e1 = float(np.abs(mean - weighted[1]).max() / np.abs(weighted[1]).max())
                e2 = float(np.abs(sigma - weighted[2]).max() / np.abs(weighted[2]).max())
                bits = bool(np.array_equal(mean, weighted[1]) and np.array_equal(sigma, weighted[2]))
                report(test="gridded_weighted", grid=name, order=order, sum_path=path, records=records,
                       counts=bool(np.array_equal(cnt, weighted[0])), mean=e1, sigma=e2, equal=bits)
                assert np.array_equal(cnt, weighted[0])
                assert e1 <= 1e-12 and e2 <= 1e-12
                if exact:
                    assert bits
        s.close()


@pytest.mark.parametrize("name", list(BC.GRIDS))
def test_gridded_output(name):
    gridded(name)


# ---------------------------------------------------------------------------
# CSI and profile boxes (box_cell_of_height, kernel_weight_exact)
# ---------------------------------------------------------------------------

def box_sums(name):
    atm, npl, tags = _inputs(name)
    grid = BC.GRIDS[name]
    kernel, placed_nodes = BC.weighting(name, atm, tags)
    zs = np.array([BC.Z(p) for p in atm["p"].tolist()])
    on_node = [int(np.count_nonzero(zs[:npl] == z)) for z in kernel[0][placed_nodes]]
    assert min(on_node) >= 1 and (zs[:npl] < kernel[0][0]).any() and (zs[:npl] > kernel[0][-1]).any(), on_node
    csi = RA.box_sums(atm, grid, T, DT, BC.QM, BC.NMEMBER, BC.QENS, kernel)
    prof = RA.box_sums(atm, grid, T, DT, BC.QAOA)
    assert all((csi[e] > 0).any() for e in range(BC.NMEMBER))
    for order in ORDERS:
        s = _simulation(name, 0, order)[0]
        for path in (0, 1, 2):
            s.set_option("sum_path", path)
            a = s.box_sums(grid, T, BC.QM, BC.NMEMBER, BC.QENS, kernel)
            b = s.box_sums(grid, T, BC.QAOA)
            same = [bool(np.array_equal(a, csi)), bool(np.array_equal(b, prof))]
            report(test="box_sums", grid=name, order=order, sum_path=path, equal=same,
                   differing=[int(np.count_nonzero(a != csi)), int(np.count_nonzero(b != prof))])
            assert all(same)
        s.close()


@pytest.mark.parametrize("name", ["A", "B"])
def test_csi_and_profile_boxes(name):
    box_sums(name)


# ---------------------------------------------------------------------------
# chemistry grid
# ---------------------------------------------------------------------------

def chem_grid(exact=False):
    """module_chem_grid on grid A against tests/refh2o2.py, driven as tests/test_gpu_h2o2_chem.py drives it (its bar:
    1e-12 on Cx; `exact`: the reference in the C library's arithmetic, bit for bit)."""
    import refh2o2
    import test_gpu_h2o2_chem as H
    names = ("m", "vmr", "Cx")
    base, npl, tags = _inputs("A")
    grid = BC.GRIDS["A"]
    ctl, clim, m0, m1, _ = H._case(10, names, grid=BC.grid_keys("chemgrid", grid))
    n = len(base["time"])
    atm = {k: base[k].copy() for k in ("time", "lon", "lat", "p")}
    atm["q"] = np.vstack([base["q"][BC.QM] * 1e7, base["q"][BC.QVMR], 10.0 ** np.random.default_rng(3).uniform(-13, -6, n)])
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.module("chem_grid", T)
    g = s.state()
    s.close()
    probe = H.Probe(ctl, clim, m0, m1, n)
    ref = atm["q"].copy()
    cell, mass = refh2o2.chem_grid(ctl, ref, H._idx(ctl), T, atm["time"], atm["p"], atm["lon"], atm["lat"], probe.temp_at,
                                   "libm" if exact else "numpy")
    assert np.array_equal(cell, BC.cells(grid, atm, T, DT))
    # one placed particle across its face: Cx of the cell it leaves and of the one it enters change by its share of the mass
    stride = (grid[5] * grid[8], grid[8], 1)
    margin = np.inf
    for i, tg in enumerate(tags):
        if tg[0] == "face" and cell[i] >= 0:
            a, here = tg[1], BC.decompose(grid, int(cell[i]))[tg[1]]
            there = here - 1 if here == tg[2] else here + 1
            m = atm["q"][0][i]
            margin = min(margin, m / mass[cell[i]])
            if 0 <= there < grid[3 * a + 2]:
                margin = min(margin, m / (mass[cell[i] + (there - here) * stride[a]] + m))
    k = names.index("Cx")
    err = H.rel(g["q"][k], ref[k])
    differing = int(np.count_nonzero(g["q"].view(np.uint64) != ref.view(np.uint64)))
    report(test="chem_grid", grid="A", err=err, differing=differing, flip_margin=float(margin))
    assert margin > 1e-6
    assert np.array_equal(g["q"][k][cell < 0], atm["q"][k][cell < 0])
    assert err <= 1e-12
    if exact:
        assert differing == 0


def test_chemistry_grid():
    chem_grid()


# ---------------------------------------------------------------------------
# the three producers of module_mixing's cell inside a time step
# ---------------------------------------------------------------------------

PRODUCERS = ((1, 1), (0, 1), (0, 0))      # (emit_keys, ahead_box)


def producers(tol=1e-10):
    """Grid A as the mixing grid of the case `full`, the internal locality order off, module_mixing in every step.  The
    placed particles are released at the time t_k of a step, so in that step they have dt = 0, nothing moves them, and
    module_mixing meets the placed bits while the background moves.

    t_k is the second step and SORT_DT = 2 DT_MOD, not the third with SORT_DT = DT_MOD: module_timesteps stores dt per
    slot before module_sort re-orders the particles, so with a module_sort in step t_k the placed
    particles take over the time steps of other slots and move -- in the reference too.  With a sort due in the step
    after t_k the step t_k still takes the branch that chooses among the three producers, which is read from
    mphip_run_timestep (mphip_api.hip, "the keys of the sort ahead ..."), not measured (there is no getter): sort_next is
    true (a sort at t_k + DT_MOD, the caller's order kept), so with emit_keys 1 and ahead_box 1 the step kernel's
    EmitKeys writes the cell; with emit_keys 0 the EmitKeys stay empty and sort_key_kernel gets the BoxArgs
    (cells_ready); with ahead_box 0 cells_ready is cleared and do_mixing runs box_index_kernel.  The step after t_k,
    with that module_sort, is run and compared too."""
    grid = BC.GRIDS["A"]
    ctl, clim, m0, m1, atm = cases.make_case("full", n=3000, grid=BC.MET_GRID)
    ctl = dict(ctl, sort_dt=2 * DT, mixing_dt=DT, mixing_trop=0.4, mixing_strat=0.1, **BC.grid_keys("mixing", grid))
    assert ctl["dt_mod"] == DT
    T = DT                            # t_k
    names = list(cases.QUANTITIES)
    pl = BC.placed(grid, T, DT, 1, times="late")
    npl = len(pl["tag"])
    for k in ("time", "lon", "lat", "p"):
        atm[k][:npl] = pl[k]
    label = names.index("rhop")      # no module changes it, module_sort carries it along: the placed particle's number
    atm["q"][label][:npl] = 1001.0 + np.arange(npl)
    for k in ("m", "vmr"):
        atm["q"][names.index(k)][:npl] *= BC.HEAVY * (1.0 + np.arange(npl) / npl)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    times = cases.step_times(o.ctl)[:3]
    assert times[1] == T and times[2] == 2 * DT
    for t in times[:2]:
        o.run_timestep(t)
    r = o.state()
    o.run_timestep(times[2])
    r_next = o.state()
    t0, t1 = T - 0.5 * DT, T + 0.5 * DT
    late = sum(1 for tg in pl["tag"] if tg[0] == "time" and tg[2] == 1 and tg[3] == 1)

    def placed_now(state):
        idx = np.nonzero(state["q"][label] > 1000.5)[0]
        num = np.rint(state["q"][label][idx] - 1001.0).astype(int)
        assert np.array_equal(np.sort(num), np.arange(npl))
        for k in ("time", "lon", "lat", "p"):
            assert np.array_equal(state[k][idx], pl[k][num]), k       # still the placed bits
        inside = ~((state["time"][idx] < t0) | (state["time"][idx] > t1))
        assert inside.sum() == npl - late and late >= 1
        return idx, num

    idx, num = placed_now(r)
    im = names.index("m")
    cell = BC.cells(grid, {k: r[k][idx] for k in ("time", "lon", "lat", "p")}, T, DT)
    mixed = int(np.count_nonzero(r["q"][im][idx] != atm["q"][im][num]))
    assert mixed > np.count_nonzero(cell >= 0) * 0.9 and np.array_equal(r["q"][im][idx][cell < 0], atm["q"][im][num][cell < 0])
    runs = []
    for emit, ahead in PRODUCERS:
        s = hip.Simulation(ctl, clim, m0, m1, atm)
        s.set_option("locality_sort_interval", 0)
        s.set_option("emit_keys", emit)
        s.set_option("ahead_box", ahead)
        s.timesteps_init(atm["time"].min(), atm["time"].max())
        for t in times[:2]:
            s.run_timestep(t)
        g = s.state()
        placed_now(g)
        s.run_timestep(times[2])
        runs.append((g, s.state()))
        if len(runs) == 1:
            for step, got, want in (("t_k", g, r), ("next", runs[0][1], r_next)):
                e = {k: cases.rel_err(got[k], want[k]) for k in ("lon", "lat", "p")}
                e["q"] = cases.q_rows_err(o.ctl, got["q"], want["q"])[0]
                e["time"] = bool(np.array_equal(got["time"], want["time"]))
                e["uvwp"] = bool(np.array_equal(got["uvwp"], want["uvwp"]))
                report(test="producers_oracle", grid="A", step=step, emit_keys=emit, ahead_box=ahead, placed_mixed=mixed, **e)
                assert e["time"] and e["uvwp"], e
                for k in ("lon", "lat", "p", "q"):
                    assert e[k] <= tol, (k, e[k])
            assert s.get_cache()["rng_ctr"] == o.cache.rng_ctr
        else:
            same = {k + ("_next" if j else ""): bool(np.array_equal(runs[0][j][k], runs[-1][j][k])) for j in (0, 1)
                    for k in ("time", "lon", "lat", "p", "q", "uvwp")}
            report(test="producers_equal", grid="A", emit_keys=emit, ahead_box=ahead, **same)
            assert all(same.values()), same
        s.close()


def test_three_producers_of_the_mixing_cell_in_a_time_step():
    producers()
