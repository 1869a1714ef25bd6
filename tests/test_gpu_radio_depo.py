"""module_radio_depo on the device (mphip_set_radio_depo) against tests/refradiodepo.py.

The factors of the two deposition modules that the restatement takes as input never come from the device: the oracle's
module_wet_depo / module_dry_depo run alone on a copy of the particles with a mass of one, which leaves aux_w / aux_d in
the mass and shows which particles each module touched (a module that acts with a factor of exactly one is
indistinguishable from one that does not act, in the restatement as on the device: it deposits nothing).

Cases `full` and `wet_henry` of tests/cases.py on the C1 grid, at most 20 000 particles.  `wet_henry` configures no dry
deposition; it runs here with `full`'s deposition velocity on top, so that both cases deposit wet and dry.  A third of
the particles sit in the lowest kilometres (inside the surface layer and below the cloud tops), every ninth particle is
not released yet (dt = 0), and the ground grid leaves a rim of the globe outside.  The cell a particle deposits into is
not downloadable; it is checked through the inventory: the planes' non-zero pattern against the restatement's cells, and
test 2's array_equal of every plane against the serial sum over the restatement's cells."""
import functools
import threading

import numpy as np
import pytest

import cases
import refradio
import refradiodepo as RD
from mptrac_amd import hip
from oracle import binding as B
from test_gpu_full_size import _ThreadAllreduce

pytestmark = pytest.mark.gpu

ACT = refradio.NAMES
NAMES = ("m", "vmr", "loss_rate") + ACT
ROW = {n: k for k, n in enumerate(NAMES)}
IDX = [ROW[a] for a in ACT]
DEP = [ROW[a] for a in RD.DEPOSITING]
GRID = (-170.0, 175.0, 69, -80.0, 85.0, 33)
NCELL = GRID[2] * GRID[5]
N = 20000
CASES = ("full", "wet_henry")


def rel_rows(a, b):
    """largest error on the row's scale"""
    top = float(np.max(np.abs(b)))
    return float(np.max(np.abs(a - b))) / top if top > 0 else (0.0 if np.array_equal(a, b) else float("inf"))


@functools.lru_cache(maxsize=None)
def inputs(case, n=N):
    ctl, clim, m0, m1, atm = cases.make_case(case, n=n, quantities=NAMES)
    if case == "wet_henry":
        ctl["dry_depo_vdep"] = cases.CASES["full"]["dry_depo_vdep"]
    rng = np.random.default_rng(20261017)
    low = np.arange(n) % 3 == 0                    # the lowest kilometres: surface layer, below the cloud tops
    atm["p"][low] = 1013.25 * np.exp(-rng.uniform(0.0, 3.0, low.sum()) / 7.0)
    atm["time"][::9] = 900.0                       # released later: dt = 0 in the first steps
    for a in ACT:
        atm["q"][ROW[a]] = 10.0 ** rng.uniform(1.0, 5.0, n)
    atm["q"][ROW["m"]] *= 1e6
    for k in atm:
        atm[k].setflags(write=False)
    return ctl, clim, m0, m1, atm


def copy_atm(atm):
    return {k: np.array(v) for k, v in atm.items()}


def depo_on(ctl):
    """(wet, dry): the deposition modules the control parameters configure (mptrac.c:7983-7993)"""
    g = lambda k, d=0.0: ctl.get(k, d)      # noqa: E731
    h = lambda k: (ctl.get(k) or (0.0, 0.0))[0]      # noqa: E731
    wet = (g("wet_depo_ic_a") > 0 or h("wet_depo_ic_h") > 0) and (g("wet_depo_bc_a") > 0 or h("wet_depo_bc_h") > 0)
    return bool(wet), g("dry_depo_vdep") > 0


def oracle_factors(ctl, clim, m0, m1, pos, dt):
    """(aux_w, acts_w, aux_d, acts_d) of the oracle's modules at the positions `pos` with the time steps dt"""
    n = len(dt)
    atm = {k: np.array(pos[k]) for k in ("time", "p", "lon", "lat")}
    atm["q"] = np.array(pos["q"])
    wet, dry = depo_on(ctl)
    out = []
    for name, on in (("wet_depo", wet), ("dry_depo", dry)):
        if not on:
            out += [np.ones(n), np.zeros(n, dtype=bool)]
            continue
        atm["q"][ROW["m"]] = 1.0
        o = B.Oracle(ctl, clim, m0, m1, atm)
        o.dt[:] = dt
        o.module(name)
        aux = o.q[ROW["m"]].copy()
        out += [aux, aux != 1.0]
    return tuple(out)


def assert_coverage(acts_w, acts_d, cells, need_wet=True, need_dry=True):
    """the oracle's result deposits enough to check anything"""
    if need_wet:
        assert acts_w.sum() >= 200, acts_w.sum()
    if need_dry:
        assert acts_d.sum() >= 200, acts_d.sum()
    used = cells[cells >= 0]
    count = np.bincount(used, minlength=NCELL + 1)
    assert (count[:NCELL] > 0).sum() >= 50 and count[:NCELL].max() >= 3, ((count > 0).sum(), count[:NCELL].max())


@functools.lru_cache(maxsize=None)
def module_alone_reference(case, only=None):
    """The restatement of one call of the module at t = 360 s after module_timesteps: (q, inventory, dt, factors).
    only = "wet" / "dry": that deposition module alone is configured."""
    ctl, clim, m0, m1, atm = inputs(case)
    ctl = configured(ctl, only)
    o = B.Oracle(ctl, clim, m0, m1, copy_atm(atm))
    o.timesteps_init()
    o.module("timesteps", T_ALONE)
    dt = o.dt.copy()
    fac = oracle_factors(ctl, clim, m0, m1, atm, dt)
    q = np.array(atm["q"])
    inv = RD.Inventory(GRID).step(T_ALONE, q, IDX, atm["lon"], atm["lat"], dt, *fac)
    assert_coverage(fac[1] & (dt != 0), fac[3] & (dt != 0), inv.cells, only != "dry", only != "wet")
    return q, inv, dt, fac


T_ALONE = 360.0


def configured(ctl, only):
    ctl = dict(ctl)
    if only == "wet":
        ctl["dry_depo_vdep"] = 0.0
    elif only == "dry":
        for k in ("wet_depo_ic_a", "wet_depo_bc_a"):
            ctl[k] = 0.0
        for k in ("wet_depo_ic_h", "wet_depo_bc_h"):
            ctl[k] = (0.0, 0.0)
    return ctl


def device_module_alone(case, only=None, atm=None, sort_dt=None, calls=1):
    ctl, clim, m0, m1, atm0 = inputs(case)
    ctl = configured(ctl, only)
    if sort_dt is not None:
        ctl["sort_dt"] = sort_dt
    atm = copy_atm(atm0) if atm is None else atm
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.set_radio_decay(NAMES, on=False)
    s.set_radio_depo(GRID)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    s.module("timesteps", T_ALONE)
    for _ in range(calls):
        s.module("radio_depo", T_ALONE)
    g, dt, inv = s.state(), s.get_cache()["dt"], s.radio_depo()
    s.close()
    return g, dt, inv


def check_against(g, inv, q, ref, atm, dt, tol):
    """rows and planes against the restatement: tol = 1e-10 on the row's / plane's scale, or 0 = bit for bit"""
    t_inv, wet, dry = inv
    assert t_inv == ref.t_inv
    occupied = np.bincount(ref.cells[ref.cells >= 0], minlength=NCELL + 1)
    for k in ("time", "p", "lon", "lat"):
        assert np.array_equal(g[k], atm[k]), k
    for name in ("m", "vmr", "loss_rate", "Arn222", "Axe133"):
        assert np.array_equal(g["q"][ROW[name]], atm["q"][ROW[name]]), name
    assert np.array_equal(g["q"][:, dt == 0], atm["q"][:, dt == 0])
    for k, name in enumerate(ACT):
        r = ROW[name]
        if name in RD.DEPOSITING:
            # the same particles changed (a deposit below 1e-9 of the activity may round away on either side) ...
            changed, acted = g["q"][r] != atm["q"][r], ref.cells >= 0
            assert not changed[~acted].any() and changed[(atm["q"][r] - q[r]) > 1e-9 * atm["q"][r]].all(), name
            for got, want, kind in ((wet[k], ref.wet[k], "wet"), (dry[k], ref.dry[k], "dry")):
                # ... into the same cells
                assert not got[occupied == 0].any() and (got != 0)[want > 1e-9 * want.max()].all(), (name, kind)
                if tol:
                    assert rel_rows(got, want) <= tol, (name, kind)
                else:
                    assert np.array_equal(got, want), (name, kind)
            if tol:
                assert rel_rows(g["q"][r], q[r]) <= tol, name
            else:
                assert np.array_equal(g["q"][r], q[r]), name
        else:
            assert not wet[k].any() and not dry[k].any(), name


@pytest.mark.parametrize("case", CASES)
def test_module_alone_against_the_restatement(case):
    q, ref, dt_ref, fac = module_alone_reference(case)
    atm = inputs(case)[4]
    g, dt, inv = device_module_alone(case)
    assert np.array_equal(dt, dt_ref) and (dt == 0).sum() >= N // 10
    check_against(g, inv, q, ref, atm, dt, 1e-10)
    assert ref.wet[:, NCELL].sum() > 0 and ref.dry[:, NCELL].sum() > 0      # the bin outside the grid is in use


def test_an_absent_activity_keeps_its_plane_at_zero():
    case = "full"
    ctl, clim, m0, m1, atm = inputs(case)
    q, ref, dt_ref, fac = module_alone_reference(case)
    s = hip.Simulation(ctl, clim, m0, m1, copy_atm(atm))
    s.set_radio_decay({a: ROW[a] for a in ACT if a != "Acs137"}, on=False)
    s.set_radio_depo(GRID)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    s.module("timesteps", T_ALONE)
    s.module("radio_depo", T_ALONE)
    g, (t_inv, wet, dry) = s.state(), s.radio_depo()
    s.close()
    k = ACT.index("Acs137")
    assert not wet[k].any() and not dry[k].any()
    assert np.array_equal(g["q"][ROW["Acs137"]], atm["q"][ROW["Acs137"]])
    k = ACT.index("Ai131")
    assert rel_rows(wet[k], ref.wet[k]) <= 1e-10 and rel_rows(dry[k], ref.dry[k]) <= 1e-10


@pytest.mark.parametrize("only", ["wet", "dry"])
@pytest.mark.parametrize("case", CASES)
def test_inventory_is_the_serial_sum_of_what_left_the_air(case, only):
    """independent of any libm bit: (uploaded - downloaded activity) summed per cell in ascending index"""
    q, ref, dt_ref, fac = module_alone_reference(case, only)
    atm = inputs(case)[4]
    g, dt, (t_inv, wet, dry) = device_module_alone(case, only)
    planes, other = (wet, dry) if only == "wet" else (dry, wet)
    assert not other.any()
    for name in RD.DEPOSITING:
        gone = atm["q"][ROW[name]] - g["q"][ROW[name]]
        assert np.array_equal(planes[ACT.index(name)], RD.serial_cell_sums(gone, ref.cells, NCELL)), name
        assert (gone[ref.cells >= 0] > 0).sum() >= 200 and not gone[ref.cells < 0].any()


def _serial_inventory(before, after, name):
    """serial ascending-index sum of what left the air, in the order of `before` / `after` (one deposition module)"""
    gone = before["q"][ROW[name]] - after["q"][ROW[name]]
    cell = np.where(gone != 0, RD.ground_cell(GRID, after["lon"], after["lat"]), -1)
    return RD.serial_cell_sums(gone, cell, NCELL), cell


@pytest.mark.parametrize("case", CASES)
def test_inventory_follows_the_external_order_not_the_stored_one(case):
    """The sums add in ascending EXTERNAL index, so the bits belong to the caller's order and to nothing else.
    (1) The same particles uploaded in a shuffled order: the particle rows mapped back are identical; the inventory is
    the serial sum in THAT order bit for bit, identical to the unshuffled one in every cell with at most two deposits
    (a + b = b + a) and within (deposits per cell) * 2^-52 of it elsewhere -- sums of three or more positive terms in
    another order are another rounding, in the restatement as on the device.  (2) module_sort makes its order the
    external one: again the serial sum in that order.  (3) The locality re-sort changes the stored order only: a run
    with a re-sort before every step and one without give identical bits."""
    atm = inputs(case)[4]
    q, ref, dt_ref, fac = module_alone_reference(case, "wet")           # (coverage of the wet part)
    g0, dt0, inv0 = device_module_alone(case, "wet")
    perm = np.random.default_rng(5).permutation(N)
    shuffled = {k: np.array(atm[k][..., perm]) for k in atm}
    g1, dt1, inv1 = device_module_alone(case, "wet", atm=shuffled)
    assert np.array_equal(g1["q"], g0["q"][:, perm]) and np.array_equal(dt1, dt0[perm])
    count = np.bincount(ref.cells[ref.cells >= 0], minlength=NCELL + 1)
    assert (count >= 3).sum() >= 1
    for name in RD.DEPOSITING:
        k = ACT.index(name)
        want, _ = _serial_inventory(shuffled, g1, name)
        assert np.array_equal(inv1[1][k], want), name
        assert np.array_equal(inv1[1][k][count <= 2], inv0[1][k][count <= 2]), name
        worst = np.max(np.abs(inv1[1][k] - inv0[1][k]) / np.maximum(inv0[1][k], 1e-300))
        print(f"{case} {name}: shuffled external order against the original one, largest relative difference {worst:.3e}")
        assert worst <= count.max() * 2.0 ** -52, name
    # (2) module_sort, then the module
    ctl, clim, m0, m1, _ = inputs(case)
    s = hip.Simulation(configured(ctl, "wet"), clim, m0, m1, copy_atm(atm))
    s.set_radio_decay(NAMES, on=False)
    s.set_radio_depo(GRID)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    s.module("timesteps", T_ALONE)
    keys, order = s.sort()
    assert not np.array_equal(order, np.arange(N))
    before = s.state()
    s.module("radio_depo", T_ALONE)
    after, inv = s.state(), s.radio_depo()
    s.close()
    for name in RD.DEPOSITING:
        want, cell = _serial_inventory(before, after, name)
        assert (cell >= 0).sum() >= 200
        assert np.array_equal(inv[1][ACT.index(name)], want), name
    # (3) the locality re-sort
    for interval in (0, 1):
        s = hip.Simulation(ctl, clim, m0, m1, copy_atm(atm))
        s.set_option("locality_sort_interval", interval)
        s.set_radio_decay(NAMES, on=False)
        s.set_radio_depo(GRID)
        s.timesteps_init(atm["time"].min(), atm["time"].max())
        times = cases.step_times(s.ctl)[:4]
        for t in times:
            s.run_timestep(t)
        inv = s.radio_depo()
        s.close()
        if interval == 0:
            base = inv
        else:
            assert inv[0] == base[0] == times[-1]
            assert np.array_equal(inv[1], base[1]) and np.array_equal(inv[2], base[2])
            assert base[1].any() and base[2].any()


def _oracle_run(ctl, clim, m0, m1, atm, times, radio_decay=True, mode="numpy"):
    """the oracle moves and mixes the particles (the activities ride in its five trace-gas slots and the age-of-air
    slot, as tests/test_gpu_radio_decay.py has it); restatements of module_radio_decay and module_radio_depo behind the
    mixing, the second with the factors of a twin of mass one at the same positions.  Also returns what module_mixing
    added to the sum of each activity row over the run; the inventory comes back with `deposits`, the total of every
    step's wet and dry sums per nuclide, [(t, wet[6], dry[6]), ...]: what an inventory that only added would hold."""
    octl = dict(ctl, qnt_tracer=tuple(IDX[:5]), qnt_aoa=IDX[5])
    o = B.Oracle(octl, clim, m0, m1, copy_atm(atm))
    o.timesteps_init()
    c = o.ctl
    inv = RD.Inventory(GRID)
    history, mixed, inv.deposits = [], np.zeros(len(ACT)), []
    for t in times:
        o.module("timesteps", t)
        if c.sort_dt > 0 and np.fmod(t, c.sort_dt) == 0:
            o.sort()
        for m in ("position", "advect", "diff_turb", "diff_meso", "convection", "position"):
            o.module(m)
        if c.mixing_trop >= 0 and c.mixing_strat >= 0 and np.fmod(t, c.mixing_dt) == 0:
            unmixed = np.array([np.sum(o.q[r]) for r in IDX])
            o.module("mixing", t)
            mixed += np.array([np.sum(o.q[r]) for r in IDX]) - unmixed
        if radio_decay:
            refradio.apply(o.q, IDX, o.dt, mode)
        fac = oracle_factors(ctl, clim, m0, m1, o.state(), o.dt)
        inv.step(t, o.q, IDX, o.lon, o.lat, o.dt, *fac)
        history.append((fac[1] & (o.dt != 0), fac[3] & (o.dt != 0), inv.cells.copy()))
        inv.deposits.append((t, inv.step_wet.sum(axis=1), inv.step_dry.sum(axis=1)))
    return o, inv, history, mixed


@functools.lru_cache(maxsize=None)
def twenty_steps_reference(case, radio_decay=True, mode="numpy"):
    """(ctl, times, oracle, inventory, history, mixed)"""
    ctl, clim, m0, m1, atm = inputs(case, n=TWENTY_N)
    ctl = dict(ctl, **cases.CASES["full"]) if case == "wet_henry" else ctl
    o = B.Oracle(ctl, clim, m0, m1, copy_atm(atm))
    o.timesteps_init()
    times = cases.step_times(o.ctl)[:20]
    return (ctl, times) + _oracle_run(ctl, clim, m0, m1, atm, times, radio_decay, mode)


TWENTY_N = 12000


def device_twenty_steps(ctl, clim, m0, m1, atm, times, radio_decay=True):
    s = hip.Simulation(ctl, clim, m0, m1, copy_atm(atm))
    s.set_radio_decay(NAMES, on=radio_decay)
    s.set_radio_depo(GRID)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    s.run_timestep(times[0])
    s.run_timesteps(times[1], len(times) - 1)
    g, inv = s.state(), s.radio_depo()
    s.close()
    return g, inv


def check_twenty_steps(g, inv, o, ref, tol):
    r = o.state()
    assert np.array_equal(g["time"], r["time"])
    for k in ("lon", "lat", "p"):
        assert cases.rel_err(g[k], r[k]) <= 1e-10, k
    t_inv, wet, dry = inv
    assert t_inv == ref.t_inv
    for k, name in enumerate(ACT):
        if tol:
            assert rel_rows(g["q"][ROW[name]], r["q"][ROW[name]]) <= tol, name
        else:
            assert np.array_equal(g["q"][ROW[name]], r["q"][ROW[name]]), name
        for got, want, kind in ((wet[k], ref.wet[k], "wet"), (dry[k], ref.dry[k], "dry")):
            if name not in RD.DEPOSITING:
                assert not got.any(), (name, kind)
            elif tol:
                assert rel_rows(got, want) <= tol, (name, kind)
            else:
                assert np.array_equal(got, want), (name, kind)


def test_twenty_steps_with_everything_on_against_the_oracle():
    """`full`: module_sort, module_mixing, decay, both deposition modules, module_radio_decay"""
    clim, m0, m1, atm = inputs("full", n=TWENTY_N)[1:]
    ctl, times, o, ref, history, _ = twenty_steps_reference("full")
    assert len(times) == 20
    for acts_w, acts_d, cells in history[-3:]:
        assert_coverage(acts_w, acts_d, cells)
    g, inv = device_twenty_steps(ctl, clim, m0, m1, atm, times)
    check_twenty_steps(g, inv, o, ref, 1e-10)
    # The ground decay over the run is visible for I-131, by itself: against the deposits of the same run (airborne decay
    # included) merely added up, the device's planes hold less, and by what exp(-lambda (t_end - t)) takes from every
    # step's deposit -- no more than 1 - exp(-lambda (t_end - t_first)), and a fair part of it, as the deposits spread
    # over the run.  (3.4e-3 of the inventory at most; the second bar, 1e-4 of that, is where a mistaken factor shows.)
    k = ACT.index("Ai131")
    lam, t_end = refradio.LAMBDA[k], times[-1]
    whole = 1.0 - np.exp(-lam * (t_end - times[0]))
    for kind, plane in ((1, inv[1][k]), (2, inv[2][k])):
        added = sum(d[kind][k] for d in ref.deposits)
        aged = sum(d[kind][k] * np.exp(-lam * (t_end - d[0])) for d in ref.deposits)
        lost = 1.0 - plane.sum() / added
        print(f"Ai131 kind {kind}: only added {added:.9e}, on the ground {plane.sum():.9e}, lost {lost:.4e} "
              f"(expected {1.0 - aged / added:.4e}, at most {whole:.4e})")
        assert 0.2 * whole < lost < whole
        assert abs(lost - (1.0 - aged / added)) <= 1e-4 * whole


def device_budget(ctl, clim, m0, m1, atm, times):
    """Twenty steps, one run_timesteps call each, with the inventory read behind every step: the state, the inventory
    and what the ground decay took from each nuclide's planes (sum of inv - inv * f over the steps, f as in step 1 of
    the semantics)."""
    s = hip.Simulation(ctl, clim, m0, m1, copy_atm(atm))
    s.set_radio_decay(NAMES, on=False)
    s.set_radio_depo(GRID)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    decayed, inv = np.zeros(len(ACT)), None
    for t in times:
        if inv is not None:
            for k in range(len(ACT)):
                f = np.exp(-refradio.LAMBDA[k] * (t - inv[0]))
                decayed[k] += sum(np.sum(plane[k] - plane[k] * f) for plane in inv[1:])
        s.run_timesteps(t, 1)
        inv = s.radio_depo()
        assert inv[0] == t
    g = s.state()
    s.close()
    return g, inv, decayed


@pytest.mark.parametrize("one_mixing_fraction", [True, False])
def test_conservation_over_twenty_steps_without_radio_decay(one_mixing_fraction):
    """Airborne activity + inventory + what the ground decay took = the activity at the start, to 1e-10, for every
    depositing nuclide, with module_radio_decay off and everything else of `full` on.

    Two things besides the deposition change these sums, and both are booked.  The ground decays whether or not
    module_radio_decay runs (step 1 of the semantics: 1e-6 of the Cs-137 inventory in this hour), so the
    inventory is read behind every step and the loss of each interval added up.  And module_mixing does not keep a
    row's sum where MIXING_TROP != MIXING_STRAT: every particle moves towards its cell's mean by a fraction of its own
    (mptrac.c:5249-5347), and `full` (1e-3 / 1e-6) gains 3.5e-5 of the Cs-137 in twenty steps this way, in the oracle
    as on the device, with or without this module.  So the budget is closed (True) with MIXING_STRAT = MIXING_TROP,
    where the mixing keeps the sums to rounding and no figure of the oracle enters, and (False) with `full` as it
    stands and the sums the oracle's mixing added.  (The positions and the deposition factors do not depend on the
    mixing fractions, so the oracle's run of `full` shows the coverage of both.)"""
    clim, m0, m1, atm = inputs("full", n=TWENTY_N)[1:]
    ctl, times, o, ref, history, mixed = twenty_steps_reference("full", radio_decay=False)
    assert_coverage(*history[-1])
    if one_mixing_fraction:
        ctl = dict(ctl, mixing_strat=ctl["mixing_trop"])
    g, (t_inv, wet, dry), decayed = device_budget(ctl, clim, m0, m1, atm, times)
    for name in RD.DEPOSITING:
        k = ACT.index(name)
        before = np.sum(atm["q"][ROW[name]])
        assert abs(mixed[k]) > 1e-7 * before, (name, mixed[k])
        gain = 0.0 if one_mixing_fraction else mixed[k]
        after = np.sum(g["q"][ROW[name]]) + wet[k].sum() + dry[k].sum() + decayed[k]
        print(f"{name}: start {before:.9e}, ground {wet[k].sum() + dry[k].sum():.6e}, ground decay {decayed[k]:.3e}, "
              f"mixing {gain:.3e}, budget off by {abs(after - before - gain) / before:.2e}")
        assert abs(after - before - gain) <= 1e-10 * before, name
        assert wet[k].sum() + dry[k].sum() > 1e-4 * before, name
    if not one_mixing_fraction:
        # one run_timesteps call per step = one call for all of them (such steps share no launch)
        h, inv = device_twenty_steps(ctl, clim, m0, m1, atm, times, radio_decay=False)
        assert np.array_equal(h["q"], g["q"]) and np.array_equal(inv[1], wet) and np.array_equal(inv[2], dry)


def test_module_off_or_never_set_changes_nothing():
    ctl, clim, m0, m1, atm = inputs("full", n=TWENTY_N)
    out = []
    for touch in (False, True):
        s = hip.Simulation(ctl, clim, m0, m1, copy_atm(atm))
        s.set_radio_decay(NAMES)
        if touch:
            s.set_radio_depo(GRID, on=False)
        s.timesteps_init(atm["time"].min(), atm["time"].max())
        times = cases.step_times(s.ctl)[:20]
        s.run_timestep(times[0])
        s.run_timesteps(times[1], len(times) - 1)
        out.append((s.state(), s.get_cache()))
        if touch:
            t_inv, wet, dry = s.radio_depo()
            assert np.isnan(t_inv) and not wet.any() and not dry.any()
        s.close()
    (g, cg), (h, ch) = out
    for k in ("time", "p", "lon", "lat", "q", "uvwp"):
        assert np.array_equal(g[k], h[k]), k
    assert np.array_equal(cg["dt"], ch["dt"]) and np.array_equal(cg["uvwp"], ch["uvwp"]) and cg["rng_ctr"] == ch["rng_ctr"]
    assert not np.array_equal(g["q"][ROW["Acs137"]], atm["q"][ROW["Acs137"]])      # (mixing and decay did act)


def test_module_on_leaves_every_other_row_alone():
    """m, vmr, loss_rate, positions, cache and counters of a 20-step run with the module on = with it off"""
    ctl, clim, m0, m1, atm = inputs("full", n=TWENTY_N)
    out = []
    for on in (False, True):
        s = hip.Simulation(ctl, clim, m0, m1, copy_atm(atm))
        s.set_radio_decay(NAMES)
        s.set_radio_depo(GRID, on=on)
        s.timesteps_init(atm["time"].min(), atm["time"].max())
        times = cases.step_times(s.ctl)[:20]
        s.run_timestep(times[0])
        s.run_timesteps(times[1], len(times) - 1)
        out.append((s.state(), s.get_cache()))
        s.close()
    (g, cg), (h, ch) = out
    for k in ("time", "p", "lon", "lat", "uvwp"):
        assert np.array_equal(g[k], h[k]), k
    for name in ("m", "vmr", "loss_rate"):
        assert np.array_equal(g["q"][ROW[name]], h["q"][ROW[name]]), name
    assert np.array_equal(cg["dt"], ch["dt"]) and cg["rng_ctr"] == ch["rng_ctr"]
    assert np.all(h["q"][ROW["Acs137"]] <= g["q"][ROW["Acs137"]] * (1 + 1e-12))


def test_two_shards_give_the_single_context():
    world, n = 2, N
    ctl, clim, m0, m1, atm = inputs("full")
    ctl = dict(ctl, sort_dt=-999.0)

    def run(shard=None, hook=None):
        s = hip.Simulation(ctl, clim, m0, m1, copy_atm(atm), shard=shard)
        s.set_radio_decay(NAMES)
        s.set_radio_depo(GRID)
        if hook:
            s.set_allreduce(hook)
        s.timesteps_init(0.0, 0.0)
        times = cases.step_times(s.ctl)[:6]
        for t in times:
            s.run_timestep(t)
        inv = s.radio_depo()
        s.close()
        return inv
    ref = run()
    ar = _ThreadAllreduce(world)
    out, errors = [None] * world, []

    def rank_main(rank):
        try:
            out[rank] = run(hip.shard_range(n, rank, world), ar.hook(rank))
        except BaseException as exc:      # noqa: BLE001
            errors.append((rank, repr(exc)))
            ar.barrier.abort()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for rank in range(world):
        assert out[rank][0] == ref[0]
        for k, name in enumerate(ACT):
            for a, b in ((out[rank][1][k], ref[1][k]), (out[rank][2][k], ref[2][k])):
                if name in RD.DEPOSITING:
                    assert b.any() and rel_rows(a, b) <= 1e-13, name
                else:
                    assert not a.any()


def test_refusals():
    ctl, clim, m0, m1, atm = inputs("full", n=200)
    s = hip.Simulation(ctl, clim, m0, m1, copy_atm(atm))

    def refused(msg, *a, **kw):
        with pytest.raises(hip.MphipError, match=msg):
            s.set_radio_depo(*a, **kw)
    with pytest.raises(hip.MphipError, match="mphip_set_radio_depo has not been called"):
        s.radio_depo()
    refused("no depositing activity", GRID)
    s.set_radio_decay({"Arn222": ROW["Arn222"], "Axe133": ROW["Axe133"]})
    refused("no depositing activity", GRID)                          # (the noble gases do not count)
    s.set_radio_decay(NAMES)
    refused("nz = 1", GRID + (0.0, 10.0, 2))
    refused("empty or inverted", (-170.0, 175.0, 0, -80.0, 85.0, 33))
    refused("empty or inverted", (175.0, -170.0, 69, -80.0, 85.0, 33))
    refused("empty or inverted", (-170.0, 175.0, 69, 85.0, 85.0, 33))
    refused("32-bit cell indices", (-170.0, 175.0, 50000, -80.0, 85.0, 50000))
    refused("null ground grid", None)
    s.ctl.direction = -1
    s.update_ctl()
    refused("DIRECTION must be 1", GRID)
    s.ctl.direction = 1
    s.ctl.met_coord_type = 1
    s.update_ctl()
    refused("MET_COORD_TYPE must be 0", GRID)
    s.ctl.met_coord_type = 0
    s.update_ctl()
    s.set_radio_depo(GRID, on=False)                                  # off: a grid alone is fine ...
    s.ctl.direction = -1
    s.update_ctl()                                                    # ... and so is any control setting
    s.ctl.direction = 1
    s.update_ctl()
    s.set_radio_depo(GRID)
    # while it is on, later calls cannot create these conditions
    s.ctl.direction = -1
    with pytest.raises(hip.MphipError, match="DIRECTION must be 1"):
        s.update_ctl()
    s.ctl.direction = 1
    s.ctl.met_coord_type = 1
    with pytest.raises(hip.MphipError, match="MET_COORD_TYPE must be 0"):
        s.update_ctl()
    s.ctl.met_coord_type = 0
    s.update_ctl()
    with pytest.raises(hip.MphipError, match="no depositing activity"):
        s.set_radio_decay({"Arn222": ROW["Arn222"]})
    with pytest.raises(hip.MphipError, match="must be called on their own"):
        s._chk(s.L.mphip_module(s.h, hip.MOD["radio_depo"] | hip.MOD["wet_depo"], 0.0))
    s.set_radio_depo(None, on=False)
    s.set_radio_decay({"Arn222": ROW["Arn222"]})                      # off again: allowed
    s.close()


def test_same_grid_keeps_the_inventory_a_new_one_starts_over():
    ctl, clim, m0, m1, atm = inputs("full", n=TWENTY_N)
    s = hip.Simulation(ctl, clim, m0, m1, copy_atm(atm))
    s.set_radio_decay(NAMES, on=False)
    s.set_radio_depo(GRID)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    s.module("timesteps", T_ALONE)
    s.module("radio_depo", T_ALONE)
    t0, wet0, dry0 = s.radio_depo()
    assert t0 == T_ALONE and wet0.any() and dry0.any()
    s.set_radio_depo(GRID, on=False)
    s.set_radio_depo(GRID, on=True)
    t1, wet1, dry1 = s.radio_depo()
    assert t1 == t0 and np.array_equal(wet1, wet0) and np.array_equal(dry1, dry0)
    s.set_radio_depo((-180.0, 180.0, 36, -90.0, 90.0, 18))
    t2, wet2, dry2 = s.radio_depo()
    assert np.isnan(t2) and wet2.shape == (6, 36 * 18 + 1) and not wet2.any() and not dry2.any()
    s.close()


def test_both_algorithms_of_the_ordered_sums_give_the_serial_sum():
    """option sum_path: the groups of cells per wave and the chain per (cell, value) -- what a crowded ground grid takes by
    itself (here: 12 x 6 cells under 20 000 particles) -- add the same summands in the same order"""
    case, coarse = "full", (-180.0, 180.0, 12, -90.0, 90.0, 6)
    ctl, clim, m0, m1, atm = inputs(case)
    module_alone_reference(case, "wet")                               # (coverage)
    got = {}
    for grid in (GRID, coarse):
        for path in (0, 1, 2):
            s = hip.Simulation(configured(ctl, "wet"), clim, m0, m1, copy_atm(atm))
            s.set_option("sum_path", path)
            s.set_radio_decay(NAMES, on=False)
            s.set_radio_depo(grid)
            s.timesteps_init(atm["time"].min(), atm["time"].max())
            s.module("timesteps", T_ALONE)
            s.module("radio_depo", T_ALONE)
            got[grid, path] = (s.state(), s.radio_depo())
            s.close()
    for grid in (GRID, coarse):
        ncell = grid[2] * grid[5]
        g, (t_inv, wet, dry) = got[grid, 0]
        for name in RD.DEPOSITING:
            gone = atm["q"][ROW[name]] - g["q"][ROW[name]]
            cell = np.where(gone != 0, RD.ground_cell(grid, atm["lon"], atm["lat"]), -1)
            assert np.array_equal(wet[ACT.index(name)], RD.serial_cell_sums(gone, cell, ncell)), (grid, name)
        for path in (1, 2):
            assert np.array_equal(got[grid, path][1][1], wet) and np.array_equal(got[grid, path][1][2], dry), (grid, path)
            assert np.array_equal(got[grid, path][0]["q"], g["q"]), (grid, path)


def test_busy_list_of_the_launch_that_moved_the_particles():
    """the headline module set (with sedimentation) writes EmitKeys::depo_busy for the deposition launch; the module
    reads the same list -- or decides from p, time and dt itself (emit_keys 0): identical bits.  (Which of the two a
    run took cannot be read from outside; module_radio_decay is off here, as the list only exists where the step's tail
    is the deposition launch alone.)"""
    names = ("m", "rp", "rhop") + ACT
    ctl, clim, m0, m1, atm = cases.make_case("full", n=N, quantities=names)
    rng = np.random.default_rng(3)
    atm["p"][::3] = 1013.25 * np.exp(-rng.uniform(0.0, 3.0, atm["p"][::3].size) / 7.0)
    for a in ACT:
        atm["q"][names.index(a)] = 10.0 ** rng.uniform(1.0, 5.0, N)
    out = []
    for emit in (1, 0):
        s = hip.Simulation(ctl, clim, m0, m1, copy_atm(atm))
        s.set_option("emit_keys", emit)
        s.set_radio_decay(names, on=False)
        s.set_radio_depo(GRID)
        s.timesteps_init(0.0, 0.0)
        for t in cases.step_times(s.ctl)[:6]:
            s.run_timestep(t)
        out.append((s.state(), s.radio_depo()))
        s.close()
    (g, a), (h, b) = out
    assert np.array_equal(g["q"], h["q"])
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[1][ACT.index("Acs137")].any() and a[2][ACT.index("Acs137")].any()
