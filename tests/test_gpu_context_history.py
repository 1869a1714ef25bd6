"""What a context computes does not depend on what the context has served before.

Every device buffer of a context grows when a call needs more than it holds and is kept otherwise (the host
layer: one owning buffer type, the capacity travels with the pointer).  One long-lived context goes through a history of
particle counts, quantity counts, output grids and option values that makes its buffers grow, stay and trade places;
after each phase it holds the bits of a fresh context that was given the same inputs and the same random-number counter
(np.array_equal on time, lon, lat, p, q, uvwp and on every returned sum: the code and the inputs are the same).  That
the values are the right ones is what tests/test_gpu_parity.py, test_gpu_analysis_outputs.py and test_gpu_full_size.py
assert."""
import numpy as np
import pytest

import box_cases
import cases
from mptrac_amd import hip

pytestmark = pytest.mark.gpu

KEYS = ("time", "lon", "lat", "p", "q", "uvwp")


def _same_state(a, b, what):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (what, key)
    assert len(np.unique(a["lon"])) >= 2, what          # (equal bits are not those of an empty result)


def _requantify(s, ctl_kw):
    """other control parameters (another quantity list) for a context that lives on"""
    s.ctl = hip.fill_ctl(hip.MphipCtl(), **ctl_kw)
    s.nq = s.ctl.nq
    s.timesteps_init(0.0, 0.0)


def _set_grid(s, nx, ny, nz):
    s.ctl.grid_nx, s.ctl.grid_ny, s.ctl.grid_nz = nx, ny, nz
    s.ctl.grid_z0, s.ctl.grid_z1 = 0.0, 30.0
    s.update_ctl()


# ---------------------------------------------------------------------------
# a. particle counts, quantity counts, output grids, analysis outputs
# ---------------------------------------------------------------------------

Q3, Q1, Q5 = ("m", "rp", "rhop"), ("m",), ("m", "rp", "rhop", "vmr", "loss_rate")
KERNEL = (np.array([0.0, 5.0, 12.0, 30.0]), np.array([0.2, 1.0, 0.6, 0.1]))
CSI = (-90.0, 120.0, 21, -40.0, 60.0, 10, 2.0, 25.0, 1)


def _grid(nx, ny, nz):
    def call(s, t, dt):
        _set_grid(s, nx, ny, nz)
        return s.grid_sums(t)
    return call


def _box(s, t, dt):
    return (s.box_sums(CSI, t, 0, kernel=KERNEL),)


def _sample(s, t, dt):
    g = s.get_atm()
    lon, lat = g["lon"][:8].copy(), g["lat"][:8].copy()
    z = np.array([box_cases.Z(float(p)) for p in g["p"][:8]])
    return s.sample_obs(t - 0.5 * dt, t + 0.5 * dt, lon, lat, z, 800.0, 6.0, KERNEL)


def _station(s, t, dt):
    g = s.get_atm()
    nhit, idx, rows = s.station_hits(t, float(g["lon"][4]), float(g["lat"][4]), 800.0, -1e100, 1e100)
    assert nhit >= 1 and idx is not None
    return np.array([nhit]), idx, rows


# (particles, quantities, what is called behind the phase's time steps)
PHASES = [(3000, Q3, (_grid(4, 2, 1), _box)),
          (1500, Q3, (_grid(36, 18, 5), _sample)),
          (2250, Q3, (_grid(4, 2, 1), _station)),
          (2250, Q1, (_grid(36, 18, 5), _box, _sample, _station)),
          (4500, Q5, (_grid(4, 2, 1), _grid(36, 18, 5), _box, _sample, _station))]


def test_grow_shrink_and_other_quantity_counts():
    """3000 -> 1500 -> 2250 -> 4500 particles with 3 -> 1 -> 5 quantities, module_sort and module_mixing in every step (the
    sort ahead, the adoption of its buffers and the order repair all run), six steps per phase; behind each phase gridded
    sums on a 4 x 2 x 1 and a 36 x 18 x 5 grid in turn and the box sums, sample and station outputs."""
    def inputs(n, names):
        ctl, clim, m0, m1, atm = cases.make_case("full", n=n, seed=100 + n, quantities=names)
        return dict(ctl, sort_dt=180.0, mixing_dt=180.0), clim, m0, m1, atm
    ctl, clim, m0, m1, atm = inputs(*PHASES[0][:2])
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.timesteps_init(0.0, 0.0)
    ts = cases.step_times(s.ctl)[:6]
    dt = s.ctl.dt_mod
    for k, (n, names, calls) in enumerate(PHASES):
        ctl, _, _, _, atm = inputs(n, names)
        if k:
            _requantify(s, ctl)
            s.replace_particles(atm)
        assert s.nq == len(names) and s.n == n
        ctr = s.get_cache()["rng_ctr"]
        f = hip.Simulation(ctl, clim, m0, m1, atm, rng_ctr=ctr)
        f.timesteps_init(0.0, 0.0)
        for t in ts:
            s.run_timestep(t)
            f.run_timestep(t)
        _same_state(s.state(), f.state(), (k, "steps"))
        for call in calls:
            got, ref = call(s, ts[-1], dt), call(f, ts[-1], dt)
            assert len(got) == len(ref)
            for a, b in zip(got, ref):
                assert np.array_equal(a, b), (k, call)
            assert any(np.count_nonzero(a) for a in got), (k, call)
        _same_state(s.state(), f.state(), (k, "outputs"))
        f.close()
    s.close()


# ---------------------------------------------------------------------------
# b. random permutations through records
# ---------------------------------------------------------------------------

def test_record_path_of_the_random_permutation():
    """70001 particles (just above the 65536 from which permute_random moves the arrays through one record per particle),
    then 66000, then 70001 again in one context, re-sorted for locality before every step so that the stored order is not
    the caller's: every set against a fresh context and against the array-by-array kernels (perm_records 0)."""
    sets = {n: cases.make_case("diff", n=n, seed=100 + n) for n in (70001, 66000)}
    ctl, clim, m0, m1, atm = sets[70001]
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.set_option("locality_sort_interval", 1)
    s.timesteps_init(0.0, 0.0)
    ts = cases.step_times(s.ctl)[:3]
    for k, n in enumerate((70001, 66000, 70001)):
        atm = sets[n][4]
        if k:
            s.replace_particles(atm)
        ctr = s.get_cache()["rng_ctr"]
        others = []
        for records in (1, 0):
            f = hip.Simulation(ctl, clim, m0, m1, atm, rng_ctr=ctr)
            f.set_option("locality_sort_interval", 1)
            f.set_option("perm_records", records)
            f.timesteps_init(0.0, 0.0)
            others.append(f)
        for t in ts:
            for c in [s] + others:
                c.run_timestep(t)
        got = s.state()
        assert not np.array_equal(got["lon"], atm["lon"])
        for f, name in zip(others, ("fresh", "perm_records 0")):
            _same_state(got, f.state(), (k, n, name))
            f.close()
    s.close()


# ---------------------------------------------------------------------------
# c. the occupied-level exchange of module_mixing
# ---------------------------------------------------------------------------

MIX_GRID = (-180.0, 180.0, 128, -90.0, 90.0, 64, 0.0, 32.0, 32)      # 2^18 boxes of 1 km depth: level = (int) z
MIX_T, MIX_N = 360.0, 2000


def _band_particles(z_lo, z_hi, seed):
    """MIX_N particles inside the time window of MIX_T with heights spread evenly over [z_lo, z_hi)"""
    rng = np.random.default_rng(seed)
    z = z_lo + (z_hi - z_lo) * (np.arange(MIX_N) + 0.5) / MIX_N
    rng.shuffle(z)
    return {"time": np.full(MIX_N, MIX_T), "lon": rng.uniform(-180.0, -90.0, MIX_N), "lat": rng.uniform(0.0, 45.0, MIX_N),
            "p": box_cases.P0 * np.exp(-z / box_cases.H0), "q": rng.uniform(1.0, 2.0, (2, MIX_N))}


def _levels(atm):
    cell = box_cases.cells(MIX_GRID, atm, MIX_T, 180.0)
    assert (cell >= 0).all()
    return sorted(set((cell % MIX_GRID[8]).tolist()))


def test_occupied_level_exchange_with_another_mixed_set_and_band():
    """module_mixing with the exchange of the occupied levels (option mix_exchange_levels, a one-rank hook that leaves the
    data alone): two mixed quantities in a band of 4 levels, then one mixed quantity in a band of 6 levels.  The second
    step needs less for the sums of the band and more for its counts than the first: each of the two buffers is
    reserved for what it holds.  Each phase equals a fresh context with the option and one with the whole-grid exchange."""
    from mptrac_amd.ctl import ctl_from_quantities
    m0, m1 = box_cases.setup("A")[2:]
    clim = cases.load_clim_tropo()
    ctl = dict(cases.BASE, mixing_trop=0.4, mixing_strat=0.1, mixing_dt=180.0, **ctl_from_quantities(("m", "vmr")))
    ctl.update(box_cases.grid_keys("mixing", MIX_GRID))
    phases = [(dict(ctl), _band_particles(10.1, 13.9, 1)), (dict(ctl, qnt_vmr=-1), _band_particles(8.1, 13.9, 2))]
    assert _levels(phases[0][1]) == [10, 11, 12, 13] and _levels(phases[1][1]) == [8, 9, 10, 11, 12, 13]
    nz, ntot = MIX_GRID[8], MIX_GRID[2] * MIX_GRID[5] * MIX_GRID[8]
    assert 8 <= nz <= 256 and ntot == 1 << 18           # the smallest grid that takes the path

    def context(kw, atm, levels):
        c = hip.Simulation(kw, clim, m0, m1, atm)
        c.set_option("mix_exchange_levels", levels)
        seen = []
        c.set_allreduce(lambda ptr, count: seen.append(count))
        return c, seen

    s, seen = context(*phases[0], 1)
    for k, (kw, atm) in enumerate(phases):
        if k:
            _requantify(s, kw)
            s.replace_particles(atm)
        del seen[:]
        s.module("mixing", MIX_T)
        got = s.state()
        nmixed, nl = 2 - k, 4 + 2 * k
        per = MIX_GRID[2] * MIX_GRID[5] * nl
        assert seen == [nz, nmixed * per, per], (k, seen)       # the occupancy, then the sums and the counts of the band
        assert not np.array_equal(got["q"][0], atm["q"][0])     # (mixing did something)
        assert np.array_equal(got["q"][1], atm["q"][1]) == bool(k)
        for levels in (1, 0):
            f, _ = context(kw, atm, levels)
            f.module("mixing", MIX_T)
            _same_state(got, f.state(), (k, levels))
            f.close()
    s.close()


# ---------------------------------------------------------------------------
# d. mphip_set_option
# ---------------------------------------------------------------------------

FLAGS = ("fuse_sort", "lazy_meteo", "pin_host_atm", "fold_resort", "turb_strat", "fuse_sort_quantities", "perm_records",
         "big_grid", "xcd_map", "generic_kernel", "mix_exchange_levels", "ahead_priority", "emit_keys", "sort_repair",
         "compact_depo", "ahead_box", "sort_ahead", "grid_records", "locality_zorder")
PHASE_TEXT = ("derive_profile_phase must be 0 (kernels), 1 (uploads), 2 (downloads), 3 (the weight table of "
              "mphip_detrend_met) or 4, 5, 6 (the extremes, their reduction, the quantisation of mphip_pack_met)")
# name: (accepted values, refused values, refusal text)
NUMBERS = {
    "locality_sort_interval": ((0, 1, 60, 100000), (-1,), "locality_sort_interval must be >= 0"),
    "step_blocks": ((8, 8192, 1048576), (7, 1048577), "step_blocks must be in 8 ... 1048576"),
    "step_blocks_multi": ((8, 32768, 1048576), (7, 1048577), "step_blocks must be in 8 ... 1048576"),
    "multi_step": ((0, 64, 4096), (-1, 4097), "multi_step must be in 0 ... 4096"),
    "derive_profile_phase": ((0, 1, 2, 3, 4, 5, 6), (-1, 7, 0.5), PHASE_TEXT),
    "sort_bits": ((0, 8, 9, 10), (-1, 1, 7, 11), "sort_bits must be 0 (automatic), 8, 9 or 10"),
    "lds_tile": ((0, 64, 2400), (-1, 1, 63, 2401), "lds_tile must be 0 or 64 ... 2400 cells"),
    "sum_path": ((0, 1, 2), (-1, 3, 0.5), "sum_path must be 0, 1 or 2"),
    "deterministic_sums": ((0, 1), (-1, 2, 0.5), "deterministic_sums must be 0 or 1"),
    "chain_blocks": ((0, 1, 4096), (), None),
    "locality_tile": ((0, 4, 64), (-1, 65), "locality_tile must be in 0 ... 64"),
}


def test_every_option_is_accepted_and_refused_as_documented():
    assert len(FLAGS) + len(NUMBERS) == 30 and not set(FLAGS) & set(NUMBERS)
    ctl, clim, m0, m1, atm = cases.make_case("full", n=97)
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    for name in FLAGS:
        for value in (0, 1, 0, 2, -1, 0.5):
            s.set_option(name, value)
    for name, (accepted, refused, text) in NUMBERS.items():
        for value in accepted:
            s.set_option(name, value)
        for value in refused:
            with pytest.raises(hip.MphipError) as exc:
                s.set_option(name, value)
            assert str(exc.value) == text, (name, value)
    with pytest.raises(hip.MphipError) as exc:
        s.set_option("no_such_option", 1)
    assert str(exc.value) == "unknown option no_such_option"
    s.close()
