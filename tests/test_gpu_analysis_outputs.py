"""The particle loops of write_csi / write_prof, write_sample and write_station on the device (mphip_box_sums,
mphip_sample_obs, mphip_station_hits) against their transcription in tests/refanalysis.py: counts, hit lists, flags AND
sums are compared with array_equal -- the decisions are made with the C library's bits and every sum is added in the
host loop's order.  Here in the library the process has loaded; tests/test_gpu_analysis_outputs_exact.py repeats the
comparisons in the reference-rounding build (MPTRAC_AMD_EXACT=1) in a child process.  With the
internal locality order off and re-sorted every 3 steps, after several time steps, on 97, 6000 and 10^6 particles, with
longitudes in [-180, 180) and in [0, 360).

Before anything is compared the inputs are checked ON THE REFERENCE to exercise what they are meant to: every rejection
of write_sample removes particles, observations with and without particles, a long chain, a particle in two cylinders,
several ensemble members, a weighting function, particles on both sides of every box bound, flagged particles and a
station buffer that is too small at first."""
import threading

import numpy as np
import pytest

import cases
import refanalysis as R
from mptrac_amd import hip
from mptrac_amd.synth import synthetic_particles

pytestmark = pytest.mark.gpu

QUANTITIES = ("m", "ens", "stat")
QM, QENS, QSTAT = 0, 1, 2
NMEMBER = 3
KERNEL = (np.array([0.0, 5.0, 12.0, 30.0]), np.array([0.2, 1.0, 0.6, 0.1]))
T_LATE = 5000.0           # release time of the particles that are not part of the time steps looked at
STEPS = 4


def _inputs(n, lon0):
    """particles and meteo data with longitudes from lon0; ensembles, flags, late releases, a cluster for the station"""
    ctl, clim, met0, met1, _ = cases.make_case("diff", n=8, quantities=QUANTITIES, lon0=lon0)
    atm = synthetic_particles(n, seed=4711, quantities=QUANTITIES, lon=(lon0, lon0 + 360.0))
    ip = np.arange(n)
    atm["q"][QENS] = ip % NMEMBER
    atm["q"][QSTAT] = (ip % 4 == 0).astype(float)
    atm["time"][ip % 11 == 10] = T_LATE
    for k in (5, 6, 7):      # three neighbours of particle 4 (which carries the flag): the station is put there
        atm["lon"][k] = atm["lon"][4] + 0.3 * (k - 4)
        atm["lat"][k] = atm["lat"][4] + 0.2 * (k - 4)
        atm["p"][k] = atm["p"][4]
    return ctl, clim, met0, met1, atm


def _stepped(n, lon0, interval, shard=None, steps=STEPS):
    """(context, time of the last step, DT_MOD) after `steps` time steps.  steps = 0: the particles as uploaded, looked at
    at their release time -- the only way to keep longitudes in [0, 360), since module_position brings every longitude
    into [-180, 180) in every step."""
    ctl, clim, met0, met1, atm = _inputs(n, lon0)
    s = hip.Simulation(ctl, clim, met0, met1, atm, shard=shard)
    s.set_option("locality_sort_interval", interval)
    s.timesteps_init(0.0, 0.0)
    dt = s.ctl.dt_mod
    for k in range(steps):
        s.run_timestep(k * dt)
    return s, max(steps - 1, 0) * dt, dt


def _boxes(lon0):
    csi = (lon0 + 90.0, lon0 + 300.0, 21, -40.0, 60.0, 10, 2.0, 25.0, 1)
    # (no particle gets beyond 87 degrees in these few steps: the observations next to the pole lie in empty columns)
    prof = (lon0 + 120.0, lon0 + 240.0, 12, -43.0, 127.0, 17, 0.0, 24.0, 8)
    return csi, prof


def _observations(state, n):
    """24 observations: eight at particles, one next to the first, one whose layer misses its particle, random ones, and
    six next to the pole"""
    rng = np.random.default_rng(99)
    at = []
    for k in range(8):       # (not one of the late releases)
        ip = (k * n) // 8
        while ip % 11 == 10:
            ip += 1
        at.append(ip)
    lon, lat, z = [], [], []
    for ip in at:
        lon.append(state["lon"][ip])
        lat.append(state["lat"][ip])
        z.append(R.Z(float(state["p"][ip])))
    lon.append(lon[0] + 1.0), lat.append(lat[0] + 0.5), z.append(z[0])         # overlaps observation 0
    lon.append(lon[1]), lat.append(lat[1]), z.append(z[1] + 10.0)              # same place, layer 10 km above
    for _ in range(8):
        lon.append(float(rng.uniform(state["lon"].min(), state["lon"].max())))
        lat.append(float(rng.uniform(-80.0, 80.0)))
        z.append(float(rng.uniform(2.0, 25.0)))
    for k in range(6):
        lon.append(lon[k]), lat.append(89.5), z.append(60.0)       # (no particle up there)
    return np.array(lon), np.array(lat), np.array(z)


def _check_everything(s, t, dt, n, lon0, long_chain):
    state = s.get_atm()
    assert state["lon"].min() >= lon0 and state["lon"].max() < lon0 + 360.0
    if lon0 == 0.0:
        assert state["lon"].max() > 300.0       # the case in [0, 360)
    else:
        assert state["lon"].min() < -100.0 and state["lon"].max() > 100.0
    xyz = R.cartesian(state)
    csi, prof = _boxes(lon0)

    # ---- box sums: CSI (members, weighting function) and profiles (one member, none) ----
    ref = R.box_sums(state, csi, t, dt, QM, NMEMBER, QENS, KERNEL)
    zs = np.array([R.Z(p) for p in state["p"].tolist()])
    assert NMEMBER >= 2 and len(KERNEL[0]) >= 3
    for lo, hi, v in ((csi[0], csi[1], state["lon"]), (csi[3], csi[4], state["lat"]), (csi[6], csi[7], zs)):
        assert (v < lo).any() and ((v >= lo) & (v < hi)).any() and (v >= hi).any()      # particles on both sides of every bound
    assert all((ref[e] > 0).any() for e in range(NMEMBER))
    got = s.box_sums(csi, t, QM, NMEMBER, QENS, KERNEL)
    assert np.array_equal(got, ref)
    ref = R.box_sums(state, prof, t, dt, QM)
    col = ref.reshape(prof[2] * prof[5], prof[8]).sum(axis=1)
    olon, olat, oz = _observations(state, n)
    ocol = np.array([R.box_cell(prof[:6] + (0.0, 1.0, 1), lo, la, 0.5) for lo, la in zip(olon.tolist(), olat.tolist())])
    ocol = np.unique(ocol[ocol >= 0])                                                   # the columns that hold observations ...
    assert (col[ocol] > 0).any() and (col[ocol] == 0).any()                             # ... with and without mass in them
    for path in (0, 1, 2):       # by crowding, the group and the chain algorithm of the ordered sums
        s.set_option("sum_path", path)
        assert np.array_equal(s.box_sums(prof, t, QM), ref), path
    s.set_option("sum_path", 0)

    # ---- samples ----
    dx, dz = 800.0, 6.0
    t0, t1 = t - 0.5 * dt, t + 0.5 * dt
    count, mass, stages, hits = R.sample_obs(state, t0, t1, olon, olat, oz, dx, dz, QM, KERNEL, xyz)
    assert stages[0][0] < n                                            # the time window removes particles ...
    assert any(a > b for a, b, _, _ in stages)                         # ... the latitude band ...
    assert any(b > c for _, b, c, _ in stages)                         # ... the distance ...
    assert any(c > d for _, _, c, d in stages)                         # ... and the depth of the layer
    assert 3 * np.count_nonzero(count) >= len(count) and (count == 0).any()
    seen = np.zeros(n, dtype=int)
    for idx in hits:
        seen[idx] += 1
    assert seen.max() >= 2                                             # a particle inside two cylinders
    if long_chain:
        assert count.max() >= 1000
    gcount, gmass = s.sample_obs(t0, t1, olon, olat, oz, dx, dz, KERNEL)
    assert np.array_equal(gcount, count)
    assert np.array_equal(gmass, mass)
    # no depth test, no weighting function, a small radius
    count, mass, _, _ = R.sample_obs(state, t0, t1, olon, olat, oz, 50.0, -999.0, QM, xyz=xyz)
    gcount, gmass = s.sample_obs(t0, t1, olon, olat, oz, 50.0, -999.0)
    assert np.array_equal(gcount, count) and np.array_equal(gmass, mass)
    assert count[:8].min() >= 1

    # ---- station: at particle 4, which carries the flag; its neighbours do not ----
    slon, slat, r = float(state["lon"][4]), float(state["lat"][4]), 800.0
    listed, rows, q_after, skipped = R.station_hits(state, t, dt, slon, slat, r, -1e100, 1e100, QSTAT, xyz)
    assert skipped >= 1 and len(listed) >= 2 and state["q"][QSTAT][4] == 1
    nhit, idx, got = s.station_hits(t, slon, slat, r, -1e100, 1e100, QSTAT, cap=len(listed) - 1)
    assert nhit == len(listed) and idx is None                         # too small a buffer: the number, nothing else ...
    assert np.array_equal(s.get_atm()["q"], state["q"])                # ... and no flag has changed
    nhit, idx, got = s.station_hits(t, slon, slat, r, -1e100, 1e100, QSTAT, cap=nhit)
    assert nhit == len(listed) and np.array_equal(idx, listed) and np.array_equal(got, rows)
    assert (got[:, 4 + QSTAT] == 1).all()
    after = s.get_atm()
    assert np.array_equal(after["q"], q_after)                         # the flags were set on the device
    for k in ("time", "p", "lon", "lat"):
        assert np.array_equal(after[k], state[k])
    nhit, idx, got = s.station_hits(t, slon, slat, r, -1e100, 1e100, QSTAT, cap=8)
    assert nhit == 0                                                   # every particle is listed once
    # without a flag quantity, inside a station time window that excludes everything / nothing
    listed, rows, _, _ = R.station_hits(after, t, dt, slon, slat, r, -1e100, 1e100, -1, xyz)
    nhit, idx, got = s.station_hits(t, slon, slat, r, -1e100, 1e100, -1, cap=len(listed))
    assert np.array_equal(idx, listed) and np.array_equal(got, rows)
    assert s.station_hits(t, slon, slat, r, t + dt, 1e100, -1, cap=4)[0] == 0


@pytest.mark.parametrize("interval", [0, 3])
@pytest.mark.parametrize("n", [97, 6000])
def test_analysis_outputs_equal_the_host_loops(n, interval):
    s, t, dt = _stepped(n, -180.0, interval)
    _check_everything(s, t, dt, n, -180.0, long_chain=False)
    s.close()


@pytest.mark.parametrize("steps", [0, 1])
@pytest.mark.parametrize("n", [97, 6000])
def test_analysis_outputs_equal_the_host_loops_with_longitudes_in_0_360(n, steps):
    """Particles and observations with longitudes in [0, 360): cos / sin of up to 2 pi (the wide branch of the C
    library's functions), boxes beyond 180 degrees.  On the particles as uploaded (see _stepped); steps = 1: after the
    time step at the release time, which moves no particle (dt = 0) but stores them in the locality order first, so the
    kernels read these longitudes through a permutation."""
    s, t, dt = _stepped(n, 0.0, 3, steps=steps)
    _check_everything(s, t, dt, n, 0.0, long_chain=False)
    s.close()


def test_analysis_outputs_equal_the_host_loops_at_1e6_particles():
    n = 10 ** 6
    s, t, dt = _stepped(n, -180.0, 3)
    _check_everything(s, t, dt, n, -180.0, long_chain=True)
    s.close()


def test_wide_cos_sin_on_the_device_are_the_c_librarys():
    """libm_cos_wide / libm_sin_wide as the kernels evaluate them against the C library: every quarter degree and 2 x 10^6
    arguments up to 7 (the CPU comparison of the same header, tests/test_libm_sincos_wide.py, covers 10^8)."""
    import math
    ctl, clim, met0, met1, atm = _inputs(97, -180.0)
    s = hip.Simulation(ctl, clim, met0, met1, atm)
    rng = np.random.default_rng(7)
    x = np.concatenate([np.arange(-720, 1441) * 0.25 * (math.pi / 180.0), rng.uniform(-7.0, 7.0, 2_000_000),
                        rng.uniform(-1e5, 1e5, 200_000)])
    assert np.array_equal(s.test_libm("cos_wide", x), np.array([math.cos(v) for v in x.tolist()]))
    assert np.array_equal(s.test_libm("sin_wide", x), np.array([math.sin(v) for v in x.tolist()]))
    s.close()


def test_error_returns():
    s, t, dt = _stepped(97, -180.0, 3)
    csi, _ = _boxes(-180.0)
    state = s.get_atm()
    # a member outside [0, nmember): the error names the particle; checked before the box test
    bad = state["q"][QENS].copy()
    bad[50] = NMEMBER
    bad[70] = -1
    s.update_quantity(QENS, bad)
    with pytest.raises(hip.MphipError, match=r"Ensemble ID out of range! \(particle 50\)"):
        s.box_sums(csi, t, QM, NMEMBER, QENS)
    with pytest.raises(R.MemberOutOfRange):
        R.box_sums(dict(state, q=np.vstack([state["q"][QM], bad, state["q"][QSTAT]])), csi, t, dt, QM, NMEMBER, QENS)
    assert s.box_sums(csi, t, QM).shape == (1, csi[2] * csi[5] * csi[8])          # without members the call is fine
    s.update_quantity(QENS, state["q"][QENS])
    # MET_COORD_TYPE 1
    s.ctl.met_coord_type = 1
    s.update_ctl()
    for call in (lambda: s.box_sums(csi, t, QM), lambda: s.sample_obs(t - dt, t + dt, [0.0], [0.0], [10.0], 50.0),
                 lambda: s.station_hits(t, 0.0, 0.0, 50.0, -1e100, 1e100)):
        with pytest.raises(hip.MphipError, match="Only lat/lon grid supported"):
            call()
    s.ctl.met_coord_type = 0
    s.update_ctl()
    s.close()
    # the station output with an index range that is not the whole simulation
    s, t, dt = _stepped(97, -180.0, 3, shard=(0, 48))
    with pytest.raises(hip.MphipError, match="all particles in one process"):
        s.station_hits(t, 0.0, 0.0, 50.0, -1e100, 1e100)
    s.close()


def test_two_index_range_shards_give_the_sums_of_the_partials():
    """Two shards on one GPU, one host thread each, their box sums and sample counts / masses added through the hook of
    mphip_set_allreduce: every rank holds the sum of the two partial results (each partial = the host loop over the
    shard's particles)."""
    from test_gpu_full_size import _ThreadAllreduce
    n, world, lon0 = 6000, 2, -180.0
    one, t, dt = _stepped(n, lon0, 3)
    state = one.get_atm()
    one.close()
    csi, _ = _boxes(lon0)
    olon, olat, oz = _observations(state, n)
    t0, t1 = t - 0.5 * dt, t + 0.5 * dt
    parts = []
    for rank in range(world):
        lo, hi = hip.shard_range(n, rank, world)
        sub = {k: (v[lo:hi] if k != "q" else v[:, lo:hi]) for k, v in state.items()}
        c, m, _, _ = R.sample_obs(sub, t0, t1, olon, olat, oz, 800.0, 6.0, QM, KERNEL)
        parts.append((R.box_sums(sub, csi, t, dt, QM, NMEMBER, QENS, KERNEL), c, m))
    want = (parts[0][0] + parts[1][0], parts[0][1] + parts[1][1], parts[0][2] + parts[1][2])
    assert (parts[0][1] > 0).any() and (parts[1][1] > 0).any()
    ar = _ThreadAllreduce(world)
    results, errors = [None] * world, []

    def rank_main(rank):
        try:
            s, _, _ = _stepped(n, lon0, 3, shard=hip.shard_range(n, rank, world))
            s.set_allreduce(ar.hook(rank))
            box = s.box_sums(csi, t, QM, NMEMBER, QENS, KERNEL)
            count, mass = s.sample_obs(t0, t1, olon, olat, oz, 800.0, 6.0, KERNEL)
            results[rank] = (box, count, mass)
            s.close()
        except BaseException as exc:      # noqa: BLE001  (a dead rank must not leave the other at the barrier)
            errors.append((rank, repr(exc)))
            ar.barrier.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for rank in range(world):
        for got, ref in zip(results[rank], want):
            assert np.array_equal(got, ref), rank
