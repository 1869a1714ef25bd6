"""What a multi-step launch (mphip_run_timesteps, the kMultiStep instantiations) keeps per particle for all of its
steps -- the external index the random numbers belong to, and the sedimentation's q[rp] and q[rhop], parked in LDS
once per particle -- against the same steps one launch each (mphip_run_timestep), bit for bit: time, position, the
mesoscale perturbations, EVERY quantity array, cache->dt and the random-number counter.

rp and rhop differ from particle to particle (seeded uniform draws of 1 ... 20 times the case's 1 um and 0.5 ... 2
times its 1000 kg/m3: terminal velocities from 1e-4 to 5e-2 m/s, far above the last bit of p), so that a value read
from another thread's slot, or from the particle a thread walked before, moves p.  n = 1000 is no multiple of the
workgroup size: the last workgroup is partial.  The block partition gives every workgroup at least 256 particles, so
a thread walks a second particle (and reuses its slot) only beyond 8 x 256 particles with the fewest blocks the
option allows: the case with n = 3000."""
import numpy as np
import pytest

import cases
from mptrac_amd import hip

pytestmark = pytest.mark.gpu

DT = cases.BASE["dt_mod"]
STATE = ("time", "lon", "lat", "p", "uvwp", "q", "dt")


def _inputs(n, release=None, sort_dt=None):
    ctl, clim, m0, m1, atm = cases.make_case("conv_sedi", n=n)
    if sort_dt:
        ctl = dict(ctl, sort_dt=sort_dt)
    rng = np.random.default_rng(20240607)
    q = list(cases.QUANTITIES)
    atm["q"][q.index("rp")] = rng.uniform(1.0, 20.0, n)
    atm["q"][q.index("rhop")] = rng.uniform(500.0, 2000.0, n)
    if release is not None:     # every seventh particle is released later: dt = 0 for it in the steps before
        atm["time"][::7] = release * DT
    return ctl, clim, m0, m1, atm


def _final_state(inputs, t0, nsteps, multi, blocks=None):
    ctl, clim, m0, m1, atm = inputs
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    try:
        if blocks:
            s.set_option("step_blocks_multi", blocks)
        s.timesteps_init(float(atm["time"].min()), float(atm["time"].max()))
        if multi:
            s.run_timesteps(t0, nsteps)
        else:
            for k in range(nsteps):
                s.run_timestep(t0 + k * DT)
        g = s.state()
        cache = s.get_cache()
        g["dt"] = cache["dt"]
        g["rng_ctr"] = cache["rng_ctr"]
    finally:
        s.close()
    return g


def _compare(inputs, t0, nsteps, blocks=None):
    one = _final_state(inputs, t0, nsteps, False, blocks)
    multi = _final_state(inputs, t0, nsteps, True, blocks)
    assert one["rng_ctr"] == multi["rng_ctr"]
    for k in STATE:
        assert np.array_equal(one[k], multi[k], equal_nan=True), k
    return one, multi


@pytest.mark.parametrize("nsteps", [1, 2, 6])
def test_per_particle_rp_rhop_and_ext(nsteps):
    inputs = _inputs(1000)
    one, multi = _compare(inputs, DT, nsteps)
    assert np.all(multi["time"] == nsteps * DT)
    q = list(cases.QUANTITIES)      # (the launch leaves the two quantities as they came)
    for name in ("rp", "rhop"):
        assert np.array_equal(multi["q"][q.index(name)], inputs[4]["q"][q.index(name)])


def test_a_thread_that_walks_several_particles_reuses_its_slot():
    # eight logical blocks of 512 particles (the last ones short or empty): threads walk two particles
    _compare(_inputs(3000), DT, 6, blocks=8)


def test_particles_released_inside_the_launch():
    one, multi = _compare(_inputs(1000, release=2.5), DT, 6)
    assert np.all(multi["time"][::7] == 6 * DT)      # (they did start)


def test_particles_that_never_start():
    # released behind the launch's last step: the step loop leaves with dt = 0 in every step
    inputs = _inputs(1000, release=4.5)
    one, multi = _compare(inputs, DT, 3)
    late = np.zeros(1000, dtype=bool)
    late[::7] = True
    assert np.all(multi["time"][late] == 4.5 * DT)
    assert np.all(multi["dt"][late] == 0)
    for k in ("lon", "lat", "p"):
        assert np.array_equal(multi[k][late], inputs[4][k][late]), k
    assert np.all(multi["time"][~late] == 3 * DT)


def test_launch_behind_module_sort():
    # SORT_DT = 4 DT_MOD and a call that starts at a multiple of it: the first step sorts (its launch gathers the
    # re-ordered particles, and the external indices are no longer the slots), the three steps behind it share a launch
    one, multi = _compare(_inputs(1000, sort_dt=4 * DT), 4 * DT, 4)
    assert np.all(multi["time"] == 7 * DT)
