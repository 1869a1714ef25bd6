"""Several time steps in one launch (mphip_run_timesteps, the kMultiStep instantiations) against the same steps one
launch each (mphip_run_timestep), bit for bit: positions, time, the mesoscale perturbations and the random-number
counter.  The multi-step kernels store the particle state once behind their last step; the cases below have
particles released inside the launch (dt = 0 in its first steps, so that the step loop leaves early for them) and
the boundary-layer closure, whose perturbations a multi-step launch holds in registers."""
import numpy as np
import pytest

import cases
from mptrac_amd import hip

pytestmark = pytest.mark.gpu

NSTEPS = 6


def _final_state(name, multi, late):
    ctl, clim, m0, m1, atm = cases.make_case(name, n=10000)
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    dt = s.ctl.dt_mod
    if late:   # every seventh particle released in the middle of the launch: dt = 0 in its first steps
        atm = dict(atm)
        atm["time"] = atm["time"].copy()
        atm["time"][::7] = 2.5 * dt
        s.close()
        s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.timesteps_init(float(atm["time"].min()), float(atm["time"].max()))
    t0 = dt
    if multi:
        s.run_timesteps(t0, NSTEPS)
    else:
        for k in range(NSTEPS):
            s.run_timestep(t0 + k * dt)
    g = s.state()
    g["rng_ctr"] = s.get_cache()["rng_ctr"]
    g["dt"] = dt
    s.close()
    return g


@pytest.mark.parametrize("name,late", [("conv_sedi", False), ("conv_sedi", True), ("pbl_meso", True)])
def test_multi_step_launch_matches_one_launch_per_step(name, late):
    one = _final_state(name, False, late)
    multi = _final_state(name, True, late)
    assert one["rng_ctr"] == multi["rng_ctr"]
    for k in ("time", "lon", "lat", "p", "uvwp"):
        assert np.array_equal(one[k], multi[k], equal_nan=True), k
    if late:   # (the late particles did start inside the launch)
        assert np.all(multi["time"][::7] > 2.5 * multi["dt"])
