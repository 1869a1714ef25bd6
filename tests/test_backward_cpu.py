"""Backward runs (DIRECTION -1) on the CPU: what the device's backward tests (tests/test_gpu_backward*.py) rest on.

The oracle is their reference, so it is held first: the numpy restatement of the modules (tests/refmodules.py) against
the oracle with every case of tests/test_oracle_second_opinion.py reversed in time -- the same test bodies, 1e-13 --,
module_timesteps against a five-line statement of mptrac.c:6016-6041 for both directions, the start / stop time
arithmetic of the oracle, the Python harness and the C host layer against one another, and the driver loop
(tests/backward.py) over two hand-overs of mptrac_get_met's backward branch.

Not marked `gpu`: nothing here opens a device.  The host-layer checks compile tests/c/release_times.c against
lib/libmptrac.so, which links lib/libmptrac_hip.so, so -- like tests/test_host_logic.py's shard_times and reread_ctl --
they need the libraries that `build()` leaves in the tree."""
import subprocess

import numpy as np
import pytest

import backward
import cases
import test_oracle_second_opinion as SO
from mptrac_amd import hip
from oracle import binding as B


# ---------------------------------------------------------------------------
# second opinion, backward
# ---------------------------------------------------------------------------

class TestSecondOpinionBackward:
    """Every test of tests/test_oracle_second_opinion.py (their bodies, their 1e-13) with DIRECTION -1, T_STOP 0 and the
    particle times mirrored (3600 - time).  The bodies assert on their inputs (SO._timesteps): the control's direction
    is -1, released particles have dt < 0, the late-released particles of the isosurf cases dt == 0."""

    @pytest.fixture(autouse=True)
    def _reversed(self, monkeypatch):
        monkeypatch.setattr(SO, "DIRECTION", -1)

    test_advect_pressure_levels = staticmethod(SO.test_advect_pressure_levels)
    test_old_latitude_rule_is_observable = staticmethod(SO.test_old_latitude_rule_is_observable)
    test_diff_turb_both_branches = staticmethod(SO.test_diff_turb_both_branches)
    test_vertical_probes_use_the_displaced_latitude = staticmethod(SO.test_vertical_probes_use_the_displaced_latitude)
    test_convection = staticmethod(SO.test_convection)
    test_sedimentation = staticmethod(SO.test_sedimentation)
    test_mixing = staticmethod(SO.test_mixing)
    test_wet_and_dry_deposition = staticmethod(SO.test_wet_and_dry_deposition)
    test_boundary_layer_closure = staticmethod(SO.test_boundary_layer_closure)
    test_advect_model_levels = staticmethod(SO.test_advect_model_levels)
    test_isosurface_modes = staticmethod(SO.test_isosurface_modes)
    test_boundary_condition_region_and_values = staticmethod(SO.test_boundary_condition_region_and_values)
    test_advect_pressure_with_model_level_winds = staticmethod(SO.test_advect_pressure_with_model_level_winds)
    test_meteo_fields_and_derived_quantities = staticmethod(SO.test_meteo_fields_and_derived_quantities)
    test_sort_keys_and_a_stable_order = staticmethod(SO.test_sort_keys_and_a_stable_order)

    def test_the_inputs_run_backward(self):
        """(the check of the checks: every second-opinion test is listed above -- a new one has to be added here --, and
        the shared bodies see negative steps and an unreleased seventh)"""
        assert {k for k in vars(SO) if k.startswith("test_")} <= set(vars(type(self)))
        o, _, t = SO._oracle("conv_sedi")
        assert o.ctl.direction == -1 and o.ctl.t_start == 3600.0 and o.ctl.t_stop == 0.0 and t == 3420.0
        assert np.all(o.dt == -180.0)
        ctl, clim, m0, m1, atm = SO._make_case("isosurf_rho", SO.N, 11)
        assert np.all(atm["time"][::7] == 3060.0) and np.all(np.delete(atm["time"], np.s_[::7]) == 3600.0)
        assert (m0.time, m1.time) == (0.0, 3600.0)


# ---------------------------------------------------------------------------
# module_timesteps
# ---------------------------------------------------------------------------

def _dt_statement(direction, t_start, t_stop, t, time):
    """mptrac.c:6016-6041 on a global grid: a particle inside [t_start, t_stop] (in the direction of travel) that the
    call's time has passed steps to that time, every other particle not at all."""
    d = direction
    moves = (d * (time - t_start) >= 0) & (d * (time - t_stop) <= 0) & (d * (time - t) < 0)
    return np.where(moves, t - time, 0.0)


def _beside(x):
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


@pytest.mark.parametrize("direction,t_start,t_stop", [(-1, 3600.0, 90.0), (1, 0.0, 3510.0), (-1, 0.0, -7110.0),
                                                      (1, -7200.0, -90.0)])
def test_module_timesteps_against_its_statement(direction, t_start, t_stop):
    """The oracle's dt, for equality, at particle times on the DT_MOD raster and off it, exactly at t_start, t_stop and
    the time of the call, one ulp either side of each, and beyond both ends -- for calls at the start, in the middle,
    at a time off the raster, at t_stop (the short last step) and one step before it."""
    dt_mod = 180.0
    calls = [t_start, t_start + direction * dt_mod, t_start + direction * 9 * dt_mod, t_start + direction * 1237.0,
             t_stop - direction * (abs(t_stop - t_start) % dt_mod), t_stop]
    for t in calls:
        times = []
        for x in (t_start, t_stop, t):
            times += _beside(x)
        times += [t_start + direction * dt_mod * k for k in range(-2, 23)]                  # the raster, past both ends
        times += [t_start + direction * (dt_mod * k + 37.0) for k in range(-2, 23)]          # off it
        times += [t_start - direction * 500.0, t_stop + direction * 500.0, -1e9, 1e9, 0.0]
        time = np.array(times)
        ctl, clim, m0, m1, atm = cases.make_case("advect", n=len(time), grid="tiny")
        ctl.update(direction=direction, t_stop=t_stop)
        atm["time"] = time.copy()
        o = B.Oracle(ctl, clim, m0, m1, atm)
        o.ctl.t_start = t_start
        o.module("timesteps", t)
        want = _dt_statement(direction, t_start, t_stop, t, time)
        assert np.array_equal(o.dt, want), (t, time[o.dt != want])
        assert np.all(direction * o.dt >= 0)
        if t != t_start:
            assert np.count_nonzero(o.dt) >= 3 and np.count_nonzero(o.dt == 0) > 5, t
        assert np.array_equal(o.time, time)


# ---------------------------------------------------------------------------
# start / stop time, the driver's step times
# ---------------------------------------------------------------------------

def _host_range(tmin, tmax, direction, dt_mod, t_stop):
    from hostfiles import compile_c_test
    exe = compile_c_test("release_times")
    args = [exe, repr(tmin), repr(tmax), "DIRECTION", str(direction), "DT_MOD", repr(dt_mod)]
    if t_stop is not None:
        args += ["T_STOP", repr(t_stop)]
    return subprocess.run(args, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("direction,tmin,tmax,t_stop,want", [
    (-1, 1000.0, 3677.0, 95.0, (3780.0, 95.0)),            # start off the raster: rounded UP; stop off the raster
    (-1, 1000.0, 3600.0, 0.0, (3600.0, 0.0)),
    (-1, -5000.0, -3677.0, -7295.0, (-3600.0, -7295.0)),   # negative times: ceil rounds towards zero
    (-1, -5000.0, -100.0, -9000.0, (0.0, -9000.0)),
    (-1, 777.0, 3677.0, None, (3780.0, 777.0)),            # no T_STOP: the earliest release
    (1, 3677.0, 5000.0, 7295.0, (3600.0, 7295.0)),
    (1, -3677.0, -1000.0, None, (-3780.0, -1000.0))])
def test_start_and_stop_time_of_a_backward_run(direction, tmin, tmax, t_stop, want):
    """module_timesteps_init three times -- the oracle's (from the particle array), the harness's
    (hip.timestep_range, what Simulation.timesteps_init hands to the device) and the C host layer's (release_time_range
    + module_timesteps_init through tests/c/release_times.c) -- and the step times of the driver loop that follow."""
    dt_mod = 180.0
    ctl, clim, m0, m1, atm = cases.make_case("advect", n=3, grid="tiny")
    ctl.update(direction=direction, dt_mod=dt_mod, t_stop=1e100 if t_stop is None else t_stop)
    atm["time"][:] = (0.5 * (tmin + tmax), tmax, tmin)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    assert (o.ctl.t_start, o.ctl.t_stop) == want
    assert hip.timestep_range(direction, dt_mod, 1e100 if t_stop is None else t_stop, tmin, tmax) == want
    res = _host_range(tmin, tmax, direction, dt_mod, t_stop)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT")][-1].split()
    assert (float(line[1]), float(line[2])) == want
    # the driver loop: from t_start in steps of DT_MOD, the last step shortened to end at t_stop
    times = cases.step_times(o.ctl)
    whole = int(np.ceil(direction * (want[1] - want[0]) / dt_mod))
    assert times == [want[0] + direction * dt_mod * k for k in range(whole)] + [want[1]]
    assert 0 < direction * (times[-1] - times[-2]) <= dt_mod


def test_a_backward_run_with_nothing_to_do_is_refused():
    with pytest.raises(hip.MphipError, match="Nothing to do"):
        hip.timestep_range(-1, 180.0, 3600.0, 0.0, 3600.0)
    res = _host_range(0.0, 3600.0, -1, 180.0, 3600.0)
    assert res.returncode != 0 and "Nothing to do" in res.stdout + res.stderr


# ---------------------------------------------------------------------------
# the driver loop over two backward hand-overs
# ---------------------------------------------------------------------------

def test_oracle_over_two_backward_handovers():
    """Three hours backward over four snapshots (case `diff`, 1000 particles): two hand-overs; every particle ends at
    T_STOP; the run that forgets the hand-overs (the snapshots of the first interval extrapolated) ends elsewhere, far
    above the device tests' 1e-10 -- the hand-over is observable --; and a forward run with the same particles over the
    same snapshots crosses the same files in the other order."""
    ctl, clim, mets, atm = backward.backward_case("diff", 1000, grid="tiny", hours=3)
    assert [m.time for m in mets] == [0.0, 3600.0, 7200.0, 10800.0] and np.all(atm["time"] == 10800.0)
    o = B.Oracle(ctl, clim, *backward.initial_mets(mets, 10800.0), atm)
    assert (o.met[0].time, o.met[1].time) == (7200.0, 10800.0)
    backward.start(o, atm["time"])
    times = cases.step_times(o.ctl)
    assert len(times) == 61 and times[0] == 10800.0 and times[-1] == 0.0
    backward.run_backward(o, mets, times, handovers=2)
    assert (o.met[0].time, o.met[1].time) == (0.0, 3600.0)
    assert np.all(o.time == 0.0) and np.all(np.isfinite(o.lon)) and np.all(np.isfinite(o.p))
    forgetful = B.Oracle(ctl, clim, mets[2], mets[3], atm)
    backward.start(forgetful, atm["time"])
    for t in times:
        forgetful.run_timestep(t)
    assert np.all(forgetful.time == 0.0)
    assert max(cases.rel_err(getattr(forgetful, k), getattr(o, k)) for k in ("lon", "lat", "p")) > 1e-6
    fwd = B.Oracle(dict(ctl, direction=1, t_stop=10800.0), clim, mets[0], mets[1], dict(atm, time=np.zeros(1000)))
    fwd.timesteps_init()
    backward.run_forward(fwd, mets, cases.step_times(fwd.ctl), handovers=2)
    assert np.all(fwd.time == 10800.0) and (fwd.met[0].time, fwd.met[1].time) == (7200.0, 10800.0)


@pytest.mark.parametrize("case,over", [("conv_sedi", {}), ("full", dict(sort_dt=0.0))], ids=["conv_sedi", "full-unsorted"])
def test_staggered_release_times_hold_what_the_device_tests_need(case, over):
    """tests/backward.py:staggered_times -- inside (t_stop, t_start] except six particles that never move, a third off
    the raster, and at every call from the second down to t = 360 a particle whose time EQUALS the call's time while
    others still wait for their release."""
    ctl, clim, mets, atm = backward.backward_case(case, 3000, grid="tiny", staggered=True, t_stop=90.0, **over)
    time = atm["time"]
    never = backward.never_released(time, 3600.0, 90.0)
    assert never.sum() == 6 and (time > 3600.0).sum() == 2 and (time == 90.0).sum() == 1
    assert np.all((time[~never] > 90.0) & (time[~never] <= 3600.0))
    off = (time[~never] % 180.0) != 0
    assert 900 < off.sum() < 1100
    o = B.Oracle(ctl, clim, *backward.initial_mets(mets, 3600.0), atm)
    backward.start(o, time, t_start=3600.0)
    times = cases.step_times(o.ctl)
    assert times[-1] == 90.0 and times[-2] == 180.0
    for t in times[1:-2]:
        assert (time == t).any() and (time[~never] < t).any(), t
    backward.run_backward(o, mets, times, handovers=0)
    assert np.all(o.time[~never] == 90.0) and np.array_equal(o.time[never], time[never])
    backward.assert_untouched(o.state(), atm, never)


def test_module_sort_rebinds_the_time_steps_of_a_staggered_release():
    """A quirk of the reference the staggered device tests meet: a step computes its time steps per INDEX
    (module_timesteps), then module_sort moves the particles to other indices and leaves the time steps where they were
    (mptrac.c:7851-7880: dt belongs to the cache, module_sort permutes atm).  With one release time nobody notices; with
    staggered ones a particle takes its new index's step, so case `full` (SORT_DT 360) ends with particles at other
    times than T_STOP -- some beyond it -- and "particles outside the run never move" holds only without module_sort.
    The device has to reproduce exactly this (tests/test_gpu_backward.py: times equal the oracle's)."""
    ctl, clim, mets, atm = backward.backward_case("full", 3000, grid="tiny", staggered=True, t_stop=90.0)
    o = B.Oracle(ctl, clim, *backward.initial_mets(mets, 3600.0), atm)
    backward.start(o, atm["time"], t_start=3600.0)
    backward.run_backward(o, mets, cases.step_times(o.ctl), handovers=0)
    assert 2000 < (o.time == 90.0).sum() < 2990 and (o.time < 89.0).sum() > 100
    assert np.all(np.isfinite(o.lon)) and np.all(np.isfinite(o.p))
