"""Backward runs (DIRECTION -1): the named cases of tests/cases.py reversed in time, release times that are staggered
over the run, and the driver loop with mptrac_get_met's backward hand-over -- for the oracle and the device alike
(tests/test_backward_cpu.py, tests/test_gpu_backward*.py)."""
import numpy as np

import cases
from mptrac_amd.synth import synthetic_met

# wind amplitudes of the snapshots at t_end + 3600 k: the forward tests' factors (cases.make_case, the hand-over tests
# of tests/test_gpu_parity.py)
SCALES = (1.0, 1.25, 0.8, 1.1)
_MAKE_CASE_KEYS = ("seed", "quantities", "lon0", "fields")


def staggered_times(n, t_start, t_stop, dt_mod):
    """Release times of a backward run from t_start (on the DT_MOD raster) down to t_stop: a third of the particles at
    t_start, a third on later step times of the raster (a particle whose time EQUALS the time of a call is not
    released by that call: `direction * (time - t) < 0`), a third 37 s off the raster -- all inside (t_stop, t_start] --
    and six that never move: two beyond t_start, three before t_stop, one exactly at t_stop."""
    i = np.arange(n)
    nsteps = int(np.floor((t_start - t_stop) / dt_mod))
    assert nsteps >= 3 and n >= 30
    raster = t_start - dt_mod * ((i * 7) % nsteps)
    time = np.where(i % 3 == 0, t_start, np.where(i % 3 == 1, raster, raster - dt_mod + 37.0)).astype(np.float64)
    time[1], time[2] = t_start + 500.0, t_start + dt_mod
    time[4], time[5], time[8] = t_stop - 100.0, t_stop - dt_mod, np.nextafter(t_stop, -np.inf)
    time[7] = t_stop
    return time


def never_released(time, t_start, t_stop):
    """Particles a backward run from t_start to t_stop leaves alone (module_timesteps, mptrac.c:6016-6041: released
    when t_stop <= time <= t_start and the call's time lies below the particle's -- which no call at or above t_stop
    does for a particle at t_stop)."""
    return (time > t_start) | (time <= t_stop)


def assert_untouched(state, atm, which):
    """Every particle of `which` (a mask over the input) is in `state` with the bits it started with -- time, position
    and quantities --, and no other particle kept its longitude."""
    q0 = np.asarray(atm["q"])
    for i in np.flatnonzero(which):
        same = (state["time"] == atm["time"][i]) & (state["lon"] == atm["lon"][i]) & (state["lat"] == atm["lat"][i]) \
            & (state["p"] == atm["p"][i]) & np.all(state["q"] == q0[:, i][:, None], axis=0)
        assert same.any(), i
    assert np.isin(state["lon"], atm["lon"]).sum() == which.sum()


def assert_staggered(time, t_start, t_stop, dt_mod, steps):
    """What the tests of the work done one step early (the next call's module_timesteps inside the sort that runs
    ahead and inside the step kernel's key output) need of their input: at each of the first `steps` calls behind the
    first, a particle whose time equals the time of the NEXT call (`<` against `<=` decides whether it moves), particles
    that call releases, and particles that go on waiting."""
    never = never_released(time, t_start, t_stop)
    assert never.sum() == 6
    for k in range(1, steps - 1):
        t, t_next = t_start - dt_mod * k, t_start - dt_mod * (k + 1)
        assert (time == t_next).any() and ((time < t) & (time > t_next)).any() and (time[~never] < t_next).any(), t


def backward_case(name, n, grid="C1", hours=1, t_end=0.0, staggered=False, **over):
    """cases.make_case(name) run backward: DIRECTION -1 from t_end + 3600 hours down to T_STOP = t_end, snapshots at
    t_end + 3600 k (k = 0 .. hours), the particle times mirrored (the late release of the isosurf cases stays a late
    release), the case's other extras as they are.  `over`: control settings on top (t_stop included), or seed /
    quantities / lon0 / fields of cases.make_case.  staggered: staggered_times() between the run's start and its T_STOP.
    Returns (ctl, clim, mets, atm); an engine starts on (mets[hours - 1], mets[hours]): initial_mets()."""
    make_kw = {k: over.pop(k) for k in _MAKE_CASE_KEYS if k in over}
    ctl, clim, m0, _, atm = cases.make_case(name, n=n, grid=grid, **make_kw)
    assert 1 <= hours < len(SCALES)
    fields = tuple(m0.f3) + tuple(m0.f2)
    mets = [synthetic_met(grid, t_end + 3600.0 * k, SCALES[k], fields=fields, lon0=make_kw.get("lon0", -180.0))
            for k in range(hours + 1)]
    t_begin = t_end + 3600.0 * hours
    atm["time"] = t_begin - atm["time"]
    ctl.update(direction=-1, t_stop=t_end)
    ctl.update(over)
    if staggered:
        atm["time"] = staggered_times(n, t_begin, ctl["t_stop"], ctl["dt_mod"])
    return ctl, clim, mets, atm


def initial_mets(mets, t_start):
    """(met0, met1) at the start of a backward run: mptrac_get_met loads the file at or before t_start - 1 and the one
    at or after t_start (the start time belongs to the interval the run moves into)."""
    k = max(i for i, m in enumerate(mets) if m.time <= t_start - 1)
    return mets[k], mets[k + 1]


def start(engine, atm_time, t_start=None):
    """module_timesteps_init on either engine; t_start given (on the raster): a start time below the latest particle
    time, as a caller of the C ABI may set it (particles beyond it are never released)."""
    if hasattr(engine, "update_ctl"):      # the device
        engine.timesteps_init(float(np.min(atm_time)), float(np.max(atm_time)) if t_start is None else t_start)
    else:
        engine.timesteps_init()
        if t_start is not None:
            engine.ctl.t_start = t_start
    if t_start is not None:
        assert engine.ctl.t_start == t_start
    cases.prepare(engine)


def run_backward(engine, mets, times, handovers, each=None, after_handover=None):
    """The driver loop (trac.c:204-226 with mptrac_get_met's branch `t < met0->time`): before a step whose
    time lies below the engine's met0 the snapshots are handed over -- the old met0 becomes met1, the next earlier
    file the new met0.  `handovers`: how many the run must make.  each(t): called behind every step; after_handover():
    behind every hand-over, before the step that needed it."""
    index = {id(m): k for k, m in enumerate(mets)}
    seen = 0
    for t in times:
        while t < engine._mets[0].time:
            engine.swap_met_backward(mets[index[id(engine._mets[0])] - 1])
            seen += 1
            if after_handover is not None:
                after_handover()
        assert engine._mets[0].time <= t <= engine._mets[1].time
        engine.run_timestep(t)
        if each is not None:
            each(t)
    assert seen == handovers, (seen, handovers)


def run_forward(engine, mets, times, handovers):
    """The same loop forward (the hand-over of the existing tests: swap_met with the next later file)."""
    index = {id(m): k for k, m in enumerate(mets)}
    seen = 0
    for t in times:
        while t > engine._mets[1].time:
            engine.swap_met(mets[index[id(engine._mets[1])] + 1])
            seen += 1
        engine.run_timestep(t)
    assert seen == handovers, (seen, handovers)
