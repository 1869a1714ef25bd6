"""Backward runs (DIRECTION -1) on the device against the CPU oracle, through the C ABI: every named case, the backward
hand-over of mptrac_get_met (mphip_swap_met + mphip_update_met on slot 0 of a running context: the axes, the packed
two-snapshot grids, a deferred module_meteo), release times spread over the run with a short last step, negative model
times in every scheduler, mphip_run_timesteps with a negative stride, and the "not observable" options of the forward
suite.  The oracle's own backward arithmetic is held by tests/test_backward_cpu.py.

Bars: tests/test_gpu_parity.py's _compare with its TOL (1e-10, every quantity row on its own scale, times equal,
cache->uvwp and the random-number counter equal); two runs of the same build: equal bits.  The functions that take a
`tol` run again in the reference-rounding build with tol = 0 (tests/test_gpu_backward_exact.py)."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import backward
import cases
import refmodules
import test_gpu_parity as P
from mptrac_amd import hip
from mptrac_amd.synth import Met
from oracle import binding as B

pytestmark = pytest.mark.gpu


def _engines(ctl, clim, mets, atm, t_start=None):
    first = backward.initial_mets(mets, mets[-1].time)
    assert first[1] is mets[-1]
    o = B.Oracle(ctl, clim, *first, atm)
    backward.start(o, atm["time"], t_start)
    s = hip.Simulation(ctl, clim, *first, atm)
    backward.start(s, atm["time"], t_start)
    assert s.ctl.direction == o.ctl.direction == -1
    assert s.ctl.t_start == o.ctl.t_start == mets[-1].time and s.ctl.t_stop == o.ctl.t_stop
    return o, s


def _worst(o, s):
    """largest error of the positions and of the quantity rows (the figures DESIGN.md section 2 quotes)"""
    g, r = s.state(), o.state()
    pos = max(cases.rel_err(g[k], r[k]) for k in ("lon", "lat", "p"))
    q = cases.q_rows_err(o.ctl, g["q"], r["q"])[0] if r["q"].size else 0.0
    return pos, q


def _report(test, name, o, s):
    pos, q = _worst(o, s)
    g, r = s.state(), o.state()
    same = (g["q"] == r["q"]) | (np.isnan(g["q"]) & np.isnan(r["q"]))
    print("BACKWARD " + json.dumps(dict(test=test, case=name, pos=pos, q=q, time=bool(np.array_equal(g["time"], r["time"])),
                                        uvwp=bool(np.array_equal(g["uvwp"], r["uvwp"])),
                                        **{k: int(np.count_nonzero(g[k] != r[k])) for k in ("lon", "lat", "p")},
                                        q_bits=int(np.count_nonzero(~same)))))


class _Frozen:
    """the oracle as it was at one moment, for _compare"""

    def __init__(self, o):
        self._state, self.ctl, self.cache = o.state(), o.ctl, SimpleNamespace(rng_ctr=o.cache.rng_ctr)

    def state(self):
        return self._state


# ---------------------------------------------------------------------------
# a. every named case
# ---------------------------------------------------------------------------

def named_case(case, tol=P.TOL, n=5003):
    ctl, clim, mets, atm = backward.backward_case(case, n)
    o, s = _engines(ctl, clim, mets, atm)
    times = cases.step_times(o.ctl)
    assert len(times) == 21 and times[0] == 3600.0 and times[-1] == 0.0
    backward.run_backward(o, mets, times, handovers=0)
    backward.run_backward(s, mets, times, handovers=0)
    _report("named", case, o, s)
    P._compare(o, s, tol)
    assert np.all(o.time == 0.0)
    s.close()


@pytest.mark.parametrize("case", list(cases.CASES))
def test_every_named_case_20_steps_backward(case):
    """tests/test_gpu_parity.py::test_run_timestep_20_steps reversed: 3600 s -> 0 on the same two snapshots."""
    named_case(case)


# ---------------------------------------------------------------------------
# b. the backward hand-over
# ---------------------------------------------------------------------------

def handover(case, hours, tol=P.TOL, n=3000, t_end=0.0, **over):
    """`hours` hours backward over hours + 1 snapshots: hours - 1 times mphip_swap_met + mphip_update_met(slot 0).  The
    device is compared with the oracle right behind every hand-over as well -- before the next step, so a module_meteo
    scheduled by the step before it (the device evaluates it lazily) must have sampled the snapshots that step saw."""
    ctl, clim, mets, atm = backward.backward_case(case, n, grid="tiny", hours=hours, t_end=t_end, **over)
    o, s = _engines(ctl, clim, mets, atm)
    times = cases.step_times(o.ctl)
    assert len(times) == 20 * hours + 1 and times[-1] == t_end
    behind = []
    backward.run_backward(o, mets, times, handovers=hours - 1, after_handover=lambda: behind.append(_Frozen(o)))
    backward.run_backward(s, mets, times, handovers=hours - 1, after_handover=lambda: P._compare(behind.pop(0), s, tol))
    assert not behind
    _report("handover", case, o, s)
    P._compare(o, s, tol)
    assert np.all(o.time == t_end) and s._mets[0] is mets[0] and s._mets[1] is mets[1]
    s.close()
    return o


@pytest.mark.parametrize("case", ["diff", "full", "zeta_full", "mlp_full", "bound_pbl_zeta", "meteo", "meteo_gated"])
def test_backward_handover_two_hours(case):
    o = handover(case, 2)
    if case.startswith("meteo"):
        # the step at 3600 s, the last one before the hand-over, schedules module_meteo (MET_DT_OUT 0.1 / 1800 s)
        assert 3600.0 % max(o.ctl.met_dt_out, 180.0) == 0


def test_two_backward_handovers_three_hours():
    handover("conv_sedi", 3)


# ---------------------------------------------------------------------------
# c. the axes follow the new met0
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("sort_dt", [720.0, 180.0])
def test_axes_follow_the_new_met0_across_a_backward_handover(sort_dt):
    """The reference sorts and interpolates on the axes of the current met0 (mptrac.c:3010-3020, 5913-5919).  Forward
    those are the old met1's after a hand-over; backward they must be the axes of the snapshot mphip_update_met has
    just put into slot 0.  Three snapshots whose latitude / pressure axes differ by a few 1e-4 (the shifts of
    test_axes_follow_met0_across_a_handover): behind the hand-over module_sort's keys and order are the oracle's, bit
    for bit -- and differ from the keys on the axes of the met0 before it --, and the end state is the oracle's.
    SORT_DT 180: module_sort in every step, so the step before the hand-over has prepared the next sort ahead of time on
    the old met0's axes (option sort_ahead); the hand-over must drop it.  (12000 particles there: of 3000 sorted
    that often, none happens to sit between the two latitude axes at the hand-over -- 9 of 12000 do.)"""
    ctl, clim, mets, atm = backward.backward_case("conv_sedi", 3000 if sort_dt == 720.0 else 12000, hours=2, sort_dt=sort_dt)

    def shifted(m, dlat, fp):
        return Met(m.time, m.lon, m.lat + dlat, m.p * fp, m.f3, m.f2)
    mets = [shifted(mets[0], -3e-4, 1.0 - 2e-7), shifted(mets[1], 4e-4, 1.0 + 3e-7), mets[2]]
    o, s = _engines(ctl, clim, mets, atm)
    times = cases.step_times(o.ctl)
    sorts = []

    def sort_oracle():
        r = o.state()
        old, new = (refmodules.Ref(o.ctl, clim, m, m).sort_keys(r["lon"], r["lat"], r["p"]) for m in (mets[1], mets[0]))
        keys, perm = o.sort()
        assert np.array_equal(keys, new) and np.count_nonzero(old != new) > 0       # (the check can see stale axes)
        sorts.append((keys, perm, np.count_nonzero(old != new)))

    def sort_device():
        keys_o, perm_o, _ = sorts[0]
        keys_s, perm_s = s.sort()
        assert np.array_equal(np.sort(keys_o), keys_s)
        assert np.array_equal(perm_o, perm_s)
    backward.run_backward(o, mets, times, handovers=1, after_handover=sort_oracle)
    backward.run_backward(s, mets, times, handovers=1, after_handover=sort_device)
    print("BACKWARD " + json.dumps(dict(test="axes", sort_dt=sort_dt, keys_that_differ_between_the_axes=int(sorts[0][2]))))
    _report("axes", "conv_sedi", o, s)
    P._compare(o, s)
    s.close()


# ---------------------------------------------------------------------------
# d. staggered release, ragged ends
# ---------------------------------------------------------------------------

def staggered(case, tol=P.TOL, n=5003, **over):
    """Release times spread over the run (backward.staggered_times: on step times, 37 s off the raster, at the start),
    six particles outside [T_STOP, t_start] or at T_STOP that never move, T_STOP = 90 s (a last step of 90 s).  With
    module_sort in the run (`full`: SORT_DT 360) the reference hands a sorted particle the time step of its new index
    (tests/test_backward_cpu.py::test_module_sort_rebinds_the_time_steps_of_a_staggered_release): there the device must
    end at the oracle's times, whatever they are, and "never move" is asserted for the runs without it."""
    ctl, clim, mets, atm = backward.backward_case(case, n, staggered=True, t_stop=90.0, **over)
    never = backward.never_released(atm["time"], 3600.0, 90.0)
    assert never.sum() == 6 and (atm["time"] > 3600.0).sum() == 2 and (atm["time"] < 90.0).sum() == 3
    o, s = _engines(ctl, clim, mets, atm, t_start=3600.0)
    times = cases.step_times(o.ctl)
    assert times[-2:] == [180.0, 90.0] and sum((atm["time"] == t).any() for t in times) >= 19
    backward.run_backward(o, mets, times, handovers=0)
    backward.run_backward(s, mets, times, handovers=0)
    _report("staggered", case, o, s)
    P._compare(o, s, tol)                         # (times: equal)
    g = s.state()
    if o.ctl.sort_dt <= 0:
        assert np.all(g["time"][~never] == 90.0)
        for k in ("time", "lon", "lat", "p", "q"):
            assert np.array_equal(g[k][..., never], atm[k][..., never]), k
        backward.assert_untouched(g, atm, never)
    else:
        assert 0 < (g["time"] != 90.0).sum() - 5 < n // 2
    s.close()


@pytest.mark.parametrize("case,over", [("conv_sedi", {}), ("full", {}), ("full", dict(sort_dt=0.0))],
                         ids=["conv_sedi", "full", "full-unsorted"])
def test_staggered_release_and_ragged_ends(case, over):
    staggered(case, **over)


# ---------------------------------------------------------------------------
# e. negative model times
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case,over", [("full", dict(sort_dt=720.0, mixing_dt=720.0)), ("meteo", dict(met_dt_out=540.0)),
                                       ("conv_sedi", dict(conv_dt=720.0))], ids=["full-sort_mixing_720", "meteo-540", "conv_sedi-conv_720"])
def test_negative_model_times(case, over):
    """0 -> -7200 s across a hand-over at -3600 s: module_sort, module_mixing, module_meteo and convection gated by fmod
    of a negative time (C's fmod keeps the sign of the time: -720 % 720 == -0, -540 % 720 == -540)."""
    o = handover(case, 2, t_end=-7200.0, **over)
    assert np.all(o.time == -7200.0)


# ---------------------------------------------------------------------------
# f. mphip_run_timesteps with a negative stride
# ---------------------------------------------------------------------------

_BATCH_BACKWARD = [("advect", None), ("conv_sedi", None), ("full", None), ("zeta_full", None), ("mlp_full", None), ("advect", 2),
                   ("diff", 1), ("meteo", "every_third"), ("meteo", "eager_third"), ("full", "sparse"), ("conv_sedi", "conv_sparse"),
                   ("conv_sedi", "bound"), ("pbl_meso", None), ("isosurf_rho", None)]


@pytest.mark.parametrize("case,variant", _BATCH_BACKWARD,
                         ids=[c if v is None else f"{c}-{v if isinstance(v, str) else 'advect%d' % v}" for c, v in _BATCH_BACKWARD])
def test_run_timesteps_equals_the_step_by_step_loop_backward(case, variant):
    """The body of test_run_timesteps_equals_the_step_by_step_loop with DIRECTION -1: the same five engines, equal
    bits, the same launch counts (seven quiet steps: one launch), the oracle afterwards."""
    assert (case, variant) in P._BATCH_CASES
    P.run_timesteps_equals_the_step_by_step_loop(case, variant, direction=-1)


def test_run_timesteps_around_a_backward_handover():
    """Two hours backward, the steps of each interval as ONE mphip_run_timesteps call, the hand-over between the two
    calls (a driver must cut a batch where mptrac_get_met would act: the step at 3600 s still belongs to the first
    interval): the bits of the step-by-step loop, and the oracle's numbers."""
    ctl, clim, mets, atm = backward.backward_case("conv_sedi", 3000, grid="tiny", hours=2)
    o, loop = _engines(ctl, clim, mets, atm)
    times = cases.step_times(o.ctl)
    backward.run_backward(o, mets, times, handovers=1)
    backward.run_backward(loop, mets, times, handovers=1)
    first = [t for t in times if t >= 3600.0]
    assert len(first) == 21 and len(times) == 41
    s = hip.Simulation(ctl, clim, mets[1], mets[2], atm)
    backward.start(s, atm["time"])
    s.set_option("multi_step", 64)
    s.run_timesteps(times[0], len(first))
    assert times[len(first)] < s._mets[0].time
    s.swap_met_backward(mets[0])
    s.run_timesteps(times[len(first)], len(times) - len(first))
    a, b = s.state(), loop.state()
    for k in ("time", "lon", "lat", "p", "q", "uvwp"):
        assert np.array_equal(a[k], b[k]), k
    assert s.get_cache()["rng_ctr"] == loop.get_cache()["rng_ctr"]
    P._compare(o, s)
    s.close()
    loop.close()


# ---------------------------------------------------------------------------
# g. not observable, backward
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("sort_dt", [180.0, 360.0])
def test_sort_ahead_of_time_is_not_observable_backward(sort_dt):
    P.sort_ahead_of_time_is_not_observable(sort_dt, direction=-1)


def test_keys_and_deposition_flags_from_the_step_kernel_are_not_observable_backward():
    P.keys_and_deposition_flags_from_the_step_kernel_are_not_observable(direction=-1)


def test_deposition_launch_with_packed_waves_equals_the_fused_tail_backward():
    P.deposition_launch_with_packed_waves_equals_the_fused_tail(direction=-1)


@pytest.mark.parametrize("case", ["conv_sedi", "full"])
def test_locality_order_is_not_observable_backward(case):
    P.locality_order_is_not_observable(case, direction=-1)


@pytest.mark.parametrize("tile", [1024, 96])
def test_lds_tile_trajectories_equal_the_launches_without_a_tile_backward(tile):
    P.lds_tile_trajectories_equal_the_launches_without_a_tile(4, tile, direction=-1)


@pytest.mark.parametrize("over", [dict(diffusion=0, conv_cape=-999.0, conv_mix_pbl=0, qnt_rp=-1, qnt_rhop=-1), dict(),
                                  dict(tdec_trop=259200.0, tdec_strat=259200.0, dry_depo_vdep=0.15, wet_depo_ic_a=1e-4,
                                       wet_depo_ic_b=0.8, wet_depo_bc_a=5e-5, wet_depo_bc_b=0.6)],
                         ids=["advect", "c3_set", "c3_set_decay_deposition"])
def test_lean_instantiations_equal_the_general_code_backward(over):
    P.lean_instantiations_equal_the_general_code(over, 4, direction=-1)
