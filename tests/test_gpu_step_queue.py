"""The step kernel's chunk queues (option step_queue; chunk_claim in csrc/mphip_kernels.hpp): the launch is a grid that
is resident at once, and its waves claim chunks of 64 particles from one queue per XCD -- and from the other XCDs' queues
once their own is used up -- instead of walking a fixed share of the particles.  Which wave takes which particle is not
observable: every case runs with the queues and with step_queue 0, the static partition, and compares the bits of time,
lon, lat, p, EVERY quantity row, cache->uvwp and cache->dt.

step_queue 1 (the default) takes the queues from 16 chunks per wave of the grid on -- more particles than a test here
may use -- so every case sets step_queue 2, the queues in every launch.  With step_blocks and step_blocks_multi at 8
the grid is 8 workgroups = 32 waves: every wave claims many chunks and steals.

All on the `tiny` grid, at most 20 000 particles.  locality_sort_interval is 3, so that a folded re-sort (the launch
reads its particles through the sort's permutation) falls inside the runs of mphip_run_timesteps.

Break checks, each tried once on a scratch copy of the kernel (profiles/r10_step_queue_ab.txt lists the failing tests):
the last chunk of a queue not handed out; a stolen chunk counted from the base of the thief's own queue.
"""
import numpy as np
import pytest

import backward
import cases
from mptrac_amd import hip

pytestmark = pytest.mark.gpu

DT = cases.BASE["dt_mod"]
STATE = ("time", "lon", "lat", "p", "q", "uvwp", "dt")
EIGHT = dict(step_blocks=8, step_blocks_multi=8)


def _inputs(case, n, direction=1):
    """(ctl, clim, met0, met1, atm) on the tiny grid; every particle with its own rp, rhop and m where the case has them
    (a value that arrives in another particle's slot moves p or shows in m)"""
    if direction == 1:
        ctl, clim, m0, m1, atm = cases.make_case(case, n=n, grid="tiny")
    else:
        ctl, clim, mets, atm = backward.backward_case(case, n, grid="tiny")
        m0, m1 = backward.initial_mets(mets, mets[-1].time)
    rng = np.random.default_rng(20241021)
    for name, lo, hi in (("rp", 1.0, 20.0), ("rhop", 500.0, 2000.0)):
        if ctl.get("qnt_" + name, -1) >= 0:
            atm["q"][ctl["qnt_" + name]] = rng.uniform(lo, hi, n)
    if ctl.get("qnt_m", -1) >= 0:
        atm["q"][ctl["qnt_m"]] = rng.permutation(n) + 1.0
    return ctl, clim, m0, m1, atm


def _run(inputs, queue, steps, multi, direction=1, **options):
    """The first `steps` time steps (at t_start, t_start +- DT, ...) with step_queue = queue: one mphip_run_timestep
    each, or (multi) the first one alone and the rest in one mphip_run_timesteps call.  Returns the state with
    cache->dt."""
    ctl, clim, m0, m1, atm = inputs
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    try:
        cases.prepare(s)
        s.set_option("locality_sort_interval", 3)
        s.set_option("step_queue", queue)
        for name, value in options.items():
            s.set_option(name, value)
        if direction == 1:
            s.timesteps_init(0.0, 0.0)
        else:
            s.timesteps_init(float(atm["time"].min()), float(atm["time"].max()))
        assert s.ctl.direction == direction
        times = cases.step_times(s.ctl)[:steps]
        assert len(times) == steps
        if multi:
            s.run_timestep(times[0])
            s.run_timesteps(times[1], steps - 1)
        else:
            for t in times:
                s.run_timestep(t)
        g = s.state()
        g["dt"] = s.get_cache()["dt"]
    finally:
        s.close()
    return g


def _same(a, b, what):
    for k in STATE:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, int(np.count_nonzero(a[k] != b[k])))


def _queue_equals_static(inputs, queue, steps, what, atm_moved=True, **kw):
    static = _run(inputs, 0, steps, False, **kw)
    for multi in (False, True):
        _same(_run(inputs, queue, steps, multi, **kw), static, (what, "multi" if multi else "single"))
    if atm_moved:
        assert not np.array_equal(static["lon"], inputs[4]["lon"])
    return static


# 1, 63, 64, 65: a part of a chunk, a whole one, one particle in the second; 255, 256, 257: the same at a workgroup's
# four waves; 513 = 64 * 8 + 1: nine chunks in queues of two -- the queues of XCDs 5, 6 and 7 are empty, XCD 4's holds
# the one-particle chunk; 1000: 16 chunks for the 32 waves of the smallest grid; 2113 = 64 * 33 + 1
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 1000, 2113])
def test_particle_counts_at_the_chunk_edges(n):
    static = _queue_equals_static(_inputs("conv_sedi", n), 2, 5, n)
    assert np.all(static["time"] == 4 * DT)      # (the steps at 0, DT, ... 4 DT)


@pytest.mark.parametrize("xcd_map", [0, 1])
def test_eight_workgroups_claim_and_steal(xcd_map):
    # 313 chunks for 32 waves (one queue without xcd_map, eight queues of 40 with it): every wave claims about ten
    # chunks, and the waves of an XCD that finishes early take the others' chunks
    static = _queue_equals_static(_inputs("conv_sedi", 20000), 2, 5, xcd_map, xcd_map=xcd_map, **EIGHT)
    assert np.all(static["time"] == 4 * DT)      # (the steps at 0, DT, ... 4 DT)


# the headline module set; two Runge-Kutta stages; a gated subset (advection and convection); the general kernel
# (single steps only: mphip_run_timesteps falls back to them); the boundary-layer closure's instantiation; winds from
# the model levels
MATRIX = [("conv_sedi", {}), ("advect_midpoint", {}), ("conv_thresh", {}), ("conv_sedi", dict(generic_kernel=1)),
          ("pbl_meso", {}), ("zeta_full", {})]


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("case,options", MATRIX, ids=[c + ("_generic" if o else "") for c, o in MATRIX])
def test_every_kind_of_instantiation_forward_and_backward(case, options, direction):
    # 3000 particles = 47 chunks for 32 waves; ten steps, in the mphip_run_timesteps run with folded re-sorts
    # (tests/test_gpu_fold_resort.py), one launch per step in the other
    inputs = _inputs(case, 3000, direction)
    _queue_equals_static(inputs, 2, 10, (case, direction), direction=direction, **EIGHT, **options)


def test_a_step_that_reads_the_stored_dt():
    # "full" sorts every second step: the key kernel of module_sort computes dt and the step launch reads it from the
    # array, so a particle that two waves process moves twice (where module_timesteps runs in the launch, the second
    # pass finds time = t, dt = 0, and leaves the particle alone)
    inputs = _inputs("full", 3000)
    assert inputs[0]["sort_dt"] == 2 * DT
    static = _run(inputs, 0, 6, False, **EIGHT)
    _same(_run(inputs, 2, 6, False, **EIGHT), static, "full")
    _same(_run(inputs, 1, 6, False, **EIGHT), static, "full, default")      # (below the default's threshold: static)
    assert np.all(static["time"] == 5 * DT)
