"""mphip_update_met_packed and mphip_prefetch_met_packed against mphip_update_met and mphip_prefetch_met: a snapshot whose
level fields go to the device as 16-bit codes and are decoded there steps exactly as the same snapshot uploaded as the
decoded floats -- positions, quantities and cache->uvwp agree in every bit.

Cases of tests/cases.py on the `tiny` grid (36 x 19 x 20 and the periodic column), 20 steps: `advect` (the winds only) and
`full` (turbulent and mesoscale diffusion, convection, wet and dry deposition: the cloud-water fields are consumed).  The
meteorology is first replaced by refpack.decode(refpack.encode(.)) within the reader's limits; run (a) uploads those floats,
run (b) the codes -- into a context that was created with OTHER snapshots, so that a packed upload that wrote nothing would
show."""
import copy

import numpy as np
import pytest

import cases
import refpack as R
from mptrac_amd import hip
from mptrac_amd.synth import synthetic_met

pytestmark = pytest.mark.gpu
N = 2000
STEPS = 20


def limits(name):
    return hip.PACK_LIMITS.get(name, hip.PACK_LIMITS_OPEN)


def coded(met, names=None):
    """(the snapshot with the level fields `names` replaced by their decoded codes, the snapshot without them, their codes)."""
    names = tuple(met.f3) if names is None else names
    dec, bare = copy.copy(met), copy.copy(met)
    dec.f3, bare.f3, packed = dict(met.f3), dict(met.f3), {}
    for f in names:
        q, scl, off = R.encode(met.f3[f])
        dec.f3[f] = R.decode(q, scl, off, *limits(f))
        del bare.f3[f]
        packed[f] = (q, scl, off)
    return dec, bare, packed


def other(met, t):
    return synthetic_met("tiny", t, 0.37, fields=tuple(met.f3) + tuple(met.f2))


def same_state(a, b):
    sa, sb = a.state(), b.state()
    for k in ("time", "p", "lon", "lat", "q", "uvwp"):
        assert R.same_bits(sa[k], sb[k]), k
    return sa


def run_pair(case, names_of):
    ctl, clim, m0, m1, atm = cases.make_case(case, n=N, grid="tiny")
    (d0, b0, p0), (d1, b1, p1) = (coded(m, names_of(m)) for m in (m0, m1))
    a = hip.Simulation(ctl, clim, d0, d1, atm)
    b = hip.Simulation(ctl, clim, other(m0, 0.0), other(m1, 3600.0), atm)
    try:
        b.update_met_packed(0, b0, p0)
        b.update_met_packed(1, b1, p1)
        for s in (a, b):
            s.timesteps_init(0.0, 0.0)
        times = cases.step_times(a.ctl)[:STEPS]
        assert len(times) == STEPS
        for t in times:
            a.run_timestep(t)
            b.run_timestep(t)
        state = same_state(a, b)
        assert not np.array_equal(state["lon"], atm["lon"])         # (they moved)
        return state
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("case", ["advect", "full"])
def test_codes_step_like_their_decoded_floats(case):
    state = run_pair(case, lambda m: None)
    if case == "full":
        ctl = cases.make_case(case, n=1, grid="tiny")[0]
        assert (state["q"][ctl["qnt_mloss_wet"]] > 0).any()         # (wet deposition acted: the cloud water was read)


@pytest.mark.parametrize("case", ["advect", "full"])
def test_half_of_the_fields_packed_and_half_float(case):
    run_pair(case, lambda m: tuple(sorted(m.f3))[::2])


def test_the_decoded_snapshot_is_not_the_original():
    """(the comparison above is not one of a snapshot with itself: the codes lose bits)"""
    m0 = cases.make_case("advect", n=1, grid="tiny")[2]
    dec = coded(m0)[0]
    assert not np.array_equal(dec.f3["u"], m0.f3["u"])


@pytest.mark.parametrize("case", ["advect", "full"])
def test_packed_prefetch_and_commit_equal_the_synchronous_swap(case):
    """prefetch_met_packed + commit_met against swap_met + update_met over 3 h with 4 snapshots (the shape of
    test_met_prefetch_and_commit_equal_the_synchronous_swap): the prefetch is issued right after each hand-over."""
    ctl, clim, m0, m1, atm = cases.make_case(case, n=N, grid="tiny")
    ctl["t_stop"] = 10800.0
    fields = tuple(m0.f3) + tuple(m0.f2)
    m2 = synthetic_met("tiny", 7200.0, 0.8, fields=fields)
    m3 = synthetic_met("tiny", 10800.0, 1.1, fields=fields)
    c = [coded(m) for m in (m0, m1, m2, m3)]
    a = hip.Simulation(ctl, clim, c[0][0], c[1][0], atm)
    b = hip.Simulation(ctl, clim, other(m0, 0.0), other(m1, 3600.0), atm)
    try:
        b.update_met_packed(0, c[0][1], c[0][2])
        b.update_met_packed(1, c[1][1], c[1][2])
        for s in (a, b):
            s.timesteps_init(0.0, 0.0)
        b.prefetch_met_packed(c[2][1], c[2][2])
        with pytest.raises(hip.MphipError):
            b.prefetch_met_packed(c[3][1], c[3][2])            # one snapshot at a time
        upcoming = [(3600.0, 2, 3), (7200.0, 3, None)]
        for t in cases.step_times(a.ctl):
            if upcoming and t > upcoming[0][0]:
                _, new1, after = upcoming.pop(0)
                a.swap_met(c[new1][0])
                b.commit_met()
                if after is not None:
                    b.prefetch_met_packed(c[after][1], c[after][2])
            a.run_timestep(t)
            b.run_timestep(t)
        assert not upcoming
        same_state(a, b)
    finally:
        a.close()
        b.close()


def test_grid_dimensions_must_match_and_bad_descriptions_are_refused():
    ctl, clim, m0, m1, atm = cases.make_case("advect", n=10, grid="tiny")
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    try:
        fields = tuple(m0.f3) + tuple(m0.f2)
        small = synthetic_met((18, 10, 20), 3600.0, 1.0, fields=fields)
        _, bare, packed = coded(small)
        with pytest.raises(hip.MphipError, match="Meteo grid dimensions do not match!"):
            s.update_met_packed(1, bare, packed)
        with pytest.raises(hip.MphipError, match="Meteo grid dimensions do not match!"):
            s.prefetch_met_packed(bare, packed)
        dec, bare, packed = coded(m1)
        with pytest.raises(hip.MphipError, match="mphip_update_met_packed: field u is given both as floats and as codes"):
            s.update_met_packed(1, dec, packed)
        q, scl, off = packed["u"]
        with pytest.raises(hip.MphipError, match="mphip_update_met_packed: field u is given as codes without scl or off"):
            s.update_met_packed(1, bare, dict(packed, u=(q, None, off)))
        with pytest.raises(hip.MphipError, match="mphip_prefetch_met_packed: field u: the limits need lo <= hi"):
            s.prefetch_met_packed(bare, dict(packed, u=(q, scl, off, 2.0, 1.0)))
        # nothing was written: the context still steps as one that never saw these calls
        ref = hip.Simulation(ctl, clim, m0, m1, atm)
        try:
            for x in (s, ref):
                x.timesteps_init(0.0, 0.0)
                x.run_timestep(0.0)
                x.run_timestep(180.0)
            same_state(s, ref)
        finally:
            ref.close()
    finally:
        s.close()
