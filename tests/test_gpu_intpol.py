"""mphip_intpol_met (Simulation.intpol_met) in the loaded library against the oracle's scalar orc_intpol_met_time_3d / _2d
on every case of tests/intpol_cases.py: compared as 64-bit patterns, NaNs in the same places, nothing left out (the points
of the not-finite rule are compared against NaN).  Then the chunking, the forms of the arguments, which pair of snapshots
the call sees, that it leaves a run's particles alone, and every refusal."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import cases
import intpol_cases as IC
import refpack as RP
from mptrac_amd import hip
from mptrac_amd.synth import FIELDS_2D, FIELDS_3D, synthetic_met

pytestmark = pytest.mark.gpu
SENTINEL = -12345.678


def context(m0=None, m1=None):
    """A context with nothing but the two snapshots: the call needs no control parameters and no particles."""
    sim = object.__new__(hip.Simulation)
    sim.L = hip.load()
    sim.h = C.c_void_p()
    assert sim.L.mphip_create(C.byref(sim.h), 0) == 0
    sim._mets, sim._next_met = [None, None], None
    if m0 is not None:
        sim.set_met(0, m0)
    if m1 is not None:
        sim.set_met(1, m1)
    return sim


def rows_of(sim, c, f3, f2):
    """every field of the case in one call; where there are more than the 32 a call takes (the axis grids: 13 + 24), the
    pressure-level fields in one call and the surface fields in another"""
    groups = (f3 + f2,) if len(f3 + f2) <= 32 else (f3, f2)
    assert len(groups) == 1 or not c["nan"].any()      # (a call without pressure-level fields does not look at p)
    return np.concatenate([sim.intpol_met_rows(c["time"], c["p"], c["lon"], c["lat"], f) for f in groups])


def check_case(c, wrong, sha):
    f3, f2 = IC.fields_of(c)
    sim = context(c["m0"], c["m1"])
    try:
        got = rows_of(sim, c, f3, f2)
    finally:
        sim.close()
    sha.update(got.tobytes())
    want = IC.expected(c, f3 + f2)
    if not IC.same_bits(got, want):
        wrong.append(c["name"] + ": " + IC.first_difference(got, want, f3 + f2))


def all_cases():
    return [IC.axis_edges(*g) for g in IC.AXIS_GRIDS] + IC.small_cases()


def census():
    """every case against the oracle: (what differs, SHA-256 of all returned bytes) -- tests/test_gpu_intpol_exact.py runs
    it in the other library"""
    wrong, sha = [], hashlib.sha256()
    for c in all_cases():
        check_case(c, wrong, sha)
    return wrong, sha.hexdigest()


@pytest.mark.parametrize("grid", IC.AXIS_GRIDS, ids=lambda g: "%g-%s-%s" % g)
def test_axis_edge_grids_are_the_oracles_bits(grid):
    c = IC.axis_edges(*grid)
    assert len(c["lon"]) == 4096 and len(IC.fields_of(c)[0]) == len(IC.F3) and len(IC.fields_of(c)[1]) == len(IC.F2)
    wrong = []
    check_case(c, wrong, hashlib.sha256())
    assert wrong == []


@pytest.mark.parametrize("c", IC.small_cases(), ids=lambda c: c["name"])
def test_small_cases_are_the_oracles_bits(c):
    wrong = []
    check_case(c, wrong, hashlib.sha256())
    assert wrong == []
    if c["nan"].any():
        sim = context(c["m0"], c["m1"])
        try:
            got = sim.intpol_met_rows(c["time"], c["p"], c["lon"], c["lat"], ("t", "ps"))
            # surface fields alone do not look at p: a point whose only fault is its pressure is answered
            surf = sim.intpol_met_rows(c["time"], c["p"], c["lon"], c["lat"], ("ps",))
        finally:
            sim.close()
        assert np.isnan(got[:, c["nan"]]).all() and np.isfinite(got[:, ~c["nan"]]).all()
        only_p = ~np.isfinite(c["p"])
        assert only_p.any() and np.isfinite(surf[0, only_p]).all() and np.isnan(surf[0, c["nan"] & ~only_p]).all()


@pytest.fixture(scope="module")
def ladder():
    c = IC.axis_edges(*IC.AXIS_GRIDS[0])
    sim = context(c["m0"], c["m1"])
    yield c, sim
    sim.close()


FIELDS = ("t", "ps", "u", "sst", "h2o", "plfc")


def test_chunks_give_the_bits_of_one_chunk(ladder):
    c, sim = ladder
    whole = sim.intpol_met_rows(c["time"], c["p"], c["lon"], c["lat"], FIELDS)
    assert IC.same_bits(whole, IC.expected(c, FIELDS))
    sim.set_option("intpol_chunk", 64)
    try:
        for n in (0, 1, 63, 64, 65, 193, 257):
            got = sim.intpol_met_rows(c["time"][:n], c["p"][:n], c["lon"][:n], c["lat"][:n], FIELDS)
            assert got.shape == (len(FIELDS), n) and IC.same_bits(got, whole[:, :n]), n
        for bad in (63, 2 ** 24 + 1):
            with pytest.raises(hip.MphipError, match="intpol_chunk"):
                sim.set_option("intpol_chunk", bad)
    finally:
        sim.set_option("intpol_chunk", 2 ** 22)


def test_argument_forms(ladder):
    c, sim = ladder
    n = 300
    p, lon, lat = (c[k][:n] for k in ("p", "lon", "lat"))
    array = sim.intpol_met(np.full(n, 1234.5), p, lon, lat, FIELDS)
    scalar = sim.intpol_met(1234.5, p, lon, lat, FIELDS)              # a scalar time is ntime = 1
    assert set(scalar) == set(FIELDS) and all(IC.same_bits(scalar[f], array[f]) for f in FIELDS)
    want = IC.oracle_rows(c["m0"], c["m1"], FIELDS, 1234.5, p, lon, lat)
    assert all(IC.same_bits(scalar[f], want[k]) for k, f in enumerate(FIELDS))
    other = sim.intpol_met(1234.5, p, lon, lat, FIELDS[::-1])          # another order
    assert all(IC.same_bits(other[f], scalar[f]) for f in FIELDS)
    twice = sim.intpol_met_rows(1234.5, p, lon, lat, ("t", "ps", "t"))   # one field twice
    assert IC.same_bits(twice[0], scalar["t"]) and IC.same_bits(twice[2], scalar["t"]) and IC.same_bits(twice[1], scalar["ps"])
    surface = sim.intpol_met(1234.5, None, lon, lat, ("ps", "sst"))      # surface fields only: no pressures
    assert IC.same_bits(surface["ps"], scalar["ps"]) and IC.same_bits(surface["sst"], scalar["sst"])


# ---- which pair the call sees ---------------------------------------------------------------------------------------
NAMES = ("t", "u", "h2o", "ps", "pbl")


def _snap(time, amp):
    return synthetic_met("tiny", time, amp, fields=NAMES)


def _points(n=257):
    atm = cases.make_case("advect", n=n, grid="tiny")[4]
    return np.linspace(-4000.0, 8000.0, n), atm["p"], atm["lon"], atm["lat"]


def _sees(sim, m0, m1):
    t, p, lon, lat = _points()
    got = sim.intpol_met_rows(t, p, lon, lat, NAMES)
    return IC.same_bits(got, IC.oracle_rows(m0, m1, NAMES, t, p, lon, lat))


def test_the_call_sees_the_resident_pair_as_the_next_step_would():
    m0, m1, m2, before = _snap(0.0, 1.0), _snap(3600.0, 1.25), _snap(7200.0, 0.8), _snap(-3600.0, 1.6)
    sim = context(m0, m1)
    try:
        assert _sees(sim, m0, m1) and not _sees(sim, m1, m2)
        sim.swap_met(m2)
        assert _sees(sim, m1, m2)
        sim.swap_met_backward(m0)            # back: (m0, m1)
        assert _sees(sim, m0, m1)
        sim.swap_met_backward(before)
        assert _sees(sim, before, m0)
    finally:
        sim.close()
    sim = context(m0, m1)
    try:
        sim.prefetch_met(m2)
        assert _sees(sim, m0, m1)            # a prefetch in flight is not visible ...
        sim.commit_met()
        assert _sees(sim, m1, m2)            # ... the committed pair is
    finally:
        sim.close()


def test_a_packed_upload_is_seen_as_decoded():
    m0, m1 = _snap(0.0, 1.0), _snap(3600.0, 1.25)
    coded = []
    for m in (m0, m1):
        dec, bare, packed = synthetic_met("tiny", m.time, 1.0, fields=NAMES), synthetic_met("tiny", m.time, 1.0, fields=NAMES), {}
        dec.f2, bare.f2 = dict(m.f2), dict(m.f2)
        for f in m.f3:
            q, scl, off = RP.encode(m.f3[f])
            dec.f3[f] = RP.decode(q, scl, off, *hip.PACK_LIMITS.get(f, hip.PACK_LIMITS_OPEN))
            del bare.f3[f]
            packed[f] = (q, scl, off)
        coded.append((dec, bare, packed))
    sim = context(_snap(0.0, 0.4), _snap(3600.0, 0.5))
    try:
        sim.update_met_packed(0, coded[0][1], coded[0][2])
        sim.update_met_packed(1, coded[1][1], coded[1][2])
        assert _sees(sim, coded[0][0], coded[1][0])
        assert not np.array_equal(coded[0][0].f3["t"], m0.f3["t"]) and not _sees(sim, m0, m1)
    finally:
        sim.close()


def test_calls_between_time_steps_leave_the_run_alone():
    """Five time steps of case `meteo`, with a call between every two: particles, uvwp, the random-number counter and the
    module_meteo quantities of the final download are those of a run without the calls."""
    ctl, clim, m0, m1, atm = cases.make_case("meteo", n=2000, grid="tiny")
    t, p, lon, lat = _points()
    runs = []
    for calls in (False, True):
        sim = hip.Simulation(ctl, clim, m0, m1, atm)
        try:
            sim.timesteps_init(0.0, 0.0)
            for k, ts in enumerate(cases.step_times(sim.ctl)[:5]):
                if calls and k:
                    got = sim.intpol_met_rows(t, p, lon, lat, ("t", "o3", "ps", "sst"))
                    assert IC.same_bits(got, IC.oracle_rows(m0, m1, ("t", "o3", "ps", "sst"), t, p, lon, lat))
                sim.run_timestep(ts)
            if calls:
                sim.intpol_met_rows(t, p, lon, lat, ("t",))       # (with module_meteo's launch of the last step pending)
            state = sim.state()
            state["rng_ctr"] = np.array([sim.get_cache()["rng_ctr"]], dtype=np.uint64).view(np.float64)
            runs.append(state)
        finally:
            sim.close()
    assert not np.array_equal(runs[0]["lon"], atm["lon"])
    meteo_rows = [cases.CASE_QUANTITIES["meteo"].index(k) for k in ("t", "o3", "ps", "sst")]
    assert all(np.isfinite(runs[0]["q"][iq]).any() and runs[0]["q"][iq].any() for iq in meteo_rows)
    for k in runs[0]:
        assert RP.same_bits(runs[0][k], runs[1][k]), k


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _raw(sim, n, time, ntime, p, lon, lat, fields, out, nfield=None):
    dp = hip._dp

    def ptr(a):
        return None if a is None else hip._ptr(a, dp)
    ids = None if fields is None else (C.c_int * max(len(fields), 1))(*fields)
    rc = sim.L.mphip_intpol_met(sim.h, n, ptr(time), ntime, ptr(p), ptr(lon), ptr(lat), len(fields or ()) if nfield is None else nfield,
                                ids, ptr(out))
    return rc, sim.L.mphip_last_error(sim.h).decode()


def test_every_refusal_writes_nothing_and_names_its_cause():
    m0, m1 = _snap(0.0, 1.0), _snap(3600.0, 1.25)
    n = 40
    t, p, lon, lat = (np.ascontiguousarray(a[:n]) for a in _points())
    T, PS = FIELDS_3D.index("t"), hip.INTPOL_2D | FIELDS_2D.index("ps")
    out = np.full((40, n), SENTINEL)

    def refused(sim, words, *args, **kw):
        rc, msg = _raw(sim, *args, **kw)
        assert rc != 0 and "mphip_intpol_met" in msg and all(w in msg for w in words), (words, rc, msg)
        assert (out == SENTINEL).all(), words

    sim = context()
    try:
        refused(sim, ("without a snapshot",), n, t, n, p, lon, lat, [T], out)
        sim.set_met(0, m0)
        refused(sim, ("without a snapshot",), n, t, n, p, lon, lat, [T], out)
        sim.set_met(1, _snap(0.0, 1.25))
        refused(sim, ("time0 == time1",), n, t, n, p, lon, lat, [T], out)
        sim.set_met(1, m1)
        refused(sim, ("n < 0",), -1, t, 1, p, lon, lat, [T], out)
        refused(sim, ("ntime",), n, t, 2, p, lon, lat, [T], out)
        refused(sim, ("ntime",), n, t, 0, p, lon, lat, [T], out)
        for k in range(5):          # a NULL lon, lat, out, time or field
            a = [t, p, lon, lat, [T], out]
            a[(2, 3, 5, 0, 4)[k]] = None
            refused(sim, ("NULL",), n, a[0], n, a[1], a[2], a[3], a[4], a[5], nfield=1)
        refused(sim, ("NULL p", "pressure-level"), n, t, n, None, lon, lat, [PS, T], out)
        refused(sim, ("nfield",), n, t, n, p, lon, lat, [T], out, nfield=0)
        refused(sim, ("nfield",), n, t, n, p, lon, lat, [T] * 33, out)
        for bad in (len(FIELDS_3D), -1, hip.INTPOL_2D | len(FIELDS_2D), 2 * hip.INTPOL_2D):
            refused(sim, ("out of range",), n, t, n, p, lon, lat, [T, bad], out)
        for name in ("pl", "ul", "vl", "wl", "zetal", "zeta_dotl"):
            refused(sim, ("model-level", name), n, t, n, p, lon, lat, [FIELDS_3D.index(name)], out)
        refused(sim, ("field o3 ", "not uploaded"), n, t, n, p, lon, lat, [T, FIELDS_3D.index("o3")], out)
        refused(sim, ("field sst ", "not uploaded"), n, t, n, p, lon, lat, [hip.INTPOL_2D | FIELDS_2D.index("sst")], out)
        only0 = synthetic_met("tiny", 0.0, 1.0, fields=NAMES + ("o3",))
        sim.set_met(0, only0)      # a field that ONE resident snapshot was uploaded without
        refused(sim, ("field o3 ", "not uploaded"), n, t, n, p, lon, lat, [FIELDS_3D.index("o3")], out)
        # ... and the accepted call next to them writes all of its rows and only those
        rc, msg = _raw(sim, n, t, n, p, lon, lat, [T, PS], out)
        assert rc == 0 and (out[:2] != SENTINEL).all() and (out[2:] == SENTINEL).all()
        assert IC.same_bits(out[:2], IC.oracle_rows(only0, m1, ("t", "ps"), t, p, lon, lat))
        out[:] = SENTINEL
        rc, msg = _raw(sim, 0, t, 1, p, lon, lat, [T], out)        # n == 0 succeeds and writes nothing
        assert rc == 0 and (out == SENTINEL).all()
    finally:
        sim.close()
    # axes that do not fit the kernel's 64 KB of LDS (16 bytes per node): 4000 + 60 + 40 nodes
    from mptrac_amd.synth import Met
    big = [Met(time, np.linspace(0.0, 359.9, 4000), np.linspace(-90.0, 90.0, 60), np.geomspace(1000.0, 1.0, 40),
               {"t": np.full((4000, 60, 40), 250.0, dtype=np.float32)}, {}) for time in (0.0, 3600.0)]
    sim = context(*big)
    try:
        refused(sim, ("4100 nodes", "LDS"), n, t, n, p, lon, lat, [T], out)
    finally:
        sim.close()


def test_the_profile_phase_counts_one_launch_per_chunk(ladder):
    """Between profile_begin and profile_end every kernel launch of the call is one event pair: n / chunk of them, rounded
    up, with a device time that is positive and below the call's wall time."""
    import time
    c, sim = ladder
    n = 257
    args = (c["time"][:n], c["p"][:n], c["lon"][:n], c["lat"][:n], FIELDS)
    sim.set_option("intpol_chunk", 64)
    try:
        sim.intpol_met_rows(*args)
        sim.profile_begin()
        t0 = time.perf_counter()
        sim.intpol_met_rows(*args)
        wall_ms = (time.perf_counter() - t0) * 1e3
        launches, ms = sim.profile_end()
        assert launches == 5 and 0.0 < ms < wall_ms, (launches, ms, wall_ms)
        sim.intpol_met_rows(*args)               # (outside begin / end nothing is recorded)
        sim.profile_begin()
        assert sim.profile_end()[0] == 0
    finally:
        sim.set_option("intpol_chunk", 2 ** 22)
