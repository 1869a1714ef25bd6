"""The sample and station outputs on the device (mphip_sample_obs, mphip_station_hits) on the edge inputs of
tests/analysis_cases.py -- particles at adjacent doubles either side of every comparison of the two loops, exact
equalities, the sliver in which the latitude band alone decides, lists of exactly 0, 1, 63, 64, 65, 128 and 129 records,
up to 1025 observations per call (more than one LDS tile, two passes of the index sort), hits either side of the scan's
chunk border, not-finite particles, flags that truncate to 0 -- against their transcription in tests/refanalysis.py.
What the inputs reach is asserted on the reference in tests/test_analysis_edges_cpu.py.

Counts, masses, hit lists, rows and flags are compared with array_equal, NaNs in the same places: the contract of the two
calls is the host loop's bits.  No tolerance anywhere.

Every case runs on the particles as uploaded, after one time step at the earliest particle time with
locality_sort_interval 3 (nobody has a time step yet: the step only stores the particles in the locality order, the
kernels read them through a permutation and write at external indices) and after the same step with the interval 0.  The
not-finite particles are looked at as uploaded only: a time step is not defined for a particle without a position.  Each
comparison prints one "ANA_EDGE {json}" line before it asserts, and a failure names the case, the call and the
observation.  tests/test_gpu_analysis_edges_exact.py runs the functions of this file in the reference-rounding build."""
import functools
import json

import numpy as np
import pytest

import analysis_cases as AC
import refanalysis as RA
from mptrac_amd import hip

pytestmark = pytest.mark.gpu

T, DT = AC.T, AC.DT_MOD


def report(**row):
    print("ANA_EDGE " + json.dumps(row))


def same(a, b):
    return bool(np.array_equal(a, b, equal_nan=True))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _setup():
    return AC.setup()


def simulation(case, variant):
    """the particles of a case on the device, bit for bit, stored as the variant asks"""
    atm = AC.particles(case)
    ctl, clim, m0, m1 = _setup()
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.set_option("locality_sort_interval", 3 if variant == "locality" else 0)
    finite = atm["time"][np.isfinite(atm["time"])]
    s.timesteps_init(float(finite.min()), float(finite.max()))
    if variant != "uploaded":
        s.run_timestep(float(finite.min()))      # dt = 0 for everybody
    g = s.get_atm()
    for k in ("time", "lon", "lat", "p", "q"):
        assert np.array_equal(bits(g[k]), bits(atm[k])), (case, variant, k)       # the placed bits are what the kernels see
    return s


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------

def check_sample(s, case, variant, name):
    args, tags = AC.sample_arguments(case, name)
    count, mass, _, _ = AC.sample_reference(case, name)
    gcount, gmass = s.sample_obs(*args)
    bad = np.nonzero((gcount != count) | ~((gmass == mass) | (np.isnan(gmass) & np.isnan(mass))))[0]
    report(test="sample", case=case, variant=variant, call=name, nobs=len(count), records=int(count.sum()),
           nan=int(np.isnan(mass).sum()), differing=len(bad))
    if len(bad):
        i = int(bad[0])
        raise AssertionError("case %s, %s, sample call %s: %d of %d observations differ, the first is %d (%s): count %d, "
                             "reference %d; mass %r, reference %r; placed particles that decide there: %s"
                             % (case, variant, name, len(bad), len(count), i, tags[i], gcount[i], count[i], float(gmass[i]),
                                float(mass[i]), AC.deciders(case, name, i)))
    assert same(gcount, count) and same(gmass, mass)


def _tags(case):
    return AC.main()[1] if case == "main" else (AC.not_finite()[1] if case == "not_finite" else [])


def check_station(s, case, variant, name, want, lon, lat, r, s0, s1, qnt_stat, cap):
    """one call with a buffer that is large enough against (listed, rows) of the reference"""
    listed, rows = want
    nhit, idx, got = s.station_hits(T, lon, lat, r, s0, s1, qnt_stat, cap=cap)
    ok = nhit == len(listed) and idx is not None and same(idx, listed) and same(got, rows)
    report(test="station", case=case, variant=variant, call=name, listed=len(listed), nhit=nhit, equal=ok)
    if not ok:
        tags = _tags(case)
        a, b = set(listed.tolist()), set(idx.tolist() if idx is not None else [])
        named = [tags[i] if i < len(tags) else i for i in sorted(a ^ b)[:8]]
        raise AssertionError("case %s, %s, station call %s: %d listed, reference %d; particles in one list only: %s%s"
                             % (case, variant, name, nhit, len(listed), named,
                                "" if a ^ b or idx is None else "; the lists agree, the rows differ"))


def unchanged(s, case, variant, name, q):
    ok = bool(np.array_equal(bits(s.get_atm()["q"]), bits(q)))
    report(test="restored", case=case, variant=variant, call=name, equal=ok)
    assert ok, "case %s, %s, %s: the quantities changed although nothing was listed" % (case, variant, name)


# ---------------------------------------------------------------------------
# the main case
# ---------------------------------------------------------------------------

def sample_decisions(variant):
    s = simulation("main", variant)
    for name in AC.sample_calls():
        if not name.startswith("nobs/"):
            check_sample(s, "main", variant, name)
    s.close()


def observation_tiles(variant):
    s = simulation("main", variant)
    for nobs in AC.NOBS:
        check_sample(s, "main", variant, "nobs/%d" % nobs)
    check_sample(s, "main", variant, "main")         # ... and a short call after the long ones
    s.close()


def station_decisions(variant):
    s = simulation("main", variant)
    q = AC.particles("main")["q"]
    for name, (site, lon, lat, r, s0, s1) in AC.station_calls().items():
        listed, rows, _, _ = AC.station_reference("main", lon, lat, r, s0, s1, -1)
        check_station(s, "main", variant, name, (listed, rows), lon, lat, r, s0, s1, -1, max(len(listed), 4))
    unchanged(s, "main", variant, "without a flag quantity", q)
    s.close()


def flag_sequence(s, case, variant, lon, lat):
    """too small a buffer (cap 0 and nhit - 1): the number alone, every quantity keeps its bits; cap = nhit and nhit + 1 on
    the uploaded flags: the list, the rows and the flags afterwards; the next call lists nobody; without a flag quantity
    everybody in reach is listed whatever the flag"""
    atm = AC.particles(case)
    listed, rows, q_after, skipped = AC.station_reference(case, lon, lat, AC.DX, *AC.EVER, AC.QSTAT)
    nhit = len(listed)
    assert nhit >= 2
    for cap in (0, nhit - 1):
        n, idx, got = s.station_hits(T, lon, lat, AC.DX, *AC.EVER, AC.QSTAT, cap=cap)
        report(test="cap", case=case, variant=variant, cap=cap, nhit=n, reference=nhit)
        assert n == nhit and idx is None, ("case %s, %s, flags: cap %d gives %d hits, reference %d (the flag values the reference "
                                           "lists: %s)" % (case, variant, cap, n, nhit, sorted(set(atm["q"][AC.QSTAT][listed].tolist()))))
        unchanged(s, case, variant, "flags, cap %d of %d" % (cap, nhit), atm["q"])
    for cap in (nhit, nhit + 1):
        s.update_quantity(AC.QSTAT, atm["q"][AC.QSTAT])
        check_station(s, case, variant, "flags, cap %d of %d" % (cap, nhit), (listed, rows), lon, lat, AC.DX, *AC.EVER, AC.QSTAT, cap)
        after = s.get_atm()
        ok = bool(np.array_equal(bits(after["q"]), bits(q_after)))
        report(test="flags_set", case=case, variant=variant, cap=cap, equal=ok, skipped=skipped)
        assert ok, "case %s, %s, flags after the call with cap %d differ from the reference's" % (case, variant, cap)
        n, idx, got = s.station_hits(T, lon, lat, AC.DX, *AC.EVER, AC.QSTAT, cap=cap)
        report(test="listed_once", case=case, variant=variant, cap=cap, nhit=n)
        assert n == 0, "case %s, %s, flags: %d particles are listed a second time" % (case, variant, n)
    every, every_rows, _, _ = RA.station_hits(dict(atm, q=q_after), T, DT, lon, lat, AC.DX, *AC.EVER, -1, AC.xyz_of(case))
    assert len(every) >= nhit + skipped
    check_station(s, case, variant, "flags, qnt_stat -1", (every, every_rows), lon, lat, AC.DX, *AC.EVER, -1, len(every))


def station_flags(variant):
    s = simulation("main", variant)
    flag_sequence(s, "main", variant, *AC.SITES["flags"])
    s.close()


def box_sums_with_the_weighting_functions():
    """mphip_box_sums once, on the placed particles: kernel_weight_exact with every weighting function of the cases (the
    faces of the boxes have their own suite, tests/test_gpu_box_edges.py)"""
    s = simulation("main", "uploaded")
    atm = AC.particles("main")
    for name, kernel in AC.kernels().items():
        want = RA.box_sums(atm, AC.BOX, T, DT, AC.QM, 1, -1, kernel)
        got = s.box_sums(AC.BOX, T, AC.QM, 1, -1, kernel)
        ok = same(got, want)
        report(test="box_sums", kernel=name, equal=ok, nan=int(np.isnan(want).sum()), cells=int(np.count_nonzero(want)))
        assert ok, "box sums with the weighting function %s differ in %d cells" % (name, np.count_nonzero(~((got == want) | (np.isnan(got) & np.isnan(want)))))
    s.close()


# ---------------------------------------------------------------------------
# particle counts, chunk borders, not-finite particles
# ---------------------------------------------------------------------------

def particle_counts(n, variant):
    case = str(n)
    s = simulation(case, variant)
    for name in ("layer", "plain"):
        check_sample(s, case, variant, name)
    _, lon, lat, _ = AC.COUNT_OBS[0]
    atm = AC.particles(case)
    listed, rows, q_after, _ = AC.station_reference(case, lon, lat, AC.DX, *AC.EVER, AC.QSTAT)
    n_, idx, got = s.station_hits(T, lon, lat, AC.DX, *AC.EVER, AC.QSTAT, cap=len(listed) - 1)
    assert n_ == len(listed) and idx is None, "case %s, %s: %d hits with too small a buffer, reference %d" % (case, variant, n_, len(listed))
    unchanged(s, case, variant, "cap %d of %d" % (len(listed) - 1, len(listed)), atm["q"])
    check_station(s, case, variant, "station", (listed, rows), lon, lat, AC.DX, *AC.EVER, AC.QSTAT, len(listed))
    assert np.array_equal(bits(s.get_atm()["q"]), bits(q_after)), "case %s, %s: flags after the station call" % (case, variant)
    assert s.station_hits(T, lon, lat, AC.DX, *AC.EVER, AC.QSTAT, cap=4)[0] == 0
    s.close()


def not_finite():
    s = simulation("not_finite", "uploaded")
    for name in ("layer", "plain"):
        check_sample(s, "not_finite", "uploaded", name)
    _, lon, lat, _ = AC.COUNT_OBS[0]
    listed, rows, _, _ = AC.station_reference("not_finite", lon, lat, AC.DX, *AC.EVER, -1)
    check_station(s, "not_finite", "uploaded", "station, qnt_stat -1", (listed, rows), lon, lat, AC.DX, *AC.EVER, -1, len(listed))
    flag_sequence(s, "not_finite", "uploaded", lon, lat)
    s.close()


# ---------------------------------------------------------------------------

@pytest.mark.parametrize("variant", AC.VARIANTS)
def test_sample_decisions(variant):
    sample_decisions(variant)


@pytest.mark.parametrize("variant", AC.VARIANTS)
def test_observation_tiles(variant):
    observation_tiles(variant)


@pytest.mark.parametrize("variant", AC.VARIANTS)
def test_station_decisions(variant):
    station_decisions(variant)


@pytest.mark.parametrize("variant", AC.VARIANTS)
def test_station_flags_and_buffer_sizes(variant):
    station_flags(variant)


@pytest.mark.parametrize("variant", AC.VARIANTS)
@pytest.mark.parametrize("n", AC.COUNTS)
def test_particle_counts_and_chunk_borders(n, variant):
    particle_counts(n, variant)


def test_not_finite_particles():
    not_finite()


def test_box_sums_with_the_weighting_functions():
    box_sums_with_the_weighting_functions()
