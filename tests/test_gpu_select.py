"""mphip_select_atm on the placed inputs of tests/select_cases.py against its definition in tests/refselect.py.

n, index and every row are compared with array_equal on bit patterns, NaNs in the same places: the contract is "what
mphip_get_atm has at those indices" and "what the host loop decides".  No tolerance anywhere.

Every particle set runs as uploaded, after one time step at the earliest particle time with locality_sort_interval 3
(the step moves nobody and stores the particles in the locality order: the kernels read them through a permutation and
write at external indices) and after the same step with the interval 0.  The not-finite particles are looked at as
uploaded only: a time step is not defined for a particle without a position.  Every call is made through the context's
page-locked rows (the default) and again with option select_direct 1.  Each comparison prints one "SELECT {json}"
line before it asserts.  tests/test_gpu_select_exact.py runs the functions of this file in the reference-rounding build."""
import json
import math

import numpy as np
import pytest

import cases
import refselect as RS
import select_cases as SC
from mptrac_amd import hip

pytestmark = pytest.mark.gpu


def report(**row):
    print("SELECT " + json.dumps(row))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def same_atm(a, b):
    return all(same_bits(a[k], b[k]) for k in ("time", "p", "lon", "lat", "q"))


def simulation(set_name, variant, shard=None):
    """the particles of a set on the device, bit for bit, stored as the variant asks"""
    atm = SC.particles(set_name)
    ctl, clim, m0, m1 = SC.setup(atm["q"].shape[0])
    s = hip.Simulation(ctl, clim, m0, m1, atm, shard=shard)
    s.set_option("locality_sort_interval", 3 if variant == "locality" else 0)
    finite = atm["time"][np.isfinite(atm["time"])]
    s.timesteps_init(float(finite.min()), float(finite.max()))
    if variant != "uploaded":
        s.run_timestep(float(finite.min()))      # dt = 0 for everybody
    return s


def check_call(s, have, set_name, variant, call, kw, rows=("time", "p", "lon", "lat", "q"), cap=None):
    """one select_atm call against the reference applied to `have`, the particles get_atm delivers"""
    want = RS.select(have, **kw) if set_name is None else SC.expected(set_name, call)
    got = s.select_atm(rows=rows, cap=cap, **kw)
    n = len(want)
    if cap is not None and cap < n:
        ok = got["n"] == n and got["index"] is None
        report(set=set_name, variant=variant, call=call, rows=list(rows), cap=cap, n=got["n"], reference=n, equal=ok)
        assert ok, "%s, %s, %s with cap %d: n = %d, reference %d" % (set_name, variant, call, cap, got["n"], n)
        return
    ref = RS.rows(have, want)
    wrong = []
    if got["n"] != n or not np.array_equal(got["index"], want):
        wrong.append("index")
    else:
        for k in ("time", "p", "lon", "lat"):
            if k in rows and not same_bits(got[k], ref[k]):
                wrong.append(k)
        for iq in range(have["q"].shape[0]):
            if ("q" in rows or "q%d" % iq in rows) and not same_bits(got["q"][iq], ref["q"][iq]):
                wrong.append("q%d" % iq)
    report(set=set_name, variant=variant, call=call, rows=list(rows), cap=cap, n=got["n"], reference=n, equal=not wrong)
    assert not wrong, "%s, %s, %s: n = %d, reference %d; differing: %s" % (set_name, variant, call, got["n"], n, wrong)


def every_call(set_name, variant):
    s = simulation(set_name, variant)
    have = s.get_atm()
    placed = SC.particles(set_name)
    assert same_atm(have, placed), (set_name, variant)       # the placed bits are what the kernels see
    for call, kw in SC.calls_of(set_name).items():
        check_call(s, have, set_name, variant, call, kw)
    s.set_option("select_direct", 1)         # ... and copied straight into the caller's arrays
    for call, kw in SC.calls_of(set_name).items():
        check_call(s, have, set_name, variant + "/direct", call, kw)
    s.set_option("select_direct", 0)
    if set_name in SC.SUBSET_CALLS:
        call = SC.SUBSET_CALLS[set_name]
        kw = SC.calls_of(set_name)[call]
        n = len(SC.expected(set_name, call))
        assert n >= 2
        for rows in SC.ROW_SUBSETS:
            if rows == ("q1",) and have["q"].shape[0] < 2:
                continue
            for cap in (n, n - 1, 0):
                check_call(s, have, set_name, variant, call, kw, rows=rows, cap=cap)
    after = s.get_atm()
    ok = same_atm(after, have)
    report(set=set_name, variant=variant, call="get_atm afterwards", equal=ok)
    assert ok, "%s, %s: the particles changed under the calls" % (set_name, variant)
    s.close()


def steps_with_calls_in_between():
    """20 steps of a case with module_sort (the external order is redefined under the calls) and the locality order in
    force, a select_atm between all steps: the bits of the run without"""
    ctl, clim, m0, m1, atm = cases.make_case("full", n=3001)
    runs = []
    for calls in (False, True):
        s = hip.Simulation(ctl, clim, m0, m1, atm)
        s.set_option("locality_sort_interval", 3)
        s.timesteps_init(0.0, 0.0)
        times = cases.step_times(s.ctl)[:20]
        for k, t in enumerate(times):
            s.run_timestep(t)
            if calls:
                got = s.select_atm(stride=1 + k % 5, time=(t - 90.0, t + 90.0), z=(2.0, 20.0), near=(10.0, 20.0, 6000.0))
                if k in (3, 11):        # (a comparison costs a download: twice)
                    have = s.get_atm()
                    check_call(s, have, None, "stepping", "step %d" % k,
                               dict(stride=1 + k % 5, time=(t - 90.0, t + 90.0), z=(2.0, 20.0), near=(10.0, 20.0, 6000.0)))
                    assert got["n"] > 0
        runs.append(s.state())
        runs[-1]["ctr"] = s.get_cache()["rng_ctr"]
        s.close()
    ok = all(np.array_equal(runs[0][k].view(np.uint8), runs[1][k].view(np.uint8)) for k in ("time", "p", "lon", "lat", "q", "uvwp"))
    ok = ok and runs[0]["ctr"] == runs[1]["ctr"]
    report(test="stepping", steps=len(times), equal=ok)
    assert len(times) == 20 and ok, "a run with select_atm between the steps differs from the run without"


REFUSALS = (
    (dict(stride=0), "mphip_select_atm: stride must be >= 1"),
    (dict(stride=-3), "mphip_select_atm: stride must be >= 1"),
    (dict(first=-1), "mphip_select_atm: first must be >= 0"),
    (dict(cap=-1), "mphip_select_atm: cap must be >= 0"),
    (dict(time=(math.nan, 1.0)), "mphip_select_atm: bad time range"),
    (dict(time=(2.0, 1.0)), "mphip_select_atm: bad time range"),
    (dict(z=(1.0, math.nan)), "mphip_select_atm: bad height range"),
    (dict(z=(3.0, 1.0)), "mphip_select_atm: bad height range"),
    (dict(lon=(math.nan, math.nan)), "mphip_select_atm: bad longitude range"),
    (dict(lon=(10.0, -10.0)), "mphip_select_atm: bad longitude range"),
    (dict(lat=(0.0, math.nan)), "mphip_select_atm: bad latitude range"),
    (dict(lat=(10.0, -10.0)), "mphip_select_atm: bad latitude range"),
    (dict(near=(0.0, 0.0, -1.0)), "mphip_select_atm: near_r must be finite and >= 0"),
    (dict(near=(0.0, 0.0, math.inf)), "mphip_select_atm: near_r must be finite and >= 0"),
    (dict(near=(0.0, 0.0, math.nan)), "mphip_select_atm: near_r must be finite and >= 0"),
)


def refusals():
    import ctypes as C
    s = simulation("n65q3", "uploaded")
    have = s.get_atm()
    for kw, message in REFUSALS:
        with pytest.raises(hip.MphipError) as err:
            s.select_atm(**kw)
        ok = message in str(err.value)
        report(test="refusal", arguments=repr(kw), message=str(err.value), equal=ok)
        assert ok, (kw, str(err.value))
    # NULL sel / nsel, and nothing written: the count keeps the value it had
    n = C.c_longlong(-77)
    sel = hip.MphipSelect(first=0, last=-1, stride=0)
    assert s.L.mphip_select_atm(s.h, C.byref(sel), 4, C.byref(n), None, None, None, None, None, None) != 0 and n.value == -77
    sel.stride = 1
    for args in ((None, 4, C.byref(n)), (C.byref(sel), 4, None)):
        assert s.L.mphip_select_atm(s.h, *args, None, None, None, None, None, None) != 0
        assert "mphip_select_atm: null argument" in s.L.mphip_last_error(s.h).decode() and n.value == -77
    assert s.L.mphip_select_atm(None, C.byref(sel), 4, C.byref(n), None, None, None, None, None, None) != 0 and n.value == -77
    assert same_atm(s.get_atm(), have)
    # a Cartesian grid: the time window and the height range work, the three horizontal tests are refused
    s.close()
    ctl, clim, m0, m1 = SC.setup()
    s = hip.Simulation(dict(ctl, met_coord_type=1), clim, m0, m1, SC.particles("n65q3"))
    for kw in (dict(lon=(0.0, 1.0)), dict(lat=(0.0, 1.0)), dict(near=(0.0, 0.0, 1.0))):
        with pytest.raises(hip.MphipError) as err:
            s.select_atm(**kw)
        assert "mphip_select_atm: lon, lat and near need a lat/lon grid" in str(err.value), str(err.value)
    check_call(s, have, None, "cartesian", "time and z", dict(stride=2, time=(SC.T0, SC.T1), z=SC.ZR))
    s.close()
    # control parameters not uploaded
    h = C.c_void_p()
    assert s.L.mphip_create(C.byref(h), 0) == 0
    assert s.L.mphip_select_atm(h, C.byref(sel), 4, C.byref(n), None, None, None, None, None, None) != 0 and n.value == -77
    message = s.L.mphip_last_error(h).decode()
    s.L.mphip_destroy(h)
    report(test="refusal", arguments="no control parameters", message=message, equal="not uploaded" in message)
    assert "mphip_select_atm: control parameters were not uploaded" in message


def one_rank_of_two():
    """a context that holds the second half of the index range (ip0 > 0): the indices are rank-local"""
    name = "n16385q3"
    n = len(SC.particles(name)["time"])
    lo = n // 2 + 1
    for variant in ("uploaded", "locality"):
        s = simulation(name, variant, shard=(lo, n))
        have = s.get_atm()
        assert len(have["time"]) == n - lo and same_bits(have["time"], SC.particles(name)["time"][lo:])
        for call, kw in (("stride7/window", dict(stride=7, time=(SC.T0, SC.T1))), ("marked", dict(lat=(80.0, 81.0))),
                         ("first/last", dict(stride=3, first=5, last=4000))):
            check_call(s, have, None, variant + ", rank 1 of 2", call, kw)
        marked = s.select_atm(lat=(80.0, 81.0), rows=("index",))["index"].tolist()
        assert marked == [e - lo for e in SC.marked(n) if e >= lo] == [16383 - lo, n - 1 - lo], marked
        s.close()


# ---------------------------------------------------------------------------

@pytest.mark.parametrize("set_name,variant", [(s, v) for s in SC.set_names() for v in SC.variants_of(s)])
def test_selection_rows_and_order(set_name, variant):
    every_call(set_name, variant)


def test_steps_with_calls_in_between_keep_their_bits():
    steps_with_calls_in_between()


def test_refusals():
    refusals()


def test_one_rank_of_two_returns_rank_local_indices():
    one_rank_of_two()
