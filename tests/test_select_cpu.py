"""What the inputs of tests/select_cases.py reach, asserted on the reference (tests/refselect.py) alone, and the
reference itself against the host loop it restates: refselect with a stride and the time step's window selects the rows
write_atm_asc writes (through the atm_conv tool, which needs no device)."""
import math
import os
import subprocess

import numpy as np
import pytest

import refanalysis as RA
import refselect as RS
import select_cases as SC
from hostfiles import write_atm_bin


def selected(set_name, call):
    return set(SC.expected(set_name, call).tolist())


def test_every_count_and_stride_is_there():
    names = SC.set_names()
    assert [n for n in SC.NPS] == [1, 63, 64, 65, 16383, 16384, 16385, 40000]
    for n in SC.NPS:
        assert "n%dq3" % n in names and len(SC.particles("n%dq3" % n)["time"]) == n
        strides = {int(c.split("/")[1]) for c in SC.count_calls(n) if c.startswith("stride/")}
        assert strides == {s for s in (1, 2, 7, 64, n - 1, n, n + 1) if s >= 1}
    for n in SC.NQ0:
        assert SC.particles("n%dq0" % n)["q"].shape == (0, n)
    # three chunks of 2^14 marks over np + 1 entries at 40 000; the chunk is exactly full at 16 383
    assert (40000 + 1 + 16383) // 16384 == 3 and (16383 + 1) % 16384 == 0 and (16384 + 1 + 16383) // 16384 == 2


@pytest.mark.parametrize("n", SC.NPS)
def test_count_sets_reach_what_their_names_claim(n):
    s = "n%dq3" % n
    every = list(range(n))
    assert SC.expected(s, "everything").tolist() == every and SC.expected(s, "stride/1").tolist() == every
    assert len(SC.expected(s, "empty")) == 0 and len(SC.expected(s, "range7/first_above_last")) == 0
    assert len(SC.expected(s, "range7/first_beyond")) == 0
    assert SC.expected(s, "one/last").tolist() == [n - 1]
    assert SC.expected(s, "marked").tolist() == SC.marked(n)
    if n > 16384:
        assert {16383, 16384, n - 1} <= selected(s, "marked")       # either side of the chunk border, and the last one
        assert selected(s, "marked/stride") == {0, 16383}
    assert SC.expected(s, "stride/%d" % (n + 1)).tolist() == [0] and SC.expected(s, "stride/%d" % n).tolist() == [0]
    if n > 2:
        assert SC.expected(s, "stride/%d" % (n - 1)).tolist() == [0, n - 1]
    assert SC.expected(s, "range7/last_on_0").tolist() == [0]
    on, below, above = (SC.expected(s, "range7/last_%s_candidate" % k).tolist() for k in ("on", "below", "above"))
    if n > 15:
        assert on == [0, 7, 14] and below == [0, 7] and above == on
        assert SC.expected(s, "range7/first_beside_candidate").tolist()[:2] == [6, 13]
        assert SC.expected(s, "range7/first_is_last").tolist() == [14]
    same = SC.expected(s, "stride/7").tolist()
    for name in ("last_beyond", "last_is_np", "last_is_np_minus_1", "first_on_0"):
        assert SC.expected(s, "range7/" + name).tolist() == same, name
    window = SC.expected(s, "window")
    if n >= 64:
        assert 0 < len(window) < n          # the window keeps most and drops some
    assert SC.expected(s, "stride7/window").tolist() == [e for e in same if e in set(window.tolist())]


def test_one_ulp_neighbours_of_every_bound_decide_differently():
    atm, tags = SC.edges()
    where = {t: i for i, t in enumerate(tags)}
    # the lower bound rejects what lies below it, the upper one what lies above; the bound itself is inside
    for k in ("time", "lon", "lat", "z"):
        got = selected("edges", k)
        for b, (inside, outside) in enumerate((("above", "below"), ("below", "above"))):
            assert where["%s/%d/on" % (k, b)] in got and where["%s/%d/%s" % (k, b, inside)] in got, (k, b)
            assert where["%s/%d/%s" % (k, b, outside)] not in got, (k, b)
        lo, hi = (selected("edges", "%s/point_%s" % (k, e)) for e in ("lo", "hi"))
        assert where[k + "/0/on"] in lo and where[k + "/0/above"] not in lo and where[k + "/0/below"] not in lo
        assert where[k + "/1/on"] in hi and where[k + "/1/above"] not in hi and where[k + "/1/below"] not in hi
        assert selected("edges", k + "/unbounded") == set(range(len(atm["time"])))
    for k in ("time", "lon", "lat"):
        for b, bound in enumerate(SC.EVERY_RANGE[k]):
            v = {s: float(atm[k][where["%s/%d/%s" % (k, b, s)]]) for s in ("below", "on", "above")}
            assert v["on"] == bound and math.nextafter(v["below"], math.inf) == bound == math.nextafter(v["above"], -math.inf)
    for b, bound in enumerate(SC.ZR):
        z = {s: RA.Z(float(atm["p"][where["z/%d/%s" % (b, s)]])) for s in ("below", "on", "above")}
        assert z["below"] < z["on"] == bound < z["above"]
    # the distance: adjacent doubles, the decision differs
    near = selected("edges", "near")
    pairs = 0
    for t, i in where.items():
        part = t.split("/")
        if part[0] == "near" and part[-1] == "lo":
            j = where["/".join(part[:-1] + ["hi"])]
            k = "lat" if atm["lon"][i] == atm["lon"][j] else "lon"
            assert math.nextafter(float(atm[k][i]), math.inf) == float(atm[k][j])
            assert (i in near) != (j in near), t
            pairs += 1
    assert pairs == 5 and where["near/centre"] in near
    r, i = SC.equal_radius()
    assert i in selected("edges", "near/r_eq/on") and i in selected("edges", "near/r_eq/above")
    assert i not in selected("edges", "near/r_eq/below")
    assert selected("edges", "near/zero") == {where["near/centre"]}
    # the criteria are ANDed
    every = set.intersection(*(selected("edges", k) for k in ("time", "lon", "lat", "z")))
    assert selected("edges", "all") == every and selected("edges", "all/near") == every & near
    assert selected("edges", "all/stride3") == {e for e in every if e % 3 == 0}
    assert 0 < len(every & near) < len(every) < len(atm["time"])


def test_not_finite_particles_pass_or_fail_as_the_definition_says():
    atm, tags = SC.not_finite()
    where = {t: i for i, t in enumerate(tags)}
    good = {i for t, i in where.items() if t.startswith("good/")}
    for k in ("time", "z", "lon", "lat", "near", "all", "all/near"):
        assert good <= selected("not_finite", k)
    # a NaN passes the test it meets; an infinity fails the range of its own coordinate
    for field, call in (("time", "time"), ("lon", "lon"), ("lat", "lat"), ("p", "z")):
        got = selected("not_finite", call)
        assert where[field + "/nan"] in got
        assert where[field + "/inf"] not in got and where[field + "/-inf"] not in got, field
    # Z(+-inf) = H0 log(+-0) = -inf: below every range; the cosine of an infinite angle is NaN: the distance test passes
    near = selected("not_finite", "near")
    for t in ("lon/nan", "lat/nan", "lon/inf", "lon/-inf", "lat/inf", "lat/-inf", "p/nan", "time/nan", "time/inf"):
        assert where[t] in near, t
    both = selected("not_finite", "all/near")
    assert all(where[f + "/nan"] in both for f in ("time", "lon", "lat", "p"))
    assert selected("not_finite", "none") == set(range(len(atm["time"])))


# ---------------------------------------------------------------------------
# the reference against write_atm_asc
# ---------------------------------------------------------------------------

def _particles_around_zero():
    """times around t = 0 with DT_MOD 180: the window's ends, their neighbours, NaN, and times well inside and outside"""
    rng = np.random.default_rng(7)
    n = 1000
    time = rng.choice(np.arange(-200.0, 200.25, 0.25), n)
    edge = [-90.0, 90.0, math.nextafter(-90.0, -math.inf), math.nextafter(-90.0, 0.0), math.nextafter(90.0, math.inf),
            math.nextafter(90.0, 0.0), math.nan, 0.0]
    for k, v in enumerate(edge):
        time[7 * (3 + 5 * k)] = v       # on candidates of stride 7
        time[7 * (3 + 5 * k) + 1] = v   # ... and beside them
    return {"time": time, "p": RA.P0 * np.exp(-rng.uniform(1.0, 20.0, n) / RA.H0), "lon": rng.uniform(-180.0, 180.0, n),
            "lat": rng.uniform(-80.0, 80.0, n), "q": rng.uniform(1.0, 2.0, (1, n))}


@pytest.mark.parametrize("atm_filter", [0, 1, 2])
def test_refselect_reproduces_the_row_set_of_write_atm_asc(tmp_path, atm_filter):
    from mptrac_amd import build
    build.build_host()
    atm = _particles_around_zero()
    write_atm_bin(tmp_path / "in.bin", atm)
    out = tmp_path / "out.tab"
    res = subprocess.run([build.ATM_CONV_BIN, "-", str(tmp_path / "in.bin"), "1", str(out), "0", "NQ", "1", "QNT_NAME[0]", "m",
                          "DT_MOD", "180", "ATM_STRIDE", "7", "ATM_FILTER", str(atm_filter)], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [ln.split() for ln in open(out) if ln.strip() and not ln.startswith("#")]
    # filter 2: the stride and the window; filters 0 and 1: the stride alone (1 blanks by the time of the row)
    index = RS.select(atm, stride=7, time=(0.0 - 0.5 * 180.0, 0.0 + 0.5 * 180.0) if atm_filter == 2 else None)
    every = RS.select(atm, stride=7)
    assert len(every) == (1000 + 6) // 7 and (len(index) < len(every)) == (atm_filter == 2)
    assert len(lines) == len(index)
    want = ["%.2f" % v for v in atm["time"][index]]
    assert [ln[0] for ln in lines] == want
    inside = set(RS.select(atm, stride=7, time=(-90.0, 90.0)).tolist())
    blank = [ln[4] in ("nan", "-nan") for ln in lines]
    assert blank == [atm_filter == 1 and e not in inside for e in index.tolist()]
    if atm_filter == 2:
        assert any(math.isnan(v) for v in atm["time"][index])     # a NaN time passes the window, as in the host loop
    assert os.path.getsize(out) > 0
