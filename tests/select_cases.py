"""Placed inputs of mphip_select_atm (select_mark_kernel, the scan of the analysis outputs, select_list_kernel,
select_row_kernel in mptrac_amd/csrc/mphip_kernels.hpp; the definition: tests/refselect.py).

  counts      np = 1, 63, 64, 65 (the wave width), 16 383, 16 384, 16 385 (the scan's chunk of 2^14 marks over np + 1
              entries) and 40 000 (three chunks); nq 3, and nq 0 at 65 and 16 385
  strides     1, 2, 7, 64, np - 1, np, np + 1
  first/last  on 0, on a candidate, one beside a candidate, last >= np, first > last
  selections  empty, everything, exactly one; hits at external indices 16 383 and 16 384 (either side of the chunk border),
              at 0 and at np - 1: the particles placed at a latitude nobody else has
  ranges      per range (time, z, lon, lat) particles on both bounds and one double beside them on both sides; for z the
              pressures are found by searching the adjacent doubles of p on the reference (box_cases.heights)
  distance    per direction the two adjacent doubles of lat / lon between which dist2 > r^2 changes (bisection on the
              reference), and a radius with r * r == dist2 of a placed particle, with its two neighbours
  not finite  NaN, +inf and -inf in time, p, lon and lat, one at a time (they pass or fail as the definition says)
  rows, cap   only `index`; only q[1]; everything; cap equal to n, n - 1 and 0

A case is (particle set, call name); what it must select is computed once per process on the reference (expected) and
shared by the GPU tests.  What the inputs reach is asserted on the reference in tests/test_select_cpu.py."""
import functools
import math

import numpy as np

import analysis_cases as AC
import refanalysis as RA
import refselect as RS
from box_cases import heights

NAMES = ("m", "stat", "aux")
T, DT_MOD = AC.T, AC.DT_MOD
T0, T1 = AC.T0, AC.T1
T_OUT = AC.T_OUT                  # outside the window; the earliest time (a time step there moves nobody)
NPS = (1, 63, 64, 65, 16383, 16384, 16385, 40000)
NQ0 = (65, 16385)                 # ... also without quantities
VARIANTS = AC.VARIANTS
MARK_LAT = 80.5                   # the latitude of the placed hits; everybody else lies south of 70 N
LON = (-30.0, 60.0)
LAT = (-20.0, 45.0)
ZR = (RA.Z(RA.P(5.0)), RA.Z(RA.P(15.0)))
CENTRE = (12.3, 41.7)
R_KM = 800.0
up, down, around = AC.up, AC.down, AC.around


@functools.lru_cache(maxsize=None)
def setup(nq=len(NAMES)):
    """(ctl, clim, met0, met1) as in analysis_cases.setup, with nq quantities"""
    import cases
    from mptrac_amd.ctl import ctl_from_quantities
    from mptrac_amd.synth import synthetic_met
    ctl = dict(cases.BASE, **ctl_from_quantities(NAMES[:nq]))
    m0 = synthetic_met(AC.MET_GRID, 0.0, 1.0, fields=cases.PRESSURE_LEVEL_FIELDS)
    m1 = synthetic_met(AC.MET_GRID, 3600.0, 1.25, fields=cases.PRESSURE_LEVEL_FIELDS)
    return ctl, cases.load_clim_tropo(), m0, m1


def _finish(rows, nq, rng, background):
    """rows [(lon, lat, p, time)] in front of a random background south of 70 N, a tenth of it outside the window"""
    n = len(rows) + background
    a = np.array(rows, dtype=np.float64).reshape(len(rows), 4)
    tb = np.full(background, T)
    tb[::10] = T_OUT
    atm = {"lon": np.concatenate([a[:, 0], rng.uniform(-180.0, 180.0, background)]),
           "lat": np.concatenate([a[:, 1], rng.uniform(-70.0, 70.0, background)]),
           "p": np.concatenate([a[:, 2], RA.P0 * np.exp(-rng.uniform(1.0, 25.0, background) / RA.H0)]),
           "time": np.concatenate([a[:, 3], tb])}
    atm = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in atm.items()}
    atm["q"] = (-1.0) ** rng.integers(2, size=(nq, n)) * 10.0 ** rng.uniform(-8.0, 8.0, (nq, n))
    return atm


# ---------------------------------------------------------------------------
# particle sets
# ---------------------------------------------------------------------------

def marked(n):
    return sorted({0, n - 1} | {i for i in (16383, 16384) if i < n})


@functools.lru_cache(maxsize=None)
def count_set(n, nq):
    rng = np.random.default_rng(4000 + n)
    atm = _finish([], nq, rng, n)
    atm["time"][0] = T_OUT        # (the earliest time is in every set)
    for i in marked(n):
        atm["lat"][i] = MARK_LAT
    return atm


def distance_pairs():
    """[(direction, lon, lat, side)]: adjacent doubles either side of dist2 > R_KM^2 around CENTRE"""
    lon0, lat0 = CENTRE
    out = []

    def far(lon, lat):
        return AC.dist2(lon0, lat0, lon, lat) > R_KM * R_KM

    for name, lo, hi in (("east", lon0 + 1.0, lon0 + 40.0), ("west", lon0 - 40.0, lon0 - 1.0)):
        a, b = AC.bisect(lambda x: far(x, lat0), lo, hi)
        out += [(name, a, lat0, "lo"), (name, b, lat0, "hi")]
    for name, lo, hi, lon in (("north", lat0 + 7.0, lat0 + 7.4, lon0), ("south", lat0 - 7.4, lat0 - 7.0, lon0),
                              ("ne", lat0 + 1.0, lat0 + 7.15, lon0 + 5.0)):
        a, b = AC.bisect(lambda y: far(lon, y), lo, hi)
        out += [(name, lon, a, "lo"), (name, lon, b, "hi")]
    return out


@functools.lru_cache(maxsize=None)
def edges():
    """(atm, tags of the placed particles): everything placed is inside every range but the one its tag names"""
    rng = np.random.default_rng(4242)
    mid = (15.0, 10.0, RA.P(10.0), T)        # inside all four ranges (not within R_KM of CENTRE)
    rows, tags = [], []

    def put(tag, lon=mid[0], lat=mid[1], p=mid[2], time=mid[3]):
        rows.append((lon, lat, p, time))
        tags.append(tag)

    put("mid")
    for k, bound in enumerate((T0, T1)):
        for v, side in around(bound):
            put("time/%d/%s" % (k, side), time=v)
    for k, bound in enumerate(LON):
        for v, side in around(bound):
            put("lon/%d/%s" % (k, side), lon=v)
    for k, bound in enumerate(LAT):
        for v, side in around(bound):
            put("lat/%d/%s" % (k, side), lat=v)
    for k, bound in enumerate(ZR):
        exact, below, above = heights(bound)
        assert exact and below is not None and above is not None
        for v, side in ((exact[0], "on"), (below, "below"), (above, "above")):      # (below: Z(p) < bound)
            put("z/%d/%s" % (k, side), p=v)
    for name, lon, lat, side in distance_pairs():
        put("near/%s/%s" % (name, side), lon=lon, lat=lat)
    put("near/centre", lon=CENTRE[0], lat=CENTRE[1])
    return _finish(rows, len(NAMES), rng, 700), tags


@functools.lru_cache(maxsize=None)
def equal_radius():
    """(r, index of a placed particle) with r * r == dist2(CENTRE, particle) to the bit and the neighbours of r on either
    side of it"""
    atm, tags = edges()
    for i, tag in enumerate(tags):
        if not tag.startswith("near/") or tag == "near/centre":
            continue
        s = AC.dist2(*CENTRE, float(atm["lon"][i]), float(atm["lat"][i]))
        r = math.sqrt(s)
        for v in (r, down(r), up(r)):
            if v * v == s and down(v) * down(v) < s < up(v) * up(v):
                return v, i
    raise AssertionError("no placed particle has a radius with r * r == dist2")


@functools.lru_cache(maxsize=None)
def not_finite():
    """(atm, tags): 30 good particles inside every range and within R_KM of CENTRE, then NaN, +inf and -inf in time, p,
    lon and lat, one at a time in such a particle, among them; then a background"""
    rng = np.random.default_rng(4343)
    rows, tags = [], []
    for j in range(30):
        rows.append([CENTRE[0] + rng.uniform(-2.0, 2.0), CENTRE[1] + rng.uniform(-2.0, 2.0), RA.P(10.0 + rng.uniform(-3.0, 3.0)), T])
        tags.append("good/%d" % j)
    for k, field in enumerate(("lon", "lat", "p", "time")):
        for v in (math.nan, math.inf, -math.inf):
            row = [CENTRE[0], CENTRE[1], RA.P(10.0), T]
            row[k] = v
            rows.append(row)
            tags.append("%s/%r" % (field, v))
    order = rng.permutation(len(rows))
    atm = _finish([rows[i] for i in order], len(NAMES), rng, 100)
    return atm, [tags[i] for i in order]


def particles(name):
    if name == "edges":
        return edges()[0]
    if name == "not_finite":
        return not_finite()[0]
    n, nq = name[1:].split("q")
    return count_set(int(n), int(nq))


def set_names():
    return ["edges", "not_finite"] + ["n%dq%d" % (n, len(NAMES)) for n in NPS] + ["n%dq0" % n for n in NQ0]


# ---------------------------------------------------------------------------
# calls
# ---------------------------------------------------------------------------

EVERY_RANGE = dict(time=(T0, T1), z=ZR, lon=LON, lat=LAT)


def count_calls(n):
    """{name: keyword arguments of select_atm} of a count set"""
    calls = {}
    for s in sorted({1, 2, 7, 64, n - 1, n, n + 1}):
        if s >= 1:
            calls["stride/%d" % s] = dict(stride=s)
    calls["stride7/window"] = dict(stride=7, time=(T0, T1))
    calls["stride2/first1/window"] = dict(stride=2, first=1, time=(T0, T1))
    # first / last with stride 7 and first 0: the candidates are 0, 7, 14, 21, ...
    for name, first, last in (("last_on_0", 0, 0), ("last_on_candidate", 0, 14), ("last_below_candidate", 0, 13),
                              ("last_above_candidate", 0, 15), ("first_on_candidate", 7, -1), ("first_on_0", 0, -1),
                              ("last_beyond", 0, n + 5), ("last_is_np", 0, n), ("last_is_np_minus_1", 0, n - 1),
                              ("first_above_last", 5, 4), ("first_is_last", 14, 14), ("first_beyond", n + 3, -1)):
        calls["range7/" + name] = dict(stride=7, first=first, last=last)
    calls["range7/first_beside_candidate"] = dict(stride=7, first=6, last=-1)
    calls["empty"] = dict(time=(1e6, 2e6))
    calls["everything"] = dict(time=(-math.inf, math.inf))
    calls["one/last"] = dict(first=n - 1, last=n - 1)
    calls["marked"] = dict(lat=(80.0, 81.0))
    calls["marked/stride"] = dict(lat=(80.0, 81.0), stride=16383)       # 0, 16 383, 32 766: one side of the border only
    calls["window"] = dict(time=(T0, T1))
    return calls


def edge_calls():
    calls = {"all": dict(EVERY_RANGE), "all/near": dict(EVERY_RANGE, near=CENTRE + (R_KM,)), "near": dict(near=CENTRE + (R_KM,)),
             "all/stride3": dict(EVERY_RANGE, stride=3), "near/zero": dict(near=CENTRE + (0.0,))}
    for k, v in EVERY_RANGE.items():
        calls[k] = {k: v}
        calls[k + "/point_lo"] = {k: (v[0], v[0])}
        calls[k + "/point_hi"] = {k: (v[1], v[1])}
        calls[k + "/unbounded"] = {k: (-math.inf, math.inf)}
    r, _ = equal_radius()
    for name, v in (("below", down(r)), ("on", r), ("above", up(r))):
        calls["near/r_eq/" + name] = dict(near=CENTRE + (v,))
    return calls


def not_finite_calls():
    calls = {"all": dict(EVERY_RANGE), "all/near": dict(EVERY_RANGE, near=CENTRE + (R_KM,)), "near": dict(near=CENTRE + (R_KM,)),
             "none": {}}
    for k, v in EVERY_RANGE.items():
        calls[k] = {k: v}
    return calls


def calls_of(set_name):
    if set_name == "edges":
        return edge_calls()
    if set_name == "not_finite":
        return not_finite_calls()
    return count_calls(int(set_name[1:].split("q")[0]))


def cases():
    """[(particle set, call name)]"""
    return [(s, c) for s in set_names() for c in calls_of(s)]


def variants_of(set_name):
    """a time step is not defined for a particle without a position: those are looked at as uploaded only"""
    return ("uploaded",) if set_name == "not_finite" else VARIANTS


@functools.lru_cache(maxsize=None)
def expected(set_name, call):
    """the external indices the reference selects"""
    return RS.select(particles(set_name), **calls_of(set_name)[call])


ROW_SUBSETS = (("index",), ("q1",), ("time", "p", "lon", "lat", "q"))
SUBSET_CALLS = {"edges": "all", "n65q3": "stride/2", "n16385q3": "stride7/window", "n40000q3": "window", "n65q0": "stride/2"}
