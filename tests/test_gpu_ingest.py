"""mphip_ingest_met (through Simulation.ingest_met) against tests/refingest.py, the restatement of the definitions in
include/mptrac_hip.h that tests/test_ingest_cpu.py pins to the host loops, on the cases of tests/ingest_cases.py.  Every
comparison is bit for bit (uint32 views, array_equal), in the library this process loaded; tests/test_gpu_ingest_exact.py
runs the same census in the other one and compares the bytes of the two.

Per case: all four stages in one call into compact arrays; into views of larger arrays whose sentinel padding must come
back untouched; each stage bit alone (the later stages from the restatement's result of the earlier ones, in met order);
the two-call form (DECODE, then the other three in met order) against the one-call form; and the met-order form in place.
Refusals return their message, write nothing, and the next valid call is still right.  A call from a second thread while
the first runs time steps returns the same bits and leaves the stepped state alone."""
import ctypes as C
import hashlib
import threading

import numpy as np
import pytest

import ingest_cases as K
import refingest as R
from mptrac_amd import hip
from mptrac_amd.hip import Snapshot
from test_gpu_regrid import bare_context, padding_untouched

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-7777.)
_REF = {}


def axes_of(case, f3=None, f2=None, lon=None):
    s = Snapshot(0.0, case["coord_type"], np.ascontiguousarray(case["lon"] if lon is None else lon),
                 np.ascontiguousarray(case["lat"]), np.ascontiguousarray(case["p"]), f3 or {}, f2 or {})
    return s


def reference(tag, what=R.ALL):
    """The restatement's result of the stages `what` from the raw values of case `tag` (computed once)."""
    if (tag, what) not in _REF:
        c = K.CASES[tag]
        _REF[tag, what] = R.ingest(c["raw"], c["lon"], c["lat"], c["p"], c["coord_type"], what)
    return _REF[tag, what]


def differences(got, ref):
    """The fields of a Snapshot that differ from the restatement's (lon2, f3, f2), as text."""
    lon2, r3, r2 = ref
    wrong = []
    if not np.array_equal(got.lon, lon2):
        wrong.append("lon")
    for name, want in list(r3.items()) + list(r2.items()):
        have = (got.f3 if want.ndim == 3 else got.f2).get(name)
        if have is None or have.shape != want.shape or not np.array_equal(R.bits(have), R.bits(want)):
            n = -1 if have is None or have.shape != want.shape else int((R.bits(have) != R.bits(want)).sum())
            wrong.append(f"{name}:{n}")
    if set(got.f3) != set(r3) or set(got.f2) != set(r2):
        wrong.append("fields")
    return wrong


def update(digest, snap):
    digest.update(np.ascontiguousarray(snap.lon).tobytes())
    for d in (snap.f3, snap.f2):
        for name in sorted(d):
            digest.update(np.ascontiguousarray(d[name]).tobytes())


def one_call(sim, tag):
    c = K.CASES[tag]
    return sim.ingest_met(c["raw"], axes_of(c), R.ALL)


def strided(sim, tag):
    """Into views of larger arrays filled with a sentinel: (snapshot, the padding came back untouched)."""
    c = K.CASES[tag]
    nx2 = sim.ingest_shape(axes_of(c), R.ALL)
    ey, ep = c["ny"] + 3, c["np"] + 5
    out = {}
    for name, (a, _) in c["raw"].items():
        big = np.full((nx2 + 1, ey, ep) if a.ndim == 3 else (nx2 + 1, ey), SENTINEL, dtype=np.float32)
        out[name] = big[:nx2, :c["ny"], :c["np"]] if a.ndim == 3 else big[:nx2, :c["ny"]]
    got = sim.ingest_met(c["raw"], axes_of(c), R.ALL, out=out, out_strides=(ey * ep, ep, ey))
    return got, all(padding_untouched(a) for a in out.values()) and all(got.f3.get(k, got.f2.get(k)) is a for k, a in out.items())


def stages_alone(sim, tag):
    """[(stage bit, snapshot, the restatement's result)]: DECODE from the raw values, every later stage from the
    restatement's result of the stages before it."""
    c = K.CASES[tag]
    rows = [(R.DECODE, sim.ingest_met(c["raw"], axes_of(c), R.DECODE), reference(tag, R.DECODE))]
    before = R.DECODE
    for bit in (R.EXTRAPOLATE, R.POLAR, R.PERIODIC):
        _, f3, f2 = reference(tag, before)
        got = sim.ingest_met(axes_of(c, f3, f2), bit)
        rows.append((bit, got, R.ingest({}, c["lon"], c["lat"], c["p"], c["coord_type"], bit, f3, f2)))
        before |= bit
    return rows


def two_calls(sim, tag):
    c = K.CASES[tag]
    first = sim.ingest_met(c["raw"], axes_of(c), R.DECODE)
    return sim.ingest_met(axes_of(c, first.f3, first.f2), R.ALL & ~R.DECODE)


def in_place(sim, tag):
    """The met-order form on arrays with one spare column, the input the view of the first nx columns: the host layer's
    use of its met_t."""
    c = K.CASES[tag]
    _, f3, f2 = reference(tag, R.DECODE)
    nx = c["nx"]
    big3 = {k: np.concatenate([a, np.full_like(a[:1], SENTINEL)]) for k, a in f3.items()}
    big2 = {k: np.concatenate([a, np.full_like(a[:1], SENTINEL)]) for k, a in f2.items()}
    met = axes_of(c, {k: a[:nx] for k, a in big3.items()}, {k: a[:nx] for k, a in big2.items()})
    nx2 = sim.ingest_shape(met, R.ALL & ~R.DECODE)
    out = {k: a[:nx2] for k, a in list(big3.items()) + list(big2.items())}
    got = sim.ingest_met(met, R.ALL & ~R.DECODE, out=out)
    spare_kept = nx2 > nx or all((a[nx:] == SENTINEL).all() for a in list(big3.values()) + list(big2.values()))
    return got, spare_kept


def census(sim, tags=None):
    """Every case through every form: (rows that differ from the restatement, sha256 of every byte the library returned)."""
    digest = hashlib.sha256()
    wrong = []
    for tag in sorted(K.CASES) if tags is None else tags:
        ref = reference(tag)
        got = one_call(sim, tag)
        update(digest, got)
        wrong += [(tag, "one_call", w) for w in differences(got, ref)]
        got, kept = strided(sim, tag)
        update(digest, got)
        wrong += [(tag, "strided", w) for w in differences(got, ref)] + ([] if kept else [(tag, "strided", "padding")])
        for bit, got, want in stages_alone(sim, tag):
            update(digest, got)
            wrong += [(tag, f"stage_{bit}", w) for w in differences(got, want)]
        got = two_calls(sim, tag)
        update(digest, got)
        wrong += [(tag, "two_calls", w) for w in differences(got, ref)]
        got, kept = in_place(sim, tag)
        update(digest, got)
        wrong += [(tag, "in_place", w) for w in differences(got, ref)] + ([] if kept else [(tag, "in_place", "spare column")])
    return wrong, digest.hexdigest()


@pytest.fixture(scope="module")
def sim():
    s = bare_context()
    yield s
    s.close()


@pytest.mark.parametrize("tag", sorted(K.CASES))
def test_all_four_stages_give_the_restatement_bits(sim, tag):
    assert differences(one_call(sim, tag), reference(tag)) == []


@pytest.mark.parametrize("tag", sorted(K.CASES))
def test_views_into_larger_arrays_and_their_padding(sim, tag):
    got, kept = strided(sim, tag)
    assert differences(got, reference(tag)) == [] and kept


@pytest.mark.parametrize("tag", sorted(K.CASES))
def test_each_stage_alone_the_two_call_form_and_in_place(sim, tag):
    for bit, got, want in stages_alone(sim, tag):
        assert differences(got, want) == [], bit
    assert differences(two_calls(sim, tag), reference(tag)) == []
    got, kept = in_place(sim, tag)
    assert differences(got, reference(tag)) == [] and kept


def test_ingest_shape_answers_without_a_context():
    L = hip.load()
    for tag, c in K.CASES.items():
        m = hip.Simulation._met_struct(None, axes_of(c))
        n = C.c_int(-1)
        assert L.mphip_ingest_shape(C.byref(m), R.ALL, C.byref(n)) == 0
        assert n.value == c["nx"] + int(R.periodic_acts(c["lon"], c["coord_type"])), tag
        assert L.mphip_ingest_shape(C.byref(m), R.ALL & ~R.PERIODIC, C.byref(n)) == 0 and n.value == c["nx"]
        assert L.mphip_ingest_shape(C.byref(m), 0, C.byref(n)) != 0 and L.mphip_ingest_shape(C.byref(m), 16, C.byref(n)) != 0


# ---- refusals ------------------------------------------------------------------------------------------------------------

def refusal_rows(sim):
    """[(name, return code, message, the outputs kept their sentinel, the message expected)] of every refusal, and after
    each one a valid call that must still be right (its differences are appended as a row of their own)."""
    tag = "all_short_fill_hit_miss_hit"
    c = K.CASES[tag]
    nx, ny, np_ = c["nx"], c["ny"], c["np"]
    rows = []

    def attempt(name, expect, mutate, what=R.ALL):
        met = axes_of(c)
        m = sim._met_struct(met)
        raw = hip.MphipIngestRaw()
        keep = []
        for f, (a, o) in c["raw"].items():
            d = raw.f3[hip.FIELDS_3D.index(f)] if a.ndim == 3 else raw.f2[hip.FIELDS_2D.index(f)]
            d.data, d.type = a.ctypes.data, hip.RAW_SHORT
            d.scale_factor, d.add_offset, d.scl = o["scale_factor"], o["add_offset"], o["scl"]
            d.fill_s, d.miss_s, d.lnsp = o.get("fill", 0), o.get("miss", 0), o.get("lnsp", 0)
        mo = hip.MphipRegridOut()
        mo.sx, mo.sy, mo.sx2 = ny * np_, np_, ny
        outs = {}
        for f, (a, o) in c["raw"].items():
            outs[f] = np.full((nx + 1, ny, np_) if a.ndim == 3 else (nx + 1, ny), SENTINEL, dtype=np.float32)
            if a.ndim == 3:
                mo.f3[hip.FIELDS_3D.index(f)] = outs[f].ctypes.data_as(hip._fp)
            else:
                mo.f2[hip.FIELDS_2D.index(f)] = outs[f].ctypes.data_as(hip._fp)
        args = dict(m=m, raw=raw, mo=mo, what=what, keep=keep, raw_ptr=C.byref(raw), m_ptr=C.byref(m), mo_ptr=C.byref(mo))
        mutate(args)
        rc = sim.L.mphip_ingest_met(sim.h, args["m_ptr"], args["raw_ptr"], args["what"], args["mo_ptr"])
        msg = sim.L.mphip_last_error(sim.h).decode() if rc else ""
        untouched = all((a == SENTINEL).all() for a in outs.values())
        rows.append((name, rc, msg, untouched, "mphip_ingest_met: " + expect))
        rows.append((name + ": the next call", 0, ";".join(differences(one_call(sim, tag), reference(tag))), True, ""))

    T, PS, ZS = hip.FIELDS_3D.index("t"), hip.FIELDS_2D.index("ps"), hip.FIELDS_2D.index("zs")
    met_order = np.zeros((nx, ny, np_), dtype=np.float32)
    big_lon = np.zeros(1 << 23)

    def set_(**kw):
        def mutate(a):
            for k, v in kw.items():
                obj, member = k.split("__")
                setattr(a[obj], member, v)
        return mutate

    attempt("what 0", "`what` must be an OR of MPHIP_INGEST_* bits", lambda a: a.update(what=0))
    attempt("what 16", "`what` must be an OR of MPHIP_INGEST_* bits", lambda a: a.update(what=16))
    attempt("what 31", "`what` must be an OR of MPHIP_INGEST_* bits", lambda a: a.update(what=31))
    attempt("null in", "null argument", lambda a: a.update(m_ptr=None))
    attempt("null out", "null argument", lambda a: a.update(mo_ptr=None))
    attempt("null raw with DECODE", "null argument", lambda a: a.update(raw_ptr=None))
    attempt("no lon", "the input axes are missing", set_(m__lon=None))
    attempt("no lat", "the input axes are missing", set_(m__lat=None))
    attempt("no p", "the input axes are missing", set_(m__p=None))
    attempt("nx 1", "meteo grid dimensions out of range", set_(m__nx=1))
    attempt("ny 1", "meteo grid dimensions out of range", set_(m__ny=1))
    attempt("np 1", "needs two pressure levels or more (np < 2)", set_(m__np=1))
    attempt("nx ny 2^24", "meteo grid too large for the device index arithmetic",
            set_(m__nx=1 << 23, m__ny=2, m__lon=big_lon.ctypes.data_as(hip._dp)))
    attempt("nx ny np 2^31", "meteo grid too large for the device index arithmetic", set_(m__nx=1 << 12, m__ny=1 << 10, m__np=1 << 9))
    attempt("out sy < np", "the output strides do not hold the grid", set_(mo__sy=np_ - 1))
    attempt("out sx < ny sy", "the output strides do not hold the grid", set_(mo__sx=(ny - 1) * np_))
    attempt("out sx no multiple of sy", "the output strides do not hold the grid", set_(mo__sx=ny * np_ + 1))
    attempt("out sx2 < ny", "the output strides do not hold the grid", set_(mo__sx2=ny - 1))

    def unknown_type(a):
        a["raw"].f3[T].type = 7
    attempt("unknown type", "field t has a raw descriptor of unknown type", unknown_type)

    def no_data(a):
        a["raw"].f3[T].data = None
    attempt("no data", "field t has a raw descriptor without data", no_data)

    def both(a):
        a["m"].f3[T] = met_order.ctypes.data_as(hip._fp)
        a["m"].sx, a["m"].sy = ny * np_, np_
    attempt("raw and met order", "field t is given both raw and in met order", both)

    def lnsp_zs(a):
        a["raw"].f2[ZS].lnsp = 1
    attempt("lnsp on zs", "field zs: lnsp belongs to the surface pressure alone", lnsp_zs)

    def lnsp_t(a):
        a["raw"].f3[T].lnsp = 1
    attempt("lnsp on t", "field t: lnsp belongs to the surface pressure alone", lnsp_t)

    def nothing(a):
        for f in range(len(hip.FIELDS_3D)):
            a["mo"].f3[f] = None
        for f in range(len(hip.FIELDS_2D)):
            a["mo"].f2[f] = None
    attempt("no field", "no field is given in `in` or `raw` and named in `out`", nothing)

    def bad_in_strides(a):
        a["raw"].f3[T].type = 0
        a["m"].f3[T] = met_order.ctypes.data_as(hip._fp)
        a["m"].sx, a["m"].sy = ny * np_, np_ - 1
    attempt("in sy < np", "unsupported meteo strides", bad_in_strides)
    return rows


N_REFUSALS = 25


def test_every_refusal_names_its_cause_writes_nothing_and_the_next_call_is_right(sim):
    rows = refusal_rows(sim)
    assert len(rows) == 2 * N_REFUSALS
    for name, rc, msg, untouched, expect in rows:
        if expect:
            assert rc != 0 and msg == expect and untouched, (name, rc, msg, untouched)
        else:
            assert msg == "", (name, msg)


def test_the_binding_reports_a_refusal_as_an_error(sim):
    c = K.CASES["winds_and_t"]
    with pytest.raises(hip.MphipError, match="mphip_ingest_met: `what` must be an OR"):
        sim.ingest_met(c["raw"], axes_of(c), 16)
    raw = dict(c["raw"])
    raw["t"] = (None, dict(c["raw"]["t"][1], type=hip.RAW_FLOAT))
    with pytest.raises(hip.MphipError, match="mphip_ingest_met: field t has a raw descriptor without data"):
        sim.ingest_met(raw, axes_of(c), R.ALL)
    assert differences(one_call(sim, "winds_and_t"), reference("winds_and_t")) == []


# ---- from a second thread ------------------------------------------------------------------------------------------------

def second_thread():
    """(errors, the reader's calls returned the restatement's bits, the stepped state equals a run without the reader)"""
    import cases
    tag = "all_short_fill_hit_miss_hit"
    states, errors, good = [], [], []
    for with_reader in (False, True):
        ctl, clim, m0, m1, atm = cases.make_case("advect", n=5000, grid="tiny")
        s = hip.Simulation(ctl, clim, m0, m1, atm)
        s.timesteps_init(0.0, 0.0)
        times = cases.step_times(s.ctl)

        def reader():
            try:
                for _ in range(4):
                    good.append(differences(one_call(s, tag), reference(tag)) == [])
            except BaseException as exc:      # noqa: BLE001
                errors.append(repr(exc))

        th = threading.Thread(target=reader)
        s.run_timestep(times[0])
        if with_reader:
            th.start()
        for k in range(1, min(17, len(times) - 3), 4):
            s.run_timesteps(times[k], 4)
        if with_reader:
            th.join()
        s.synchronize()
        states.append(s.state())
        s.close()
    same = all(np.array_equal(states[0][k], states[1][k]) for k in ("time", "lon", "lat", "p"))
    return errors, len(good) == 4 and all(good), same


def test_a_call_from_a_second_thread_while_the_first_steps():
    errors, good, same = second_thread()
    assert errors == [] and good and same
