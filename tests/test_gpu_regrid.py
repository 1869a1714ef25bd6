"""mphip_regrid_met (through Simulation.regrid_met) against tests/refregrid.py, the restatement of the definitions in
include/mptrac_hip.h, on the cases of tests/regrid_cases.py.

libmptrac_hip_exact.so returns the restatement's bits -- NaNs in the same places --, degenerate columns (NaN, equal
pressures, non-monotone) included.  libmptrac_hip.so: SAMPLE within 2 float ulp (the bar of the geopotential's
smoothing); ML2PL on finite monotone columns within ulp_float(ref) + 16 2^-53 (|f[k]| + |f[k+1]|): one float rounding
boundary, and the forward bound of LIN's four double roundings with a fast division and a contracted final sum, which
matters only where the result cancels to near zero.  A process loads one library: each runs in a child that reports
per case what it measured (as tests/test_gpu_metprep.py does); the refusals and the layouts run in both."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refregrid as R        # noqa: E402
import regrid_cases as K     # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-7777.)


def bare_context():
    import ctypes as C
    from mptrac_amd import hip
    sim = object.__new__(hip.Simulation)
    sim.L = hip.load()
    sim.h = C.c_void_p()
    assert sim.L.mphip_create(C.byref(sim.h), 0) == 0
    return sim


def compare(got, ref, bound=None):
    """Worst distances of one field: NaN pattern, float ulp, and (ML2PL in the default library) the share of the bound."""
    ng, nr = np.isnan(got), np.isnan(ref)
    both = ~ng & ~nr
    d = R.ulp_distance(got[both], ref[both])
    row = dict(nan_mismatch=int((ng != nr).sum()), bits_differ=int((d != 0).sum()), max_ulp=int(d.max()) if d.size else 0,
               zero_sign=int((np.signbit(got[both]) != np.signbit(ref[both])).sum()))
    if bound is not None:
        err = np.abs(got[both].astype(np.float64) - ref[both].astype(np.float64))
        row["share"] = float((err / bound[both]).max()) if err.size else 0.0
    return row


def worst(rows):
    out = dict(nan_mismatch=0, bits_differ=0, max_ulp=0, zero_sign=0, share=0.0)
    for r in rows:
        for k in r:
            out[k] = max(out[k], r[k])
    return out


def compare_snapshots(got, ref, bounds=None):
    assert sorted(got.f3) == sorted(ref.f3) and sorted(got.f2) == sorted(ref.f2), (sorted(got.f3), sorted(ref.f3))
    assert np.array_equal(got.lon, ref.lon) and np.array_equal(got.lat, ref.lat) and np.array_equal(got.p, ref.p)
    rows = [compare(got.f3[n], ref.f3[n], None if bounds is None else bounds[n]) for n in ref.f3]
    rows += [compare(got.f2[n], ref.f2[n]) for n in ref.f2]
    return worst(rows)


def sentinel_like(shape3, names3, names2, strides=None):
    nx, ny, n = shape3
    out = {}
    for f in names3:
        out[f] = np.full(shape3, SENTINEL) if strides is None else \
            np.full((nx, strides[0] // strides[1], strides[1]), SENTINEL)[:, :ny, :n]
    for f in names2:
        out[f] = np.full((nx, ny), SENTINEL) if strides is None else np.full((nx, strides[2]), SENTINEL)[:, :ny]
    return out


def untouched(a):
    return bool((a == SENTINEL).all() and (a.base is None or (a.base == SENTINEL).all()))


def padding_untouched(a):
    big = a.base.copy()
    big[tuple(slice(0, n) for n in a.shape)] = SENTINEL
    return bool((big == SENTINEL).all())


# ---- the child: every case, one library --------------------------------------------------------------------------------

def child_ml2pl(sim, exact, rows):
    for nx, ny in K.ML_GRIDS:
        for npl in K.ML_LEVELS:
            for met_np in K.ML_TARGETS:
                for asc in (False, True):
                    met = K.ml_atmosphere(nx, ny, npl, ascending=asc)
                    q = K.targets(met_np)
                    ref = R.ml2pl(met, q)
                    got = sim.regrid_met(met, "ml2pl", met_p=q)
                    row = compare_snapshots(got, ref, R.ml2pl_bound(met, q, ref))
                    rows.append(dict(kind="ml2pl", case=[nx, ny, npl, met_np, asc], **row))
    for asc in (False, True):        # targets on the levels of a column, one double ulp either side, at and beyond the ends
        for npl in (7, 137):
            met = K.ml_atmosphere(9, 8, npl, ascending=asc)
            q = K.targets_on_levels(met)
            ref = R.ml2pl(met, q)
            got = sim.regrid_met(met, "ml2pl", met_p=q)
            rows.append(dict(kind="ml2pl", case=["on_levels", npl, asc], **compare_snapshots(got, ref, R.ml2pl_bound(met, q, ref))))
    if exact:
        for kind in K.DEGENERATE:
            met = K.degenerate(kind)
            q = K.targets(5)
            with np.errstate(all="ignore"):
                ref = R.ml2pl(met, q)
            rows.append(dict(kind="degenerate", case=[kind], **compare_snapshots(sim.regrid_met(met, "ml2pl", met_p=q), ref)))


def child_ml2pl_layouts(sim, rows):
    met = K.ml_atmosphere(9, 8, 7)
    q = K.targets(5)
    ref = R.ml2pl(met, q)
    compact = sim.regrid_met(met, "ml2pl", met_p=q)
    same = lambda a, b: bool(np.array_equal(a.view(np.int32), b.view(np.int32)))      # noqa: E731
    # strided input against compact input
    view = K.strided(met)
    got = sim.regrid_met(view, "ml2pl", met_p=q)
    ok = all(same(got.f3[n], compact.f3[n]) for n in ref.f3) and all(same(got.f2[n], compact.f2[n]) for n in ref.f2)
    rows.append(dict(kind="layout", case=["strided_input"], ok=ok))
    # strided output: the padding stays
    st = (11 * 9, 9, 11)
    out = sentinel_like((9, 8, 5), ref.f3, ref.f2, st)
    got = sim.regrid_met(met, "ml2pl", met_p=q, out=out, out_strides=st)
    ok = all(same(out[n], compact.f3[n]) and padding_untouched(out[n]) for n in ref.f3) \
        and all(same(out[n], compact.f2[n]) and padding_untouched(out[n]) for n in ref.f2)
    rows.append(dict(kind="layout", case=["strided_output"], ok=ok))
    # a subset of the fields: the outputs of absent fields stay, and so does an output the caller leaves out
    part = K.ml_atmosphere(9, 8, 7)
    part.f3 = {n: a for n, a in part.f3.items() if n in ("pl", "t", "u", "o3")}
    del part.f2["zs"]
    out = sentinel_like((9, 8, 5), R.PL_FIELDS + ("pl", "ul", "wl"), ("ps", "zs", "ts", "pbl"))
    out["u"] = None
    got = sim.regrid_met(part, "ml2pl", met_p=q, out=out)
    ok = sorted(got.f3) == ["o3", "t"] and same(got.f3["t"], compact.f3["t"]) and same(got.f3["o3"], compact.f3["o3"]) \
        and sorted(got.f2) == ["ps", "ts"] and same(got.f2["ps"], compact.f2["ps"]) \
        and all(untouched(out[n]) for n in out if n not in ("t", "o3", "u", "ps", "ts"))
    rows.append(dict(kind="layout", case=["subset"], ok=bool(ok)))
    # out aliasing in: the strided arrays are regridded in place
    view = K.strided(met)
    st = view.strides
    out = {n: a.base[:, :met.ny, :5] for n, a in view.f3.items() if n != "pl"}
    out.update({n: a for n, a in view.f2.items()})
    pl_before = view.f3["pl"].base.copy()
    got = sim.regrid_met(view, "ml2pl", met_p=q, out=out, out_strides=st)
    ok = all(same(out[n], compact.f3[n]) for n in ref.f3) and all(same(out[n], compact.f2[n]) for n in ref.f2) \
        and np.array_equal(view.f3["pl"].base, pl_before) \
        and all(same(out[n].base[:, :met.ny, 5:7], K.strided(met).f3[n][:, :, 5:7]) for n in ref.f3)
    rows.append(dict(kind="layout", case=["in_place"], ok=bool(ok)))


def refused(sim, met, what, out, **kw):
    from mptrac_amd import hip
    try:
        sim.regrid_met(met, what, out=out, **kw)
    except hip.MphipError as exc:
        return all(untouched(a) for a in out.values()), str(exc)
    return False, "accepted"


def child_refusals(sim, rows):
    q = K.targets(5)

    def ml_case(name, met, **kw):
        kw.setdefault("met_p", q)
        shape = (met.nx, met.ny, max(len(kw["met_p"]), 1))
        out = sentinel_like(shape, R.ML_FIELDS, K.SURFACE)
        ok, msg = refused(sim, met, "ml2pl", out, **kw)
        rows.append(dict(kind="refusal", case=[name], ok=ok, message=msg))

    met = K.ml_atmosphere(5, 3, 7)
    one = K.ml_atmosphere(5, 3, 2)
    one.f3 = {k: np.ascontiguousarray(v[:, :, :1]) for k, v in one.f3.items()}
    one.np = one.npl = 1
    ml_case("npl_1", one)
    other = K.ml_atmosphere(5, 3, 7)
    other.npl = 6
    ml_case("np_is_not_npl", other)
    nopl = K.ml_atmosphere(5, 3, 7)
    del nopl.f3["pl"]
    ml_case("no_pl", nopl)
    ml_case("met_np_1", met, met_p=q[:1])
    ml_case("met_p_ascending", met, met_p=q[::-1])
    ml_case("met_p_equal", met, met_p=[500.0, 500.0, 100.0])
    ml_case("met_p_negative", met, met_p=[500.0, -1.0])
    ml_case("met_p_nan", met, met_p=[500.0, np.nan])
    ml_case("met_p_inf", met, met_p=[np.inf, 500.0])
    tall = K.ml_atmosphere(2, 2, 16400, fields=("t",))       # 4 (16400 | 1) bytes for one column: beyond 64 KB
    ml_case("too_many_levels", tall)

    def sample_case(name, grid, **kw):
        met, _, _ = K.sample_input(grid)
        n = R.shape((met.nx, met.ny, met.np), [max(kw.get(k, 1), 1) for k in ("met_dx", "met_dy", "met_dp")])
        out = sentinel_like(n, met.f3, met.f2)
        ok, msg = refused(sim, met, "sample", out, **kw)
        rows.append(dict(kind="refusal", case=[name], ok=ok, message=msg))

    sample_case("dx_0", "identity", met_dx=0)
    sample_case("dy_negative", "identity", met_dy=-2)
    sample_case("sp_0", "identity", met_sp=0)
    sample_case("sx_beyond_nx", "identity", met_sx=11)
    sample_case("nx2_1", "identity", met_dx=9)
    sample_case("ny2_1", "identity", met_dy=7)
    sample_case("np2_1", "identity", met_dp=6)
    sample_case("tile_beyond_lds", K.TOO_LARGE_TILE, met_sx=11, met_sy=11, met_sp=4)
    out = sentinel_like((9, 7, 6), ("t",), ("ps",))
    ok, msg = refused(sim, K.sample_input("identity")[0], 4, out)
    rows.append(dict(kind="refusal", case=["what"], ok=ok, message=msg))


def child_sample(sim, rows):
    for name in K.SAMPLE_CASES:
        met, d, s = K.sample_input(name)
        for nan in (False, True):
            if nan and name not in ("strides_and_smoothing", "half_widths_3_2_2"):
                continue
            if nan:
                met = K.with_nan(met)
            with np.errstate(all="ignore"):
                ref = R.sample(met, d, s)
            got = sim.regrid_met(met, "sample", met_dx=d[0], met_dy=d[1], met_dp=d[2], met_sx=s[0], met_sy=s[1], met_sp=s[2])
            rows.append(dict(kind="sample", case=[name, nan], **compare_snapshots(got, ref)))
    # strided input and output
    met, d, s = K.sample_input("strides_and_smoothing")
    opts = dict(met_dx=d[0], met_dy=d[1], met_dp=d[2], met_sx=s[0], met_sy=s[1], met_sp=s[2])
    compact = sim.regrid_met(met, "sample", **opts)
    st = (7 * 5, 5, 6)
    out = sentinel_like((5, 3, 3), met.f3, met.f2, st)
    sim.regrid_met(K.strided(met), "sample", out=out, out_strides=st, **opts)
    ok = all(np.array_equal(out[n], compact.f3[n]) and padding_untouched(out[n]) for n in met.f3) \
        and all(np.array_equal(out[n], compact.f2[n]) and padding_untouched(out[n]) for n in met.f2)
    rows.append(dict(kind="layout", case=["sample_strided"], ok=bool(ok)))


def child_both(sim, rows):
    """Both bits in one call against the two calls in sequence: the same bits; and against the restatement."""
    for d, s in (((2, 3, 2), (2, 2, 2)), ((1, 1, 1), (1, 1, 1)), ((2, 2, 1), (2, 2, 1))):
        met = K.ml_atmosphere(9, 8, 137)
        q = K.targets(60)
        opts = dict(met_dx=d[0], met_dy=d[1], met_dp=d[2], met_sx=s[0], met_sy=s[1], met_sp=s[2])
        one = sim.regrid_met(met, ("ml2pl", "sample"), met_p=q, **opts)
        first = sim.regrid_met(met, "ml2pl", met_p=q)
        two = sim.regrid_met(first, "sample", **opts)
        ok = sorted(one.f3) == sorted(two.f3) and sorted(one.f2) == sorted(two.f2) \
            and all(np.array_equal(one.f3[n].view(np.int32), two.f3[n].view(np.int32)) for n in one.f3) \
            and all(np.array_equal(one.f2[n].view(np.int32), two.f2[n].view(np.int32)) for n in one.f2) \
            and np.array_equal(one.p, two.p) and np.array_equal(one.lon, two.lon) and np.array_equal(one.lat, two.lat)
        rows.append(dict(kind="layout", case=["both", list(d), list(s)], ok=bool(ok)))
        ref = R.sample(R.ml2pl(met, q), d, s)
        rows.append(dict(kind="both", case=[list(d), list(s)], **compare_snapshots(one, ref)))


def child():
    from mptrac_amd import hip
    version = hip.load().mphip_version().decode()
    print("library:", version, flush=True)
    exact = "reference rounding" in version
    sim = bare_context()
    rows = []
    child_ml2pl(sim, exact, rows)
    child_ml2pl_layouts(sim, rows)
    child_refusals(sim, rows)
    child_sample(sim, rows)
    child_both(sim, rows)
    sim.close()
    print("JSON " + json.dumps(rows))


def _run_child(exact):
    env = dict(os.environ, MPTRAC_AMD_EXACT="1" if exact else "0")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=300,
                         env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert ("reference rounding" in lib) == exact, lib
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("JSON ")][0][5:])


@pytest.fixture(scope="module")
def exact_rows():
    return _run_child(True)


@pytest.fixture(scope="module")
def default_rows():
    return _run_child(False)


def _of(rows, kind):
    sel = [r for r in rows if r["kind"] == kind]
    assert sel, kind
    return sel


N_ML = len(K.ML_GRIDS) * len(K.ML_LEVELS) * len(K.ML_TARGETS) * 2 + 4


def test_exact_library_returns_the_restatements_bits(exact_rows):
    assert len(_of(exact_rows, "ml2pl")) == N_ML and len(_of(exact_rows, "degenerate")) == len(K.DEGENERATE)
    assert len(_of(exact_rows, "sample")) == len(K.SAMPLE_CASES) + 2 and len(_of(exact_rows, "both")) == 3
    for kind in ("ml2pl", "degenerate", "sample", "both"):
        for r in _of(exact_rows, kind):
            assert r["nan_mismatch"] == 0 and r["bits_differ"] == 0 and r["zero_sign"] == 0, r


def test_default_library_ml2pl_within_the_bound(default_rows):
    """Largest share of the bound measured: 0.18, largest distance 1 float ulp."""
    rows = _of(default_rows, "ml2pl")
    assert len(rows) == N_ML
    print("ml2pl: largest share of the bound", max(r["share"] for r in rows), "largest float ulp", max(r["max_ulp"] for r in rows))
    for r in rows:
        assert r["nan_mismatch"] == 0 and r["share"] <= 1.0, r


def test_default_library_sample_within_two_ulp(default_rows):
    rows = _of(default_rows, "sample")
    assert len(rows) == len(K.SAMPLE_CASES) + 2
    print("sample: largest float ulp", max(r["max_ulp"] for r in rows))       # (measured: 0)
    for r in rows:
        assert r["nan_mismatch"] == 0 and r["max_ulp"] <= 2, r


@pytest.mark.parametrize("lib", ["exact", "default"])
def test_layouts_subsets_aliasing_and_both_bits(lib, exact_rows, default_rows):
    rows = _of(exact_rows if lib == "exact" else default_rows, "layout")
    assert sorted(r["case"][0] for r in rows) == sorted(["strided_input", "strided_output", "subset", "in_place", "sample_strided",
                                                         "both", "both", "both"])
    for r in rows:
        assert r["ok"], r


@pytest.mark.parametrize("lib", ["exact", "default"])
def test_every_refusal_writes_nothing(lib, exact_rows, default_rows):
    rows = _of(exact_rows if lib == "exact" else default_rows, "refusal")
    assert len(rows) == 19
    for r in rows:
        assert r["ok"] and r["message"].startswith("mphip_regrid_met: "), r


if __name__ == "__main__" and "--child" in sys.argv:
    child()
