"""mphip_detrend_met (through Simulation.detrend_met) against tests/refdetrend.py, the restatement of the definition in
include/mptrac_hip.h, on the cases of tests/detrend_cases.py.

libmptrac_hip_exact.so returns the restatement's bits, NaNs and infinities in the same places.  libmptrac_hip.so may
differ through the one float division: |got - ref| <= 2 ulp_float(|b_ref|) + ulp_float(|ref|) with b_ref the
restatement's background (measured: 0, the division is IEEE in both libraries).  A process loads one library: each runs in
a child that reports per case what it measured (as tests/test_gpu_regrid.py does); the layouts, the refusals, the scratch
and the call from a second thread run in both."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detrend_cases as K       # noqa: E402
import refdetrend as R          # noqa: E402
from refregrid import ulp_distance      # noqa: E402
from test_gpu_regrid import bare_context, padding_untouched      # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-7777.)


def same_bits(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32)))


def compare(got, ref, bg):
    """One field: where the restatement is finite the distance in float ulp and the share of the default library's bound;
    elsewhere the same NaN or the same infinity."""
    fin = np.isfinite(ref)
    other = int((~same_bits_each(got[~fin], ref[~fin]) & ~(np.isnan(got[~fin]) & np.isnan(ref[~fin]))).sum())
    other += int((~np.isfinite(got[fin])).sum())
    g, r, b = got[fin], ref[fin], bg[fin]
    ok = np.isfinite(g)
    d = ulp_distance(g[ok], r[ok])
    with np.errstate(all="ignore"):
        bound = 2.0 * np.spacing(np.abs(b[ok])).astype(np.float64) + np.spacing(np.abs(r[ok])).astype(np.float64)
        err = np.abs(g[ok].astype(np.float64) - r[ok].astype(np.float64))
    return dict(nonfinite_mismatch=other, bits_differ=int((d != 0).sum()), max_ulp=int(d.max()) if d.size else 0,
                zero_sign=int((np.signbit(g[ok]) != np.signbit(r[ok])).sum()),
                share=float((err / bound).max()) if err.size else 0.0)


def same_bits_each(a, b):
    return np.ascontiguousarray(a).view(np.int32) == np.ascontiguousarray(b).view(np.int32)


def worst(rows):
    out = dict(nonfinite_mismatch=0, bits_differ=0, max_ulp=0, zero_sign=0, share=0.0)
    for r in rows:
        for k in r:
            out[k] = max(out[k], r[k])
    return out


# ---- the child: every case, one library --------------------------------------------------------------------------------

def child_cases(sim, rows):
    first = {}
    for name in list(K.CASES) + ["smallest", "widest"]:        # (again at the end: the scratch has grown meanwhile)
        met, scale = K.case(name)
        ref = K.reference(name)
        got = sim.detrend_met(met, scale)
        assert sorted(got) == sorted(ref)
        if name in first:
            rows.append(dict(kind="layout", case=["again_" + name], ok=all(same_bits(got[f], first[name][f]) for f in got)))
            continue
        first[name] = got
        rows.append(dict(kind="case", case=[name], **worst([compare(got[f], ref[f][0], ref[f][1]) for f in ref])))


def child_layouts(sim, rows):
    met, scale = K.case("poles")
    compact = sim.detrend_met(met, scale)
    # (h) strided input and output: the padding survives
    view = K.strided(met)
    out = {f: np.full_like(view.f3[f].base, SENTINEL)[:, :met.ny, :met.np] for f in R.FIELDS}
    sim.detrend_met(view, scale, out=out, out_strides=view.strides[:2])
    ok = all(same_bits(out[f], compact[f]) and padding_untouched(out[f]) for f in R.FIELDS) \
        and all((view.f3[f].base[:, met.ny:, :] == -5555.0).all() and (view.f3[f].base[:, :, met.np:] == -5555.0).all()
                for f in R.FIELDS)
    rows.append(dict(kind="layout", case=["strided"], ok=bool(ok)))
    # (i) in place
    met2, _ = K.case("poles")
    got = sim.detrend_met(met2, scale, out=dict(met2.f3))
    ok = all(got[f] is met2.f3[f] and same_bits(met2.f3[f], compact[f]) for f in R.FIELDS)
    rows.append(dict(kind="layout", case=["in_place"], ok=bool(ok)))
    # in place in a strided view
    view = K.strided(met)
    sim.detrend_met(view, scale, out=dict(view.f3), out_strides=view.strides[:2])
    ok = all(same_bits(view.f3[f], compact[f]) and (view.f3[f].base[:, met.ny:, :] == -5555.0).all()
             and (view.f3[f].base[:, :, met.np:] == -5555.0).all() for f in R.FIELDS)
    rows.append(dict(kind="layout", case=["in_place_strided"], ok=bool(ok)))
    # (j) only u present; only t requested (the other outputs are handed over all the same and stay as they are)
    only_u = K.atmosphere(met.lon, met.lat, met.np, 2, fields=("u",))
    only_u.f3["u"] = met.f3["u"]
    got = sim.detrend_met(only_u, scale)
    rows.append(dict(kind="layout", case=["only_u"], ok=bool(sorted(got) == ["u"] and same_bits(got["u"], compact["u"]))))
    got = sim.detrend_met(met, scale, fields=("t",))
    rows.append(dict(kind="layout", case=["only_t"], ok=bool(sorted(got) == ["t"] and same_bits(got["t"], compact["t"]))))
    # other slots of `out` and the axes stay untouched
    import ctypes as C
    from mptrac_amd import hip
    m = sim._met_struct(met)
    mo = hip.MphipRegridOut()
    mo.sx, mo.sy, mo.sx2 = met.ny * met.np, met.np, met.ny
    arrays = {f: np.full((met.nx, met.ny, met.np), SENTINEL) for f in hip.FIELDS_3D}
    planes = {f: np.full((met.nx, met.ny), SENTINEL) for f in hip.FIELDS_2D}
    axes = [np.full(n, -1.0) for n in (met.nx, met.ny, met.np)]
    for i, f in enumerate(hip.FIELDS_3D):
        mo.f3[i] = hip._ptr(arrays[f], hip._fp)
    for i, f in enumerate(hip.FIELDS_2D):
        mo.f2[i] = hip._ptr(planes[f], hip._fp)
    mo.lon, mo.lat, mo.p = (hip._ptr(a, hip._dp) for a in axes)
    rc = sim.L.mphip_detrend_met(sim.h, C.byref(m), C.byref(hip.MphipDetrend(scale)), C.byref(mo))
    ok = rc == 0 and all(same_bits(arrays[f], compact[f]) for f in R.FIELDS) \
        and all((arrays[f] == SENTINEL).all() for f in hip.FIELDS_3D if f not in R.FIELDS) \
        and all((planes[f] == SENTINEL).all() for f in planes) and all((a == -1.0).all() for a in axes)
    rows.append(dict(kind="layout", case=["other_slots"], ok=bool(ok)))


def child_refusals(sim, rows):
    import ctypes as C
    from mptrac_amd import hip
    base, scale = K.case("smallest")

    def attempt(name, word, change=None, scale=scale, null_opt=False, met=None, fields=R.FIELDS):
        met = met or base
        lon, lat, p = met.lon.copy(), met.lat.copy(), met.p.copy()
        snap = K.Snap(lon, lat, p, met.f3, {}, met.time)
        m = sim._met_struct(snap)
        mo = hip.MphipRegridOut()
        mo.sx, mo.sy, mo.sx2 = met.ny * met.np, met.np, met.ny
        outs = {f: np.full((met.nx, met.ny, met.np), SENTINEL) for f in fields}
        for f in fields:
            mo.f3[hip.FIELDS_3D.index(f)] = hip._ptr(outs[f], hip._fp)
        if change:
            change(m, mo, lon, lat)
        opt = hip.MphipDetrend(scale)
        rc = sim.L.mphip_detrend_met(sim.h, C.byref(m), None if null_opt else C.byref(opt), C.byref(mo))
        msg = sim.L.mphip_last_error(sim.h).decode()
        rows.append(dict(kind="refusal", case=[name], message=msg,
                         ok=bool(rc != 0 and word in msg and all((a == SENTINEL).all() for a in outs.values()))))

    def setter(**kw):
        def change(m, mo, lon, lat):
            for k, v in kw.items():
                setattr(m, k, v)
        return change

    def out_setter(**kw):
        def change(m, mo, lon, lat):
            for k, v in kw.items():
                setattr(mo, k, v)
        return change

    def axis(which, i, v):
        def change(m, mo, lon, lat):
            (lon if which == "lon" else lat)[i] = v
        return change

    attempt("null_opt", "null argument", null_opt=True)
    attempt("null_lon", "axes", setter(lon=None))
    attempt("null_lat", "axes", setter(lat=None))
    attempt("null_p", "axes", setter(p=None))
    attempt("nx_1", "dimensions", setter(nx=1))
    attempt("ny_1", "dimensions", setter(ny=1))
    attempt("np_1", "np < 2", setter(np=1))
    attempt("columns_2^24", "too large", setter(nx=1 << 13, ny=1 << 11))
    attempt("cells_2^31", "too large", setter(nx=1 << 12, ny=1 << 11, np=1 << 8))
    attempt("in_sy", "strides", setter(sy=1))
    attempt("in_sx", "strides", setter(sx=base.np))
    attempt("out_sy", "strides", out_setter(sy=1))
    attempt("out_sx", "strides", out_setter(sx=base.np))
    attempt("cartesian", "coord_type", setter(coord_type=1))
    for name, v in (("scale_nan", float("nan")), ("scale_inf", float("inf")), ("scale_0", 0.0), ("scale_negative", -5.0)):
        attempt(name, "met_detrend", scale=v)
    attempt("dlon_0", "dlon", axis("lon", 1, float(base.lon[0])))
    attempt("dlon_nan", "dlon", axis("lon", 1, float("nan")))
    attempt("dlat_0", "dlat", axis("lat", 1, float(base.lat[0])))
    attempt("dlat_inf", "dlat", axis("lat", 0, float("inf")))
    attempt("no_field", "none of the fields", fields=("h2o",))


N_REFUSALS = 23


def child_second_thread(rows):
    """The reader thread's call while the first thread steps: the same bits as alone."""
    import threading
    import cases
    from mptrac_amd import hip
    ctl, clim, m0, m1, atm = cases.make_case("advect", n=5000, grid="tiny")
    sim = hip.Simulation(ctl, clim, m0, m1, atm)
    sim.timesteps_init(0.0, 0.0)
    times = cases.step_times(sim.ctl)
    met, scale = K.case("two_workgroups")
    alone = sim.detrend_met(met, scale)
    got, errors = [], []

    def reader():
        try:
            for _ in range(4):
                got.append(sim.detrend_met(met, scale))
        except BaseException as exc:      # noqa: BLE001
            errors.append(repr(exc))

    th = threading.Thread(target=reader)
    sim.run_timestep(times[0])
    th.start()
    k = 1
    while th.is_alive() and k + 4 <= len(times):
        sim.run_timesteps(times[k], 4)
        k += 4
    th.join()
    sim.synchronize()
    state = sim.state()
    sim.close()
    ok = not errors and len(got) == 4 and all(same_bits(g[f], alone[f]) for g in got for f in alone) \
        and bool(np.isfinite(state["lon"]).all())
    rows.append(dict(kind="layout", case=["second_thread"], ok=bool(ok), steps=k, errors=errors))


LAYOUTS = ["again_smallest", "again_widest", "strided", "in_place", "in_place_strided", "only_u", "only_t", "other_slots",
           "second_thread"]


def child():
    from mptrac_amd import hip
    version = hip.load().mphip_version().decode()
    print("library:", version, flush=True)
    sim = bare_context()
    rows = []
    child_cases(sim, rows)
    child_layouts(sim, rows)
    child_refusals(sim, rows)
    sim.close()
    child_second_thread(rows)
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


def test_exact_library_returns_the_restatements_bits(exact_rows):
    rows = _of(exact_rows, "case")
    assert sorted(r["case"][0] for r in rows) == sorted(K.CASES)
    for r in rows:
        assert r["nonfinite_mismatch"] == 0 and r["bits_differ"] == 0 and r["zero_sign"] == 0, r


def test_default_library_within_the_bound(default_rows):
    """Largest share of the bound measured: 0 (no value differs from the restatement's)."""
    rows = _of(default_rows, "case")
    assert sorted(r["case"][0] for r in rows) == sorted(K.CASES)
    print("detrend: largest share of the bound", max(r["share"] for r in rows), "largest float ulp", max(r["max_ulp"] for r in rows))
    for r in rows:
        assert r["nonfinite_mismatch"] == 0 and r["share"] <= 1.0, r


@pytest.mark.parametrize("lib", ["exact", "default"])
def test_layouts_subsets_aliasing_scratch_and_second_thread(lib, exact_rows, default_rows):
    rows = _of(exact_rows if lib == "exact" else default_rows, "layout")
    assert sorted(r["case"][0] for r in rows) == sorted(LAYOUTS)
    for r in rows:
        assert r["ok"], r


@pytest.mark.parametrize("lib", ["exact", "default"])
def test_every_refusal_writes_nothing_and_names_its_cause(lib, exact_rows, default_rows):
    rows = _of(exact_rows if lib == "exact" else default_rows, "refusal")
    assert len(rows) == N_REFUSALS
    for r in rows:
        assert r["ok"] and r["message"].startswith("mphip_detrend_met: "), r


if __name__ == "__main__" and "--child" in sys.argv:
    child()
