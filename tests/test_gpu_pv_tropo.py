"""MPHIP_PREP_PV and MPHIP_PREP_TROPO of mphip_derive_met (through Simulation.derive_met) against tests/reftropo.py, the
restatement of the definitions in include/mptrac_hip.h.

1. Three grids -- 9 x 7 x 20, 37 x 19 x 20 (703 columns: no multiple of a workgroup's columns; 19 rows and 20 levels: no
   multiple of the stencil's tile) and 5 x 5 x 137 (the fewest rows the polar copy admits; 137 levels: the fewest columns per
   workgroup) --, latitudes ascending and descending, compact and as views into arrays of larger extents; met_tropo 1 ... 5
   with the linear and the cubic spline, z and (met_tropo 5) pv given as the restatement's float fields, so that both
   libraries start from the same numbers; met_tropo 4 also on atmosphere2, where some columns have a second tropopause.
   libmptrac_hip_exact.so returns the restatement's float bits, NaNs in the same places.  The default library: the same NaN
   pattern; pt, tt, zt, h2ot within 2 float ulp (the bar of the other derived fields: double results ~1e-13 apart rounded
   to float once, and tests/test_tropo_cpu.py shows that no branch is decided by less than 1e-9); pv within 2 float ulp of
   the restatement plus 32 * 2^-53 * S, S the sum of the magnitudes of the three terms whose sum pv is -- the forward bound
   of that sum's roundings, so that cancellation is not charged to the kernel.  The restatement is computed once, by the
   parent, and handed to the children (one per library) in a file.
2. GEOPOT | PV | TROPO in one call equals three calls that pass z and pv back in, bit for bit (exact library).
3. A bit writes only its outputs, a refused call nothing, and the message names the cause.
4. Calls between time steps do not disturb a run.
5. The LDS limit of the tropopause kernel (1011 levels run, 1012 are refused) and a NaN in a profile.
"""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refmetprep as R      # noqa: E402
import reftropo as T        # noqa: E402
from test_gpu_metprep import bare_context, with_clim, ulp_distance, padding_untouched, SENTINEL      # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS = [(9, 7, 20), (37, 19, 20), (5, 5, 137)]
SEED = 2024
TROPO = ("pt", "tt", "zt", "h2ot")
FIELDS_3 = ("z", "pv")
FIELDS_2 = ("o3c", "pbl", "pct", "pcb", "cl", "plcl", "plfc", "pel", "cape", "cin") + TROPO
# (met_tropo, met_tropo_spline, atmosphere2)
TROPO_CASES = [(mode, method, False) for mode in (1, 2, 3, 4, 5) for method in (0, 1)] + [(4, 0, True), (4, 1, True)]


def case_name(key, second, what):
    return "%dx%dx%d_%d_%d_%s" % (key[0], key[1], key[2], int(key[4]), int(second), what)


def with_fields(met, **f3):
    """The snapshot with further level fields (z, pv)."""
    from mptrac_amd.synth import Met
    view = Met.__new__(Met)
    view.__dict__.update(met.__dict__)
    view.f3 = dict(met.f3, **f3)
    return view


def without(met, *names):
    from mptrac_amd.synth import Met
    view = Met.__new__(Met)
    view.__dict__.update(met.__dict__)
    view.f3 = {k: v for k, v in met.f3.items() if k not in names}
    view.f2 = {k: v for k, v in met.f2.items() if k not in names}
    return view


def sentinel_outputs(met):
    """Every output array of mphip_derive_met with the strides of the snapshot, filled with the sentinel (padding included)."""
    out = {}
    strides = getattr(met, "strides", None)
    for f in FIELDS_3 + FIELDS_2:
        if strides is None:
            out[f] = np.full((met.nx, met.ny, met.np) if f in FIELDS_3 else (met.nx, met.ny), SENTINEL, dtype=np.float32)
        elif f in FIELDS_3:
            out[f] = np.full((met.nx, strides[0] // strides[1], strides[1]), SENTINEL, dtype=np.float32)[:, :met.ny, :met.np]
        else:
            out[f] = np.full((met.nx, strides[2]), SENTINEL, dtype=np.float32)[:, :met.ny]
    return out


def untouched(out, but=()):
    return all((a == SENTINEL).all() for f, a in out.items() if f not in but) and all(padding_untouched(a) for a in out.values())


def given(key, second):
    """The snapshot with the restatement's z and pv as input fields."""
    return with_fields(T.snapshot(key, second), z=T.z_field(key, second), pv=T.pv_reference(key, second)[0])


# ---- the comparison, in a child per library ----------------------------------------------------------------------------

def compare(got, ref, S=None):
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    both = ~nan_g & ~nan_r
    d = ulp_distance(got[both], ref[both])
    s = dict(nan_mismatch=int((nan_g != nan_r).sum()), nan=int(nan_r.sum()), finite=int((~nan_r).sum()),
             bits_differ=int((d != 0).sum()), max_ulp=int(d.max()) if d.size else 0, padding_ok=padding_untouched(got))
    if S is not None:
        g, r = got[both].astype(np.float64), ref[both].astype(np.float64)
        bound = 2. * np.spacing(np.abs(ref[both])).astype(np.float64) + 32. * 2. ** -53 * S[both]
        s["bound_ratio"] = float((np.abs(g - r) / bound).max())
        s["max_abs"] = float(np.abs(g - r).max())
    return s


def child(path):
    from mptrac_amd import hip
    version = hip.load().mphip_version().decode()
    print("library:", version, flush=True)
    exact = "reference rounding" in version
    refs = np.load(path)
    sim = with_clim(bare_context())
    rows = []
    for grid in GRIDS:
        for desc in (False, True):
            key = grid + (SEED, desc)
            for layout in ("compact", "strided"):
                for second in (False, True):
                    met = given(key, second)
                    view = met if layout == "compact" else R.strided(met)
                    where = dict(grid=list(grid), desc=desc, layout=layout, second=second)
                    if not second:
                        out = sentinel_outputs(view)
                        got = sim.derive_met(view, "pv", out=out)
                        assert sorted(got) == ["pv"] and untouched(out, ("pv",))
                        rows.append(dict(where, what="pv", fields=dict(pv=compare(
                            got["pv"], refs[case_name(key, second, "pv")], refs[case_name(key, second, "S")]))))
                    for mode, method, sec in TROPO_CASES:
                        if sec != second:
                            continue
                        out = sentinel_outputs(view)
                        got = sim.derive_met(view, "tropo", out=out, met_tropo=mode, met_tropo_spline=method)
                        assert sorted(got) == sorted(TROPO) and untouched(out, TROPO)
                        name = case_name(key, second, "tropo%d%d" % (mode, method))
                        rows.append(dict(where, what="tropo", mode=mode, method=method,
                                         fields={f: compare(got[f], refs[name + "_" + f]) for f in TROPO}))
    # one call against three: z and pv travel between the kernels on the device, or through the caller's arrays
    fused = []
    if exact:
        for key, layout in (((37, 19, 20, SEED, False), "compact"), ((9, 7, 20, SEED, True), "strided")):
            met = T.snapshot(key)
            for mode in (3, 5):
                view = met if layout == "compact" else R.strided(met)
                one = sim.derive_met(view, ("geopot", "pv", "tropo"), met_tropo=mode)
                z = sim.derive_met(view, "geopot")["z"]
                pv = sim.derive_met(view, "pv")["pv"]
                staged_in = with_fields(met, z=np.ascontiguousarray(z), pv=np.ascontiguousarray(pv))
                staged = sim.derive_met(staged_in if layout == "compact" else R.strided(staged_in), "tropo", met_tropo=mode)
                same = np.array_equal(one["z"], z) and np.array_equal(one["pv"].view(np.uint32), pv.view(np.uint32)) and all(
                    np.array_equal(one[f].view(np.uint32), staged[f].view(np.uint32)) for f in TROPO)
                fused.append(dict(grid=list(key[:3]), layout=layout, mode=mode, same=bool(same),
                                  finite=int(np.isfinite(one["pt"]).sum())))
    sim.close()
    print("JSON " + json.dumps(dict(rows=rows, fused=fused)))


@pytest.fixture(scope="module")
def reference_file(tmp_path_factory):
    """The restatement of every compared case, once: {case name: array}."""
    arrays = {}
    for grid in GRIDS:
        for desc in (False, True):
            key = grid + (SEED, desc)
            arrays[case_name(key, False, "pv")], arrays[case_name(key, False, "S")] = T.pv_reference(key)
            for mode, method, second in TROPO_CASES:
                ref, _ = T.tropo_reference(key, mode, method, second)
                for f in TROPO:
                    arrays[case_name(key, second, "tropo%d%d" % (mode, method)) + "_" + f] = ref[f]
    path = str(tmp_path_factory.mktemp("reftropo") / "ref.npz")
    np.savez(path, **arrays)
    return path


def _run_child(exact, path):
    env = dict(os.environ, MPTRAC_AMD_EXACT="1" if exact else "0")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], capture_output=True, text=True,
                         timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert ("reference rounding" in lib) == exact, lib
    got = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("JSON ")][0][5:])
    assert len(got["rows"]) == len(GRIDS) * 2 * 2 * (1 + len(TROPO_CASES))
    return got


@pytest.fixture(scope="module")
def exact_rows(reference_file):
    return _run_child(True, reference_file)


@pytest.fixture(scope="module")
def fast_rows(reference_file):
    return _run_child(False, reference_file)


def _of_grid(got, grid):
    mine = [r for r in got["rows"] if tuple(r["grid"]) == grid]
    assert len(mine) == 2 * 2 * (1 + len(TROPO_CASES))
    return mine


def _where(r):
    return {k: r[k] for k in ("desc", "layout", "second", "what", "mode", "method") if k in r}


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_reference_rounding_library_returns_the_restatements_bits(exact_rows, grid):
    for r in _of_grid(exact_rows, grid):
        for f, s in r["fields"].items():
            print(grid, _where(r), f, s)
            assert s["nan_mismatch"] == 0 and s["bits_differ"] == 0 and s["padding_ok"], (_where(r), f, s)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_default_library_tropopause_within_two_float_ulp(fast_rows, grid):
    for r in _of_grid(fast_rows, grid):
        if r["what"] != "tropo":
            continue
        for f, s in r["fields"].items():
            print(grid, _where(r), f, s)
            assert s["nan_mismatch"] == 0 and s["max_ulp"] <= 2 and s["padding_ok"], (_where(r), f, s)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_default_library_pv_within_the_forward_bound_of_its_sum(fast_rows, grid):
    """|got - ref| <= 2 float ulp of ref + 32 * 2^-53 * S.  Measured on the MI355X (largest over layouts and latitude
    orders, all three grids): distance 0 float ulp, |got - ref| / bound 0 -- the default library returned the restatement's
    bits."""
    for r in _of_grid(fast_rows, grid):
        if r["what"] != "pv":
            continue
        s = r["fields"]["pv"]
        print(grid, _where(r), "pv: largest distance %d float ulp, |got - ref| <= %.3g, at most %.3g of the bound"
              % (s["max_ulp"], s["max_abs"], s["bound_ratio"]))
        assert s["nan_mismatch"] == 0 and s["nan"] == 0 and s["bound_ratio"] <= 1.0 and s["padding_ok"], (_where(r), s)


def test_one_call_equals_three_staged_calls(exact_rows):
    assert len(exact_rows["fused"]) == 4
    for r in exact_rows["fused"]:
        assert r["same"] and r["finite"] > 0, r


def test_the_comparison_sees_nan_and_values(exact_rows):
    """Not vacuous: the compared fields hold the restatement's numbers of finite values and NaNs, both where
    tests/test_tropo_cpu.py says both occur (a second tropopause in atmosphere2; the cold point on 37 x 19 x 20), no NaN in
    pv and in the WMO and dynamical tropopause."""
    for grid in GRIDS:
        for r in _of_grid(exact_rows, grid):
            if r["desc"] or r["layout"] != "compact":
                continue
            key = grid + (SEED, False)
            if r["what"] == "pv":
                assert r["fields"]["pv"]["nan"] == 0 and r["fields"]["pv"]["finite"] == grid[0] * grid[1] * grid[2]
                continue
            ref, _ = T.tropo_reference(key, r["mode"], r["method"], r["second"])
            for f in TROPO:
                s = r["fields"][f]
                assert s["nan"] == int(np.isnan(ref[f]).sum()) and s["finite"] == int(np.isfinite(ref[f]).sum()), (_where(r), f)
            n, ncol = r["fields"]["pt"]["nan"], grid[0] * grid[1]
            if r["mode"] == 4 and r["second"]:
                assert 0 < n < ncol, _where(r)
            if r["mode"] == 2 and grid == (37, 19, 20):
                assert 0 < n < ncol, _where(r)
            if r["mode"] in (1, 3, 5):
                assert n == 0, _where(r)


# ---- bits and refusals (the library this process loads) ------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim():
    s = with_clim(bare_context())
    yield s
    s.close()


KEY = (9, 7, 20, SEED, False)


@pytest.mark.parametrize("bit,fields", [("pv", ("pv",)), ("tropo", TROPO)])
@pytest.mark.parametrize("layout", ["compact", "strided"])
def test_one_bit_writes_only_its_outputs(sim, bit, fields, layout):
    met = given(KEY, False)
    view = met if layout == "compact" else R.strided(met)
    out = sentinel_outputs(view)
    got = sim.derive_met(view, bit, out=out)
    assert sorted(got) == sorted(fields) and untouched(out, fields)
    for f in fields:
        assert np.isfinite(out[f]).all() and (out[f] != SENTINEL).all(), f


def _raw_call(sim, met, bits, outputs, **opts):
    """mphip_derive_met with exactly the output arrays `outputs` (derive_met itself always provides those of a requested bit)."""
    from mptrac_amd import hip
    o = hip.MphipPrep(3, 0.1, 5.0, -1, -1, 0.0, int(opts.get("met_tropo", 3)), 3.5, 380., 1)
    m = sim._met_struct(met)
    mo = hip.MphipMetOut()
    for f, a in outputs.items():
        if f in hip.FIELDS_3D:
            mo.f3[hip.FIELDS_3D.index(f)] = hip._ptr(a, hip._fp)
        else:
            mo.f2[hip.FIELDS_2D.index(f)] = hip._ptr(a, hip._fp)
    rc = sim.L.mphip_derive_met(sim.h, C.byref(m), bits, C.byref(o), C.byref(mo))
    return rc, sim.L.mphip_last_error(sim.h).decode()


def _cartesian(met):
    view = with_fields(met)
    view.coord_type = 1
    return view


def _sliced(met, nx=None, ny=None, n=None):
    from mptrac_amd.synth import Met
    sx, sy, sp = slice(0, nx), slice(0, ny), slice(0, n)
    return Met(met.time, met.lon[sx], met.lat[sy], met.p[sp], {k: v[sx, sy, sp] for k, v in met.f3.items()},
               {k: v[sx, sy] for k, v in met.f2.items()})


# (bit, how the snapshot is changed, options, what the message must say)
REFUSALS = [
    ("pv", lambda m: without(m, "u"), {}, "MPHIP_PREP_PV needs the fields t, u, v"),
    ("pv", lambda m: without(m, "t"), {}, "MPHIP_PREP_PV needs the fields t, u, v"),
    ("pv", _cartesian, {}, "coord_type 0"),
    ("pv", lambda m: _sliced(m, ny=4), {}, "ny < 5"),
    ("pv", lambda m: _sliced(m, nx=1), {}, "grid dimensions out of range"),
    ("tropo", lambda m: without(m, "h2o"), {}, "MPHIP_PREP_TROPO needs the fields t, h2o and z"),
    ("tropo", lambda m: without(m, "t"), {}, "MPHIP_PREP_TROPO needs the fields t, h2o and z"),
    ("tropo", lambda m: without(m, "z"), {}, "MPHIP_PREP_TROPO needs the fields t, h2o and z"),
    ("tropo", lambda m: without(m, "pv"), dict(met_tropo=5), "met_tropo 5 needs the fields pv"),
    ("tropo", None, dict(met_tropo=0), "met_tropo must be"),
    ("tropo", None, dict(met_tropo=6), "met_tropo must be"),
    ("tropo", None, dict(met_tropo_spline=2), "met_tropo_spline must be"),
    ("tropo", None, dict(met_tropo_spline=-1), "met_tropo_spline must be"),
    ("tropo", lambda m: _sliced(m, n=2), dict(met_tropo=2), "np < 3"),
    ("tropo", lambda m: _sliced(m, n=2), dict(met_tropo=3), "np < 3"),
    ("tropo", lambda m: _sliced(m, n=2), dict(met_tropo=4), "np < 3"),
    ("tropo", lambda m: _sliced(m, n=2), dict(met_tropo=5), "np < 3"),
    ("tropo", _cartesian, dict(met_tropo=1), "met_utm_ref_lat"),
]


@pytest.mark.parametrize("bit,change,opts,cause", REFUSALS, ids=["%s-%d" % (r[0], i) for i, r in enumerate(REFUSALS)])
def test_refused_calls_write_nothing_and_name_the_cause(sim, bit, change, opts, cause):
    import re
    from mptrac_amd.hip import MphipError
    met = given(KEY, False)
    view = change(met) if change else met
    out = sentinel_outputs(view)
    with pytest.raises(MphipError, match="mphip_derive_met.*" + re.escape(cause)):
        sim.derive_met(view, bit, out=out, **opts)
    assert untouched(out)


def test_two_levels_are_enough_for_the_climatological_tropopause(sim):
    two = _sliced(given(KEY, False), n=2)
    got = sim.derive_met(two, "tropo", met_tropo=1)
    assert np.isfinite(got["pt"]).all()


@pytest.mark.parametrize("bit,leave_out,cause", [("pv", "pv", "needs the output array pv")]
                         + [("tropo", f, "needs the output arrays pt, tt, zt, h2ot") for f in TROPO])
def test_a_missing_output_array_is_refused(sim, bit, leave_out, cause):
    from mptrac_amd import hip
    met = given(KEY, False)
    out = sentinel_outputs(met)
    rc, msg = _raw_call(sim, met, hip.PREP[bit], {f: a for f, a in out.items() if f != leave_out})
    assert rc != 0 and cause in msg, msg
    assert untouched(out)


def _tall(n):
    """2 x 2 columns on n levels from 1000 to 1 hPa: 6.5 K/km to a tropopause at 10.05 ... 13.05 km, isothermal above."""
    from mptrac_amd.synth import Met
    p = 1000. * np.exp(-np.arange(n) * (math.log(1000.) / (n - 1)))
    zlev = 7. * np.log(1013.25 / p)
    ztrop = np.array([[10.05, 11.05], [12.05, 13.05]])
    t = 290. - 6.5 * np.minimum(zlev[None, None, :], ztrop[:, :, None])
    h2o = np.maximum(1e-2 * np.exp(-zlev / 2.), 3e-6)[None, None, :] * np.ones((2, 2, 1))
    z = zlev[None, None, :] * np.ones((2, 2, 1))
    return Met(0., [0., 1.], [10., 11.], p, dict(t=t, h2o=h2o, z=z), dict(ps=np.full((2, 2), 1000.)))


def test_the_lds_limit_of_the_tropopause_kernel(sim):
    """met_tropo 3 / 4 keep 60 np + 4824 bytes of LDS for the axis tables and one column: 1011 levels fit 64 KB (one column
    per workgroup, the restatement's result), 1012 are refused; the cold point, without the fine profile, still takes them."""
    from mptrac_amd.hip import MphipError
    met = _tall(1011)
    got = sim.derive_met(met, "tropo", met_tropo=3)
    p = met.p.tolist()
    zc = [T.Z(x) for x in p]
    for ix in range(2):
        for iy in range(2):
            m = T.Margin()
            pt = T.tropo_pt(3, 1, zc, p, met.f3["t"][ix, iy].astype(np.float64).tolist(), None, m)
            want = [pt] + [T.env(p, met.f3[f][ix, iy].astype(np.float64).tolist(), pt, m) for f in ("t", "z", "h2o")]
            assert math.isfinite(pt) and m.value >= 1e-9
            for f, w in zip(TROPO, want):
                assert ulp_distance(got[f][ix, iy:iy + 1], np.array([w], dtype=np.float32)).max() <= 2, (ix, iy, f)
    met = _tall(1012)
    for mode in (3, 4):
        out = sentinel_outputs(met)
        with pytest.raises(MphipError, match="too many pressure levels for one column in 64 KB of LDS"):
            sim.derive_met(met, "tropo", out=out, met_tropo=mode)
        assert untouched(out)
    assert np.isfinite(sim.derive_met(met, "tropo", met_tropo=2)["pt"]).all()


@pytest.mark.parametrize("mode,method", [(2, 1), (3, 1), (3, 0), (4, 1), (5, 1), (5, 0)])
def test_a_nan_in_a_profile_makes_that_columns_tropopause_nan(sim, mode, method):
    """A NaN temperature at 8.9 km in one column: the fine values every mode looks at hold a NaN there (through the cubic
    spline's coefficients everywhere, through the linear one in the two intervals around the level), so pt, tt, zt, h2ot of
    that column are NaN; every other column keeps the restatement's value (met_tropo 4 on atmosphere2, where some have one)."""
    second = mode == 4
    met = given(KEY, second)
    t = met.f3["t"].copy()
    ix, iy = 3, 4
    t[ix, iy, 4] = np.nan
    got = sim.derive_met(with_fields(met, t=t), "tropo", met_tropo=mode, met_tropo_spline=method)
    ref, _ = T.tropo_reference(KEY, mode, method, second)
    p = met.p.tolist()
    assert math.isnan(T.tropo_pt(mode, method, [T.Z(x) for x in p], p, t[ix, iy].astype(np.float64).tolist(),
                                 met.f3["pv"][ix, iy].astype(np.float64).tolist(), T.Margin()))
    others = np.ones((met.nx, met.ny), dtype=bool)
    others[ix, iy] = False
    for f in TROPO:
        assert np.isnan(got[f][ix, iy]), f
        assert np.array_equal(np.isnan(got[f][others]), np.isnan(ref[f][others])), f
        both = others & ~np.isnan(ref[f])
        assert both.any()
        assert ulp_distance(got[f][both], ref[f][both]).max() <= 2, f


def test_the_climatological_tropopause_needs_the_climatology():
    from mptrac_amd.hip import MphipError
    met = given(KEY, False)
    fresh = bare_context()
    try:
        out = sentinel_outputs(met)
        with pytest.raises(MphipError, match="mphip_update_clim"):
            fresh.derive_met(met, "tropo", out=out, met_tropo=1)
        assert untouched(out)
        assert np.isfinite(fresh.derive_met(met, "tropo")["pt"]).all()      # the other definitions do not need it
    finally:
        fresh.close()


# ---- a run is not disturbed -------------------------------------------------------------------------------------------------

def test_calls_between_time_steps_do_not_disturb_a_run():
    """Twenty steps of the case "full" with a derive_met call (GEOPOT | PV | TROPO, every met_tropo in turn) between the
    steps end with the bits of the run without."""
    import cases
    from mptrac_amd.hip import Simulation
    met = R.atmosphere(37, 19, 20, SEED, False)
    states = []
    for derive in (False, True):
        ctl, clim, met0, met1, atm = cases.make_case("full", n=2000, grid="tiny")
        run = Simulation(ctl, clim, met0, met1, atm)
        try:
            cases.prepare(run)
            tmin, tmax = float(atm["time"].min()), float(atm["time"].max())
            run.timesteps_init(tmin, tmax)
            for k, t in enumerate(cases.step_times(run.ctl)[:20]):
                run.run_timestep(t)
                if derive:
                    mode = 1 + k % 5
                    got = run.derive_met(met, ("geopot", "pv", "tropo"), met_tropo=mode)
                    # (this atmosphere has no second tropopause: tests/test_tropo_cpu.py)
                    assert np.isfinite(got["pv"]).all() and np.isfinite(got["pt"]).any() == (mode != 4)
            states.append(run.state())
        finally:
            run.close()
    a, b = states
    for k in ("time", "lon", "lat", "p", "q", "uvwp"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


if __name__ == "__main__" and "--child" in sys.argv:
    child(sys.argv[sys.argv.index("--child") + 1])
