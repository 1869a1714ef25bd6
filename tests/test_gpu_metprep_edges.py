"""mphip_derive_met on the edge snapshots of tests/metprep_cases.py against the restatement (tests/refmetprep.py,
tests/reftropo.py): surfaces ON pressure levels and one float ulp beside them, the 300 hPa stop of PBL 3, cloud water AT
met_cloud_min, axes of 3 and 4 levels and axes that begin above or end below the tropopause search, 600 and 1819 levels
(4, 8, 16 and 1 columns per workgroup; 1820 refused), level counts around the potential vorticity's tile of 32, the largest
smoothing tile and half-widths beyond the grid, a Cartesian grid with met_utm_ref_lat, non-default met_pbl_min / _max /
met_cloud_min, and NaN, infinities, 0 and negative values in ps, t, h2o, ts, zs.

One child per library and step; the restatement is computed once, by the parent, and handed over in a file; JSON rows come
back.  libmptrac_hip_exact.so returns the restatement's float bits: NaNs in the same places, infinities equal in sign,
padding of strided outputs untouched.  The default library is held to the project's existing bars: the same NaN / inf
pattern, every finite value within 2 float ulp, pv within 2 float ulp plus 32 * 2^-53 * S (tests/test_gpu_pv_tropo.py);
tests/test_metprep_edges_cpu.py shows that on the finite inputs no comparison between computed values is decided by less
than 1e-9.  Refused calls write nothing and name the cause.

The step "nonfinite" (smooth_shapes -- whose snapshots hold NaN levels -- and nonfinite) runs last, in children of its
own under their own time limit; after a child that died or ran out of time no further child is started.  Why its kernels
end on every listed input (read against prep_geopot_kernel, prep_cape_kernel, prep_pbl_kernel, prep_tropo_kernel):
  * every level loop (prep_loc's walk, the geopotential recurrences, the ozone and cloud sums, the parcel's mean, both PBL
    searches, the spline's solve and walk) counts an index up or down to a bound that is np - 1, np - 2 or 0, whatever the
    values are; the tropopause searches count a fine-grid index up to 170 and look at most 20 points (index 190 of 201)
    ahead.  loc(NaN) = 0 and loc(q <= 0) = np - 2: both inside the column.
  * the bisection of the lifted condensation level halves [ptop, pbot] with ptop = P(20) finite.  ps is taken as NaN when
    it is infinite, so pbot is finite or NaN.  Finite: whichever end moves, pbot - ptop halves and falls below 0.1 (a NaN
    in theta or h2o makes the humidity test false, which moves pbot: it still halves).  NaN: plcl is NaN, pbot becomes NaN,
    `pbot - ptop > 0.1` is false: one pass.  ps <= 0 takes no level into the parcel: the loops are not entered.
  * the two ascents divide p by pfac > 1 per pass and end when p <= plcl resp. p <= 0.75 clim_tropo (finite and positive,
    from the table and the column's latitude, never from the column's values; the kernel also ends at p <= 0); p starts at
    ps resp. plcl, finite, or NaN, which makes `p > ...` false: one pass.  NaN in t, h2o only enters d, cape, cin.
  * log, exp, pow of the device library mask their table indices (& 127) and return on zero, negative, infinite and NaN
    arguments before any table is read.
No huge finite ps is among the inputs: it is no edge of the definition and only lengthens the ascent.

Measured on the MI355X (profiles/metprep_edges.json): both libraries, every family: largest distance 0 float ulp, pv at 0 of
its bound, 135 299 finite values compared per library.  profiles/metprep_edges_breaks.txt: which of these tests fail on
eleven one-token breaks of the kernels.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import metprep_cases as C       # noqa: E402
import refmetprep as R          # noqa: E402
from test_gpu_metprep import bare_context, with_clim, ulp_distance, padding_untouched, SENTINEL      # noqa: E402
from test_gpu_pv_tropo import sentinel_outputs      # noqa: E402

pytestmark = pytest.mark.gpu

STEPS = ("finite", "nonfinite")
TIME_LIMIT = {"finite": 300, "nonfinite": 120}      # seconds per child; each takes a few
FAMILIES = {"finite": ("levels_era5", "short_axes", "tall_axes", "pv_shapes", "cartesian", "options"),
            "nonfinite": ("smooth_shapes", "nonfinite")}


def with_ref_lat(sim, lat):
    """mphip_update_ctl with met_utm_ref_lat (all else default)."""
    from mptrac_amd import hip
    sim.ctl = hip.fill_ctl(hip.MphipCtl(), met_coord_type=1, met_utm_ref_lat=lat)
    sim.update_ctl()
    return sim


def compare(got, ref, S=None):
    nan_g, nan_r, inf_g, inf_r = np.isnan(got), np.isnan(ref), np.isinf(got), np.isinf(ref)
    with np.errstate(invalid="ignore"):
        wrong = (nan_g != nan_r) | (inf_g != inf_r) | (inf_g & inf_r & (got != ref))
    both = np.isfinite(got) & np.isfinite(ref)
    d = ulp_distance(got[both], ref[both])
    s = dict(pattern_mismatch=int(wrong.sum()), nan=int(nan_r.sum()), inf=int(inf_r.sum()), finite=int(both.sum()),
             bits_differ=int((d != 0).sum()), max_ulp=int(d.max()) if d.size else 0, padding_ok=padding_untouched(got))
    if S is not None:
        both &= np.isfinite(S)
        g, r = got[both].astype(np.float64), ref[both].astype(np.float64)
        bound = 2. * np.spacing(np.abs(ref[both])).astype(np.float64) + 32. * 2. ** -53 * S[both]
        s["bound_ratio"] = float((np.abs(g - r) / bound).max()) if g.size else 0.0
    return s


def untouched(out, but=()):
    return all((a == SENTINEL).all() for f, a in out.items() if f not in but) and all(padding_untouched(a) for a in out.values())


def child(step, path):
    from mptrac_amd import hip
    print("library:", hip.load().mphip_version().decode(), flush=True)
    refs = np.load(path)
    sim = with_clim(bare_context())
    cart = with_ref_lat(with_clim(bare_context()), C.REF_LAT)
    rows = []
    for i, call in enumerate(C.calls(step)):
        if call["given"]:
            met = C.given(call["met"], pv="pv" not in call["what"] and call["opts"].get("met_tropo") == 5)
        else:
            met = C.snapshot(call["met"])
        view = R.strided(met) if call["strided"] else met
        out = sentinel_outputs(view)
        ctx = cart if call["ref_lat"] is not None else sim
        row = dict(id=call["id"], family=call["family"], fields={})
        fields = [f for b in call["what"] for f in C.BIT_FIELDS[b]]
        try:
            got = ctx.derive_met(view, call["what"], out=out, **call["opts"])
        except hip.MphipError as e:
            row.update(refused=str(e), untouched=untouched(out))
        else:
            assert sorted(got) == sorted(fields)
            row.update(refused=None, untouched=untouched(out, fields))
            for f in fields:
                S = refs["%d_S" % i] if f == "pv" else None
                row["fields"][f] = compare(got[f], refs["%d_%s" % (i, f)], S)
        rows.append(row)
        print("done", call["id"], flush=True)
    sim.close()
    cart.close()
    print("JSON " + json.dumps(rows))


@pytest.fixture(scope="module")
def reference_files(tmp_path_factory):
    """The restatement of every call, once: per step a file {"<index of the call>_<field>": array}."""
    paths = {}
    for step in STEPS:
        arrays = {}
        for i, call in enumerate(C.calls(step)):
            if not call["refused"]:
                for f, a in C.expected(call).items():
                    arrays["%d_%s" % (i, f)] = a
        paths[step] = str(tmp_path_factory.mktemp("refedges") / (step + ".npz"))
        np.savez(paths[step], **arrays)
    return paths


_STOP = {}       # set by a child that died or ran out of time: nothing more is started on the device
_ROWS = {}


def _run_child(step, exact, path):
    if _STOP:
        pytest.fail("not run: an earlier child ended abnormally (%s)" % _STOP["why"])
    env = dict(os.environ, MPTRAC_AMD_EXACT="1" if exact else "0")
    env.pop("MPHIP_LIB", None)
    try:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, path], capture_output=True,
                             text=True, timeout=TIME_LIMIT[step], env=env, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _STOP["why"] = "%s child over its time limit after: %s" % (step, (e.stdout or b"")[-300:])
        raise
    if res.returncode != 0:
        if res.returncode < 0 or res.returncode in (124, 134, 137, 139) or "illegal memory access" in res.stderr:
            _STOP["why"] = "%s child: exit status %d" % (step, res.returncode)
        raise AssertionError(res.stdout[-2000:] + res.stderr[-3000:])
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert ("reference rounding" in lib) == exact, lib
    rows = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("JSON ")][0][5:])
    assert [r["id"] for r in rows] == [c["id"] for c in C.calls(step)]
    _ROWS[(step, exact)] = rows
    return rows


@pytest.fixture(scope="module")
def exact_finite(reference_files):
    return _run_child("finite", True, reference_files["finite"])


@pytest.fixture(scope="module")
def fast_finite(reference_files):
    return _run_child("finite", False, reference_files["finite"])


@pytest.fixture(scope="module")
def exact_nonfinite(reference_files):
    return _run_child("nonfinite", True, reference_files["nonfinite"])


@pytest.fixture(scope="module")
def fast_nonfinite(reference_files):
    return _run_child("nonfinite", False, reference_files["nonfinite"])


def _family(rows, family):
    mine = [r for r in rows if r["family"] == family and r["refused"] is None]
    assert mine, family
    return mine


def _assert_bits(rows, family):
    for r in _family(rows, family):
        assert r["untouched"], r["id"]
        for f, s in r["fields"].items():
            print(r["id"], f, s)
            assert s["pattern_mismatch"] == 0 and s["bits_differ"] == 0 and s["padding_ok"], (r["id"], f, s)


def _assert_bars(rows, family):
    for r in _family(rows, family):
        assert r["untouched"], r["id"]
        for f, s in r["fields"].items():
            print(r["id"], f, s)
            assert s["pattern_mismatch"] == 0 and s["padding_ok"], (r["id"], f, s)
            if f == "pv":
                assert s["bound_ratio"] <= 1.0, (r["id"], s)
            else:
                assert s["max_ulp"] <= 2, (r["id"], f, s)


def _assert_refusals(rows, step):
    want = [c for c in C.calls(step) if c["refused"]]
    assert want
    for c in want:
        r = next(r for r in rows if r["id"] == c["id"])
        assert r["refused"] and "mphip_derive_met" in r["refused"] and c["refused"] in r["refused"], r
        assert r["untouched"], r["id"]
    assert all(r["refused"] is None for r in rows if r["id"] not in {c["id"] for c in want})


def worst_by_family(rows):
    out = {}
    for r in rows:
        w = out.setdefault(r["family"], dict(max_ulp=0, pv_bound_ratio=0.0, values=0))
        for s in r["fields"].values():
            w["max_ulp"] = max(w["max_ulp"], s["max_ulp"])
            w["pv_bound_ratio"] = max(w["pv_bound_ratio"], s.get("bound_ratio", 0.0))
            w["values"] += s["finite"]
    return out


# ---- step "finite" ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES["finite"])
def test_reference_rounding_library_returns_the_restatements_bits(exact_finite, family):
    _assert_bits(exact_finite, family)


@pytest.mark.parametrize("family", FAMILIES["finite"])
def test_default_library_within_the_existing_bars(fast_finite, family):
    """Measured on the MI355X, largest over the calls of a family: 0 float ulp in every family, pv at 0 of its bound
    (profiles/metprep_edges.json)."""
    _assert_bars(fast_finite, family)


def test_too_many_levels_are_refused_and_write_nothing(exact_finite, fast_finite):
    n = C.level_limit()
    assert C.snapshot("tall_limit").np == n and C.snapshot("tall_beyond").np == n + 1
    for rows in (exact_finite, fast_finite):
        _assert_refusals(rows, "finite")
        ran = [r for r in rows if "|tall_limit|" in r["id"]]
        assert len(ran) == 1 and ran[0]["refused"] is None and ran[0]["fields"]["z"]["finite"] == 6 * n


def test_the_comparison_sees_values_nan_and_both_layouts(exact_finite):
    """Not vacuous: finite values and NaNs side by side where the restatement has both; strided calls among them."""
    era5 = [r for r in _family(exact_finite, "levels_era5") if "|geopot+" in r["id"]]
    assert len(era5) == 4 and sum("strided" in r["id"] for r in era5) == 2
    for r in era5:
        assert 0 < r["fields"]["pct"]["nan"] < 63 and r["fields"]["pbl"]["finite"] == 63 and 0 < r["fields"]["pel"]["finite"] < 63
    assert sum(r["fields"]["pt"]["finite"] for r in _family(exact_finite, "short_axes")) > 0
    assert sum(r["fields"]["pt"]["nan"] for r in _family(exact_finite, "short_axes")) > 0
    assert all(r["fields"]["pv"]["finite"] > 0 and r["fields"]["pv"]["nan"] == 0 for r in _family(exact_finite, "pv_shapes"))
    assert sum("strided" in r["id"] for r in _family(exact_finite, "pv_shapes")) == len(_family(exact_finite, "pv_shapes")) // 2


# ---- step "nonfinite": last, on its own ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES["nonfinite"])
def test_reference_rounding_library_returns_the_restatements_bits_on_nonfinite_inputs(exact_finite, fast_finite, exact_nonfinite,
                                                                                      family):
    _assert_bits(exact_nonfinite, family)


@pytest.mark.parametrize("family", FAMILIES["nonfinite"])
def test_default_library_within_the_existing_bars_on_nonfinite_inputs(exact_finite, fast_finite, exact_nonfinite,
                                                                      fast_nonfinite, family):
    """The NaN / inf pattern matches everywhere; the bars apply to the values that are finite in both."""
    _assert_bars(fast_nonfinite, family)


def test_smoothing_beyond_the_tile_or_the_grid_is_refused(exact_nonfinite, fast_nonfinite):
    for rows in (exact_nonfinite, fast_nonfinite):
        _assert_refusals(rows, "nonfinite")


def test_nonfinite_results_hold_nan_infinities_and_values(exact_nonfinite):
    z = [r for r in _family(exact_nonfinite, "nonfinite") if "|geopot+" in r["id"]]
    assert len(z) == 4
    for r in z:
        s = r["fields"]["z"]
        assert s["nan"] > 0 and s["finite"] > 0 and (s["inf"] > 0) == ("sx0" in r["id"])      # the smoothing skips -inf
    for r in _family(exact_nonfinite, "smooth_shapes"):
        assert r["fields"]["z"]["nan"] > 0 and r["fields"]["z"]["finite"] > 0


def test_record_the_worst_distances():
    """With METPREP_EDGES_PROFILE=<file>: the worst distances per family of the children that ran, as JSON."""
    path = os.environ.get("METPREP_EDGES_PROFILE")
    if path and _ROWS:
        doc = {("exact" if exact else "default") + "/" + step: worst_by_family(rows) for (step, exact), rows in _ROWS.items()}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__" and "--child" in sys.argv:
    child(sys.argv[-2], sys.argv[-1])
