"""mphip_derive_met (through Simulation.derive_met) against tests/refmetprep.py, the per-column restatement of the
definitions in include/mptrac_hip.h.

1. Three grids -- 9 x 7 x 20, 37 x 19 x 20 (703 columns: no multiple of a workgroup's columns, with the periodic column)
   and 5 x 4 x 137 -- compact and as views into arrays of larger extents (sy = np + 5, sx = (ny + 3) sy, sx2 = ny + 3),
   latitudes ascending and descending, met_pbl 2 and 3, smoothing automatic, off and 2 / 1.  libmptrac_hip_exact.so
   returns the reference's float bits, NaNs in the same places; the default library the same NaN pattern and every
   finite value within 2 float ulp -- the double results differ by ~1e-13 relative and are rounded to float once (one
   ulp), and smoothing inputs one ulp apart gives one more.  That also pins the ladder step of plfc and pel: neighbouring
   steps are 1.4 % apart.  tests/test_metprep_cpu.py checks that no branch of the reference is decided by less than 1e-9,
   so nothing is left out.  A process loads one library: each runs in a child (as tests/test_gpu_exact_library.py does).
2. Each bit alone leaves the outputs of the other bits alone, a refused call all of them.
3. Calls between time steps do not disturb a run.
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

import refmetprep as R      # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS = [(9, 7, 20), (37, 19, 20), (5, 4, 137)]
SMOOTHING = [(-1, -1), (0, 0), (2, 1)]
FIELDS = ("z", "o3c", "pbl", "pct", "pcb", "cl", "plcl", "plfc", "pel", "cape", "cin")
ALL = ("geopot", "o3c", "pbl", "cloud", "cape")
SENTINEL = np.float32(-7777.)


def bare_context():
    """A context with nothing uploaded (no control parameters, no climatology, no particles)."""
    import ctypes as C
    from mptrac_amd import hip
    sim = object.__new__(hip.Simulation)
    sim.L = hip.load()
    sim.h = C.c_void_p()
    assert sim.L.mphip_create(C.byref(sim.h), 0) == 0
    return sim


def with_clim(sim):
    from mptrac_amd import hip
    from mptrac_amd.clim import load_clim_tropo
    time, lat, tropo = load_clim_tropo()
    tropo = np.ascontiguousarray(tropo)
    sim._chk(sim.L.mphip_update_clim(sim.h, len(time), len(lat), hip._ptr(time, hip._dp), hip._ptr(lat, hip._dp),
                                     hip._ptr(tropo, hip._dp), tropo.shape[1]))
    return sim


def ulp_distance(a, b):
    """Distance in float32 steps between finite values (elementwise)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def sentinel_outputs(met):
    """All eleven output arrays with the strides of the snapshot, filled with the sentinel (padding included)."""
    out = {}
    strides = getattr(met, "strides", None)
    for f in FIELDS:
        if strides is None:
            out[f] = np.full((met.nx, met.ny, met.np) if f == "z" else (met.nx, met.ny), SENTINEL, dtype=np.float32)
        elif f == "z":
            out[f] = np.full((met.nx, strides[0] // strides[1], strides[1]), SENTINEL, dtype=np.float32)[:, :met.ny, :met.np]
        else:
            out[f] = np.full((met.nx, strides[2]), SENTINEL, dtype=np.float32)[:, :met.ny]
    return out


def padding_untouched(a):
    if a.base is None:
        return True
    big = a.base.copy()
    big[tuple(slice(0, n) for n in a.shape)] = SENTINEL
    return bool((big == SENTINEL).all())


# ---- the comparison, in a child per library ----------------------------------------------------------------------------

def child():
    from mptrac_amd import hip
    print("library:", hip.load().mphip_version().decode(), flush=True)
    sim = with_clim(bare_context())
    rows = []
    for nx, ny, n in GRIDS:
        for desc in (False, True):
            key = (nx, ny, n, 2024, desc)
            met = R.atmosphere(*key)
            for layout in ("compact", "strided"):
                view = met if layout == "compact" else R.strided(met)
                for met_pbl in (3, 2):
                    for sx, sy in SMOOTHING:
                        ref, _ = R.reference(key, met_pbl, sx, sy)
                        out = sentinel_outputs(view)
                        got = sim.derive_met(view, ALL, out=out, met_pbl=met_pbl, met_geopot_sx=sx, met_geopot_sy=sy)
                        row = dict(grid=[nx, ny, n], desc=desc, layout=layout, met_pbl=met_pbl, smooth=[sx, sy], fields={})
                        assert sorted(got) == sorted(FIELDS)
                        for f in FIELDS:
                            g, r = got[f], ref[f]
                            nan_g, nan_r = np.isnan(g), np.isnan(r)
                            both = ~nan_g & ~nan_r
                            d = ulp_distance(g[both], r[both])
                            row["fields"][f] = dict(nan_mismatch=int((nan_g != nan_r).sum()), nan=int(nan_r.sum()),
                                                    bits_differ=int((d != 0).sum()), max_ulp=int(d.max()) if d.size else 0,
                                                    padding_ok=padding_untouched(g))
                        rows.append(row)
    sim.close()
    print("JSON " + json.dumps(rows))


def _run_child(exact):
    env = dict(os.environ, MPTRAC_AMD_EXACT="1" if exact else "0")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=600,
                         env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert ("reference rounding" in lib) == exact, lib
    rows = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("JSON ")][0][5:])
    assert len(rows) == len(GRIDS) * 2 * 2 * 2 * len(SMOOTHING)
    return rows


@pytest.fixture(scope="module")
def exact_rows():
    return _run_child(True)


@pytest.fixture(scope="module")
def fast_rows():
    return _run_child(False)


def _of_grid(rows, grid):
    mine = [r for r in rows if tuple(r["grid"]) == grid]
    assert len(mine) == 2 * 2 * 2 * len(SMOOTHING)
    return mine


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_reference_rounding_library_returns_the_references_bits(exact_rows, grid):
    for r in _of_grid(exact_rows, grid):
        where = {k: r[k] for k in ("desc", "layout", "met_pbl", "smooth")}
        for f, s in r["fields"].items():
            print(grid, where, f, s)
            assert s["nan_mismatch"] == 0 and s["bits_differ"] == 0 and s["padding_ok"], (where, f, s)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_default_library_within_two_float_ulp(fast_rows, grid):
    for r in _of_grid(fast_rows, grid):
        where = {k: r[k] for k in ("desc", "layout", "met_pbl", "smooth")}
        for f, s in r["fields"].items():
            print(grid, where, f, s)
            assert s["nan_mismatch"] == 0 and s["max_ulp"] <= 2 and s["padding_ok"], (where, f, s)


def test_the_comparison_sees_nan_and_values(exact_rows):
    """Not vacuous: the compared fields hold NaNs (columns without a parcel, without cloud, without free convection) and
    finite values side by side."""
    r = _of_grid(exact_rows, GRIDS[1])[0]
    for f in ("pct", "pcb", "plcl", "plfc", "pel", "cin"):
        assert 0 < r["fields"][f]["nan"] < 37 * 19, f
    for f in ("z", "o3c", "pbl", "cl"):
        assert r["fields"][f]["nan"] == 0, f


# ---- bits and refusals (the library this process loads) ------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim():
    s = with_clim(bare_context())
    yield s
    s.close()


KEY = (9, 7, 20, 2024, False)
BIT_FIELDS = {"geopot": ("z",), "o3c": ("o3c",), "pbl": ("pbl",), "cloud": ("pct", "pcb", "cl"),
              "cape": ("plcl", "plfc", "pel", "cape", "cin")}


@pytest.mark.parametrize("bit", ALL)
@pytest.mark.parametrize("layout", ["compact", "strided"])
def test_one_bit_writes_only_its_outputs(sim, bit, layout):
    met = R.atmosphere(*KEY)
    view = met if layout == "compact" else R.strided(met)
    ref, _ = R.reference(KEY, 3, -1, -1)
    out = sentinel_outputs(view)
    got = sim.derive_met(view, bit, out=out)
    assert sorted(got) == sorted(BIT_FIELDS[bit])
    for f in FIELDS:
        if f in BIT_FIELDS[bit]:
            both = ~np.isnan(ref[f])
            assert np.array_equal(np.isnan(out[f]), np.isnan(ref[f])) and ulp_distance(out[f][both], ref[f][both]).max() <= 2, f
        else:
            assert (out[f] == SENTINEL).all(), f
        assert padding_untouched(out[f]), f


def _without(met, *names):
    from mptrac_amd.synth import Met
    view = Met.__new__(Met)
    view.__dict__.update(met.__dict__)
    view.f3 = {k: v for k, v in met.f3.items() if k not in names}
    view.f2 = {k: v for k, v in met.f2.items() if k not in names}
    return view


REFUSALS = [("geopot", "zs", {}), ("o3c", "o3", {}), ("pbl", "ts", {}), ("pbl", "us", dict(met_pbl=2)),
            ("pbl", "z", dict(met_pbl=2)), ("cloud", "iwc", {}), ("cape", "h2o", {}), ("pbl", None, dict(met_pbl=1))]


@pytest.mark.parametrize("bit,missing,opts", REFUSALS, ids=[f"{b}-{m}" for b, m, _ in REFUSALS])
def test_refused_calls_write_nothing(sim, bit, missing, opts):
    from mptrac_amd.hip import MphipError
    met = R.atmosphere(*KEY)
    view = _without(met, missing) if missing else met
    out = sentinel_outputs(view)
    with pytest.raises(MphipError, match="mphip_derive_met"):
        sim.derive_met(view, bit, out=out, **opts)
    assert all((a == SENTINEL).all() for a in out.values())


def test_pbl_2_takes_a_given_z(sim):
    """met_pbl 2 without the GEOPOT bit reads z from the input: the same pbl as deriving both in one call."""
    met = R.atmosphere(*KEY)
    both = sim.derive_met(met, ("geopot", "pbl"), met_pbl=2)
    from mptrac_amd.synth import Met
    given = Met.__new__(Met)
    given.__dict__.update(met.__dict__)
    given.f3 = dict(met.f3, z=both["z"])
    alone = sim.derive_met(given, "pbl", met_pbl=2)
    assert np.array_equal(alone["pbl"], both["pbl"])


def test_cape_needs_the_tropopause_climatology_and_two_levels(sim):
    from mptrac_amd.hip import MphipError
    from mptrac_amd.synth import Met
    met = R.atmosphere(*KEY)
    fresh = bare_context()
    try:
        out = sentinel_outputs(met)
        with pytest.raises(MphipError, match="mphip_update_clim"):
            fresh.derive_met(met, "cape", out=out)
        assert all((a == SENTINEL).all() for a in out.values())
        assert fresh.derive_met(met, "o3c")["o3c"].shape == (met.nx, met.ny)      # the other bits do not need it
    finally:
        fresh.close()
    one = Met(met.time, met.lon, met.lat, met.p[:1], {k: v[:, :, :1] for k, v in met.f3.items()}, dict(met.f2))
    out = sentinel_outputs(one)
    with pytest.raises(MphipError, match="np < 2"):
        sim.derive_met(one, ALL, out=out)
    assert all((a == SENTINEL).all() for a in out.values())


# ---- a run is not disturbed -------------------------------------------------------------------------------------------------

def test_calls_between_time_steps_do_not_disturb_a_run():
    """Twenty steps of the case "full" with a derive_met call between the steps end with the bits of the run without."""
    import cases
    from mptrac_amd.hip import Simulation
    met = R.atmosphere(37, 19, 20, 2024, False)
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
                    got = run.derive_met(met, ALL, met_pbl=2 if k % 2 else 3)
                    assert np.isfinite(got["z"]).all()
            states.append(run.state())
        finally:
            run.close()
    a, b = states
    for k in ("time", "lon", "lat", "p", "q", "uvwp"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


if __name__ == "__main__" and "--child" in sys.argv:
    child()
