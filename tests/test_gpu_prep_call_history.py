"""The result of a preprocessing call does not depend on which preprocessing calls its context has served before.

mphip_derive_met, mphip_regrid_met, mphip_detrend_met, mphip_ingest_met, mphip_unpack_met and mphip_pack_met take their
device scratch from one pool that hands its buffers out from the first again at every call: a buffer
may have served a call of another kind, with another element type (floats, doubles, row records, raw shorts, blocks of
scales, offsets and codes) and another size.  One context runs a sequence that mixes the six kinds, small after large and
large after small, with a refused call in between; every accepted call is compared bit for bit (integer views of the
element's width) with the same call made alone on a context created just for it, by the same library in the same
process.  Equality is exact: the code and the inputs are the same.  That the values are the right ones is what
tests/test_gpu_metprep.py, test_gpu_pv_tropo.py, test_gpu_regrid.py, test_gpu_detrend.py, test_gpu_ingest.py and
test_gpu_pack.py assert.

The ingest, unpack and pack rows are the smallest cases of tests/ingest_cases.py and tests/pack_cases.py (2 x 2 x 2) that
give a periodic column from two longitudes, both poles, and a field of two levels with distinct ranges; for each,
tests/refingest.py and tests/refpack.py alone give two distinct finite values or more in every returned array, the
per-level scl and off included.

The derive bits are those that need no climatology.  MPHIP_PREP_PV is refused below five rows, so on 5 x 4 x 137 the call
leaves it out and a call on 5 x 5 x 137 with every bit follows.  A process loads one library: each runs in a child (as
tests/test_gpu_regrid.py does)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detrend_cases as D       # noqa: E402
import ingest_cases as I        # noqa: E402
import pack_cases as Q          # noqa: E402
import refmetprep as M          # noqa: E402
import regrid_cases as K        # noqa: E402
from test_gpu_regrid import bare_context, sentinel_like, untouched      # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-7777.)
BITS = ("geopot", "o3c", "pbl", "cloud", "pv", "tropo")


def derive(nx, ny, n, bits=BITS):
    def call(sim):
        return sim.derive_met(M.atmosphere(nx, ny, n), bits, met_pbl=3, met_tropo=3)
    return call


def detrend(name):
    def call(sim):
        met, scale = D.case(name)
        return sim.detrend_met(met, scale)
    return call


def _fields(snap):
    out = {"f3_" + k: v for k, v in snap.f3.items()}
    out.update({"f2_" + k: v for k, v in snap.f2.items()})
    out.update(lon=snap.lon, lat=snap.lat, p=snap.p)
    return out


def regrid_both(sim):
    """ML2PL and SAMPLE in one call on 19 x 11 x 20: strided input, strided output."""
    met = K.ml_atmosphere(19, 11, 20)
    shape = (10, 11, 7)                              # strides 2, 1, 3 of 19 x 11 x 20 target levels
    st = ((11 + 3) * (7 + 2), 7 + 2, 11 + 3)
    out = sentinel_like(shape, [f for f in met.f3 if f != "pl"], list(met.f2), st)
    got = sim.regrid_met(K.strided(met), ("ml2pl", "sample"), met_p=K.targets(20), out=out, out_strides=st,
                         met_dx=2, met_dy=1, met_dp=3, met_sx=2, met_sy=3, met_sp=2)
    assert (got.f3["t"].shape, got.f2["ps"].shape) == (shape, shape[:2])
    return _fields(got)


def regrid_smallest(sim):
    met, d, s = K.sample_input("sx_minus_1_is_nx")
    return _fields(sim.regrid_met(met, "sample", met_dx=d[0], met_dy=d[1], met_dp=d[2], met_sx=s[0], met_sy=s[1], met_sp=s[2]))


def ingest_all_stages(sim):
    """Decode (raw shorts), extrapolate, both poles and the periodic column in one call on 2 x 2 x 2."""
    from mptrac_amd.hip import Snapshot
    c = I.CASES["shape_2x2x2_short"]
    axes = Snapshot(0.0, c["coord_type"], np.ascontiguousarray(c["lon"]), np.ascontiguousarray(c["lat"]),
                    np.ascontiguousarray(c["p"]), {}, {})
    got = sim.ingest_met(c["raw"], axes, ("decode", "extrapolate", "polar", "periodic"))
    assert got.f3["u"].shape == (3, 2, 2) and got.lat[0] == 90.0 and got.lat[-1] == -90.0
    return _fields(got)


def _grid_2x2x2():
    from mptrac_amd.hip import Snapshot
    return Snapshot(0.0, 0, np.arange(2, dtype=np.float64), np.arange(2, dtype=np.float64), np.arange(2, 0, -1.0), {}, {})


def unpack_hand(sim):
    return sim.unpack_met(_grid_2x2x2(), {"t": Q.DECODE["hand_2x2x2"]})


def pack_smooth(sim):
    """Two levels of distinct ranges: the codes, and scl and off per level."""
    met = _grid_2x2x2()
    met.f3["t"] = Q.ENCODE["smooth_2x2x2"]
    codes, scl, off = sim.pack_met(met)["t"]
    return dict(t_codes=codes, t_scl=scl, t_off=off)


def refused(sim):
    """A detrending with a NaN scale: refused, and its outputs stay as they are."""
    from mptrac_amd import hip
    met, _ = D.case("smallest")
    out = {f: np.full((met.nx, met.ny, met.np), SENTINEL) for f in met.f3}
    try:
        sim.detrend_met(met, float("nan"), out=out)
    except hip.MphipError as exc:
        return all(untouched(a) for a in out.values()), str(exc)
    return False, "accepted"


# (name, call); None: the refused call
SEQUENCE = [("detrend_smallest", detrend("smallest")),
            ("derive_37x19x20", derive(37, 19, 20)),
            ("ingest_all_stages_2x2x2_short", ingest_all_stages),
            ("regrid_ml2pl_sample_19x11x20", regrid_both),
            ("derive_5x4x137", derive(5, 4, 137, tuple(b for b in BITS if b != "pv"))),
            ("unpack_hand_2x2x2", unpack_hand),
            ("derive_5x5x137", derive(5, 5, 137)),
            ("pack_smooth_2x2x2", pack_smooth),
            ("detrend_two_workgroups", detrend("two_workgroups")),
            ("regrid_sx_minus_1_is_nx", regrid_smallest),
            ("refused", None),
            ("derive_9x7x20", derive(9, 7, 20)),
            ("detrend_smallest_again", detrend("smallest"))]


def child():
    from mptrac_amd import hip
    print("library:", hip.load().mphip_version().decode(), flush=True)
    history = bare_context()
    rows = []
    for name, call in SEQUENCE:
        if call is None:
            ok, msg = refused(history)
            rows.append(dict(name=name, refused=ok, message=msg))
            continue
        got = call(history)
        alone_ctx = bare_context()
        alone = call(alone_ctx)
        alone_ctx.close()
        assert sorted(got) == sorted(alone) and got
        fields = {}
        for f in got:
            a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(alone[f])
            bits = "i%d" % a.itemsize            # (float32 fields, float64 axes, scl and off, uint16 codes)
            fields[f] = dict(differ=int((a.view(bits) != b.view(bits)).sum()) if a.shape == b.shape else -1,
                             distinct=int(len(np.unique(b[np.isfinite(b)]))))
        rows.append(dict(name=name, fields=fields))
    history.close()
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


@pytest.fixture(scope="module", params=["exact", "default"])
def rows(request):
    return _run_child(request.param == "exact")


def test_every_call_returns_the_bits_of_the_same_call_alone(rows):
    assert [r["name"] for r in rows] == [name for name, _ in SEQUENCE]
    for r in rows:
        if "fields" in r:
            assert r["fields"], r
            for f, s in r["fields"].items():
                assert s["differ"] == 0, (r["name"], f, s)


def test_the_comparison_sees_values(rows):
    """Every compared field holds two distinct finite values or more: equal bits are not those of an empty result."""
    for r in rows:
        for f, s in r.get("fields", {}).items():
            assert s["distinct"] >= 2, (r["name"], f, s)


def test_the_refused_call_writes_nothing(rows):
    r = [r for r in rows if r["name"] == "refused"]
    assert len(r) == 1 and r[0]["refused"], r
    assert r[0]["message"].startswith("mphip_detrend_met: ") and "met_detrend" in r[0]["message"], r


if __name__ == "__main__" and "--child" in sys.argv:
    child()
