"""The cases of tests/intpol_cases.py without a device: the oracle's scalar orc_intpol_met_time_3d / _2d -- the reference of
the device tests -- against the numpy statement of tests/refmodules.py (Ref.time_3d / time_2d: Weights, space_3d and the
2-D rule space_2d) at 1e-13; a census ON THE INPUTS that they reach what the call can get wrong; the ABI of
mphip_intpol_met in the header, the export map, the Python mirror and the option table; and the control key
HIP_DEVICE_INTPOL."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import hostfiles as hf
import intpol_cases as IC
import refmodules as R
from mptrac_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-13


def _numpy_rows(c, f3, f2):
    ref = R.Ref(None, (np.zeros(1), np.zeros(1), np.zeros((1, 1))), c["m0"], c["m1"])
    good = ~c["nan"]
    t, p, lon, lat = (c[k][good] for k in ("time", "p", "lon", "lat"))
    rows = np.full((len(f3) + len(f2), len(good)), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, name in enumerate(f3):
            rows[k, good] = ref.time_3d(name, t, p, lon, lat)
        for k, name in enumerate(f2):
            rows[len(f3) + k, good] = ref.time_2d(name, t, lon, lat)
    return rows


def _check(c):
    f3, f2 = IC.fields_of(c)
    assert f3 and f2
    want = IC.expected(c, f3 + f2)
    got = _numpy_rows(c, f3, f2)
    assert np.array_equal(np.isnan(got), np.isnan(want)), c["name"]
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    ok = np.isfinite(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1.0)
    assert err.size and err.max() <= TOL, (c["name"], err.max())


@pytest.mark.parametrize("lon0,lat,p", IC.AXIS_GRIDS)
def test_oracle_against_the_numpy_statement_on_the_axis_edge_grids(lon0, lat, p):
    c = IC.axis_edges(lon0, lat, p)
    f3, f2 = IC.fields_of(c)
    assert set(f3) == set(IC.F3) and set(f2) == set(IC.F2)       # every pressure-level and surface field
    _check(c)


@pytest.mark.parametrize("c", IC.small_cases(), ids=lambda c: c["name"])
def test_oracle_against_the_numpy_statement_on_the_small_cases(c):
    _check(c)


# ---- census: conditions on the inputs --------------------------------------------------------------------------------
@pytest.mark.parametrize("lon0,lat,p", IC.AXIS_GRIDS)
def test_census_every_node_and_its_neighbours_occur_on_every_axis(lon0, lat, p):
    c = IC.axis_edges(lon0, lat, p)
    m = c["m0"]
    assert len(c["lon"]) == IC.N_AXIS
    for axis, points, keep in ((m.lon, c["lon"], lambda v: True), (m.lat, c["lat"], lambda v: abs(v) <= 90.0),
                               (m.p, c["p"], lambda v: True)):
        have = set(points.tolist())
        for x in axis:
            for v in (x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)):
                assert not keep(v) or float(v) in have, (x, v)
    # both ends and beyond, +- 360 degrees
    assert c["lon"].max() > m.lon[-1] + 300.0 and (c["lon"] == m.lon[0] + 360.0).any() and (c["lon"] == m.lon[-1] - 360.0).any()
    assert c["p"].max() > m.p.max() and c["p"].min() < m.p.min()
    wt = (c["m1"].time - c["time"]) / (c["m1"].time - c["m0"].time)
    assert (wt == 0).any() and (wt == 1).any() and (wt == 0.5).any() and (wt < 0).any() and (wt > 1).any()
    assert set(IC.time_cycle(c["m0"].time, c["m1"].time).tolist()) <= set(c["time"].tolist())


def test_census_every_branch_of_the_surface_rule_is_reached():
    c = IC.nonfinite()
    m0, m1 = c["m0"], c["m1"]
    w = R.Weights(m0, None, c["lon"], c["lat"], three_d=False)
    a = m0.f2["ps"]
    corners = np.stack([a[w.ix, w.iy], a[w.ix, w.iy + 1], a[w.ix + 1, w.iy], a[w.ix + 1, w.iy + 1]])
    nearest = ~np.isfinite(corners).all(axis=0)
    assert {int(k) for k in np.count_nonzero(np.isnan(corners[:, nearest]), axis=0)} >= {1, 2, 3, 4}
    assert np.isinf(corners).any()
    for qx in (True, False):        # the four quadrants, with a corner that is not finite
        for qy in (True, False):
            assert (nearest & ((w.wx < 0.5) == qx) & ((w.wy < 0.5) == qy) & (w.wx != 0.5) & (w.wy != 0.5)).any(), (qx, qy)
    assert (nearest & (w.wx == 0.5)).any() and (nearest & (w.wy == 0.5)).any()       # both ties
    wt = (m1.time - c["time"]) / (m1.time - m0.time)
    assert np.isnan(m1.f2["pbl"]).all() and np.isnan(m0.f2["ts"]).all()              # one whole snapshot NaN, either one
    assert (wt == 0.5).any() and (wt == np.nextafter(0.5, 0.0)).any() and (wt == np.nextafter(0.5, 1.0)).any()
    assert (wt < 0.5).any() and (wt > 0.5).any()                                     # both snapshot choices
    w3 = R.Weights(m0, c["p"], c["lon"], c["lat"])
    t = m0.f3["t"]
    assert np.isnan(t[w3.ix, w3.iy, w3.ip]).any() or np.isnan(t[w3.ix + 1, w3.iy + 1, w3.ip + 1]).any()


def test_census_other_grids_and_bad_points():
    for coord_type in (0, 1):
        c = IC.regional(coord_type)
        assert c["m0"].coord_type == coord_type and c["m0"].lon[0] == 10.0 and c["m0"].lon[-1] == 40.0
        assert {9.5, -10.0, 40.5, 60.0} <= set(c["lon"].tolist())
    assert (IC.two_cubed()["m0"].nx, IC.two_cubed()["m0"].ny, IC.two_cubed()["m0"].np) == (2, 2, 2)
    c = IC.bad_points()
    bad = np.stack([c[k] for k in ("time", "p", "lon", "lat")])
    for k in range(4):
        for test in (np.isnan, lambda v: v == np.inf, lambda v: v == -np.inf):
            assert (test(bad[k]) & np.isfinite(np.delete(bad, k, axis=0)).all(axis=0)).any(), k
    assert (c["lon"] == 2e9).any() and np.array_equal(c["nan"], ~np.isfinite(bad).all(axis=0) | (np.abs(c["lon"]) > 1e9))
    assert np.isnan(IC.expected(c, ("t", "ps"))[:, c["nan"]]).all() and np.isfinite(IC.expected(c, ("t", "ps"))[:, ~c["nan"]]).all()


# ---- the ABI -----------------------------------------------------------------------------------------------------------
def test_abi_header_export_map_python_mirror_and_option_table():
    header = open(os.path.join(ROOT, "include", "mptrac_hip.h")).read()
    proto = re.search(r"int mphip_intpol_met\(([^;]*)\);", header)
    assert proto, "mphip_intpol_met is not declared in include/mptrac_hip.h"
    args = " ".join(proto.group(1).split())
    assert args == ("mphip_ctx *ctx, long long n, const double *time, long long ntime, const double *p, const double *lon, "
                    "const double *lat, int nfield, const int *field, double *out")
    flag = re.search(r"#define MPHIP_INTPOL_2D\s+(\d+)", header)
    assert flag and int(flag.group(1)) == 256
    from mptrac_amd import hip
    from mptrac_amd.synth import FIELDS_3D
    assert hip.INTPOL_2D == int(flag.group(1)) and hip.INTPOL_2D > len(FIELDS_3D) and hip.INTPOL_2D & (hip.INTPOL_2D - 1) == 0
    exported = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "mptrac_amd", "csrc", "abi.map")).read())
    assert any(fnmatch.fnmatchcase("mphip_intpol_met", pat.strip()) for pat in exported)
    mirror = open(os.path.join(ROOT, "mptrac_amd", "hip.py")).read()
    assert re.search(r"L\.mphip_intpol_met\.argtypes = \[C\.c_void_p, C\.c_longlong, _dp, C\.c_longlong, _dp, _dp, _dp, C\.c_int, "
                     r"C\.POINTER\(C\.c_int\), _dp\]", mirror)
    assert callable(getattr(hip.Simulation, "intpol_met", None))
    api = open(os.path.join(ROOT, "mptrac_amd", "csrc", "mphip_api.hip")).read()
    row = re.search(r'number\("intpol_chunk", &mphip_ctx::intpol_chunk, kRange, 64, 1 << 24,', api)
    assert row and re.search(r"int intpol_chunk = 1 << 22;", api)
    assert '"intpol_chunk"' in header


# ---- the control key ---------------------------------------------------------------------------------------------------
def _met_conv(tmp, *extra):
    build.build_host()
    hf.write_ctl(os.path.join(tmp, "trac.ctl"), {"NQ": 0, "METBASE": os.path.join(tmp, "met"), "MET_TYPE": 1})
    r = subprocess.run([build.MET_CONV_BIN, os.path.join(tmp, "trac.ctl"), os.path.join(tmp, "absent_2022_06_02_00.bin"), "1",
                        os.path.join(tmp, "out.bin"), "1", *extra], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    return r.returncode, r.stdout.decode()


@pytest.mark.parametrize("value", ["0", "1"])
def test_hip_device_intpol_accepted(tmp_path, value):
    """The control file passes: the tool goes on to the file, which is absent."""
    rc, out = _met_conv(str(tmp_path), "HIP_DEVICE_INTPOL", value)
    assert "Cannot open file" in out and "HIP_DEVICE_INTPOL = " + value in out and "Set HIP_DEVICE_INTPOL" not in out, out[-1500:]


@pytest.mark.parametrize("value", ["2", "-1"])
def test_hip_device_intpol_refused_with_the_keys_name(tmp_path, value):
    rc, out = _met_conv(str(tmp_path), "HIP_DEVICE_INTPOL", value)
    assert rc != 0 and "Error" in out and "HIP_DEVICE_INTPOL" in out, out[-1500:]
