"""The restatement tests/refingest.py pinned to the host loops that are the definition of mphip_ingest_met, without a
device: every case of tests/ingest_cases.py is written as a netCDF file (scipy.io.netcdf_file: floats, or packed shorts
with scale_factor / add_offset, with _FillValue / missing_value attributes), read by the host layer's reader
(tests/c/ingest_host.c: mptrac_read_met with HIP_MET_PREP 0, HIP_MET_INGEST 0, into a fresh met_t) and compared with the
restatement bit for bit -- every level and surface field of the case, the extent nx2 and the longitudes.

The program is the host layer's sources compiled with EP = 130, so that the cases with 65 and 129 levels fit the fixed
extents (the library of the package is built with EP = 64)."""
import os
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

import ingest_cases as K
import refingest as R
from mptrac_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
NC_NAME = {"t": "t", "u": "u", "v": "v", "w": "w", "h2o": "q", "o3": "o3", "lwc": "clwc", "rwc": "crwc", "iwc": "ciwc",
           "swc": "cswc", "cc": "cc", "ps": "sp", "zs": "z", "ts": "t2m", "us": "u10m", "vs": "v10m", "ess": "iews", "nss": "inss",
           "shf": "ishf", "lsm": "lsm", "sst": "sstk", "pbl": "blp", "cape": "cape", "cin": "cin"}


def write_nc(path, case):
    """The case as a classic netCDF file the reader accepts: axes lon / lat (x / y on a Cartesian grid), lev in Pa."""
    x, y = ("lon", "lat") if case["coord_type"] == 0 else ("x", "y")
    with netcdf_file(path, "w") as f:
        f.createDimension(x, case["nx"])
        f.createDimension(y, case["ny"])
        f.createDimension("lev", case["np"])
        for name, axis in ((x, case["lon"]), (y, case["lat"]), ("lev", 100.0 * case["p"])):
            v = f.createVariable(name, "d", (name,))
            v[:] = axis
        for name, (a, opt) in case["raw"].items():
            short = a.dtype == np.int16
            nc = "lnsp" if opt.get("lnsp") else NC_NAME[name]
            v = f.createVariable(nc, "h" if short else "f", ("lev", y, x) if a.ndim == 3 else (y, x))
            v[:] = a
            kind = np.int16 if short else np.float32
            if "fill" in opt:
                v._FillValue = kind(opt["fill"])
            if "miss" in opt:
                v.missing_value = kind(opt["miss"])
            if short:
                v.scale_factor = np.float64(opt["scale_factor"])
                v.add_offset = np.float64(opt["add_offset"])


@pytest.fixture(scope="module")
def ingest_host():
    """tests/c/ingest_host.c and the host layer's sources as one program with EP = 130."""
    build.build_host()
    out_dir = os.path.join(HERE, "c", "build")
    os.makedirs(out_dir, exist_ok=True)
    src, exe = os.path.join(HERE, "c", "ingest_host.c"), os.path.join(out_dir, "ingest_host")
    host = [os.path.join(build.HOST_DIR, f) for f in ("mptrac.c", "ctlfile.c", "nc_classic.c", "nc_hdf5.c", "rendezvous.c",
                                                       "output.c")]
    newest = max(os.path.getmtime(f) for f in [src, *host, os.path.join(build.HOST_DIR, "mptrac.h")])
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        defs = [f"-D{k}={v}" for k, v in dict(build.HOST_DIMS, EP=130, NP=1000).items()]
        defs.append('-DMPTRAC_AMD_DATA_DIR="%s"' % os.path.join(os.path.dirname(build.HOST_DIR), "data"))
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-mcmodel=medium", *defs, "-I", build.HOST_DIR, "-o", exe, src,
                               *host, "-L" + build.LIBDIR, "-lmptrac_hip", "-Wl,-rpath," + build.LIBDIR,
                               "-Wl,-rpath,/opt/rocm/lib", "-lm", "-lpthread", "-lz"])
    return exe


def read_dump(path):
    raw = open(path, "rb").read()
    nx, ny, np_ = np.frombuffer(raw, dtype=np.int32, count=3)
    at = 12
    lon = np.frombuffer(raw, dtype=np.float64, count=nx, offset=at)
    at += 8 * nx
    f3, f2 = {}, {}
    for name in K.LEVEL_FIELDS:
        f3[name] = np.frombuffer(raw, dtype=np.uint32, count=nx * ny * np_, offset=at).reshape(nx, ny, np_)
        at += 4 * nx * ny * np_
    for name in K.SURFACE_FIELDS:
        f2[name] = np.frombuffer(raw, dtype=np.uint32, count=nx * ny, offset=at).reshape(nx, ny)
        at += 4 * nx * ny
    assert at == len(raw)
    return lon, f3, f2


@pytest.mark.parametrize("tag", sorted(K.CASES))
def test_host_reader_gives_the_restatement_bits(tag, ingest_host, tmp_path):
    case = K.CASES[tag]
    path = str(tmp_path / "met_2001_02_03_04.nc")
    write_nc(path, case)
    dump = str(tmp_path / "dump.bin")
    res = subprocess.run([ingest_host, path, dump, str(case["coord_type"])], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    lon, f3, f2 = read_dump(dump)
    lon2, r3, r2 = R.ingest(case["raw"], case["lon"], case["lat"], case["p"], case["coord_type"], R.ALL)
    assert np.array_equal(lon, lon2)
    for name, ref in list(r3.items()) + list(r2.items()):
        got = (f3 if ref.ndim == 3 else f2)[name]
        assert got.shape == ref.shape, name
        differ = int((got != R.bits(ref)).sum())
        assert differ == 0, f"{name}: {differ} of {got.size} values differ"


def test_the_cases_hold_what_they_are_named_for():
    nxs, nps, nys = set(), set(), set()
    lows = set()
    for case in K.CASES.values():
        nxs.add(case["nx"]), nps.add(case["np"]), nys.add(case["ny"])
        assert case["nx"] * case["ny"] * case["np"] <= K.MOST
        _, f3, _ = R.ingest(case["raw"], case["lon"], case["lat"], case["p"], case["coord_type"], R.DECODE)
        bad = np.zeros(f3["t"].shape, dtype=bool)
        for name in ("t", "u", "v", "w"):
            if name in f3:
                bad |= ~np.isfinite(f3[name])
        low = np.where(bad.any(axis=2), case["np"] - 1 - np.argmax(bad[:, :, ::-1], axis=2), -1)
        lows |= {("-1", "0", "np-2", "np-1")[k] for k, v in enumerate((-1, 0, case["np"] - 2, case["np"] - 1)) if (low == v).any()}
    assert nxs == nps == set(K.EXTENTS) and nys == set(K.NYS)
    assert lows == {"-1", "0", "np-2", "np-1"}
    acts = {(R.polar_acts(c["lat"], c["coord_type"]), R.periodic_acts(c["lon"], c["coord_type"])) for c in K.CASES.values()}
    assert acts == {(True, True), (True, False), (False, True), (False, False)}
    edge, below = K.CASES["poles_edge_ny5_coord0_float"], K.CASES["poles_below_ny5_coord0_float"]
    assert abs(edge["lat"][0]) == 89.999 == abs(edge["lat"][-1]) and R.polar_acts(edge["lat"], 0)
    assert abs(below["lat"][-1]) == np.nextafter(89.999, 0.0) and not R.polar_acts(below["lat"], 0)
    miss = K.lon_axis(64, "miss")
    assert abs(abs(miss[-1] - miss[0] + miss[1] - miss[0] - 360) - 0.02) < 1e-9 and not R.periodic_acts(miss, 0)


def _met_conv(tmp_path, value):
    """met_conv on a netCDF file that is absent: the control keys are read before the file is looked for."""
    build.build_host()
    res = subprocess.run([build.MET_CONV_BIN, "-", str(tmp_path / "absent_2001_02_03_04.nc"), "0", str(tmp_path / "out.bin"), "1",
                          "MET_TYPE", "0", "HIP_MET_INGEST", value], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=120)
    return res, res.stdout


@pytest.mark.parametrize("value", ["0", "1"])
def test_hip_met_ingest_accepted(tmp_path, value):
    res, out = _met_conv(tmp_path, value)
    assert "Cannot open file" in out and "HIP_MET_INGEST = " + value in out and "Set HIP_MET_INGEST" not in out, out[-1500:]


@pytest.mark.parametrize("value", ["2", "-1"])
def test_hip_met_ingest_refused_with_the_keys_name(tmp_path, value):
    res, out = _met_conv(tmp_path, value)
    assert res.returncode != 0 and "Set HIP_MET_INGEST to 0 or 1!" in out, out[-1500:]
