"""MET_TYPE 2 through the drop-in boundary: `met_conv` 1 -> 2 -> 1 and `trac` on the world of tests/test_host_driver.py
(four hourly files on the 37 x 19 x 20 grid, 3000 particles, three hours, gridded output every hour with the implicit
volume mixing ratio: the temperature at the cell centres is read on the host, the lazy met_need_floats path).

The type-2 file is byte for byte what tests/packfiles.py writes from the restatement, and the file converted back is the
restatement's decode within the reader's limits.  `trac` writes the same particle and grid files from the type-2 files with
HIP_MET_PACKED 1 (codes to the device), with HIP_MET_PACKED 0 (decoded when read) and from the type-1 files converted back,
each also with the read-ahead thread of HIP_MET_PREFETCH 1."""
import os
import subprocess

import numpy as np
import pytest

import hostfiles as hf
import packfiles as pf
import refpack as R
from mptrac_amd import build
from test_gpu_metprep_driver import read_met_bin
from test_host_driver import QUANT, _setup

pytestmark = pytest.mark.gpu
HOURS = 3


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    return r.returncode, r.stdout.decode()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The type-1 files (base `met`), their type-2 conversions (`pck`) and those converted back (`back`)."""
    tmp = str(tmp_path_factory.mktemp("pack"))
    trac, mets, atm = _setup(tmp, n=3000, hours=HOURS, extra={"MOLMASS": 64.066})
    ctl = os.path.join(tmp, "trac.ctl")
    for m in mets:
        src = hf.met_filename(os.path.join(tmp, "met"), m.time)
        pck = pf.met_pck_filename(os.path.join(tmp, "pck"), m.time)
        back = hf.met_filename(os.path.join(tmp, "back"), m.time)
        rc, out = _run([build.MET_CONV_BIN, ctl, src, "1", pck, "2"])
        assert rc == 0, out[-2000:]
        rc, out = _run([build.MET_CONV_BIN, ctl, pck, "2", back, "1"])
        assert rc == 0 and "Decoded on the device" in out, out[-2000:]
    return dict(tmp=tmp, trac=trac, mets=mets)


def _trac(world, leg, *args):
    d = os.path.join(world["tmp"], leg)
    os.makedirs(d)
    for name in ("trac.ctl", "atm_in"):
        with open(os.path.join(world["tmp"], name), "rb") as a, open(os.path.join(d, name), "wb") as b:
            b.write(a.read())
    open(os.path.join(d, "dirlist"), "w").write(d + "\n")
    rc, out = _run([world["trac"], os.path.join(d, "dirlist"), "trac.ctl", "atm_in", *args])
    assert rc == 0, out[-3000:]
    return d, out


def _outputs(d):
    names = sorted(f for f in os.listdir(d) if f.startswith(("atm_2022", "grid_2022")))
    assert len([f for f in names if f.startswith("atm_")]) == HOURS + 1 and any(f.startswith("grid_") for f in names)
    return {f: open(os.path.join(d, f), "rb").read() for f in names}


def test_met_conv_writes_the_restatement_file_and_half_the_level_bytes(world):
    for m in world["mets"]:
        pck = pf.met_pck_filename(os.path.join(world["tmp"], "pck"), m.time)
        raw = open(pck, "rb").read()
        assert len(raw) == pf.file_size(m.nx, m.ny, m.np)
        assert raw == pf.met_pck_bytes(m)
        src = hf.met_filename(os.path.join(world["tmp"], "met"), m.time)
        assert os.path.getsize(src) - len(raw) == 13 * (2 * m.nx * m.ny * m.np - 16 * m.np)


def test_met_conv_back_to_type_1_is_the_restatement_decode(world):
    for m in world["mets"]:
        time, axes, f2, f3 = read_met_bin(hf.met_filename(os.path.join(world["tmp"], "back"), m.time))
        first = read_met_bin(hf.met_filename(os.path.join(world["tmp"], "met"), m.time))
        assert time == m.time and all(np.array_equal(a, b) for a, b in zip(axes, first[1]))
        for name in hf.SURF_ORDER:
            assert f2[name].tobytes() == first[2][name].tobytes(), name
        for name in hf.LEVEL_ORDER:
            ref = R.roundtrip(pf.level_field(m, name), *pf.LIMITS[name])
            assert R.same_bits(f3[name], ref), name
        assert not np.array_equal(f3["u"], first[3]["u"])


@pytest.fixture(scope="module")
def packed_run(world):
    d, out = _trac(world, "packed", "METBASE", os.path.join(world["tmp"], "pck"), "MET_TYPE", "2")
    assert "Decoded on the device" in out       # (the grid output's temperature: the lazy path, once per snapshot)
    return _outputs(d)


def test_trac_writes_the_same_files_from_codes_and_from_floats(world, packed_run):
    d, out = _trac(world, "unpacked", "METBASE", os.path.join(world["tmp"], "pck"), "MET_TYPE", "2", "HIP_MET_PACKED", "0")
    assert _outputs(d) == packed_run
    d, out = _trac(world, "back_run", "METBASE", os.path.join(world["tmp"], "back"), "MET_TYPE", "1")
    assert "Decoded on the device" not in out
    assert _outputs(d) == packed_run
    # (and the packed meteorology is not the original one)
    d, out = _trac(world, "first", "METBASE", os.path.join(world["tmp"], "met"), "MET_TYPE", "1")
    last = "atm_2022_06_02_%02d_00_00.bin" % HOURS
    assert _outputs(d)[last] != packed_run[last]
    assert len(hf.read_atm_bin(os.path.join(d, last), len(QUANT))["lon"]) == 3000


@pytest.mark.parametrize("leg,args", [("packed_ahead", ("pck", "2", "HIP_MET_PACKED", "1")),
                                      ("unpacked_ahead", ("pck", "2", "HIP_MET_PACKED", "0")),
                                      ("back_ahead", ("back", "1"))])
def test_the_read_ahead_thread_hands_over_the_same(world, packed_run, leg, args):
    d, out = _trac(world, leg, "METBASE", os.path.join(world["tmp"], args[0]), "MET_TYPE", args[1], *args[2:],
                   "HIP_MET_PREFETCH", "1")
    assert out.count("Meteo data from the read-ahead") == 2, out[-3000:]
    assert _outputs(d) == packed_run
