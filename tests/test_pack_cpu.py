"""The 16-bit packed level fields without a device: the restatement tests/refpack.py on the cases of tests/pack_cases.py, the
file writer tests/packfiles.py, and what `trac` and `met_conv` accept and refuse of MET_TYPE before any device is needed.

The bound of the round trip follows from the definition: the code is the nearest step of width scl (half a step, up to the
rounding of one double division and one double sum, which are 2^-53 relative and vanish in the next term) and the decoded
double is rounded to float once (half a float ulp; a whole one is allowed): |decode(encode(x)) - x| <= scl / 2 +
ulp_float(|decoded|)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hostfiles as hf
import pack_cases as K
import packfiles as pf
import refpack as R
from mptrac_amd import build


@pytest.mark.parametrize("name", sorted(K.ENCODE))
def test_round_trip_stays_within_half_a_step_and_a_float_ulp(name):
    x = K.ENCODE[name]
    q, scl, off = R.encode(x)
    assert q.dtype == np.uint16 and q.shape == x.shape and scl.shape == off.shape == (x.shape[2],)
    assert int(q.max()) <= R.TOP, "a code above 65533"
    assert np.isfinite(scl).all() and np.isfinite(off).all() and (scl > 0).all() and not np.signbit(off[off == 0]).any()
    back = R.decode(q, scl, off)
    err = np.abs(back.astype(np.float64) - x.astype(np.float64))
    bound = scl / 2 + R.ulp_float(back)
    print(name, "largest distance in steps:", float((err / scl).max()), "share of the bound:", float((err / bound).max()))
    assert (err <= bound).all()
    # every level reaches code 0, and 65533 unless it is constant
    flat = q.reshape(-1, x.shape[2])
    const = x.reshape(-1, x.shape[2]).min(axis=0) == x.reshape(-1, x.shape[2]).max(axis=0)
    assert (flat.min(axis=0) == 0).all() and (flat.max(axis=0)[~const] == R.TOP).all() and (scl[const] == 1).all()


def test_the_cases_hold_what_they_are_named_for():
    for nx, ny, nlev in K.GRIDS:
        tag = f"{nx}x{ny}x{nlev}"
        q, scl, off = R.encode(K.ENCODE["edges_" + tag])
        assert scl[0] == 1 and (q[:, :, 0] == 0).all() and off[0] == np.float32(273.15)
        assert q[0, 0, -1] == 0 and q[-1, -1, -1] == R.TOP and off[-1] == 150.0
        z = K.ENCODE["negative_" + tag]
        assert np.signbit(z[::2, :, 0]).all() and (z <= 0).all()
        q, scl, off = R.encode(z)
        assert scl[0] == 1 and off[0] == 0 and not np.signbit(off[0])
        h = K.ENCODE["halves_" + tag]
        q, scl, off = R.encode(h)
        assert (scl == 1).all() and (off == 0).all()
        r = (h.astype(np.float64) - off) / scl + .5
        inner = (h > 0) & (h < 65533)
        assert inner.any() and (r[inner] == np.floor(r[inner])).all() and (q[inner] == r[inner]).all()
        codes = K.DECODE["hand_" + tag][0]
        assert {0, 65533, 65534, 65535} <= set(codes.reshape(-1).tolist())


@pytest.mark.parametrize("name", sorted(K.DECODE))
def test_every_code_decodes_within_the_limits(name):
    q, scl, off, lo, hi = K.DECODE[name]
    v = R.decode(q, scl, off, lo, hi)
    assert v.dtype == np.float32 and not np.isnan(v).any()
    assert (v >= np.float32(lo)).all() and (v <= np.float32(hi)).all()
    if name.startswith("wild"):
        nlev = q.shape[2]
        assert (v[:, :, 0] == np.float32(lo)).all()             # scl NaN: a NaN becomes lo
        if nlev != 3:       # (three levels: the last one is the level whose off is -inf)
            assert (v[:, :, -1] == np.float32(hi)).all()        # off +inf: hi
        if nlev > 2:
            assert (v[:, :, 2] == np.float32(lo)).all()         # off -inf: lo
            assert set(np.unique(v[:, :, 1]).tolist()) <= {float(np.float32(lo)), float(np.float32(hi))}   # scl inf: q = 0 is a NaN


@pytest.mark.parametrize("name", sorted(K.NOT_FINITE))
def test_a_value_that_is_not_finite_is_refused_with_its_level(name):
    x, level = K.NOT_FINITE[name]
    with pytest.raises(R.NotFinite) as e:
        R.encode(x)
    assert e.value.level == level


def test_the_file_writer_lays_out_what_the_definition_says(tmp_path):
    from mptrac_amd.synth import synthetic_met
    met = synthetic_met("tiny", 3600.0, 1.0)
    raw = pf.met_pck_bytes(met)
    assert len(raw) == pf.file_size(met.nx, met.ny, met.np)
    assert struct.unpack_from("<iid", raw, 0) == (2, 104, 3600.0) and struct.unpack_from("<i", raw, len(raw) - 4) == (999,)
    # half the level-field bytes of the MET_TYPE 1 file, but for the scales and offsets
    path = str(tmp_path / "a.bin")
    hf.write_met_bin(path, met)
    assert os.path.getsize(path) - len(raw) == 13 * (2 * met.nx * met.ny * met.np - 16 * met.np)
    # the first level field (z) sits behind the header, the axes and 24 planes
    at = 28 + 8 * (met.nx + met.ny + met.np) + 24 * 4 * met.nx * met.ny
    q, scl, off = R.encode(pf.level_field(met, "z"))
    assert raw[at:at + 8 * met.np] == scl.tobytes() and raw[at + 16 * met.np:at + 16 * met.np + 2 * q.size] == q.tobytes()


# ---- the drivers, up to the point where a device or a file is needed ------------------------------------------------------

def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    return r.returncode, r.stdout.decode()


def _ctl(tmp, **keys):
    path = os.path.join(tmp, "trac.ctl")
    hf.write_ctl(path, dict({"NQ": 0, "METBASE": os.path.join(tmp, "met")}, **keys))
    return path


def test_met_conv_accepts_type_2_and_refuses_type_3(tmp_path):
    build.build_host()
    tmp = str(tmp_path)
    ctl = _ctl(tmp)
    absent, out_file = os.path.join(tmp, "absent.pck"), os.path.join(tmp, "out.bin")
    rc, out = _run([build.MET_CONV_BIN, ctl, absent, "2", out_file, "1"])
    assert rc != 0 and "Cannot open file" in out and "This build reads" not in out, out[-1500:]
    rc, out = _run([build.MET_CONV_BIN, ctl, absent, "3", out_file, "1"])
    assert rc != 0 and "This build reads MET_TYPE 0" in out and " 1 (" in out and " 2 (" in out, out[-1500:]
    # ... and on the writing side, behind a file that can be read without a device
    from mptrac_amd.synth import synthetic_met
    src = os.path.join(tmp, "in.bin")
    hf.write_met_bin(src, synthetic_met("tiny", 0.0, 1.0))
    rc, out = _run([build.MET_CONV_BIN, ctl, src, "1", out_file, "3"])
    assert rc != 0 and "This build writes MET_TYPE 0" in out and " 1 (" in out and " 2 (" in out, out[-1500:]
    assert not os.path.exists(out_file)


def test_trac_accepts_type_2_and_refuses_type_3_in_the_control_file(tmp_path):
    build.build_host()
    tmp = str(tmp_path)
    with open(os.path.join(tmp, "dirs"), "w") as f:
        f.write(tmp + "\n")
    _ctl(tmp, MET_TYPE=2, HIP_MET_PACKED=0)
    rc, out = _run([build.TRAC_BIN, os.path.join(tmp, "dirs"), "trac.ctl", "absent.tab"])
    assert rc != 0 and "Cannot open file" in out and "MET_TYPE" not in out.split("Error")[-1], out[-1500:]
    rc, out = _run([build.TRAC_BIN, os.path.join(tmp, "dirs"), "trac.ctl", "absent.tab", "HIP_MET_PACKED", "2"])
    assert rc != 0 and "HIP_MET_PACKED" in out.split("Error")[-1], out[-1500:]
    rc, out = _run([build.TRAC_BIN, os.path.join(tmp, "dirs"), "trac.ctl", "absent.tab", "MET_TYPE", "3"])
    last = out.split("Error")[-1]
    assert rc != 0 and "MET_TYPE 3" in last and all(w in last for w in ("0 (", "1 (", "2 (")), out[-1500:]
    # ADVECT_VERT_COORD 2 stays refused for type 2 as for type 1
    rc, out = _run([build.TRAC_BIN, os.path.join(tmp, "dirs"), "trac.ctl", "absent.tab", "ADVECT_VERT_COORD", "2"])
    assert rc != 0 and "requires meteo data on model levels" in out, out[-1500:]


def test_a_type_1_file_read_as_type_2_is_the_wrong_type(tmp_path):
    build.build_host()
    from mptrac_amd.synth import synthetic_met
    tmp = str(tmp_path)
    src = os.path.join(tmp, "in.bin")
    hf.write_met_bin(src, synthetic_met("tiny", 0.0, 1.0))
    rc, out = _run([build.MET_CONV_BIN, _ctl(tmp), src, "2", os.path.join(tmp, "out.bin"), "1"])
    assert rc != 0 and "Wrong MET_TYPE of binary data!" in out, out[-1500:]
    # ... and the version check stays
    raw = bytearray(pf.met_pck_bytes(synthetic_met("tiny", 0.0, 1.0)))
    raw[4:8] = struct.pack("<i", 103)
    with open(os.path.join(tmp, "old.pck"), "wb") as f:
        f.write(raw)
    rc, out = _run([build.MET_CONV_BIN, _ctl(tmp), os.path.join(tmp, "old.pck"), "2", os.path.join(tmp, "out.bin"), "1"])
    assert rc != 0 and "Wrong version of binary data!" in out, out[-1500:]
