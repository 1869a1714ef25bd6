"""The control keys of the regridding in mptrac_read_ctl (no device needed: the control file is read first): what
HIP_MET_PREP >= 1 accepts for netCDF input, what stays refused, and that a refusal without HIP_MET_PREP names the key."""
import os
import subprocess

import pytest

import hostfiles as hf
from mptrac_amd import build

MET_P = (900.0, 700.0, 500.0, 300.0)


def _met_conv(tmp, *extra, model_levels=True, prep=1):
    build.build_host()
    keys = {"NQ": 0, "METBASE": os.path.join(tmp, "met"), "MET_TYPE": 0, "HIP_MET_PREP": prep}
    if model_levels:
        keys.update({"MET_VERT_COORD": 1, "MET_NP": len(MET_P)})
        keys.update({"MET_P[%d]" % i: p for i, p in enumerate(MET_P)})
    hf.write_ctl(os.path.join(tmp, "trac.ctl"), keys)
    r = subprocess.run([build.MET_CONV_BIN, os.path.join(tmp, "trac.ctl"), os.path.join(tmp, "absent_2022_06_02_00.nc"), "0",
                        os.path.join(tmp, "out.bin"), "1", *extra], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    return r.returncode, r.stdout.decode()


@pytest.mark.parametrize("extra,model_levels", [((), True), (("ADVECT_VERT_COORD", "2"), True), (("MET_DX", "2", "MET_SP", "3"), True),
                                                (("MET_DX", "2", "MET_DY", "2", "MET_SX", "2", "MET_SY", "2"), False)])
def test_accepted_with_hip_met_prep(tmp_path, extra, model_levels):
    """The control file passes: the tool goes on to the file, which is absent."""
    rc, out = _met_conv(str(tmp_path), *extra, model_levels=model_levels)
    assert "Cannot open file" in out and "not part of this build" not in out, out[-1500:]


@pytest.mark.parametrize("extra,model_levels,words", [
    (("HIP_MET_PREP", "0"), True, ("MET_VERT_COORD", "HIP_MET_PREP")),
    (("HIP_MET_PREP", "0", "MET_NP", "4"), False, ("MET_NP", "HIP_MET_PREP")),
    (("HIP_MET_PREP", "0", "MET_DX", "2"), False, ("MET_DX", "HIP_MET_PREP")),
    (("HIP_MET_PREP", "0", "MET_SP", "2"), False, ("MET_SP", "HIP_MET_PREP")),
    (("MET_VERT_COORD", "2"), True, ("MET_VERT_COORD", "not part of this build")),
    (("MET_VERT_COORD", "0"), True, ("MET_NP needs MET_VERT_COORD 1",)),
    (("MET_NP", "1"), True, ("2 <= MET_NP",)),
    (("MET_NP", "1000"), True, ("2 <= MET_NP",)),
    (("MET_P[2]", "800"), True, ("strictly descending",)),
    (("MET_P[3]", "-1"), True, ("strictly descending",)),
    (("MET_DX", "0"), False, ("MET_DX must be",)),
    (("MET_DETREND", "5"), False, ("MET_DETREND", "not part of this build")),
    (("MET_CLAMS", "1"), False, ("MET_CLAMS", "not part of this build")),
    (("MET_CONVENTION", "1"), False, ("MET_CONVENTION", "not part of this build")),
    (("MET_RELHUM", "1"), False, ("MET_RELHUM", "not part of this build")),
    (("ADVECT_VERT_COORD", "2"), False, ("requires meteo data on model levels",)),
    (("ADVECT_VERT_COORD", "2", "MET_TYPE", "1"), True, ("requires meteo data on model levels",)),
    (("ADVECT_VERT_COORD", "2", "MET_DX", "2"), True, ("MET_DX", "not sampled")),
    (("ADVECT_VERT_COORD", "2", "MET_SY", "2"), True, ("MET_SY", "not sampled")),
    (("ADVECT_VERT_COORD", "1", "QNT_NAME[0]", "zeta", "NQ", "1"), True, ("diabatic",)),
    (("ADVECT_VERT_COORD", "3", "QNT_NAME[0]", "eta", "NQ", "1"), True, ("etadot",))])
def test_refused(tmp_path, extra, model_levels, words):
    rc, out = _met_conv(str(tmp_path), *extra, model_levels=model_levels)
    assert rc != 0 and "Error" in out and all(w in out for w in words), out[-1500:]
