"""module_radio_decay without a device: the restatement (tests/refradio.py) on its own -- dt = 0, exactness of the
Bateman solution over split steps, Pb-210 ingrowth against the closed form, the two arithmetic modes -- and the
interface that carries the module: the header's declarations, both libraries' exports, the Python binding and the name
helper."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import refradio
from mptrac_amd import build, ctl as ctlmod, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = len(refradio.NAMES)


def _state(n=2000, seed=5, decades=(-2.0, 6.0)):
    rng = np.random.default_rng(seed)
    q = np.empty((N + 2, n))
    q[0] = rng.uniform(1e6, 1e9, n)            # an untouched quantity in row 0 (m)
    q[1:N + 1] = 10.0 ** rng.uniform(*decades, (N, n))
    q[N + 1] = rng.uniform(0, 1, n)            # ... and one behind the activities
    return q, list(range(1, N + 1))


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))


def test_header_declares_the_module():
    with open(os.path.join(ROOT, "include", "mptrac_hip.h")) as f:
        h = f.read()
    assert re.search(r"MPHIP_MOD_RADIO_DECAY\s*=\s*1\s*<<\s*25", h)
    assert re.search(r"MPHIP_RN_RN222\s*=\s*0,\s*MPHIP_RN_PB210,\s*MPHIP_RN_BE7,\s*MPHIP_RN_CS137,\s*MPHIP_RN_I131,"
                     r"\s*MPHIP_RN_XE133,\s*MPHIP_NRADIO", h)
    assert re.search(r"int\s+mphip_set_radio_decay\s*\(\s*mphip_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*,\s*const\s+int\s+"
                     r"qnt\s*\[\s*MPHIP_NRADIO\s*\]\s*\)\s*;", h)
    # the activity order of the header is the restatement's and the binding's
    assert refradio.NAMES == ctlmod.RADIO_ACTIVITIES


def test_module_bit_does_not_pick_another_step_instantiation():
    """the public bit is kGated's; the step kernel masks carry an internal bit of the tail instead"""
    with open(os.path.join(ROOT, "mptrac_amd", "csrc", "mphip_kernels.hpp")) as f:
        k = f.read()
    m = re.search(r"constexpr unsigned kRadioDecay = 1u << (\d+);", k)
    assert m
    bit = 1 << int(m.group(1))
    flags = {}
    for name in ("kTwoStage", "kGated", "kMultiStep", "kMLWinds", "kBigGrid", "kPblClosure", "kEmitKeys", "kStoreDt"):
        f_ = re.search(r"constexpr unsigned %s = 1u << (\d+);" % name, k)
        flags[name] = 1 << int(f_.group(1))
    assert all(bit != v for v in flags.values()), flags
    assert bit not in set(hip.MOD.values())
    assert re.search(r"kTailModules = [^;]*kRadioDecay", k)


def test_both_libraries_export_the_entry_point():
    for path in build.build_hip_both():
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT mphip_set_radio_decay\b", out), path


def test_python_binding_and_name_helper():
    assert hip.MOD["radio_decay"] == 1 << 25
    assert callable(getattr(hip.Simulation, "set_radio_decay"))
    names = ("m", "Abe7", "vmr", "Arn222", "Apb210", "Axe133")
    assert ctlmod.radio_from_quantities(names) == (3, 4, 1, -1, -1, 5)
    assert ctlmod.radio_from_quantities(("m",)) == (-1,) * N
    # the ctl dicts stay as they are: the activities are not control parameters
    out = ctlmod.ctl_from_quantities(names)
    assert set(out) == {"nq", "qnt_m", "qnt_vmr"}


def test_dt_zero_leaves_everything():
    q, idx = _state()
    dt = np.zeros(q.shape[1])
    for mode in ("numpy", "libm"):
        r = refradio.apply(q.copy(), idx, dt, mode)
        assert np.array_equal(r, q)
    # mixed: the dt = 0 columns keep their bits, the others decay
    dt[::3] = 3600.0
    r = refradio.apply(q.copy(), idx, dt)
    assert np.array_equal(r[:, dt == 0], q[:, dt == 0])
    assert np.all(r[1:N + 1, dt != 0] != q[1:N + 1, dt != 0])
    assert np.array_equal(r[[0, N + 1]], q[[0, N + 1]])


@pytest.mark.parametrize("dt", [3600.0, -3600.0, 86400.0 * 30])
def test_two_half_steps_are_one_full_step(dt):
    """the Bateman solution is exact: two steps of dt / 2 give one step of dt (to rounding).  Activities within a
    decade of each other: a Pb-210 activity far below the Rn-222 ingrowth of a backward step is a difference of
    nearly equal terms (ill-conditioned, whatever the formula)"""
    q, idx = _state(decades=(0.0, 1.0))
    d = np.full(q.shape[1], dt)
    one = refradio.apply(q.copy(), idx, d)
    two = refradio.apply(refradio.apply(q.copy(), idx, d / 2), idx, d / 2)
    assert _rel(two, one) <= 1e-14
    assert np.array_equal(one[[0, N + 1]], q[[0, N + 1]])


def test_pb210_ingrowth_from_pure_radon():
    """pure Rn-222 (no Pb-210) after one Rn-222 half-life: half of it left, Pb-210 as the closed form has it"""
    a0 = 1e6
    T = refradio.HALF_LIFE[refradio.RN]
    q = np.array([[a0], [0.0]])
    r = refradio.apply(q.copy(), [0, 1, -1, -1, -1, -1], np.array([T]))
    assert abs(r[0, 0] - a0 / 2) <= 1e-14 * a0
    pb = refradio.pb_ingrowth_closed_form(a0, T)
    assert abs(r[1, 0] - pb) <= 1e-12 * pb
    # the ingrowth is small (Pb-210 lives ~2000 times as long) but present: activity ratio lambda_pb / lambda_rn / 2
    ratio = refradio.HALF_LIFE[refradio.RN] / refradio.HALF_LIFE[refradio.PB]
    assert abs(r[1, 0] / a0 - 0.5 * ratio) <= 0.01 * 0.5 * ratio
    # without Rn-222 Pb-210 only decays
    r = refradio.apply(np.array([[a0]]), [-1, 0, -1, -1, -1, -1], np.array([T]))
    assert r[0, 0] == a0 * math.exp(-refradio.LAMBDA[refradio.PB] * T)


def test_each_nuclide_decays_by_its_half_life():
    for k in range(N):
        idx = [-1] * N
        idx[k] = 0
        r = refradio.apply(np.array([[1.0]]), idx, np.array([refradio.HALF_LIFE[k]]))
        assert abs(r[0, 0] - 0.5) <= 1e-15, refradio.NAMES[k]


def test_numpy_and_libm_modes_agree():
    q, idx = _state(n=3000, seed=9)
    rng = np.random.default_rng(9)
    dt = rng.choice([-3600.0, -600.0, 0.0, 60.0, 600.0, 3600.0, 86400.0], q.shape[1])
    a = refradio.apply(q.copy(), idx, dt, "numpy")
    b = refradio.apply(q.copy(), idx, dt, "libm")
    assert _rel(a, b) <= 1e-15


def test_constants_table():
    """one table: the half-lives of evaluated nuclear data, in seconds; device code holds the same numbers"""
    d, y = 86400.0, 365.25 * 86400.0
    assert refradio.HALF_LIFE == (3.8235 * d, 22.20 * y, 53.22 * d, 30.08 * y, 8.0252 * d, 5.2475 * d)
    with open(os.path.join(ROOT, "mptrac_amd", "csrc", "mphip_device.hpp")) as f:
        src = f.read()
    m = re.search(r"kRadioHalfLife\[MPHIP_NRADIO\] = \{([^}]*)\}", src)
    assert m
    vals = [v.strip() for v in m.group(1).split(",")]
    assert vals == ["3.8235 * kRadioDay", "22.20 * kRadioYear", "53.22 * kRadioDay", "30.08 * kRadioYear",
                    "8.0252 * kRadioDay", "5.2475 * kRadioDay"]
