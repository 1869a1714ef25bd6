"""module_tracer_chem without a device: the restatement's clim_photo (tests/reftracer.py) at the ends of its three axes and
with negative table entries, ARRHENIUS without an activation term, and the interface that carries the module -- the
hip-only ctl key, the module bit, the header's declarations and the route-A glue."""
import ctypes as C
import os
import re

import numpy as np

import reftracer
from mptrac_amd import hip
from mptrac_amd.ctl import CTL_FIELDS, HIP_CTL_FIELDS, HIP_ONLY_KEYS, fill_ctl, make_ctl_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _photo(values=None):
    p = np.array([100.0, 30.0, 10.0, 3.0])
    sza = np.array([0.2, 0.6, 1.0])
    o3c = np.array([250.0, 300.0, 350.0])
    rng = np.random.default_rng(3)
    tab = rng.uniform(1e-7, 1e-6, (4, 3, 3)) if values is None else values
    return reftracer.Photo(p, sza, o3c, {"ccl4": tab})


def test_clim_photo_clamps_at_every_axis_end():
    ph = _photo()
    inner = dict(p=20.0, sza=0.7, o3c=310.0)
    ends = [("p", 1e4, 100.0, 90.0), ("p", 0.01, 3.0, 3.5), ("sza", 0.0, 0.2, 0.25), ("sza", 3.0, 1.0, 0.95),
            ("o3c", 100.0, 250.0, 255.0), ("o3c", 500.0, 350.0, 345.0)]
    for axis, beyond, end, inward in ends:
        a = ph.rate("ccl4", **dict(inner, **{axis: beyond}))
        b = ph.rate("ccl4", **dict(inner, **{axis: end}))
        assert a == b, (axis, beyond)
        assert ph.rate("ccl4", **dict(inner, **{axis: inward})) != a, axis      # (the clamp, not a flat table)
    # every corner of the table clamps to its node
    r = ph.rates["ccl4"]
    for ip, pv in ((0, 1e4), (3, 0.01)):
        for iz, zv in ((0, -1.0), (2, 4.0)):
            for io, ov in ((0, 0.0), (2, 1e3)):
                assert abs(ph.rate("ccl4", pv, zv, ov) - r[ip, iz, io]) <= 1e-15 * r[ip, iz, io]   # (LIN at x1: an ulp)


def test_clim_photo_interpolates_and_hits_the_nodes():
    ph = _photo()
    r = ph.rates["ccl4"]
    for ip in range(4):
        for iz in range(3):
            for io in range(3):
                assert abs(ph.rate("ccl4", ph.p[ip], ph.sza[iz], ph.o3c[io]) - r[ip, iz, io]) <= 1e-15 * r[ip, iz, io]
    # trilinear: the mean of a cell's eight nodes at the centre (pressure: linear in p)
    c = ph.rate("ccl4", 0.5 * (ph.p[1] + ph.p[2]), 0.8, 325.0)
    assert abs(c - r[1:3, 1:3, 1:3].mean()) <= 1e-14 * c


def test_clim_photo_is_never_negative():
    neg = -np.ones((4, 3, 3)) * 1e-7
    ph = _photo(neg)
    for args in ((20.0, 0.7, 310.0), (1e4, 0.0, 0.0), (3.0, 1.0, 350.0)):
        assert ph.rate("ccl4", *args) == 0.0
    mixed = np.ones((4, 3, 3)) * 1e-7
    mixed[:, 1:, :] = -3e-7              # positive at sza[0], negative beyond: the zero crossing lies inside (0.2, 0.6)
    ph = _photo(mixed)
    assert ph.rate("ccl4", 20.0, 0.25, 300.0) > 0
    assert ph.rate("ccl4", 20.0, 0.5, 300.0) == 0.0
    assert ph.rate("ccl4", 20.0, 0.9, 300.0) == 0.0


def test_arrhenius_without_activation_is_the_factor():
    for mode in ("numpy", "libm"):
        for t in (180.0, 215.3, 300.0):
            for name in ("Cccl4", "Cccl3f"):
                a, b = reftracer.ARRHENIUS[name]
                assert b == 0 and reftracer.arrhenius(a, b, t, mode) == a
            a, b = reftracer.ARRHENIUS["Cccl2f2"]
            assert reftracer.arrhenius(a, b, t, mode) > a           # b < 0: faster when colder


def test_restatement_leaves_dt_zero_and_sf6_alone():
    ph = reftracer.synthetic_photo(1)
    n = 6
    q = np.full((3, n), 1e-10)
    idx = {"Cccl4": 0, "Csf6": 1, "Cn2o": -1}
    dt = np.array([180.0, 0.0, 180.0, 0.0, -180.0, 180.0])
    z = np.zeros(n)
    out = reftracer.apply(q.copy(), idx, ph, z + 1800.0, z + 10.0, np.linspace(-170, 170, n), z + 10.0, z + 220.0,
                          z + 1e-13, z + 300.0, dt)
    assert np.array_equal(out[1:], q[1:])
    assert np.array_equal(out[0, dt == 0], q[0, dt == 0])
    assert np.all(out[0, dt > 0] < q[0, dt > 0]) and np.all(out[0, dt < 0] > q[0, dt < 0])   # (dt < 0: backward)


def test_ctl_key_is_hip_only_and_appended():
    names = [n for n, _, _ in HIP_CTL_FIELDS]
    assert names[-2:] == ["tracer_chem", "pad5"]
    assert "tracer_chem" in HIP_ONLY_KEYS
    assert "tracer_chem" not in [n for n, _, _ in CTL_FIELDS]      # (the oracle's struct is CTL_FIELDS alone)
    Old = make_ctl_struct("Old", HIP_CTL_FIELDS[:-2])
    assert hip.MphipCtl.tracer_chem.offset == C.sizeof(Old)       # every earlier member keeps its offset
    for n, _, _ in HIP_CTL_FIELDS[:-2]:
        assert getattr(hip.MphipCtl, n).offset == getattr(Old, n).offset
    c = fill_ctl(hip.MphipCtl(), tracer_chem=1)
    assert c.tracer_chem == 1 and fill_ctl(hip.MphipCtl()).tracer_chem == 0
    assert hip.MOD["tracer_chem"] == 1 << 24
    assert hasattr(hip.Simulation, "update_clim_photo")


def test_header_declares_the_module_and_the_upload():
    txt = open(os.path.join(ROOT, "include", "mptrac_hip.h")).read()
    assert re.search(r"MPHIP_MOD_TRACER_CHEM\s*=\s*1\s*<<\s*24", txt)
    body = txt[txt.index("typedef struct {", txt.index("Hot-path subset of ctl_t")):txt.index("} mphip_ctl_t;")]
    assert re.search(r"int tracer_chem;\s*int pad5;\s*$", body)
    assert re.search(r"int mphip_update_clim_photo\(mphip_ctx \*ctx, int np, int nsza, int no3c, const double \*p,\s*"
                     r"const double \*sza,\s*const double \*o3c, const double \*const rate\[MPHIP_NTR\]\);", txt)


def test_glue_hands_over_the_module():
    glue = open(os.path.join(ROOT, "integration", "mptrac_hip_glue.c")).read()
    assert "X(tracer_chem)" in glue
    assert "mphip_update_clim_photo(" in glue and "clim->photo" in glue
    refusal = re.search(r"if \(([^)]*)\)\s*ERRMSG\(\"MPTRAC_HIP: KPP", glue)
    assert refusal and "tracer_chem" not in refusal.group(1)
    assert "kpp_chem" in refusal.group(1) and "radio_decay" in refusal.group(1)
