"""tests/reftropo.py, the restatement of potential vorticity and the tropopause that the GPU tests compare with, against
independent knowledge: a library spline, analytic profiles, and the conditions the GPU comparison rests on (no branch
decided by less than 1e-9; finite and NaN columns side by side where the GPU test says it sees both).  Also the layout of
mphip_prep_t's Python mirror."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import reftropo as T      # noqa: E402

GRIDS = [(9, 7, 20), (37, 19, 20), (5, 5, 137)]
SEED = 2024


def test_spline_is_the_natural_cubic_spline():
    interpolate = pytest.importorskip("scipy.interpolate")
    rng = np.random.default_rng(5)
    for n in (3, 4, 7, 20, 137):
        x = np.cumsum(rng.uniform(0.05, 2.5, n))
        y = rng.normal(220., 30., n)
        x2 = np.sort(rng.uniform(x[0], x[-1], 300))
        want = interpolate.CubicSpline(x, y, bc_type="natural")(x2)
        got = np.array(T.spline(x.tolist(), y.tolist(), x2.tolist(), 1))
        assert np.abs(got - want).max() <= 1e-11, n      # (absolute, on values near 220: measured 2.3e-13)


@pytest.mark.parametrize("method", [0, 1])
def test_spline_through_a_line_is_the_line_and_the_ends_clamp(method):
    rng = np.random.default_rng(6)
    x = np.cumsum(rng.uniform(0.1, 2., 12)).tolist()
    y = [250. - 6.5 * v for v in x]
    inside = np.linspace(x[0], x[-1], 57).tolist()
    got = T.spline(x, y, inside, method)
    assert np.abs(np.array(got) - (250. - 6.5 * np.array(inside))).max() < 1e-11
    out = T.spline(x, y, [x[0] - 3., x[0], x[-1], x[-1] + 5.], method)
    assert out == [y[0], y[0], y[-1], y[-1]]


def _analytic_column(dz, n):
    zlev = [dz * (k + 1) for k in range(n)]      # (a level at 12 km: the kink is a node)
    p = [T.P(z) for z in zlev]
    t = [288. - 6.5 * min(z, 12.) for z in zlev]
    return p, [T.Z(x) for x in p], t


@pytest.mark.parametrize("method,dz,n", [(0, 0.5, 60), (0, 0.1, 300), (1, 0.1, 300)])
def test_wmo_tropopause_of_an_analytic_profile(method, dz, n):
    """6.5 K/km up to 12 km and isothermal above: the first fine point from which the lapse rate to each of the next twenty
    stays at or below 2 K/km is the one at 12.0 km.  (The cubic spline rounds the kink off over a level spacing, so for it
    the levels are as fine as the fine grid.)"""
    p, zc, t = _analytic_column(dz, n)
    pt = T.tropo_pt(3, method, zc, p, t, None, T.Margin())
    assert pt == T.P2[75] and abs(T.Z2[75] - 12.0) < 1e-12
    # ... and without a second lapse-rate layer there is no second tropopause
    assert math.isnan(T.tropo_pt(4, method, zc, p, t, None, T.Margin()))


def test_pv_of_an_isothermal_atmosphere_at_rest():
    n, t0 = 12, 230.
    lat = [41., 43., 45., 47., 49.]
    lon = [0., 2., 4.]
    p = [900. * math.exp(-0.3 * k) for k in range(n)]
    t = [[[t0] * n for _ in lat] for _ in lon]
    zero = [[[0.] * n for _ in lat] for _ in lon]
    pv, S = T.pv_field(lon, lat, p, t, zero, zero)
    f = 2 * 2 * math.pi / 86400. * math.sin(math.radians(45.))
    assert abs(f - 2 * 7.2722052e-5 * math.sqrt(0.5)) < 1e-12      # twice the rotation rate of a solar day times sin 45 deg
    theta = [t0 * (1000. / p[k]) ** 0.286 for k in range(n)]
    pa = [100. * x for x in p]               # Pa
    for k in range(n):
        # the definition's difference quotient of theta, written out here on pressures in Pa: the three-point formula on an
        # uneven axis in the interior, the one-sided quotient at the two ends
        if 0 < k < n - 1:
            a, b = pa[k] - pa[k - 1], pa[k + 1] - pa[k]
            dthdp = (a * a * theta[k + 1] - b * b * theta[k - 1] + (b * b - a * a) * theta[k]) / (a * b * (a + b))
        elif k == 0:
            dthdp = (theta[1] - theta[0]) / (pa[1] - pa[0])
        else:
            dthdp = (theta[n - 1] - theta[n - 2]) / (pa[n - 1] - pa[n - 2])
        want = -1e6 * T.G0 * dthdp * f
        assert abs(pv[1, 2, k] - want) <= 1e-12 * abs(want) + 0.5 * float(np.spacing(np.float32(abs(want)))), k
        assert pv[1, 2, k] > 0 and abs(S[1, 2, k] - pv[1, 2, k]) <= 1e-6 * S[1, 2, k]
        if 0 < k < n - 1:
            # ... and that quotient is the analytic d theta / d p to a few per cent on an axis with p[k+1] / p[k] = 0.74
            exact = -0.286 * t0 * (1000. / p[k]) ** 0.286 / (100. * p[k])
            assert abs(dthdp - exact) < 0.05 * abs(exact), k
    # the rows next to the ends copy rows 2 and ny - 3 (here the same row)
    assert (pv[:, 0] == pv[:, 2]).all() and (pv[:, 1] == pv[:, 2]).all() and (pv[:, 3] == pv[:, 2]).all() and (pv[:, 4] == pv[:, 2]).all()


def _cases():
    for grid in GRIDS:
        for desc in (False, True):
            for mode in (1, 2, 3, 4, 5):
                for method in (0, 1):
                    yield grid + (SEED, desc), mode, method, False
            for method in (0, 1):
                yield grid + (SEED, desc), 4, method, True


def test_no_branch_is_decided_by_less_than_1e_9():
    """The condition under which the default library (double results an ulp or two off) takes the restatement's branches."""
    for key, mode, method, second in _cases():
        _, margin = T.tropo_reference(key, mode, method, second)
        assert margin.min() >= 1e-9, (key, mode, method, second, margin.min())


def test_mode_4_finds_second_tropopauses_in_some_columns_only():
    for grid in GRIDS:
        for method in (0, 1):
            out, _ = T.tropo_reference(grid + (SEED, False), 4, method, True)
            nan = int(np.isnan(out["pt"]).sum())
            assert 0 < nan < out["pt"].size, (grid, method, nan)
            for f in ("tt", "zt", "h2ot"):
                assert np.array_equal(np.isnan(out[f]), np.isnan(out["pt"]))


def test_cold_point_is_missing_in_some_columns_only():
    for method in (0, 1):
        out, _ = T.tropo_reference((37, 19, 20, SEED, False), 2, method)
        nan = int(np.isnan(out["pt"]).sum())
        assert 0 < nan < 37 * 19, (method, nan)


def test_wmo_and_dynamical_tropopause_are_found_everywhere():
    for grid in GRIDS:
        for mode in (3, 5):
            out, _ = T.tropo_reference(grid + (SEED, False), mode, 1)
            assert np.isfinite(out["pt"]).all() and np.isfinite(out["zt"]).all(), (grid, mode)


def test_prep_structure_keeps_the_old_offsets_and_its_size():
    from mptrac_amd import hip
    old = [("met_pbl", C.c_int), ("met_pbl_min", C.c_double), ("met_pbl_max", C.c_double), ("met_geopot_sx", C.c_int),
           ("met_geopot_sy", C.c_int), ("met_cloud_min", C.c_double)]

    class Old(C.Structure):
        _fields_ = old
    for name, _ in old:
        assert getattr(hip.MphipPrep, name).offset == getattr(Old, name).offset, name
    names = [f[0] for f in hip.MphipPrep._fields_]
    assert names[len(old):] == ["met_tropo", "met_tropo_pv", "met_tropo_theta", "met_tropo_spline"]
    assert hip.MphipPrep.met_tropo.offset == C.sizeof(Old)
    assert hip.PREP["pv"] == 32 and hip.PREP["tropo"] == 64
    L = hip.load()
    L.mphip_sizeof_prep.restype = C.c_size_t
    assert L.mphip_sizeof_prep() == C.sizeof(hip.MphipPrep)
