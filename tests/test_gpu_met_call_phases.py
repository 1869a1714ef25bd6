"""The event pairs mphip_profile_begin / _end count in each of the six meteo calls, per value of the option
derive_profile_phase the call uses: what tools/gpu_*_cost.py read as launches, uploads and downloads.

A pair brackets one kernel (phase 0), all uploads of the call (1), all its downloads (2), the host's weight table of
mphip_detrend_met (3), or one of the three kernels of mphip_pack_met alone (4, 5, 6).  The counts below are literals, each
with its derivation from the call's code; nothing is recorded outside begin / end.  The grids are tiny: the counts depend
on which fields and stages a call has, not on its extents.  The values of the calls are what tests/test_gpu_metprep.py,
test_gpu_pv_tropo.py, test_gpu_regrid.py, test_gpu_detrend.py, test_gpu_ingest.py and test_gpu_pack.py assert."""
import numpy as np
import pytest

import detrend_cases as D
import ingest_cases as I
import metprep_cases as P
import pack_cases as Q
import regrid_cases as K
from mptrac_amd.hip import Snapshot
from test_gpu_metprep import bare_context, with_clim

pytestmark = pytest.mark.gpu


def derive_every_bit(sim):
    """3 x 5 x 3 (PV needs five rows, the WMO tropopause three levels), smoothing on."""
    sim.derive_met(P.pv_shape(3, 5, 3), ("geopot", "o3c", "pbl", "cloud", "cape", "pv", "tropo"), met_geopot_sx=2,
                   met_geopot_sy=2, met_pbl=3, met_tropo=3)


def regrid_ml2pl_sample(sim):
    """5 x 4 x 6 model levels to 6 pressure levels, then every second column: n3 = 2 level fields (t, u; pl is the
    pressure, not a field of the call), n2 = 3 surface fields (ps, zs, ts)."""
    got = sim.regrid_met(K.ml_atmosphere(5, 4, 6, fields=("t", "u")), ("ml2pl", "sample"), met_p=K.targets(6), met_dx=2,
                         met_sx=2)
    assert (sorted(got.f3), sorted(got.f2)) == (["t", "u"], ["ps", "ts", "zs"])


def detrend_smallest(sim):
    met, scale = D.case("smallest")
    sim.detrend_met(met, scale)


def ingest_all_stages(sim):
    """2 x 2 x 2, seven raw fields (t, u, v, w, h2o, ps, zs), both poles, a periodic longitude axis."""
    c = I.CASES["shape_2x2x2_short"]
    axes = Snapshot(0.0, c["coord_type"], np.ascontiguousarray(c["lon"]), np.ascontiguousarray(c["lat"]),
                    np.ascontiguousarray(c["p"]), {}, {})
    got = sim.ingest_met(c["raw"], axes, ("decode", "extrapolate", "polar", "periodic"))
    assert len(c["raw"]) == 7 and got.f3["u"].shape == (3, 2, 2) and abs(got.lat[0]) == abs(got.lat[-1]) == 90.0


def _grid_2x2x2():
    return Snapshot(0.0, 0, np.arange(2, dtype=np.float64), np.arange(2, dtype=np.float64), np.arange(2, 0, -1.0), {}, {})


def unpack_two_fields(sim):
    sim.unpack_met(_grid_2x2x2(), {"t": Q.DECODE["hand_t_2x2x2"], "u": Q.DECODE["hand_2x2x2"]})


def pack_two_fields(sim):
    met = _grid_2x2x2()
    met.f3.update(t=Q.ENCODE["smooth_2x2x2"], u=Q.ENCODE["negative_2x2x2"])
    sim.pack_met(met)


# call: {phase: pairs}
PAIRS = {
    # 0: prep_geopot, prep_smooth, prep_o3c, prep_cloud, prep_pbl, prep_cape, prep_pv with prep_pv_polar (one pair around
    #    the field and its polar rows), prep_tropo = 8;  1: one pair around every upload;  2: one around every download
    derive_every_bit: {0: 8, 1: 1, 2: 1},
    # 0: regrid_ml2pl once for all level fields, then regrid_sample per level field and per surface field:
    #    1 + n3 + n2 = 1 + 2 + 3
    regrid_ml2pl_sample: {0: 6, 1: 1, 2: 1},
    # 0: detrend_kernel;  3: the pair around the host's weight table
    detrend_smallest: {0: 1, 1: 1, 2: 1, 3: 1},
    # 0: ingest_decode per raw field (7), ingest_extrapolate (1), ingest_polar per pole (2), ingest_periodic (1)
    ingest_all_stages: {0: 11, 1: 1, 2: 1},
    # 0: met_unpack per field
    unpack_two_fields: {0: 2, 1: 1, 2: 1},
    # 0: met_pack_extremes, met_pack_reduce and met_pack_quantise per field: 3 nf;  4, 5, 6: one of the three per field
    pack_two_fields: {0: 6, 1: 1, 2: 1, 4: 2, 5: 2, 6: 2},
}
CASES = [(call, phase) for call, phases in PAIRS.items() for phase in phases]


@pytest.fixture(scope="module")
def sim():
    s = with_clim(bare_context())
    yield s
    s.close()


@pytest.mark.parametrize("call,phase", CASES, ids=[f"{call.__name__}-phase{phase}" for call, phase in CASES])
def test_pairs_per_phase(sim, call, phase):
    try:
        sim.set_option("derive_profile_phase", phase)
        sim.profile_begin()
        call(sim)
        pairs, ms = sim.profile_end()
        print(f"{call.__name__} phase {phase}: {pairs} pairs, {ms:.4f} ms")
        assert pairs == PAIRS[call][phase] and ms >= 0.0, (pairs, ms)
        call(sim)                                # (outside begin / end nothing is recorded)
        sim.profile_begin()
        assert sim.profile_end()[0] == 0
    finally:
        sim.set_option("derive_profile_phase", 0)
