"""The table of module_diff_meso's wind deviations (DevMet::meso, meso_table_kernel): {sd_u, sd_v, sd_w} per raw grid
cell, built from the packed wind records when they are packed and read by the lean step kernels with 32-bit offsets
instead of summing the cell's 16 wind values per particle and step.  The general kernels (option generic_kernel 1) keep
the sums and are the yardstick: every comparison is array_equal on time, lon, lat, p, every quantity and uvwp.

Grids: A = (9, 6, 5): 9 x 5 x 4 cells, no axis a multiple of the brick edge 4; B = (3, 4, 3): fewer than four cells on
every axis (and, for the table alone, (1, 2, 2): one cell, the smallest grid mphip_update_met accepts); C = "tiny".
Particles: 3000 seeded ones, the first of them replaced by hand-placed ones -- the last longitude cell and the periodic
column, grid lines of all three axes, the pole rows, the top and bottom level intervals, above the top and below the
lowest level.

Break checks, each tried once on a scratch copy of the sources (profiles/r08_meso_table_ab.txt lists what failed): the
table not rebuilt at a hand-over, the brick count along iy rounded down, met1 summed before met0.
"""
import numpy as np
import pytest

import backward
import cases
from mptrac_amd import hip
from mptrac_amd.synth import synthetic_met

pytestmark = pytest.mark.gpu

GRID_A, GRID_B, GRID_ONE_CELL, GRID_C = (9, 6, 5), (3, 4, 3), (1, 2, 2), "tiny"
GRIDS = {"A": GRID_A, "B": GRID_B, "C": GRID_C}
N = 3000
STATE = ("time", "lon", "lat", "p", "q", "uvwp")
DT = cases.BASE["dt_mod"]
MOVERS = ("timesteps", "diff_turb", "diff_meso", "convection", "sedi", "position2")


def _place(atm, met):
    """hand-placed particles in the first slots"""
    lon, lat, p = met.lon, met.lat, met.p      # (p descends: p[0] is the lowest level)

    def mid(a, i):
        return 0.5 * (a[i] + a[i + 1])

    ny, npl = len(lat), len(p)
    lat_in, p_in = mid(lat, ny // 2 - 1) + 0.3, mid(p, npl // 2 - 1)
    pts = [
        (mid(lon, len(lon) - 2), lat_in, p_in),                   # the last longitude cell
        (lon[-1], lat_in, p_in), (lon[-1], lat[1], p[1]),         # the periodic column
        (lon[0], lat_in, p_in), (np.nextafter(lon[-1], 0.0), lat_in, p_in),
        (lon[1], lat_in, p_in), (mid(lon, 0), lat[1], p_in), (mid(lon, 0), lat_in, p[1]),      # grid lines, one axis each
        (lon[1], lat[1], p[1]), (lon[len(lon) - 2], lat[ny - 2], p[npl - 2]),                  # ... and all three at once
        (mid(lon, 1), lat[0] + 0.1 * (lat[1] - lat[0]), p_in),                                 # the pole rows
        (mid(lon, 1), lat[-1] - 0.1 * (lat[-1] - lat[-2]), p_in),
        (mid(lon, 0), lat[0], p_in), (mid(lon, 0), lat[-1], mid(p, 0)),
        (mid(lon, 0), lat_in, mid(p, 0)), (mid(lon, 1), lat_in, mid(p, npl - 2)),              # bottom and top intervals
        (mid(lon, 0), lat_in, p[0]), (mid(lon, 1), lat_in, p[-1]),
        (mid(lon, 0), lat_in, 0.6 * p[-1]), (mid(lon, 1), lat[1], 0.6 * p[-1]),                # above the top level
        (mid(lon, 0), lat_in, 1.02 * p[0]), (lon[-1], lat[-1] - 0.1 * (lat[-1] - lat[-2]), 1.02 * p[0]),   # below the lowest
    ]
    for i, (x, y, z) in enumerate(pts):
        atm["lon"][i], atm["lat"][i], atm["p"][i] = x, y, z
    return atm


def _inputs(case, grid, direction=1, **over):
    if direction == 1:
        ctl, clim, m0, m1, atm = cases.make_case(case, n=N, grid=grid)
    else:
        ctl, clim, mets, atm = backward.backward_case(case, N, grid=grid)
        m0, m1 = mets
    ctl = dict(ctl, **over)
    return ctl, clim, m0, m1, _place(atm, m0)


def _same(a, b, what=""):
    for k in STATE:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, int(np.count_nonzero(a[k] != b[k])))


def _steps(s, n=6):
    for t in cases.step_times(s.ctl)[:n]:
        s.run_timestep(t)


def _movers(s, n=3):
    """the movers behind module_advect as one call of the C ABI, with the dt module_timesteps stored: the lean
    instantiation that runs module_diff_meso without an advection in front of it (no cached corners)"""
    times = cases.step_times(s.ctl)
    for t in times[1:1 + n]:
        s._chk(s.L.mphip_module(s.h, sum(hip.MOD[m] for m in MOVERS), t))


def _lean_and_general(inputs, run, options=()):
    ctl, clim, m0, m1, atm = inputs
    out = []
    for generic in (0, 1):
        s = hip.Simulation(ctl, clim, m0, m1, atm)
        try:
            s.set_option("generic_kernel", generic)
            for k, v in options:
                s.set_option(k, v)
            s.timesteps_init(float(atm["time"].min()), float(atm["time"].max()))
            run(s)
            out.append(s.state())
        finally:
            s.close()
    _same(out[0], out[1], "lean / general")
    return out[0]


# ---------------------------------------------------------------------------
# 1. table contents
# ---------------------------------------------------------------------------

def _reference_table(m0, m1):
    """module_diff_meso's statistics (mptrac.c:4287-4318) for every raw cell: float32 accumulation in the reference's
    order -- i (lon), j (lat), k (level), met0 before met1."""
    nx, ny, npl = m0.nx, m0.ny, m0.np
    out = np.zeros((nx - 1, ny - 1, npl - 1, 3), dtype=np.float32)
    sixteen = np.float32(16.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for q, name in enumerate("uvw"):
            mean = np.zeros((nx - 1, ny - 1, npl - 1), dtype=np.float32)
            sig = np.zeros_like(mean)
            for i in (0, 1):
                for j in (0, 1):
                    for k in (0, 1):
                        for m in (m0, m1):
                            v = m.f3[name][i:nx - 1 + i, j:ny - 1 + j, k:npl - 1 + k]
                            mean = mean + v
                            sig = sig + v * v
            assert mean.dtype == np.float32 and sig.dtype == np.float32
            m16 = mean / sixteen
            var = sig / sixteen - m16 * m16
            out[..., q] = np.where(var > 0, np.sqrt(np.where(var > 0, var, 0)), np.float32(0))
    return out


def _device_table(m0, m1):
    ctl, clim, _, _, atm = cases.make_case("conv_sedi", n=16, grid=GRID_C)
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    try:
        return s.test_meso_table((m0.nx, m0.ny, m0.np))
    finally:
        s.close()


def _mets(grid):
    return synthetic_met(grid, 0.0, 1.0, fields=cases.PRESSURE_LEVEL_FIELDS), \
        synthetic_met(grid, 3600.0, 1.25, fields=cases.PRESSURE_LEVEL_FIELDS)


@pytest.mark.parametrize("grid", [GRID_A, GRID_B, GRID_ONE_CELL], ids=["A", "B", "one_cell"])
def test_table_equals_the_sums_in_the_reference_order(grid):
    m0, m1 = _mets(grid)
    want = _reference_table(m0, m1)
    got = _device_table(m0, m1)
    assert got.shape == want.shape
    assert np.array_equal(got, want), int(np.count_nonzero(got != want))
    if grid != GRID_ONE_CELL:      # (its two columns are one, at the poles: next to no wind)
        assert np.count_nonzero(got[..., 0]) > 0 and np.count_nonzero(got[..., 1]) > 0


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_one_bad_corner_zeroes_its_eight_cells_and_no_other(bad):
    m0, m1 = _mets(GRID_A)
    clean = _device_table(m0, m1)
    i, j, k = 4, 2, 2      # an inner node: the corner of eight cells, in two bricks along ix
    for name in "uvw":
        m1.f3[name][i, j, k] = bad
    got = _device_table(m0, m1)
    assert np.array_equal(got, _reference_table(m0, m1))
    hit = np.zeros(clean.shape[:3], dtype=bool)
    hit[i - 1:i + 1, j - 1:j + 1, k - 1:k + 1] = True
    assert hit.sum() == 8
    assert np.all(got[hit] == 0)
    assert np.array_equal(got[~hit], clean[~hit])
    assert np.all(clean[hit][:, 0] > 0)


# ---------------------------------------------------------------------------
# 2. lean equals general
# ---------------------------------------------------------------------------

NO_TURB = dict(turb_dx_pbl=0.0, turb_dx_trop=0.0, turb_dx_strat=0.0, turb_dz_pbl=0.0, turb_dz_trop=0.0, turb_dz_strat=0.0)
# name: (case, control settings on top, direction, what runs)
SETS = {
    "module_alone": ("conv_sedi", {}, 1, _movers),
    "advect_and_module": ("diff", NO_TURB, 1, _steps),                      # (a gated subset: no turbulent diffusion)
    "c3_rk4": ("conv_sedi", dict(advect=4), 1, _steps),
    "c3_midpoint": ("conv_sedi", dict(advect=2), 1, _steps),
    "gated_no_convection": ("conv_sedi", dict(conv_cape=-999.0), 1, _steps),
    "c3p_closure": ("pbl_meso", {}, 1, _steps),
    "model_level_winds": ("zeta_full", {}, 1, _steps),
    "backward": ("conv_sedi", {}, -1, _steps),
}


@pytest.mark.parametrize("modules", list(SETS))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_lean_equals_general(grid, modules):
    case, over, direction, run = SETS[modules]
    inputs = _inputs(case, GRIDS[grid], direction, **over)
    g = _lean_and_general(inputs, run)
    moved = np.count_nonzero(g["uvwp"][:, 0])
    assert moved > N // 2, moved      # (module_diff_meso ran)


# ---------------------------------------------------------------------------
# 3. launch shapes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("grid", ["A", "C"])
def test_seven_steps_in_one_call_equal_the_loop(grid):
    """mphip_run_timesteps with eight logical blocks (a thread walks two particles) and a locality re-sort every three
    steps (folded into the launch behind it) against one mphip_run_timestep per step."""
    ctl, clim, m0, m1, atm = _inputs("conv_sedi", GRIDS[grid])
    out, launches = [], []
    for batched in (True, False):
        s = hip.Simulation(ctl, clim, m0, m1, atm)
        try:
            s.set_option("locality_sort_interval", 3)
            s.set_option("fold_resort", 1)
            s.set_option("step_blocks_multi", 8)
            s.timesteps_init(0.0, 0.0)
            times = cases.step_times(s.ctl)
            s.profile_begin()
            if batched:
                s.run_timesteps(times[1], 7)
            else:
                for t in times[1:8]:
                    s.run_timestep(t)
            launches.append(s.profile_end()[0])
            out.append(s.state())
        finally:
            s.close()
    _same(out[0], out[1], "one call / loop")
    assert launches[0] < launches[1] == 7      # (steps shared launches)
    assert np.all(out[0]["time"] == 7 * DT)


# ---------------------------------------------------------------------------
# 4. hand-over
# ---------------------------------------------------------------------------

def _three_snapshots(grid):
    f = cases.PRESSURE_LEVEL_FIELDS
    return [synthetic_met(grid, 3600.0 * k, amp, fields=f) for k, amp in enumerate((1.0, 1.25, 0.8))]


@pytest.mark.parametrize("path", ["swap", "commit", "one_slot"])
def test_hand_over_rebuilds_the_table(path):
    """swap, commit: two moving steps up to met1's time, the hand-over to (met1, met2), three steps beyond -- through
    mphip_swap_met + mphip_update_met, and through mphip_prefetch_met + mphip_commit_met (the set packed beside the
    steps).  one_slot: no hand-over, but a new met1 (other winds, the same time) uploaded into slot 1 alone between the
    third and the fourth of six steps inside one interval."""
    first = 2700.0 if path == "one_slot" else 3240.0
    ctl, clim, _, _, atm = _inputs("conv_sedi", GRID_A, t_stop=7200.0)
    mets = _three_snapshots(GRID_A)
    atm["time"][:] = first
    other = synthetic_met(GRID_A, 3600.0, 0.7, fields=cases.PRESSURE_LEVEL_FIELDS)
    times = [first + DT * k for k in range(6)]
    out = []
    for generic in (0, 1):
        s = hip.Simulation(ctl, clim, mets[0], mets[1], atm)
        try:
            s.set_option("generic_kernel", generic)
            s.timesteps_init(first, first)
            if path == "commit":
                s.prefetch_met(mets[2])
            for k, t in enumerate(times):
                if path == "swap" and t > s._mets[1].time:
                    s.swap_met(mets[2])
                if path == "commit" and t > s._mets[1].time:
                    s.commit_met()
                if path == "one_slot" and k == 3:
                    s.set_met(1, other)
                s.run_timestep(t)
            assert s._mets[1] is (other if path == "one_slot" else mets[2])
            out.append(s.state())
        finally:
            s.close()
    _same(out[0], out[1], "lean / general after the hand-over")
    assert np.all(out[0]["time"] == times[-1])
    assert np.count_nonzero(out[0]["uvwp"][:, 0]) > N // 2


# ---------------------------------------------------------------------------
# 5. the module switched on late
# ---------------------------------------------------------------------------

def test_module_switched_on_after_the_upload():
    """Uploaded and stepped with both mesoscale factors 0 (no table), then control parameters with the module on."""
    inputs = _inputs("conv_sedi", GRID_A, turb_mesox=0.0, turb_mesoz=0.0)

    def run(s):
        times = cases.step_times(s.ctl)
        for t in times[:3]:
            s.run_timestep(t)
        assert np.count_nonzero(s.get_cache()["uvwp"]) == 0
        s.ctl.turb_mesox = s.ctl.turb_mesoz = 0.16
        s.update_ctl()
        for t in times[3:6]:
            s.run_timestep(t)

    g = _lean_and_general(inputs, run)
    assert np.count_nonzero(g["uvwp"][:, 2]) > N // 2
