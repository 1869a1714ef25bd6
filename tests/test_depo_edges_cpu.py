"""The reference side of the decision-edge tests (tests/depo_cases.py): the oracle's module_convection,
module_wet_depo and module_dry_depo (and module_diff_turb on the shortcut cases) against the numpy restatement
tests/refmodules.py on every case, at that file's bar (tests/test_oracle_second_opinion.py: 1e-13 relative), with
the particles either side agrees to act on compared one by one.  Two independent statements of the decisions agree
here before the device is held to them (tests/test_gpu_depo_edges.py).

The census (depo_cases.census) counts per named branch the particles that took it according to the restatement; every
branch the case set exists for must be reached, so a case that drifts off its edge fails here instead of passing."""
import functools
import json

import numpy as np
import pytest

import depo_cases as D
from oracle import binding as B

TOL = 1e-13
NAMES = sorted(D.all_cases())


@functools.lru_cache(maxsize=None)
def oracle_modules(name):
    """{module: (state before, oracle after, dt, rs)} from the case's positions, every module on its own"""
    case = D.all_cases()[name]
    atm = case["atm"]
    out = {}
    for module in case["modules"]:
        o = B.Oracle(case["ctl"], case["clim"], case["m0"], case["m1"], atm)
        o.ctl.t_start, o.ctl.t_stop = D.T_START, D.T_STOP
        o.lon[:], o.lat[:] = case["m0"].lon[1], case["m0"].lat[1]
        o.module("timesteps", case["t"])
        assert np.array_equal(o.dt, case["t"] - atm["time"]) and np.all(o.dt != 0)
        o.lon[:], o.lat[:] = atm["lon"], atm["lat"]
        o.module(module)
        n = o.n
        out[module] = (o.state(), o.dt.copy(), o.rs[:3 * n].copy() if module == "diff_turb" else o.rs[:n].copy())
    return out


def _rel(a, b):
    with np.errstate(invalid="ignore"):
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        err = np.where(same, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
    return float(np.max(np.nan_to_num(err, nan=np.inf))) if err.size else 0.0


def _row_err(case, a, q, row):
    """tests/test_oracle_second_opinion.py's bar for a quantity row: the largest difference on the row's scale, the
    mloss_* rows (m (1 - aux), a difference of numbers near 1) on the mass row's; finite values only, the others are
    compared by class"""
    b = q[row]
    fin = np.isfinite(b) & np.isfinite(a)
    ref_row = q[case["quantities"].index("m")] if case["quantities"][row].startswith("mloss") else b
    ref_fin = ref_row[np.isfinite(ref_row)]
    scale = max(float(np.max(np.abs(ref_fin))) if ref_fin.size else 0.0, 1e-300)
    return float(np.max(np.abs(a[fin] - b[fin]))) / scale if fin.any() else 0.0


def acted(before, after):
    """particles with any value changed (bits, NaN == NaN)"""
    ch = np.zeros(len(before["p"]), dtype=bool)
    for k in ("lon", "lat", "p"):
        ch |= ~((before[k] == after[k]) | (np.isnan(before[k]) & np.isnan(after[k])))
    q0, q1 = np.asarray(before["q"]).reshape(np.asarray(after["q"]).shape), np.asarray(after["q"])
    if q1.size:
        ch |= np.any(~((q0 == q1) | (np.isnan(q0) & np.isnan(q1))), axis=0)
    return ch


@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_the_restatement(name):
    case = D.all_cases()[name]
    atm = case["atm"]
    for module, (r, dt, rs) in oracle_modules(name).items():
        st = D.reference_state(dict(case, modules=(module,)), rs)[module]
        # the same particles, one by one: whoever the restatement acts on and whose values change, the oracle changed,
        # and the oracle changed nobody else (a factor exp(-dt 0) = 1 acts and changes nothing, on both sides)
        want = {"lon": st.get("lon", atm["lon"]), "lat": st.get("lat", atm["lat"]), "p": st["p"],
                "q": np.array([st["q"][k] for k in case["quantities"]])}
        assert np.array_equal(acted(atm, r), acted(atm, want)), (module, np.nonzero(acted(atm, r) != acted(atm, want))[0][:10])
        for k in ("lon", "lat", "p"):
            assert _rel(want[k], r[k]) <= TOL, (module, k, _rel(want[k], r[k]))
        for row, qn in enumerate(case["quantities"]):
            # same class where a value is not finite (dz = 0: a rate of +inf, a factor of 0)
            assert np.array_equal(np.isnan(want["q"][row]), np.isnan(r["q"][row])), (module, qn)
            assert np.array_equal(np.isinf(want["q"][row]), np.isinf(r["q"][row])), (module, qn)
            err = _row_err(case, want["q"][row], r["q"], row)
            assert err <= TOL, (module, qn, err)
        assert np.array_equal(r["time"], atm["time"])


@functools.lru_cache(maxsize=None)
def full_census():
    total = {}
    for name in NAMES:
        case = D.all_cases()[name]
        rs = {m: v[2] for m, v in oracle_modules(name).items()}
        state = {"ctl": None}
        for module in case["modules"]:
            one = D.reference_state(dict(case, modules=(module,)), rs[module])
            state.update(one)
        for k, v in D.census(case, state).items():
            total[k] = total.get(k, 0) + v
    return total


def test_every_branch_is_reached():
    total = full_census()
    print("DEPO_CENSUS " + json.dumps(total, sort_keys=True))
    missing = [k for k in D.required_branches() if total.get(k, 0) == 0]
    assert not missing, missing


def test_extrapolation_beyond_the_longitude_axis_is_real():
    """On a regional longitude / latitude grid the reference continues the last cell's slope beyond the axis (the
    longitude is shifted by 360 degrees, not clamped): there are particles ABOVE the smallest node value of ps - dp, pct
    and the convective top that the oracle deposits / convects all the same.  On the Cartesian grid it clamps, and no
    such particle exists.  The premise of the device's shortcuts (interpolated value >= smallest node value) holds only
    for the second."""
    found = {}
    for name in NAMES:
        if not name.startswith("extrap-"):
            continue
        case = D.all_cases()[name]
        atm, mods = case["atm"], oracle_modules(name)
        ps_min = min(float(m.f2["ps"].min()) for m in (case["m0"], case["m1"]))
        pct_min = min(float(m.f2["pct"].min()) for m in (case["m0"], case["m1"]))
        top_min = min(min(float(m.f2["pel"].min()) for m in (case["m0"], case["m1"])), 740.0)      # pbl - 0.5 (ps - pbl) >= 790
        found[name] = dict(dry=int(np.count_nonzero(acted(atm, mods["dry_depo"][0]) & (atm["p"] < ps_min - 30.0 - 1.0))),
                           wet=int(np.count_nonzero(acted(atm, mods["wet_depo"][0]) & (atm["p"] < pct_min - 1.0))),
                           conv=int(np.count_nonzero(acted(atm, mods["convection"][0]) & (atm["p"] < top_min - 1.0))))
        assert np.all(mods["dry_depo"][1] != 0)
    print("DEPO_EXTRAPOLATION " + json.dumps(found))
    for name, f in found.items():
        if "regional" in name:
            assert f["dry"] + f["wet"] + f["conv"] > 0, (name, f)
        else:
            assert f == dict(dry=0, wet=0, conv=0), (name, f)
    assert sum(f["dry"] for f in found.values()) > 0 and sum(f["wet"] for f in found.values()) > 0
    assert sum(f["conv"] for f in found.values()) > 0


# ---------------------------------------------------------------------------
# the time-step configuration: what each workgroup of the deposition launch finds
# ---------------------------------------------------------------------------

def workgroup_size(n, blocks):
    """block_geom of mptrac_amd/csrc/mphip_api.hip: the particles of one logical block (a multiple of 256)"""
    per_block = -(-n // blocks)
    return max(256, -(-per_block // 256) * 256)


@functools.lru_cache(maxsize=None)
def run_oracle(mixing):
    """(case, oracle, step times, state behind every step): three calls of the time loop, the first with dt = 0"""
    import cases
    case = D.run_case(mixing)
    o = B.Oracle(case["ctl"], case["clim"], case["m0"], case["m1"], case["atm"])
    o.timesteps_init()
    times = cases.step_times(o.ctl)[:3]
    between = []
    for t in times:
        o.run_timestep(t)
        between.append(o.state())
    return case, o, times, between


def not_skipped(case, state):
    """per particle: does a shortcut of the deposition launch NOT apply (DevMet::pct_skip / ps_skip; every particle time
    of the run lies between the snapshots)"""
    b, dp = case["bounds"], case["ctl"].get("dry_depo_dp", 30.0)
    return (state["p"] > b["pct"]) | ~(state["p"] < b["ps"] - dp)


@pytest.mark.parametrize("mixing", [True, False], ids=["behind_mixing", "fused_tail"])
def test_time_step_case_gives_the_workgroups_the_intended_lists(mixing):
    """From the bounds of the scene's own fields and the order the oracle's module_sort leaves: in the steps that move,
    the workgroups of SEGMENT particles behind the probes hold 0, 1, 63, 64, 65 and 257 particles that no shortcut
    skips; the idle ones are skipped by both; and the particles on the bounds fall on either side of each."""
    case, o, times, between = run_oracle(mixing)
    n = len(case["atm"]["p"])
    assert workgroup_size(n, -(-n // D.SEGMENT)) == D.SEGMENT
    ident = case["quantities"].index("mloss_decay")
    tags = np.array(case["tags"])
    first = int(np.nonzero(np.char.startswith(tags, "run.bound"))[0][0]) // D.SEGMENT - len(D.BUSY_COUNTS)
    assert first * D.SEGMENT + len(D.BUSY_COUNTS) * D.SEGMENT == int(np.nonzero(np.char.startswith(tags, "run.bound"))[0][0])
    assert np.isfinite(case["bounds"]["pct"]) and np.isfinite(case["bounds"]["ps"])
    for state in between[1:]:
        number = state["q"][ident].astype(np.int64)
        assert mixing == (not np.array_equal(number, np.arange(n)))              # (module_sort did permute the arrays)
        busy = not_skipped(case, state)
        blocks = busy[:(n // D.SEGMENT) * D.SEGMENT].reshape(-1, D.SEGMENT).sum(axis=1)
        assert tuple(blocks[first:first + len(D.BUSY_COUNTS)]) == D.BUSY_COUNTS, blocks
        assert np.array_equal(busy[tags[number] == "run.idle"], np.zeros((tags == "run.idle").sum(), dtype=bool))
        assert busy[tags[number] == "run.busy"].all()
        b, dp = case["bounds"], case["ctl"].get("dry_depo_dp", 30.0)
        for which in ("pct", "ps"):
            p = state["p"][np.char.startswith(tags[number], "run.bound." + which)]
            taken = p <= b["pct"] if which == "pct" else p < b["ps"] - dp
            assert 0 < taken.sum() < len(p), (which, p)
        p = state["p"][np.char.startswith(tags[number], "run.bound.conv")]
        assert 0 < (p < b["conv"]).sum() < len(p)
    # the oracle acts on every busy particle and on no idle one
    final = between[-1]
    number = final["q"][ident].astype(np.int64)
    atm = case["atm"]
    moved = np.any(final["q"] != atm["q"][:, number], axis=0) | (final["p"] != atm["p"][number])
    assert moved[tags[number] == "run.busy"].all() and not moved[tags[number] == "run.idle"].any()
    assert moved[~np.char.startswith(tags[number], "run.")].sum() > 100


@pytest.mark.parametrize("sign", [1, -1], ids=["east", "west"])
def test_particles_that_cross_the_edge_within_a_step_keep_their_dt(sign):
    """The time-step form of the extrapolation cases: the oracle moves the crossing group beyond the axis in the first
    moving step and then deposits / convects particles that lie above every node value of ps - dp, pct and the convective
    top; in the following step their dt is 0 and nothing changes.  The group inside the domain has no such particle."""
    import cases
    case = D.extrap_run_case(sign)
    atm = case["atm"]
    o = B.Oracle(case["ctl"], case["clim"], case["m0"], case["m1"], atm)
    o.timesteps_init()
    times = cases.step_times(o.ctl)[:3]
    o.run_timestep(times[0])
    o.run_timestep(times[1])
    one = o.state()
    lon = case["m0"].lon
    crossing = np.array(case["tags"]) == "extrap_run.crossing"
    outside = (one["lon"] < lon[0]) | (one["lon"] > lon[-1])
    assert np.array_equal(outside, crossing) and np.all(o.dt == 180.0)
    b = D.field_bounds(case["m0"], case["m1"], case["ctl"])
    high = atm["p"] < min(b["pct"], b["ps"] - 30.0, b["conv"]) - 1.0          # above all three bounds
    acted = np.any(one["q"][:4] != atm["q"][:4], axis=0) | (one["p"] != atm["p"])
    assert (acted & high & crossing).sum() >= 64 and not (acted & high & ~crossing).any()
    o.run_timestep(times[2])
    two = o.state()
    assert np.all(o.dt[crossing] == 0) and np.array_equal(two["q"][:, crossing], one["q"][:, crossing])
