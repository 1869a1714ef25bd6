"""The edge inputs of the sample and station outputs (tests/analysis_cases.py) on the reference alone: they do what they
claim.  Every comparison of the two loops has placed particles on both sides at adjacent doubles, exact equalities exist
for time, depth, distance and the band, every site has particles the band rejects and the chord alone would accept, the
clusters give exactly the listed counts, the order of addition shows in the bits of every long list, and every tile and
chunk index named in analysis_cases carries a hit.  No GPU.  One "ANA_CASE {json}" line of facts per case."""
import json
import math

import numpy as np
import pytest

import analysis_cases as AC
import refanalysis as RA


def report(**row):
    print("ANA_CASE " + json.dumps(row))


def test_every_comparison_has_particles_on_both_sides():
    f = AC.facts_main()
    report(**f)
    # eight sites: 6 directions each for five of them, 2 at a pole, 3 at 89.5 N
    assert f["distance_pairs"] == 5 * 6 + 2 * 2 + 3
    assert f["dx_equal"]["equal"] and f["dx_equal"]["below"] and f["dx_equal"]["above"]
    assert f["band_pairs"] == 5 * 2 + 3
    assert set(f["band_rejects_what_the_chord_accepts"]) == set(AC.EDGE_SITES)
    assert all(n >= len(AC.SLIVER) for n in f["band_rejects_what_the_chord_accepts"].values())
    assert "equator/north" in f["band_equal"] and "equator/south" in f["band_equal"]
    # p < p_top is outside, p == p_top and p == p_bottom inside, p > p_bottom outside; 5e-324: top == bottom
    for dz in ("1.5", "6"):
        assert f["depth_below_on_above"][dz + "/top"] == (False, True, True)
        assert f["depth_below_on_above"][dz + "/bottom"] == (True, True, False)
    assert f["depth_below_on_above"]["4.94066e-324/top"] == f["depth_below_on_above"]["4.94066e-324/bottom"] == (False, True, False)
    assert f["time_below_on_above"] == {"270": (False, True, True), "450": (True, True, False)}
    assert all(all(n) for n in f["nodes_below_on_above"]) and f["under_first_node"] and f["over_last_node"]


def test_the_band_is_a_decision():
    """the measurement behind the sliver: on a meridian the chord stays <= dx up to |dlat| = (1 + 6e-4) reach_lat, and the
    band alone rejects there"""
    lon, lat = AC.SITES["mid"]
    reach = AC.reach_lat(AC.DX)
    chord = {f: math.sqrt(AC.dist2(lon, lat, lon, lat + (1.0 + f) * reach)) for f in AC.SLIVER + (7e-4,)}
    report(case="band", chord_km=chord)
    assert all(chord[f] <= AC.DX for f in AC.SLIVER) and chord[7e-4] > AC.DX


def test_list_lengths_and_the_order_of_addition():
    f = AC.facts_lists()
    report(case="lists", **f)
    want = {"list/%d" % n: n for n in AC.LENGTHS}
    want["list/65b"] = 65
    want.update({"five/%d" % k: 1 for k in range(5)})
    assert f["counts"] == want
    assert set(f["order_of_addition_shows"]) >= {"list/129", "list/128", "list/65", "list/65b", "list/64", "list/63"}
    assert all(f["order_of_addition_shows"].values())
    assert f["most_cylinders_around_a_particle"] >= 5
    assert all(f["stages_remove"])          # the band, the distance and the depth each reject particles
    # the two identical observations have identical results; the empty one lies between two crowded ones
    obs = [o[0] for o in AC.main()[2]]
    count, mass, _, hits = AC.sample_reference("main", "main")
    a, b = obs.index("list/65"), obs.index("list/65b")
    assert np.array_equal(hits[a], hits[b]) and mass[a] == mass[b]
    e = obs.index("list/0")
    assert count[e - 1] == 129 and count[e] == 0 and count[e + 1] == 128


def test_depth_time_and_radius_calls_decide_as_claimed():
    atm, tags, obs = AC.main()
    names = [o[0] for o in obs]
    d, t = names.index("site/depth"), names.index("site/time")

    def hit_tags(name, i):
        return {tags[j] for j in AC.sample_reference("main", name)[3][i].tolist() if j < len(tags)}

    off = hit_tags("dz/0", d)
    assert off == hit_tags("dz/-999", d) and len(off) == 19           # the depth test is off: all 18 and the centre
    tiny = hit_tags("dz/4.94066e-324", d)                              # on, with top == bottom == P(z)
    assert tiny == {"centre/depth", "depth/4.94066e-324/top/on", "depth/4.94066e-324/bottom/on"}
    normal = hit_tags("dz/1.5", d)
    assert {"depth/1.5/top/on", "depth/1.5/top/above", "depth/1.5/bottom/on", "depth/1.5/bottom/below"} <= normal
    assert not {"depth/1.5/top/below", "depth/1.5/bottom/above", "depth/6/top/on", "depth/6/bottom/on"} & normal
    assert hit_tags("t_point", t) == {"time/360/on", "centre/time"} and hit_tags("t_reversed", t) == set()
    window = hit_tags("main", t)
    assert {"time/270/on", "time/270/above", "time/450/on", "time/450/below"} <= window
    assert not {"time/270/below", "time/450/above", "time/100/on", "time/1000/on"} & window
    # dx * dx == dist2: inside; one double less: outside
    dx, site, i = AC.equal_radius()
    k = names.index("site/" + site)
    assert tags[i] in hit_tags("dx_eq/on", k) and tags[i] in hit_tags("dx_eq/above", k) and tags[i] not in hit_tags("dx_eq/below", k)
    report(case="calls", depth_off=len(off), depth_tiny=len(tiny), depth_normal=len(normal), window=len(window), dx_equal=dx)


def test_weighting_functions():
    """the repeated inner node is never divided by, the repeated last node gives NaN on it -- as C's division does"""
    atm, tags, obs = AC.main()
    w = [o[0] for o in obs].index("site/wfn")
    kern = AC.kernels()
    on_node = float(atm["p"][tags.index("node/2/on")])
    for name in ("nk0", "nk1"):
        assert RA.kernel_weight(list(kern[name][0]), list(kern[name][1]), on_node) == 1.0
    assert RA.kernel_weight(list(kern["nk5"][0]), list(kern["nk5"][1]), on_node) == 0.6
    assert RA.kernel_weight(list(kern["rep4"][0]), list(kern["rep4"][1]), on_node) == 0.5
    assert math.isnan(RA.kernel_weight(list(kern["rep3"][0]), list(kern["rep3"][1]), on_node))
    assert RA.kernel_weight(list(kern["rep3"][0]), list(kern["rep3"][1]), float(atm["p"][tags.index("node/2/above")])) == 0.5
    below = RA.kernel_weight(list(kern["rep3"][0]), list(kern["rep3"][1]), float(atm["p"][tags.index("node/2/below")]))
    assert 0.2 < below <= 1.0              # (the first interval: its width is not zero)
    masses = {name: float(AC.sample_reference("main", "kernel/" + name)[1][w]) for name in kern}
    report(case="weighting", mass_at_the_site=masses)
    assert masses["nk0"] == masses["nk1"] and math.isnan(masses["rep3"])
    assert len({masses[k] for k in ("nk0", "nk2", "nk5", "rep4")}) == 4


def test_the_division_of_the_weighting_function_keeps_its_bits():
    """numpy's float64 division under errstate against Python's /, on the nodes of the existing tests and random ones"""
    rng = np.random.default_rng(5)
    kz, kw = [0.0, 5.0, 12.0, 30.0], [0.2, 1.0, 0.6, 0.1]
    for p in RA.P0 * np.exp(-rng.uniform(-2.0, 35.0, 2000) / RA.H0):
        z = RA.Z(float(p))
        if kz[0] <= z <= kz[-1]:
            lo = max(k for k in range(3) if kz[k] <= z)
            assert RA.kernel_weight(kz, kw, float(p)) == kw[lo] + (kw[lo + 1] - kw[lo]) / (kz[lo + 1] - kz[lo]) * (z - kz[lo])


@pytest.mark.parametrize("nobs", AC.NOBS)
def test_tile_indices_carry_hits(nobs):
    obs = AC.tiled(nobs)
    count, mass, _, _ = AC.sample_reference("main", "nobs/%d" % nobs)
    assert len(obs) == len(count) == nobs
    slots = sorted({s for s in AC.TILE_SLOTS + (nobs - 1,) if 0 <= s < nobs})
    report(case="nobs/%d" % nobs, slots={s: (obs[s][0], int(count[s])) for s in slots}, hits=int(np.count_nonzero(count)),
           records=int(count.sum()))
    assert all(count[s] >= 63 if obs[s][0].startswith("list/") else count[s] >= 5 for s in slots)
    fillers = [i for i, o in enumerate(obs) if o[0].startswith("filler")]
    assert all(count[i] == 0 for i in fillers) and len(fillers) >= nobs - 60
    if nobs > 1:
        assert count[0] == count[nobs - 1] == 65 and mass[0] == mass[nobs - 1]      # identical, tiles apart
    if nobs > 1024:
        assert nobs - 1 >= 1 << 10        # an observation index that needs the second pass of the index sort


@pytest.mark.parametrize("n", AC.COUNTS)
def test_particle_counts_and_chunk_borders(n):
    atm, placed = AC.count_case(n)
    count, mass, stages, hits = AC.sample_reference(str(n), "layer")
    first = set(hits[0].tolist())
    report(case="count/%d" % n, placed=placed, counts=count.tolist())
    assert first == set(placed)
    listed = AC.station_reference(str(n), AC.COUNT_OBS[0][1], AC.COUNT_OBS[0][2], AC.DX, *AC.EVER, AC.QSTAT)[0]
    assert listed.tolist() == placed
    if n > 16385:
        assert set(AC.BORDER) <= first and 16383 >> 14 == 0 and 16384 >> 14 == 1 and n - 1 == AC.BORDER[-1]
        t = atm["time"]
        inside = ~((t < AC.T0) | (t > AC.T1))
        assert inside[512:768].sum() == 1 and inside[767] and not inside[768:1280].any()
        # ... and they would be hits but for their time
        late = dict(atm, time=np.full(n, AC.T))
        assert RA.sample_obs(late, AC.T0, AC.T1, [20.0], [30.0], [AC.Z_OBS], AC.DX, AC.DZ, -1)[0][0] >= 768


def test_not_finite_particles_are_hits_where_the_negated_comparisons_say_so():
    atm, tags = AC.not_finite()
    out = {}
    for name in ("layer", "plain"):
        count, mass, _, hits = AC.sample_reference("not_finite", name)
        out[name] = sorted(tags[i] for i in hits[0].tolist() if not tags[i].startswith(("good", "background")))
    listed = AC.station_reference("not_finite", 20.0, 30.0, AC.DX, *AC.EVER, -1)[0]
    out["station"] = sorted(tags[i] for i in listed.tolist() if not tags[i].startswith(("good", "background")))
    report(case="not_finite", **out)
    # a NaN is inside every comparison; an infinity is outside where it is compared, a NaN where it goes through cos / sin
    assert out["plain"] == sorted(["lon/nan", "lon/inf", "lon/-inf", "lat/nan", "p/nan", "p/inf", "p/-inf", "time/nan"])
    assert out["layer"] == sorted(["lon/nan", "lon/inf", "lon/-inf", "lat/nan", "p/nan", "time/nan"])
    assert out["station"] == sorted(["lon/nan", "lon/inf", "lon/-inf", "lat/nan", "lat/inf", "lat/-inf", "p/nan", "p/inf",
                                     "p/-inf", "time/nan"])
    assert not np.isnan(atm["q"][AC.QSTAT]).any()


def test_station_windows_and_flags():
    atm, tags, _ = AC.main()
    out = {}
    for name, (site, lon, lat, r, s0, s1) in AC.station_calls().items():
        listed = AC.station_reference("main", lon, lat, r, s0, s1, -1)[0]
        out[name] = [tags[i] for i in listed.tolist()]
    report(case="station", listed={k: len(v) for k, v in out.items()})
    w = {k[7:]: set(v) for k, v in out.items() if k.startswith("window/")}
    assert w["reversed"] == set() and w["point"] == {"time/360/on", "centre/time"}
    assert {"time/300/on", "time/300/above", "time/400/on", "time/400/below"} <= w["inside"]
    assert not {"time/300/below", "time/400/above"} & w["inside"]
    assert {"time/270/on", "time/300/on"} <= w["over_t0"] and not {"time/270/below", "time/300/above", "time/100/on"} & w["over_t0"]
    assert {"time/400/on", "time/450/on"} <= w["over_t1"] and not {"time/400/below", "time/450/above", "time/1000/on"} & w["over_t1"]
    assert "time/360.5/on" in w["cuts_above"] and "time/360.5/above" not in w["cuts_above"] and "time/270/on" in w["cuts_above"]
    assert "time/350.25/on" in w["cuts_below"] and "time/350.25/below" not in w["cuts_below"] and "time/450/on" in w["cuts_below"]
    # the meridional pairs lie beyond the band: only the station output decides on their distance
    for site in AC.EDGE_SITES:
        got = set(out["dist/" + site])
        for d in ("north", "south"):
            pair = [t for t in tags if t.startswith("dist/%s/%s/" % (site, d))]
            if pair:
                assert len(pair) == 2 and len(got & set(pair)) == 1, (site, d)
    r, site, i = AC.equal_radius()
    assert tags[i] in out["r_eq/on"] and tags[i] in out["r_eq/above"] and tags[i] not in out["r_eq/below"]
    # flags: (int) truncates; the listed particles' flags become 1, the others keep their bits
    lon, lat = AC.SITES["flags"]
    listed, rows, q_after, skipped = AC.station_reference("main", lon, lat, AC.DX, *AC.EVER, AC.QSTAT)
    flags = [float(atm["q"][AC.QSTAT][i]) for i in listed.tolist()]
    assert sorted(flags) == sorted(2 * [f for f in AC.FLAGS if int(f) == 0]) and {0.5, -0.5, 1e-300} <= set(flags)
    assert skipped == 2 * sum(1 for f in AC.FLAGS if int(f) != 0)
    assert (q_after[AC.QSTAT][listed] == 1).all()
    report(case="flags", listed=len(listed), skipped=skipped, values=sorted(set(flags)))
