"""The cases of tests/sort_cases.py do what they are named for -- without a device.  tests/test_gpu_sort_edges.py is only as
good as that: a case whose keys no longer reach the second chunk of the scan, or whose 4097th mover has become a stayer,
would pass there and check nothing.

The launch arithmetic of radix_passes and repair_sort (mptrac_amd/csrc/mphip_api.hip) and the constants of the kernels
(mphip_kernels.hpp) are restated in sort_cases.py on literals, and the literals are compared with the source text here.
The oracle confirms that every placed particle has the intended key, that module_sort's permutation is numpy's stable
argsort (ties by index), and that the movers of every repair case are those the case claims."""
import os
import re

import numpy as np
import pytest

import sort_cases as S
from oracle import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(name):
    with open(os.path.join(ROOT, "mptrac_amd", "csrc", name)) as f:
        return f.read()


def test_the_restated_constants_are_those_of_the_source():
    hpp, api = _source("mphip_kernels.hpp"), _source("mphip_api.hip")
    for name, value in (("kSortThreads", S.SORT_THREADS), ("kSortRounds", S.SORT_ROUNDS), ("kScanThreads", S.SCAN_THREADS),
                        ("kRepairTile", S.REPAIR_TILE), ("kMergeTile", S.MERGE_TILE), ("kRadixMaxBits", S.RADIX_MAX_BITS)):
        assert re.search(rf"constexpr int {name} = {value};", hpp), name
    assert f"constexpr int kScanPerSmall = {S.SCAN_PER_SMALL}, kScanPerLarge = {S.SCAN_PER_LARGE};" in hpp
    assert "constexpr int kSortTile = kSortThreads * kSortRounds;" in hpp and S.SORT_TILE == 4096
    assert "constexpr int kPerWave = kSortTile / kWaves;" in hpp and S.WAVE_SHARE == 1024
    assert "key[r] = valid ? keys_in[i * in_stride] : 0xffffffffu;" in hpp          # the padding lanes' key
    assert "counts[(size_t) d * ntiles + blockIdx.x] = h[d];" in hpp                # the counter layout
    assert "const int per = (ntiles + 1023) / 1024;" in hpp                         # repair_scan_kernel
    # radix_passes: digit choice, passes, counters, chunk length
    assert "if ((key_bits + b - 1) / b < (key_bits + bits - 1) / bits)" in api
    assert "const int passes = (key_bits + bits - 1) / bits;" in api
    assert "const size_t m = ((size_t) 1 << bits) * ntiles;" in api
    assert "(m + kScanThreads * kScanPerSmall - 1) / (kScanThreads * kScanPerSmall) <= (size_t) kScanThreads;" in api
    assert "const int chunk_shift = small ? 12 : 14;" in api
    assert re.search(r"while \(key_bits < 32 && \(kmax >> key_bits\) != 0\)\s+key_bits\+\+;", api)
    assert "unsigned long long kmax = (unsigned long long) ctx->nx * ctx->ny * ctx->npl;" in api
    # repair_sort
    assert "const int ntiles = (int) ((n + kRepairTile - 1) / kRepairTile);" in api
    assert "const int nmerge = (int) ((n + kMergeTile - 1) / kMergeTile);" in api


def test_every_grid_has_the_pass_plan_it_is_named_for():
    for grid, (key_bits, bits, passes, pair) in S.PLANS.items():
        P = S.plan(grid, 4097)
        assert (P["key_bits"], P["bits"], P["passes"], P["pair"]) == (key_bits, bits, passes, pair), grid
        nx, ny, npl = S.dims(grid)
        assert S.usable(grid)[-1] == ((nx - 2) * ny + ny - 2) * npl + npl - 2 < nx * ny * npl - 1
    assert [S.bits_for(k) for k in (0, 1, 2, 255, 256, 0xffffffff)] == [1, 1, 2, 8, 9, 32]
    # the forced widths: every instantiation meets one, two and three passes
    for bits in (8, 9, 10):
        assert {S.plan(g, 4097, bits)["passes"] for g, _, _, b in S.FORCED if b == bits} == {1, 2, 3}, bits
    # one pass: no usable key has the digit of the padding lanes
    for grid in ("p1b8", "p1b9", "p1b10"):
        assert S.usable(grid)[-1] < (1 << S.PLANS[grid][1]) - 1


SCAN = {("p2b8", 65536): (16, 1), ("p2b8", 65537): (17, 2), ("p2b8", 69633): (18, 2),
        ("p1b10", 16385): (5, 2), ("p1b10", 20481): (6, 2)}


def _digit(keys, P, pass_):
    return (keys >> (P["bits"] * pass_)) & ((1 << P["bits"]) - 1)


@pytest.mark.parametrize("case", [c + (0,) for c in S.SCRATCH] + S.FORCED, ids=S.case_id)
def test_every_pattern_reaches_the_path_it_is_named_for(case):
    grid, pattern, n, bits = case
    keys, U, P = S.pattern_keys(*case), S.usable(grid), S.plan(grid, n, bits)
    assert keys.shape == (n,) and np.all(np.isin(keys, U))
    radix = 1 << P["bits"]
    if pattern.startswith("equal"):
        assert np.all(keys == (U[0] if pattern == "equal_first" else U[-1]))
    elif pattern == "sorted":
        assert np.all(np.diff(keys) >= 0) and len(np.unique(keys)) == min(n, len(U))
    elif pattern == "descending":
        assert np.all(np.diff(keys) <= 0) and len(np.unique(keys)) == min(n, len(U))
    elif pattern.startswith("alternate"):
        period = int(pattern[9:])
        runs = np.diff(np.flatnonzero(np.r_[True, np.diff(keys) != 0, True]))
        assert set(runs[:-1]) == {period} and runs[-1] <= period and set(keys) == {U[0], U[-1]}
        assert period in (1, 64, S.WAVE_SHARE, S.SORT_TILE) and n > S.SORT_TILE + period - 1
        # the two keys differ in every digit of the plan
        assert all(_digit(U[:1], P, k) != _digit(U[-1:], P, k) for k in range(P["passes"]))
    elif pattern == "low_radix_1":
        assert P["passes"] >= 2 and np.all(_digit(keys, P, 0) == radix - 1)
        assert len(np.unique(keys)) > 1 or len(U) < 2 * radix          # ((7, 8, 7) at 8 bits: 255 is the only such key)
        assert n % 64 != 0                                    # a ragged round: valid and padding lanes share the digit
    elif pattern == "top_only":
        top = P["bits"] * (P["passes"] - 1)
        assert len(np.unique(keys & ((1 << top) - 1))) == 1 and len(np.unique(keys)) > 1
    elif pattern == "bottom_only":
        assert len(np.unique(keys >> P["bits"])) == 1 and len(np.unique(keys)) > 1
    elif pattern == "tied":
        v, c = np.unique(keys, return_counts=True)
        assert 100 < len(v) <= 300 and c.max() >= n // 2
    elif pattern == "uniform":
        ntiles, nchunks = SCAN[(grid, n)]
        assert (P["ntiles"], P["nchunks"], P["chunk"]) == (ntiles, nchunks, 4096)
        counter = _digit(keys, P, 0) * ntiles + np.arange(n) // S.SORT_TILE       # first pass: the input order
        assert (counter.max() >= P["chunk"]) == (nchunks == 2)
        if nchunks == 2:
            assert P["chunk"] % ntiles != 0                   # the chunk border falls inside a digit's row
            assert P["chunk"] // ntiles == {17: 240, 18: 227, 5: 819, 6: 682}[ntiles]
        if grid == "p2b8":                                    # its second pass stays inside the first chunk
            assert _digit(U, P, 1).max() <= (14060 - 1) >> 8 == 54 and 55 * ntiles <= P["chunk"]
    else:
        raise KeyError(pattern)


def test_the_patterns_cover_the_sizes_and_the_plans():
    sizes = {n for _, _, n in S.SCRATCH}
    assert sizes >= {1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 65536, 65537, 69633, 16385, 20481}
    assert len(S.SCRATCH) + len(S.FORCED) < 100
    by_pattern = {}
    for grid, pattern, n in S.SCRATCH:
        by_pattern.setdefault("alternate" if pattern.startswith("alternate") else pattern, set()).add(S.PLANS[grid][2])
    for pattern, passes in by_pattern.items():
        assert passes >= ({2} if pattern == "low_radix_1" else {1, 2}), pattern
    assert {p for _, p, _ in S.SCRATCH if p.startswith("alternate")} == {"alternate%d" % k for k in (1, 64, 1024, 4096)}
    # a tile that ends exactly on a round, a wave's share and the tile
    last = {S.plan(g, n)["last_tile"] for g, _, n in S.SCRATCH}
    assert last >= {64, S.WAVE_SHARE, S.SORT_TILE, 1, 63, 65}


def _scratch_cases_by_grid():
    seen = {}
    for grid, pattern, n, bits in [c + (0,) for c in S.SCRATCH] + S.FORCED:
        seen.setdefault(grid, {})[(pattern, n, bits)] = None
    return [(g, list(v)) for g, v in seen.items()]


@pytest.mark.parametrize("grid,cases", _scratch_cases_by_grid(), ids=lambda v: v if isinstance(v, str) else "")
def test_the_oracle_finds_the_placed_keys_and_sorts_like_the_stable_argsort(grid, cases):
    for pattern, n, bits in cases:
        keys = S.pattern_keys(grid, pattern, n, bits)
        ctl, clim, m0, m1, atm = S.scratch_inputs(grid, keys)
        assert np.array_equal(S.keys_of(grid, atm["lon"], atm["lat"], atm["p"]), keys), (pattern, n)
        o = B.Oracle(ctl, clim, m0, m1, atm)
        keys_o, perm_o = o.sort()
        assert np.array_equal(keys_o, keys), (pattern, n)                       # (keys in slot order)
        ref = np.argsort(keys, kind="stable")
        assert np.array_equal(perm_o, ref), (pattern, n)
        assert np.array_equal(o.q[0], ref + 1.0) and np.array_equal(o.lon, atm["lon"][ref])


# ---- the repair ------------------------------------------------------------------------------------------------------------

def _tie_orders(step):
    """(a mover sorts in front of a stayer of its key, a stayer in front of a mover): ties in both slot orders"""
    keys, mv = step["keys"], step["movers"]
    order = step["perm"]
    k, m = keys[order], mv[order]
    same = k[1:] == k[:-1]
    return bool(np.any(same & m[:-1] & ~m[1:])), bool(np.any(same & ~m[:-1] & m[1:]))


def _claims(name, case, steps):
    n = case["n"]
    count = [int(s["movers"].sum()) for s in steps]
    first = steps[2]["movers"]          # the first module_sort behind a step that moved somebody: slots of the initial order
    tiles = np.add.reduceat(first, np.arange(0, n, S.REPAIR_TILE))
    if name == "none":
        assert count == [0, 0, 0, 0]
    elif name == "all":
        assert count == [0, 0, n, n]
    elif name == "one_first":
        assert count == [0, 0, 1, 1] and first[0]
    elif name == "one_last":
        assert count == [0, 0, 1, 1] and first[n - 1]
    elif name == "one_stayer":
        assert count == [0, 0, n - 1, n - 1] and not first[n // 2]
    elif name == "tiles":
        assert list(tiles[:5]) == [0, S.REPAIR_TILE, 0, 1, S.REPAIR_TILE - 1] and tiles[5:].sum() == 0
    elif name == "cross4096":
        assert count == [0, 0, S.SORT_TILE, S.SORT_TILE + 1]
    elif name == "runs":
        sides = S.merge_sides(steps[2])
        assert (S.MERGE_TILE, 0) in sides and (0, S.MERGE_TILE) in sides and any(a and b for a, b in sides)
    else:                               # mixed, one_pass, the sizes: about 15 % movers, ties in both slot orders
        assert 0.1 * n < count[2] < 0.2 * n and count[3] >= count[2]
        assert _tie_orders(steps[2]) == (True, True)
    if name[1:].isdigit():
        assert n == int(name[1:]) and S.repair_plan(n)["tiles"] == -(-n // 1024)
    if name == "one_pass":
        assert S.PLANS[case["grid"]][2] == 1
    else:
        assert S.PLANS[case["grid"]][2:] == (2, 0)          # the movers' radix sort ends in the pair it started in


@pytest.mark.parametrize("name", S.REPAIR)
def test_the_movers_of_every_repair_case_are_those_it_claims(name):
    case = S.repair_case(name)
    assert np.all(np.diff(case["keys"]) >= 0) and np.all(np.isin(case["keys"], S.moving_cells(case["grid"], True))
                                                         | np.isin(case["keys"], S.moving_cells(case["grid"], False)))
    model, oracle = S.model_run(case), S.oracle_run(name)
    assert len(model) == len(oracle) == case["steps"] == 4
    for a, b in zip(model, oracle):
        assert np.array_equal(a["keys"], b["keys"]), (name, a["t"])
        assert np.array_equal(b["perm"], np.argsort(b["keys"], kind="stable")) and np.array_equal(a["perm"], b["perm"])
        assert np.array_equal(a["movers"], b["movers"])
    _claims(name, case, oracle)
    # nobody comes closer than 0.09 cell widths to a grid line, and the masses are still a permutation of 1 ... n
    lon = oracle[-1]["state"]["lon"]
    glon = S.axes(case["grid"])[0]
    frac = ((lon - glon[0]) / (glon[1] - glon[0])) % 1.0
    assert frac.min() > 0.09 and frac.max() < 0.91
    assert np.array_equal(np.sort(oracle[-1]["state"]["q"][0]), np.arange(1.0, case["n"] + 1.0))


def test_the_sizes_of_the_repair_cases_sit_on_both_sides_of_the_tiles():
    sizes = {S.repair_case(name)["n"] for name in S.REPAIR}
    assert sizes >= {1023, 1024, 1025, 2047, 2048, 2049, 4097, 20011}
    assert [S.repair_plan(n)["tiles"] for n in (1023, 1024, 1025)] == [1, 1, 2]
    assert [S.repair_plan(n)["merge_tiles"] for n in (2047, 2048, 2049)] == [1, 1, 2]
    assert all(S.repair_plan(n)["per"] == 1 for n in sizes)


def test_the_large_repair_case_takes_two_tiles_per_thread_of_the_scan():
    """n = 1 049 601: 1026 tiles of 1024 slots (the last one holds a single slot), so repair_scan_kernel sums two tiles
    per thread, and thread 512 is the last one with work.  The model only (tests/test_gpu_sort_edges.py checks this case
    against the numpy stable argsort and the run without the repair)."""
    case = S.repair_case(S.BIG)
    n = case["n"]
    R = S.repair_plan(n)
    assert (n, R["tiles"], R["per"], n - 1025 * S.REPAIR_TILE) == (1049601, 1026, 2, 1)
    steps = S.model_run(case)
    count = [int(s["movers"].sum()) for s in steps]
    assert len(steps) == 3 and count[:2] == [0, 0] and 0.14 * n < count[2] < 0.16 * n
    assert S.plan(case["grid"], count[2])["ntiles"] > 1 and _tie_orders(steps[2]) == (True, True)
