"""The cases of tests/pack_edge_cases.py do what they are named for -- without a device.  tests/test_gpu_pack_edges.py is
only as good as that: a case that no longer makes a second pass, or whose planted minimum has moved to workgroup 3, would
pass there and check nothing.

The launch arithmetic of pack_stream and mphip_pack_met (mptrac_amd/csrc/mphip_api.hip) and of the kernels
(mphip_pack.hpp) is restated here on literals, and the literals are compared with the source text: a later change of a
constant fails here first."""
import os
import re

import numpy as np
import pytest

import pack_edge_cases as E
import refpack as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

THREADS, VEC, MAX_BLOCKS = 256, 8, 2048         # lanes of a workgroup, values of a lane and pass, workgroups of a launch
LDS_LEVELS = 4096                               # levels whose {scl, off} table is read from LDS
RED_LEVELS, RED_PARTS = 64, 16                  # the reduction: levels per workgroup, slices side by side (1024 lanes)
COLS, LDS_BYTES = 64, 65536                     # the extremes: most columns per workgroup, and the LDS they may take
PASS = MAX_BLOCKS * THREADS * VEC


def _source(name):
    with open(os.path.join(ROOT, "mptrac_amd", "csrc", name)) as f:
        return f.read()


def _constant(text, name):
    expr = re.search(rf"constexpr int {name} = ([0-9 */]+);", text).group(1)
    return eval(expr.replace("/", "//"), {"__builtins__": {}})          # (digits, blanks, * and / only)


def test_the_restated_constants_are_those_of_the_source():
    hpp, api = _source("mphip_pack.hpp"), _source("mphip_api.hip")
    assert _constant(hpp, "kPkThreads") == THREADS and _constant(hpp, "kPkVec") == VEC
    assert _constant(hpp, "kPkMaxBlocks") == MAX_BLOCKS and PASS == 4194304
    assert _constant(hpp, "kPkLdsLevels") == LDS_LEVELS and LDS_LEVELS * 16 == LDS_BYTES
    assert _constant(hpp, "kPkRedLevels") == RED_LEVELS
    assert _constant(hpp, "kPkRedThreads") == RED_LEVELS * RED_PARTS == 1024
    assert "constexpr int kParts = kPkRedThreads / kPkRedLevels;" in hpp and "blk += kParts" in hpp
    # the plan of the streaming kernels
    assert re.search(r"P\.head = .*std::min<size_t>\(n, \(\(16 - \(\(uintptr_t\) q & 15\)\) & 15\) / sizeof\(unsigned short\)\);", api)
    assert re.search(r"P\.grid = .*\(nvec \+ kPkThreads - 1\) / kPkThreads, 1\), kPkMaxBlocks\)\);", api)
    assert "P.table_in_lds = nlev <= kPkLdsLevels;" in api
    assert "P.lds = P.table_in_lds ? 2 * (size_t) nlev * sizeof(double) : 0;" in api
    # the columns per workgroup of mphip_pack_met
    assert "const size_t col_bytes = (size_t) (nlev[i] | 1) * sizeof(float);" in api
    m = re.search(r"cpb\[i\] = \(int\) std::min<size_t>\((\d+), \((\d+) \* (\d+)\) / col_bytes\);", api)
    assert int(m.group(1)) == COLS and int(m.group(2)) * int(m.group(3)) == LDS_BYTES
    assert E.columns_per_workgroup(137) == COLS


def plan(n, nlev, shift=0):
    """pack_stream and the loop bounds of the streaming kernels for n values whose codes start `shift` elements behind a
    16-byte boundary."""
    head = min(n, (8 - shift) % 8)
    nvec = (n - head) // VEC
    blocks = min(max(-(-nvec // THREADS), 1), MAX_BLOCKS)
    stride = blocks * THREADS
    in_lds = nlev <= LDS_LEVELS
    return dict(head=head, nvec=nvec, tail=n - head - nvec * VEC, blocks=blocks, stride=stride, passes=-(-nvec // stride),
                last=nvec % stride, step=stride * VEC % nlev, in_lds=in_lds, lds=16 * nlev if in_lds else 0)


def lanes_that_wrap(P, nlev):
    """The levels of the lanes whose `lev += step` passes nlev before a pass that they still take part in."""
    g = np.arange(min(P["stride"], P["nvec"]), dtype=np.int64)
    lev = (P["head"] + g * VEC) % nlev
    out = []
    for k in range(1, P["passes"]):
        alive = g + k * P["stride"] < P["nvec"]
        out.append(lev[alive & (lev + P["step"] >= nlev)])
        lev = (lev + P["step"]) % nlev
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def extremes_plan(ncol, nlev):
    cpb = E.columns_per_workgroup(nlev)
    nblk = -(-ncol // cpb) if cpb else 0
    return dict(cpb=cpb, nblk=nblk, lds=cpb * (nlev | 1) * 4, last=ncol - (nblk - 1) * cpb if cpb else 0,
                red_blocks=-(-nlev // RED_LEVELS))


# ---- STRIDE ------------------------------------------------------------------------------------------------------------

def test_the_stride_grids_make_a_second_pass_with_the_step_they_name():
    seen = {}
    for shape in E.STRIDE:
        nx, ny, nlev = shape
        n = nx * ny * nlev
        for shift in (0, 3, 5):
            P = plan(n, nlev, shift)
            assert P["blocks"] == MAX_BLOCKS and P["passes"] >= 2 and 0 < P["last"] < P["stride"], (shape, shift)
            assert P["step"] == PASS % nlev
        seen[shape] = (n, plan(n, nlev), extremes_plan(nx * ny, nlev))
    n, P, X = seen[(257, 241, 137)]
    assert n == 8485369 and n % 8 == 1 and P["passes"] == 3 and P["tail"] == 1 and P["step"] == 49 and P["in_lds"]
    wrap = lanes_that_wrap(P, 137)
    assert wrap.size and wrap.min() == 88 and X["nblk"] == 968 and X["red_blocks"] == 3
    n, P, X = seen[(257, 257, 64)]
    assert n == 4227136 and P["passes"] == 2 and P["step"] == 0 and lanes_that_wrap(P, 64).size == 0
    n, P, X = seen[(1183, 1183, 3)]
    assert n == 4198467 and P["passes"] == 2 and P["step"] == 1 and P["tail"] == 3 and VEC > 2 * 3
    wrap = lanes_that_wrap(P, 3)
    assert wrap.size and set(wrap.tolist()) == {2} and X["nblk"] == 21868 and X["last"] == 1
    # the decoder only: the table is read from global memory and `% nlev` takes three whole columns off the stride
    n, P, X = seen[(2, 2, 1100000)]
    assert n == 4400000 and P["passes"] == 2 and not P["in_lds"] and P["lds"] == 0
    assert P["step"] == 894304 == PASS - 3 * 1100000 and X["cpb"] == 0
    assert set(E.STRIDE_DECODE_ONLY) == {(2, 2, 1100000)} and set(E.STRIDE_CENSUS) < set(E.STRIDE)
    sizes = sorted(E.STRIDE, key=lambda s: s[0] * s[1] * s[2])
    assert set(E.STRIDE_CENSUS) == set(sizes[:2])                # (the census leaves out the two largest)


@pytest.mark.parametrize("shape", [s for s in E.STRIDE if s not in E.STRIDE_DECODE_ONLY], ids=E.tag_of)
def test_every_level_of_a_stride_field_has_its_own_scale_and_offset(shape):
    q, scl, off = E.encoded(shape)
    assert len(set(scl.tolist())) == shape[2] and len(set(off.tolist())) == shape[2]
    check_reference(E.field(shape), (q, scl, off))
    hq, hscl, hoff = E.hand_codes(shape)
    assert len(set(hscl.tolist())) == shape[2] and len(set(hoff.tolist())) == shape[2]
    assert {0, 65533, 65534, 65535} <= set(hq.reshape(-1)[:8].tolist())


def test_the_tall_column_has_a_pair_of_its_own_for_every_level():
    q, scl, off = E.hand_codes((2, 2, 1100000))
    assert len(set(scl.tolist())) == 1100000 and len(set(off.tolist())) == 1100000


# ---- the reference on the new encode cases -----------------------------------------------------------------------------

def check_reference(x, enc=None):
    """What tests/test_pack_cpu.py asserts of the old cases: the round trip within half a step and a float ulp, code 0 in
    every level and 65533 in every level that is not constant."""
    q, scl, off = R.encode(x) if enc is None else enc
    assert int(q.max()) <= R.TOP
    assert np.isfinite(scl).all() and np.isfinite(off).all() and (scl > 0).all() and not np.signbit(off[off == 0]).any()
    back = R.decode(q, scl, off)
    err = np.abs(back.astype(np.float64) - x.astype(np.float64))
    assert (err <= scl / 2 + R.ulp_float(back)).all()
    flat, cols = E.columns(q), E.columns(x)
    const = cols.min(axis=0) == cols.max(axis=0)
    assert (flat.min(axis=0) == 0).all() and (flat.max(axis=0)[~const] == R.TOP).all() and (scl[const] == 1).all()
    return q, scl, off


# ---- DEPTH -------------------------------------------------------------------------------------------------------------

def test_the_depth_grids_give_a_slice_of_the_reduction_a_second_partial():
    want = {(2, 520, 3): (64, 17, 16, 1), (2, 1056, 3): (64, 33, 64, 1), (33, 32, 70): (64, 17, 32, 2),
            (40, 26, 256): (63, 17, 32, 4)}
    assert set(want) == set(E.DEPTH_GRIDS)
    for shape, (cpb, nblk, last, red_blocks) in want.items():
        X = extremes_plan(shape[0] * shape[1], shape[2])
        assert (X["cpb"], X["nblk"], X["last"], X["red_blocks"]) == (cpb, nblk, last, red_blocks), shape
        assert X["lds"] <= LDS_BYTES and nblk > RED_PARTS
        per_slice = [len(range(part, nblk, RED_PARTS)) for part in range(RED_PARTS)]
        assert max(per_slice) >= 2 and (nblk != 17 or per_slice == [2] + [1] * 15)
    assert extremes_plan(40 * 26, 256)["last"] < 63 and extremes_plan(2 * 520, 3)["last"] < 64      # ragged last workgroups


@pytest.mark.parametrize("name", sorted(E.DEPTH))
def test_a_planted_value_decides_its_level_from_workgroup_16_or_later(name):
    x, plants = E.DEPTH[name]
    levels, groups = E.DEPTH_GRIDS[x.shape]
    X = extremes_plan(x.shape[0] * x.shape[1], x.shape[2])
    cols = E.columns(x)
    assert plants
    for what, lev, col in plants:
        wg = col // X["cpb"]
        assert lev in levels and wg >= RED_PARTS and (wg in groups or wg == X["nblk"] - 1)
        part = wg % RED_PARTS
        assert list(range(part, X["nblk"], RED_PARTS)).index(wg) >= 1          # the slice's second partial or a later one
        if what in ("min", "max"):
            pick = np.argmin if what == "min" else np.argmax
            v = cols[:, lev]
            assert pick(v) == col and (v == v[col]).sum() == 1                  # no other workgroup holds an equal one
            if what == "max":
                assert col == len(v) - 1
        else:
            sign = np.signbit(cols[:, lev])
            assert (cols[:, lev] == 0).all() and col == RED_PARTS * X["cpb"]
            early = what == "zeros_neg_first"
            assert (sign[:col] == early).all() and (sign[col:] != early).all()
    q, scl, off = check_reference(x)
    for what, lev, col in plants:
        if what == "min":
            assert q[np.unravel_index(col, x.shape[:2])][lev] == 0 and off[lev] == cols[col, lev]
        elif what == "max":
            assert q[np.unravel_index(col, x.shape[:2])][lev] == R.TOP
        else:
            assert off[lev] == 0 and not np.signbit(off[lev]) and scl[lev] == 1 and (q[:, :, lev] == 0).all()
    whats = {p[0] for _, pl in E.DEPTH.values() for p in pl}
    assert whats == {"min", "max", "zeros_neg_first", "zeros_pos_first"}
    assert any(p[2] // 64 == 32 for _, pl in E.DEPTH.values() for p in pl if p[0] == "min")     # (likewise workgroup 32)


@pytest.mark.parametrize("name", sorted(E.DEPTH_NOT_FINITE))
def test_a_value_that_is_not_finite_sits_in_workgroup_16_or_the_last_column_only(name):
    x, lev, col = E.DEPTH_NOT_FINITE[name]
    X = extremes_plan(x.shape[0] * x.shape[1], x.shape[2])
    cols = E.columns(x)
    bad = ~np.isfinite(cols)
    assert bad.sum() == 1 and bad[col, lev] and lev > 0
    assert (np.isnan(cols[col, lev]) if name.startswith("nan") else np.isposinf(cols[col, lev]))
    wg = col // X["cpb"]
    assert wg == (X["nblk"] - 1 if "_last_" in name else RED_PARTS) and wg >= RED_PARTS
    assert ("_last_" not in name) or col == cols.shape[0] - 1
    with pytest.raises(R.NotFinite) as e:
        R.encode(x)
    assert e.value.level == lev
    assert len(E.DEPTH_NOT_FINITE) == 4 * len(E.DEPTH_GRIDS)


# ---- HEADS -------------------------------------------------------------------------------------------------------------

def test_the_heads_hold_every_corner_of_the_scalar_head_and_tail():
    assert [nx * ny * nlev for nx, ny, nlev in E.HEADS] == [4, 6, 8, 9, 12, 15, 16, 20, 25, 75]
    assert E.SHIFTS == tuple(range(8)) and any(s[2] == 1 for s in E.HEADS)
    behind = set()
    for nx, ny, nlev in E.HEADS:
        n = nx * ny * nlev
        for shift in E.SHIFTS:
            P = plan(n, nlev, shift)
            assert P["head"] == min(n, (8 - shift) % 8) and P["head"] + P["nvec"] * VEC + P["tail"] == n
            assert P["blocks"] == 1 and P["passes"] <= 1 and 0 <= P["tail"] < VEC and P["in_lds"]
            if n < (8 - shift) % 8:
                behind.add("n < head")
                assert P["nvec"] == 0 and P["tail"] == 0
            else:
                behind.add(n - P["head"])
                assert P["nvec"] == (n - P["head"]) // 8
    assert {"n < head", 0, 1, 7, 8, 9} <= behind
    assert {plan(n, 1, s)["head"] for n in (25,) for s in E.SHIFTS} == set(range(8))
    for shape in E.HEADS:
        check_reference(E.field(shape))


# ---- LIMITS ------------------------------------------------------------------------------------------------------------

def test_the_limits_stand_on_both_sides_of_every_border():
    got = {}
    for shape in E.LIMITS:
        nx, ny, nlev = shape
        P, X = plan(nx * ny * nlev, nlev), extremes_plan(nx * ny, nlev)
        got[nlev] = (P["in_lds"], P["lds"], X["cpb"], X["lds"])
        assert P["lds"] <= LDS_BYTES and X["lds"] <= LDS_BYTES and P["passes"] == 1
        if shape not in E.LIMITS_REFUSED:
            check_reference(E.field(shape))
    assert got[4096][:2] == (True, 65536) and got[4097][:2] == (False, 0)
    assert got[255][2:] == (64, 65280) and got[256][2:] == (63, 64764)
    assert got[16383][2:] == (1, 65532) and got[16384][2] == 0
    assert set(E.LIMITS_REFUSED) == {(2, 2, 16384)} and sorted(got) == [255, 256, 4096, 4097, 16383, 16384]
