"""mphip_unpack_met and mphip_pack_met on the cases of tests/pack_edge_cases.py -- the grid-stride loop of the streaming
kernels, a reduction of the extremes that is deeper than its 16 slices, every scalar head and tail, nlev = 1 and the LDS
limits -- against tests/refpack.py, bit for bit, in the library this process loaded (tests/test_gpu_pack_edges_exact.py runs
edge_census in the other one and compares the bytes of the two).  tests/test_pack_edges_cpu.py asserts without a device that
every case reaches the path it is named for.

Every check is a row (label, arrays the library returned, arrays of the restatement): the tests assert the rows of their
group one by one, edge_census takes them all."""
import functools
import hashlib

import numpy as np
import pytest

import pack_edge_cases as E
import refpack as R
from mptrac_amd import hip
from test_gpu_pack import grid_of, pack_one, sentinel_outputs, unaligned, unpack_one, untouched
from test_gpu_regrid import bare_context

pytestmark = pytest.mark.gpu
PASS = 4194304                      # values of one pass of the streaming kernels
LIMITS_T = (0.0, 1e34)              # the reader's limits of t: negative values become 0
TOO_TALL = "mphip_pack_met: too many levels for one column in 64 KB of LDS$"


@pytest.fixture(scope="module")
def sim():
    s = bare_context()
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def decoded(shape, lo, hi):
    """refpack.decode of the hand-made codes of a grid, kept."""
    return R.decode(*E.hand_codes(shape), lo, hi)


def unpack_at(sim, case, shift=None):
    """unpack_met into a compact array; the codes start `shift` elements behind a 16-byte boundary (None: as they are)."""
    if shift is None:
        return unpack_one(sim, case)
    return unpack_one(sim, (unaligned(case[0], shift),) + tuple(case[1:]))


def pack_at(sim, x, shift=None):
    """pack_met (codes, scl, off); into a code array that starts `shift` elements behind a 16-byte boundary."""
    if shift is None:
        return pack_one(sim, x)
    met = grid_of(x.shape)
    met.f3["t"] = x
    out = {"t": (unaligned(np.zeros(x.shape, dtype=np.uint16), shift), np.empty(x.shape[2]), np.empty(x.shape[2]))}
    return sim.pack_met(met, out=out)["t"]


def first_difference(got, ref):
    """None, or (values that differ, flat index of the first one, the pass of the streaming kernel it belongs to)."""
    if R.same_bits(got, ref):
        return None
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.dtype, ref.shape)
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    differ = np.flatnonzero(np.ascontiguousarray(got).reshape(-1).view(bits) != np.ascontiguousarray(ref).reshape(-1).view(bits))
    return int(differ.size), int(differ[0]), int(differ[0]) // PASS


def differing(row):
    label, got, ref = row
    assert len(got) == len(ref)
    return [(label, k) + d for k, (g, r) in enumerate(zip(got, ref)) for d in [first_difference(g, r)] if d]


# ---- the rows ----------------------------------------------------------------------------------------------------------

def unpack_rows(sim, shape, combos):
    q, scl, off = E.hand_codes(shape)
    for shift, (lo, hi) in combos:
        got = unpack_at(sim, (q, scl, off, lo, hi), shift)
        yield ("unpack", E.tag_of(shape), shift, lo), (got,), (decoded(shape, lo, hi),)


def pack_rows(sim, shape, shifts, x=None, ref=None, name=None):
    x = E.field(shape) if x is None else x
    ref = (E.encoded(shape) if x is E.field(shape) else R.encode(x)) if ref is None else ref
    for shift in shifts:
        yield ("pack", name or E.tag_of(shape), shift), pack_at(sim, x, shift), ref


TWO = ((None, R.OPEN), (5, LIMITS_T))
FOUR = TWO + ((None, LIMITS_T), (5, R.OPEN))


def stride_rows(sim, shape, what=("unpack", "pack"), combos=FOUR):
    if "unpack" in what:
        yield from unpack_rows(sim, shape, combos)
    if "pack" in what and shape not in E.STRIDE_DECODE_ONLY:
        yield from pack_rows(sim, shape, (None, 3))


def depth_rows(sim):
    for name, (x, _) in sorted(E.DEPTH.items()):
        yield from pack_rows(sim, x.shape, (None,), x=x, name=name)


def heads_rows(sim, what=("unpack", "strided", "pack")):
    for shape in E.HEADS:
        q, scl, off = E.hand_codes(shape)
        for shift in E.SHIFTS:
            if "unpack" in what:
                yield from unpack_rows(sim, shape, ((shift, R.OPEN),))
            if "strided" in what:       # (unpack_one asserts that the padding of the view survives)
                got = unpack_one(sim, (unaligned(q, shift), scl, off) + LIMITS_T, "strided")
                yield ("unpack strided", E.tag_of(shape), shift), (got,), (decoded(shape, *LIMITS_T),)
            if "pack" in what:
                yield from pack_rows(sim, shape, (shift,))


def limits_rows(sim, shape):
    yield from unpack_rows(sim, shape, TWO)
    if shape not in E.LIMITS_REFUSED:
        yield from pack_rows(sim, shape, (None, 3))


def edge_census(sim, stride=E.STRIDE_CENSUS):
    """Every case through both calls, the STRIDE grids `stride` among them: (rows that differ from the restatement,
    sha256 of every byte the library returned)."""
    digest = hashlib.sha256()
    wrong = []

    def take(rows):
        for row in rows:
            for g in row[1]:
                digest.update(np.ascontiguousarray(g).tobytes())
            wrong.extend(list(map(str, d)) for d in differing(row))

    for shape in stride:
        take(stride_rows(sim, shape, combos=TWO))
    take(depth_rows(sim))
    take(heads_rows(sim))
    for shape in E.LIMITS:
        take(limits_rows(sim, shape))
    return wrong, digest.hexdigest()


def check(rows, at_least=1):
    count = 0
    for row in rows:
        assert differing(row) == [], row[0]
        count += 1
    assert count >= at_least


# ---- STRIDE ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", E.STRIDE, ids=E.tag_of)
def test_unpack_met_beyond_one_pass_gives_the_restatement_bits(sim, shape):
    """(a mismatch names: the values that differ, the flat index of the first one and its pass, index // 4 194 304)"""
    check(stride_rows(sim, shape, what=("unpack",)), 4)


@pytest.mark.parametrize("shape", [s for s in E.STRIDE if s not in E.STRIDE_DECODE_ONLY], ids=E.tag_of)
def test_pack_met_beyond_one_pass_gives_the_restatement_bits(sim, shape):
    check(stride_rows(sim, shape, what=("pack",)), 2)
    assert int(E.encoded(shape)[0].max()) == R.TOP


def test_pack_met_refuses_a_column_taller_than_the_lds_and_writes_nothing(sim):
    for shape in E.STRIDE_DECODE_ONLY + E.LIMITS_REFUSED:
        met = grid_of(shape)
        met.f3["t"] = E.field(shape)
        out = {"t": sentinel_outputs(shape)}
        with pytest.raises(hip.MphipError, match=TOO_TALL):
            sim.pack_met(met, out=out)
        assert untouched(out["t"])


# ---- DEPTH -------------------------------------------------------------------------------------------------------------

def test_pack_met_finds_the_extremes_behind_workgroup_16(sim):
    """scl, off and the codes, the sign of off included: +0. for a level of zeros whichever workgroups hold which sign."""
    check(depth_rows(sim), len(E.DEPTH))
    for name, (x, plants) in E.DEPTH.items():
        if name.startswith("zeros"):
            q, scl, off = pack_one(sim, x)
            lev = plants[0][1]
            assert off[lev] == 0 and not np.signbit(off[lev]) and scl[lev] == 1


@pytest.mark.parametrize("name", sorted(E.DEPTH_NOT_FINITE))
def test_pack_met_refuses_a_value_that_is_not_finite_behind_workgroup_16(sim, name):
    x, level, _ = E.DEPTH_NOT_FINITE[name]
    met = grid_of(x.shape)
    met.f3.update(u=E.field(x.shape), t=x)            # (a field that is fine is not written either)
    out = {"t": sentinel_outputs(x.shape), "u": sentinel_outputs(x.shape)}
    with pytest.raises(hip.MphipError, match=rf"mphip_pack_met: field t holds a value that is not finite at level {level}$"):
        sim.pack_met(met, out=out)
    assert untouched(out["t"]) and untouched(out["u"])


# ---- HEADS -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["unpack", "strided", "pack"])
def test_every_head_and_tail_gives_the_restatement_bits(sim, what):
    check(heads_rows(sim, what=(what,)), len(E.HEADS) * len(E.SHIFTS))


# ---- LIMITS ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", E.LIMITS, ids=E.tag_of)
def test_both_sides_of_the_lds_limits_give_the_restatement_bits(sim, shape):
    check(limits_rows(sim, shape), 2 if shape in E.LIMITS_REFUSED else 4)
