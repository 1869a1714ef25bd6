"""mphip_unpack_met and mphip_pack_met (through Simulation.unpack_met / pack_met) against tests/refpack.py, the restatement
of the definition in include/mptrac_hip.h, on the cases of tests/pack_cases.py: every comparison is bit for bit, in the
library this process loaded (tests/test_gpu_pack_exact.py runs the same checks in the other one and compares the bytes of
the two).

The decoder: every case into compact arrays, into views of arrays with the fixed extents of a met_t (the padding survives),
and from a code array that starts one element behind a 16-byte boundary (the scalar head of the kernel).  The encoder:
scl, off and codes; into an unaligned code array too.  Refusals return their message and write nothing."""
import hashlib

import numpy as np
import pytest

import pack_cases as K
import refpack as R
from mptrac_amd import hip
from mptrac_amd.hip import Snapshot
from test_gpu_regrid import bare_context, padding_untouched

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-7777.)
TAGS = [f"{nx}x{ny}x{nlev}" for nx, ny, nlev in K.GRIDS]


def grid_of(shape, field="t"):
    """A snapshot that carries nothing but the extents of a field (pack_met / unpack_met read no axis)."""
    nx, ny, nlev = shape
    s = Snapshot(0.0, 0, np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nlev, 0, -1.0), {}, {})
    return s


def unaligned(a, shift=1):
    """A C-contiguous copy of `a` that starts `shift` elements behind a 64-byte boundary."""
    raw = np.empty(a.size + 64, dtype=a.dtype)
    skew = (-raw.ctypes.data % 64) // a.itemsize + shift
    view = raw[skew:skew + a.size].reshape(a.shape)
    view[...] = a
    assert view.ctypes.data % 16 == shift * a.itemsize and view.flags["C_CONTIGUOUS"]
    return view


def decode_cases(tag):
    """name -> (codes, scl, off, lo, hi): the hand-made ones, and the restatement's codes of every finite case through
    open limits and through those of t."""
    out = {k: v for k, v in K.DECODE.items() if k.endswith("_" + tag)}
    for k, x in K.ENCODE.items():
        if k.endswith("_" + tag):
            q, scl, off = R.encode(x)
            out["enc_" + k] = (q, scl, off, *R.OPEN)
            out["enc_t_" + k] = (q, scl, off, 0.0, 1e34)
    return out


def unpack_one(sim, case, how="compact"):
    q, scl, off, lo, hi = case
    met = grid_of(q.shape)
    if how == "unaligned":
        q = unaligned(q)
    if how == "strided":
        big = np.full((q.shape[0], q.shape[1] + 3, q.shape[2] + 5), SENTINEL, dtype=np.float32)
        view = big[:, :q.shape[1], :q.shape[2]]
        got = sim.unpack_met(met, {"t": (q, scl, off, lo, hi)}, out={"t": view},
                             out_strides=((q.shape[1] + 3) * (q.shape[2] + 5), q.shape[2] + 5))["t"]
        assert got is view and padding_untouched(view)
        return got
    return sim.unpack_met(met, {"t": (q, scl, off, lo, hi)})["t"]


def pack_one(sim, x, how="compact"):
    met = grid_of(x.shape)
    met.f3["t"] = x
    if how == "unaligned":
        out = {"t": (unaligned(np.zeros(x.shape, dtype=np.uint16), 3), np.empty(x.shape[2]), np.empty(x.shape[2]))}
        return sim.pack_met(met, out=out)["t"]
    return sim.pack_met(met)["t"]


def census(sim):
    """Every case through both calls: (rows that differ from the restatement, sha256 of every byte the library returned)."""
    digest = hashlib.sha256()
    wrong = []
    for tag in TAGS:
        for name, case in sorted(decode_cases(tag).items()):
            ref = R.decode(*case)
            for how in ("compact", "strided", "unaligned"):
                got = unpack_one(sim, case, how)
                digest.update(np.ascontiguousarray(got).tobytes())
                if not R.same_bits(got, ref):
                    wrong.append(("unpack", name, how))
        for name, x in sorted(K.ENCODE.items()):
            if not name.endswith("_" + tag):
                continue
            ref = R.encode(x)
            for how in ("compact", "unaligned"):
                got = pack_one(sim, x, how)
                for g, r in zip(got, ref):
                    digest.update(np.ascontiguousarray(g).tobytes())
                    if not R.same_bits(g, r):
                        wrong.append(("pack", name, how))
    return wrong, digest.hexdigest()


@pytest.fixture(scope="module")
def sim():
    s = bare_context()
    yield s
    s.close()


@pytest.mark.parametrize("how", ["compact", "strided", "unaligned"])
@pytest.mark.parametrize("tag", TAGS)
def test_unpack_met_gives_the_restatement_bits(sim, tag, how):
    cases = decode_cases(tag)
    assert len(cases) == 5 + 2 * 6
    for name, case in cases.items():
        ref = R.decode(*case)
        got = unpack_one(sim, case, how)
        assert not np.isnan(ref).any()          # (a NaN becomes lo: none survives the limits, on either side)
        assert R.same_bits(got, ref), (name, int((got.view(np.uint32) != ref.view(np.uint32)).sum()))


@pytest.mark.parametrize("how", ["compact", "unaligned"])
@pytest.mark.parametrize("tag", TAGS)
def test_pack_met_gives_the_restatement_bits(sim, tag, how):
    names = [k for k in K.ENCODE if k.endswith("_" + tag)]
    assert len(names) == 6
    for name in names:
        q, scl, off = pack_one(sim, K.ENCODE[name], how)
        rq, rscl, roff = R.encode(K.ENCODE[name])
        assert R.same_bits(scl, rscl) and R.same_bits(off, roff), name
        assert R.same_bits(q, rq), (name, int((q != rq).sum()))
        assert int(q.max()) <= R.TOP


def test_several_fields_in_one_call_and_a_field_that_is_skipped(sim):
    a, b, c = (K.ENCODE[k + "_37x19x137"] for k in ("smooth", "edges", "negative"))
    met = grid_of(a.shape)
    met.f3.update(t=a, u=b, w=c)
    got = sim.pack_met(met, fields=("t", "u"))
    assert sorted(got) == ["t", "u"]
    for f, x in (("t", a), ("u", b)):
        assert all(R.same_bits(g, r) for g, r in zip(got[f], R.encode(x)))
    back = sim.unpack_met(grid_of(a.shape), {"t": got["t"], "u": got["u"] + R.OPEN})
    assert R.same_bits(back["t"], R.decode(*got["t"], 0.0, 1e34)) and R.same_bits(back["u"], R.decode(*got["u"]))
    # model-level fields take npl levels
    ml = grid_of((9, 7, 20))
    ml.np, ml.npl = 4, 20
    ml.p = ml.p[:4]
    ml.f3["ul"] = K.ENCODE["smooth_9x7x20"]
    q, scl, off = sim.pack_met(ml)["ul"]
    assert all(R.same_bits(g, r) for g, r in zip((q, scl, off), R.encode(ml.f3["ul"])))
    del ml.f3["ul"]
    assert R.same_bits(sim.unpack_met(ml, {"ul": (q, scl, off)})["ul"], R.decode(q, scl, off))


# ---- refusals: the message, and nothing written ---------------------------------------------------------------------------

def sentinel_outputs(shape):
    return (np.full(shape, 4242, dtype=np.uint16), np.full(shape[2], -1.5), np.full(shape[2], -2.5))


def untouched(out):
    return bool((out[0] == 4242).all() and (out[1] == -1.5).all() and (out[2] == -2.5).all())


@pytest.mark.parametrize("name", sorted(K.NOT_FINITE))
def test_pack_met_refuses_a_value_that_is_not_finite(sim, name):
    x, level = K.NOT_FINITE[name]
    met = grid_of(x.shape)
    met.f3.update(u=K.smooth(*x.shape), t=x)          # (a field that is fine is not written either)
    out = {"t": sentinel_outputs(x.shape), "u": sentinel_outputs(x.shape)}
    with pytest.raises(hip.MphipError, match=rf"mphip_pack_met: field t holds a value that is not finite at level {level}$"):
        sim.pack_met(met, out=out)
    assert untouched(out["t"]) and untouched(out["u"])


def test_a_field_given_twice_and_codes_without_scl_are_refused(sim):
    x = K.ENCODE["smooth_9x7x20"]
    q, scl, off = R.encode(x)
    met = grid_of(x.shape)
    met.f3["t"] = x.copy()
    target = np.full(x.shape, SENTINEL, dtype=np.float32)
    with pytest.raises(hip.MphipError, match="mphip_unpack_met: field t is given both as floats and as codes"):
        sim.unpack_met(met, {"t": (q, scl, off)}, out={"t": target})
    met = grid_of(x.shape)
    for rec, what in (((q, None, off), "without scl or off"), ((q, scl, None), "without scl or off"),
                      ((q, scl, off, 1.0, 0.0), "lo <= hi"), ((q, scl, off, np.nan, 1.0), "lo <= hi")):
        with pytest.raises(hip.MphipError, match="mphip_unpack_met: field t.*" + what):
            sim.unpack_met(met, {"t": rec}, out={"t": target})
    assert (target == SENTINEL).all()
    # the encoder: codes to write without a place for scl
    met.f3["t"] = x
    out = {"t": (np.full(x.shape, 4242, dtype=np.uint16), None, np.full(20, -2.5))}
    with pytest.raises(hip.MphipError, match="mphip_pack_met: field t is given as codes without scl or off"):
        sim.pack_met(met, out=out)
    assert (out["t"][0] == 4242).all() and (out["t"][2] == -2.5).all()
    # strides that do not hold the grid; nothing to do
    with pytest.raises(hip.MphipError, match="mphip_unpack_met: the output strides do not hold the grid"):
        m = sim._met_packed_struct(grid_of(x.shape), {"t": (q, scl, off)})
        mo = hip.MphipMet()
        mo.sx, mo.sy = 7 * 20, 19
        mo.f3[hip.FIELDS_3D.index("t")] = hip._ptr(target, hip._fp)
        sim._chk(sim.L.mphip_unpack_met(sim.h, m, mo))
    with pytest.raises(hip.MphipError, match="mphip_pack_met: no field"):
        sim.pack_met(grid_of(x.shape))
    assert (target == SENTINEL).all()


def test_the_whole_census_has_no_row_that_differs(sim):
    wrong, digest = census(sim)
    assert wrong == [] and len(digest) == 64
