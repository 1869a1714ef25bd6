"""The 16-bit packed level fields of MET_TYPE 2 files, restated in numpy from the definition in include/mptrac_hip.h (at
mphip_met_packed_t), independently of the device code: every operation is numpy's IEEE operation on the named type, one
ufunc per operation, so nothing is fused.

A level field is float32 [nx][ny][nlev]; codes are uint16 of the same shape; scl / off are float64 [nlev]."""
import numpy as np

OPEN = (-1e34, 1e34)        # limits that leave every decoded finite value of a meteo field alone
TOP = 65533                 # the largest code the encoder writes


class NotFinite(ValueError):
    """encode(): a level holds a value that is not finite (`level`: the first such level)."""

    def __init__(self, level):
        super().__init__(f"a value that is not finite at level {level}")
        self.level = level


def encode(x):
    """(codes, scl, off) of a field.  Per level: min and max over all columns as doubles; off = min + 0. (a zero of either
    sign becomes +0.); scl = (max != min) ? (max - min) / 65533. : 1.; q = (unsigned short) (((double) x - off) / scl + .5)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3
    xd = x.astype(np.float64)
    bad = ~np.isfinite(xd).all(axis=(0, 1))
    if bad.any():
        raise NotFinite(int(np.flatnonzero(bad)[0]))
    mn = xd.min(axis=(0, 1)) + 0.0
    mx = xd.max(axis=(0, 1))
    rng = mx - mn
    scl = np.where(mx != mn, rng / 65533., 1.)
    d = xd - mn
    r = d / scl
    h = r + .5
    return h.astype(np.uint16), scl, mn         # (0.5 <= h < 65534: the conversion truncates)


def clamp(v, lo, hi):
    """fminf(fmaxf(v, lo), hi) as the C library evaluates them: the first argument unless the comparison says otherwise --
    a NaN becomes lo, a zero that equals a limit keeps its sign."""
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(invalid="ignore"):
        v = np.where(v >= lo, v, lo)
        return np.where(v <= hi, v, hi).astype(np.float32)


def decode(q, scl, off, lo=OPEN[0], hi=OPEN[1]):
    """The floats of codes: v = (float) ((double) q * scl[ip] + off[ip]) -- product, sum, one rounding to float -- and the
    limits.  Every code decodes, whatever scl and off are."""
    q = np.asarray(q)
    assert q.dtype == np.uint16
    with np.errstate(all="ignore"):
        prod = q.astype(np.float64) * np.asarray(scl, dtype=np.float64)
        total = prod + np.asarray(off, dtype=np.float64)
        v = total.astype(np.float32)
    return clamp(v, lo, hi)


def roundtrip(x, lo=OPEN[0], hi=OPEN[1]):
    return decode(*encode(x), lo, hi)


def ulp_float(a):
    """The spacing of float32 at |a|."""
    return np.spacing(np.abs(np.asarray(a, dtype=np.float32))).astype(np.float64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
