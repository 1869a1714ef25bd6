"""Seeded edge cases of the 16-bit packed level fields that tests/pack_cases.py is too small to reach, shared by
tests/test_pack_edges_cpu.py (which asserts that every case reaches what it is named for) and tests/test_gpu_pack_edges*.py.
The grids (nx, ny, nlev) are the smallest that take each path of the launch code (pack_stream and mphip_pack_met in
mptrac_amd/csrc/mphip_api.hip, the kernels of mphip_pack.hpp):

STRIDE   more values than one pass of the streaming kernels (2048 workgroups x 256 lanes x 8 values = 4 194 304): the
         grid-stride loop runs again and the level of a lane advances by step = 4 194 304 mod nlev.
DEPTH    more than 16 workgroups of the extremes kernel: a slice of the reduction takes a second partial, and the value
         that decides a level lives in workgroup 16 or later, or in the ragged last workgroup, only.
HEADS    n = 4 ... 75 values, each with the code array 0 ... 7 elements behind a 16-byte boundary: the scalar head and tail
         of the streaming kernels, n < head, n == head, fewer than 8 values behind the head, and nlev = 1.
LIMITS   nlev at both sides of the LDS table of the streaming kernels (4096 | 4097) and of the columns per workgroup of the
         extremes kernel (255 | 256, and 16 383 | 16 384: one column in 64 KB | the refusal).

The large arrays are built on first use and kept (a field of 8.5 M values costs most of a second); nothing here is changed
by a test."""
import functools

import numpy as np

import pack_cases as K
import refpack as R

SHIFTS = tuple(range(8))            # code elements between a 16-byte boundary and the first code

# ---- STRIDE ------------------------------------------------------------------------------------------------------------
STRIDE = ((257, 241, 137), (257, 257, 64), (1183, 1183, 3), (2, 2, 1100000))
STRIDE_DECODE_ONLY = ((2, 2, 1100000),)         # the encoder refuses its levels
STRIDE_CENSUS = ((257, 257, 64), (1183, 1183, 3))       # (the census leaves out the two largest)


def tag_of(shape):
    return "x".join(str(k) for k in shape)


@functools.lru_cache(maxsize=None)
def field(shape):
    """The smooth field of a grid (its seed is the grid's): every level has its own minimum and range."""
    x = K.smooth(*shape, seed=sum(shape))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def hand_codes(shape):
    """(codes, scl, off) as pack_cases._decode_cases makes them: seeded codes with the special ones at both ends, and a
    scale and an offset of its own for every level (a level decoded with its neighbour's pair differs in every value)."""
    nlev = shape[2]
    rng = np.random.default_rng(5000 + sum(shape))
    q = rng.integers(0, 65536, shape, dtype=np.uint16)
    special = np.array([0, 1, 65533, 65534, 65535, 32768, 255, 256], dtype=np.uint16)
    flat = q.reshape(-1)
    if flat.size >= 2 * len(special):
        flat[-len(special):] = special[::-1]
    flat[:len(special)] = special[:flat.size]
    scl = 10.0 ** rng.uniform(-6.0, 1.0, nlev)
    off = rng.normal(0.0, 50.0, nlev)
    for a in (q, scl, off):
        a.setflags(write=False)
    return q, scl, off


@functools.lru_cache(maxsize=None)
def encoded(shape):
    """refpack.encode of field(shape)."""
    out = R.encode(field(shape))
    for a in out:
        a.setflags(write=False)
    return out


# ---- DEPTH -------------------------------------------------------------------------------------------------------------
# grid -> (the three levels that are edited, the workgroups of the extremes kernel whose columns take a planted value)
DEPTH_GRIDS = {(2, 520, 3): ((0, 1, 2), (16,)), (2, 1056, 3): ((0, 1, 2), (16, 32)), (33, 32, 70): ((5, 66, 69), (16,)),
               (40, 26, 256): ((0, 130, 255), (16,))}


def columns_per_workgroup(nlev):
    """mphip_pack_met: the columns a workgroup of the extremes kernel stages within 64 KB at the pitch nlev | 1."""
    return min(64, 65536 // ((nlev | 1) * 4))


def columns(x):
    """The field as [column][level], a view: column = ix ny + iy, the order the kernels see."""
    return x.reshape(-1, x.shape[2])


def _depth_cases():
    """DEPTH: name -> (field, plants), plants = [(what, level, column)] with what in min | max (the level's only extreme),
    zeros_neg_first | zeros_pos_first (the column of the first zero of the other sign).  DEPTH_NOT_FINITE: name -> (field,
    level, column)."""
    finite, bad = {}, {}
    for shape, (levels, groups) in DEPTH_GRIDS.items():
        tag = tag_of(shape)
        cpb = columns_per_workgroup(shape[2])
        ncol = shape[0] * shape[1]
        first = [g * cpb + 3 for g in groups]            # a column inside workgroup 16 (32), not its first one
        base = K.smooth(*shape, seed=sum(shape))
        la, lb, lc = levels
        # the minimum of a level in workgroup 16 only (and of another in workgroup 32), the maximum in the last column
        x = base.copy()
        c = columns(x)
        plants = [("min", la, first[0]), ("max", lb, ncol - 1)]
        c[first[0], la] = c[:, la].min() - np.float32(50.0)
        c[ncol - 1, lb] = c[:, lb].max() + np.float32(50.0)
        if len(first) > 1:
            c[first[1], lc] = c[:, lc].min() - np.float32(50.0)
            plants.append(("min", lc, first[1]))
        finite[f"extremes_{tag}"] = (x, plants)
        # a level of zeros: one sign in workgroups 0 ... 15, the other from workgroup 16 on
        for name, early in (("zeros_neg_first", -0.0), ("zeros_pos_first", 0.0)):
            x = base.copy()
            c = columns(x)
            c[:16 * cpb, lb] = np.float32(early)
            c[16 * cpb:, lb] = np.float32(-early)
            finite[f"{name}_{tag}"] = (x, [(name, lb, 16 * cpb)])
        for what, value in (("nan", np.nan), ("inf", np.inf)):
            for where, col, lev in (("wg16", first[0], lc), ("last", ncol - 1, lb)):
                x = base.copy()
                columns(x)[col, lev] = np.float32(value)
                bad[f"{what}_{where}_{tag}"] = (x, lev, col)
    return finite, bad


DEPTH, DEPTH_NOT_FINITE = _depth_cases()

# ---- HEADS -------------------------------------------------------------------------------------------------------------
HEADS = ((2, 2, 1), (2, 3, 1), (2, 2, 2), (3, 3, 1), (2, 2, 3), (3, 5, 1), (2, 2, 4), (2, 2, 5), (5, 5, 1), (5, 5, 3))

# ---- LIMITS ------------------------------------------------------------------------------------------------------------
LIMITS = ((2, 2, 4096), (2, 2, 4097), (2, 2, 255), (2, 2, 256), (2, 2, 16383), (2, 2, 16384))
LIMITS_REFUSED = ((2, 2, 16384),)               # by the encoder: no column fits 64 KB of LDS at the pitch nlev | 1
