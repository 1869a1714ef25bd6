"""Seeded cases of the 16-bit packed level fields, shared by tests/test_pack_cpu.py and tests/test_gpu_pack*.py.

Grids (nx, ny, nlev), small ones at which the arithmetic of a value can go wrong: 9 x 7 x 20; 37 x 19 x 137 (703 columns:
several workgroups of the extremes kernel with a ragged last one, and 137 is no multiple of 8); 5 x 5 x 3 (75 values: the
8-wide path has a tail, and a lane's 8 values wrap the level more than once); 2 x 2 x 2; 2 x 2 x 4099 (a tall axis past the
LDS table of 4096 levels).  None of them reaches the grid stride of the streaming kernels, a second partial in a slice of
the reduction, more than two alignments of the code array, one level or the LDS limits themselves: those cases are in
tests/pack_edge_cases.py.

ENCODE: name -> float32 field, all finite.  DECODE: name -> (codes, scl, off, lo, hi), codes chosen by hand, scl / off also
NaN and infinite.  NOT_FINITE: name -> (field, first level that is not finite)."""
import numpy as np

GRIDS = ((9, 7, 20), (37, 19, 137), (5, 5, 3), (2, 2, 2), (2, 2, 4099))


def smooth(nx, ny, nlev, seed=0):
    """A temperature-like field: a trend along the levels, waves along the columns, a little seeded noise."""
    rng = np.random.default_rng(1000 + seed)
    ix, iy, ip = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nlev), indexing="ij")
    x = 288.0 - 70.0 * ip / max(nlev - 1, 1) + 12.0 * np.sin(0.7 * ix + 0.1 * ip) * np.cos(0.9 * iy) \
        + rng.normal(0.0, 0.3, (nx, ny, nlev))
    return x.astype(np.float32)


def _encode_cases():
    out = {}
    for g, (nx, ny, nlev) in enumerate(GRIDS):
        tag = f"{nx}x{ny}x{nlev}"
        x = smooth(nx, ny, nlev, g)
        out[f"smooth_{tag}"] = x
        # a constant level (scl = 1); a level whose minimum is the first and whose maximum is the very last value of the field
        y = x.copy()
        y[:, :, 0] = np.float32(273.15)
        y[:, :, -1] = np.clip(y[:, :, -1], 200.0, 300.0)
        y[0, 0, -1] = np.float32(150.0)
        y[-1, -1, -1] = np.float32(350.0)
        out[f"edges_{tag}"] = y
        # negative values and zeros of both signs: a level of zeros only, a level whose maximum is -0.f
        z = -np.abs(x) * np.float32(0.01)
        z[:, :, 0] = 0.0
        z[::2, :, 0] = -0.0
        z[0, 0, -1] = -0.0
        out[f"negative_{tag}"] = z.astype(np.float32)
        out[f"tiny_{tag}"] = (x * np.float32(1e-9)).astype(np.float32)
        out[f"huge_{tag}"] = (x * np.float32(1e6)).astype(np.float32)
        # scl = 1 exactly (the level spans 0 ... 65533) and values k + 0.5: (x - off) / scl + .5 is an integer
        rng = np.random.default_rng(2000 + g)
        h = (rng.integers(0, 65533, (nx, ny, nlev)) + 0.5).astype(np.float32)
        h[0, 0, :] = 0.0
        h[-1, -1, :] = 65533.0
        out[f"halves_{tag}"] = h
    return out


def _decode_cases():
    out = {}
    special = np.array([0, 1, 65533, 65534, 65535, 32768, 255, 256], dtype=np.uint16)
    for g, (nx, ny, nlev) in enumerate(GRIDS):
        tag = f"{nx}x{ny}x{nlev}"
        rng = np.random.default_rng(3000 + g)
        q = rng.integers(0, 65536, (nx, ny, nlev)).astype(np.uint16)
        flat = q.reshape(-1)
        flat[-len(special):] = special[::-1]        # (the smallest grid has 8 values: the first eight win there)
        flat[:len(special)] = special
        scl = 10.0 ** rng.uniform(-6.0, 1.0, nlev)
        off = rng.normal(0.0, 50.0, nlev)
        out[f"hand_{tag}"] = (q, scl, off, -1e34, 1e34)
        out[f"hand_t_{tag}"] = (q, scl, off, 0.0, 1e34)                 # the limits of t: negative values become 0
        out[f"hand_cc_{tag}"] = (q, scl * 1e-5, off * 1e-2, 0.0, 1.0)   # ... of cc
        # scl / off that are not finite, through both pairs of limits
        s2, o2 = scl.copy(), off.copy()
        s2[0] = np.nan
        o2[-1] = np.inf
        if nlev > 2:
            s2[1] = np.inf
            o2[2] = -np.inf
        if nlev > 4:
            s2[3] = -np.inf
            o2[4] = np.nan
        out[f"wild_t_{tag}"] = (q, s2, o2, 0.0, 1e34)
        out[f"wild_cc_{tag}"] = (q, s2, o2, 0.0, 1.0)
    return out


def _not_finite_cases():
    x = smooth(9, 7, 20)
    a, b, c = x.copy(), x.copy(), x.copy()
    a[3, 2, 5] = np.nan
    b[8, 6, 19] = np.inf
    c[0, 0, 0] = -np.inf
    c[4, 4, 7] = np.nan
    return {"nan": (a, 5), "inf_last": (b, 19), "minus_inf_first": (c, 0)}


ENCODE = _encode_cases()
DECODE = _decode_cases()
NOT_FINITE = _not_finite_cases()
