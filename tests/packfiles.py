"""MET_TYPE 2 files (16-bit packed level fields) from numpy, for the driver tests: the layout of hostfiles.write_met_bin
with every level field as scl[np] doubles, off[np] doubles and nx ny np unsigned shorts, encoded by tests/refpack.py."""
import struct

import numpy as np

import refpack as R
from hostfiles import LEVEL_ORDER as LEVEL, SURF_ORDER as SURFACE, met_filename

VERSION = 104
# the limits the reader applies to the level fields, in file order (z, t, u, v, w, pv, h2o, o3, lwc, rwc, iwc, swc, cc)
LIMITS = {"z": R.OPEN, "t": (0.0, 1e34), "u": R.OPEN, "v": R.OPEN, "w": R.OPEN, "pv": R.OPEN, "h2o": (0.0, 1e34),
          "o3": (0.0, 1e34), "lwc": (0.0, 1e34), "rwc": (0.0, 1e34), "iwc": (0.0, 1e34), "swc": (0.0, 1e34), "cc": (0.0, 1.0)}


def met_pck_filename(metbase, t):
    return met_filename(metbase, t)[:-3] + "pck"


def level_field(met, name):
    """The field as the reader of a MET_TYPE 1 file hands it on: zeros if the snapshot lacks it, within the reader's limits."""
    f = met.f3.get(name)
    if f is None:
        return np.zeros((met.nx, met.ny, met.np), dtype=np.float32)
    return R.clamp(np.ascontiguousarray(f, dtype=np.float32), *LIMITS[name])


def met_pck_bytes(met):
    """The bytes of the MET_TYPE 2 file of a snapshot (a field the snapshot lacks is written as zeros, as in type 1)."""
    parts = [struct.pack("<ii", 2, VERSION), struct.pack("<d", met.time), struct.pack("<iii", met.nx, met.ny, met.np)]
    parts += [np.asarray(a, dtype="<f8").tobytes() for a in (met.lon, met.lat, met.p)]
    for name in SURFACE:
        f = met.f2.get(name)
        parts.append((np.zeros((met.nx, met.ny), dtype="<f4") if f is None else np.ascontiguousarray(f, dtype="<f4")).tobytes())
    for name in LEVEL:
        q, scl, off = R.encode(level_field(met, name))
        parts += [scl.astype("<f8").tobytes(), off.astype("<f8").tobytes(), q.astype("<u2").tobytes()]
    parts.append(struct.pack("<i", 999))
    return b"".join(parts)


def write_met_pck(path, met):
    with open(path, "wb") as f:
        f.write(met_pck_bytes(met))


def file_size(nx, ny, np_):
    """The exact size of a MET_TYPE 2 file from its shape: header and axes, 24 float planes, 13 level fields of 16 np bytes
    of scales and offsets and 2 bytes per value, the trailer."""
    return 8 + 8 + 12 + 8 * (nx + ny + np_) + 24 * 4 * nx * ny + 13 * (16 * np_ + 2 * nx * ny * np_) + 4


def decoded(met):
    """The snapshot as a reader of its MET_TYPE 2 file sees it: every level field replaced by decode(encode(.)) within the
    field's limits (a copy; the surface fields are shared)."""
    import copy
    out = copy.copy(met)
    out.f3 = dict(met.f3)
    for name in LEVEL:
        if name in met.f3:
            out.f3[name] = R.roundtrip(level_field(met, name), *LIMITS[name])
    return out
