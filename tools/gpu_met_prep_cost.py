#!/usr/bin/env python3
"""Cost of mphip_derive_met (the derived fields of the meteo preprocessing, HIP_MET_PREP) on the grid of workload C3
(721 x 361 x 137, the synthetic snapshot of bench.py with the fields the derivation reads): per MPHIP_PREP_* bit and for
all bits together
  the wall time of the call (host clock; the call returns when the results are in the caller's arrays),
  the device time of every kernel, of the uploads and of the downloads -- event pairs of the library on the call's own
    stream (mphip_profile_begin / _end with the option "derive_profile_phase" 0 / 1 / 2), each in a call of its own
    outside the timed ones,
and, as the yardstick, the wall time of mphip_update_met for the same snapshot (what the time loop pays per file anyway).
Every variant is warmed up once (scratch allocation, code objects); the smallest of --rounds calls is reported beside all
of them.  Writes profiles/met_prep_cost.json and prints it as one JSON line.
  tools/gpu_met_prep_cost.py [--grid C3] [--rounds R]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cases                                   # noqa: E402
from mptrac_amd import hip                     # noqa: E402
from mptrac_amd.synth import GRIDS, synthetic_met   # noqa: E402

FIELDS = ("u", "v", "w", "t", "h2o", "z", "o3", "lwc", "rwc", "iwc", "swc", "ps", "pbl", "cape", "cin", "pel", "pct", "pcb", "cl",
          "ts", "zs", "us", "vs")
VARIANTS = {
    "geopot": (("geopot",), {}),
    "geopot_unsmoothed": (("geopot",), dict(met_geopot_sx=0, met_geopot_sy=0)),
    "o3c": (("o3c",), {}),
    "pbl_3": (("pbl",), dict(met_pbl=3)),
    "pbl_2_given_z": (("pbl",), dict(met_pbl=2)),
    "cloud": (("cloud",), {}),
    "cape": (("cape",), {}),
    "all_pbl_3": (("geopot", "o3c", "pbl", "cloud", "cape"), dict(met_pbl=3)),
    "all_pbl_2": (("geopot", "o3c", "pbl", "cloud", "cape"), dict(met_pbl=2)),
}


def timed(fn, rounds):
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="C3", choices=sorted(GRIDS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "met_prep_cost.json"))
    args = ap.parse_args()
    ctl, clim, _, _, atm = cases.make_case("advect", n=1000, grid="tiny")
    met = synthetic_met(args.grid, 0.0, 1.0, fields=FIELDS)
    sim = hip.Simulation(ctl, clim, met, met, atm)
    out = {"grid": [met.nx, met.ny, met.np], "library": sim.L.mphip_version().decode(), "rounds": args.rounds, "variants": {}}
    sim.set_met(1, met)
    ms = timed(lambda: sim.set_met(1, met), args.rounds)
    out["update_met_wall_ms"] = min(ms)
    out["update_met_wall_ms_all"] = ms
    for name, (what, opts) in VARIANTS.items():
        def call():
            return sim.derive_met(met, what, **opts)
        call()
        ms = timed(call, args.rounds)
        row = {"wall_ms": min(ms), "wall_ms_all": ms}
        for phase, key in ((0, "kernels"), (1, "uploads"), (2, "downloads")):
            sim.set_option("derive_profile_phase", phase)
            sim.profile_begin()
            call()
            n, dev_ms = sim.profile_end()
            row[key + "_ms"] = dev_ms
            if phase == 0:
                row["kernel_launches"] = n
        sim.set_option("derive_profile_phase", 0)
        out["variants"][name] = row
    sim.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
