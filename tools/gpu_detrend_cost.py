#!/usr/bin/env python3
"""Cost of mphip_detrend_met on the grid of workload C3 (721 x 361 x 137, the synthetic snapshot of bench.py), the four
fields t, u, v, w, with MET_DETREND 500, 1000 and 2000 km.  Per scale, each figure the best of --rounds calls after a
warm-up call:
  kernel_ms   the stencil kernel (device events around its launch: option derive_profile_phase 0),
  table_ms    the host's build of the weight table (derive_profile_phase 3),
  wall_ms     the whole call (host clock; the call returns when the results are in the caller's arrays),
next to the mphip_update_met of the same snapshot in the same process, the taps per point (mean over the points, and the
largest), the table's size, and the achieved rate: one multiply and one add per tap, field and point (they are not fused:
the definition rounds the product), against the FP32 vector peak of 157.3 TFLOP/s, which counts a fused multiply-add
as two operations -- separate multiplies and adds can reach half of it unless they are issued as packed instructions.
Writes profiles/detrend_cost.json and prints it as one JSON line.
  tools/gpu_detrend_cost.py [--grid C3] [--rounds R]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FIELDS = ("t", "u", "v", "w")
SCALES = (500.0, 1000.0, 2000.0)
PEAK_FP32_VECTOR = 157.3e12


def main():
    import numpy as np
    import cases
    import refdetrend as R
    from mptrac_amd import hip
    from mptrac_amd.synth import GRIDS, synthetic_met
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="C3", choices=sorted(GRIDS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detrend_cost.json"))
    args = ap.parse_args()

    ctl, clim, _, _, atm = cases.make_case("advect", n=1000, grid="tiny")
    met = synthetic_met(args.grid, 0.0, 1.0, fields=FIELDS)
    sim = hip.Simulation(ctl, clim, met, met, atm)
    out = {"grid": [met.nx, met.ny, met.np], "fields": len(FIELDS), "rounds": args.rounds,
           "library": sim.L.mphip_version().decode(), "peak_fp32_vector_flops": PEAK_FP32_VECTOR, "scales": {}}
    sim.set_met(1, met)
    ms = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        sim.set_met(1, met)
        ms.append((time.perf_counter() - t0) * 1e3)
    out["update_met"] = {"wall_ms": min(ms), "wall_ms_all": ms}
    res = {f: np.empty_like(met.f3[f]) for f in FIELDS}
    points = met.nx * met.ny * met.np
    for scale in SCALES:
        sy, sx = R.half_widths(met.lon, met.lat, scale)
        taps = R.taps(met.lon, met.lat, scale)
        table = sum((min(iy + sy, met.ny - 1) - max(iy - sy, 0) + 1) * (sx[iy] + 1) for iy in range(met.ny))
        row = {"sy": sy, "sx_min": min(sx), "sx_max": max(sx), "taps_mean": sum(taps) / len(taps), "taps_max": max(taps),
               "table_floats": table}
        sim.detrend_met(met, scale, out=res)        # warm-up: code object, scratch
        kernel, wall, build = [], [], []
        for phase, into in ((0, kernel), (3, build)):
            sim.set_option("derive_profile_phase", phase)
            for _ in range(args.rounds):
                sim.profile_begin()
                t0 = time.perf_counter()
                sim.detrend_met(met, scale, out=res)
                if phase == 0:
                    wall.append((time.perf_counter() - t0) * 1e3)
                pairs, t_ms = sim.profile_end()
                assert pairs == 1, pairs
                into.append(t_ms)
        sim.set_option("derive_profile_phase", 0)
        madds = float(len(FIELDS)) * points * row["taps_mean"]
        row.update(kernel_ms=min(kernel), kernel_ms_all=kernel, table_ms=min(build), table_ms_all=build, wall_ms=min(wall),
                   wall_ms_all=wall, multiply_adds=madds, multiply_adds_per_s=madds / (min(kernel) * 1e-3),
                   share_of_fp32_vector_peak=2.0 * madds / (min(kernel) * 1e-3) / PEAK_FP32_VECTOR)
        out["scales"][str(int(scale))] = row
    sim.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
