#!/usr/bin/env python3
"""Cost of the tracer chemistry in the time step: workload C3 of bench.py (same particle count and time loop -- one
mphip_run_timesteps call for the timed steps after untimed warm-up steps) with the four trace gases Cccl4, Cccl3f,
Cccl2f2, Cn2o added (and a total ozone column field, synthetic O(1D) and photolysis tables), TRACER_CHEM off ("off")
and on ("on"), alternating in one process.  Prints one JSON line with ms per step of both and the ratio.  Kernel
statistics: run it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_tracer_chem_cost.py` (a separate run).
  tools/gpu_tracer_chem_cost.py [--steps K] [--warmup W] [--rounds R] [--particles N] [--mode both|off|on]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bench                     # noqa: E402  (inputs of the workloads)
import refclim                   # noqa: E402
import reftracer                 # noqa: E402
from mptrac_amd import hip       # noqa: E402
from mptrac_amd.ctl import ctl_from_quantities   # noqa: E402

O1D = refclim.synthetic_zonal_mean(11, scale=1e-13)
PHOTO = reftracer.synthetic_photo(4)
NAMES = ("m", "rp", "rhop") + reftracer.SPECIES


def tracer_inputs(mode, steps_total, particles=None):
    """C3's inputs with the four trace gases, an o3c field and (mode "on") TRACER_CHEM"""
    ctl, clim, met0, met1, atm, _, _ = bench.build_inputs("C3", 0, 1, steps_total, particles)
    n = len(atm["time"])
    atm["q"] = np.vstack([atm["q"], np.full((4, n), 1e-10)])
    ctl.update(ctl_from_quantities(NAMES), tracer_chem=1 if mode == "on" else 0)
    for m in (met0, met1):
        lam = np.radians(m.lon)[:, None]
        phi = np.radians(m.lat)[None, :]
        m.f2["o3c"] = np.ascontiguousarray(300.0 + 60.0 * np.sin(phi) + 15.0 * np.cos(lam), dtype=np.float32)
    return ctl, clim + ({"o1d": O1D, "photo": PHOTO.upload_args()},), met0, met1, atm


def run(mode, args):
    steps_total = args.warmup + args.steps + 1
    ctl, clim, met0, met1, atm = tracer_inputs(mode, steps_total, args.particles or None)
    sim = hip.Simulation(ctl, clim, met0, met1, atm)
    sim.timesteps_init(atm["time"].min(), atm["time"].max())
    dt = sim.ctl.dt_mod
    for k in range(args.warmup):
        sim.run_timestep(k * dt)
    sim.synchronize()
    t0 = time.perf_counter()
    sim.run_timesteps(args.warmup * dt, args.steps)
    sim.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    q = sim.get_atm()["q"][3:7]
    sim.close()
    return ms, float(np.sum(q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--particles", type=float, default=0)
    ap.add_argument("--mode", choices=("both", "off", "on"), default="both")
    args = ap.parse_args()
    if args.particles:
        args.particles = int(args.particles)
    if args.mode != "both":
        ms, _ = run(args.mode, args)
        print(json.dumps({"workload": "C3", "tracers": NAMES[3:], "mode": args.mode, "ms_per_step": ms}))
        return
    res = {"off": [], "on": []}
    total = {}
    for _ in range(args.rounds):
        for mode in ("off", "on"):
            ms, qsum = run(mode, args)
            res[mode].append(ms)
            total[mode] = qsum
    print(json.dumps({"workload": "C3", "tracers": NAMES[3:], "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step_off": min(res["off"]), "ms_per_step_on": min(res["on"]),
                      "ratio": min(res["on"]) / min(res["off"]), "all_off": res["off"], "all_on": res["on"],
                      "tracer_sum_off": total["off"], "tracer_sum_on": total["on"]}))


if __name__ == "__main__":
    main()
