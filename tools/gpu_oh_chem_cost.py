#!/usr/bin/env python3
"""Cost of module_oh_chem in the time step: workload C3 of bench.py (same inputs, particle count and time loop -- one
mphip_run_timesteps call for the timed steps after untimed warm-up steps) with SPECIES SO2's OH chemistry (reaction 3,
OH_CHEM of the preset) on and off, alternating in one process.  Prints one JSON line with ms per step of both and the
ratio.  Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_oh_chem_cost.py` (a
separate run).
Counters: `rocprofv3 --pmc ... -- python tools/gpu_oh_chem_cost.py --mode on` (and --mode off), a run per mode.
  tools/gpu_oh_chem_cost.py [--steps K] [--warmup W] [--rounds R] [--particles N] [--mode both|on|off]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bench                     # noqa: E402  (inputs of the workloads)
import refchem                   # noqa: E402
import refclim                   # noqa: E402
from mptrac_amd import hip       # noqa: E402


def run(oh_on, args):
    steps_total = args.warmup + args.steps + 1
    ctl, clim, met0, met1, atm, _, _ = bench.build_inputs("C3", 0, 1, steps_total, args.particles or None)
    if oh_on:
        ctl.update(oh_chem_reaction=refchem.PRESETS["SO2"][0], oh_chem=refchem.PRESETS["SO2"][1])
    clim = clim + ({"oh": refclim.synthetic_zonal_mean(8, scale=1e-12)},)
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
    m = sim.get_atm()["q"][ctl["qnt_m"]] if ctl.get("qnt_m", -1) >= 0 else np.zeros(1)
    sim.close()
    return ms, float(np.sum(m))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--particles", type=float, default=0)
    ap.add_argument("--mode", choices=("both", "on", "off"), default="both",
                    help="on / off: one configuration only (a counter run of its own, rocprofv3 --pmc)")
    args = ap.parse_args()
    if args.mode != "both":
        ms, _ = run(args.mode == "on", args)
        print(json.dumps({"workload": "C3", "species": "SO2", "mode": args.mode, "ms_per_step": ms}))
        return
    on, off, mass = [], [], {}
    for _ in range(args.rounds):
        for flag, dst in ((False, off), (True, on)):
            ms, msum = run(flag, args)
            dst.append(ms)
            mass[flag] = msum
    res = {"workload": "C3", "species": "SO2", "steps": args.steps, "warmup": args.warmup,
           "ms_per_step_off": min(off), "ms_per_step_on": min(on), "ratio": min(on) / min(off),
           "all_off": off, "all_on": on, "mass_sum_off": mass[False], "mass_sum_on": mass[True]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
