#!/usr/bin/env python3
"""Cost of the SO2 chemistry in the time step: workload C3 of bench.py (same particle count and time loop -- one
mphip_run_timesteps call for the timed steps after untimed warm-up steps; the meteo fields gain lwc and rwc) with
SPECIES SO2's OH chemistry alone ("oh") and with OH + H2O2 + Cx on the default chemistry grid ("so2"), alternating in
one process.  Prints one JSON line with ms per step of both and the ratio.  Kernel statistics: run it under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_h2o2_chem_cost.py` (a separate run).
  tools/gpu_h2o2_chem_cost.py [--steps K] [--warmup W] [--rounds R] [--particles N] [--mode both|oh|so2]"""
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
from mptrac_amd.synth import synthetic_met   # noqa: E402

OH = refclim.synthetic_zonal_mean(8, scale=1e-12)
H2O2 = refclim.synthetic_zonal_mean(9, scale=1e-9)


def so2_inputs(mode, steps_total, particles=None):
    """C3's inputs with cloud water, SO2's OH chemistry and (mode "so2") the H2O2 chemistry and quantity Cx"""
    ctl, clim, met0, met1, atm, _, _ = bench.build_inputs("C3", 0, 1, steps_total, particles)
    fields = bench.WORKLOADS["C3"][4] + ("lwc", "rwc")
    met0 = synthetic_met("C3", met0.time, 1.0, fields=fields)
    met1 = synthetic_met("C3", met1.time, 1.25, fields=fields)
    ctl.update(oh_chem_reaction=refchem.PRESETS["SO2"][0], oh_chem=refchem.PRESETS["SO2"][1], molmass=64.066,
               chemgrid_nx=360, chemgrid_ny=180, chemgrid_nz=1, chemgrid_lon0=-180.0, chemgrid_lon1=180.0,
               chemgrid_lat0=-90.0, chemgrid_lat1=90.0, chemgrid_z0=-5.0, chemgrid_z1=85.0)   # (the default grid)
    if mode == "so2":
        n = len(atm["time"])
        atm["q"] = np.vstack([atm["q"], np.zeros((1, n))])
        ctl.update(h2o2_chem_reaction=1, qnt_Cx=ctl["nq"], nq=ctl["nq"] + 1)
    return ctl, clim + ({"oh": OH, "h2o2": H2O2},), met0, met1, atm


def run(mode, args):
    steps_total = args.warmup + args.steps + 1
    ctl, clim, met0, met1, atm = so2_inputs(mode, steps_total, args.particles or None)
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
    m = sim.get_atm()["q"][ctl["qnt_m"]]
    sim.close()
    return ms, float(np.sum(m))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--particles", type=float, default=0)
    ap.add_argument("--mode", choices=("both", "oh", "so2"), default="both")
    args = ap.parse_args()
    if args.particles:
        args.particles = int(args.particles)
    if args.mode != "both":
        ms, _ = run(args.mode, args)
        print(json.dumps({"workload": "C3", "species": "SO2", "mode": args.mode, "ms_per_step": ms}))
        return
    res = {"oh": [], "so2": []}
    mass = {}
    for _ in range(args.rounds):
        for mode in ("oh", "so2"):
            ms, msum = run(mode, args)
            res[mode].append(ms)
            mass[mode] = msum
    print(json.dumps({"workload": "C3", "species": "SO2", "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step_oh": min(res["oh"]), "ms_per_step_oh_h2o2_cx": min(res["so2"]),
                      "ratio": min(res["so2"]) / min(res["oh"]), "all_oh": res["oh"], "all_oh_h2o2_cx": res["so2"],
                      "mass_sum_oh": mass["oh"], "mass_sum_oh_h2o2_cx": mass["so2"]}))


if __name__ == "__main__":
    main()
