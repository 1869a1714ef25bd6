#!/usr/bin/env python3
"""Cost of the analysis outputs on the device: workload C3 of bench.py (10^7 particles) after 20 time steps, ms per call of
  mphip_box_sums on a 360 x 180 x 1 grid with a weighting function (a CSI grid) and on a 36 x 18 x 60 grid (profiles),
  mphip_sample_obs with 500 observations in the time step at SAMPLE_DX 50 and 800 km,
  mphip_station_hits at 800 km,
each beside mphip_get_atm of the same context in the same process -- the download of all particles is the floor of the
path these calls replace, before any host loop runs.  Writes profiles/analysis_outputs_cost.json and prints it.
Kernel statistics: `rocprofv3 --kernel-trace --stats -- python tools/gpu_analysis_outputs_cost.py` (a separate run).
  tools/gpu_analysis_outputs_cost.py [--steps K] [--rounds R] [--particles N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bench                     # noqa: E402  (inputs of the workloads)
from mptrac_amd import hip       # noqa: E402

KERNEL = (np.array([0.0, 5.0, 12.0, 30.0]), np.array([0.2, 1.0, 0.6, 0.1]))


def timed(fn, rounds):
    fn()                         # (buffers are allocated by the first call)
    best = float("inf")
    for _ in range(rounds):
        t0 = time.perf_counter()
        out = fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--particles", type=float, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analysis_outputs_cost.json"))
    args = ap.parse_args()
    ctl, clim, met0, met1, atm, _, _ = bench.build_inputs("C3", 0, 1, args.steps + 2, int(args.particles) or None)
    sim = hip.Simulation(ctl, clim, met0, met1, atm)
    sim.timesteps_init(atm["time"].min(), atm["time"].max())
    dt = sim.ctl.dt_mod
    sim.run_timestep(0.0)
    sim.run_timesteps(dt, args.steps)
    sim.synchronize()
    t = args.steps * dt
    qm = sim.ctl.qnt_m
    state = sim.get_atm()
    rng = np.random.default_rng(1)
    pick = rng.integers(0, sim.n, 500)          # observations where particles are
    olon, olat = state["lon"][pick], state["lat"][pick]
    oz = 7.0 * np.log(1013.25 / state["p"][pick])
    res = {"workload": "C3", "particles": sim.n, "steps": args.steps, "rounds": args.rounds, "ms": {}, "found": {}}
    res["ms"]["get_atm"], _ = timed(lambda: sim.get_atm(state), args.rounds)
    res["ms"]["box_sums_360x180x1_kernel"], s = timed(
        lambda: sim.box_sums((-180.0, 180.0, 360, -90.0, 90.0, 180, 0.0, 100.0, 1), t, qm, kernel=KERNEL), args.rounds)
    res["found"]["box_sums_360x180x1_kernel"] = float(s.sum())
    res["ms"]["box_sums_36x18x60"], s = timed(
        lambda: sim.box_sums((-180.0, 180.0, 36, -90.0, 90.0, 18, 0.0, 60.0, 60), t, qm), args.rounds)
    res["found"]["box_sums_36x18x60"] = float(s.sum())
    for dx in (50.0, 800.0):
        key = "sample_obs_500_dx%d" % dx
        res["ms"][key], (count, _) = timed(lambda dx=dx: sim.sample_obs(t - 0.5 * dt, t + 0.5 * dt, olon, olat, oz, dx, 2.0, KERNEL),
                                           args.rounds)
        res["found"][key] = int(count.sum())
    res["ms"]["station_hits_800"], (nhit, _, _) = timed(
        lambda: sim.station_hits(t, float(olon[0]), float(olat[0]), 800.0, -1e100, 1e100, cap=1 << 20), args.rounds)
    res["found"]["station_hits_800"] = int(nhit)
    res["beats_download"] = {k: v < res["ms"]["get_atm"] for k, v in res["ms"].items() if k != "get_atm"}
    sim.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
