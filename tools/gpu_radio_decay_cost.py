#!/usr/bin/env python3
"""Cost of module_radio_decay in the time step: workload C3 of bench.py (same particle count and time loop -- one
mphip_run_timesteps call for the timed steps after untimed warm-up steps) in three variants, alternating in one process:
  "c3"   C3 unchanged,
  "off"  C3 with the six activities Arn222 ... Axe133 added as quantities (registered, RADIO_DECAY off),
  "on"   the same with RADIO_DECAY on.
Writes profiles/radio_decay_cost.json (ms per step of each, the ratio on / off, the step-kernel time per step and the
launches per step from the library's kernel events in a second, untimed run of as many steps, the step kernels' VGPRs
and scratch from the library's metadata) and prints it as one JSON line.
  tools/gpu_radio_decay_cost.py [--steps K] [--warmup W] [--rounds R] [--particles N] [--mode all|c3|off|on]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import bench                     # noqa: E402  (inputs of the workloads)
import refradio                  # noqa: E402
from mptrac_amd import hip       # noqa: E402
from mptrac_amd.ctl import ctl_from_quantities   # noqa: E402

NAMES = ("m", "rp", "rhop") + refradio.NAMES


def radio_inputs(mode, steps_total, particles=None):
    """C3's inputs; modes "off" / "on": with the six activities (1e3 ... 1e6 Bq, seeded) behind C3's quantities.
    Returns (ctl, clim, met0, met1, atm, the activity indices or None)."""
    ctl, clim, met0, met1, atm, _, _ = bench.build_inputs("C3", 0, 1, steps_total, particles)
    if mode == "c3":
        return ctl, clim, met0, met1, atm, None
    n = len(atm["time"])
    rng = np.random.default_rng(20261016)
    atm["q"] = np.vstack([atm["q"], 10.0 ** rng.uniform(3.0, 6.0, (len(refradio.NAMES), n))])
    ctl.update(ctl_from_quantities(NAMES))
    return ctl, clim, met0, met1, atm, [NAMES.index(x) for x in refradio.NAMES]


def run(mode, args):
    steps_total = args.warmup + 2 * args.steps + 1
    ctl, clim, met0, met1, atm, idx = radio_inputs(mode, steps_total, args.particles or None)
    sim = hip.Simulation(ctl, clim, met0, met1, atm)
    if idx is not None:
        sim.set_radio_decay(idx, on=(mode == "on"))
    sim.timesteps_init(atm["time"].min(), atm["time"].max())
    dt = sim.ctl.dt_mod
    for k in range(args.warmup):
        sim.run_timestep(k * dt)
    sim.synchronize()
    t0 = time.perf_counter()
    sim.run_timesteps(args.warmup * dt, args.steps)
    sim.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    sim.profile_begin()          # (the kernel events: a run of their own, outside the timed one)
    sim.run_timesteps((args.warmup + args.steps) * dt, args.steps)
    launches, kernel_ms = sim.profile_end()
    q = sim.get_atm()["q"][3:] if idx is not None else np.zeros(1)
    sim.close()
    return ms, kernel_ms / args.steps, launches / args.steps, float(np.sum(q))


def step_kernel_resources():
    import kernel_resources as kr
    import subprocess
    lib = hip.lib_path()
    out = []
    for r in kr.resources(lib):
        name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
        if "step_kernel" in name:
            out.append({"kernel": name, "vgpr": int(r["vgpr"]), "scratch": int(r["scratch"])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--particles", type=float, default=0)
    ap.add_argument("--mode", choices=("all", "c3", "off", "on"), default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radio_decay_cost.json"))
    args = ap.parse_args()
    if args.particles:
        args.particles = int(args.particles)
    modes = ("c3", "off", "on") if args.mode == "all" else (args.mode,)
    res = {m: [] for m in modes}
    kern = {m: [] for m in modes}
    total, launches = {}, {}
    for _ in range(args.rounds):
        for mode in modes:
            ms, kms, nl, qsum = run(mode, args)
            res[mode].append(ms)
            kern[mode].append(kms)
            launches[mode] = nl
            total[mode] = qsum
    out = {"workload": "C3", "particles": args.particles or 10 ** 7, "activities": refradio.NAMES, "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds}
    for m in modes:
        out[f"ms_per_step_{m}"] = min(res[m])
        out[f"all_{m}"] = res[m]
        out[f"step_kernel_ms_per_step_{m}"] = min(kern[m])
        out[f"launches_per_step_{m}"] = launches[m]
    if "on" in res and "off" in res:
        out["ratio_on_off"] = min(res["on"]) / min(res["off"])
        out["activity_sum_off"], out["activity_sum_on"] = total["off"], total["on"]
    out["step_kernels"] = step_kernel_resources()
    line = json.dumps(out)
    if args.mode == "all":
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
