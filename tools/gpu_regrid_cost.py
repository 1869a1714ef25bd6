#!/usr/bin/env python3
"""Cost of mphip_regrid_met on the grid of workload C3 (721 x 361 columns, the synthetic snapshot of bench.py taken as 137
model levels whose pressure follows the surface pressure), all eleven level fields:
  ml2pl     137 model levels to 60 pressure levels,
  sample    MET_DX MET_DY MET_DP = 2 2 1, MET_SX MET_SY MET_SP = 2 2 1 on the 721 x 361 x 60 result of ml2pl,
  both      the two in one call.
Per kernel the device time (one worker under `rocprofv3 --kernel-trace --stats`, no counters in that run; --rounds + 1
calls per variant in a fixed order, the first of each dropped), the bytes it must move (every input value once, every
output value once) and the resulting rate; per call the wall time (host clock; the call returns when the results are in
the caller's arrays) next to the mphip_update_met of the same snapshot, in a second worker without the profiler.
Writes profiles/regrid_cost.json and prints it as one JSON line.
  tools/gpu_regrid_cost.py [--grid C3] [--rounds R]"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FIELDS = ("u", "v", "w", "t", "h2o", "o3", "lwc", "rwc", "iwc", "swc", "cc", "ps", "pbl", "cape", "cin", "pel", "pct", "pcb",
          "cl", "ess", "nss", "shf")
MET_NP = 60
SAMPLE = dict(met_dx=2, met_dy=2, met_dp=1, met_sx=2, met_sy=2, met_sp=1)
VARIANTS = ("ml2pl", "sample", "both")


def setup(grid):
    import numpy as np
    import cases
    from mptrac_amd import hip
    from mptrac_amd.synth import synthetic_met
    ctl, clim, _, _, atm = cases.make_case("advect", n=1000, grid="tiny")
    met = synthetic_met(grid, 0.0, 1.0, fields=FIELDS)
    sim = hip.Simulation(ctl, clim, met, met, atm)
    ml = hip.Snapshot(met.time, met.coord_type, met.lon, met.lat, met.p, dict(met.f3), dict(met.f2))
    ml.f3["pl"] = np.ascontiguousarray(met.p[None, None, :] * (met.f2["ps"].astype(np.float64) / met.p[0])[:, :, None],
                                       dtype=np.float32)
    met_p = np.exp(np.linspace(np.log(1000.0), np.log(1.2 * met.p[-1]), MET_NP))
    return sim, met, ml, met_p


def calls(sim, ml, met_p):
    first = sim.regrid_met(ml, "ml2pl", met_p=met_p)
    return {"ml2pl": lambda: sim.regrid_met(ml, "ml2pl", met_p=met_p),
            "sample": lambda: sim.regrid_met(first, "sample", **SAMPLE),
            "both": lambda: sim.regrid_met(ml, ("ml2pl", "sample"), met_p=met_p, **SAMPLE)}, first


def worker_trace(grid, rounds):
    sim, met, ml, met_p = setup(grid)
    fn, first = calls(sim, ml, met_p)        # (one more ml2pl call in front of the timed ones)
    for name in VARIANTS:
        for _ in range(rounds + 1):
            got = fn[name]()
    out = {"grid": [met.nx, met.ny, met.np], "met_np": MET_NP, "sampled": [got.nx, got.ny, got.np],
           "library": sim.L.mphip_version().decode(), "level_fields": len(first.f3), "surface_fields": len(first.f2)}
    sim.close()
    print("JSON " + json.dumps(out), flush=True)


def worker_wall(grid, rounds):
    sim, met, ml, met_p = setup(grid)
    fn, _ = calls(sim, ml, met_p)
    out = {}
    sim.set_met(1, met)
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        sim.set_met(1, met)
        ms.append((time.perf_counter() - t0) * 1e3)
    out["update_met"] = {"wall_ms": min(ms), "wall_ms_all": ms}
    for name in VARIANTS:
        fn[name]()
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            fn[name]()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"wall_ms": min(ms), "wall_ms_all": ms}
    sim.close()
    print("JSON " + json.dumps(out), flush=True)


def _json_line(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith("JSON ")][-1][5:])


def kernel_times(trace_csv, rounds, info):
    """Per variant and kernel: device ms per call (the launches of one call summed), bytes and GB/s."""
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))

    def of(name):
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows if name in r["Kernel_Name"]]

    def per_call(ms, launches, ncalls):
        assert len(ms) == launches * ncalls, (len(ms), launches, ncalls)
        return [sum(ms[i * launches:(i + 1) * launches]) for i in range(ncalls)]

    def summary(ms, launches, nbytes):
        best = min(ms)
        return {"launches_per_call": launches, "min_ms": best, "median_ms": statistics.median(ms), "all_ms": ms,
                "bytes": nbytes, "gb_per_s": nbytes / best * 1e-6}
    nx, ny, npl = info["grid"]
    nx2, ny2, np2 = info["sampled"]
    n3, n2, mnp = info["level_fields"], info["surface_fields"], info["met_np"]
    ncol, ncol2 = nx * ny, nx2 * ny2
    b_ml = 4 * ncol * ((n3 + 1) * npl + n3 * mnp)
    b_s3, b_s2 = 4 * n3 * (ncol * mnp + ncol2 * np2), 4 * n2 * (ncol + ncol2)
    r1 = rounds + 1
    ml = of("regrid_ml2pl_kernel")           # 1 call in front, then ml2pl x r1 and both x r1
    lev, sur = of("regrid_sample_kernel<16>"), of("regrid_sample_kernel<1>")
    assert len(ml) == 1 + 2 * r1 and len(lev) == 2 * r1 * n3 and len(sur) == 2 * r1 * n2, (len(ml), len(lev), len(sur))
    lev_calls, sur_calls = per_call(lev, n3, 2 * r1), per_call(sur, n2, 2 * r1)
    return {
        "ml2pl": {"regrid_ml2pl_kernel": summary(ml[2:1 + r1], 1, b_ml)},
        "sample": {"regrid_sample_kernel<16>": summary(lev_calls[1:r1], n3, b_s3),
                   "regrid_sample_kernel<1>": summary(sur_calls[1:r1], n2, b_s2)},
        "both": {"regrid_ml2pl_kernel": summary(ml[2 + r1:], 1, b_ml),
                 "regrid_sample_kernel<16>": summary(lev_calls[r1 + 1:], n3, b_s3),
                 "regrid_sample_kernel<1>": summary(sur_calls[r1 + 1:], n2, b_s2)},
    }


def main():
    from mptrac_amd.synth import GRIDS
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="C3", choices=sorted(GRIDS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--worker", choices=("trace", "wall"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regrid_cost.json"))
    args = ap.parse_args()
    if args.worker:
        return (worker_trace if args.worker == "trace" else worker_wall)(args.grid, args.rounds)
    me = [sys.executable, os.path.abspath(__file__), "--grid", args.grid, "--rounds", str(args.rounds), "--worker"]
    prof = tempfile.mkdtemp(prefix="regrid_cost_")
    r = subprocess.run(["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", prof, "-o", "t", "--",
                        *me, "trace"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    out = _json_line(r.stdout)
    out["rounds"] = args.rounds
    out["sample_options"] = SAMPLE
    out["kernels"] = kernel_times(glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)[0], args.rounds, out)
    r = subprocess.run(["timeout", "-k", "10", "420", *me, "wall"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    out["calls"] = _json_line(r.stdout)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
