#!/usr/bin/env python3
"""Cost of MPHIP_PREP_PV and MPHIP_PREP_TROPO of mphip_derive_met on the grid of workload C3 (721 x 361 x 137, the synthetic
snapshot of bench.py with the fields the derivation reads and a temperature field that has a tropopause; z and pv are given,
so that every bit is timed alone):
  the device time of prep_pv_kernel, of prep_pv_polar_kernel and of prep_tropo_kernel for met_tropo 1 ... 5 (cubic spline):
    one worker process under `rocprofv3 --kernel-trace --stats` (no counters in that run), which makes --rounds + 1 calls
    per variant in a fixed order; the dispatches are told apart by that order and the first of each variant (scratch
    allocation, code objects) is dropped; the smallest and the median of the rest are reported,
  the wall time of the whole call (host clock; the call returns when the results are in the caller's arrays) with the five
    bits of HIP_MET_PREP 1 and with all seven (met_tropo 3), in a second worker process without the profiler -- same
    machine, same session.
Writes profiles/pv_tropo_cost.json and prints it as one JSON line.
  tools/gpu_pv_tropo_cost.py [--grid C3] [--rounds R]"""
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

FIELDS = ("u", "v", "w", "t", "h2o", "z", "pv", "o3", "lwc", "rwc", "iwc", "swc", "ps", "pbl", "cape", "cin", "pel", "pct", "pcb",
          "cl", "ts", "zs", "us", "vs")
OLD = ("geopot", "o3c", "pbl", "cloud", "cape")
MODES = (1, 2, 3, 4, 5)


def setup(grid):
    import numpy as np
    import cases
    from mptrac_amd import hip
    from mptrac_amd.synth import synthetic_met
    ctl, clim, _, _, atm = cases.make_case("advect", n=1000, grid="tiny")
    met = synthetic_met(grid, 0.0, 1.0, fields=FIELDS)
    # the synthetic temperature has no tropopause (the searches would end at their first point): 6.5 K/km up to a tropopause
    # between 9 and 16.5 km that varies with latitude and longitude, isothermal above
    z = 7. * np.log(1013.25 / met.p)
    lat, lon = np.radians(met.lat)[None, :, None], np.radians(met.lon)[:, None, None]
    ztrop = 12.5 + 3.5 * np.cos(2. * lat) + 0.5 * np.sin(3. * lon)
    met.f3["t"] = np.ascontiguousarray(288. + 15. * np.cos(lat) - 6.5 * np.minimum(z[None, None, :], ztrop), dtype=np.float32)
    return hip.Simulation(ctl, clim, met, met, atm), met


def worker_trace(grid, rounds):
    import numpy as np
    sim, met = setup(grid)
    finite = {}
    for _ in range(rounds + 1):
        sim.derive_met(met, "pv")
    for mode in MODES:
        for _ in range(rounds + 1):
            got = sim.derive_met(met, "tropo", met_tropo=mode)
        finite[str(mode)] = int(np.isfinite(got["pt"]).sum())
    out = {"grid": [met.nx, met.ny, met.np], "library": sim.L.mphip_version().decode(), "finite_pt": finite}
    sim.close()
    print("JSON " + json.dumps(out), flush=True)


def worker_wall(grid, rounds):
    sim, met = setup(grid)
    out = {}
    for name, what in (("old_five_bits", OLD), ("all_seven_bits", OLD + ("pv", "tropo")), ("pv", ("pv",)), ("tropo_3", ("tropo",))):
        sim.derive_met(met, what)
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            sim.derive_met(met, what)
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"wall_ms": min(ms), "wall_ms_all": ms}
    sim.close()
    print("JSON " + json.dumps(out), flush=True)


def _json_line(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith("JSON ")][-1][5:])


def kernel_times(trace_csv, rounds):
    """{variant: {min_ms, median_ms}} from the dispatches of the kernel trace, in the worker's order."""
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))

    def of(name):
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows if name in r["Kernel_Name"]]

    def summary(ms):
        return {"min_ms": min(ms), "median_ms": statistics.median(ms), "all_ms": ms}
    pv, polar, tropo = of("prep_pv_kernel"), of("prep_pv_polar_kernel"), of("prep_tropo_kernel")
    assert len(pv) == len(polar) == rounds + 1 and len(tropo) == len(MODES) * (rounds + 1), (len(pv), len(polar), len(tropo))
    out = {"prep_pv_kernel": summary(pv[1:]), "prep_pv_polar_kernel": summary(polar[1:])}
    for i, mode in enumerate(MODES):
        out["prep_tropo_kernel_met_tropo_%d" % mode] = summary(tropo[i * (rounds + 1) + 1:(i + 1) * (rounds + 1)])
    return out


def main():
    from mptrac_amd.synth import GRIDS
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="C3", choices=sorted(GRIDS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--worker", choices=("trace", "wall"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pv_tropo_cost.json"))
    args = ap.parse_args()
    if args.worker:
        return (worker_trace if args.worker == "trace" else worker_wall)(args.grid, args.rounds)
    me = [sys.executable, os.path.abspath(__file__), "--grid", args.grid, "--rounds", str(args.rounds), "--worker"]
    prof = tempfile.mkdtemp(prefix="pv_tropo_cost_")
    r = subprocess.run(["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", prof, "-o", "t", "--",
                        *me, "trace"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    out = _json_line(r.stdout)
    out["rounds"] = args.rounds
    out["kernels"] = kernel_times(glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)[0], args.rounds)
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
