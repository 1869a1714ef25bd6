#!/usr/bin/env python3
"""Cost of mphip_select_atm beside mphip_get_atm of the same context: workload C3 of bench.py (10^7 particles with its
quantities) after 20 time steps, the locality order in force.  Every figure is the best of --rounds after a warm-up, all
variants alternating in one process, every call into arrays that exist:
  get_atm            the download of everything (the floor of the path the selection replaces)
  stride1            every particle, all rows: the selection's worst case
  stride100          every hundredth particle, all rows
  stride100_window   ... of which a range keeps half (the time window if the particle times differ, else a height range)
  near_1pct          a disc around a particle that keeps about 1 %
each through the context's page-locked rows (the default) and with option select_direct 1 (straight into the caller's
arrays), as the whole call and as device events per stage (option select_profile_phase: mark, scan, list, row gathers,
copies).  --bench-parent-lib PATH: bench.py on C3 with that library and this tree's, alternating twice each.
Writes profiles/select_cost.json and prints it as one JSON line.
  tools/gpu_select_cost.py [--steps K] [--rounds R] [--particles N] [--bench-parent-lib PATH] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bench                     # noqa: E402  (inputs of the workloads)
from mptrac_amd import hip       # noqa: E402

PHASES = {1: "mark", 2: "scan", 3: "list", 4: "rows", 5: "copies"}
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


class Caller:
    """mphip_select_atm into arrays that exist (what a C caller's persistent buffers are)"""

    def __init__(self, sim):
        self.sim = sim
        n, nq = sim.n, sim.nq
        self.index = np.zeros(n, dtype=np.int32)
        self.rows = np.zeros((4 + nq, n))
        self.qp = (_dp * hip.NQ_MAX)()
        for iq in range(nq):
            self.qp[iq] = self.rows[4 + iq].ctypes.data_as(_dp)
        self.n = C.c_longlong(0)

    def __call__(self, sel):
        r = self.rows
        rc = self.sim.L.mphip_select_atm(self.sim.h, C.byref(sel), self.sim.n, C.byref(self.n), self.index.ctypes.data_as(_ip),
                                         r[0].ctypes.data_as(_dp), r[1].ctypes.data_as(_dp), r[2].ctypes.data_as(_dp),
                                         r[3].ctypes.data_as(_dp), self.qp)
        assert rc == 0, self.sim.L.mphip_last_error(self.sim.h).decode()
        return self.n.value


def selection(stride=1, time=None, z=None, near=None):
    s = hip.MphipSelect(first=0, last=-1, stride=stride)
    if time is not None:
        s.use_time, s.t0, s.t1 = 1, time[0], time[1]
    if z is not None:
        s.use_z, s.z0, s.z1 = 1, z[0], z[1]
    if near is not None:
        s.use_near, s.near_lon, s.near_lat, s.near_r = 1, near[0], near[1], near[2]
    return s


def bench_ab(parent_lib):
    runs, order = {}, ["parent1", "new", "parent2", "new2"]
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "3", "--no-cpu-baseline"]
    for name in order:
        env = dict(os.environ)
        env.pop("MPHIP_LIB", None)
        if name.startswith("parent"):
            env["MPHIP_LIB"] = os.path.abspath(parent_lib)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env, cwd=ROOT, timeout=600)
        assert r.returncode == 0, name
        d = json.loads(r.stdout.decode().strip().splitlines()[-1])
        assert d["unit"] == "particle-steps/s", d["unit"]
        runs[name] = {"particle_steps_per_s": d["value"], "ms_per_step": d["ms_per_step"]}
        print(name, json.dumps(runs[name]), flush=True)
    p = [runs["parent1"]["ms_per_step"], runs["parent2"]["ms_per_step"]]
    mean = sum(p) / 2
    return {"command": "bench.py --gpus 1 --steps 60 --warmup 3 --no-cpu-baseline", "order": order, "runs": runs,
            "parent_spread": abs(p[0] - p[1]) / mean,
            "new_over_parent_mean": [runs["new"]["ms_per_step"] / mean, runs["new2"]["ms_per_step"] / mean],
            "note": "parent: the library of the commit before this one, loaded through MPHIP_LIB into the same tree; one "
                    "session, one process per run"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--particles", type=float, default=0)
    ap.add_argument("--bench-parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_cost.json"))
    args = ap.parse_args()
    ctl, clim, met0, met1, atm, _, _ = bench.build_inputs("C3", 0, 1, args.steps + 2, int(args.particles) or None)
    sim = hip.Simulation(ctl, clim, met0, met1, atm)
    sim.timesteps_init(atm["time"].min(), atm["time"].max())
    dt = sim.ctl.dt_mod
    sim.run_timestep(0.0)
    sim.run_timesteps(dt, args.steps)
    sim.synchronize()
    state = sim.get_atm()
    # a range that keeps half: the time window if the times differ, else heights above the median
    if state["time"].min() < state["time"].max():
        half = dict(time=(float(np.median(state["time"])), float(state["time"].max())))
    else:
        half = dict(z=(float(np.median(7.0 * np.log(1013.25 / state["p"]))), 1e9))
    # a disc that keeps about 1 %: the 1 % quantile of the chord from a particle
    lam, phi = np.deg2rad(state["lon"]), np.deg2rad(state["lat"])
    xyz = 6367.421 * np.stack([np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)])
    chord = np.sqrt(((xyz - xyz[:, :1]) ** 2).sum(axis=0))
    disc = (float(state["lon"][0]), float(state["lat"][0]), float(np.quantile(chord, 0.01)))
    del xyz, chord, lam, phi
    variants = {"stride1": selection(1), "stride100": selection(100), "stride100_window": selection(100, **half),
                "near_1pct": selection(1, near=disc)}
    call = Caller(sim)
    names = ["get_atm"] + ["%s/%s" % (v, m) for v in variants for m in ("staged", "direct")]

    def run(name):
        if name == "get_atm":
            sim.get_atm(state)
            return sim.n
        v, mode = name.split("/")
        sim.set_option("select_direct", 1 if mode == "direct" else 0)
        return call(variants[v])

    res = {"workload": "C3", "particles": sim.n, "nq": sim.nq, "steps": args.steps, "rounds": args.rounds,
           "library": sim.L.mphip_version().decode(), "half_by": list(half)[0], "disc_km": disc[2], "call_ms": {}, "selected": {},
           "event_ms": {}, "call_ms_all": {n: [] for n in names}}
    for name in names:                       # warm-up: buffers, first touch
        res["selected"][name] = run(name)
    for _ in range(args.rounds):             # all variants alternating
        for name in names:
            t0 = time.perf_counter()
            run(name)
            res["call_ms_all"][name].append((time.perf_counter() - t0) * 1e3)
    res["call_ms"] = {n: min(v) for n, v in res["call_ms_all"].items()}
    for name in names[1:]:
        res["event_ms"][name] = {}
        for phase, label in PHASES.items():
            sim.set_option("select_profile_phase", phase)
            best = float("inf")
            for _ in range(args.rounds):
                sim.profile_begin()
                run(name)
                launches, ms = sim.profile_end()
                best = min(best, ms)
            res["event_ms"][name][label] = best
            res["event_ms"][name][label + "_pairs"] = launches
    sim.set_option("select_profile_phase", 0)
    sim.set_option("select_direct", 0)
    g = res["call_ms"]["get_atm"]
    res["over_get_atm"] = {n: v / g for n, v in res["call_ms"].items() if n != "get_atm"}
    res["bytes"] = {"get_atm": sim.n * 8 * (4 + sim.nq)}
    for name in names[1:]:
        res["bytes"][name] = res["selected"][name] * (4 + 8 * (4 + sim.nq))
    res["passes_over_np"] = {"get_atm_scatter": 4 + sim.nq, "select": 3}
    sim.close()

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    write()
    if args.bench_parent_lib:
        res["bench_c3"] = bench_ab(args.bench_parent_lib)
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
