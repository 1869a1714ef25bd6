#!/usr/bin/env python3
"""Cost of mphip_ingest_met on the grid of workload C3 (720 longitudes in the file, 721 with the periodic column the call
adds, x 361 x 137; eleven level and thirteen surface fields), stored as floats and as packed shorts, every figure the best
of --rounds after a warm-up:
  kernels     device events (mphip_profile_begin / _end, derive_profile_phase 0) around the launches of one stage: the
              decode + axis reversal of the level fields and of the surface fields (a DECODE call with only those), the
              extrapolation, the two polar launches and the periodic copy (a met-order call with that bit alone); the
              bytes the algorithm moves over that time as a rate, and its share of what a float4 copy reaches (6.29 TB/s,
              the micro-architecture guide) and of the specified HBM peak (8.0 TB/s);
  call        wall time of the whole call with all four stages, and the device time of its uploads and downloads
              (phases 1 and 2);
  read_met    (unless --no-host) tools/c/ingest_read_loop.c, the host layer compiled with production extents: mptrac_read_met
              of one page-cached netCDF file (the packed shorts) with HIP_MET_INGEST 0 and 1 alternating in one process;
  bench_c3    (--bench-parent-lib PATH) bench.py with that library and this tree's alternating twice in one session.
Writes profiles/met_ingest_cost.json and prints it as one JSON line.
  tools/gpu_met_ingest_cost.py [--rounds R] [--no-host] [--bench-parent-lib PATH [--only-bench]]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_PEAK_SPEC = 8.0e12          # B/s, HBM3E peak of the MI355X as specified
HBM_COPY_MEASURED = 6.29e12     # B/s, a float4 copy
NX, NY, NP = 720, 361, 137
LEVEL = ("t", "u", "v", "w", "h2o", "o3", "lwc", "rwc", "iwc", "swc", "cc")
SURFACE = ("ps", "zs", "ts", "us", "vs", "ess", "nss", "shf", "lsm", "sst", "pbl", "cape", "cin")
NC_NAME = {"t": "t", "u": "u", "v": "v", "w": "w", "h2o": "q", "o3": "o3", "lwc": "clwc", "rwc": "crwc", "iwc": "ciwc",
           "swc": "cswc", "cc": "cc", "ps": "sp", "zs": "z", "ts": "t2m", "us": "u10m", "vs": "v10m", "ess": "iews", "nss": "inss",
           "shf": "ishf", "lsm": "lsm", "sst": "sstk", "pbl": "blp", "cape": "cape", "cin": "cin"}
FILL = -32767


def best(ms):
    return {"ms": min(ms), "ms_all": ms}


def rated(row, nbytes):
    rate = nbytes / (row["ms"] * 1e-3)
    row.update(bytes=nbytes, bytes_per_s=rate, share_of_hbm_float4_copy=rate / HBM_COPY_MEASURED,
               share_of_hbm_peak_spec=rate / HBM_PEAK_SPEC)
    return row


def raw_fields(np, short):
    """{name: (array, options)}: a smooth field plus noise per slot, the fill value below a wavy ground on the lowest levels"""
    rng = np.random.default_rng(2024)
    base3 = rng.integers(-30000, 30000, size=(NP, NY, NX), dtype=np.int16)
    base2 = rng.integers(-30000, 30000, size=(NY, NX), dtype=np.int16)
    ground = (3 + 2 * np.sin(np.arange(NX) * 0.05)[None, :] * np.cos(np.arange(NY) * 0.03)[:, None]).astype(int)      # levels
    below = np.arange(NP)[:, None, None] < ground[None]
    raw = {}
    for n, name in enumerate(LEVEL + SURFACE):
        a = np.roll(base3 if name in LEVEL else base2, 17 * n, axis=-1)
        opt = dict(scl=1.0, fill=FILL)
        if short:
            a = a.copy()
            opt.update(scale_factor=float(np.float32(1e-3)), add_offset=float(np.float32(n)))
        else:
            a = a.astype(np.float32) * np.float32(1e-3) + np.float32(n)
            opt["fill"] = float(np.float32(-9.99e8))
        if name in LEVEL:
            a[below] = opt["fill"]
        raw[name] = (a, opt)
    return raw


def write_nc(np, path, raw, lon, lat, p):
    from scipy.io import netcdf_file
    with netcdf_file(path, "w", version=2) as f:
        for name, axis in (("lon", lon), ("lat", lat), ("lev", 100.0 * p)):
            f.createDimension(name, len(axis))
            f.createVariable(name, "d", (name,))[:] = axis
        for name, (a, opt) in raw.items():
            v = f.createVariable(NC_NAME[name], "h", ("lev", "lat", "lon") if a.ndim == 3 else ("lat", "lon"))
            v[:] = a
            v._FillValue = np.int16(opt["fill"])
            v.scale_factor, v.add_offset = np.float64(opt["scale_factor"]), np.float64(opt["add_offset"])


def read_met_loop(np, rounds, raw, lon, lat, p):
    """tools/c/ingest_read_loop.c against this tree's host layer, production extents"""
    import hostfiles as hf
    from mptrac_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ingest_read_loop")
        src = [os.path.join(build.HOST_DIR, f) for f in ("mptrac.c", "ctlfile.c", "nc_classic.c", "nc_hdf5.c", "rendezvous.c",
                                                          "output.c")]
        defs = ["-DNP=1000", "-DNQ=15", "-DEX=724", "-DEY=364", "-DEP=140",
                '-DMPTRAC_AMD_DATA_DIR="%s"' % os.path.join(ROOT, "mptrac_amd", "data")]
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-mcmodel=medium", *defs, "-I", build.HOST_DIR, "-o", exe,
                               os.path.join(ROOT, "tools", "c", "ingest_read_loop.c"), *src, "-L" + build.LIBDIR, "-lmptrac_hip",
                               "-Wl,-rpath," + build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-lpthread", "-lz"])
        path = os.path.join(tmp, "met_2022_06_02_00.nc")
        write_nc(np, path, raw, lon, lat, p)
        size = os.path.getsize(path)
        hf.write_ctl(os.path.join(tmp, "loop.ctl"), {"NQ": 0, "MET_TYPE": 0, "MET_PBL": 0, "MET_CAPE": 0})
        r = subprocess.run([exe, os.path.join(tmp, "loop.ctl"), path, str(rounds)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=1500)
        text = r.stdout.decode()
        assert r.returncode == 0, text[-3000:]
    row = json.loads([ln for ln in text.splitlines() if ln.startswith("JSON ")][-1][5:])
    assert row["differ"] == 0 and row["checksum"][0] == row["checksum"][1], row
    a, b = row.pop("ms_ingest_0"), row.pop("ms_ingest_1")
    row.update(file_bytes=size, storage="packed shorts", hip_met_ingest_0=best(a), hip_met_ingest_1=best(b),
               ratio=min(b) / min(a), note="mptrac_read_met of one page-cached file, HIP_MET_PREP 0, the two settings "
               "alternating in one process; t, u, v, w, h2o of the two snapshots compared word for word")
    return row


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
    n = [runs["new"]["ms_per_step"], runs["new2"]["ms_per_step"]]
    mean = sum(p) / 2
    return {"command": "bench.py --gpus 1 --steps 60 --warmup 3 --no-cpu-baseline", "order": order, "runs": runs,
            "parent_spread": abs(p[0] - p[1]) / mean, "new_spread": abs(n[0] - n[1]) / (sum(n) / 2),
            "new_over_parent_mean": [x / mean for x in n],
            "note": "parent: the library of the commit before this one, loaded through MPHIP_LIB into the same tree; one "
                    "session, one process per run"}


def main():
    import numpy as np
    from mptrac_amd import hip
    from mptrac_amd.hip import Snapshot
    from test_gpu_regrid import bare_context
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--only-bench", action="store_true", help="add bench_c3 to the file --out that an earlier run wrote")
    ap.add_argument("--bench-parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "met_ingest_cost.json"))
    args = ap.parse_args()
    if args.only_bench:
        out = json.load(open(args.out))
        out["bench_c3"] = bench_ab(args.bench_parent_lib)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out["bench_c3"]))
        return

    lon, lat = -180.0 + 0.5 * np.arange(NX), 90.0 - 0.5 * np.arange(NY)
    p = 1013.25 * np.exp(-np.arange(NP) * (60.0 / (NP - 1)) / 7.0)
    axes = Snapshot(0.0, 0, lon, lat, p, {}, {})
    sim = bare_context()
    n3, n2 = NX * NY * NP * len(LEVEL), NX * NY * len(SURFACE)
    out = {"grid_in_the_file": [NX, NY, NP], "grid": [NX + 1, NY, NP], "level_fields": list(LEVEL), "surface_fields": list(SURFACE),
           "values": n3 + n2, "rounds": args.rounds, "library": sim.L.mphip_version().decode(),
           "hbm_peak_spec_bytes_per_s": HBM_PEAK_SPEC, "hbm_float4_copy_bytes_per_s": HBM_COPY_MEASURED}

    def timed(call, phase, launches):
        sim.set_option("derive_profile_phase", phase)
        ms = []
        for _ in range(args.rounds):
            sim.profile_begin()
            call()
            pairs, t_ms = sim.profile_end()
            assert launches is None or pairs == launches, (pairs, launches)
            ms.append(t_ms)
        sim.set_option("derive_profile_phase", 0)
        return best(ms)

    shorts = None
    for short in (False, True):
        label = "short" if short else "float"
        raw = raw_fields(np, short)
        if short:
            shorts = raw
        raw3, raw2 = {k: raw[k] for k in LEVEL}, {k: raw[k] for k in SURFACE}
        size = 2 if short else 4
        res = sim.ingest_met(raw, axes, 15)                   # (warm-up: the scratch pool, first touch of the outputs)
        assert res.nx == NX + 1
        outs = dict(res.f3, **res.f2)
        print(label, "warm-up done", flush=True)
        wall = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            sim.ingest_met(raw, axes, 15, out=outs)
            wall.append((time.perf_counter() - t0) * 1e3)
        row = {"call_all_stages_wall": best(wall),
               "uploads": rated(timed(lambda: sim.ingest_met(raw, axes, 15, out=outs), 1, None), size * (n3 + n2)),
               "downloads": rated(timed(lambda: sim.ingest_met(raw, axes, 15, out=outs), 2, None),
                                  4 * (n3 + n2) // NX * (NX + 1))}
        print(label, "whole call", json.dumps(row["call_all_stages_wall"]), flush=True)
        o3 = {k: v[:NX] for k, v in res.f3.items()}
        o2 = {k: v[:NX] for k, v in res.f2.items()}
        row["decode_level_fields"] = rated(timed(lambda: sim.ingest_met(raw3, axes, 1, out=o3), 0, len(LEVEL)), (size + 4) * n3)
        row["decode_surface_fields"] = rated(timed(lambda: sim.ingest_met(raw2, axes, 1, out=o2), 0, len(SURFACE)), (size + 4) * n2)
        print(label, "decode", json.dumps(row["decode_level_fields"]), flush=True)
        if not short:       # the stages behind the decode do not see how the values were stored
            met = Snapshot(0.0, 0, lon, lat, p, o3, o2)
            sim.ingest_met(raw, axes, 1, out=dict(o3, **o2))
            ncell = NX * NY * NP
            stages = {"extrapolate": rated(timed(lambda: sim.ingest_met(met, 2, out=dict(o3, **o2)), 0, 1), 4 * 4 * ncell),
                      "polar": rated(timed(lambda: sim.ingest_met(met, 4, out=dict(o3, **o2)), 0, 2), 2 * 2 * 2 * 4 * NX * NP),
                      "periodic": rated(timed(lambda: sim.ingest_met(met, 8, out=outs), 0, 1),
                                        2 * 4 * (NY * NP * len(LEVEL) + NY * len(SURFACE)))}
            stages["extrapolate"]["bytes_note"] = "t, u, v, w read once; the fills (3 to 5 of 137 levels per column) not counted"
            stages["polar"]["bytes_note"] = "u, v of two neighbour rows read, of two pole rows written; one lane per level"
            out["stages_behind_the_decode"] = stages
            print("stages", json.dumps({k: v["ms"] for k, v in stages.items()}), flush=True)
        out[label] = row
    sim.close()
    if not args.no_host:
        out["read_met"] = read_met_loop(np, args.rounds, shorts, lon, lat, p)
        print("read_met", json.dumps(out["read_met"]), flush=True)
    if args.bench_parent_lib:
        out["bench_c3"] = bench_ab(args.bench_parent_lib)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
