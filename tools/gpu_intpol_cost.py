#!/usr/bin/env python3
"""Cost of mphip_intpol_met on the grid of workload C3 (721 x 361 x 137), every figure the best of --rounds after a warm-up:
  device      scattered points (10^6 and 10^7) and the centres of a 360 x 180 x 90 output grid in grid order (level
              fastest), for `t` alone and for `t, h2o, o3, u, v, w, ps, pbl`: the kernel time (the call's own profile
              phase: mphip_profile_begin / _end around the call) and the whole call beside it (copies in and out
              included, into an array that exists), as points per second and against the bytes the call must move:
              32 B in and 8 B per field out per point (`bytes_io`), and with the gathered lines on top (`bytes_with_lines`:
              two snapshots x four columns x one 128-byte line per pressure-level field, two lines of two corners per
              surface field -- what scattered points cannot avoid; points in grid order share most of them);
  host        (--host-tree DIR: a tree whose host layer is compiled with production extents; the parent commit's for the
              comparison) tools/c/intpol_host_loop.c: mptrac_amd_intpol_3d at the same 360 x 180 x 90 centres, one call
              per cell as write_grid makes them, from MET_TYPE 1 files and from MET_TYPE 2 files with HIP_MET_PACKED 1
              (the first pass pays the decode and download of met_need_floats); the device call for `t` at these points
              against it, after a float and after a packed upload;
  bench_c3    (--bench-parent-lib PATH) bench.py with that library and this tree's alternating in one session.
Writes profiles/intpol_cost.json and prints it as one JSON line.
  tools/gpu_intpol_cost.py [--rounds R] [--host-tree DIR] [--bench-parent-lib PATH]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FIELDS_8 = ("t", "h2o", "o3", "u", "v", "w", "ps", "pbl")
GRID = (360, 180, 90)
LINE = 128


def context(hip, m0, m1):
    sim = object.__new__(hip.Simulation)
    sim.L = hip.load()
    sim.h = C.c_void_p()
    assert sim.L.mphip_create(C.byref(sim.h), 0) == 0
    sim._mets, sim._next_met = [None, None], None
    sim.set_met(0, m0)
    sim.set_met(1, m1)
    return sim


def measure(np, sim, pts, fields, rounds):
    t, p, lon, lat = pts
    n = len(lon)
    out = np.zeros((len(fields), n))
    sim.intpol_met_rows(t, p, lon, lat, fields, out=out)       # warm-up: buffers, first touch of `out`
    kernel, call = [], []
    for _ in range(rounds):
        sim.profile_begin()
        t0 = time.perf_counter()
        sim.intpol_met_rows(t, p, lon, lat, fields, out=out)
        call.append((time.perf_counter() - t0) * 1e3)
        launches, ms = sim.profile_end()
        kernel.append(ms)
    n3 = sum(1 for f in fields if f not in ("ps", "pbl"))
    bytes_io = n * (32 + 8 * len(fields))
    bytes_lines = n * LINE * (8 * n3 + 4 * (len(fields) - n3))
    k, c = min(kernel) * 1e-3, min(call) * 1e-3
    return {"points": n, "fields": list(fields), "launches": launches, "kernel_ms": min(kernel), "kernel_ms_all": kernel,
            "call_ms": min(call), "call_ms_all": call, "points_per_s_kernel": n / k, "points_per_s_call": n / c,
            "bytes_io": bytes_io, "bytes_with_lines": bytes_io + bytes_lines, "bytes_io_per_s_kernel": bytes_io / k,
            "bytes_with_lines_per_s_kernel": (bytes_io + bytes_lines) / k, "bytes_io_per_s_call": bytes_io / c,
            "checksum": float(np.nansum(out))}


def host_loop(args, tmp, mets):
    """tools/c/intpol_host_loop.c against the host layer of --host-tree, production extents"""
    import hostfiles as hf
    tree = os.path.abspath(args.host_tree)
    host, lib = os.path.join(tree, "mptrac_amd", "host"), os.path.join(tree, "mptrac_amd", "lib")
    exe = os.path.join(tmp, "intpol_host_loop")
    src = [os.path.join(host, f) for f in ("mptrac.c", "ctlfile.c", "nc_classic.c", "nc_hdf5.c", "rendezvous.c", "output.c")]
    defs = ["-DNP=1000", "-DNQ=15", "-DEX=724", "-DEY=364", "-DEP=140",
            '-DMPTRAC_AMD_DATA_DIR="%s"' % os.path.join(ROOT, "mptrac_amd", "data")]
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-mcmodel=medium", *defs, "-I", host, "-o", exe,
                           os.path.join(ROOT, "tools", "c", "intpol_host_loop.c"), *src, "-L" + lib, "-lmptrac_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-lpthread", "-lz"])
    files = []
    for m in mets:
        files.append(hf.met_filename(os.path.join(tmp, "met"), m.time))
        hf.write_met_bin(files[-1], m)
    hf.write_ctl(os.path.join(tmp, "loop.ctl"), {"NQ": 0, "MET_TYPE": 1})
    r = subprocess.run([exe, os.path.join(tmp, "loop.ctl"), files[0], files[1], tmp, *map(str, GRID)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    text = r.stdout.decode()
    assert r.returncode == 0, text[-3000:]
    row = json.loads([ln for ln in text.splitlines() if ln.startswith("JSON ")][-1][5:])
    row["host_tree"] = args.host_tree_label or tree
    for f in files:
        os.remove(f)
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
    mean = sum(p) / 2
    return {"command": "bench.py --gpus 1 --steps 60 --warmup 3 --no-cpu-baseline", "order": order, "runs": runs,
            "parent_spread": abs(p[0] - p[1]) / mean,
            "new_over_parent_mean": [runs["new"]["ms_per_step"] / mean, runs["new2"]["ms_per_step"] / mean],
            "note": "parent: the library of the commit before this one, loaded through MPHIP_LIB into the same tree; one "
                    "session, one process per run"}


def main():
    import numpy as np
    from mptrac_amd import hip
    from mptrac_amd.synth import pressure_from_z, synthetic_met
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-tree", default=None)
    ap.add_argument("--host-tree-label", default=None)
    ap.add_argument("--bench-parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intpol_cost.json"))
    args = ap.parse_args()

    mets = [synthetic_met("C3", 3600.0 * k, 1.0 + 0.25 * k, fields=FIELDS_8) for k in range(2)]
    sim = context(hip, *mets)
    out = {"grid": [mets[0].nx, mets[0].ny, mets[0].np], "rounds": args.rounds, "library": sim.L.mphip_version().decode(),
           "intpol_chunk": 2 ** 22, "output_grid": list(GRID), "line_bytes": LINE}
    rng = np.random.default_rng(12345)
    sets = {}
    for n in (10 ** 6, 10 ** 7):
        sets["scattered_%.0e" % n] = (np.array([1800.0]), pressure_from_z(rng.uniform(0.0, 30.0, n)), rng.uniform(-180.0, 180.0, n),
                                      rng.uniform(-90.0, 90.0, n))
    nx, ny, nz = GRID
    lon = -180.0 + 360.0 / nx * (np.arange(nx) + 0.5)
    lat = -90.0 + 180.0 / ny * (np.arange(ny) + 0.5)
    z = 30.0 / nz * (np.arange(nz) + 0.5)
    g = np.meshgrid(lon, lat, pressure_from_z(z), indexing="ij")      # [ix][iy][iz], level fastest
    sets["grid_order"] = (np.array([1800.0]), np.ascontiguousarray(g[2].ravel()), np.ascontiguousarray(g[0].ravel()),
                          np.ascontiguousarray(g[1].ravel()))
    out["device"] = {name: {"t": measure(np, sim, pts, ("t",), args.rounds), "eight": measure(np, sim, pts, FIELDS_8, args.rounds)}
                     for name, pts in sets.items()}
    if args.host_tree:
        with tempfile.TemporaryDirectory(prefix="intpol_cost_") as tmp:
            host = host_loop(args, tmp, mets)
        # the device call at the same points: after a float upload (above) and after a packed upload of the same snapshots
        floats = out["device"]["grid_order"]["t"]
        import copy
        for slot, m in enumerate(mets):
            bare = copy.copy(m)
            bare.f3 = {}
            sim.update_met_packed(slot, bare, sim.pack_met(m))
        packed = measure(np, sim, sets["grid_order"], ("t",), args.rounds)
        out["host"] = dict(host, device_call_ms_float_upload=floats["call_ms"], device_call_ms_packed_upload=packed["call_ms"],
                           host_over_device_float_files=min(host["float_files_ms"]) / floats["call_ms"],
                           host_over_device_packed_files=host["packed_files_ms"][0] / packed["call_ms"],
                           note="float files: the better of the host's two passes; packed files: its first pass, which decodes "
                                "and downloads the level fields of both snapshots (met_need_floats) as every run's first "
                                "gridded output does; the device call: copies in and out included")
    sim.close()

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    write()
    if args.bench_parent_lib:
        out["bench_c3"] = bench_ab(args.bench_parent_lib)
        write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
