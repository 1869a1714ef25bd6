#!/usr/bin/env python3
"""Cost of the 16-bit packed meteo fields on the grid of workload C3 (721 x 361 x 137, the nine level fields a run
uploads), every figure the best of --rounds after a warm-up, both upload paths alternating in one process:
  upload      wall time of mphip_update_met_packed (codes, decoded on the device) against mphip_update_met (the decoded
              floats) for the same snapshot;
  kernels     device events around met_unpack_kernel (mphip_unpack_met, derive_profile_phase 0) and around the three
              launches of mphip_pack_met (phases 4, 5, 6: extremes, their reduction, quantisation), summed over the nine
              fields; the bytes each algorithm must move (6 B per value decoded or quantised, 4 B per value for the
              extremes) over that time as a rate and as a share of the HBM peak of the micro-architecture guide (8.0 TB/s
              specified; 6.29 TB/s is what a float4 copy reaches there);
  prefetch    the stepping rate of workload C3 with a new snapshot every 20 steps handed over by mphip_prefetch_met_packed /
              mphip_commit_met against mphip_prefetch_met / mphip_commit_met (the procedure of tools/gpu_met_overlap.py).
Writes profiles/met_pack_cost.json and prints it as one JSON line.
  tools/gpu_met_pack_cost.py [--rounds R] [--no-prefetch]"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_PEAK_SPEC = 8.0e12          # B/s, HBM3E peak of the MI355X as specified
HBM_COPY_MEASURED = 6.29e12     # B/s, a float4 copy
INTERVALS, PER = 4, 20


def best(ms):
    return {"ms": min(ms), "ms_all": ms}


def prefetch_rate(packed):
    """Particle-steps per second with a hand-over every PER steps, the upload beside the time steps."""
    import bench
    from mptrac_amd import hip
    from mptrac_amd.synth import synthetic_met
    ctl, clim, m0, m1, atm, n_local, n_total = bench.build_inputs("C3", 0, 1, PER - 1)
    fields = tuple(m0.f3) + tuple(m0.f2)
    ctl.update(t_stop=3600.0 * (INTERVALS + 2))
    spare = [synthetic_met("C3", 3600.0 * (k + 2), 1.0 + 0.1 * k, fields=fields) for k in range(3)]
    s = hip.Simulation(ctl, clim, m0, m1, atm, n_total=n_total, shard=(0, n_local))
    codes = [None] * 3
    if packed:      # the codes of the three buffers, and the buffers without their level fields
        for w in range(3):
            codes[w] = s.pack_met(spare[w])
            spare[w].f3 = {}

    def prefetch(w, t):
        spare[w].time = t
        if packed:
            s.prefetch_met_packed(spare[w], codes[w])
        else:
            s.prefetch_met(spare[w])

    s.timesteps_init(0.0, 0.0)
    dt = s.ctl.dt_mod
    k = 0
    for _ in range(PER):
        s.run_timestep(k * dt)
        k += 1
    for w in range(3):          # untimed: every buffer once (first touch of the host arrays, the code buffer)
        prefetch(w, 3600.0 * (w + 2))
        s.commit_met()
    s.run_timestep(k * dt)
    prefetch(0, 3600.0 * 2)
    while not s.prefetch_done():
        time.sleep(0.001)
    s.synchronize()
    host_ms = []
    t0 = time.perf_counter()
    for it in range(INTERVALS):
        s.commit_met()
        for j in range(PER):
            if j == 4:
                h0 = time.perf_counter()
                prefetch((it + 1) % 3, 3600.0 * (it + 3))
                host_ms.append((time.perf_counter() - h0) * 1e3)
            s.run_timestep(k * dt)
            k += 1
    s.synchronize()
    wall = time.perf_counter() - t0
    s.close()
    return {"particle_steps_per_s": n_local * INTERVALS * PER / wall, "ms_per_step": wall / (INTERVALS * PER) * 1e3,
            "host_ms_of_the_prefetch_call": sum(host_ms) / len(host_ms)}


def main():
    import numpy as np
    import cases
    from mptrac_amd import hip
    from mptrac_amd.synth import synthetic_met
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-prefetch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "met_pack_cost.json"))
    args = ap.parse_args()

    ctl, clim, _, _, atm = cases.make_case("advect", n=1000, grid="tiny")
    met = synthetic_met("C3", 3600.0, 1.0, fields=cases.PRESSURE_LEVEL_FIELDS)
    names = tuple(met.f3)
    sim = hip.Simulation(ctl, clim, met, met, atm)
    values = met.nx * met.ny * met.np * len(names)
    out = {"grid": [met.nx, met.ny, met.np], "level_fields": list(names), "values": values, "rounds": args.rounds,
           "library": sim.L.mphip_version().decode(), "hbm_peak_spec_bytes_per_s": HBM_PEAK_SPEC,
           "hbm_float4_copy_bytes_per_s": HBM_COPY_MEASURED}
    packed = sim.pack_met(met)                                  # (warm-up of the encoder; the codes of what follows)
    bare, dec = copy.copy(met), copy.copy(met)
    bare.f3 = {}
    dec.f3 = sim.unpack_met(bare, packed)                       # (warm-up of the decoder; the floats the codes stand for)
    # the whole upload call, alternating
    sim.set_met(1, dec)
    sim.update_met_packed(1, bare, packed)
    floats, codes = [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        sim.set_met(1, dec)
        floats.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        sim.update_met_packed(1, bare, packed)
        codes.append((time.perf_counter() - t0) * 1e3)
    out["upload"] = {"update_met": best(floats), "update_met_packed": best(codes), "ratio": min(codes) / min(floats),
                     "bytes_floats": 4 * values, "bytes_codes": 2 * values}
    # the kernels
    res = {f: np.empty_like(dec.f3[f]) for f in names}
    target = {f: packed[f] for f in names}
    kernels = {}
    for label, phase, bytes_per_value, call in (("unpack", 0, 6, lambda: sim.unpack_met(bare, packed, out=res)),
                                                ("pack_extremes", 4, 4, lambda: sim.pack_met(met, out=target)),
                                                ("pack_reduce", 5, 0, lambda: sim.pack_met(met, out=target)),
                                                ("pack_quantise", 6, 6, lambda: sim.pack_met(met, out=target))):
        sim.set_option("derive_profile_phase", phase)
        ms = []
        for _ in range(args.rounds):
            sim.profile_begin()
            call()
            pairs, t_ms = sim.profile_end()
            assert pairs == len(names), (label, pairs)
            ms.append(t_ms)
        row = best(ms)
        row["launches"] = len(names)
        if bytes_per_value:
            rate = bytes_per_value * values / (min(ms) * 1e-3)
            row.update(bytes=bytes_per_value * values, bytes_per_s=rate, share_of_hbm_peak_spec=rate / HBM_PEAK_SPEC,
                       share_of_hbm_float4_copy=rate / HBM_COPY_MEASURED)
        kernels[label] = row
    sim.set_option("derive_profile_phase", 0)
    out["kernels"] = kernels
    sim.close()
    if not args.no_prefetch:
        a, b = prefetch_rate(False), prefetch_rate(True)
        out["prefetch"] = {"floats": a, "codes": b, "ratio": b["particle_steps_per_s"] / a["particle_steps_per_s"],
                           "steps_per_snapshot": PER, "hand_overs": INTERVALS}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
