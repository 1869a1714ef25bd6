"""bench.py end to end at a small particle count (GPU): the one JSON line the driver parses carries every field of
the contract, the step counts it was asked for, a roofline measured live and a CPU baseline."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--device-warmup-ms", "0"], ["--workload", "C5"]], ids=["default", "no_device_warmup", "C5"])
def test_bench_prints_the_contract_line(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--particles", "2e5",
           "--cpu-sample", "20000", "--cpu-steps", "2", "--device-warmup-ms", "30", *extra]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "particle-steps/s" and d["unit"] == "particle-steps/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"] == "synthetic"
    assert abs(d["value"] - 2e5 * 4 / (d["ms_per_step"] * 4e-3)) <= 1e-6 * d["value"] and d["value"] > 1e7   # (a floor only: the suite may share the GPU between workers)
    cfg = d["config"]
    assert isinstance(cfg["workload"], str) and cfg["particles_per_gpu"] == 200000 and "model" not in cfg
    assert ("none" in cfg["device_warmup"]) == ("--device-warmup-ms" in extra and extra[extra.index("--device-warmup-ms") + 1] == "0")
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    # (2e5 particles touch ~100 MB of meteo records: inside the Infinity Cache, no share of the HBM roof is claimed)
    assert r["kernel_ms"] > 0 and r["frac"] is None and "Infinity Cache" in r["frac_note"] and r["frac_one_launch_per_step"] is None
    assert abs(r["achieved"] - r["algorithmic_bytes_per_step"] / (r["kernel_ms"] * 1e-3) / 1e9) <= 1e-9 * r["achieved"]
    assert r["kernel_ms"] <= d["ms_per_step"] * 1.02 and "traffic" in r
    # one rank: no communicator; the per-rank kernel times the driver reads are there
    assert cfg["rccl_ranks"] == 0 and len(r["kernel_ms_per_rank"]) == 1
    if "C5" in extra:   # a step of several unlike kernels is priced as a whole (wall time per step)
        assert r["step_kernel_launches_per_step"] == 2 and abs(r["kernel_ms"] - d["ms_per_step"]) <= 1e-9 * r["kernel_ms"]
        assert r["step_kernel_ms_per_step"] < r["kernel_ms"]
    else:
        # (2e5 particles: the K steps go to the library as one call and share launches)
        assert r["step_kernel_launches_per_step"] <= 1 and r["kernel_ms"] == r["step_kernel_ms_per_step"]
        assert "mphip_run_timesteps" in cfg["time_loop"]
    # both bounds stated: the HBM pricing under both launch regimes, the modelled VALU-issue roof (None at
    # an overridden particle count: the committed instruction mix belongs to the workload's own), what pins the oracle
    assert "alu" in r and "algorithmic" in r["basis"]
    assert any("RK4" in m for m in d["parity"]["restatement_only"]) and d["parity"]["pinned_by_reference_goldens"]
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "particle-steps/s" and c["cores"] >= 1 and c["value"] > 1e4
    assert "sample" in c and c["value_1_thread"] > 0


def test_dump_outputs_writes_float64_within_the_limit_and_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs (CPU part): every array of the step as float64 .npy, the whole set within the size limit, the
    particles whole while they fit and otherwise the same seeded sample on every call."""
    import numpy as np
    import bench
    rng = np.random.default_rng(7)
    n, ncell, nq = 5000, 300, len(bench.WORKLOADS["C3"][3])
    atm = {k: rng.random(n) for k in ("time", "lon", "lat", "p")}
    atm["q"] = rng.random((nq, n))
    grid = (rng.integers(0, 50, ncell).astype(np.int32), rng.random((nq, ncell)), rng.random((nq, ncell)))

    whole = bench.dump_outputs(str(tmp_path / "whole"), "C3", atm, grid)
    assert not whole["particles_sampled"] and whole["particles"] == n
    assert np.array_equal(np.load(tmp_path / "whole" / "lon.npy"), atm["lon"])
    assert np.array_equal(np.load(tmp_path / "whole" / "grid_count.npy"), grid[0].astype(np.float64))

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200000)
    a = bench.dump_outputs(str(tmp_path / "a"), "C3", atm, grid)
    b = bench.dump_outputs(str(tmp_path / "b"), "C3", atm, grid)
    assert a["particles_sampled"] and 0 < a["particles"] < n and a["bytes"] <= 200000
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == a["files"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) == a["bytes"]
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and np.array_equal(x, y), f
    idx = np.load(tmp_path / "a" / "particle_index.npy").astype(np.int64)
    assert np.all(np.diff(idx) > 0) and np.array_equal(np.load(tmp_path / "a" / "p.npy"), atm["p"][idx])
    for iq, name in enumerate(bench.WORKLOADS["C3"][3]):
        assert np.array_equal(np.load(tmp_path / "a" / f"q_{name}.npy"), atm["q"][iq][idx])
        assert np.array_equal(np.load(tmp_path / "a" / f"grid_sum_{name}.npy"), grid[1][iq])
        assert np.array_equal(np.load(tmp_path / "a" / f"grid_sumsq_{name}.npy"), grid[2][iq])


def test_dump_outputs_of_a_workload_with_many_quantities_stay_within_the_limit(tmp_path):
    """C3m carries eleven quantities: 39 files, whose .npy headers count against the 64 MB as much as their data, at
    the output grid of the bench (360 x 180) and more particles than fit."""
    import numpy as np
    import bench
    quantities = bench.WORKLOADS["C3m"][3]
    n, ncell, nq = 700000, 360 * 180, len(quantities)
    rng = np.random.default_rng(11)
    atm = {k: rng.random(n) for k in ("time", "lon", "lat", "p")}
    atm["q"] = rng.random((nq, n))
    grid = (rng.integers(0, 50, ncell).astype(np.int32), rng.random((nq, ncell)), rng.random((nq, ncell)))
    d = bench.dump_outputs(str(tmp_path), "C3m", atm, grid)
    names = os.listdir(tmp_path)
    assert len(names) == d["files"] == 1 + 2 * nq + 1 + 4 + nq
    total = sum(os.path.getsize(tmp_path / f) for f in names)
    assert total == d["bytes"] and total <= bench.DUMP_LIMIT_BYTES
    assert d["particles_sampled"] and d["particles"] < n
    # as many particles as the limit allows: one more in each of the 5 + nq particle files would not fit
    m = d["particles"]
    assert total - (5 + nq) * bench.npy_bytes(m) + (5 + nq) * bench.npy_bytes(m + 1) > bench.DUMP_LIMIT_BYTES


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_timed_step_and_repeat(tmp_path):
    """--dump-outputs end to end: two runs with the same arguments write the same files bit for bit, the particles
    carry the time of the last timed step (warm-up W + K timed steps after t = 0; the ten single-launch steps behind
    the timed region come later), and a run too large for the limit is sampled."""
    import numpy as np
    steps, warmup = 3, 2
    lines = {}
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
               "--particles", "1.2e6", "--no-cpu-baseline", "--device-warmup-ms", "30", "--no-multi-gpu-probe",
               "--dump-outputs", str(tmp_path / run)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
        out = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, res.stdout[-2000:]
        lines[run] = json.loads(out[0])
    d = lines["a"]
    assert d["steps"] == steps and d["ms_per_step"] > 0
    dump = d["dump_outputs"]
    assert dump["particles_sampled"] and dump["bytes"] <= 64 * 10 ** 6
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == dump["files"]
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and np.array_equal(x, y, equal_nan=True), f
    assert np.all(np.load(tmp_path / "a" / "time.npy") == (warmup + steps) * d["config"]["dt_mod"])
    assert np.load(tmp_path / "a" / "grid_count.npy").sum() >= 0.999 * 1.2e6
