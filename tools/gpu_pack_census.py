#!/usr/bin/env python3
"""Census of the 16-bit packed level fields in both libraries (GPU box): every case of tests/pack_cases.py through
mphip_unpack_met (compact, strided, from an unaligned code array) and mphip_pack_met (compact, into an unaligned code
array) -- tests/test_gpu_pack.py's census -- in a child per library; per library the results that differ from
tests/refpack.py in any bit and the SHA-256 of every byte returned.  Writes profiles/met_pack_census.json.
  tools/gpu_pack_census.py [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
sys.path[:0] = [ROOT, ROOT + "/tests"]
from mptrac_amd import hip
import test_gpu_pack as T
sim = T.bare_context()
wrong, digest = T.census(sim)
sim.close()
n_unpack = sum(3 * len(T.decode_cases(tag)) for tag in T.TAGS)
n_pack = 2 * len(T.K.ENCODE)
print("JSON " + json.dumps({"library": hip.load().mphip_version().decode(), "unpack_results": n_unpack,
                            "pack_results": n_pack, "differ_from_the_restatement": wrong, "sha256": digest}))
""".replace("ROOT", repr(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "met_pack_census.json"))
    args = ap.parse_args()
    rows = []
    for exact in ("0", "1"):
        env = dict(os.environ, MPTRAC_AMD_EXACT=exact)
        env.pop("MPHIP_LIB", None)
        res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        if res.returncode != 0:
            sys.exit(res.stdout[-2000:] + res.stderr[-3000:])
        rows.append([json.loads(ln[5:]) for ln in res.stdout.splitlines() if ln.startswith("JSON ")][0])
    out = {"libraries": rows, "identical_bytes": rows[0]["sha256"] == rows[1]["sha256"]}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
