#!/usr/bin/env python3
"""Same-box A/B timing of builds of libalink_hip.so (KMeans v10 variants): every build runs the fused kernel on
the same synthetic 1e8 x 128 bf16 table (tools/kmeans_kernel_bench.py in a child process with ALINK_HIP_LIB),
in ``--rounds`` alternating rounds, so clock drift and box-to-box spread hit all builds alike.

    python tools/kmeans_ab.py --libs base=alink_amd/ops/libalink_hip.so,pk=variants/libalink_hip_pk.so \
        [--rounds 3] [--rows 100000000] [--k 100] [--modes 0] [--iters 15] [--b2b 20] [--configs v10:1,v10:0]

Prints one JSON line per (round, build, mode) and a summary line with the median ms per build and mode.  With
``--b2b N`` every child also times N back-to-back launches with alternating direction, as bench.py issues them
(``b2b_ms`` per line, ``|b2b`` keys in the summary).

``--configs`` goes to kmeans_kernel_bench.py as it is.  Its default, ``v10:0``, is the production launch
(non-temporal X loads).  Profiles older than profiles/kmeans_v10_sweep.txt were taken with ``v10:1`` (default-policy
loads), which this tool then passed unconditionally: pass ``--configs v10:1`` to compare with them.  With several
configs the summary keys carry ``:kernel:flags=F`` behind the build's name.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--modes", default="0")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--sub-rows", default="")
    ap.add_argument("--b2b", type=int, default=0)
    ap.add_argument("--configs", default="v10:0",
                    help="kmeans_kernel_bench.py configs: v10:0 = the production launch, v10:1 = default-policy loads")
    a = ap.parse_args()
    libs = [kv.split("=", 1) for kv in a.libs.split(",")]
    res = {}
    for r in range(a.rounds):
        for name, path in libs:
            env = dict(os.environ)
            env["ALINK_HIP_LIB"] = os.path.join(ROOT, path) if not os.path.isabs(path) else path
            cmd = [sys.executable, os.path.join(ROOT, "tools", "kmeans_kernel_bench.py"), "--rows", str(a.rows),
                   "--k", str(a.k), "--configs", a.configs, "--modes", a.modes, "--iters", str(a.iters)]
            if a.sub_rows:
                cmd += ["--sub-rows", a.sub_rows]
            if a.b2b > 0:
                cmd += ["--b2b", str(a.b2b)]
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                print(json.dumps({"build": name, "round": r, "error": out.stderr[-2000:]}), flush=True)
                return 1
            for line in out.stdout.splitlines():
                if line.startswith("{"):
                    d = json.loads(line)
                    d.update({"build": name, "round": r})
                    print(json.dumps(d), flush=True)
                    if "," in a.configs:
                        name_c = f"{name}:{d['kernel']}:flags={d['flags']}"
                    else:
                        name_c = name
                    res.setdefault((name_c, d["rows"], d["mode"]), []).append(d["ms"])
                    if "b2b_ms" in d:
                        res.setdefault((name_c, d["rows"], f"{d['mode']}|b2b"), []).append(d["b2b_ms"])
    summ = {f"{key[0]}|rows={key[1]}|mode={key[2]}": sorted(v)[len(v) // 2] for key, v in res.items()}
    print(json.dumps({"summary_median_ms": summ}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
