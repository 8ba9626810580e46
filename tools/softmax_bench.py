#!/usr/bin/env python3
"""Softmax regression on one GPU: the fused gradient and line-search passes (``ops/softmax_fused.py``,
``csrc/softmax_fused.hip``) against the chain they replace (``profiles/softmax_fused.txt``).

    python tools/softmax_bench.py                            # the four shapes and the sweep
    python tools/softmax_bench.py --shapes 1000000x33:10 --reps 5 --sweep ""

Per shape ``n x m : K`` (fp64 rows on the device, K classes, k1 = K - 1 coefficient rows) it times, after a warm-up of
both paths at that shape, the two paths alternated in the same process with device events:

* the gradient: ``fused_grad`` (m <= 128) or ``rows`` for R plus ``tn_matmul`` (wider m) against the former
  ``grad_sum`` (the logits GEMM, the K16 epilogue, ``tn_matmul``);
* the line search of 11 steps: ``search_losses`` against the former ``calc_search_values`` (two GEMMs, the K16 search
  epilogue).

Printed per shape: medians, minima and spread ((max - min) / median), the bytes each path moves at the least against
one load of X, that load's time at the 6.12 TB/s load-only rate README records, and the largest relative difference
of the two paths' results.

``--sweep``: gradient and search at 33 x 10 and 129 x 32 over small n, host clock around a synchronised call: the
largest n at which the former path still wins sets ``SOFTMAX_MIN_ROWS``.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "10000000x33:10,20000000x9:5,2000000x129:32,1000000x513:10"
SWEEP = "64,1000,10000,30000,100000,300000"
NSTEPS = 11
LOAD_BPS = 25.6e9 / 4.18e-3         # README: the bf16 KMeans kernel's load-only pass over 1e8 x 128 bf16


def timed(fn):
    """Milliseconds of one call of ``fn`` (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    """Milliseconds of one call of ``fn`` on the host clock, device idle before and after."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "spread": (max(t) - min(t)) / statistics.median(t),
            "samples": len(t)}


def alternate(new, old, reps, clock):
    t_new, t_old = [], []
    for _ in range(reps):
        t_new.append(clock(new))
        t_old.append(clock(old))
    return t_new, t_old


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def passes(n, m, k1, dev, seed):
    """The four closures (gradient and search, new and former path) on drawn data, and the dict their results go to."""
    from alink_amd.ops import softmax as S, softmax_fused as F
    from alink_amd.ops.gemm import tn_matmul
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn((n, m), dtype=torch.float64, device=dev, generator=g)
    W = torch.randn((k1, m), dtype=torch.float64, device=dev, generator=g) * (3.0 / m ** 0.5)
    D = torch.randn((k1, m), dtype=torch.float64, device=dev, generator=g) / m ** 0.5
    y = torch.randint(0, k1 + 1, (n,), device=dev, generator=g).double()
    w = torch.rand(n, dtype=torch.float64, device=dev, generator=g) + 0.5
    assert F.supported(X, k1)
    out = {}

    def grad_new():
        if m <= F.SOFTMAX_FUSED_GRAD_MAX_M:
            out["g1"] = F.fused_grad(X, y, w, W)[0]
        else:
            out["g1"] = tn_matmul(X, F.rows(X, y, w, W, ("R",))["R"]).T

    def grad_old():         # the body of the former SoftmaxObjFunc.grad_sum
        out["g0"] = tn_matmul(X, S.softmax_grad(X @ W.T, y, w)[0]).T

    def search_new():
        out["s1"] = F.search_losses(X, y, w, W, D, 0.37, NSTEPS)

    def search_old():       # the body of the former SoftmaxObjFunc.calc_search_values
        out["s0"] = S.softmax_search(X @ W.T, X @ D.T, y, w, 0.37, NSTEPS)
    return grad_new, grad_old, search_new, search_old, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x m : K")
    ap.add_argument("--sweep", default=SWEEP, help="comma-separated n of the small-n sweep, or empty")
    ap.add_argument("--sweep-shapes", default="33:10,129:32", help="comma-separated m : K of the sweep")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd.ops import _lib, softmax_fused as F
    _lib.require()
    dev = torch.device("cuda:0")
    for shape in [s for s in a.shapes.split(",") if s]:
        size, K = shape.split(":")
        n, m = (int(v) for v in size.split("x"))
        k1 = int(K) - 1
        gn, go, sn, so, out = passes(n, m, k1, dev, a.seed)
        for fn in (gn, go, sn, so):
            fn()
        tg1, tg0 = alternate(gn, go, a.reps, timed)
        ts1, ts0 = alternate(sn, so, a.reps, timed)
        xb, blk = 8 * n * m, 8 * n * k1
        fused = m <= F.SOFTMAX_FUSED_GRAD_MAX_M
        print(json.dumps({
            "n": n, "m": m, "K": k1 + 1, "grad_new": stats(tg1), "grad_old": stats(tg0),
            "grad_speedup_median": statistics.median(tg0) / statistics.median(tg1),
            "search_new": stats(ts1), "search_old": stats(ts0),
            "search_speedup_median": statistics.median(ts0) / statistics.median(ts1),
            "x_bytes": xb, "x_load_ms": xb / LOAD_BPS * 1e3,
            # X reads plus the [n, k1] blocks written and read back (eta w+r, R w+r / ec, ed w+r), y and w aside
            "grad_bytes_new": xb if fused else 2 * xb + 2 * blk, "grad_bytes_old": 2 * xb + 4 * blk,
            "search_bytes_new": xb, "search_bytes_old": 2 * xb + 4 * blk,
            "grad_over_x_load": statistics.median(tg1) / (xb / LOAD_BPS * 1e3),
            "search_over_x_load": statistics.median(ts1) / (xb / LOAD_BPS * 1e3),
            "chunk_rows": F.softmax_chunk_rows(n, k1, m) if fused else None,
            "max_rel_diff": {"G": rel(out["g1"], out["g0"]), "search": rel(out["s1"], out["s0"])},
            "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}), flush=True)
        del gn, go, sn, so, out
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    if a.sweep:
        for ms in a.sweep_shapes.split(","):
            m, K = (int(v) for v in ms.split(":"))
            for n in [int(v) for v in a.sweep.split(",")]:
                gn, go, sn, so, _ = passes(n, m, K - 1, dev, a.seed)
                for _ in range(3):
                    for fn in (gn, go, sn, so):
                        fn()
                tg1, tg0 = alternate(gn, go, 3 * a.reps, wall)
                ts1, ts0 = alternate(sn, so, 3 * a.reps, wall)
                print(json.dumps({"sweep": True, "n": n, "m": m, "K": K, "grad_new": stats(tg1),
                                  "grad_old": stats(tg0), "search_new": stats(ts1), "search_old": stats(ts0),
                                  "former_path_wins": statistics.median(tg0) < statistics.median(tg1)
                                  or statistics.median(ts0) < statistics.median(ts1)}), flush=True)


if __name__ == "__main__":
    main()
