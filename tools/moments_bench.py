#!/usr/bin/env python3
"""The moment pass and the fused PCA projection on one GPU (``ops/moments.py``, ``csrc/moments.hip``) against the
chains they replace (``profiles/moments.txt``).

    python tools/moments_bench.py                        # the five shapes, the two projections and the sweep
    python tools/moments_bench.py --shapes 1000000x512 --project "" --sweep ""

Per shape ``n x d`` (fp64 rows on the device, columns of mean 5 and unit spread) it times with device events, after a
warm-up of both paths at that shape, the two paths alternated in the same process:

* new: one ``moments(X, shift)`` call (the three row kernels and the merge);
* former: ``train_pca``'s chain ``X.sum(0)``, ``(X * X).sum(0)``, ``tn_matmul(X, X)``.

Printed per shape: medians and minima, the spread (max - min over the median) of the former path's runs, the new
pass over the floor of one load of X at the 6.12 TB/s load-only rate README records and over the floor of the
n d (d + 1) useful operations of the upper triangle at the 78.6 TFLOP/s fp64 matrix rate, and ``select``: whether
the new pass is no slower than the former chain by more than that spread.

``--project n x nx x k``: ``pca_project`` against the former gather / subtract / divide / where / GEMM chain.
``--sweep``: both moment paths over small n on the host clock around a synchronised call: the largest n at which the
former chain still wins sets ``MOMENTS_MIN_ROWS``.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "20000000x8,10000000x32,2000000x128,1000000x512,200000x1024"
PROJECT = "10000000x32x8,2000000x128x16"
SWEEP = "64,256,1024,4096,16384,65536,262144"
LOAD_BPS = 25.6e9 / 4.18e-3         # README: the bf16 KMeans kernel's load-only pass over 1e8 x 128 bf16
MFMA_FLOPS = 78.6e12                # fp64 matrix rate of the MI355X data sheet


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
    return {"median_ms": statistics.median(t), "min_ms": min(t), "samples": len(t)}


def alternate(new, old, reps, old_reps, clock):
    for _ in range(2):
        new()
        old()
    t_new, t_old = [], []
    for i in range(reps):
        t_new.append(clock(new))
        if i < old_reps:
            t_old.append(clock(old))
    return t_new, t_old


def compare(t_new, t_old):
    spread = (max(t_old) - min(t_old)) / statistics.median(t_old)
    ratio = statistics.median(t_new) / statistics.median(t_old)
    return {"new": stats(t_new), "former": stats(t_old), "former_spread": spread, "new_over_former": ratio,
            "select": ratio <= 1.0 + spread}


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x d")
    ap.add_argument("--project", default=PROJECT, help="comma-separated n x nx x k, or empty")
    ap.add_argument("--sweep", default=SWEEP, help="comma-separated n of the small-n sweep, or empty")
    ap.add_argument("--sweep-d", default="8,32,128", help="comma-separated d of the sweep")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--old-reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd.ops import _lib, moments as M
    from alink_amd.ops.gemm import tn_matmul
    _lib.require()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(a.seed)

    def draw(n, d):
        return torch.randn((n, d), dtype=torch.float64, device=dev, generator=g) + 5.0

    def passes(X, state):
        shift = X[0].clone()

        def new():
            state["new"] = M.moments(X, shift)

        def old():
            state["old"] = (X.sum(0), (X * X).sum(0), tn_matmul(X, X))
        return shift, new, old

    for shape in [s for s in a.shapes.split(",") if s]:
        n, d = (int(v) for v in shape.split("x"))
        X = draw(n, d)
        state = {}
        shift, new, old = passes(X, state)
        res = compare(*alternate(new, old, a.reps, a.old_reps, timed))
        t, C = state["new"]
        s, _, G = state["old"]      # the same statistics from both: sum x and X^T X
        diff = {"sum": rel(t + n * shift, s),
                "gram": rel(C + torch.outer(shift, t) + torch.outer(t, shift) + n * torch.outer(shift, shift), G)}
        state.clear()
        load_ms = 8 * n * d / LOAD_BPS * 1e3
        mfma_ms = n * d * (d + 1) / MFMA_FLOPS * 1e3
        med = res["new"]["median_ms"]
        print(json.dumps({"n": n, "d": d, **res, "load_floor_ms": load_ms, "over_load_floor": med / load_ms,
                          "mfma_floor_ms": mfma_ms, "over_mfma_floor": med / mfma_ms,
                          "chunk_rows": M.moments_chunk_rows(n, d), "max_rel_diff": diff,
                          "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}), flush=True)
        del X, new, old, t, C, s, G
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    for shape in [s for s in a.project.split(",") if s]:
        n, nx, k = (int(v) for v in shape.split("x"))
        X = draw(n, nx)
        idx = torch.arange(1, nx, device=dev)           # column 0 dropped as a constant column is
        mean, std = torch.full((nx - 1,), 5.0, dtype=torch.float64, device=dev), \
            torch.rand(nx - 1, dtype=torch.float64, device=dev, generator=g) + 0.5
        coef = torch.randn((k, nx - 1), dtype=torch.float64, device=dev, generator=g)
        sstd = torch.rand(k, dtype=torch.float64, device=dev, generator=g) + 0.5
        ok = std.abs() > 1e-12
        col_mean, col_scale = torch.zeros(nx, dtype=torch.float64, device=dev), \
            torch.zeros(nx, dtype=torch.float64, device=dev)
        col_mean[idx], col_scale[idx] = mean, std
        table = torch.zeros((k, nx), dtype=torch.float64, device=dev)
        table[:, idx] = coef
        img = M.project_table(table.cpu(), dev)
        state = {}

        def new():
            state["new"] = M.pca_project(X, col_mean, col_scale, img, sstd)

        def old():          # PcaModelMapper._project_device
            Z = X[:, idx]
            Zs = (Z - mean[None, :]) / std[None, :]
            Z = torch.where(ok[None, :], Zs, torch.zeros_like(Z))
            state["old"] = Z @ coef.T / sstd[None, :]
        res = compare(*alternate(new, old, a.reps, a.old_reps, timed))
        pass_ms = 8 * n * (nx + k) / LOAD_BPS * 1e3
        print(json.dumps({"project": True, "n": n, "nx": nx, "k": k, **res, "load_floor_ms": pass_ms,
                          "over_load_floor": res["new"]["median_ms"] / pass_ms,
                          "max_rel_diff": rel(state["new"], state["old"])}), flush=True)
        del X, state
        torch.cuda.empty_cache()

    if a.sweep:
        for d in [int(v) for v in a.sweep_d.split(",")]:
            for n in [int(v) for v in a.sweep.split(",")]:
                _, new, old = passes(draw(n, d), {})
                res = compare(*alternate(new, old, 4 * a.reps, 4 * a.reps, wall))
                print(json.dumps({"sweep": True, "n": n, "d": d, **res,
                                  "former_path_wins": res["new_over_former"] > 1.0}), flush=True)


if __name__ == "__main__":
    main()
