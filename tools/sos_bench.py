#!/usr/bin/env python3
"""Stochastic Outlier Selection on one GPU: the fused kernels (``ops/sos.py``, ``csrc/sos.hip``) against the path
they replace, ``ALINK_SOS_HIP=0`` (``profiles/sos.txt``).

    python tools/sos_bench.py                                  # the seven shapes
    python tools/sos_bench.py --shapes 20000x8 --reps 7

Per shape ``n x d`` (standard-normal fp64 rows on the device) it times ``sos_scores`` after a warm-up of both paths
at that shape, with device events, the two paths alternated in the same process, then the search and the products
kernel alone (their launches only, the centring and the image outside).

Printed per shape: medians and minima; the mean and the largest ``iters``; the passes the workgroups made (a
workgroup of 64 rows passes until its slowest row is done: ``max iters + 1``) against the passes the rows needed
(``iters + 1``); the time per pair and evaluation of the search and per pair of the products, next to the matrix-core
floor of ``2 d`` flops per pair at the 6e13 flop/s of ``profiles/kmeans_dense64.txt`` (at d = 8 that floor is 0.3 ps,
so the products figure there is the measured cost of one fp64 ``exp`` and one division per pair); and the largest
difference of the scores between the two paths.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "20000x8,50000x32,100000x32,20000x128,20000x256,20000x512,20000x1024"
FLOPS = 6e13                        # profiles/kmeans_dense64.txt: the fp64 matrix cores on this loop shape


def timed(fn):
    """Milliseconds of one call of ``fn`` (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "samples": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x d")
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd.models.outlier.sos import sos_scores
    from alink_amd.ops import _lib, sos as S
    _lib.require()
    dev = torch.device("cuda:0")

    for shape in [s for s in a.shapes.split(",") if s]:
        n, d = (int(v) for v in shape.split("x"))
        X = torch.randn((n, d), dtype=torch.float64, device=dev,
                        generator=torch.Generator(device=dev).manual_seed(a.seed))
        assert S.sos_supported(X)
        state = {}

        def new_path():
            state["new"] = S.scores(X, a.perplexity)

        def old_path():
            os.environ["ALINK_SOS_HIP"] = "0"
            try:
                state["old"] = sos_scores(X, a.perplexity)
            finally:
                os.environ.pop("ALINK_SOS_HIP", None)
        for _ in range(a.warmup):
            new_path()
            old_path()
        t_new, t_old = [], []
        for i in range(max(a.reps, a.old_reps)):
            if i < a.reps:
                t_new.append(timed(new_path))
            if i < a.old_reps:
                t_old.append(timed(old_path))
        peak = torch.cuda.max_memory_allocated() / 1e9
        diff = float((state["new"] - state["old"]).abs().max())
        state.clear()
        prep = S._prepare(X)
        found = {}

        def search():
            found["s"] = S._search_hip(prep, a.perplexity, 0, n, 0)

        def products():
            S._products_hip(prep, found["s"][0], found["s"][1], 0, n, 0)
        alone = {}
        for name, fn in (("search", search), ("products", products)):
            fn()
            torch.cuda.synchronize()
            alone[name] = stats([timed(fn) for _ in range(a.reps)])
        iters = found["s"][2].to(torch.int64)
        pad = torch.zeros(-(-n // 64) * 64, dtype=torch.int64, device=dev)
        pad[:n] = iters
        wg_passes = pad.view(-1, 64).max(1).values + 1
        row_evals = float((iters + 1).sum())                    # evaluations the rows needed
        done_evals = float(wg_passes.sum()) * 64                # evaluations the workgroups made
        print(json.dumps({
            "n": n, "d": d, "perplexity": a.perplexity, "new": stats(t_new), "old": stats(t_old),
            "speedup_median": statistics.median(t_old) / statistics.median(t_new),
            "new_median_below_old_median": statistics.median(t_new) < statistics.median(t_old),
            "kernels": alone, "iters_mean": float(iters.double().mean()), "iters_max": int(iters.max()),
            "workgroup_passes_mean": float(wg_passes.double().mean()),
            "passes_made_over_needed": done_evals / row_evals,
            "search_ps_per_pair_eval": alone["search"]["median_ms"] * 1e9 / (done_evals * n),
            "products_ps_per_pair": alone["products"]["median_ms"] * 1e9 / (float(n) * n),
            "mfma_floor_ps_per_pair": 2.0 * d / FLOPS * 1e12,
            "max_score_diff": diff, "peak_mem_GB": peak}), flush=True)
        del X, prep, found
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()


if __name__ == "__main__":
    main()
