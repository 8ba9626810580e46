#!/usr/bin/env python3
"""Sparse-vector KMeans on one GPU: seeded synthetic CSR rows with Zipf-distributed columns through
``ops/kmeans_sparse.py`` (``profiles/kmeans_sparse.txt``).

    python tools/kmeans_sparse_bench.py --n 100000 --d 16384 --k 100 --dist EUCLIDEAN --dense   # against densified
    python tools/kmeans_sparse_bench.py --n 2000000 --d 262144 --k 100 --dist COSINE            # the target shape

Prints one JSON line: per Lloyd superstep the sparse assign+accumulate time and its ``nearest`` / ``accum`` parts
(medians of ``--reps`` warmed-up samples of ``--inner`` calls each; with ``--dense`` the densified fp64 step of
``ops/kmeans.assign_accumulate`` is timed alternately with the sparse one), the one-time CSC build, peak device
memory, and the gathered bytes per second of ``nearest`` (``nnz * kp * 8 / t``; the time includes transposing and
padding the centroids, as every superstep does).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def zipf_csr(n, d, nnz, seed, device):
    """``n`` rows of about ``nnz`` distinct columns each, column j drawn with probability ~ 1/(j+1) (log-uniform
    over [1, d+1)), values uniform in [0.5, 1.5); duplicates inside a row are dropped."""
    g = torch.Generator(device=device).manual_seed(seed)
    u = torch.rand(n * nnz, generator=g, device=device, dtype=torch.float64)
    col = (torch.exp(u * torch.log(torch.tensor(float(d + 1), dtype=torch.float64, device=device))) - 1.0)
    col = col.to(torch.int64).clamp_(0, d - 1)
    row = torch.arange(n, device=device).repeat_interleave(nnz)
    key = torch.unique(row * d + col)            # sorted: rows ascend, columns ascend inside a row
    del u, col, row
    row, col = key // d, key % d
    crow = torch.zeros(n + 1, dtype=torch.int64, device=device)
    crow[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    val = torch.rand(key.numel(), generator=g, device=device, dtype=torch.float64) + 0.5
    return crow, col, val


def timed(fn, inner=1):
    """Milliseconds per call of ``fn`` over ``inner`` back-to-back calls (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return [a.elapsed_time(b) / inner]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=1 << 14)
    ap.add_argument("--nnz", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--dist", default="EUCLIDEAN")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls per timed sample")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense", action="store_true", help="also time the densified fp64 step, alternately")
    a = ap.parse_args()
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import _lib, kmeans as kops, kmeans_sparse as ksp
    _lib.require()
    dev = torch.device("cuda:0")
    crow, col, val = zipf_csr(a.n, a.d, a.nnz, a.seed, dev)
    fm = FeatureMatrix(crow=crow, col=col, val=val, ncols=a.d)
    nnz = int(col.numel())
    if a.dist.upper() == "COSINE":
        nrm = ksp.row_sqnorm(fm).sqrt_()
        fm = FeatureMatrix(crow=crow, col=col, val=val / nrm.clamp_min(1e-300)[fm.row_ids()], ncols=a.d)
    pick = torch.randperm(a.n, generator=torch.Generator().manual_seed(a.seed + 1))[:a.k]
    C = ksp.take_dense(fm, pick)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    build = timed(lambda: ksp.prepare(fm))[0]
    csc = ksp.prepare(fm)
    out = {"n": a.n, "d": a.d, "k": a.k, "dist": a.dist.upper(), "nnz": nnz, "nnz_per_row": nnz / a.n,
           "csc_build_ms": build, "work_items": csc.nwork, "multi_chunk_columns": csc.nmulti,
           "longest_column": int((torch.bincount(col, minlength=a.d)).max())}
    state = {}

    def nearest():
        state["idx"], _, state["cnt"] = ksp.nearest_hip(fm, C, a.dist, True, False, True)

    def accum():
        state["buf"] = ksp.accumulate_hip(fm, state["idx"], a.k, a.d, state["cnt"])

    def sparse_step():
        state["buf"] = ksp.assign_accumulate(fm, C, a.dist)

    Xd = fm.to_dense() if a.dense else None

    def dense_step():
        state["dbuf"] = kops.assign_accumulate(Xd, C)

    for _ in range(a.warmup):
        sparse_step()
        if a.dense:
            dense_step()
    t_sparse, t_dense, t_near, t_acc = [], [], [], []
    for _ in range(a.reps):                   # alternating runs
        t_sparse += timed(sparse_step, a.inner)
        if a.dense:
            t_dense += timed(dense_step, a.inner)
        t_near += timed(nearest, a.inner)
        t_acc += timed(accum, a.inner)
    med = statistics.median
    kp = max(64, (a.k + 63) // 64 * 64)
    out.update({"sparse_step_ms": med(t_sparse), "sparse_step_ms_all": t_sparse, "nearest_ms": med(t_near),
                "nearest_ms_all": t_near, "accum_ms": med(t_acc), "accum_ms_all": t_acc,
                "nearest_gather_TBps": nnz * kp * 8 / (med(t_near) * 1e-3) / 1e12,
                "table_MB": a.d * kp * 8 / 1e6, "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9})
    if a.dense:
        out.update({"dense_step_ms": med(t_dense), "dense_step_ms_all": t_dense,
                    "dense_matrix_GB": a.n * a.d * 8 / 1e9,
                    "counts_equal": bool(torch.equal(state["buf"][:, -1], state["dbuf"][:, -1])),
                    "max_sum_diff": float((state["buf"] - state["dbuf"]).abs().max())})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
