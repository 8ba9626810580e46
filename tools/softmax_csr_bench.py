#!/usr/bin/env python3
"""Softmax regression on CSR rows on one GPU: the row pass and the gradient gather (``ops/softmax_csr.py``,
``csrc/softmax_csr.hip``) against the chain they replace (``profiles/softmax_csr.txt``).

    python tools/softmax_csr_bench.py                           # the shapes, the 1e7-row run and the sweep
    python tools/softmax_csr_bench.py --shapes 200000 --alone "" --sweep ""

Rows are hashed documents: ``--entries`` (100) stored entries per row under ``--features`` (2^18) columns plus the
prefixed intercept column, int64 column indices, ``--classes`` (20) labels.  Per ``n`` of ``--shapes`` it times, after
a warm-up of both paths (which also builds the cached CSC view), the two paths alternated in the same process with
device events:

* the gradient: ``grad`` against ``grad_torch`` (``fm.mm``, the softmax formulas, ``fm.rmm`` with its float atomics);
* the line search of 11 steps: ``search_losses`` against ``search_losses_torch``;

and, for the new path alone, the row pass (``rows`` for R and the loss), the gather (``gather``) with the bytes per
second of its R lines (entries x k1 x 8 B over its time), the merge of the intercept column's chunks (the gather of a
matrix cut down to that column) and the NaiveBayes CSR row kernel on the same rows and a table of the same size
(the same walk of ``csr_rows.h``; it writes ``prob [n, L]`` where the row pass writes ``R [n, k1]``).
``--alone``: the new path only, at sizes whose ``[nnz, k1]`` blocks the former path cannot hold.
``--sweep``: gradient plus search at two shapes over small n, host clock around a synchronised call: the smallest n
from which the new path wins at both sets ``SOFTMAX_CSR_MIN_ROWS``.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NSTEPS = 11


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


def documents(n, entries, features, k1, dev, seed):
    """(fm, y, w, W, D): n rows of ``entries`` random columns each (sorted inside a row; a repeated column is kept, as
    a hasher's collisions are) behind a prefixed intercept column."""
    from alink_amd.models.common.features import FeatureMatrix
    g = torch.Generator(device=dev).manual_seed(seed)
    col = torch.randint(0, features, (n, entries), device=dev, generator=g).sort(1).values.reshape(-1)
    val = torch.rand(n * entries, dtype=torch.float64, device=dev, generator=g) + 0.5
    crow = torch.arange(n + 1, device=dev, dtype=torch.int64) * entries
    fm = FeatureMatrix(crow=crow, col=col, val=val, ncols=features).prefix_one()
    m = fm.ncols
    W = torch.randn((k1, m), dtype=torch.float64, device=dev, generator=g) * (3.0 / entries ** 0.5)
    D = torch.randn((k1, m), dtype=torch.float64, device=dev, generator=g) / entries ** 0.5
    y = torch.randint(0, k1 + 1, (n,), device=dev, generator=g).double()
    w = torch.rand(n, dtype=torch.float64, device=dev, generator=g) + 0.5
    return fm, y, w, W, D


def new_path_alone(fm, y, w, W, reps):
    """Timings of the new path's parts and the NaiveBayes row kernel on the same rows."""
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import naive_bayes as NB, softmax_csr as S
    k1, m = W.shape
    n, nnz = fm.nrows, int(fm.val.numel())
    R = S.rows(fm, y, w, W, ("R",))["R"]
    # the intercept column alone: its n entries are the only multi-chunk column of hashed documents
    one = FeatureMatrix(crow=torch.arange(n + 1, device=fm.val.device), col=torch.zeros_like(fm.col[:n]),
                        val=torch.ones_like(fm.val[:n]), ncols=m)
    nb_rows, table = NB.predict_rows(fm, m), NB.Table(W, torch.zeros(k1, dtype=torch.float64, device=W.device))
    parts = {"rows_R_loss": lambda: S.rows(fm, y, w, W, ("R", "loss")), "gather": lambda: S.gather(fm, R),
             "intercept_column_gather_and_merge": lambda: S.gather(one, R),
             "nb_rows_csr_prob": lambda: NB.predict(nb_rows, table, want_prob=True)}
    out = {}
    for name, fn in parts.items():
        fn()
        out[name] = stats([timed(fn) for _ in range(reps)])
    out["gather_R_line_bytes_per_s"] = nnz * k1 * 8 / (out["gather"]["median_ms"] * 1e-3)
    out["rows_entry_bytes_per_s"] = nnz * 16 / (out["rows_R_loss"]["median_ms"] * 1e-3)
    out["intercept_chunks"] = -(-n // 512)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200000,1000000", help="comma-separated n, both paths alternated")
    ap.add_argument("--alone", default="10000000", help="comma-separated n of the new path alone, or empty")
    ap.add_argument("--sweep", default="64,1000,10000,100000", help="comma-separated n of the small-n sweep, or empty")
    ap.add_argument("--sweep-shapes", default="262144:100:20,4096:20:5", help="features : entries : classes")
    ap.add_argument("--features", type=int, default=1 << 18)
    ap.add_argument("--entries", type=int, default=100)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd.ops import _lib, softmax_csr as S
    _lib.require()
    dev = torch.device("cuda:0")
    k1 = a.classes - 1
    for n in [int(v) for v in a.shapes.split(",") if v]:
        fm, y, w, W, D = documents(n, a.entries, a.features, k1, dev, a.seed)
        out = {}
        gn = lambda: out.__setitem__("g1", S.grad(fm, y, w, W)[0])
        go = lambda: out.__setitem__("g0", S.grad_torch(fm, y, w, W)[0])
        sn = lambda: out.__setitem__("s1", S.search_losses(fm, y, w, W, D, 0.37, NSTEPS))
        so = lambda: out.__setitem__("s0", S.search_losses_torch(fm, y, w, W, D, 0.37, NSTEPS))
        for fn in (gn, go, sn, so):
            fn()
        tg1, tg0 = alternate(gn, go, a.reps, timed)
        ts1, ts0 = alternate(sn, so, a.reps, timed)
        print(json.dumps({
            "n": n, "m": fm.ncols, "entries": int(fm.val.numel()), "K": a.classes,
            "grad_new": stats(tg1), "grad_old": stats(tg0),
            "grad_speedup_median": statistics.median(tg0) / statistics.median(tg1),
            "search_new": stats(ts1), "search_old": stats(ts0),
            "search_speedup_median": statistics.median(ts0) / statistics.median(ts1),
            "former_block_bytes": int(fm.val.numel()) * k1 * 8,
            "max_rel_diff": {"G": rel(out["g1"], out["g0"]), "search": rel(out["s1"], out["s0"])},
            "new_path_parts": new_path_alone(fm, y, w, W, a.reps),
            "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}), flush=True)
        del fm, y, w, W, D, out, gn, go, sn, so
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    for n in [int(v) for v in a.alone.split(",") if v]:
        fm, y, w, W, D = documents(n, a.entries, a.features, k1, dev, a.seed)
        gn = lambda: S.grad(fm, y, w, W)
        sn = lambda: S.search_losses(fm, y, w, W, D, 0.37, NSTEPS)
        t_prepare = wall(gn)            # the first call builds the CSC view
        sn()
        print(json.dumps({
            "alone": True, "n": n, "m": fm.ncols, "entries": int(fm.val.numel()), "K": a.classes,
            "first_grad_with_csc_build_ms": t_prepare, "grad_new": stats([timed(gn) for _ in range(a.reps)]),
            "search_new": stats([timed(sn) for _ in range(a.reps)]),
            "former_block_bytes": int(fm.val.numel()) * k1 * 8,
            "new_path_parts": new_path_alone(fm, y, w, W, a.reps),
            "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}), flush=True)
        del fm, y, w, W, D, gn, sn
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    if a.sweep:
        for shape in a.sweep_shapes.split(","):
            features, entries, K = (int(v) for v in shape.split(":"))
            for n in [int(v) for v in a.sweep.split(",")]:
                fm, y, w, W, D = documents(n, entries, features, K - 1, dev, a.seed)
                new = lambda: (S.grad(fm, y, w, W), S.search_losses(fm, y, w, W, D, 0.37, NSTEPS))
                old = lambda: (S.grad_torch(fm, y, w, W), S.search_losses_torch(fm, y, w, W, D, 0.37, NSTEPS))
                for _ in range(3):
                    new()
                    old()
                t1, t0 = alternate(new, old, 3 * a.reps, wall)
                print(json.dumps({"sweep": True, "n": n, "features": features, "entries": entries, "K": K,
                                  "grad_plus_search_new": stats(t1), "grad_plus_search_old": stats(t0),
                                  "former_path_wins": statistics.median(t0) < statistics.median(t1)}), flush=True)


if __name__ == "__main__":
    main()
