#!/usr/bin/env python3
"""Dense fp64 KMeans on one GPU: ``ops/kmeans_dense64.py`` against the torch fp64 path it replaces
(``profiles/kmeans_dense64.txt``).

    python tools/kmeans_dense64_bench.py                       # the four shapes of the profile
    python tools/kmeans_dense64_bench.py --shapes 1000000x37x20 --reps 10

Per shape ``n x d x k`` it times, with device events and after a warm-up of every path at that shape:

* ``assign_accumulate`` (the Lloyd step) against ``ops.kmeans.assign_accumulate_torch``;
* ``nearest_counts`` against 2k+1 candidates (the k-means|| weights pass) and ``nearest`` distances against the
  torch kind of ``ops/kmeans_rows.py`` (chunked ``pairwise_distance``) for the same candidates;
* ``nearest`` with the predict shape (k centroids), which has no torch counterpart worth timing: the mapper built
  the whole [n, k] matrix.

Old and new runs alternate in one process, ``--reps`` samples each.  Printed per shape: both medians and minima,
the bytes and FLOP of the shape, the two floors (bytes over the 6.12 TB/s load-only rate README records for the
bf16 kernel, 25.6 GB in 4.18 ms; FLOP over the 78.6 TFLOP/s fp64 matrix rate of the MI355X data sheet), which floor
binds, whether the new median is at least 10 % under the old minimum, and max |old - new| of the [k, d+1] buffers.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "10000000x128x100,4000000x300x100,20000000x16x50,2000000x768x256"
LOAD_BPS = 25.6e9 / 4.18e-3         # README: the bf16 kernel's load-only pass over 1e8 x 128 bf16
F64_MFMA_FLOPS = 78.6e12            # MI355X data sheet, fp64 matrix


def timed(fn):
    """Milliseconds of one call of ``fn`` (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def min_dist_torch(X, C, chunk=1 << 20):
    """The minimum distance as the torch kind of ``ops/kmeans_rows.py`` computes it for fp64 rows (EUCLIDEAN)."""
    from alink_amd.models.clustering.kmeans import pairwise_distance
    return torch.cat([pairwise_distance(X[s:s + chunk], C, "EUCLIDEAN").min(1).values
                      for s in range(0, X.shape[0], chunk)])


def ab(new, old, reps):
    """Alternating samples: (new times, old times) in ms."""
    tn, to = [], []
    for _ in range(reps):
        tn.append(timed(new))
        to.append(timed(old))
    return tn, to


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x d x k")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd.ops import _lib, kmeans as kops, kmeans_dense64 as kd
    from alink_amd.ops.kmeans_rows import rows
    _lib.require()
    dev = torch.device("cuda:0")
    for shape in a.shapes.split(","):
        n, d, k = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(a.seed)
        X = torch.randn((n, d), dtype=torch.float64, device=dev, generator=g)
        pick = torch.randperm(n, generator=torch.Generator().manual_seed(a.seed + 1))[:2 * k + 1].to(dev)
        cand = X[pick].contiguous()
        C = cand[:k].contiguous()
        assert kd.dense64_selected(X, k)
        R = rows(X, "EUCLIDEAN")
        state = {}

        def new_step():
            state["new"] = kd.assign_accumulate(X, C)

        def old_step():
            state["old"] = kops.assign_accumulate_torch(X, C)

        def new_counts():
            state["cnt"] = kd.nearest_counts(X, cand, "EUCLIDEAN")

        def new_dist():
            state["nd"] = R.nearest(cand)[1]

        def old_dist():
            state["od"] = min_dist_torch(X, cand)

        def new_predict():
            state["pred"] = kd.nearest(X, C, "EUCLIDEAN")

        fns = (new_step, old_step, new_counts, new_dist, old_dist, new_predict)
        for _ in range(a.warmup):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        t_new, t_old = ab(new_step, old_step, a.reps)
        t_nd, t_od = ab(new_dist, old_dist, a.reps)
        t_cnt = [timed(new_counts) for _ in range(a.reps)]
        t_pred = [timed(new_predict) for _ in range(a.reps)]
        nt = kd.tiles(k)
        kpad = (k + 16 * nt - 1) // (16 * nt) * 16 * nt
        dpad = (d + 31) // 32 * 32
        step_bytes = 2.0 * n * d * 8                    # the rows are read by the nearest pass and by the sums
        step_flop = 2.0 * n * dpad * kpad
        fl_b, fl_f = step_bytes / LOAD_BPS * 1e3, step_flop / F64_MFMA_FLOPS * 1e3
        out = {"n": n, "d": d, "k": k, "reps": a.reps,
               "assign_accumulate_new": stats(t_new), "assign_accumulate_torch": stats(t_old),
               "speedup_median": statistics.median(t_old) / statistics.median(t_new),
               "new_median_10pct_under_old_min": statistics.median(t_new) <= 0.9 * min(t_old),
               "step_bytes": step_bytes, "step_flop": step_flop, "floor_bytes_ms": fl_b, "floor_mfma_ms": fl_f,
               "floor_binds": "bytes" if fl_b >= fl_f else "mfma",
               "min_dist_new_2k1": stats(t_nd), "min_dist_torch_2k1": stats(t_od),
               "min_dist_new_10pct_under_old_min": statistics.median(t_nd) <= 0.9 * min(t_od),
               "nearest_counts_2k1": stats(t_cnt), "nearest_predict": stats(t_pred),
               "counts_equal": bool(torch.equal(state["new"][:, -1], state["old"][:, -1])),
               "max_abs_buffer_diff": float((state["new"] - state["old"]).abs().max()),
               "max_abs_min_dist_diff": float((state["nd"] - state["od"]).abs().max()),
               "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}
        print(json.dumps(out), flush=True)
        del X, state
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()


if __name__ == "__main__":
    main()
