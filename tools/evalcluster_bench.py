#!/usr/bin/env python3
"""EvalClusterBatchOp on one GPU: the fused row pass and exact cluster sums (``ops/evalcluster.py``) against the host
path they replace, ``ALINK_EVALCLUSTER_HIP=0`` (``profiles/evalcluster.txt``).

    python tools/evalcluster_bench.py                            # the two dense shapes and the CSR shape
    python tools/evalcluster_bench.py --shapes 1000000x37x8 --reps 5 --csr ""

Per dense shape ``n x d x k`` (fp64 rows on the device, an int64 prediction column on the device) it times, after a
warm-up of every path at that shape:

* the whole operator (host clock around a call that ends in a device synchronise: the cluster ids, both passes, the
  centre distances, the metrics' JSON), new against ``ALINK_EVALCLUSTER_HIP=0`` in the same process, alternated;
  ``--old-reps`` samples of the old path (its per-row Python loop over the prediction column takes seconds);
* the three passes alone with device events: ``sorted_work`` + ``cluster_sums``, ``row_pass``, ``cluster_row_sums``.

Printed per shape: medians and minima, the bytes of one pass over the rows, that over the 6.12 TB/s load-only rate
README records as the floor, how far the row pass sits from it, and the largest relative difference of the numeric
metrics between the two paths.  The CSR shape ``n x d x k @ nnz`` is reported alone: its dense matrix does not exist,
so the old path cannot run; its floor is one pass over the CSR arrays.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "10000000x128x100,20000000x16x50"
CSR = "200000x262144x100@100"
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
    return {"median_ms": statistics.median(t), "min_ms": min(t), "samples": len(t)}


def operator(mt, flag, state, key):
    from alink_amd import EvalClusterBatchOp
    from alink_amd.operator.batch.source import TableSourceBatchOp

    def run():
        if flag is None:
            os.environ.pop("ALINK_EVALCLUSTER_HIP", None)
        else:
            os.environ["ALINK_EVALCLUSTER_HIP"] = flag
        try:
            op = EvalClusterBatchOp().setVectorCol("v").setPredictionCol("p")
            state[key] = json.loads(op.linkFrom(TableSourceBatchOp(mt)).collect()[0][0])
        finally:
            os.environ.pop("ALINK_EVALCLUSTER_HIP", None)
    return run


def passes(R, cid, k, reps, warmup):
    """Medians of the three passes alone on the rows object ``R``."""
    from alink_amd.ops import evalcluster as ev
    state = {}

    def sums():
        state["work"] = ev.sorted_work(R, cid, k)
        state["buf"] = ev.cluster_sums(R, cid, k, state["work"])

    def rowp():
        buf, d = state["buf"], R.d
        cnt = buf[:, d].contiguous()
        state["block"] = ev.row_pass(R, cid, buf[:, :d] / cnt.clamp_min(1.0)[:, None], cnt,
                                     buf[:, d + 1].contiguous(), "EUCLIDEAN")

    def rsums():
        state["rs"] = ev.cluster_row_sums(state["block"], cid, k, state["work"])
    out = {}
    for name, fn in (("sorted_work+cluster_sums", sums), ("row_pass", rowp), ("cluster_row_sums", rsums)):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        out[name] = stats([timed(fn) for _ in range(reps)])
    return out


def rel_diff(a, b):
    worst = 0.0
    for key, v in a.items():
        if key in ("clusterArray", "countArray", "k", "count"):
            assert v == b[key], key
            continue
        x, y = float(v), float(b[key])
        if x == x or y == y:
            worst = max(worst, abs(x - y) / max(abs(x), abs(y), 1e-300))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x d x k")
    ap.add_argument("--csr", default=CSR, help="n x d x k @ entries per row, or empty")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd import useLocalEnv
    from alink_amd.common.linalg.block import SparseBlock
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import _lib, evalcluster as ev
    from alink_amd.ops.kmeans_rows import _Dense64Rows, _SparseRows
    _lib.require()
    dev = torch.device("cuda:0")
    useLocalEnv(1, device="cuda:0")

    for shape in [s for s in a.shapes.split(",") if s]:
        n, d, k = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(a.seed)
        pred = torch.randint(0, k, (n,), device=dev, generator=g)
        centres = torch.randn((k, d), dtype=torch.float64, device=dev, generator=g) * 4.0
        X = torch.randn((n, d), dtype=torch.float64, device=dev, generator=g)
        X += centres[pred]
        del centres
        mt = MTable(TableSchema(["v", "p"], [Types.DENSE_VECTOR, Types.LONG]), [Column(X), Column(pred)])
        state = {}
        new_op, old_op = operator(mt, None, state, "new"), operator(mt, "0", state, "old")
        for _ in range(a.warmup):
            new_op()
        old_op()            # the old path's warm-up is one full run
        t_new, t_old = [], []
        for i in range(a.reps):
            t_new.append(wall(new_op))
            if i < a.old_reps:
                t_old.append(wall(old_op))
        peak = torch.cuda.max_memory_allocated() / 1e9
        R = ev.eval_rows(FeatureMatrix(X), d, "EUCLIDEAN")
        assert type(R) is _Dense64Rows
        alone = passes(R, pred.to(torch.int32), k, a.reps, a.warmup)
        floor = n * d * 8 / LOAD_BPS * 1e3
        print(json.dumps({"n": n, "d": d, "k": k, "operator_new": stats(t_new), "operator_old": stats(t_old),
                          "speedup_median": statistics.median(t_old) / statistics.median(t_new),
                          "passes": alone, "one_pass_bytes": n * d * 8, "floor_ms": floor,
                          "row_pass_over_floor": alone["row_pass"]["median_ms"] / floor,
                          "max_rel_metric_diff": rel_diff(state["new"], state["old"]),
                          "silhouette": state["new"]["silhouetteCoefficient"], "peak_mem_GB": peak}), flush=True)
        del X, mt, R, pred, state
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    if a.csr:
        shape, nnz = a.csr.split("@")
        n, d, k = (int(v) for v in shape.split("x"))
        nnz = int(nnz)
        g = torch.Generator(device=dev).manual_seed(a.seed)
        pred = torch.randint(0, k, (n,), device=dev, generator=g)
        # documents of nnz distinct columns: a random start and odd strides keep the columns of a row distinct
        start = torch.randint(0, d, (n, 1), device=dev, generator=g)
        stride = torch.randint(0, d // (2 * nnz), (n, 1), device=dev, generator=g) * 2 + 1
        col = ((start + stride * torch.arange(nnz, device=dev)[None, :]) % d).reshape(-1)
        val = torch.rand(n * nnz, dtype=torch.float64, device=dev, generator=g) + 0.5
        crow = torch.arange(n + 1, device=dev) * nnz
        mt = MTable(TableSchema(["v", "p"], [Types.SPARSE_VECTOR, Types.LONG]),
                    [Column(SparseBlock(crow, col, val, d)), Column(pred)])
        state = {}
        new_op = operator(mt, None, state, "new")
        for _ in range(a.warmup):
            new_op()
        t_new = [wall(new_op) for _ in range(a.reps)]
        peak = torch.cuda.max_memory_allocated() / 1e9
        R = ev.eval_rows(FeatureMatrix(crow=crow, col=col, val=val, ncols=d), d, "EUCLIDEAN")
        assert type(R) is _SparseRows
        alone = passes(R, pred.to(torch.int32), k, a.reps, a.warmup)
        csr_bytes = n * nnz * 16 + (n + 1) * 8
        floor = csr_bytes / LOAD_BPS * 1e3
        print(json.dumps({"csr": True, "n": n, "d": d, "k": k, "entries_per_row": nnz, "operator_new": stats(t_new),
                          "passes": alone, "one_pass_bytes": csr_bytes, "floor_ms": floor,
                          "row_pass_over_floor": alone["row_pass"]["median_ms"] / floor,
                          "dense_matrix_GB": n * d * 8 / 1e9, "count": state["new"]["count"],
                          "silhouette": state["new"]["silhouetteCoefficient"], "peak_mem_GB": peak}), flush=True)


if __name__ == "__main__":
    main()
