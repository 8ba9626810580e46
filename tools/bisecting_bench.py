#!/usr/bin/env python3
"""BisectingKMeans on one GPU: the descent kernel and exact child sums (``ops/bisecting.py``, ``Rows.descend`` /
``Rows.child_stats``) against the torch chain they replace (``profiles/bisecting.txt``).

    python tools/bisecting_bench.py                            # the three dense shapes and the CSR shape
    python tools/bisecting_bench.py --shapes 1000000x37x8 --reps 10 --csr ""

Per dense shape ``n x d x k`` it times, with device events and after a warm-up of every path at that shape:

* one inner iteration, ``descend(levels=1)`` + ``child_stats``, with ``k / 2`` dividing nodes and every row in one of
  them (the last bisecting round's load), HIP kind against the same rows forced to the torch kind;
* the whole ``train_bisecting_kmeans`` (``--train-iters`` inner iterations per round), new against
  ``ALINK_KMEANS_DENSE64=0``;
* prediction with the trained model on the device column, new against ``ALINK_KMEANS_DENSE64=0``.

Old and new runs alternate in one process, ``--reps`` samples each (``--train-reps`` for training).  Printed per
shape: medians and minima of both paths, the bytes an iteration must move (the rows once for the descent and once for
the sums), that over the 6.12 TB/s load-only rate README records as the floor, how far the descent alone sits from
its half of it, whether the new median is at least 10 % under the old minimum, whether the child counts are equal and
max |old - new| of the statistics buffer.  The CSR shape ``n x d x k @ nnz`` is reported alone: its dense matrix
does not exist.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "4000000x128x64,20000000x16x32,1000000x768x32"
CSR = "200000x262144x16@100"
LOAD_BPS = 25.6e9 / 4.18e-3         # README: the bf16 KMeans kernel's load-only pass over 1e8 x 128 bf16


def timed(fn):
    """Milliseconds of one call of ``fn`` (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def ab(new, old, reps):
    tn, to = [], []
    for _ in range(reps):
        tn.append(timed(new))
        to.append(timed(old))
    return tn, to


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t)}


def round_table(m, d, seed, dev):
    """The table of a round with ``m`` dividing nodes (ids m .. 2m-1) and their children, random centres."""
    from alink_amd.ops.bisecting import tree_table
    rng = np.random.default_rng(seed)
    split = list(range(m, 2 * m))
    kids = [x for c in split for x in (2 * c, 2 * c + 1)]
    centers = {c: rng.normal(size=d) for c in kids}
    return tree_table(centers, split + kids, False, dev)


def iteration(R, table, start, m, state, key):
    def run():
        slot = R.descend(table, start.clone(), 1)
        state[key] = R.child_stats(slot - m, 2 * m)
    return run


def column(X):
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    return MTable(TableSchema(["v"], [Types.DENSE_VECTOR]), [Column(X)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x d x k")
    ap.add_argument("--csr", default=CSR, help="n x d x k @ entries per row, or empty")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--train-reps", type=int, default=3)
    ap.add_argument("--train-iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd import BisectingKMeansPredictBatchOp, useLocalEnv
    from alink_amd.common.model.converter import SimpleModelDataConverter
    from alink_amd.common.params import Params
    from alink_amd.common.table import MTable
    from alink_amd.models.clustering.bisecting import train_bisecting_kmeans
    from alink_amd.operator.batch.source import TableSourceBatchOp
    from alink_amd.ops import _lib
    from alink_amd.ops.kmeans_rows import _Dense64Rows, _SparseRows, _TorchRows, rows
    _lib.require()
    dev = torch.device("cuda:0")
    env = useLocalEnv(1, device="cuda:0")
    os.environ.pop("ALINK_KMEANS_DENSE64", None)

    def forced(flag, fn):
        def run():
            if flag is None:
                os.environ.pop("ALINK_KMEANS_DENSE64", None)
            else:
                os.environ["ALINK_KMEANS_DENSE64"] = flag
            try:
                return fn()
            finally:
                os.environ.pop("ALINK_KMEANS_DENSE64", None)
        return run

    for shape in [s for s in a.shapes.split(",") if s]:
        n, d, k = (int(v) for v in shape.split("x"))
        m = k // 2
        g = torch.Generator(device=dev).manual_seed(a.seed)
        X = torch.randn((n, d), dtype=torch.float64, device=dev, generator=g)
        new_rows, old_rows = rows(X, "EUCLIDEAN"), _TorchRows(X, "EUCLIDEAN")
        assert type(new_rows) is _Dense64Rows
        table = round_table(m, d, a.seed, dev)
        start = torch.randint(0, m, (n,), device=dev, generator=g).to(torch.int32)
        state = {}
        new_it, old_it = iteration(new_rows, table, start, m, state, "new"), \
            iteration(old_rows, table, start, m, state, "old")

        def new_descend():
            new_rows.descend(table, start.clone(), 1)

        mt = column(X)
        p = Params().set("vectorCol", "v").set("k", k).set("maxIter", a.train_iters)
        new_train = forced(None, lambda: state.__setitem__("model", train_bisecting_kmeans(mt, p, env)))
        old_train = forced("0", lambda: state.__setitem__("model_old", train_bisecting_kmeans(mt, p, env)))
        for _ in range(a.warmup):
            for fn in (new_it, old_it, new_descend):
                fn()
        new_train()
        old_train()
        model = MTable.from_rows(state["model"], SimpleModelDataConverter().getModelSchema(), replicated=True)

        def predict():
            op = BisectingKMeansPredictBatchOp().setPredictionCol("p").setReservedCols([])
            state["pred"] = op.linkFrom(TableSourceBatchOp(model), TableSourceBatchOp(mt)).getOutputTable()
        new_pred, old_pred = forced(None, predict), forced("0", predict)
        new_pred()
        old_pred()
        torch.cuda.synchronize()
        t_new, t_old = ab(new_it, old_it, a.reps)
        t_desc = [timed(new_descend) for _ in range(a.reps)]
        t_tn, t_to = ab(new_train, old_train, a.train_reps)
        t_pn, t_po = ab(new_pred, old_pred, a.train_reps)
        it_bytes = 2.0 * n * d * 8
        floor = it_bytes / LOAD_BPS * 1e3
        out = {"n": n, "d": d, "k": k, "dividing": m, "reps": a.reps,
               "iteration_new": stats(t_new), "iteration_torch": stats(t_old),
               "speedup_median": statistics.median(t_old) / statistics.median(t_new),
               "new_median_10pct_under_old_min": statistics.median(t_new) <= 0.9 * min(t_old),
               "iteration_bytes": it_bytes, "floor_ms": floor,
               "descend_alone": stats(t_desc), "descend_over_its_floor": statistics.median(t_desc) / (floor / 2),
               "train_new": stats(t_tn), "train_torch": stats(t_to), "train_iters": a.train_iters,
               "predict_new": stats(t_pn), "predict_torch": stats(t_po),
               "counts_equal": bool(torch.equal(state["new"][:, d], state["old"][:, d])),
               "max_abs_stats_diff": float((state["new"] - state["old"]).abs().max()),
               "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}
        print(json.dumps(out), flush=True)
        del X, state, new_rows, old_rows, mt, start
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    if a.csr:
        shape, nnz = a.csr.split("@")
        n, d, k = (int(v) for v in shape.split("x"))
        nnz, m = int(nnz), k // 2
        from alink_amd.models.common.features import FeatureMatrix
        g = torch.Generator(device=dev).manual_seed(a.seed)
        col = torch.randint(0, d, (n, nnz), device=dev, generator=g).sort(1).values     # a repeated column just adds
        fm = FeatureMatrix(crow=torch.arange(n + 1, device=dev) * nnz, col=col.reshape(-1),
                           val=torch.randn(n * nnz, dtype=torch.float64, device=dev, generator=g), ncols=d)
        R = rows(fm, "EUCLIDEAN")
        assert type(R) is _SparseRows
        table = round_table(m, d, a.seed, dev)
        start = torch.randint(0, m, (n,), device=dev, generator=g).to(torch.int32)
        state = {}
        it = iteration(R, table, start, m, state, "new")
        for _ in range(a.warmup):
            it()
        torch.cuda.synchronize()
        t = [timed(it) for _ in range(a.reps)]
        t_desc = [timed(lambda: R.descend(table, start.clone(), 1)) for _ in range(a.reps)]
        print(json.dumps({"csr": True, "n": n, "d": d, "k": k, "dividing": m, "entries_per_row": nnz,
                          "iteration_new": stats(t), "descend_alone": stats(t_desc),
                          "dense_matrix_GB": n * d * 8 / 1e9, "rows_counted": float(state["new"][:, d].sum()),
                          "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}), flush=True)


if __name__ == "__main__":
    main()
