#!/usr/bin/env python3
"""Chi-square tests on one GPU: the device path of the four chi-square operators (``ops/chisq.py``,
``ops/csrc/chisq.hip``, ``models/statistics/chisq.py``) by stage, the counts kernel by variant, and the host path it
leaves in place (``profiles/chisq.txt``).

    python tools/chisq_bench.py                                 # every part below, written to profiles/chisq.txt
    python tools/chisq_bench.py --rows 1000000 --host-rows 0 --cross "" --out /tmp/chisq.txt

Shapes (``--rows`` rows each):

* ``csr_counts``: documents of ``--draws`` Zipf draws over ``--features`` hashed features as CSR counts, 20 labels;
* ``csr_tfidf``: the same rows with tf-idf values scaled per document, so nearly every value of a column is distinct;
* ``dense``: ``--dense-cols`` dense fp64 columns with 16 distinct values each;
* ``table``: 8 integer table columns.

Per shape: ``chi_square_arrays`` by stage (coding and sorts, counts kernel, column sums, statistic kernel, p-values)
after one warm-up at a hundredth of the rows, and end to end through the operator.  For the two kernels: entries (or
cells) per second and the bytes they move per second beside 6.3 TB/s (HBM, streamed) of the MI355X -- context, not
a pass mark.  The counts kernel runs with both variants (LDS histogram / per-entry global atomics) on the skewed
``csr_counts`` stream and on the nearly all-distinct ``csr_tfidf`` stream.  ``--host-rows``: the host path against the
device path on a slice of the table shape and (``--host-docs``) of the CSR shape, in this process: seconds, equal df
and the largest relative difference in value.  ``--cross``: both paths at each of these row counts of the table shape,
for the crossover ``CHISQ_MIN_CELLS``.

One JSON line per part.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BPS = 6.3e12
BACKEND = None
LABELS = 20


def csr_rows(n, features, draws, seed, dev, chunk=1000000):
    """``(crow, col int32, count float64)`` of ``n`` documents of ``draws`` Zipf(1) draws over ``features`` hashed
    features (a random permutation of the ranks), generated ``chunk`` documents at a time."""
    g = torch.Generator(device=dev).manual_seed(seed)
    w = 1.0 / torch.arange(1, features + 1, device=dev, dtype=torch.float64)
    cdf = torch.cumsum(w / w.sum(), 0)
    perm = torch.randperm(features, device=dev, generator=g)
    lens, cols, vals = [], [], []
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        ids = torch.searchsorted(cdf, torch.rand((m, draws), device=dev, generator=g, dtype=torch.float64))
        ids = perm[ids.clamp(max=features - 1)]
        key = (torch.arange(m, device=dev)[:, None] * features + ids).reshape(-1)
        key, cnt = torch.unique(key, return_counts=True)
        doc = torch.div(key, features, rounding_mode="floor")
        lens.append(torch.bincount(doc, minlength=m))
        cols.append((key - doc * features).to(torch.int32))
        vals.append(cnt.to(torch.float64))
        del ids, key, cnt, doc
    crow = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.cat(lens), 0, out=crow[1:])
    return crow, torch.cat(cols), torch.cat(vals)


def vector_table(crow, col, val, features, label):
    from alink_amd.common.linalg import SparseBlock
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import Types
    return MTable.from_columns(["vec", "label"], [Types.SPARSE_VECTOR, Types.LONG],
                               [Column(SparseBlock(crow, col, val, features)), Column(label)])


def dense_table(X, label):
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import Types
    return MTable.from_columns(["vec", "label"], [Types.DENSE_VECTOR, Types.LONG], [Column(X), Column(label)])


def int_table(n, cols, seed, dev):
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import Types
    g = torch.Generator(device=dev).manual_seed(seed)
    label = torch.randint(0, LABELS, (n,), device=dev, generator=g)
    vals = [Column((torch.randint(0, 32, (n,), device=dev, generator=g) + (label % (j + 1))) % 32) for j in range(cols)]
    names = ["c%d" % j for j in range(cols)]
    return MTable.from_columns(names + ["label"], [Types.LONG] * (cols + 1), vals + [Column(label)]), names


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def stages(mt, cols, vec, dev, warm):
    """Seconds per stage of ``chi_square_arrays`` on ``mt`` (``warm``: a smaller table run first), and its result."""
    from alink_amd.models.statistics import chisq as CQ
    if warm is not None:
        CQ.chi_square_arrays(warm, cols, vec, "label", BACKEND, dev)
    stats = {}
    sync(dev)
    t0 = time.perf_counter()
    got = CQ.chi_square_arrays(mt, cols, vec, "label", BACKEND, dev, stats=stats)
    sync(dev)
    stats["total"] = time.perf_counter() - t0
    return stats, got


def kernel_rates(stats, L):
    """Entries per second and bytes per second of the two kernels from a run's stage seconds."""
    out = {}
    if stats.get("counts"):
        out["counts_entries_per_s"] = stats["entries"] / stats["counts"]
        out["counts_read_bytes_per_s"] = 8 * stats["entries"] / stats["counts"]        # g and lab, int32 each
        out["counts_of_hbm"] = out["counts_read_bytes_per_s"] / HBM_BPS
    if stats.get("stat"):
        out["stat_cells_per_s"] = stats["categories"] * L / stats["stat"]
        out["stat_read_bytes_per_s"] = 8 * stats["categories"] * L / stats["stat"]     # cnt int64
        out["stat_of_hbm"] = out["stat_read_bytes_per_s"] / HBM_BPS
    return out


def operator_seconds(mt, cols, vec, flag):
    from alink_amd import (ChiSquareTestBatchOp, TableSourceBatchOp, VectorChiSquareTestBatchOp)
    os.environ["ALINK_CHISQ_HIP"] = flag
    op = VectorChiSquareTestBatchOp().setSelectedCol(vec) if vec else ChiSquareTestBatchOp().setSelectedCols(cols)
    op.setLabelCol("label")
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    op.linkFrom(TableSourceBatchOp(mt))
    rows = op.getOutputTable().num_rows
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return time.perf_counter() - t0, op, rows


def compare(dev_op, host_op):
    a = {r.colName: r for r in dev_op.collectChiSquareTest()}
    worst, same_df = 0.0, True
    for r in host_op.collectChiSquareTest():
        d = a[r.colName]
        same_df = same_df and d.df == r.df
        if r.value:
            worst = max(worst, abs(d.value - r.value) / r.value)
    return same_df, worst


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000000)
    ap.add_argument("--features", type=int, default=2 ** 18)
    ap.add_argument("--draws", type=int, default=100)
    ap.add_argument("--dense-cols", type=int, default=128)
    ap.add_argument("--host-rows", type=int, default=10000000)
    ap.add_argument("--host-docs", type=int, default=100)
    ap.add_argument("--cross", default="100,200,300,400,500,700,1000,3000")
    ap.add_argument("--parts", default="csr,dense,table")
    ap.add_argument("--out", default=os.path.join("profiles", "chisq.txt"))
    ap.add_argument("--device", default="cuda:0", help="cpu: a dry run of this script through the torch twins")
    a = ap.parse_args(argv)
    from alink_amd import useLocalEnv
    from alink_amd.ops import _lib
    from alink_amd.ops import chisq as Q
    dev = torch.device(a.device)
    global BACKEND
    if dev.type == "cuda":
        _lib.require()
        BACKEND = Q.DEVICE
    else:
        BACKEND = Q.TWIN
    useLocalEnv(1, device=a.device)
    lines = []

    def emit(part, **kw):
        line = json.dumps(dict(part=part, **kw), default=float)
        print(line, flush=True)
        lines.append(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    emit("setup", rows=a.rows, features=a.features, draws=a.draws, dense_cols=a.dense_cols, host_rows=a.host_rows,
         host_docs=a.host_docs, cross=a.cross, parts=a.parts, labels=LABELS,
         device=torch.cuda.get_device_name(0) if dev.type == "cuda" else "cpu", budget_bytes=Q.CHISQ_BUDGET_BYTES,
         min_cells=Q.CHISQ_MIN_CELLS)
    parts = a.parts.split(",")
    g = torch.Generator(device=dev).manual_seed(1)
    if "csr" in parts:
        n = a.rows
        t0 = time.perf_counter()
        crow, col, val = csr_rows(n, a.features, a.draws, 5, dev)
        label = torch.randint(0, LABELS, (n,), device=dev, generator=g)
        sync(dev)
        emit("csr_generated", rows=n, nnz=int(col.numel()), seconds=time.perf_counter() - t0)
        wn = max(n // 100, 1000)
        wa = int(crow[wn])
        for name in ("csr_counts", "csr_tfidf"):
            if name == "csr_tfidf":
                df = torch.bincount(col.to(torch.int64), minlength=a.features).to(torch.float64)
                scale = torch.rand(n, device=dev, generator=g, dtype=torch.float64) + 0.5
                rows_of = torch.repeat_interleave(torch.arange(n, device=dev), crow[1:] - crow[:-1])
                val = val * torch.log((n + 1.0) / (df + 1.0))[col.to(torch.int64)] * scale[rows_of]
                del rows_of, df, scale
            mt = vector_table(crow, col, val, a.features, label)
            warm = vector_table(crow[:wn + 1].clone(), col[:wa], val[:wa], a.features, label[:wn])
            for variant in (0, 1):
                Q.CHISQ_VARIANT = variant
                stats, _ = stages(mt, None, "vec", dev, warm)
                emit(name + "_stages", variant=variant, **stats, **kernel_rates(stats, LABELS))
            Q.CHISQ_VARIANT = 0
            secs, _, rows = operator_seconds(mt, None, "vec", "1")
            emit(name + "_operator", seconds=secs, output_rows=rows)
        if a.host_docs:
            hn = a.host_docs
            ha = int(crow[hn])
            small = vector_table(crow[:hn + 1].clone(), col[:ha], val[:ha], a.features, label[:hn])
            ds, dop, _ = operator_seconds(small, None, "vec", "1")
            hs, hop, _ = operator_seconds(small, None, "vec", "0")
            same, worst = compare(dop, hop)
            emit("csr_host_slice", docs=hn, host_seconds=hs, device_seconds=ds, equal_df=same, worst_rel_value=worst)
        del crow, col, val, mt, warm
        if dev.type == "cuda":
            torch.cuda.empty_cache()
    if "dense" in parts:
        n = a.rows
        X = torch.randint(0, 16, (n, a.dense_cols), device=dev, generator=g).to(torch.float64) * 0.25
        label = torch.randint(0, LABELS, (n,), device=dev, generator=g)
        wn = max(n // 100, 1000)
        stats, _ = stages(dense_table(X, label), None, "vec", dev, dense_table(X[:wn], label[:wn]))
        emit("dense_stages", **stats, **kernel_rates(stats, LABELS))
        secs, _, rows = operator_seconds(dense_table(X, label), None, "vec", "1")
        emit("dense_operator", seconds=secs, output_rows=rows)
        del X
        if dev.type == "cuda":
            torch.cuda.empty_cache()
    if "table" in parts:
        mt, names = int_table(a.rows, 8, 9, dev)
        warm, _ = int_table(max(a.rows // 100, 1000), 8, 9, dev)
        stats, _ = stages(mt, names, None, dev, warm)
        emit("table_stages", **stats, **kernel_rates(stats, LABELS))
        secs, _, rows = operator_seconds(mt, names, None, "1")
        emit("table_operator", seconds=secs, output_rows=rows)
        if a.host_rows:
            small = mt.slice(0, a.host_rows)
            ds, dop, _ = operator_seconds(small, names, None, "1")
            hs, hop, _ = operator_seconds(small, names, None, "0")
            same, worst = compare(dop, hop)
            emit("table_host_slice", rows=a.host_rows, host_seconds=hs, device_seconds=ds, equal_df=same,
                 worst_rel_value=worst)
        for r in [int(x) for x in a.cross.split(",") if x]:
            small = mt.slice(0, r)
            operator_seconds(small, names, None, "1")
            ds = min(operator_seconds(small, names, None, "1")[0] for _ in range(3))
            hs = min(operator_seconds(small, names, None, "0")[0] for _ in range(3))
            emit("cross", rows=r, cells=8 * r, host_ms=hs * 1e3, device_ms=ds * 1e3)
    os.environ.pop("ALINK_CHISQ_HIP", None)


if __name__ == "__main__":
    main(sys.argv[1:])
