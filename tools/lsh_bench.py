#!/usr/bin/env python3
"""LSH similarity join and top-N on one GPU: the device path (``ops/lsh.py``, ``ops/csrc/lsh.hip``) against the host
path it leaves in place (``profiles/lsh.txt``).

    python tools/lsh_bench.py                                   # every shape below
    python tools/lsh_bench.py --join 50000 --big 0 --dense "" --reps 5

Shapes, each after a warm-up of every path at that shape and timed with device events:

* ``--join n``: the JACCARD join operator on ``n x n`` near-duplicate documents of ``--entries`` entries over 2^18
  features (``n / 4`` base documents, 4 copies a side, 3 entries moved per copy), device path against
  ``ALINK_LSH_HIP=0`` alternating in one process, ``--reps`` / ``--host-reps`` samples; equal rows are checked;
* ``--big n``: the device path alone on ``n x n`` of the same documents, by stage;
* ``--dense n x d``: EUCLIDEAN top-N of the device path on dense noisy copies of ``n / 8`` centres, by stage;
* the EUCLIDEAN top-N on the ``--join`` documents as CSR rows (values scaled so that projections spread over
  buckets), by stage: the host path would densify ``[n, 2^18]``.  The EUCLIDEAN shapes take
  ``--euclid-projections`` projections per table: with 2, a bucket of width 2 collects a few per cent of all pairs.

Printed per shape as one JSON line: medians and minima, whether the device median is at least 10 % under the host
minimum, the MinHash kernel's time per (entry x hash function), the pair kernels' gathered bytes per second beside
the 5.5 TB/s random-row gather rate of the MI355X (context, not a pass mark), and the share of the device path spent
in the torch sorts of ``candidate_pairs`` and ``top_n``.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NCOLS = 2 ** 18
GATHER_BPS = 5.5e12


def timed(fn):
    """Milliseconds of one call of ``fn`` (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t)}


def documents(n, entries, seed, dev, scale=1.0):
    """(left, right) sparse ``FeatureMatrix`` of ``n`` documents each: ``n / 4`` base documents of ``entries``
    strictly ascending columns below 2^18 (gaps of at least 2), 4 copies a side, 3 entries of a copy moved by one."""
    from alink_amd.models.common.features import FeatureMatrix
    g = torch.Generator(device=dev).manual_seed(seed)
    nb = max(n // 4, 1)
    gap = max(2, NCOLS // entries - 1)
    base = torch.cumsum(torch.randint(2, gap + 1, (nb, entries), device=dev, generator=g), 1) - 2
    out = []
    for _ in range(2):
        col = base[torch.arange(n, device=dev) % nb].clone()
        pos = torch.randint(0, entries, (n, 3), device=dev, generator=g)
        col.scatter_(1, pos, col.gather(1, pos) + 1)        # the next column is free: gaps are at least 2
        val = (torch.randint(1, 9, (n * entries,), device=dev, generator=g).to(torch.float64) / 4.0) * scale
        out.append(FeatureMatrix(crow=torch.arange(n + 1, device=dev) * entries, col=col.reshape(-1), val=val,
                                 ncols=NCOLS))
    return out


def table(fm, first_id=0):
    from alink_amd.common.linalg import SparseBlock
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import Types
    ids = torch.arange(first_id, first_id + fm.nrows, dtype=torch.int64)
    vec = Column(fm.dense) if fm.dense is not None else Column(SparseBlock(fm.crow, fm.col, fm.val, fm.ncols))
    return MTable.from_columns(["id", "vec"], [Types.LONG, Types.VECTOR], [Column(ids), vec])


def join_op(lt, rt, a, state, key):
    from alink_amd import ApproxVectorSimilarityJoinLSHBatchOp, TableSourceBatchOp

    def run():
        op = ApproxVectorSimilarityJoinLSHBatchOp().setLeftIdCol("id").setRightIdCol("id").setLeftCol("vec") \
            .setRightCol("vec").setDistanceType("JACCARD").setDistanceThreshold(a.threshold) \
            .setNumProjectionsPerTable(a.projections).setNumHashTables(a.tables).setSeed(a.seed)
        state[key] = op.linkFrom(TableSourceBatchOp(lt), TableSourceBatchOp(rt)).getOutputTable()
    return run


def forced_host(fn):
    def run():
        os.environ["ALINK_LSH_HIP"] = "0"
        try:
            return fn()
        finally:
            os.environ.pop("ALINK_LSH_HIP", None)
    return run


def jaccard_stages(L, R, a, reps):
    """Stage times of the device JACCARD join on two sparse matrices."""
    from alink_amd.models.similarity.lsh import MinHashLSH
    from alink_amd.ops import lsh as K
    lsh = MinHashLSH(a.seed, a.projections, a.tables)
    s = {}

    def canon():
        s["A"], s["B"] = K.canonical_csr(L), K.canonical_csr(R)

    def hashes():
        s["ha"], s["hb"] = K.minhash_tables(s["A"], lsh.A, lsh.B), K.minhash_tables(s["B"], lsh.A, lsh.B)

    def cand():
        s["ai"], s["bi"] = K.candidate_pairs(s["ha"], s["hb"])

    def dist():
        s["d"] = K.pair_jaccard(s["A"], s["B"], s["ai"], s["bi"])
    stages = (("canonical_csr", canon), ("minhash", hashes), ("candidate_pairs", cand), ("pair_jaccard", dist))
    for _, fn in stages:
        fn()
    torch.cuda.synchronize()
    t = {name: [timed(fn) for _ in range(reps)] for name, fn in stages}
    entries = s["A"].nnz + s["B"].nnz
    m = int(s["ai"].numel())
    rows_bytes = float((s["A"].crow[s["ai"] + 1] - s["A"].crow[s["ai"]]).sum()
                       + (s["B"].crow[s["bi"] + 1] - s["B"].crow[s["bi"]]).sum()) * 8
    total = sum(statistics.median(v) for v in t.values())
    return {"stages": {k: stats(v) for k, v in t.items()}, "entries_hashed": entries, "candidates": m,
            "minhash_ns_per_entry_function": statistics.median(t["minhash"]) * 1e6
            / (entries * a.projections * a.tables),
            "pair_gather_TBps": rows_bytes / (statistics.median(t["pair_jaccard"]) * 1e-3) / 1e12,
            "gather_reference_TBps": GATHER_BPS / 1e12,
            "torch_sort_share": statistics.median(t["candidate_pairs"]) / total}


def euclid_stages(Q, D, a, reps, top_n):
    """Stage times of the device EUCLIDEAN top-N (queries ``Q``, dictionary ``D``), dense blocks or sparse."""
    import numpy as np
    from alink_amd.models.similarity.lsh import BucketRandomProjectionLSH
    from alink_amd.ops import lsh as K
    T, P, d = a.tables, a.euclid_projections, int(D.ncols)
    lsh = BucketRandomProjectionLSH(a.seed, d, P, T, a.width)
    Rt = torch.as_tensor(np.ascontiguousarray(lsh.R.reshape(T * P, d).T), device=Q.device)
    s = {}
    sparse = Q.is_sparse

    def canon():
        s["A"], s["B"] = (K.canonical_csr(Q), K.canonical_csr(D)) if sparse else (Q.dense, D.dense)

    def hashes():
        s["ha"] = K.brp_tables(Q.mm(Rt).contiguous(), lsh.r, lsh.width, T)
        s["hb"] = K.brp_tables(D.mm(Rt).contiguous(), lsh.r, lsh.width, T)

    def cand():
        s["ai"], s["bi"] = K.candidate_pairs(s["ha"], s["hb"])

    def dist():
        s["d"] = K.pair_euclidean(s["A"], s["B"], s["ai"], s["bi"])

    def top():
        s["top"] = K.top_n(s["ai"], s["bi"], s["d"], top_n)
    stages = (("rows", canon), ("project_and_hash", hashes), ("candidate_pairs", cand), ("pair_euclidean", dist),
              ("top_n", top))
    for _, fn in stages:
        fn()
    torch.cuda.synchronize()
    t = {name: [timed(fn) for _ in range(reps)] for name, fn in stages}
    m = int(s["ai"].numel())
    if sparse:
        A, B = s["A"], s["B"]
        rows_bytes = float((A.crow[s["ai"] + 1] - A.crow[s["ai"]]).sum()
                           + (B.crow[s["bi"] + 1] - B.crow[s["bi"]]).sum()) * 16
    else:
        rows_bytes = 2.0 * m * d * 8
    total = sum(statistics.median(v) for v in t.values())
    return {"stages": {k: stats(v) for k, v in t.items()}, "candidates": m, "kept": int(s["top"][0].numel()),
            "pair_gather_TBps": rows_bytes / (statistics.median(t["pair_euclidean"]) * 1e-3) / 1e12,
            "gather_reference_TBps": GATHER_BPS / 1e12,
            "torch_sort_share": (statistics.median(t["candidate_pairs"]) + statistics.median(t["top_n"])) / total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--join", type=int, default=200000, help="documents a side of the shared JACCARD join, or 0")
    ap.add_argument("--big", type=int, default=10000000, help="documents a side of the device-only join, or 0")
    ap.add_argument("--dense", default="1000000x128", help="n x d of the dense EUCLIDEAN top-N, or empty")
    ap.add_argument("--entries", type=int, default=100)
    ap.add_argument("--tables", type=int, default=4)
    ap.add_argument("--projections", type=int, default=2)
    ap.add_argument("--euclid-projections", type=int, default=4, help="projections per table of the EUCLIDEAN shapes")
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--width", type=float, default=2.0)
    ap.add_argument("--top-n", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd import useLocalEnv
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import _lib
    _lib.require()
    dev = torch.device("cuda:0")
    useLocalEnv(1, device="cuda:0")
    os.environ.pop("ALINK_LSH_HIP", None)

    if a.join:
        L, R = documents(a.join, a.entries, a.seed, dev)
        lt, rt = table(L), table(R, a.join)
        state = {}
        new, old = join_op(lt, rt, a, state, "new"), forced_host(join_op(lt, rt, a, state, "old"))
        new()
        old()                                   # the warm-up of the host path is a whole run
        torch.cuda.synchronize()
        t_new, t_old = [], []
        for i in range(max(a.reps, a.host_reps)):       # alternating while both have samples left
            if i < a.reps:
                t_new.append(timed(new))
            if i < a.host_reps:
                t_old.append(timed(old))
        same = state["new"].num_rows == state["old"].num_rows and all(
            torch.equal(x.values, y.values) for x, y in zip(state["new"].cols, state["old"].cols))
        out = {"shape": "jaccard_join", "n": a.join, "entries": a.entries, "tables": a.tables,
               "projections": a.projections, "device": stats(t_new), "host": stats(t_old),
               "speedup_median": statistics.median(t_old) / statistics.median(t_new),
               "device_median_10pct_under_host_min": statistics.median(t_new) <= 0.9 * min(t_old),
               "rows_out": state["new"].num_rows, "rows_equal": bool(same)}
        out.update(jaccard_stages(L, R, a, a.reps))
        print(json.dumps(out), flush=True)
        # the same documents as CSR rows under EUCLIDEAN top-N, values scaled for buckets of --width
        scale = 256.0
        Ls = FeatureMatrix(crow=L.crow, col=L.col, val=L.val * scale, ncols=NCOLS)
        Rs = FeatureMatrix(crow=R.crow, col=R.col, val=R.val * scale, ncols=NCOLS)
        out = {"shape": "euclidean_topn_csr", "n": a.join, "entries": a.entries, "value_scale": scale,
               "tables": a.tables, "projections": a.euclid_projections, "width": a.width, "top_n": a.top_n,
               "dense_matrix_GB": a.join * NCOLS * 8 / 1e9}
        out.update(euclid_stages(Rs, Ls, a, a.reps, a.top_n))
        out["peak_mem_GB"] = torch.cuda.max_memory_allocated() / 1e9
        print(json.dumps(out), flush=True)
        del L, R, Ls, Rs, lt, rt, state
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    if a.dense:
        n, d = (int(v) for v in a.dense.split("x"))
        g = torch.Generator(device=dev).manual_seed(a.seed)
        centres = torch.randn((max(n // 8, 1), d), dtype=torch.float64, device=dev, generator=g) * 40.0
        rows = [centres[torch.arange(n, device=dev) % centres.shape[0]]
                + 0.05 * torch.randn((n, d), dtype=torch.float64, device=dev, generator=g) for _ in range(2)]
        out = {"shape": "euclidean_topn_dense", "n": n, "d": d, "tables": a.tables,
               "projections": a.euclid_projections, "width": a.width, "top_n": a.top_n}
        out.update(euclid_stages(FeatureMatrix(rows[1]), FeatureMatrix(rows[0]), a, a.reps, a.top_n))
        out["peak_mem_GB"] = torch.cuda.max_memory_allocated() / 1e9
        print(json.dumps(out), flush=True)
        del rows, centres
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    if a.big:
        L, R = documents(a.big, a.entries, a.seed, dev)
        out = {"shape": "jaccard_join_device_only", "n": a.big, "entries": a.entries, "tables": a.tables,
               "projections": a.projections}
        out.update(jaccard_stages(L, R, a, max(2, a.reps // 3)))
        out["total_median_ms"] = sum(v["median_ms"] for v in out["stages"].values())
        out["peak_mem_GB"] = torch.cuda.max_memory_allocated() / 1e9
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
