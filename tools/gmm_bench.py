#!/usr/bin/env python3
"""GMM on one GPU: the fused EM step and the device posterior (``ops/gmm.py``, ``csrc/gmm_em.hip``) against the path
they replace, ``ALINK_GMM_HIP=0`` (``profiles/gmm.txt``).

    python tools/gmm_bench.py                            # the four shapes and the predict operator
    python tools/gmm_bench.py --shapes 1000000x32x10 --reps 5 --predict ""

Per shape ``n x d x k`` (fp64 rows on the device, a mixture of k blobs, parameters near the blobs) it times, after a
warm-up of both paths at that shape, one EM step's statistics with device events, the two paths alternated in the
same process:

* new: ``em_step`` on the centred rows (the E pass and the M pass);
* old: the calls of ``train_gmm``'s loop under ``ALINK_GMM_HIP=0``: ``estep`` (one GEMM into ``[n, k d]`` chunks and
  the epilogue kernel; a Python loop over the components above k = 64), ``R.sum(0)``, ``R^T X`` and
  ``_weighted_syrk``;
* the E pass and the M pass alone.

Printed per shape: medians and minima; the bytes of one pass over the rows and ``R`` and their time at the 6.12 TB/s
load-only rate README records; the flops of each pass (E: ``2 n k d^2``, M: ``n k d (d + 1)``, the upper triangle)
over the 6e13 flop/s of ``profiles/kmeans_dense64.txt``; how far each pass sits from the larger of its two floors;
and the largest difference of the updated parameters (w, mu, Sigma, each relative to the array's largest magnitude)
and of the log-likelihood between the two paths.

``--predict n x d x k``: ``GmmPredictBatchOp`` (prediction column only) on the device table, new against
``ALINK_GMM_HIP=0``, host clock around a call that ends in a device synchronise.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "10000000x32x10,2000000x128x16,20000000x8x5,4000000x16x100"
PREDICT = "10000000x32x10"
LOAD_BPS = 25.6e9 / 4.18e-3         # README: the bf16 KMeans kernel's load-only pass over 1e8 x 128 bf16
FLOPS = 6e13                        # profiles/kmeans_dense64.txt: the fp64 matrix cores on this loop shape


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


def blobs(n, d, k, dev, seed):
    """(X [n, d], mu [k, d], Sigma [k, d, d], w [k]): k blobs of unit noise around centres from 2 N(0, 1), and
    parameters near them."""
    g = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.randn((k, d), dtype=torch.float64, device=dev, generator=g) * 2.0
    X = torch.randn((n, d), dtype=torch.float64, device=dev, generator=g)
    X += centres[torch.randint(0, k, (n,), device=dev, generator=g)]
    mu = centres + 0.1 * torch.randn((k, d), dtype=torch.float64, device=dev, generator=g)
    A = torch.randn((k, d, d), dtype=torch.float64, device=dev, generator=g)
    S = A @ A.transpose(1, 2) / (4 * d) + torch.eye(d, dtype=torch.float64, device=dev)
    w = torch.full((k,), 1.0 / k, dtype=torch.float64, device=dev)
    return X, mu, S, w


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x d x k")
    ap.add_argument("--predict", default=PREDICT, help="n x d x k of the predict operator, or empty")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd import useLocalEnv
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    from alink_amd.models.clustering.gmm import _root_inv, _weighted_syrk
    from alink_amd.ops import _lib, gmm as G
    from alink_amd.ops.gemm import tn_matmul
    _lib.require()
    dev = torch.device("cuda:0")
    useLocalEnv(1, device="cuda:0")

    for shape in [s for s in a.shapes.split(",") if s]:
        n, d, k = (int(v) for v in shape.split("x"))
        X, mu, S, w = blobs(n, d, k, dev, a.seed)
        xbar = X.mean(0)
        X0 = X - xbar
        mu0 = mu - xbar
        W, logdet, rank = _root_inv(S)
        logw = torch.log(w)
        assert G.em_selected(X0, k)
        state = {}

        def new_step():
            state["new"] = G.em_step(X0, mu0, W, logdet, rank, logw)

        def old_step():
            R, ll = G.estep(X0, mu0, W, logdet, rank, logw)
            state["old"] = (R.sum(0), tn_matmul(R, X), _weighted_syrk(R, X), ll)
            del R

        def e_pass():
            state["R"] = G._em_rows(X0, mu0, W, logdet, rank, logw, True, False, 0)[0]

        def m_pass():
            G._em_moments(X0, state["R"], 0, 0)
        for _ in range(a.warmup):
            new_step()
            old_step()
        t_new, t_old = [], []
        for i in range(a.reps):
            t_new.append(timed(new_step))
            if i < a.old_reps:
                t_old.append(timed(old_step))
        peak = torch.cuda.max_memory_allocated() / 1e9
        # the update of either path
        rs, xs, xxs, ll, _ = state["new"]
        m0 = xs / rs[:, None]
        new_par = (rs / n, xbar + m0, xxs / rs[:, None, None] - m0[:, :, None] * m0[:, None, :])
        rs_o, xs_o, xxs_o, ll_o = state["old"]
        m_o = xs_o / rs_o[:, None]
        old_par = (rs_o / n, m_o, xxs_o / rs_o[:, None, None] - m_o[:, :, None] * m_o[:, None, :])
        diff = {"w": rel(new_par[0], old_par[0]), "mu": rel(new_par[1], old_par[1]),
                "Sigma": rel(new_par[2], old_par[2]), "ll": abs(float(ll) - float(ll_o)) / abs(float(ll_o))}
        state.clear()
        alone = {}
        for name, fn in (("E", e_pass), ("M", m_pass)):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            alone[name] = stats([timed(fn) for _ in range(a.reps)])
        pass_bytes = n * d * 8 + n * k * 8
        pass_ms = pass_bytes / LOAD_BPS * 1e3
        flops = {"E": 2.0 * n * k * d * d, "M": 1.0 * n * k * d * (d + 1)}
        floors = {p: max(pass_ms, flops[p] / FLOPS * 1e3) for p in flops}
        print(json.dumps({"n": n, "d": d, "k": k, "step_new": stats(t_new), "step_old": stats(t_old),
                          "speedup_median": statistics.median(t_old) / statistics.median(t_new),
                          "new_median_below_old_min": statistics.median(t_new) < min(t_old),
                          "passes": alone, "one_pass_bytes": pass_bytes, "one_pass_ms": pass_ms,
                          "flop_ms": {p: flops[p] / FLOPS * 1e3 for p in flops},
                          "over_floor": {p: alone[p]["median_ms"] / floors[p] for p in flops},
                          "chunk_rows": G.em_chunk_rows(n, k, d), "max_rel_diff": diff, "peak_mem_GB": peak}),
              flush=True)
        del X, X0, state
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    if a.predict:
        from alink_amd import GmmPredictBatchOp, GmmTrainBatchOp
        from alink_amd.operator.batch.source import TableSourceBatchOp
        n, d, k = (int(v) for v in a.predict.split("x"))
        X, _, _, _ = blobs(n, d, k, dev, a.seed)
        schema = TableSchema(["v"], [Types.DENSE_VECTOR])
        head = TableSourceBatchOp(MTable(schema, [Column(X[:200000].clone())]))
        model = GmmTrainBatchOp().setVectorCol("v").setK(k).setMaxIter(3).linkFrom(head)
        src = TableSourceBatchOp(MTable(schema, [Column(X)]))
        state = {}

        def run(flag):
            def go():
                if flag is None:
                    os.environ.pop("ALINK_GMM_HIP", None)
                else:
                    os.environ["ALINK_GMM_HIP"] = flag
                try:
                    out = GmmPredictBatchOp().setPredictionCol("p").linkFrom(model, src).getOutputTable()
                    state[flag] = out.col("p").values
                finally:
                    os.environ.pop("ALINK_GMM_HIP", None)
            return go
        new_op, old_op = run(None), run("0")
        for _ in range(a.warmup):
            new_op()
            old_op()
        t_new, t_old = [], []
        for i in range(a.reps):
            t_new.append(wall(new_op))
            if i < a.old_reps:
                t_old.append(wall(old_op))
        same = None
        if isinstance(state.get(None), torch.Tensor) and isinstance(state.get("0"), torch.Tensor):
            same = float((state[None].cpu() == state["0"].cpu()).double().mean())
        print(json.dumps({"predict": True, "n": n, "d": d, "k": k, "operator_new": stats(t_new),
                          "operator_old": stats(t_old),
                          "rows_per_s_new": n / (statistics.median(t_new) * 1e-3),
                          "rows_per_s_old": n / (statistics.median(t_old) * 1e-3),
                          "equal_predictions_share": same}), flush=True)


if __name__ == "__main__":
    main()
