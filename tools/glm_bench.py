#!/usr/bin/env python3
"""GLM on one GPU: the fused IRLS statistics pass, a whole ``train_glm`` and the predict mapper (``ops/glm.py``,
``csrc/glm.hip``) against the path they replace, ``ALINK_GLM_HIP=0`` (``profiles/glm.txt``).

    python tools/glm_bench.py                            # the three shapes, the predict operator and the sweep
    python tools/glm_bench.py --shapes 1000000x32:poisson:log --reps 5 --predict "" --sweep ""

Per shape ``n x k : family : link`` (fp64 rows on the device, y drawn from the family around a known model) it times,
after a warm-up of both paths at that shape, the two paths alternated in the same process:

* one IRLS statistics pass (mode STEP) with device events: ``irls_stats`` against the former calls of ``_irls``
  (the GEMV, the elementwise chain, ``_weight_stats``'s two ``[n, k+2]`` copies and ``tn_matmul``);
* ``glm_summary``'s row pass (``rows`` for ``pred`` and the four ordered sums, both reduction levels), new path only;
* one whole ``train_glm`` (``--iters`` iterations at most) on the host clock, ending in a device synchronise.

Printed per shape: medians and minima, the bytes of one pass over X, y, w and off and their time at the 6.12 TB/s
load-only rate README records, how far the fused pass sits from that floor, and the largest relative difference of
the statistics and of the trained coefficients between the two paths.

``--predict n x k``: ``GlmPredictBatchOp`` on a device table, new against ``ALINK_GLM_HIP=0``, host clock.
``--sweep``: the statistics pass at k = 32 and k = 126 over small n, host clock around a synchronised call: the
largest n at which the former path still wins sets ``GLM_MIN_ROWS``.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "10000000x32:poisson:log,20000000x8:binomial:logit,2000000x126:gamma:inverse"
PREDICT = "10000000x32"
SWEEP = "64,1000,10000,30000,100000,300000,1000000"
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


def alternate(new, old, reps, old_reps, clock):
    t_new, t_old = [], []
    for i in range(reps):
        t_new.append(clock(new))
        if i < old_reps:
            t_old.append(clock(old))
    return t_new, t_old


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def draw(n, k, fam, dev, seed):
    """(X, y, w, off, beta, b0): X uniform in [0.1, 1], a model whose mean stays in (0.2, 0.8), y from the family."""
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.rand((n, k), dtype=torch.float64, device=dev, generator=g) * 0.9 + 0.1
    beta = torch.full((k,), 0.45 / k, dtype=torch.float64, device=dev)
    b0 = {"poisson": -1.5, "binomial": -0.3, "gamma": 1.5}[fam]
    eta = X @ beta + b0
    mu = {"poisson": torch.exp, "binomial": torch.sigmoid, "gamma": torch.reciprocal}[fam](eta)
    u = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
    if fam == "poisson":
        y = torch.poisson(mu, generator=g)
    elif fam == "binomial":
        y = (u < mu).double()
    else:
        y = mu * (0.5 + u)
    w = torch.rand(n, dtype=torch.float64, device=dev, generator=g) + 0.5
    return X, y, w, torch.zeros(n, dtype=torch.float64, device=dev), beta, b0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x k : family : link")
    ap.add_argument("--predict", default=PREDICT, help="n x k of the predict operator, or empty")
    ap.add_argument("--sweep", default=SWEEP, help="comma-separated n of the small-n sweep, or empty")
    ap.add_argument("--sweep-k", default="32,126", help="comma-separated k of the sweep")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd import useLocalEnv
    from alink_amd.common.params import Params
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    from alink_amd.models.regression import glm as M
    from alink_amd.ops import _lib, glm as G
    from alink_amd.ops.gemm import tn_matmul
    _lib.require()
    dev = torch.device("cuda:0")
    useLocalEnv(1, device="cuda:0")

    def flagged(flag, fn):
        def go():
            os.environ["ALINK_GLM_HIP"] = flag
            try:
                return fn()
            finally:
                os.environ.pop("ALINK_GLM_HIP", None)
        return go

    def passes(X, y, w, off, beta, b0, fl, state):
        model = M.WlsModel(beta.cpu().numpy(), b0, [], True, 0)
        d = M.GlmData(X, y, w, off)

        def new():
            state["new"] = G.irls_stats(X, y, w, off, beta, b0, *M._kernel_args(fl), G.STEP)

        def old():          # the body of _irls's loop under ALINK_GLM_HIP=0, without the all-reduce and the solve
            eta = X @ beta + model.intercept + off
            mu = fl.fitted(eta)
            deriv = fl.link.derivative(mu)
            z = eta - off + (y - mu) * deriv
            ww = w / (deriv * deriv * fl.family.variance(mu))
            Z = torch.cat([X, torch.ones_like(z)[:, None], z[:, None]], 1)
            state["old"] = (tn_matmul(Z, Z * ww[:, None]), (ww * ww).sum())
        return d, new, old

    for shape in [s for s in a.shapes.split(",") if s]:
        size, fam, link = shape.split(":")
        n, k = (int(v) for v in size.split("x"))
        X, y, w, off, beta, b0 = draw(n, k, fam, dev, a.seed)
        fl = M.FamilyLink(fam, 0.0, link, 1.0)
        assert G.supported(X, fam, link)
        state = {}
        d, new, old = passes(X, y, w, off, beta, b0, fl, state)
        new()
        old()
        t_new, t_old = alternate(new, old, a.reps, a.old_reps, timed)
        diff = {"G": rel(state["new"][1], state["old"][0]), "wwsum": rel(state["new"][0], state["old"][1])}
        state.clear()
        p = Params().set("family", fam).set("link", link).set("regParam", 0.0).set("fitIntercept", True) \
            .set("maxIter", a.iters).set("epsilon", 1e-12)
        fit = {}

        def train(flag):
            def go():
                fit[flag] = M.train_glm(d, p)
            return flagged(flag, go)
        train("1")()
        train("0")()
        f_new, f_old = alternate(train("1"), train("0"), a.reps, a.old_reps, wall)
        diff["coefficients"] = float(abs(fit["1"].coefficients - fit["0"].coefficients).max()
                                     / abs(fit["0"].coefficients).max())

        def summary_pass():         # glm_summary's row pass: pred and the four ordered sums
            G.rows(X, y, w, off, beta, b0, *M._kernel_args(fl), ("pred", "sums"))
        summary_pass()
        t_rows = [timed(summary_pass) for _ in range(a.reps)]
        pass_bytes = 8 * n * (k + 3)
        floor_ms = pass_bytes / LOAD_BPS * 1e3
        print(json.dumps({"n": n, "k": k, "family": fam, "link": link, "pass_new": stats(t_new),
                          "pass_old": stats(t_old),
                          "pass_speedup_median": statistics.median(t_old) / statistics.median(t_new),
                          "summary_row_pass": stats(t_rows),
                          "train_new": stats(f_new), "train_old": stats(f_old),
                          "train_speedup_median": statistics.median(f_old) / statistics.median(f_new),
                          "one_pass_bytes": pass_bytes, "one_pass_ms": floor_ms,
                          "over_floor": statistics.median(t_new) / floor_ms, "chunk_rows": G.glm_chunk_rows(n, k),
                          "max_rel_diff": diff, "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}), flush=True)
        del X, y, w, off, d, new, old
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    if a.sweep:
        fl = M.FamilyLink("poisson", 0.0, "log", 1.0)
        for k in [int(v) for v in a.sweep_k.split(",")]:
            for n in [int(v) for v in a.sweep.split(",")]:
                state = {}
                _, new, old = passes(*draw(n, k, "poisson", dev, a.seed), fl, state)
                for _ in range(3):
                    new()
                    old()
                t_new, t_old = alternate(new, old, 4 * a.reps, 4 * a.reps, wall)
                print(json.dumps({"sweep": True, "n": n, "k": k, "pass_new": stats(t_new), "pass_old": stats(t_old),
                                  "former_path_wins": statistics.median(t_old) < statistics.median(t_new)}),
                      flush=True)

    if a.predict:
        from alink_amd import GlmPredictBatchOp, GlmTrainBatchOp
        from alink_amd.operator.batch.source import TableSourceBatchOp
        n, k = (int(v) for v in a.predict.split("x"))
        X, y, _, _, _, _ = draw(n, k, "poisson", dev, a.seed)
        names = ["f%d" % j for j in range(k)]
        schema = TableSchema(names + ["y"], [Types.DOUBLE] * (k + 1))

        def table(rows):
            return TableSourceBatchOp(MTable(schema, [Column(X[:rows, j].contiguous()) for j in range(k)]
                                             + [Column(y[:rows].contiguous())]))
        model = GlmTrainBatchOp().setFamily("poisson").setFeatureCols(names).setLabelCol("y").setMaxIter(3) \
            .linkFrom(table(200000))
        src = table(n)
        out = {}

        def run(flag):
            def go():
                out[flag] = GlmPredictBatchOp().setPredictionCol("p").linkFrom(model, src).getOutputTable() \
                    .col("p").values
            return flagged(flag, go)
        run("1")()
        run("0")()
        t_new, t_old = alternate(run("1"), run("0"), a.reps, a.old_reps, wall)
        print(json.dumps({"predict": True, "n": n, "k": k, "operator_new": stats(t_new), "operator_old": stats(t_old),
                          "rows_per_s_new": n / (statistics.median(t_new) * 1e-3),
                          "rows_per_s_old": n / (statistics.median(t_old) * 1e-3),
                          "max_rel_diff": rel(torch.as_tensor(out["1"]).cpu(), torch.as_tensor(out["0"]).cpu())}),
              flush=True)


if __name__ == "__main__":
    main()
