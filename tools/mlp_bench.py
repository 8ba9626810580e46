#!/usr/bin/env python3
"""The multilayer perceptron on one GPU: the fused gradient, line-search and predict passes (``ops/mlp_fused.py``,
``csrc/mlp_fused.hip``) against the paths they replace (``profiles/mlp_fused.txt``).

    python tools/mlp_bench.py                            # the three shapes and the sweep
    python tools/mlp_bench.py --shapes 1000000x32:16:10 --reps 5 --sweep ""

Per shape ``n x d0 : h.. : C`` (fp64 rows on the device) it times, after a warm-up of both paths at that shape, the two
paths alternated in the same process with device events, medians of ``--reps``:

* the gradient: ``fused_grad`` against ``ops/mlp.mlp_grad`` (library GEMMs and the epilogue kernels);
* the line search of 4 steps: ``search_losses`` against the former ``calc_search_values`` (one torch forward per step);
* predict: ``rows`` for P and the label on the device against the former mapper's forward on the host (the copy of X
  to the host included: the former mapper extracts the features there), host clock around a synchronised call.

``--sweep``: gradient and search at the same networks over small n, host clock around a synchronised call: the
smallest n from which the fused path wins both at every shape sets ``MLP_MIN_ROWS``.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "10000000x32:16:10,2000000x128:64:10,20000000x8:5:3"
SWEEP = "64,256,1024,4096,16384,65536,262144"
NSTEPS = 4


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


def passes(n, layers, dev, seed):
    """The six closures (gradient, search and predict, new and former path) on drawn data, and their results."""
    from alink_amd.models.classification.mlp import mlp_forward, weight_size
    from alink_amd.ops import mlp as M, mlp_fused as F
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn((n, layers[0]), dtype=torch.float64, device=dev, generator=g)
    coef = torch.randn(weight_size(layers), dtype=torch.float64, device=dev, generator=g) * 0.5
    dirv = torch.randn(weight_size(layers), dtype=torch.float64, device=dev, generator=g) * 0.1
    y = torch.randint(0, layers[-1], (n,), device=dev, generator=g).double()
    w = torch.rand(n, dtype=torch.float64, device=dev, generator=g) + 0.5
    assert F.supported(X, layers)
    out = {}

    def grad_new():
        out["g1"] = F.fused_grad(X, y, w, coef, layers)[0]

    def grad_old():
        out["g0"] = M.mlp_grad(X, y, w, coef, layers)[0]

    def search_new():
        out["s1"] = F.search_losses(X, y, w, coef, dirv, layers, 0.37, NSTEPS)

    def search_old():       # the body of OptimObjFunc._losses_at over MlpObjFunc._ce
        res = []
        for s in range(NSTEPS):
            P = mlp_forward(X, coef - dirv * (s * 0.37), layers)
            res.append((-torch.log(P.gather(1, y.long()[:, None])[:, 0].clamp_min(1e-300)) * w).sum())
        out["s0"] = torch.stack(res)

    def predict_new():
        res = F.rows(X, y, w, coef, layers, ("P", "label"))
        out["p1"], out["l1"] = res["P"].cpu(), res["label"].cpu()

    def predict_old():      # the former mapper: features and weights on the host
        P = mlp_forward(X.cpu(), coef.cpu(), layers)
        out["p0"], out["l0"] = P, P.argmax(1)
    return grad_new, grad_old, search_new, search_old, predict_new, predict_old, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x d0 : h.. : C")
    ap.add_argument("--sweep", default=SWEEP, help="comma-separated n of the small-n sweep, or empty")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--predict-rows", type=int, default=1000000, help="rows of the predict comparison at most")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd.ops import _lib, mlp_fused as F
    _lib.require()
    dev = torch.device("cuda:0")
    shapes = []
    for shape in [s for s in a.shapes.split(",") if s]:
        size, rest = shape.split(":", 1)
        n, d0 = (int(v) for v in size.split("x"))
        shapes.append((n, [d0] + [int(v) for v in rest.split(":")]))
    for n, layers in shapes:
        gn, go, sn, so, _, _, out = passes(n, layers, dev, a.seed)
        for fn in (gn, go, sn, so):
            fn()
        tg1, tg0 = alternate(gn, go, a.reps, timed)
        ts1, ts0 = alternate(sn, so, a.reps, timed)
        res = {"n": n, "layers": layers, "grad_new": stats(tg1), "grad_old": stats(tg0),
               "grad_speedup_median": statistics.median(tg0) / statistics.median(tg1),
               "search_new": stats(ts1), "search_old": stats(ts0),
               "search_speedup_median": statistics.median(ts0) / statistics.median(ts1),
               "x_bytes": 8 * n * layers[0], "chunk_rows": F.mlp_chunk_rows(n, layers),
               "max_rel_diff": {"grad": rel(out["g1"], out["g0"]), "search": rel(out["s1"], out["s0"])},
               "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}
        del gn, go, sn, so, out
        torch.cuda.empty_cache()
        npred = min(n, a.predict_rows)
        *_, pn, po, out = passes(npred, layers, dev, a.seed)
        pn(), po()
        tp1, tp0 = alternate(pn, po, a.reps, wall)
        res.update({"predict_rows": npred, "predict_new": stats(tp1), "predict_old": stats(tp0),
                    "predict_speedup_median": statistics.median(tp0) / statistics.median(tp1),
                    "predict_max_abs_diff": float((out["p1"] - out["p0"]).abs().max()),
                    "predict_labels_differ": int((out["l1"].long() != out["l0"]).sum())})
        print(json.dumps(res), flush=True)
        del pn, po, out
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    if a.sweep:
        for _, layers in shapes:
            for n in [int(v) for v in a.sweep.split(",")]:
                gn, go, sn, so, _, _, _ = passes(n, layers, dev, a.seed)
                for _ in range(3):
                    for fn in (gn, go, sn, so):
                        fn()
                tg1, tg0 = alternate(gn, go, 3 * a.reps, wall)
                ts1, ts0 = alternate(sn, so, 3 * a.reps, wall)
                print(json.dumps({"sweep": True, "n": n, "layers": layers, "grad_new": stats(tg1),
                                  "grad_old": stats(tg0), "search_new": stats(ts1), "search_old": stats(ts0),
                                  "former_path_wins": statistics.median(tg0) < statistics.median(tg1)
                                  or statistics.median(ts0) < statistics.median(ts1)}), flush=True)


if __name__ == "__main__":
    main()
