#!/usr/bin/env python3
"""The fused Newton pass on one GPU (``ops/newton.py``, ``csrc/newton.hip``) against the three calls it replaces in
``calc_hessian_gradient_loss``: ``hessian_sum``, ``grad_sum`` and ``loss_per_sample`` (``profiles/newton.txt``).

    python tools/newton_bench.py                        # the seven shapes and the sweep
    python tools/newton_bench.py --shapes 1000000x32:log --sweep ""

Per shape ``n x d : loss`` (``log``, ``square``, ``aft`` with d the length of ``coef``, or ``softmaxK`` with K classes
and d columns; fp64 rows on the device) it times, after a warm-up of both paths at that shape, one ``calc_hessian_gradient_loss`` under ``ALINK_NEWTON_HIP=1``
and under ``=0``, alternated in the same process, with device events (the call ends in a copy of its two sums to
the host, so the events close after the work).  Printed per shape: medians of ``--reps`` and minima, the time of one
load of X at the 6.12 TB/s load-only rate README records, the time of the n d (d + 1) useful operations of the upper
triangle (softmax: times the k1 (k1 + 1) / 2 class pairs) at the 78.6 TFLOP/s fp64 matrix rate, the ratios of the
fused pass to both, each path's peak memory over the resident rows, and the largest relative difference of H, g and the loss between the paths.

``--sweep``: the same two calls at d = 32 and d = 128 over small n on the host clock: ``NEWTON_MIN_ROWS`` is the
smallest n from which the fused pass is never slower.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "10000000x32:log,2000000x128:log,20000000x8:square,10000000x17:aft," \
    "10000000x33:softmax10,20000000x9:softmax5,2000000x128:softmax8"
SWEEP = "64,256,1024,4096,16384,65536,262144"
LOAD_BPS = 25.6e9 / 4.18e-3         # README: the bf16 KMeans kernel's load-only pass over 1e8 x 128 bf16
MFMA_FLOPS = 78.6e12                # fp64 matrix rate of the MI355X data sheet


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "samples": len(t)}


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x d : loss")
    ap.add_argument("--sweep", default=SWEEP, help="comma-separated n of the small-n sweep, or empty")
    ap.add_argument("--sweep-d", default="32,128")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.models.linear import objfunc as O
    from alink_amd.ops import _lib, newton as N
    _lib.require()
    dev = torch.device("cuda:0")

    def problem(n, d, loss):
        """The objective, its partition and a coefficient vector with |eta| of order 1."""
        g = torch.Generator(device=dev).manual_seed(a.seed)
        k = d - 1 if loss == "aft" else d
        k1 = int(loss[7:]) - 1 if loss.startswith("softmax") else 1
        X = torch.randn((n, k), dtype=torch.float64, device=dev, generator=g)
        coef = torch.randn(d * k1, dtype=torch.float64, device=dev, generator=g) / d ** 0.5
        u = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        if loss.startswith("softmax"):
            obj, y, w = O.SoftmaxObjFunc(k1 + 1), torch.floor(u * (k1 + 1)), u + 0.5
        elif loss == "aft":
            obj, y, w = O.AftRegObjFunc(), torch.randn(n, dtype=torch.float64, device=dev, generator=g), \
                (u < 0.7).double()
        else:
            obj = O.UnaryLossObjFunc(O.LogLossFunc() if loss == "log" else O.SquareLossFunc())
            y, w = (torch.sign(u - 0.5) if loss == "log" else u), u + 0.5
        data = O.LabeledData(FeatureMatrix(X), y, w)
        out = {}

        def run(flag):
            def go():
                os.environ["ALINK_NEWTON_HIP"] = flag
                calls = N.NEWTON_CALLS
                out[flag] = obj.calc_hessian_gradient_loss(data, coef)
                assert (N.NEWTON_CALLS > calls) == (flag == "1")
            return go
        return run("1"), run("0"), out

    def alternate(new, old, reps, clock):
        t_new, t_old = [], []
        for _ in range(reps):
            t_new.append(clock(new))
            t_old.append(clock(old))
        return t_new, t_old

    def peak(fn, resident):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - resident) / 1e9

    for shape in [s for s in a.shapes.split(",") if s]:
        size, loss = shape.split(":")
        n, d = (int(v) for v in size.split("x"))
        new, old, out = problem(n, d, loss)
        new()
        old()
        resident = torch.cuda.memory_allocated()
        t_new, t_old = alternate(new, old, a.reps, timed)
        k = d - 1 if loss == "aft" else d
        load_ms = 8 * n * k / LOAD_BPS * 1e3
        k1 = int(loss[7:]) - 1 if loss.startswith("softmax") else 1
        mfma_ms = n * k * (k + 1) * (k1 * (k1 + 1) // 2) / MFMA_FLOPS * 1e3
        med = statistics.median(t_new)
        print(json.dumps({"n": n, "d": d, "loss": loss, "fused": stats(t_new), "former": stats(t_old),
                          "speedup_median": statistics.median(t_old) / med, "one_load_ms": load_ms,
                          "over_one_load": med / load_ms, "useful_mfma_ms": mfma_ms, "over_useful_mfma": med / mfma_ms,
                          "peak_over_resident_GB": {"fused": peak(new, resident), "former": peak(old, resident)},
                          "max_rel_diff": {"H": rel(out["1"][0], out["0"][0]), "g": rel(out["1"][1], out["0"][1]),
                                           "loss": rel(out["1"][3], out["0"][3])}}), flush=True)
        del new, old, out
        torch.cuda.empty_cache()

    if a.sweep:
        for d in [int(v) for v in a.sweep_d.split(",")]:
            for n in [int(v) for v in a.sweep.split(",")]:
                new, old, _ = problem(n, d, "log")
                for _ in range(3):
                    new()
                    old()
                t_new, t_old = alternate(new, old, 4 * a.reps, wall)
                print(json.dumps({"sweep": True, "n": n, "d": d, "fused": stats(t_new), "former": stats(t_old),
                                  "former_path_wins": statistics.median(t_old) < statistics.median(t_new)}),
                      flush=True)
    os.environ.pop("ALINK_NEWTON_HIP", None)


if __name__ == "__main__":
    main()
