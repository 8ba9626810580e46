#!/usr/bin/env python3
"""The pairwise-complete moment pass on one GPU (``ops/moments.pairwise_moments``, ``csrc/moments.hip``) against the
four-GEMM chain it replaces (``profiles/pairwise_moments.txt``).

    python tools/pairwise_bench.py                       # the four shapes and the sweep
    python tools/pairwise_bench.py --shapes 1000000x512 --sweep ""

Per shape ``n x d`` (fp64 columns of mean 5 and unit spread on the device, zero-filled where absent, and their
presence mask, ``--missing`` of the cells absent: what ``correlation`` holds) it times with device events, after a
warm-up of both paths, the two paths alternated in the same process (the clocks and the rule ``select`` are those of
``tools/moments_bench.py``):

* new: the ``where`` that writes NaN into the absent cells and one ``pairwise_moments(X, shift)`` call;
* former: ``_pearson_pairwise``'s chain, the mask as fp64, the zero fill, ``A * A`` and four ``tn_matmul``.

Printed per shape: medians and minima, the former path's spread, each path's peak memory over the resident columns and
mask, the new pass over the floor of one load of X at the 6.12 TB/s load-only rate README records and over the floor
of its useful matrix operations, six times the n d (d + 1) of the plain upper triangle, at the 78.6 TFLOP/s fp64
matrix rate.  ``--sweep``: both paths over small n on the host clock around a synchronised call: ``PAIRWISE_MIN_ROWS``
is the smallest swept n from which the new pass wins at every swept width.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from moments_bench import LOAD_BPS, MFMA_FLOPS, alternate, compare, rel, timed, wall  # noqa: E402

SHAPES = "20000000x8,10000000x32,2000000x128,1000000x512"
SWEEP = "64,256,1024,4096,16384,65536,262144"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x d")
    ap.add_argument("--sweep", default=SWEEP, help="comma-separated n of the small-n sweep, or empty")
    ap.add_argument("--sweep-d", default="8,32,128", help="comma-separated d of the sweep")
    ap.add_argument("--missing", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd.ops import _lib, moments as M
    from alink_amd.ops.gemm import tn_matmul
    _lib.require()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(a.seed)

    def passes(n, d, state):
        valid = torch.rand((n, d), device=dev, generator=g) >= a.missing
        X = torch.where(valid, torch.randn((n, d), dtype=torch.float64, device=dev, generator=g) + 5.0, 0.0)
        shift = torch.full((d,), 5.0, dtype=torch.float64, device=dev)

        def new():
            state["new"] = M.pairwise_moments(torch.where(valid, X, float("nan")), shift)

        def old():
            Mk, A = valid.to(X.dtype), torch.where(valid, X, torch.zeros_like(X))
            state["old"] = torch.stack([tn_matmul(Mk, Mk), tn_matmul(A, Mk), tn_matmul(A * A, Mk), tn_matmul(A, A)])
        return shift, new, old

    def peak(fn):
        """GB that one call of ``fn`` allocates at its peak over what is resident before it."""
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 1e9

    for shape in [s for s in a.shapes.split(",") if s]:
        n, d = (int(v) for v in shape.split("x"))
        state = {}
        shift, new, old = passes(n, d, state)
        res = compare(*alternate(new, old, a.reps, a.reps, timed))
        state.clear()
        mem = {"new": peak(new), "former": peak(old)}
        N, S, Q, P = state["new"]
        oN, oS, oQ, oP = state["old"]       # the former sums are unshifted: undo the shift of the new ones
        h = shift[:, None]
        diff = {"N": rel(N, oN), "S": rel(S + h * N, oS), "Q": rel(Q + 2 * h * S + h * h * N, oQ),
                "P": rel(P + h * S.T + h.T * S + h * h.T * N, oP)}
        state.clear()
        load_ms = 8 * n * d / LOAD_BPS * 1e3
        mfma_ms = 6 * n * d * (d + 1) / MFMA_FLOPS * 1e3
        med = res["new"]["median_ms"]
        print(json.dumps({"n": n, "d": d, **res, "load_floor_ms": load_ms, "over_load_floor": med / load_ms,
                          "mfma_floor_ms": mfma_ms, "over_mfma_floor": med / mfma_ms, "max_rel_diff": diff,
                          "peak_extra_GB": mem}), flush=True)
        del new, old, N, S, Q, P, oN, oS, oQ, oP
        torch.cuda.empty_cache()

    if a.sweep:
        for d in [int(v) for v in a.sweep_d.split(",")]:
            for n in [int(v) for v in a.sweep.split(",")]:
                _, new, old = passes(n, d, {})
                res = compare(*alternate(new, old, 4 * a.reps, 4 * a.reps, wall))
                print(json.dumps({"sweep": True, "n": n, "d": d, **res,
                                  "former_path_wins": res["new_over_former"] > 1.0}), flush=True)


if __name__ == "__main__":
    main()
