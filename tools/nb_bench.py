#!/usr/bin/env python3
"""NaiveBayesText on one GPU: the exact label sums and the fused score / argmax / softmax kernels
(``ops/naive_bayes.py``) against the path they replace, ``ALINK_NB_HIP=0`` (``profiles/naive_bayes.txt``).

    python tools/nb_bench.py                    # the CSR shape, the dense shape, the gate sweep, the 1e7-row run
    python tools/nb_bench.py --big 0 --gate ""  # the A/B shapes alone

Per shape (CSR documents ``n x d x L @ entries``, dense fp64 rows ``n x d x L``; Multinomial and Bernoulli, with and
without a detail column) it times, after a warm-up of every path at that shape:

* the per-label sums, the train operator and the predict mapper on a loaded model (host clock around a call that ends
  in a device synchronise; the model's JSON is parsed once, outside the timing), new against ``ALINK_NB_HIP=0`` in the
  same process, alternated; the old path runs at ``--old-rows`` rows where its buffers still fit (its Bernoulli CSR
  path densifies every row: ``--old-bern-rows``; its detail column is a per-row Python loop: ``--old-detail-rows``),
  the new path at the same row count next to it;
* the prediction kernel alone with device events, against the bytes of one pass over the rows at the 6.12 TB/s
  load-only rate README records as the floor and, for CSR rows, against the table bytes it gathers (``kp`` doubles
  per stored entry);
* the largest difference between the two paths' detail probabilities.

``--gate``: the row counts of the crossover sweep (the Multinomial CSR predict mapper without a detail column, new
against old at each count); ``--big``: the row count at which the new path's sums and kernel run alone (the old
path's ``[nnz, L]`` buffer does not fit).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CSR = "200000x262144x20@100"
DENSE = "1000000x128x20"
GATE = "1,8,32,128,256,1024,4096,16384,65536"
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


def med(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "samples": len(t)}


def flagged(flag, fn):
    def run():
        os.environ["ALINK_NB_HIP"] = flag
        try:
            return fn()
        finally:
            os.environ.pop("ALINK_NB_HIP", None)
    return run


def ab(new, old, reps, old_reps, warmup=1):
    """Alternated samples of the two paths: (new stats, old stats)."""
    for _ in range(warmup):
        new()
        old()
    t_new, t_old = [], []
    for i in range(reps):
        t_new.append(wall(new))
        if i < old_reps:
            t_old.append(wall(old))
    return med(t_new), med(t_old)


def csr_docs(n, d, L, nnz, bernoulli, dev, seed):
    """Documents of ``nnz`` distinct columns (a random start and an odd stride per row) whose values and columns lean
    on the label: (crow, col int64, val, label int64)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    label = torch.randint(0, L, (n,), device=dev, generator=g)
    start = torch.randint(0, d, (n, 1), device=dev, generator=g) + label[:, None] * 7
    stride = torch.randint(0, d // (2 * nnz), (n, 1), device=dev, generator=g) * 2 + 1
    col = ((start + stride * torch.arange(nnz, device=dev)[None, :]) % d).reshape(-1)
    del start, stride
    if bernoulli:
        val = torch.ones(n * nnz, dtype=torch.float64, device=dev)
    else:
        val = torch.randint(1, 5, (n * nnz,), device=dev, generator=g).to(torch.float64)
    return torch.arange(n + 1, device=dev) * nnz, col, val, label


def table(vec, label, sparse, size=None):
    from alink_amd.common.linalg.block import SparseBlock
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    v = Column(SparseBlock(*vec, size)) if sparse else Column(vec)
    return MTable(TableSchema(["v", "label"], [Types.SPARSE_VECTOR if sparse else Types.DENSE_VECTOR, Types.LONG]),
                  [v, Column(label)])


def head(mt, m):
    """The first ``m`` rows of a bench table."""
    from alink_amd.common.table import Column, MTable
    v = mt.col("v").values
    return MTable(mt.schema, [Column(v[:m] if isinstance(v, torch.Tensor) else v.take(slice(0, m))),
                              Column(mt.col("label").values[:m])])


def train_op(mt, mtype):
    from alink_amd import NaiveBayesTextTrainBatchOp
    from alink_amd.operator.batch.source import TableSourceBatchOp
    op = NaiveBayesTextTrainBatchOp().setVectorCol("v").setLabelCol("label").setModelType(mtype) \
        .linkFrom(TableSourceBatchOp(mt))
    op.getOutputTable()
    return op


def predict_op(model, mt, detail, state=None, key=None):
    from alink_amd import NaiveBayesTextPredictBatchOp
    from alink_amd.operator.batch.source import TableSourceBatchOp
    op = NaiveBayesTextPredictBatchOp().setVectorCol("v").setPredictionCol("p").setReservedCols(["label"])
    if detail:
        op = op.setPredictionDetailCol("d")
    out = op.linkFrom(model, TableSourceBatchOp(mt)).getOutputTable()
    if state is not None:
        state[key] = out
    return out


def kernel(mt, tab, bern, reps):
    """Device-event medians of the prediction kernel alone on the table's rows against the model operand ``tab``
    (``ops.naive_bayes.Table``), with the byte figures."""
    from alink_amd.models.common.features import extract_features
    from alink_amd.ops import csr, naive_bayes as nb
    fm = extract_features(mt, None, "v", torch.device("cuda:0"))
    rows = nb.predict_rows(fm, tab.d)
    out = {}
    for want in (False, True):
        nb.predict(rows, tab, None, bern, want)
        torch.cuda.synchronize()
        out["prob" if want else "pred"] = med([timed(lambda: nb.predict(rows, tab, None, bern, want))
                                               for _ in range(reps)])
    n = rows.n
    if fm.is_sparse:
        entries = int(fm.col.numel())
        rows_bytes = entries * (fm.col.element_size() + 8) + (n + 1) * 8
        out["table_bytes_gathered"] = entries * csr.kp(tab.L) * 8
        out["gather_TBps_pred"] = round(out["table_bytes_gathered"] / out["pred"]["median_ms"] / 1e9, 3)
    else:
        rows_bytes = n * tab.d * 8
    out["one_pass_bytes"] = rows_bytes
    out["floor_ms"] = round(rows_bytes / LOAD_BPS * 1e3, 4)
    out["pred_over_floor"] = round(out["pred"]["median_ms"] / out["floor_ms"], 2)
    out["prob_over_floor"] = round(out["prob"]["median_ms"] / out["floor_ms"], 2)
    return out


def loaded_mapper(model, mt, detail):
    """The predict mapper on the trained model: the model's JSON is parsed here, once, outside every timing."""
    from alink_amd.common.params import Params
    from alink_amd.models.classification.naive_bayes import NaiveBayesTextModelMapper
    p = Params().set("vectorCol", "v").set("predictionCol", "p").set("reservedCols", ["label"])
    if detail:
        p = p.set("predictionDetailCol", "d")
    mapper = NaiveBayesTextModelMapper(model.getOutputTable().schema, mt.schema, p)
    mapper.loadModel(model.collect())
    return mapper


def sums_ab(part, L, a):
    """The per-label sums alone: ``label_sums`` against the one-hot product it replaces."""
    from alink_amd.models.common.features import extract_features
    from alink_amd.ops import naive_bayes as nb
    fm = extract_features(part, None, "v", torch.device("cuda:0"))
    y = part.col("label").values
    d, n = fm.ncols, part.num_rows

    def new():
        return nb.label_sums(nb.train_rows(fm, d), y, None, L)

    def old():
        Y = torch.zeros((n, L), dtype=torch.float64, device=y.device)
        Y[torch.arange(n, device=y.device), y] = 1.0
        return fm.rmm(Y, d).T.contiguous(), Y.sum(0)
    t_new, t_old = ab(new, old, a.reps, a.old_reps)
    f_new, f_old = new()[0], old()[0]
    return {"rows": n, "new": t_new, "old": t_old, "speedup_median": round(t_old["median_ms"] / t_new["median_ms"], 2),
            "max_abs_diff": float((f_new - f_old).abs().max())}


def mapper_ab(model, sub, detail, reps, old_reps):
    """Alternated samples of the loaded mapper on ``sub``: (new, old, the two outputs' columns)."""
    mapper = loaded_mapper(model, sub, detail)
    state = {}

    def run(key):
        def go():
            state[key] = mapper._map_columns(sub)
        return go
    t_new, t_old = ab(flagged("1", run("new")), flagged("0", run("old")), reps, old_reps)
    return t_new, t_old, state


def shape_run(name, mt, a, old_rows, old_bern_rows, L):
    from alink_amd.ops import naive_bayes as nb
    n = mt.num_rows
    for mtype in ("Multinomial", "Bernoulli"):
        rec = {"shape": name, "model": mtype, "n": n}
        cap = min(n, old_bern_rows if (mtype == "Bernoulli" and name.startswith("csr")) else old_rows)
        full = head(mt, min(n, old_rows))
        if mtype == "Multinomial":      # the sums do not depend on the model type
            rec["label_sums"] = sums_ab(full, L, a)
        t_new, t_old = ab(flagged("1", lambda: train_op(full, mtype)), flagged("0", lambda: train_op(full, mtype)),
                          a.reps, a.old_reps)
        rec["train_operator"] = {"rows": full.num_rows, "new": t_new, "old": t_old,
                                 "speedup_median": round(t_old["median_ms"] / t_new["median_ms"], 2)}
        model = flagged("1", lambda: train_op(mt, mtype))()
        for detail in (False, True):
            m = min(cap, a.old_detail_rows) if detail else cap
            sub = head(mt, m)
            t_new, t_old, state = mapper_ab(model, sub, detail, a.reps, a.old_reps)
            key = "predict_detail" if detail else "predict"
            rec[key] = {"rows": m, "new": t_new, "old": t_old,
                        "speedup_median": round(t_old["median_ms"] / t_new["median_ms"], 2)}
            rec["labels_equal" + ("_detail" if detail else "")] = \
                state["new"][0].to_list() == state["old"][0].to_list()
            if detail:
                worst = 0.0
                for x, y in zip(state["new"][1].to_list(), state["old"][1].to_list()):
                    px, py = json.loads(x), json.loads(y)
                    worst = max(worst, max(abs(px[k] - py[k]) for k in px))
                rec["max_prob_diff"] = worst
            del state
        rec["predict_operator_new_full"] = med([wall(flagged("1", lambda: predict_op(model, mt, False)))
                                                for _ in range(a.reps)])
        mapper = loaded_mapper(model, mt, False)
        bern = mtype == "Bernoulli"
        th, pi = mapper.model["theta"], mapper.model["pi"]
        rec["kernel"] = kernel(mt, nb.Table(mapper.minmat, pi + mapper.phi) if bern else nb.Table(th, pi), bern,
                               a.reps)
        del mapper
        rec["peak_mem_GB"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csr", default=CSR, help="n x d x L @ entries per row, or empty")
    ap.add_argument("--dense", default=DENSE, help="n x d x L, or empty")
    ap.add_argument("--gate", default=GATE, help="row counts of the crossover sweep, or empty")
    ap.add_argument("--big", type=int, default=10_000_000, help="rows of the new path's run alone, 0 for none")
    ap.add_argument("--old-rows", type=int, default=200_000)
    ap.add_argument("--old-bern-rows", type=int, default=500)
    ap.add_argument("--old-detail-rows", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from alink_amd import useLocalEnv
    from alink_amd.ops import _lib
    _lib.require()
    dev = torch.device("cuda:0")
    useLocalEnv(1, device="cuda:0")

    if a.csr:
        shape, nnz = a.csr.split("@")
        n, d, L = (int(v) for v in shape.split("x"))
        nnz = int(nnz)
        crow, col, val, label = csr_docs(n, d, L, nnz, True, dev, a.seed)      # 0 / 1 documents serve both models
        mt = table((crow, col, val), label, True, d)
        shape_run(f"csr {a.csr}", mt, a, a.old_rows, a.old_bern_rows, L)
        if a.gate:
            model = flagged("1", lambda: train_op(mt, "Multinomial"))()
            sweep = []
            for m in (int(v) for v in a.gate.split(",")):
                t_new, t_old, _ = mapper_ab(model, head(mt, m), False, 7, 7)
                sweep.append({"rows": m, "new_ms": t_new["median_ms"], "old_ms": t_old["median_ms"]})
            faster = [s["rows"] for s in sweep if s["new_ms"] < s["old_ms"]]
            print(json.dumps({"gate_sweep": "csr Multinomial predict mapper, no detail", "points": sweep,
                              "first_rows_new_faster": min(faster) if faster else None}), flush=True)
            del model
        del mt, crow, col, val, label
        torch.cuda.empty_cache()
        if a.big:
            torch.cuda.reset_peak_memory_stats()
            crow, col, val, label = csr_docs(a.big, d, L, nnz, True, dev, a.seed + 1)
            mt = table((crow, col, val), label, True, d)
            from alink_amd.models.common.features import extract_features
            from alink_amd.ops import naive_bayes as nb
            fm = extract_features(mt, None, "v", dev)

            def sums():
                return nb.label_sums(nb.train_rows(fm, d), label, None, L)
            first = wall(sums)                  # builds the CSC view of the rows
            t_sums = med([wall(sums) for _ in range(3)])
            feat, wsum = sums()
            # the model on the device, by the operator's formulas at smoothing 1 (the operator's own host loop over
            # the label column is not what this run measures)
            pi = torch.log(wsum + 1.0) - torch.log(wsum.sum() + L)
            for mtype in ("Multinomial", "Bernoulli"):
                bern = mtype == "Bernoulli"
                th = torch.log(feat + 1.0) - torch.log(wsum + 2.0 if bern else feat.sum(1) + d)[:, None]
                if bern:
                    tmp = torch.log(1.0 - torch.exp(th))
                    tab = nb.Table((th - tmp).cpu(), (pi + tmp.sum(1)).cpu())
                else:
                    tab = nb.Table(th.cpu(), pi.cpu())
                rec = {"shape": f"csr {a.big}x{d}x{L}@{nnz}", "model": mtype, "new_path_alone": True,
                       "label_sums_first_ms": round(first, 1), "label_sums": t_sums,
                       "kernel": kernel(mt, tab, bern, 3),
                       "old_path_nnz_L_buffer_GB": a.big * nnz * L * 8 / 1e9,
                       "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2)}
                print(json.dumps(rec), flush=True)
                del tab, th
            del fm, feat, wsum
            del mt, crow, col, val, label
            torch.cuda.empty_cache()

    if a.dense:
        n, d, L = (int(v) for v in a.dense.split("x"))
        g = torch.Generator(device=dev).manual_seed(a.seed)
        label = torch.randint(0, L, (n,), device=dev, generator=g)
        lean = (torch.arange(d, device=dev)[None, :] % L) == label[:, None]
        X = (torch.rand((n, d), device=dev, generator=g) < 0.2 + 0.2 * lean).to(torch.float64)
        del lean
        shape_run(f"dense {a.dense}", table(X, label, False), a, a.old_rows, a.old_rows, L)


if __name__ == "__main__":
    main()
