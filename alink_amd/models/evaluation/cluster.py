"""Clustering evaluation (reference ``A/operator/batch/evaluation/EvalClusterBatchOp.java``,
``A/operator/common/evaluation/{ClusterEvaluationUtil,ClusterMetricsSummary}.java``).

Per-cluster count / vector sum / squared-norm sum are segment sums on the device, merged by one all-reduce;
a second pass gives per-cluster distance sums and the silhouette (the reference's closed form using the
cluster sums, so it stays O(N k) instead of O(N^2)).  External indices (NMI, purity, RI, ARI) come from the
[prediction x label] contingency matrix.

Both passes run on the row kinds of ``ops/kmeans_rows.py`` through ``ops/evalcluster.py``: fp64 and CSR rows on the
HIP kernels (a fused row pass without an [n, k] block, sums without float atomics; a sparse column wider than 1024
is never densified), every other kind in torch; integer tensor columns give their cluster slots and the contingency
matrix on the device.  ``ALINK_EVALCLUSTER_HIP=0`` runs ``_cluster_metrics_host``, the former path, instead.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np
import torch

from ...common.params import Params
from ...common.table import MTable
from ...parallel import comm
from ..common.features import extract_features
from .metrics import ClusterMetrics

__all__ = ["cluster_metrics", "contingency_params"]


def _pget(p, name):
    try:
        return p.get(name) if p.contains(name) else None
    except KeyError:
        return None


def contingency_params(mat: np.ndarray) -> dict:
    """NMI / purity / RI / ARI of a [pred][label] count matrix (``extractParamsFromConfusionMatrix``)."""
    m = np.asarray(mat, dtype=np.int64)
    actual, pred = m.sum(0), m.sum(1)
    total = int(m.sum())
    comb = lambda x: x * (x - 1) // 2  # noqa: E731
    ent = lambda f: 0.0 if f == 0 else (f / total) * math.log(f / total)  # noqa: E731
    ea = sum(ent(int(a)) for a in actual) / -math.log(2)
    ep = sum(ent(int(p)) for p in pred) / -math.log(2)
    tpfp = int(sum(comb(int(a)) for a in actual))
    tpfn = int(sum(comb(int(p)) for p in pred))
    mi, purity, tp = 0.0, 0.0, 0
    for i in range(m.shape[0]):
        purity += int(m[i].max()) if m.shape[1] else 0
        for j in range(m.shape[1]):
            v = int(m[i, j])
            if v:
                mi += v / total * math.log(total * v / pred[i] / actual[j])
            tp += comb(v)
    purity /= total
    mi /= math.log(2)
    fp, fn = tpfp - tp, tpfn - tp
    totc = comb(total)
    tn = totc - tp - fn - fp
    expected = tpfp * tpfn / totc
    mx = (tpfp + tpfn) / 2
    return {"NMI": 2.0 * mi / (ea + ep), "purity": purity, "ri": (tp + tn) / (tp + tn + fp + fn),
            "ari": (tp - expected) / (mx - expected)}


def cluster_metrics(mt: MTable, params: Params, env) -> ClusterMetrics:
    """The operator's metrics: the row kinds and kernels of ``ops/evalcluster.py``, or with
    ``ALINK_EVALCLUSTER_HIP=0`` the host path below (dense rows, an [n, k] block), which is also the tests' oracle."""
    from ...ops.evalcluster import DIST_CODES
    dist = _pget(params, "distanceType") or "EUCLIDEAN"
    dist = str(getattr(dist, "name", dist)).upper()
    if os.environ.get("ALINK_EVALCLUSTER_HIP", "") == "0" or dist not in DIST_CODES:
        return _cluster_metrics_host(mt, params, env)       # any other distance type is evaluated as it always was
    return _cluster_metrics_rows(mt, params, env, dist)


def _slots(col, dev):
    """(distinct ids of this rank as strings, slot_of, columnar) of a prediction or label column: ``slot_of(order)``
    gives the rows' positions (int64 on ``dev``, -1 for a null) in the global id list ``order``.  An integer tensor
    column is mapped on its device (``columnar``: ``torch.unique``, a lookup over the distinct values,
    ``Column.nulls`` masked); any other column goes row by row."""
    v = col.values
    if isinstance(v, torch.Tensor) and v.dim() == 1 and not v.is_floating_point() and not v.is_complex() \
            and v.dtype != torch.bool:
        v = v.to(dev)
        ok = ~col.nulls.to(dev) if col.nulls is not None else torch.ones(v.shape, dtype=torch.bool, device=dev)
        uniq = torch.unique(v[ok])
        strs = [str(x) for x in uniq.tolist()]

        def slot_of(order):
            if not strs:
                return torch.full(v.shape, -1, dtype=torch.int64, device=dev)
            index = {c: i for i, c in enumerate(order)}
            lut = torch.tensor([index[s] for s in strs], dtype=torch.int64, device=dev)
            pos = torch.searchsorted(uniq, v).clamp_max(len(strs) - 1)      # a null's fill value may be past the end
            return torch.where(ok, lut[pos], torch.full_like(pos, -1))
        return strs, slot_of, True
    vals = col.to_list()

    def slot_of(order):
        index = {c: i for i, c in enumerate(order)}
        return torch.tensor([-1 if p is None else index[str(p)] for p in vals], dtype=torch.int64, device=dev)
    return sorted({str(p) for p in vals if p is not None}), slot_of, False


def _gather_ids(strs):
    ids = set()
    for part in comm.all_gather_object(sorted(set(strs))):
        ids.update(part)
    return ids


def _centre_distances(mean: torch.Tensor, code: int) -> np.ndarray:
    """The [k, k] distances between the cluster means, in row blocks of the mean table, read back once."""
    from ...ops import evalcluster as ev
    k, d = mean.shape
    step = max(1, (1 << 25) // max(1, k * d))
    D = torch.cat([ev.distance(mean[i:i + step, None, :], mean[None, :, :], code) for i in range(0, k, step)])
    return D.cpu().numpy()


def _cluster_metrics_rows(mt: MTable, params: Params, env, dist: str) -> ClusterMetrics:
    from ...ops import evalcluster as ev
    pred_col = params.get("predictionCol")
    label_col = _pget(params, "labelCol")
    vec_col = _pget(params, "vectorCol")
    dev = env.device
    out = Params()
    pstrs, pslot, pcolumnar = _slots(mt.col(pred_col), dev)
    ids = _gather_ids(pstrs)
    cids = sorted(ids)      # string order: "10" < "2"
    k = len(cids)
    slot = pslot(cids)
    if vec_col:
        code = ev.DIST_CODES[dist]
        # rows without a prediction keep the slot -1: they add nothing to any sum and are not taken out
        fm = extract_features(mt, None, vec_col, dev)
        d = max(comm.all_gather_object(int(fm.ncols)))
        rows = ev.eval_rows(fm, d, dist)
        cid = slot.to(torch.int32)
        work = ev.sorted_work(rows, cid, k)         # the one stable sort of this evaluation
        buf = ev.cluster_sums(rows, cid, k, work).reshape(-1)
        comm.all_reduce(buf, "sum")
        buf = buf.reshape(k, d + 2)
        s, cnt, n2 = buf[:, :d], buf[:, d].contiguous(), buf[:, d + 1].contiguous()
        mean = s / cnt.clamp_min(1.0)[:, None]
        block = ev.row_pass(rows, cid, mean, cnt, n2, dist)
        rs = ev.cluster_row_sums(block, cid, k, work)
        buf2 = torch.cat([rs[:, 0], rs[:, 1], rs[:, 2].sum().reshape(1)])
        comm.all_reduce(buf2, "sum")
        dsum, d2sum, silsum = buf2[:k], buf2[k:2 * k], float(buf2[-1])
        total = float(cnt.sum())
        gmean = s.sum(0) / total
        ssb = float((ev.distance(mean, gmean[None, :], code) ** 2 * cnt).sum())
        ssw = float(d2sum.sum())
        comp = dsum / cnt.clamp_min(1.0)
        compactness = float(comp.sum()) / k
        compn, cntn = comp.cpu().numpy(), cnt.cpu().numpy()
        sep, dbi = 0.0, np.zeros(k)
        if k > 1:
            D = _centre_distances(mean, code)
            upper = np.triu_indices(k, 1)
            sep = float(D[upper].sum())
            pair = compn[:, None] + compn[None, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.where(D != 0, pair / np.where(D != 0, D, 1.0), np.inf)
            np.fill_diagonal(t, 0.0)
            dbi = np.maximum(t.max(1), 0.0)
        out.set("SSB", ssb)
        out.set("SSW", ssw)
        out.set("compactness", compactness)
        out.set("k", k)
        out.set("count", int(total))
        out.set("seperation", 2 * sep / (k * k - k) if k > 1 else 0.0)
        out.set("daviesBouldin", float(dbi.sum() / k))
        out.set("calinskiHarabaz", ssb * (total - k) / ssw / (k - 1) if k > 1 and ssw > 0 else float("nan"))
        out.set("clusterArray", cids)
        out.set("countArray", [float(c) for c in cntn])
        out.set("silhouetteCoefficient", silsum / total)
    else:
        t = torch.bincount(slot[slot >= 0], minlength=k).to(device="cpu", dtype=torch.float64)
        comm.all_reduce(t, "sum")
        out.set("count", int(t.sum()))
        out.set("k", k)
        out.set("clusterArray", cids)
        out.set("countArray", [float(c) for c in t.tolist()])
    if label_col:
        lstrs, lslot, lcolumnar = _slots(mt.col(label_col), dev)
        lab_arr = sorted(_gather_ids(lstrs), reverse=True)
        L = len(lab_arr)
        if pcolumnar and lcolumnar:
            # one bincount of pred * L + label; both id lists are in descending string order here
            pi, li = k - 1 - slot, lslot(lab_arr)
            both = (slot >= 0) & (li >= 0)
            mat = torch.bincount(pi[both] * L + li[both], minlength=k * L).reshape(k, L) \
                .to(device="cpu", dtype=torch.float64)
        else:
            preds, labels = mt.column_values(pred_col), mt.column_values(label_col)
            pi = {p: i for i, p in enumerate(sorted(ids, reverse=True))}
            li = {l: i for i, l in enumerate(lab_arr)}
            mat = torch.zeros((k, L), dtype=torch.float64)
            for p, l in zip(preds, labels):
                if p is not None and l is not None:
                    mat[pi[str(p)], li[str(l)]] += 1
        comm.all_reduce(mat, "sum")
        for key, v in contingency_params(mat.numpy().astype(np.int64)).items():
            out.set(key, v)
    return ClusterMetrics(out)


def _cluster_metrics_host(mt: MTable, params: Params, env) -> ClusterMetrics:
    pred_col = params.get("predictionCol")
    label_col = _pget(params, "labelCol")
    vec_col = _pget(params, "vectorCol")
    dist = str(_pget(params, "distanceType") or "EUCLIDEAN")
    dist = getattr(dist, "name", dist).upper() if not isinstance(dist, str) else dist.upper()
    dev = env.device
    preds = mt.column_values(pred_col)
    out = Params()
    # global cluster id list (string order)
    ids = set()
    for part in comm.all_gather_object(sorted({str(p) for p in preds if p is not None})):
        ids.update(part)
    cids = sorted(ids)
    k = len(cids)
    index = {c: i for i, c in enumerate(cids)}
    if vec_col:
        rows = [i for i, p in enumerate(preds) if p is not None and mt.column_values(vec_col)[i] is not None] \
            if False else [i for i, p in enumerate(preds) if p is not None]
        sub = mt.take(rows)
        X = extract_features(sub, None, vec_col, dev).to_dense().double()
        cid = torch.tensor([index[str(preds[i])] for i in rows], dtype=torch.long, device=dev)
        if dist != "EUCLIDEAN":
            # reference getClusterStatistics: every non-Euclidean distance (COSINE, CITYBLOCK) sums unit vectors
            X = X / X.norm(dim=1, keepdim=True).clamp_min(1e-300)
        d = X.shape[1]
        d = max(comm.all_gather_object(int(d)))
        if X.shape[1] < d:
            X = torch.nn.functional.pad(X, (0, d - X.shape[1]))
        cnt = torch.zeros(k, dtype=torch.float64, device=dev).index_add_(0, cid, torch.ones_like(cid, dtype=torch.float64))
        s = torch.zeros((k, d), dtype=torch.float64, device=dev).index_add_(0, cid, X)
        n2 = torch.zeros(k, dtype=torch.float64, device=dev).index_add_(0, cid, (X * X).sum(1))
        buf = torch.cat([cnt, s.reshape(-1), n2])
        comm.all_reduce(buf, "sum")
        cnt, s, n2 = buf[:k], buf[k:k + k * d].reshape(k, d), buf[k + k * d:]
        mean = s / cnt.clamp_min(1.0)[:, None]

        def dfun(a, b):
            # ContinuousDistance.calc of the metric (CosineDistance divides by both norms; CITYBLOCK = ManHattan)
            if dist == "COSINE":
                cross = a.norm(dim=-1) * b.norm(dim=-1)
                dot = (a * b).sum(-1)
                return 1.0 - torch.where(cross > 0, dot / torch.where(cross > 0, cross, torch.ones_like(cross)),
                                         torch.zeros_like(dot))
            if dist == "CITYBLOCK":
                return (a - b).abs().sum(-1)
            return torch.sqrt(((a - b) ** 2).sum(-1).clamp_min(0.0))

        own = dfun(X, mean[cid])
        dsum = torch.zeros(k, dtype=torch.float64, device=dev).index_add_(0, cid, own)
        d2sum = torch.zeros(k, dtype=torch.float64, device=dev).index_add_(0, cid, own * own)
        # silhouette (closed form over cluster sums; the reference's non-Euclidean form uses 1 - x.mean)
        if dist != "EUCLIDEAN":
            dis = 1.0 - X @ mean.T                                         # [n, k]
            cur = torch.where(cnt[cid] > 1, dis.gather(1, cid[:, None])[:, 0] * cnt[cid] / (cnt[cid] - 1),
                              torch.zeros_like(own))
        else:
            xn = (X * X).sum(1, keepdim=True)
            dis = cnt[None, :] * xn - 2 * cnt[None, :] * (X @ mean.T) + n2[None, :]
            cur = torch.where(cnt[cid] > 1, dis.gather(1, cid[:, None])[:, 0] / (cnt[cid] - 1).clamp_min(1.0),
                              torch.zeros_like(own))
            dis = dis / cnt[None, :].clamp_min(1.0)
        dis = dis.scatter(1, cid[:, None], float("inf"))
        nb = dis.min(1).values if k > 1 else torch.full_like(own, float("inf"))
        sil = torch.where(cur < nb, 1 - cur / nb, nb / cur - 1)
        sil = torch.nan_to_num(sil, nan=0.0)
        buf2 = torch.cat([dsum, d2sum, sil.sum().reshape(1)])
        comm.all_reduce(buf2, "sum")
        dsum, d2sum, silsum = buf2[:k], buf2[k:2 * k], float(buf2[-1])
        total = float(cnt.sum())
        gmean = s.sum(0) / total
        cntn, meann = cnt.cpu().numpy(), mean
        ssb = float((dfun(mean, gmean[None, :]) ** 2 * cnt).sum())
        ssw = float(d2sum.sum())
        comp = (dsum / cnt.clamp_min(1.0))
        compactness = float(comp.sum()) / k
        sep = 0.0
        dbi = np.zeros(k)
        compn = comp.cpu().numpy()
        for i in range(k):
            for j in range(i + 1, k):
                dd = float(dfun(mean[i], mean[j]))
                sep += dd
                t = (compn[i] + compn[j]) / dd if dd != 0 else float("inf")
                dbi[i] = max(dbi[i], t)
                dbi[j] = max(dbi[j], t)
        out.set("SSB", ssb)
        out.set("SSW", ssw)
        out.set("compactness", compactness)
        out.set("k", k)
        out.set("count", int(total))
        out.set("seperation", 2 * sep / (k * k - k) if k > 1 else 0.0)
        out.set("daviesBouldin", float(dbi.sum() / k))
        out.set("calinskiHarabaz", ssb * (total - k) / ssw / (k - 1) if k > 1 and ssw > 0 else float("nan"))
        out.set("clusterArray", cids)
        out.set("countArray", [float(c) for c in cntn])
        out.set("silhouetteCoefficient", silsum / total)
    else:
        cnt = np.zeros(k)
        for p in preds:
            if p is not None:
                cnt[index[str(p)]] += 1
        t = torch.tensor(cnt, dtype=torch.float64)
        comm.all_reduce(t, "sum")
        out.set("count", int(t.sum()))
        out.set("k", k)
        out.set("clusterArray", cids)
        out.set("countArray", [float(c) for c in t.tolist()])
    if label_col:
        labels = mt.column_values(label_col)
        ls = set()
        for part in comm.all_gather_object(sorted({str(l) for l in labels if l is not None})):
            ls.update(part)
        lab_arr = sorted(ls, reverse=True)
        pred_arr = sorted(ids, reverse=True)
        li = {l: i for i, l in enumerate(lab_arr)}
        pi = {p: i for i, p in enumerate(pred_arr)}
        mat = torch.zeros((len(pred_arr), len(lab_arr)), dtype=torch.float64)
        for p, l in zip(preds, labels):
            if p is not None and l is not None:
                mat[pi[str(p)], li[str(l)]] += 1
        comm.all_reduce(mat, "sum")
        for key, v in contingency_params(mat.numpy().astype(np.int64)).items():
            out.set(key, v)
    return ClusterMetrics(out)
