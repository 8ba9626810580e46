"""Cluster evaluation passes over one rank's rows (``models/evaluation/cluster.py``): the per-cluster sums, the fused
row pass and the per-cluster sums of its output, on the row kinds of ``ops/kmeans_rows.py``.

* ``eval_rows(fm, d, dist_type)`` -> the rows object: CSR where ``sparse_selected`` takes the column (a sparse
  column wider than 1024, ``ALINK_KMEANS_SPARSE`` honoured), else a dense fp64 block under ``d`` columns; every
  non-Euclidean type (COSINE and CITYBLOCK, the reference's ``getClusterStatistics``) normalises the rows first;
* ``sorted_work(rows, cid, k)`` -> the one stable sort of an evaluation (None for the torch kinds);
* ``cluster_sums(rows, cid, k)`` -> ``[k, d+2] = [sum x | count | sum |x|^2]``: ``Rows.child_stats``;
* ``row_pass(rows, cid, mean, cnt, n2, dist_type)`` -> fp64 ``[n, 3] = [own, own^2, sil]`` per row: the distance to
  the mean of the row's own cluster and the reference's closed-form silhouette
  (``ClusterEvaluationUtil.calSilhouetteCoefficient``), with no ``[n, k]`` buffer on the GPU;
* ``cluster_row_sums(block, cid, k)`` -> ``[k, 3]``, through ``kmeans_dense64.accumulate``.

A row whose ``cid`` is outside ``[0, k)`` adds nothing to any sum and gets a zero row in the block.

GPU: ``csrc/evalcluster.hip`` — fp64 rows (1 <= d <= 1024) on the fp64 matrix cores with the means staged in LDS,
CSR rows one wave per row against the transposed mean table (the row walk of ``csrc/csr_rows.h``, handed over by
``ops/csr.py``); the sums through the sort-based dense accumulate and the
CSC accumulate, no float atomics: bitwise identical from run to run and for every grid.
Every other kind (CPU rows, fp32 rows, wider dense rows, an empty partition): the torch functions below, chunked
over rows; CSR rows never become a dense matrix.  Non-finite rows are not guaranteed to agree between the two.

With a GPU present a missing kernel library raises, unless ``ALINK_ALLOW_TORCH_FALLBACK=1``.
"""
from __future__ import annotations

import torch

from . import _lib, csr, kmeans_dense64 as kd64, kmeans_rows as krows

__all__ = ["DIST_CODES", "eval_rows", "sorted_work", "cluster_sums", "row_pass", "cluster_row_sums", "distance",
           "row_pass_torch"]

DIST_CODES = {"EUCLIDEAN": 0, "COSINE": 1, "CITYBLOCK": 2}
EVALCLUSTER_CALLS = 0   # launches of the HIP row pass (tests read it)
TORCH_CHUNK = 1 << 14   # dense rows per chunk of the torch path
SPARSE_CHUNK = 1 << 12  # CSR rows per chunk of the torch path (the gathered [entries, k] block sets the size)


def _dist_code(dist_type: str) -> int:
    try:
        return DIST_CODES[dist_type.upper()]
    except KeyError:
        raise ValueError(f"cluster evaluation supports EUCLIDEAN, COSINE and CITYBLOCK, not {dist_type}") from None


def eval_rows(fm, d: int, dist_type: str):
    """The rows object of one rank's ``FeatureMatrix`` under the global vector size ``d``."""
    unit = _dist_code(dist_type) != 0
    if fm.is_sparse and krows.sparse_selected(True, d):
        return krows.rows(krows.sparse_rows(fm, d, "COSINE" if unit else "EUCLIDEAN"), "EUCLIDEAN")
    if fm.is_sparse:
        fm.set_ncols(d)
    X = fm.to_dense().to(torch.float64)
    if X.shape[1] < d:
        X = torch.nn.functional.pad(X, (0, d - X.shape[1]))
    if unit:
        X = X / X.norm(dim=1, keepdim=True).clamp_min(1e-300)
    return krows.rows(X.contiguous(), "EUCLIDEAN")


def _hip_kind(rows, k: int):
    """"f64" / "csr" when the HIP kernels take these rows, else None (an empty partition launches nothing)."""
    if rows.n == 0:
        return None
    if isinstance(rows, krows._Dense64Rows):
        return "f64" if kd64.use_hip(rows.X, k) else None
    if isinstance(rows, krows._SparseRows):
        return "csr" if csr.use_hip(rows.X) else None
    return None


def sorted_work(rows, cid: torch.Tensor, k: int):
    """The work list of the rows' clusters for ``cluster_sums`` and ``cluster_row_sums``: one stable sort per
    evaluation on the HIP kinds, None on the others."""
    if _hip_kind(rows, k) is None:
        return None
    return kd64.sorted_work(cid, int(k), ignore_outside=True)


def cluster_sums(rows, cid: torch.Tensor, k: int, work=None, grid: int = 0) -> torch.Tensor:
    """fp64 ``[k, d+2] = [sum x | count | sum |x|^2]`` of the rows per cluster."""
    return rows.child_stats(cid, int(k), sqnorm=True, grid=grid, work=work)


def cluster_row_sums(block: torch.Tensor, cid: torch.Tensor, k: int, work=None, grid: int = 0) -> torch.Tensor:
    """fp64 ``[k, 3]``: the columns of ``row_pass``'s block summed per cluster, rows in ascending order."""
    if work is not None and block.shape[0] > 0:
        return kd64.accumulate_work(block, work, int(k), grid)[:, :3]
    return kd64.accumulate(block, cid, int(k), grid, ignore_outside=True)[:, :3]


# ---------------------------------------------------------------------------------------------------
# torch path (CPU, fp32, wide dense rows; the formulas of the operator's host path)
# ---------------------------------------------------------------------------------------------------
def distance(a: torch.Tensor, b: torch.Tensor, code: int) -> torch.Tensor:
    """``ContinuousDistance.calc`` along the last axis (CosineDistance divides by both norms, 1 where one is 0;
    CITYBLOCK = ManHattan)."""
    if code == 1:
        cross = a.norm(dim=-1) * b.norm(dim=-1)
        dot = (a * b).sum(-1)
        return 1.0 - torch.where(cross > 0, dot / torch.where(cross > 0, cross, torch.ones_like(cross)),
                                 torch.zeros_like(dot))
    if code == 2:
        return (a - b).abs().sum(-1)
    return torch.sqrt(((a - b) ** 2).sum(-1).clamp_min(0.0))


def _finish(own, dot, xn, cs, ok, cnt, n2, code: int) -> torch.Tensor:
    """[m, 3] of a chunk from the own distances, the dots [m, k], |x|^2 and the clamped clusters ``cs``."""
    k = cnt.shape[0]
    if code == 0:
        dis = cnt[None, :] * xn[:, None] - 2 * cnt[None, :] * dot + n2[None, :]
        nbv = dis / cnt[None, :].clamp_min(1.0)
    else:
        dis = 1.0 - dot
        nbv = dis
    disown = dis.gather(1, cs[:, None])[:, 0]
    cn = cnt[cs]
    cur = disown / (cn - 1).clamp_min(1.0) if code == 0 else disown * cn / torch.where(cn > 1, cn - 1, cn)
    cur = torch.where(cn > 1, cur, torch.zeros_like(cur))
    nb = nbv.scatter(1, cs[:, None], float("inf")).min(1).values if k > 1 else torch.full_like(own, float("inf"))
    sil = torch.where(cur < nb, 1 - cur / nb, nb / cur - 1)
    sil = torch.where(sil != sil, torch.zeros_like(sil), sil)
    res = torch.stack([own, own * own, sil], 1)
    return torch.where(ok[:, None], res, torch.zeros_like(res))


def _row_pass_dense_torch(X, cid, mean, cnt, n2, code: int) -> torch.Tensor:
    n, k = X.shape[0], mean.shape[0]
    out = torch.zeros((n, 3), dtype=torch.float64, device=X.device)
    for s in range(0, n, TORCH_CHUNK):
        x = X[s:s + TORCH_CHUNK].to(torch.float64)
        c = cid[s:s + TORCH_CHUNK].to(torch.int64)
        ok = (c >= 0) & (c < k)
        cs = torch.where(ok, c, torch.zeros_like(c))
        out[s:s + TORCH_CHUNK] = _finish(distance(x, mean[cs], code), x @ mean.T, (x * x).sum(1), cs, ok, cnt, n2,
                                         code)
    return out


def _row_pass_csr_torch(fm, d: int, cid, mean, cnt, n2, code: int) -> torch.Tensor:
    """Chunked CSR products; ``own`` through the entries alone, in the kernel's rearranged forms."""
    n, k = fm.nrows, mean.shape[0]
    dev = fm.val.device
    out = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    col, val = csr.clipped(fm, d)                  # entries outside [0, d) are (0, 0.0): they add nothing
    safe = krows.sparse_view(fm, d, val.to(torch.float64))
    safe.col = col
    Mt = mean.t().contiguous()
    m2, m1 = (mean * mean).sum(1), mean.abs().sum(1)
    for s in range(0, n, SPARSE_CHUNK):
        sub = safe[s:s + SPARSE_CHUNK]
        m = sub.nrows
        c = cid[s:s + m].to(torch.int64)
        ok = (c >= 0) & (c < k)
        cs = torch.where(ok, c, torch.zeros_like(c))
        dot = sub.mm(Mt)
        xn = torch.zeros(m, dtype=torch.float64, device=dev)
        part = torch.zeros(m, dtype=torch.float64, device=dev)
        if sub.val.numel():
            rid, v = sub.row_ids(), sub.val
            xn.index_add_(0, rid, v * v)
            if code != 1:
                mj = mean[cs[rid], sub.col]
                part.index_add_(0, rid, (v - mj) ** 2 - mj * mj if code == 0 else (v - mj).abs() - mj.abs())
        if code == 0:
            own = torch.sqrt((m2[cs] + part).clamp_min(0.0))
        elif code == 2:
            own = m1[cs] + part
        else:
            cross = torch.sqrt(xn) * torch.sqrt(m2[cs])
            own = 1.0 - torch.where(cross > 0, dot.gather(1, cs[:, None])[:, 0]
                                    / torch.where(cross > 0, cross, torch.ones_like(cross)), torch.zeros_like(cross))
        out[s:s + m] = _finish(own, dot, xn, cs, ok, cnt, n2, code)
    return out


def row_pass_torch(rows, cid: torch.Tensor, mean: torch.Tensor, cnt: torch.Tensor, n2: torch.Tensor,
                   dist_type: str) -> torch.Tensor:
    """Torch implementation of ``row_pass`` (and the path of every kind the kernels do not take)."""
    code = _dist_code(dist_type)
    dev = rows.device
    mean, cnt, n2 = (t.to(device=dev, dtype=torch.float64) for t in (mean, cnt, n2))
    if isinstance(rows, krows._SparseRows):
        return _row_pass_csr_torch(rows.X, rows.d, cid, mean, cnt, n2, code)
    return _row_pass_dense_torch(rows.X, cid, mean, cnt, n2, code)


# ---------------------------------------------------------------------------------------------------
# HIP path
# ---------------------------------------------------------------------------------------------------
def _cluster_records(slots: int, mean, cnt, n2) -> torch.Tensor:
    """[slots, 8] fp64 per-cluster records of the kernels: cnt, n2, 1 / max(cnt, 1), |m|^2, sum |m|, zero padding;
    zero rows past k."""
    k = mean.shape[0]
    stat = torch.zeros((slots, 8), dtype=torch.float64, device=mean.device)
    stat[:k, 0] = cnt
    stat[:k, 1] = n2
    stat[:k, 2] = 1.0 / cnt.clamp_min(1.0)
    stat[:k, 3] = (mean * mean).sum(1)
    stat[:k, 4] = mean.abs().sum(1)
    return stat


def _row_pass_f64(X, cid, mean, cnt, n2, code: int, grid: int) -> torch.Tensor:
    dev = X.device
    n, d = X.shape
    k = mean.shape[0]
    img, _, nt, nblk = kd64.centroid_image(mean, 1, dev)       # the COSINE code: plain dots
    stat = _cluster_records(nblk * nt * 16, mean, cnt, n2)
    out = torch.empty((n, 3), dtype=torch.float64, device=dev)
    _lib.call("alink_evalcluster_rows_f64", X.data_ptr(), n, d, cid.data_ptr(), img.data_ptr(), mean.data_ptr(),
              stat.data_ptr(), k, nt, nblk, code, out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    return out


def _row_pass_csr(fm, d: int, cid, mean, cnt, n2, code: int, grid: int) -> torch.Tensor:
    dev = fm.val.device
    n = fm.nrows
    k = mean.shape[0]
    kp = csr.kp(k)
    Mt = csr.padded_transpose(mean, kp)
    stat = _cluster_records(kp, mean, cnt, n2)
    alive, head = csr.row_args(fm, d)      # alive: the arrays behind head's pointers
    out = torch.empty((n, 3), dtype=torch.float64, device=dev)
    _lib.call("alink_evalcluster_rows_csr", *head, cid.data_ptr(), Mt.data_ptr(), stat.data_ptr(), k, kp, code,
              out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    return out


def row_pass(rows, cid: torch.Tensor, mean: torch.Tensor, cnt: torch.Tensor, n2: torch.Tensor, dist_type: str,
             grid: int = 0) -> torch.Tensor:
    """fp64 ``[n, 3] = [own, own^2, sil]`` of every row against the cluster means ``mean`` [k, d] with the global
    counts ``cnt`` [k] and squared-norm sums ``n2`` [k]; ``cid`` int32 / int64 [n].  On the GPU the same bits for
    every launch and every ``grid``."""
    global EVALCLUSTER_CALLS
    code = _dist_code(dist_type)
    k = int(mean.shape[0])
    if mean.dim() != 2 or int(mean.shape[1]) != rows.d or k < 1 or cnt.shape != (k,) or n2.shape != (k,):
        raise ValueError("cluster mean shape mismatch")
    if cid.dim() != 1 or int(cid.shape[0]) != rows.n:
        raise ValueError("cid must be an [n] tensor")
    kind = _hip_kind(rows, k)
    if kind is None:
        return row_pass_torch(rows, cid, mean, cnt, n2, dist_type)
    dev = rows.device
    mean = mean.to(device=dev, dtype=torch.float64).contiguous()
    cnt, n2 = cnt.to(device=dev, dtype=torch.float64), n2.to(device=dev, dtype=torch.float64)
    cid = cid.to(device=dev, dtype=torch.int32).contiguous()
    if kind == "f64":
        out = _row_pass_f64(rows.X, cid, mean, cnt, n2, code, grid)
    else:
        out = _row_pass_csr(rows.X, rows.d, cid, mean, cnt, n2, code, grid)
    EVALCLUSTER_CALLS += 1
    return out
