"""Sparse-vector KMeans: nearest centroid and per-cluster sums of CSR rows against dense centroids, in fp64.

The rows are a sparse ``FeatureMatrix`` (``crow`` int64 ``[n+1]``, ``col`` int32 / int64, ``val`` fp64) — what the
NLP counters, the feature hasher and ``extract_features`` produce on the device — and never become a dense
``[n, d]`` matrix.  Reference: ``KMeansUtil.updateSumMatrix`` (``KMeansUtil.java:76-83``) adds a sparse sample's
stored entries into the dense sum matrix, ``FastDistance`` takes sparse samples against dense centroids.

* ``nearest(fm, C, dist_type)`` -> ``(idx int64 [n], dist fp64 [n])``: ``dist`` is the SQUARED distance for
  EUCLIDEAN and ``1 - x.c`` for COSINE (rows and centroids normalised by the caller);
* ``nearest_counts(fm, C, dist_type)`` -> exact int64 ``[k]`` counts (the k-means|| weights pass);
* ``assign_accumulate(fm, C, dist_type)`` -> the ``[k, d+1]`` fp64 buffer ``[sum_x | count]`` of ``ops/kmeans.py``;
* ``prepare(fm)``: the CSC view of the rows (a stable sort of the entries by column, built once per training run
  and cached on the matrix) with its (column, chunk) work list.

GPU: ``csrc/kmeans_sparse.hip`` — one wave per row for the assignment (the CSR row walk of ``csrc/csr_rows.h``
against the transposed, padded centroid table), one wave per (column, chunk of ``ACCUM_CHUNK`` entries) for the sums,
no float atomics: the sums are bitwise identical from run to run and for every grid.  Entries whose column is outside
``[0, d)`` are ignored.  Which matrices go to the kernels and how their arrays are handed over: ``ops/csr.py``.
CPU (and the oracle of the tests): ``nearest_torch`` / ``assign_accumulate_torch``, chunked over rows.

With a GPU present a missing kernel library raises, unless ``ALINK_ALLOW_TORCH_FALLBACK=1``.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from . import _lib, csr

__all__ = ["ACCUM_CHUNK", "sparse_supported", "sparse_selected", "prepare", "nearest", "nearest_counts",
           "assign_accumulate", "nearest_torch", "assign_accumulate_torch", "row_sqnorm", "take_dense",
           "accumulate_torch", "nearest_hip"]

ACCUM_CHUNK = 512       # entries of one column that one wave sums; longer columns are split and merged in order
DENSE_DMAX = 1024       # the largest d a dense HIP KMeans kernel covers (ops/kmeans.py): sparse input wider than
                        # this takes the sparse path.  It is also the dense fp64 limit (ops/kmeans_dense64.py)
SPARSE_CALLS = 0        # launches of the HIP sparse path (tests read it)
TORCH_CHUNK = 1 << 14   # rows per chunk of the torch path


def sparse_selected(column_is_sparse: bool, vector_size: int) -> bool:
    """The selection rule: a sparse column whose global vector size exceeds ``DENSE_DMAX``;
    ``ALINK_KMEANS_SPARSE=1`` takes every sparse column, ``=0`` none.  Dense input is never selected."""
    if not column_is_sparse:
        return False
    flag = os.environ.get("ALINK_KMEANS_SPARSE", "")
    if flag == "1":
        return True
    if flag == "0":
        return False
    return int(vector_size) > DENSE_DMAX


sparse_supported = csr.supported    # whether the HIP kernels take a matrix, under the name the tests ask by


def _dist_code(dist_type: str) -> int:
    dt = dist_type.upper()
    if dt not in ("EUCLIDEAN", "COSINE"):
        raise ValueError(f"sparse KMeans supports EUCLIDEAN and COSINE, not {dist_type}")
    return int(dt == "COSINE")


# ---------------------------------------------------------------------------------------------------
# torch path (CPU, oracle)
# ---------------------------------------------------------------------------------------------------
def row_sqnorm(fm, d: Optional[int] = None) -> torch.Tensor:
    """|x|^2 per row over the entries inside [0, d), summed in entry order (on the GPU by the CSR mat-vec kernel,
    which has a fixed order; ``index_add_`` there would sum by atomics)."""
    d = fm.ncols if d is None else int(d)
    n = fm.nrows
    out = torch.zeros(n, dtype=torch.float64, device=fm.val.device)
    if n == 0 or fm.val.numel() == 0 or d == 0:
        return out
    col, val = csr.clipped(fm, d)
    if val.is_cuda and _lib.available():
        from .feature import csr_mv
        return csr_mv(fm.crow, col, val * val, torch.ones(d, dtype=torch.float64, device=val.device))
    return out.index_add_(0, fm.row_ids(), (val * val).to(torch.float64))


def take_dense(fm, idx: torch.Tensor, d: Optional[int] = None) -> torch.Tensor:
    """The few rows ``idx`` of a sparse matrix as a dense fp64 ``[m, d]`` block (candidate centroids); entries
    outside ``[0, d)`` are dropped."""
    d = fm.ncols if d is None else int(d)
    dev = fm.val.device
    idx = idx.to(device=dev, dtype=torch.int64).reshape(-1)
    m = int(idx.shape[0])
    out = torch.zeros((m, d), dtype=torch.float64, device=dev)
    if m == 0 or fm.val.numel() == 0:
        return out
    starts = fm.crow[idx]
    counts = fm.crow[idx + 1] - starts
    off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(counts, 0)
    total = int(off[-1])
    if total == 0:
        return out
    rid = torch.repeat_interleave(torch.arange(m, device=dev), counts, output_size=total)
    pos = torch.arange(total, device=dev) - off[:-1][rid] + starts[rid]
    col = fm.col[pos].to(torch.int64)
    ok = (col >= 0) & (col < d)
    # a CSR row stores a column once, so the scatter has no colliding writes
    out[rid[ok], col[ok]] = fm.val[pos][ok].to(torch.float64)
    return out


def _scores_torch(fm, C: torch.Tensor, cosine: int, chunk: int):
    """Yields (first row, scores [m, k], |x|^2 [m]) per row chunk; score = |c|^2 - 2 x.c, or -x.c for COSINE."""
    k, d = C.shape
    Cd = C.to(device=fm.val.device, dtype=torch.float64)
    Ct = Cd.t().contiguous()
    cn = (Cd * Cd).sum(1)
    col, val = csr.clipped(fm, d)
    counts = fm.crow[1:] - fm.crow[:-1]
    n = fm.nrows
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        a, b = int(fm.crow[s]), int(fm.crow[e])
        m = e - s
        dot = torch.zeros((m, k), dtype=torch.float64, device=val.device)
        xn = torch.zeros(m, dtype=torch.float64, device=val.device)
        if b > a:
            rid = torch.repeat_interleave(torch.arange(m, device=val.device), counts[s:e], output_size=b - a)
            v = val[a:b].to(torch.float64)
            dot.index_add_(0, rid, v[:, None] * Ct[col[a:b]])
            xn.index_add_(0, rid, v * v)
        yield s, (-dot if cosine else cn[None, :] - 2.0 * dot), xn


def nearest_torch(fm, C: torch.Tensor, dist_type: str, chunk: int = TORCH_CHUNK) -> Tuple[torch.Tensor, torch.Tensor]:
    """Torch reference of ``nearest``: (idx int64 [n], squared distance / 1 - x.c fp64 [n])."""
    cosine = _dist_code(dist_type)
    n = fm.nrows
    dev = fm.val.device
    idx = torch.zeros(n, dtype=torch.int64, device=dev)
    dist = torch.zeros(n, dtype=torch.float64, device=dev)
    for s, sc, xn in _scores_torch(fm, C, cosine, chunk):
        best, bi = sc.min(1)
        idx[s:s + bi.shape[0]] = bi
        dist[s:s + bi.shape[0]] = 1.0 + best if cosine else (xn + best).clamp_min(0.0)
    return idx, dist


def accumulate_torch(fm, idx: torch.Tensor, k: int, d: int) -> torch.Tensor:
    """Torch path of the per-cluster sums: [k, d+1] fp64 ``[sum_x | count]`` of the rows' clusters ``idx`` int64 [n]
    (every value in [0, k))."""
    buf = torch.zeros((k, d + 1), dtype=torch.float64, device=fm.val.device)
    if fm.nrows == 0:
        return buf
    buf[:, d] = torch.bincount(idx, minlength=k).to(torch.float64)
    if fm.val.numel():
        col, val = csr.clipped(fm, d)
        buf.view(-1).index_add_(0, idx[fm.row_ids()] * (d + 1) + col, val.to(torch.float64))
    return buf


def assign_accumulate_torch(fm, C: torch.Tensor, dist_type: str, chunk: int = TORCH_CHUNK) -> torch.Tensor:
    """Torch reference of ``assign_accumulate``: [k, d+1] fp64 ``[sum_x | count]`` of the nearest-centroid
    assignment; on the CPU every (cluster, column) sum runs in ascending row order."""
    k, d = C.shape
    return accumulate_torch(fm, nearest_torch(fm, C, dist_type, chunk)[0], k, d)


# ---------------------------------------------------------------------------------------------------
# HIP path
# ---------------------------------------------------------------------------------------------------
def nearest_hip(fm, C: torch.Tensor, dist_type: str, want_idx: bool, want_dist: bool, want_counts: bool,
                 grid: int = 0):
    """``alink_kmeans_sparse_nearest`` with the outputs the caller asks for: (idx int32 [n], dist fp64 [n],
    counts int64 [csr.kp(k)]), each None unless wanted.  Nothing is launched for an empty matrix."""
    global SPARSE_CALLS
    cosine = _dist_code(dist_type)
    dev = fm.val.device
    k, d = C.shape
    n = fm.nrows
    idx = torch.zeros(n, dtype=torch.int32, device=dev) if want_idx else None
    dist = torch.zeros(n, dtype=torch.float64, device=dev) if want_dist else None
    kpad = csr.kp(k)
    counts = torch.zeros(kpad, dtype=torch.int64, device=dev) if want_counts else None
    if n == 0:      # nothing is launched for an empty partition
        return idx, dist, counts
    if k < 1 or d < 1:
        raise ValueError("sparse KMeans needs at least one centroid and one column")
    Cd = C.to(device=dev, dtype=torch.float64)
    Ct = csr.padded_transpose(Cd, kpad)
    cn = torch.full((kpad,), float("inf"), dtype=torch.float64, device=dev)     # +inf on the padded clusters
    cn[:k] = 0.0 if cosine else (Cd * Cd).sum(1)
    alive, head = csr.row_args(fm, d)      # alive: the arrays behind head's pointers
    _lib.call("alink_kmeans_sparse_nearest", *head, Ct.data_ptr(), cn.data_ptr(), kpad, 1.0 if cosine else 2.0,
              cosine, idx.data_ptr() if want_idx else None, dist.data_ptr() if want_dist else None,
              counts.data_ptr() if want_counts else None, int(grid), _lib.stream_ptr(dev))
    SPARSE_CALLS += 1
    return idx, dist, counts


def nearest(fm, C: torch.Tensor, dist_type: str, grid: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Nearest centroid per row: (idx int64 [n], dist fp64 [n]) — squared distance for EUCLIDEAN, ``1 - x.c`` for
    COSINE.  Equal scores go to the lowest centroid index; an empty row takes ``argmin |c|^2``."""
    if csr.use_hip(fm):
        idx, dist, _ = nearest_hip(fm, C, dist_type, True, True, False, grid)
        return idx.to(torch.int64), dist
    return nearest_torch(fm, C, dist_type)


def nearest_counts(fm, C: torch.Tensor, dist_type: str, grid: int = 0) -> torch.Tensor:
    """Rows per nearest centroid, exact int64 [k] (integer atomics on the GPU, no per-row output)."""
    k = C.shape[0]
    if csr.use_hip(fm):
        return nearest_hip(fm, C, dist_type, False, False, True, grid)[2][:k]
    return torch.bincount(nearest_torch(fm, C, dist_type)[0], minlength=k)


class _Csc:
    """CSC view of a CSR matrix for the accumulate kernel: entries stably sorted by column (rows ascend inside a
    column) and the (column, chunk) work list, every chunk at most ``ACCUM_CHUNK`` consecutive entries."""
    __slots__ = ("d", "rows", "vals", "nwork", "wcol", "wstart", "wlen", "wslot", "nmulti", "mcol", "mfirst",
                 "mcount", "nslots")


def prepare(fm, d: Optional[int] = None) -> _Csc:
    """The CSC index of ``fm`` for ``d`` columns, built once and cached on the matrix."""
    d = fm.ncols if d is None else int(d)
    cached = getattr(fm, "_kmeans_csc", None)
    if cached is not None and cached.d == d:
        return cached
    dev = fm.val.device
    col = fm.col.to(torch.int64)
    # entries outside [0, d) get the key d: they sort behind every column and no work item covers them
    key = torch.where((col >= 0) & (col < d), col, torch.full_like(col, d))
    skey, order = torch.sort(key, stable=True)
    del key, col
    csc = _Csc()
    csc.d = d
    csc.rows = fm.row_ids().index_select(0, order).to(torch.int32)
    csc.vals = fm.val.index_select(0, order).contiguous()
    del order
    cnt = torch.bincount(skey, minlength=d + 1)[:d]
    del skey
    colptr = torch.zeros(d + 1, dtype=torch.int64, device=dev)
    colptr[1:] = torch.cumsum(cnt, 0)
    nch = (cnt + (ACCUM_CHUNK - 1)) // ACCUM_CHUNK
    multi = nch > 1
    nwork, nmulti, nslots = (int(v) for v in torch.stack([nch.sum(), multi.sum(), (nch * multi).sum()]).tolist())
    csc.nwork, csc.nmulti, csc.nslots = nwork, nmulti, nslots
    first_work = torch.cumsum(nch, 0) - nch                      # a column's first work item
    csc.wcol = torch.repeat_interleave(torch.arange(d, device=dev), nch, output_size=nwork)
    chunk = torch.arange(nwork, device=dev) - first_work[csc.wcol]
    csc.wstart = colptr[csc.wcol] + chunk * ACCUM_CHUNK
    csc.wlen = torch.minimum(colptr[csc.wcol + 1] - csc.wstart,
                             torch.full_like(csc.wstart, ACCUM_CHUNK)).to(torch.int32)
    slots = nch * multi
    first_slot = torch.cumsum(slots, 0) - slots                  # a multi-chunk column's first partial row
    csc.wslot = torch.where(multi[csc.wcol], first_slot[csc.wcol] + chunk, torch.full_like(chunk, -1))
    csc.mcol = torch.nonzero(multi).reshape(-1)
    csc.mfirst = first_slot[csc.mcol].contiguous()
    csc.mcount = nch[csc.mcol].contiguous()
    fm._kmeans_csc = csc
    return csc


def accumulate_hip(fm, idx: torch.Tensor, k: int, d: int, counts: Optional[torch.Tensor] = None,
                   grid: int = 0) -> torch.Tensor:
    """[k, d+1] fp64 ``[sum_x | count]`` of the rows' clusters ``idx`` (int32 [n]) through the CSC view; the same
    bits for every launch and every ``grid``."""
    global SPARSE_CALLS
    dev = fm.val.device
    buf = torch.zeros((k, d + 1), dtype=torch.float64, device=dev)
    n = fm.nrows
    if n == 0:
        return buf
    if idx.dtype != torch.int32 or int(idx.numel()) != n or not idx.is_contiguous():
        raise ValueError("idx must be a contiguous int32 [n] tensor")
    if counts is None:
        counts = torch.bincount(idx.to(torch.int64), minlength=k)
    buf[:, d] = counts[:k].to(torch.float64)
    csc = prepare(fm, d)
    if csc.nwork == 0:
        return buf
    kpad = csr.kp(k)
    sumT = torch.zeros((d, kpad), dtype=torch.float64, device=dev)
    part = torch.empty((max(csc.nslots, 1), kpad), dtype=torch.float64, device=dev)
    _lib.call("alink_kmeans_sparse_accum", csc.rows.data_ptr(), csc.vals.data_ptr(), idx.data_ptr(), csc.nwork,
              csc.wcol.data_ptr(), csc.wstart.data_ptr(), csc.wlen.data_ptr(), csc.wslot.data_ptr(), csc.nmulti,
              csc.mcol.data_ptr(), csc.mfirst.data_ptr(), csc.mcount.data_ptr(), kpad, sumT.data_ptr(),
              part.data_ptr(), int(grid), _lib.stream_ptr(dev))
    SPARSE_CALLS += 1
    buf[:, :d] = sumT[:, :k].t()
    return buf


def assign_accumulate(fm, C: torch.Tensor, dist_type: str, grid: int = 0) -> torch.Tensor:
    """The Lloyd step's ``[k, d+1]`` fp64 buffer ``[sum_x | count]`` for this rank's sparse rows."""
    k, d = C.shape
    if csr.use_hip(fm):
        idx, _, counts = nearest_hip(fm, C, dist_type, True, False, True, grid)
        return accumulate_hip(fm, idx, k, d, counts, grid)
    return assign_accumulate_torch(fm, C, dist_type)
