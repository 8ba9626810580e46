"""Locality-sensitive hashing on the device: table hashes and pair distances (``csrc/lsh.hip``), and the bucket join
and top-N selection around them in torch.

The host path of ``models/similarity/lsh.py`` is the CPU path and the oracle: ``minhash_tables`` equals
``MinHashLSH.hash``, ``pair_jaccard`` equals ``MinHashLSH.distance`` bit for bit, ``candidate_pairs`` equals
``_candidates`` and ``top_n`` the loop of ``approx_nearest_neighbors``.  Rows are a dense fp64 block or the
canonical CSR rows of ``canonical_csr`` (no zero values, strictly ascending columns); neither is ever densified,
and every kernel result depends on the rows alone, never on the launch or its ``grid``.

``device_selected(device)`` decides whether the operators take this path: a CUDA device and
``_lib.kernels_enabled()`` (no quiet fall-back); ``ALINK_LSH_HIP=0`` turns it off.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["CsrRows", "device_selected", "canonical_csr", "minhash_tables", "brp_tables", "pair_jaccard",
           "pair_euclidean", "candidate_pairs", "top_n", "LSH_CALLS", "PAIR_BUDGET", "MAX_COL"]

LSH_CALLS = 0           # launches of the HIP LSH kernels (tests read it)
PAIR_BUDGET = 2 ** 26   # candidate pairs one chunk of queries may expand to before ``unique``
MAX_COL = 2 ** 31 - 1   # MinHash takes (1 + col) in 32 bits as the reference does: columns stay below this


class CsrRows(NamedTuple):
    """Canonical CSR rows: ``crow`` int64 [n + 1], ``col`` int64 [nnz] strictly ascending inside a row, ``val`` fp64
    [nnz] without zeros, under ``ncols`` columns."""
    crow: torch.Tensor
    col: torch.Tensor
    val: torch.Tensor
    ncols: int

    @property
    def nrows(self) -> int:
        return int(self.crow.shape[0]) - 1

    @property
    def nnz(self) -> int:
        return int(self.col.shape[0])

    @property
    def device(self):
        return self.val.device


def device_selected(device) -> bool:
    """True when the LSH operators run on the device: a CUDA device, not switched off by ``ALINK_LSH_HIP=0``, and
    the kernel library by the one fall-back rule (``_lib.kernels_enabled``: a missing library is an error)."""
    if torch.device(device).type != "cuda" or os.environ.get("ALINK_LSH_HIP", "1") == "0":
        return False
    return _lib.kernels_enabled()


def _crow_of(rid: torch.Tensor, n: int) -> torch.Tensor:
    crow = torch.zeros(n + 1, dtype=torch.int64, device=rid.device)
    if rid.numel():
        crow[1:] = torch.cumsum(torch.bincount(rid, minlength=n), 0)
    return crow


def canonical_csr(fm) -> Optional[CsrRows]:
    """The rows of a ``FeatureMatrix`` as canonical CSR on its device, or None when they are not device-eligible
    (a column index twice in a row, a column outside ``[0, 2^31 - 1)``, or more than ``2^31 - 1`` columns): the
    caller then takes the host path.  Entries with ``val == 0`` are dropped (``NaN != 0`` stays), the rule of the
    host path's ``_Rows``; a dense block becomes CSR through ``nonzero``; rows are sorted only if one is found
    out of order."""
    if int(fm.ncols) > MAX_COL:
        return None
    n = fm.nrows
    if not fm.is_sparse:
        X = fm.dense.to(torch.float64)
        nz = X != 0
        idx = nz.nonzero()
        return CsrRows(_crow_of(idx[:, 0], n), idx[:, 1].contiguous(), X[nz], int(fm.ncols))
    col, val = fm.col.to(torch.int64), fm.val.to(torch.float64)
    counts = fm.crow[1:] - fm.crow[:-1]
    rid = torch.repeat_interleave(torch.arange(n, device=val.device), counts, output_size=int(col.numel()))
    crow = fm.crow.to(torch.int64)
    keep = val != 0
    if not bool(keep.all()):
        rid, col, val = rid[keep], col[keep], val[keep]
        crow = _crow_of(rid, n)
    if col.numel():
        if int(col.min()) < 0 or int(col.max()) >= MAX_COL:
            return None
        same = rid[1:] == rid[:-1]
        if bool((same & (col[1:] <= col[:-1])).any()):
            o = torch.argsort(col, stable=True)
            o = o[torch.argsort(rid[o], stable=True)]       # by (row, col)
            col, val = col[o], val[o]
            if bool((same & (col[1:] == col[:-1])).any()):
                return None
    return CsrRows(crow.contiguous(), col.contiguous(), val.contiguous(), int(fm.ncols))


def _ran() -> None:
    global LSH_CALLS
    LSH_CALLS += 1


def _check_csr(rows: CsrRows, what: str) -> None:
    if not (rows.val.is_cuda and rows.crow.dtype == torch.int64 and rows.col.dtype == torch.int64
            and rows.val.dtype == torch.float64 and rows.crow.is_contiguous() and rows.col.is_contiguous()
            and rows.val.is_contiguous() and rows.col.numel() == rows.val.numel() and rows.crow.numel() >= 1
            and rows.crow.device == rows.val.device and rows.col.device == rows.val.device):
        raise ValueError(f"{what}: canonical CSR rows (int64 crow / col, fp64 val, contiguous) on a GPU are needed")


def _check_pairs(pa: torch.Tensor, pb: torch.Tensor, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    if pa.dtype != torch.int64 or pb.dtype != torch.int64 or pa.dim() != 1 or pa.shape != pb.shape \
            or pa.device != dev or pb.device != dev:
        raise ValueError("the pair lists must be int64 [m] tensors on the rows' device")
    return pa.contiguous(), pb.contiguous()


def minhash_tables(rows: CsrRows, A, B, grid: int = 0) -> torch.Tensor:
    """int32 [n, T] MinHash table hashes of canonical CSR rows on a GPU for the coefficients ``A``, ``B`` [T, P]
    (``MinHashLSH.A`` / ``.B``): equal to ``MinHashLSH.hash``."""
    _check_csr(rows, "minhash_tables")
    A, B = np.asarray(A, dtype=np.int64), np.asarray(B, dtype=np.int64)
    if A.ndim != 2 or A.shape != B.shape or A.size == 0 or min(A.min(), B.min()) < 0 or max(A.max(), B.max()) >= 2 ** 31:
        raise ValueError("minhash_tables: A and B must be [T, P] coefficients in [0, 2^31)")
    T, P = A.shape
    dev, n = rows.device, rows.nrows
    out = torch.empty((n, T), dtype=torch.int32, device=dev)
    if n == 0:
        return out
    if rows.nnz == 0:       # only empty rows: every function keeps the prime, nothing to read
        from ..models.similarity.lsh import HASH_PRIME, murmur3_32_words
        h = int(murmur3_32_words(np.full((1, P), HASH_PRIME, dtype=np.int64))[0])
        return out.fill_(h)
    a = torch.from_numpy(A.astype(np.int32).reshape(-1)).to(dev)
    b = torch.from_numpy(B.astype(np.int32).reshape(-1)).to(dev)
    _lib.call("alink_lsh_minhash", rows.crow.data_ptr(), rows.col.data_ptr(), rows.val.data_ptr(), n, a.data_ptr(),
              b.data_ptr(), T, P, out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    _ran()
    return out


def brp_tables(dots: torch.Tensor, r, width: float, num_tables: int, grid: int = 0) -> torch.Tensor:
    """int32 [n, T] bucket-random-projection table hashes of the projections ``dots`` fp64 [n, T * P] on a GPU with
    offsets ``r`` [T * P] and bucket width ``width``: murmur over the low 32 bits of
    ``(int64) floor((dot + r) / width)``, a true fp64 division.  Non-finite projections, and quotients outside the
    int64 range, are not guaranteed to hash as on the host."""
    if not (dots.is_cuda and dots.dtype == torch.float64 and dots.dim() == 2 and dots.is_contiguous()):
        raise ValueError("brp_tables: contiguous fp64 [n, T * P] projections on a GPU are needed")
    n, F = dots.shape
    T = int(num_tables)
    if T < 1 or F < T or F % T or not float(width) > 0:
        raise ValueError("brp_tables: T * P columns and a positive width are needed")
    r = torch.as_tensor(np.asarray(r, dtype=np.float64).reshape(-1)).to(dots.device)
    if int(r.numel()) != F:
        raise ValueError("brp_tables: one offset per projection is needed")
    out = torch.empty((n, T), dtype=torch.int32, device=dots.device)
    if n == 0:
        return out
    _lib.call("alink_lsh_brp_hash", dots.data_ptr(), n, r.data_ptr(), float(width), T, F // T, out.data_ptr(),
              int(grid), _lib.stream_ptr(dots.device))
    _ran()
    return out


def pair_jaccard(a: CsrRows, b: CsrRows, pa: torch.Tensor, pb: torch.Tensor, grid: int = 0) -> torch.Tensor:
    """fp64 [m] Jaccard distances of the index sets of rows ``pa`` of ``a`` and ``pb`` of ``b``, bit-equal to
    ``jaccard_distance_sets``.  A pair with an index outside its matrix gets NaN."""
    _check_csr(a, "pair_jaccard")
    _check_csr(b, "pair_jaccard")
    pa, pb = _check_pairs(pa, pb, a.device)
    m = int(pa.numel())
    out = torch.empty(m, dtype=torch.float64, device=a.device)
    if m == 0:
        return out
    if a.nnz == 0 and b.nnz == 0:       # only empty rows on both sides: every distance is 0, nothing to read
        return out.zero_()
    _lib.call("alink_lsh_pair_jaccard", a.crow.data_ptr(), a.col.data_ptr(), a.nrows, a.nnz, b.crow.data_ptr(),
              b.col.data_ptr(), b.nrows, b.nnz, pa.data_ptr(), pb.data_ptr(), m, out.data_ptr(), int(grid),
              _lib.stream_ptr(a.device))
    _ran()
    return out


def pair_euclidean(a, b, pa: torch.Tensor, pb: torch.Tensor, grid: int = 0) -> torch.Tensor:
    """fp64 [m] Euclidean distances of rows ``pa`` of ``a`` and ``pb`` of ``b``: two ``CsrRows`` (the sum runs over
    the union of the two rows' entries) or two contiguous fp64 [., d] GPU blocks of one ``d >= 1``.  The lanes per
    pair are fixed for the call (from ``d``; from the two matrices' mean row length), so a distance depends on its
    two rows alone; identical rows give exactly 0.  A pair with an index outside its matrix gets NaN."""
    if isinstance(a, CsrRows) != isinstance(b, CsrRows):
        raise ValueError("pair_euclidean: both sides dense or both sides CSR")
    if isinstance(a, CsrRows):
        _check_csr(a, "pair_euclidean")
        _check_csr(b, "pair_euclidean")
        dev = a.device
    else:
        for x in (a, b):
            if not (x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and x.is_contiguous()):
                raise ValueError("pair_euclidean: contiguous fp64 [n, d] GPU rows are needed")
        if a.shape[1] != b.shape[1] or a.shape[1] < 1 or a.shape[1] >= 2 ** 31:
            raise ValueError("pair_euclidean: both sides need the same vector size d >= 1")
        dev = a.device
    pa, pb = _check_pairs(pa, pb, dev)
    m = int(pa.numel())
    out = torch.empty(m, dtype=torch.float64, device=dev)
    if m == 0:
        return out
    if isinstance(a, CsrRows):
        _lib.call("alink_lsh_pair_euclid_csr", a.crow.data_ptr(), a.col.data_ptr(), a.val.data_ptr(), a.nrows, a.nnz,
                  b.crow.data_ptr(), b.col.data_ptr(), b.val.data_ptr(), b.nrows, b.nnz, pa.data_ptr(),
                  pb.data_ptr(), m, out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    else:
        _lib.call("alink_lsh_pair_euclid_f64", a.data_ptr(), int(a.shape[0]), b.data_ptr(), int(b.shape[0]),
                  int(a.shape[1]), pa.data_ptr(), pb.data_ptr(), m, out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    _ran()
    return out


def candidate_pairs(ha: torch.Tensor, hb: torch.Tensor, budget: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Distinct pairs (a, b) with ``ha[a, t] == hb[b, t]`` in at least one table ``t``, sorted by (a, b), as two
    int64 tensors: ``_candidates`` of the host path, in torch on any device.  Per table ``hb[:, t]`` is sorted
    once and every ``ha[a, t]`` finds its run by two binary searches; runs are expanded for a chunk of queries
    whose runs hold at most ``budget`` pairs (default ``PAIR_BUDGET``; a single query is the smallest chunk),
    packed as ``a * m + b`` and made distinct by ``unique``."""
    n, T = ha.shape
    m = int(hb.shape[0])
    dev = ha.device
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    if n == 0 or m == 0 or T == 0:
        return empty, empty.clone()
    budget = PAIR_BUDGET if budget is None else int(budget)
    order, lo, cnt = [], [], []
    for t in range(T):
        srt, o = torch.sort(hb[:, t].contiguous(), stable=True)
        q = ha[:, t].contiguous()
        l = torch.searchsorted(srt, q, right=False)
        order.append(o)
        lo.append(l)
        cnt.append(torch.searchsorted(srt, q, right=True) - l)
    # per table a contiguous scan along its own [n]: one cumsum down the rows of an [n, T] block made the whole join
    # 25 times slower (profiles/lsh.txt)
    cum_t = torch.zeros((T, n + 1), dtype=torch.int64, device=dev)
    for t in range(T):
        torch.cumsum(cnt[t], 0, out=cum_t[t, 1:])
    cum = cum_t.sum(0)                                                  # pairs of the queries before each one
    keys = []
    start = 0
    while start < n:
        # the last query whose runs still fit the budget; the host reads the chunk's end and its T totals
        end = int(torch.searchsorted(cum, cum[start] + budget, right=True)) - 1
        end = min(max(end, start + 1), n)
        tot = (cum_t[:, end] - cum_t[:, start]).tolist()
        parts = []
        for t in range(T):
            if tot[t] == 0:
                continue
            c = cnt[t][start:end]
            a = torch.repeat_interleave(torch.arange(start, end, device=dev), c, output_size=tot[t])
            first = cum_t[t, start:end] - cum_t[t, start]               # where each query's run starts in the chunk
            pos = torch.arange(tot[t], device=dev) - first[a - start]
            parts.append(a * m + order[t][lo[t][a] + pos])
        if parts:
            keys.append(torch.unique(torch.cat(parts)))
        start = end
    if not keys:
        return empty, empty.clone()
    key = torch.cat(keys)                                               # chunks ascend in a: sorted as a whole
    a = torch.div(key, m, rounding_mode="floor")
    return a, key - a * m


def top_n(qi: torch.Tensor, di: torch.Tensor, dist: torch.Tensor, n: int):
    """(query, dict, distance, rank) of the ``n`` nearest candidates of every query, by query then rank from 1:
    the loop of ``approx_nearest_neighbors`` as two stable sorts (by distance, then by query).  The pairs come
    sorted by (query, dict), so equal distances keep the ascending dict index, as the host's stable sort does."""
    o = torch.argsort(dist, stable=True)
    o = o[torch.argsort(qi[o], stable=True)]
    q, d, x = qi[o], di[o], dist[o]
    rank = torch.arange(int(q.numel()), device=q.device) - torch.searchsorted(q, q, right=False) + 1
    keep = rank <= int(n)
    return q[keep], d[keep], x[keep], rank[keep]
