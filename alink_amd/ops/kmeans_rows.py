"""KMeans rows: which kernel family serves one rank's rows, decided once per run.

``rows(X, dist_type)`` wraps a rank's rows in the object that initialisation, the Lloyd queue and prediction ask
everything of (``models/clustering/kmeans.py``).  The kind is chosen there and nowhere else; ``ALINK_KMEANS_DENSE64``
and the kernel library's availability are read there:

* CSR rows (a sparse ``FeatureMatrix``, from a sparse vector column that ``sparse_selected`` takes):
  ``ops/kmeans_sparse.py`` assigns and sums them in fp64, EUCLIDEAN and COSINE; only candidate rows are densified.
* bf16 GPU rows, d in {64, 128, 256}, EUCLIDEAN: the MFMA nearest-centroid kernels of ``ops/kmeans.py``
  (``csrc/kmeans_nearest.hip``) for the k-means|| passes, one streaming pass for the first cost.
* fp64 GPU rows, 1 <= d <= 1024 (an ordinary vector column, ``VectorAssembler`` output), EUCLIDEAN and COSINE:
  ``ops/kmeans_dense64.py``, exact fp64 without float atomics; ``ALINK_KMEANS_DENSE64=0`` turns it off.
* anything else (CPU rows, fp32 rows, HAVERSINE, an empty partition): chunked ``pairwise_distance`` in torch.

The Lloyd step of every tensor kind is ``ops.kmeans.assign_accumulate``, the one ladder over dense tensors: that
choice depends on k.  With a GPU present a missing kernel library raises, unless ``ALINK_ALLOW_TORCH_FALLBACK=1``.
Distances are FastDistance values (EUCLIDEAN: the plain distance, COSINE: ``1 - x.c``); the callers normalise.

BisectingKMeans asks the same objects for its two steps: ``descend(table, slot, levels)`` compares every row with
the split plane of its own tree node (``ops/bisecting.py``) and ``child_stats(slot, nslots)`` sums the rows per
child.  fp64 GPU rows and CSR GPU rows take the HIP kernels; every other kind keeps the torch arithmetic.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, bisecting as bops, csr, kmeans as kops, kmeans_dense64 as kd64, kmeans_sparse as ksp
from .kmeans_sparse import sparse_selected  # noqa: F401  (the selection rule of sparse columns, for the callers)

__all__ = ["rows", "Rows", "column_kind", "sparse_selected", "sparse_rows", "pairwise_distance"]

CHUNK = 1 << 20         # rows per chunk of the torch distances
SPARSE_CHUNK = 1 << 16  # rows per chunk of the CSR product behind the [n, k] distances
SPARSE, DENSE, UNDECIDED = 1, 0, -1     # column_kind


def pairwise_distance(X: torch.Tensor, C: torch.Tensor, distance_type: str) -> torch.Tensor:
    """[n, k] FastDistance values (EUCLIDEAN: sqrt|x-c|^2, COSINE: 1 - x.c on normalised inputs,
    HAVERSINE: great-circle km on (lat, lon) degrees)."""
    dt = distance_type.upper()
    if dt == "COSINE":
        return 1.0 - X @ C.T
    if dt == "HAVERSINE":
        lat1 = torch.deg2rad(X[:, 0:1])
        lon1 = torch.deg2rad(X[:, 1:2])
        lat2 = torch.deg2rad(C[:, 0])[None, :]
        lon2 = torch.deg2rad(C[:, 1])[None, :]
        a = torch.sin((lat2 - lat1) / 2) ** 2 + torch.cos(lat1) * torch.cos(lat2) * torch.sin((lon2 - lon1) / 2) ** 2
        return 2 * 6371.0 * torch.asin(torch.sqrt(a.clamp(0, 1)))
    xn = (X * X).sum(1, keepdim=True)
    cn = (C * C).sum(1)[None, :]
    return torch.sqrt((xn + cn - 2.0 * (X @ C.T)).abs())


def column_kind(values) -> int:
    """What a vector column's values are: ``DENSE`` (a tensor block, dense vectors or dense vector strings),
    ``SPARSE`` (a ``SparseBlock``, sparse vectors or sparse vector strings) or ``UNDECIDED`` (no row to tell by)."""
    from ..common.linalg import SparseBlock, SparseVector
    if isinstance(values, torch.Tensor):
        return DENSE
    if isinstance(values, SparseBlock):
        return SPARSE
    first = next((x for x in values if x is not None), None)
    if first is None:
        return UNDECIDED
    return int(isinstance(first, SparseVector) or (isinstance(first, str) and ("$" in first or ":" in first)))


class Rows:
    """One rank's rows under one distance type: ``n``, ``d``, ``device``; ``fused_update``, whether the fused HIP
    centroid update (it prepares the dense assign kernel's operands) may follow their Lloyd step.  Every kind has
    ``take(idx)`` -> rows as a dense fp64 block [m, d] (candidate centroids), ``distances(C)`` -> fp64 [n, k], and
    ``nearest(C, dist_all=None)`` -> (idx int64 [n], distance fp64 [n]) of every row's nearest centroid; where that
    is the row minimum of ``dist_all``, the caller's ``distances(C)``, it is read from there: no pass over the rows."""
    fused_update = True
    n = property(lambda self: len(self.X))
    device = property(lambda self: self.X.device)

    def __init__(self, X, dist_type: str):
        self.X, self.dist_type = X, dist_type

    def first_cost(self, c: torch.Tensor):
        """The first k-means|| cost, against the single centre ``c`` [1, d]: (cost fp64 [n], its local total)."""
        cost = self.nearest(c)[1]
        return cost, cost.sum()

    def nearest_counts(self, C: torch.Tensor) -> torch.Tensor:
        """int64 [m]: the rows per nearest centroid (the k-means|| weights pass)."""
        return torch.bincount(self.nearest(C)[0], minlength=C.shape[0])

    def assign_accumulate(self, C: torch.Tensor, step: int) -> torch.Tensor:
        """The Lloyd step's [k, d+1] fp64 buffer ``[sum_x | count]`` at superstep ``step``; an empty partition
        launches nothing."""
        if self.n == 0:
            return torch.zeros((C.shape[0], C.shape[1] + 1), dtype=torch.float64, device=C.device)
        return self._assign_accumulate(C, step)

    def queue_assign(self, k: int):
        """``launch(C, step, skip)``, which queues superstep ``step``'s fused assign kernel ahead of time, or None."""
        return None

    def descend(self, table, slot: torch.Tensor, levels: int, grid: int = 0) -> torch.Tensor:
        """The rows' tree slots (int32 [n]) after up to ``levels`` levels down ``table`` (``ops.bisecting.tree_table``)
        from ``slot``: a row whose slot descends goes left iff its plane says so (equality and NaN go right), any
        other row keeps its slot.  The HIP kinds move ``slot`` in place and return it.  An empty partition launches
        nothing."""
        if self.n == 0 or levels <= 0 or table.P == 0:
            return slot
        return self._descend(table, slot, int(levels), grid)

    def child_stats(self, slot: torch.Tensor, nslots: int, sqnorm: bool = True, grid: int = 0,
                    work=None) -> torch.Tensor:
        """fp64 ``[nslots, d + 2] = [sum_x | count | sum |x|^2]`` of the rows per slot; rows whose slot is outside
        ``[0, nslots)`` add nothing.  ``sqnorm=False`` may leave the last column zero (only the EUCLIDEAN cost reads
        it).  An empty partition launches nothing.  ``work``: the sorted work list of these slots
        (``kmeans_dense64.sorted_work(slot, nslots, ignore_outside=True)``) where the caller has it already; the
        HIP kinds then do not sort again, the torch kinds never sort."""
        if self.n == 0:
            return torch.zeros((int(nslots), self.d + 2), dtype=torch.float64, device=slot.device)
        return self._child_stats(slot, int(nslots), sqnorm, grid, work)

    def row_sqnorm(self) -> torch.Tensor:
        """|x|^2 per row, fp64 [n], computed once per rows object."""
        if getattr(self, "_sqnorm", None) is None:
            self._sqnorm = self._row_sqnorm()
        return self._sqnorm


def _torch_go_left(dots, L: torch.Tensor, R: torch.Tensor, cosine: bool) -> torch.Tensor:
    """bool [n, m]: the comparison of the torch kinds, from the children's centres L, R [m, d] and ``dots(M)`` =
    ``X @ M.T``: exactly the expressions BisectingKMeans always evaluated."""
    if cosine:
        dl = 1.0 - dots(L / L.norm(dim=1, keepdim=True))
        dr = 1.0 - dots(R / R.norm(dim=1, keepdim=True))
        return dl < dr
    V = R - L
    mid = 0.5 * (R + L)
    length = (mid * V).sum(1)
    return dots(V) < length[None, :]


def _torch_descend(dots, table, slot: torch.Tensor, levels: int) -> torch.Tensor:
    """``Rows.descend`` through [n, P] products: every descending slot's plane against every row, one column kept."""
    dev = slot.device
    L, R = torch.as_tensor(table.lc, device=dev), torch.as_tensor(table.rc, device=dev)
    left, right = table.left.to(torch.int64), table.right.to(torch.int64)
    go_left = None
    for _ in range(levels):
        s = slot.to(torch.int64)
        inside = (s >= 0) & (s < table.S)
        sc = torch.where(inside, s, torch.zeros_like(s))
        has = inside & (left[sc] >= 0)
        which = torch.where(has, sc, torch.zeros_like(sc))      # the descending slots are 0 .. P-1
        if go_left is None:     # the planes do not change between the levels
            go_left = _torch_go_left(dots, L, R, table.cosine)
        gl = go_left.gather(1, which[:, None])[:, 0]
        slot = torch.where(has, torch.where(gl, left[sc], right[sc]), s).to(torch.int32)
    return slot


class _SparseRows(Rows):
    """CSR rows on ``ops/kmeans_sparse.py``."""
    fused_update = False
    d = property(lambda self: int(self.X.ncols))

    def take(self, idx: torch.Tensor) -> torch.Tensor:
        return ksp.take_dense(self.X, idx)

    def nearest(self, C, dist_all=None):
        idx, d2 = ksp.nearest(self.X, C, self.dist_type)
        return idx, (d2.sqrt_() if self.dist_type == "EUCLIDEAN" else d2)      # the kernel's squared distance

    def nearest_counts(self, C):
        return ksp.nearest_counts(self.X, C, self.dist_type)

    def _assign_accumulate(self, C, step):
        return ksp.assign_accumulate(self.X, C, self.dist_type)

    def _dot_chunks(self, C: torch.Tensor):
        """Yields (first row, ``X[s:e] @ C.T`` fp64 [m, k]) in row chunks of the CSR product."""
        fm, d = self.X, self.d
        col, val = csr.clipped(fm, d)
        safe = sparse_view(fm, d, val)
        safe.col = col
        Ct = C.t().contiguous()
        for s in range(0, fm.nrows, SPARSE_CHUNK):
            yield s, safe[s:s + SPARSE_CHUNK].mm(Ct)

    def distances(self, C: torch.Tensor) -> torch.Tensor:
        """[n, k] fp64 distances, in row chunks of the CSR product (the result is the only dense block)."""
        fm, d = self.X, self.d
        cn = (C * C).sum(1)[None, :]
        xn = ksp.row_sqnorm(fm, d)
        parts = []
        for s, dot in self._dot_chunks(C):
            parts.append(1.0 - dot if self.dist_type == "COSINE" else
                         torch.sqrt((xn[s:s + SPARSE_CHUNK, None] + cn - 2.0 * dot).abs()))
        return torch.cat(parts) if parts else torch.zeros((0, C.shape[0]), dtype=torch.float64, device=fm.device)

    def _row_sqnorm(self):
        return ksp.row_sqnorm(self.X, self.d)

    def _descend(self, table, slot, levels, grid):
        if csr.use_hip(self.X):
            return bops.descend_csr(self.X, table, slot, levels, grid)
        return _torch_descend(lambda M: torch.cat([dot for _, dot in self._dot_chunks(M)]), table, slot, levels)

    def _child_stats(self, slot, nslots, sqnorm, grid, work=None):
        fm, d = self.X, self.d
        buf = torch.zeros((nslots, d + 2), dtype=torch.float64, device=fm.device)
        idx = torch.where((slot >= 0) & (slot < nslots), slot, torch.full_like(slot, -1)).to(torch.int32)
        counts = torch.bincount(idx.to(torch.int64) + 1, minlength=nslots + 1)[1:]
        if csr.use_hip(fm):
            buf[:, :d + 1] = ksp.accumulate_hip(fm, idx.contiguous(), nslots, d, counts, grid)
            if sqnorm:      # the per-row norms through the dense accumulate at d = 1: no float atomics here either
                sq = self.row_sqnorm()[:, None]
                buf[:, d + 1] = (kd64.accumulate(sq, idx, nslots, grid, ignore_outside=True) if work is None else
                                 kd64.accumulate_work(sq, work, nslots, grid))[:, 0]
            return buf
        key = torch.where(idx >= 0, idx, torch.full_like(idx, nslots)).to(torch.int64)      # a spare last slot
        buf[:, :d + 1] = ksp.accumulate_torch(fm, key, nslots + 1, d)[:nslots]
        buf[:, d + 1] = torch.zeros(nslots + 1, dtype=torch.float64, device=fm.device).index_add_(
            0, key, self.row_sqnorm())[:nslots]
        return buf


def sparse_view(fm, ncols: int, val: Optional[torch.Tensor] = None):
    """The same CSR arrays as ``fm`` (or other values) under ``ncols`` columns, as a new FeatureMatrix."""
    from ..models.common.features import FeatureMatrix
    return FeatureMatrix(crow=fm.crow, col=fm.col, val=fm.val if val is None else val, ncols=int(ncols))


def sparse_rows(fm, d: int, dist_type: str):
    """CSR rows as the sparse kind takes them: fp64 values under ``d`` columns (the global vector size: an empty
    partition knows none) and, for COSINE, scaled by the row norm over the columns inside [0, d); zero rows stay."""
    fm = sparse_view(fm, d, fm.val.to(torch.float64))
    if dist_type.upper() != "COSINE" or fm.nrows == 0 or fm.val.numel() == 0:
        return fm
    nrm = ksp.row_sqnorm(fm, d).sqrt_()
    nrm = torch.where(nrm > 0, nrm, torch.ones_like(nrm))
    return sparse_view(fm, d, fm.val / nrm[fm.row_ids()])


class _TorchRows(Rows):
    """Tensor rows on chunked ``pairwise_distance``; the base of the tensor kinds."""
    d = property(lambda self: int(self.X.shape[1]) if self.X.dim() == 2 else 1)

    def take(self, idx: torch.Tensor) -> torch.Tensor:
        return self.X.index_select(0, idx).to(torch.float64)

    def _chunks(self, C):
        Cf = C.to(torch.float32 if self.X.dtype in (torch.bfloat16, torch.float16) else self.X.dtype)
        for s in range(0, max(self.n, 1), CHUNK):       # an empty partition: one empty chunk
            yield pairwise_distance(self.X[s:s + CHUNK].to(Cf.dtype), Cf, self.dist_type)

    def distances(self, C: torch.Tensor) -> torch.Tensor:
        """[n, k] fp64 distances, computed in the rows' precision (fp32 for bf16 / fp16 rows)."""
        return torch.cat([dist.double() for dist in self._chunks(C)])

    def nearest(self, C, dist_all=None):
        best = [dist.min(1) for dist in ([dist_all] if dist_all is not None else self._chunks(C))]
        return torch.cat([b.indices for b in best]), torch.cat([b.values.to(torch.float64) for b in best])

    def _assign_accumulate(self, C, step):
        return kops.assign_accumulate(self.X, C, reverse=kops.serpentine_reverse(step))

    def _row_sqnorm(self):
        return (self.X * self.X).sum(1)

    def _descend(self, table, slot, levels, grid):
        return _torch_descend(lambda M: self.X @ M.T, table, slot, levels)

    def _child_stats(self, slot, nslots, sqnorm, grid, work=None):
        # segment sums as one [m, n] x [n, d + 2] GEMM over the rows that have a slot
        from .gemm import tn_matmul
        X, d = self.X, self.d
        ok = (slot >= 0) & (slot < nslots)
        Xs, ps = X[ok], slot[ok].to(torch.int64)
        norm2 = self.row_sqnorm()[ok]
        onehot = torch.nn.functional.one_hot(ps, nslots).to(X.dtype)
        return torch.zeros((nslots, d + 2), dtype=torch.float64, device=X.device) + tn_matmul(
            onehot, torch.cat([Xs, torch.ones_like(norm2)[:, None], norm2[:, None]], 1))

    def queue_assign(self, k):
        if not kops.hip_supported(self.X, k):       # never an empty partition
            return None
        return lambda C, step, skip: kops.assign_accumulate_hip(self.X, C, reverse=kops.serpentine_reverse(step),
                                                                skip=skip)


class _Bf16Rows(_TorchRows):
    """bf16 GPU rows on the nearest-centroid kernels of ``ops/kmeans.py`` (EUCLIDEAN)."""

    def nearest(self, C, dist_all=None):
        if C.shape[0] == 1:     # one new centre: one streaming pass, fp64 distances straight out
            return torch.zeros(1, dtype=torch.int64, device=self.device).expand(self.n), kops.cost1_hip(self.X, C[0])
        idx, d2 = kops.nearest_hip(self.X, C)
        return idx.to(torch.int64), d2.to(torch.float64).sqrt_()

    def first_cost(self, c):
        # the pass also leaves per-wave sums: the threshold's total without a second pass over the cost
        cost, psum = kops.cost1_hip(self.X, c[0], with_sum=True)
        return cost, psum.sum()

    def nearest_counts(self, C):
        return kops.nearest_counts_hip(self.X, C)      # one pass, no per-row output


class _Dense64Rows(_TorchRows):
    """fp64 GPU rows on ``ops/kmeans_dense64.py`` (EUCLIDEAN / COSINE)."""

    def nearest(self, C, dist_all=None):
        if dist_all is not None:
            return super().nearest(C, dist_all)
        idx, d2 = kd64.nearest(self.X, C, self.dist_type)
        return idx, (d2.sqrt_() if self.dist_type == "EUCLIDEAN" else d2)      # the kernel's squared distance

    def nearest_counts(self, C):
        return kd64.nearest_counts(self.X, C, self.dist_type)

    def _descend(self, table, slot, levels, grid):
        if kd64.use_hip(self.X, 1):
            return bops.descend_f64(self.X, table, slot, levels, grid)
        return super()._descend(table, slot, levels, grid)

    def _child_stats(self, slot, nslots, sqnorm, grid, work=None):
        if not kd64.use_hip(self.X, nslots):
            return super()._child_stats(slot, nslots, sqnorm, grid)
        # one stable sort of the slots serves both accumulates; rows without a slot sort last and are not read
        X, d = self.X, self.d
        if work is None:
            work = kd64.sorted_work(slot, nslots, ignore_outside=True)
        buf = torch.zeros((nslots, d + 2), dtype=torch.float64, device=X.device)
        buf[:, :d + 1] = kd64.accumulate_work(X, work, nslots, grid)
        if sqnorm:
            buf[:, d + 1] = kd64.accumulate_work(self.row_sqnorm()[:, None], work, nslots, grid)[:, 0]
        return buf


def rows(X, dist_type: str) -> Rows:
    """The rows object of one rank's rows ``X``: a tensor [n, d], a ``FeatureMatrix``, or such an object itself."""
    dt = dist_type.upper()
    if isinstance(X, Rows):
        return X
    if not isinstance(X, torch.Tensor):
        if not X.is_sparse:
            return rows(X.dense, dt)
        if dt not in ("EUCLIDEAN", "COSINE"):
            raise ValueError(f"sparse KMeans supports EUCLIDEAN and COSINE, not {dist_type}")
        return _SparseRows(X, dt)
    if dt == "EUCLIDEAN" and kops.nearest_supported(X) and _lib.kernels_enabled():
        return _Bf16Rows(X, dt)
    # an empty partition launches nothing and stays on the torch kind
    if dt in ("EUCLIDEAN", "COSINE") and X.shape[0] > 0 and kd64.dense64_selected(X, 1):
        return _Dense64Rows(X, dt)
    return _TorchRows(X, dt)
