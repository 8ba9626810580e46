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
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, kmeans as kops, kmeans_dense64 as kd64, kmeans_sparse as ksp
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

    def distances(self, C: torch.Tensor) -> torch.Tensor:
        """[n, k] fp64 distances, in row chunks of the CSR product (the result is the only dense block)."""
        fm, d = self.X, self.d
        col, val = ksp._clipped(fm, d)
        safe = sparse_view(fm, d, val)
        safe.col = col
        Ct = C.t().contiguous()
        cn = (C * C).sum(1)[None, :]
        xn = ksp.row_sqnorm(fm, d)
        parts = []
        for s in range(0, fm.nrows, SPARSE_CHUNK):
            dot = safe[s:s + SPARSE_CHUNK].mm(Ct)
            parts.append(1.0 - dot if self.dist_type == "COSINE" else
                         torch.sqrt((xn[s:s + SPARSE_CHUNK, None] + cn - 2.0 * dot).abs()))
        return torch.cat(parts) if parts else torch.zeros((0, C.shape[0]), dtype=torch.float64, device=fm.device)


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
    if dt == "EUCLIDEAN" and kops.nearest_supported(X):
        if _lib.available():
            return _Bf16Rows(X, dt)
        if not _lib.torch_fallback_allowed():
            _lib.require()      # raises: no quiet fall-back on a GPU
    # an empty partition launches nothing and stays on the torch kind
    if dt in ("EUCLIDEAN", "COSINE") and X.shape[0] > 0 and kd64.dense64_selected(X, 1):
        return _Dense64Rows(X, dt)
    return _TorchRows(X, dt)
