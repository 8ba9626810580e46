"""Dense fp64 KMeans: nearest centroid and per-cluster sums of fp64 rows ``[n, d]`` of any vector size, in fp64.

What an ordinary vector column is on the device (vector strings, ``DenseVector``s, ``VectorAssembler`` output):
a contiguous fp64 tensor whose d is whatever the data has — 4, 37, 100, 300, 768 — which none of the bf16 / fp32
kernels of ``ops/kmeans.py`` take.

* ``nearest(X, C, dist_type)`` -> ``(idx int64 [n], dist fp64 [n])``: ``dist`` is the SQUARED distance for
  EUCLIDEAN and ``1 - x.c`` for COSINE (rows and centroids normalised by the caller);
* ``nearest_counts(X, C, dist_type)`` -> exact int64 ``[k]`` counts (the k-means|| weights pass);
* ``accumulate(X, idx, k)`` -> the ``[k, d+1]`` fp64 buffer ``[sum_x | count]`` of ``ops/kmeans.py``;
* ``assign_accumulate(X, C)`` -> ``accumulate`` of the EUCLIDEAN ``nearest`` (the Lloyd step).

GPU: ``csrc/kmeans_dense64.hip`` — the scores ``x.c - |c|^2/2`` on the fp64 matrix cores
(``v_mfma_f64_16x16x4_f64``) with the centroids staged in LDS, an argmax that gives bit-equal scores to the lowest
index, and no ``[n, k]`` buffer anywhere; the sums through a stable sort of the rows by cluster, one wave per
(cluster, chunk of ``ACCUM_ROWS`` rows, 64-dim slice) adding rows in ascending order, chunk partials merged in chunk
order — no float atomics, bitwise identical from launch to launch and for every grid.
CPU (and the oracle of the tests): ``nearest_torch`` / ``assign_accumulate_torch``, chunked over rows.

``ALINK_KMEANS_DENSE64=0`` keeps fp64 rows on the torch path.  With a GPU present a missing kernel library raises,
unless ``ALINK_ALLOW_TORCH_FALLBACK=1``.
"""
from __future__ import annotations

import os
from typing import Tuple

import torch

from . import _lib
from .kmeans_sparse import DENSE_DMAX

__all__ = ["ACCUM_ROWS", "dense64_supported", "dense64_selected", "nearest", "nearest_counts", "accumulate",
           "assign_accumulate", "nearest_torch", "assign_accumulate_torch",
           # shared with ops/evalcluster.py, ops/sos.py, ops/gmm.py and ops/kmeans_rows.py (csrc/dense64_mfma.h)
           "use_hip", "tiles", "centroid_image", "sorted_work", "accumulate_work"]

ACCUM_ROWS = 256        # rows of one cluster that one wave sums; longer clusters are split and merged in order
DENSE64_CALLS = 0       # launches of the HIP dense fp64 path (tests read it)
TORCH_CHUNK = 1 << 14   # rows per chunk of the torch path
NT_MAX = 8              # centroid tiles of 16 per block of the nearest kernel (csrc/kmeans_dense64.hip)


def dense64_supported(X, k: int) -> bool:
    """Whether the HIP kernels take these rows: a contiguous fp64 [n, d] tensor on a GPU, 1 <= d <= DENSE_DMAX,
    n < 2^31, k >= 1."""
    return (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float64 and X.dim() == 2
            and X.is_contiguous() and 1 <= X.shape[1] <= DENSE_DMAX and X.shape[0] < 2 ** 31 and int(k) >= 1)


def dense64_selected(X, k: int) -> bool:
    """The selection rule: ``dense64_supported`` rows, unless ``ALINK_KMEANS_DENSE64=0``."""
    return dense64_supported(X, k) and os.environ.get("ALINK_KMEANS_DENSE64", "") != "0"


def use_hip(X: torch.Tensor, k: int) -> bool:
    """Whether these rows go to the HIP kernels of the dense fp64 tile loop (``csrc/dense64_mfma.h``): False on the
    CPU, an error for GPU rows the kernels do not take, else whether the kernel library is enabled."""
    if not X.is_cuda:
        return False
    if not dense64_supported(X, k):
        raise ValueError("dense fp64 KMeans on the GPU needs contiguous fp64 [n, d] rows with 1 <= d <= "
                         f"{DENSE_DMAX}, fewer than 2^31 rows and k >= 1")
    return _lib.kernels_enabled()


def _dist_code(dist_type: str) -> int:
    dt = dist_type.upper()
    if dt not in ("EUCLIDEAN", "COSINE"):
        raise ValueError(f"dense fp64 KMeans supports EUCLIDEAN and COSINE, not {dist_type}")
    return int(dt == "COSINE")


def _check(X: torch.Tensor, C: torch.Tensor) -> None:
    if X.dim() != 2 or C.dim() != 2 or C.shape[1] != X.shape[1] or C.shape[0] < 1:
        raise ValueError("centroid shape mismatch")


# ---------------------------------------------------------------------------------------------------
# torch path (CPU, oracle)
# ---------------------------------------------------------------------------------------------------
def nearest_torch(X: torch.Tensor, C: torch.Tensor, dist_type: str,
                  chunk: int = TORCH_CHUNK) -> Tuple[torch.Tensor, torch.Tensor]:
    """Torch reference of ``nearest``: (idx int64 [n], squared distance / 1 - x.c fp64 [n]).  The score is
    ``x.c - |c|^2/2`` and ``argmax`` takes the first of equal scores (and index 0 for an all-NaN row)."""
    cosine = _dist_code(dist_type)
    _check(X, C)
    n = X.shape[0]
    Cd = C.to(device=X.device, dtype=torch.float64)
    half = torch.zeros(Cd.shape[0], dtype=torch.float64, device=X.device) if cosine else 0.5 * (Cd * Cd).sum(1)
    idx = torch.zeros(n, dtype=torch.int64, device=X.device)
    dist = torch.zeros(n, dtype=torch.float64, device=X.device)
    for s in range(0, n, chunk):
        xc = X[s:s + chunk].to(torch.float64)
        sc = xc @ Cd.T - half
        bi = sc.argmax(1)
        best = sc.gather(1, bi[:, None])[:, 0]
        idx[s:s + chunk] = bi
        dist[s:s + chunk] = 1.0 - best if cosine else ((xc * xc).sum(1) - 2.0 * best).clamp_min(0.0)
    return idx, dist


def _accumulate_torch(X: torch.Tensor, idx: torch.Tensor, k: int) -> torch.Tensor:
    n, d = X.shape
    buf = torch.zeros((k, d + 1), dtype=torch.float64, device=X.device)
    if n == 0:
        return buf
    idx = idx.to(torch.int64)
    buf[:, :d].index_add_(0, idx, X.to(torch.float64))
    buf[:, d] = torch.bincount(idx, minlength=k).to(torch.float64)
    return buf


def assign_accumulate_torch(X: torch.Tensor, C: torch.Tensor, chunk: int = TORCH_CHUNK) -> torch.Tensor:
    """Torch reference of ``assign_accumulate``: [k, d+1] fp64 ``[sum_x | count]`` of the nearest-centroid
    assignment; on the CPU every (cluster, dim) sum runs in ascending row order."""
    return _accumulate_torch(X, nearest_torch(X, C, "EUCLIDEAN", chunk)[0], C.shape[0])


# ---------------------------------------------------------------------------------------------------
# HIP path
# ---------------------------------------------------------------------------------------------------
def tiles(k: int) -> int:
    """Tiles of 16 table rows per block of the image (NT of ``csrc/dense64_mfma.h``): the power of two that covers
    k, at most NT_MAX."""
    nt = 1
    while nt < NT_MAX and 16 * nt < k:
        nt *= 2
    return nt


def centroid_image(C: torch.Tensor, cosine: int, dev):
    """The lane-ordered image of the table ``C`` [k, d] that every kernel of the dense fp64 tile loop stages in LDS;
    the layout and the operand maps it serves are described once, in ``csrc/dense64_mfma.h``.  Returns
    ``(img, ninit, nt, nblk)``: the rows zero-padded to ``nblk`` whole blocks of 16 ``nt = tiles(k)`` rows and whole
    chunks of 32 dims, img [nblk, ndch, u = 2, nt, g = 4, m = 16, s = 4] where the element is row
    ``(blk * nt + t) * 16 + m``, dim ``dch * 32 + 16 u + 4 g + s``; and the accumulator start
    ninit [nblk * 16 nt] = -|c|^2/2 (0 for COSINE, ``cosine = 1``, and on the padded slots)."""
    k, d = C.shape
    nt = tiles(k)
    nblk = (k + 16 * nt - 1) // (16 * nt)
    ndch = (d + 31) // 32
    Cd = C.to(device=dev, dtype=torch.float64)
    pad = torch.zeros((nblk * nt * 16, ndch * 32), dtype=torch.float64, device=dev)
    pad[:k, :d] = Cd
    img = pad.view(nblk, nt, 16, ndch, 2, 4, 4).permute(0, 3, 4, 1, 5, 2, 6).contiguous()
    # |c|^2 from the padded copy, whose rows all start on the same alignment: a row sum of the [k, d] tensor itself
    # may take another order for an odd row of an odd d, and duplicate centroids would then differ in the last bit
    ninit = torch.zeros(nblk * nt * 16, dtype=torch.float64, device=dev) if cosine else -0.5 * (pad * pad).sum(1)
    return img, ninit, nt, nblk


def _nearest_hip(X: torch.Tensor, C: torch.Tensor, dist_type: str, want_idx: bool, want_dist: bool,
                 want_counts: bool, grid: int = 0):
    global DENSE64_CALLS
    cosine = _dist_code(dist_type)
    _check(X, C)
    dev = X.device
    k, d = C.shape
    n = X.shape[0]
    idx = torch.zeros(n, dtype=torch.int32, device=dev) if want_idx else None
    dist = torch.zeros(n, dtype=torch.float64, device=dev) if want_dist else None
    counts = torch.zeros(k, dtype=torch.int64, device=dev) if want_counts else None
    if n == 0:      # nothing is launched for an empty partition
        return idx, dist, counts
    img, ninit, nt, nblk = centroid_image(C, cosine, dev)
    _lib.call("alink_kmeans_dense64_nearest", X.data_ptr(), n, d, img.data_ptr(), ninit.data_ptr(), k, nt, nblk,
              cosine, idx.data_ptr() if want_idx else None, dist.data_ptr() if want_dist else None,
              counts.data_ptr() if want_counts else None, int(grid), _lib.stream_ptr(dev))
    DENSE64_CALLS += 1
    return idx, dist, counts


def nearest(X: torch.Tensor, C: torch.Tensor, dist_type: str, grid: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Nearest centroid per row: (idx int64 [n], dist fp64 [n]) — squared distance for EUCLIDEAN, ``1 - x.c`` for
    COSINE.  Bit-equal scores go to the lowest centroid index; a row with a NaN goes to index 0."""
    _dist_code(dist_type)
    if use_hip(X, C.shape[0]):
        idx, dist, _ = _nearest_hip(X, C, dist_type, True, True, False, grid)
        return idx.to(torch.int64), dist
    return nearest_torch(X, C, dist_type)


def nearest_counts(X: torch.Tensor, C: torch.Tensor, dist_type: str, grid: int = 0) -> torch.Tensor:
    """Rows per nearest centroid, exact int64 [k] (integer adds on the GPU, no per-row output)."""
    _dist_code(dist_type)
    k = C.shape[0]
    if use_hip(X, k):
        return _nearest_hip(X, C, dist_type, False, False, True, grid)[2]
    return torch.bincount(nearest_torch(X, C, dist_type)[0], minlength=k)


def sorted_work(idx: torch.Tensor, k: int, ignore_outside: bool = False):
    """The work list of the accumulate kernel (``csrc/kmeans_dense64.hip``) for the rows' clusters ``idx`` int32 /
    int64 [n], shared by KMeans, BisectingKMeans and EvalCluster: one stable sort, then
    (perm, nchunk, wstart, wlen, cfirst, nch, cnt).  Every value must be in [0, k), unless ``ignore_outside``: such
    rows then get the key ``k``, sort behind every cluster, and no chunk covers them (they are never read)."""
    dev = idx.device
    key = idx.to(torch.int32)
    if ignore_outside:
        key = torch.where((key >= 0) & (key < k), key, torch.full_like(key, k))
    # a stable sort keeps the rows of a cluster in ascending order; the chunk list follows from the counts alone
    skey, perm = torch.sort(key, stable=True)
    cnt = torch.bincount(skey, minlength=k + 1)[:k] if ignore_outside else torch.bincount(skey, minlength=k)
    if int(cnt.shape[0]) != k:
        raise ValueError("idx holds a cluster outside [0, k)")
    del skey, key
    first = torch.cumsum(cnt, 0) - cnt                            # a cluster's first position in perm
    nch = (cnt + (ACCUM_ROWS - 1)) // ACCUM_ROWS
    cfirst = (torch.cumsum(nch, 0) - nch).contiguous()            # a cluster's first chunk
    wc = torch.repeat_interleave(torch.arange(k, device=dev), nch)       # the chunks' clusters (one size read)
    nchunk = int(wc.shape[0])
    wstart = first[wc] + (torch.arange(nchunk, device=dev) - cfirst[wc]) * ACCUM_ROWS
    wlen = torch.minimum(first[wc] + cnt[wc] - wstart, torch.full_like(wstart, ACCUM_ROWS)).to(torch.int32)
    return perm, nchunk, wstart.contiguous(), wlen.contiguous(), cfirst, nch.contiguous(), cnt.contiguous()


def accumulate_work(X: torch.Tensor, work, k: int, grid: int = 0) -> torch.Tensor:
    """[k, d+1] of the rows ``X`` [n, d] through a work list of ``sorted_work`` (one list serves several ``X``), by
    ``alink_kmeans_dense64_accum``: the same bits for every launch and every ``grid``."""
    global DENSE64_CALLS
    n, d = X.shape
    dev = X.device
    perm, nchunk, wstart, wlen, cfirst, nch, cnt = work
    part = torch.empty((max(nchunk, 1), d), dtype=torch.float64, device=dev)
    buf = torch.empty((k, d + 1), dtype=torch.float64, device=dev)
    _lib.call("alink_kmeans_dense64_accum", X.data_ptr(), d, perm.data_ptr(), nchunk, wstart.data_ptr(),
              wlen.data_ptr(), k, cfirst.data_ptr(), nch.data_ptr(), cnt.data_ptr(), part.data_ptr(), buf.data_ptr(),
              int(grid), _lib.stream_ptr(dev))
    DENSE64_CALLS += 1
    return buf


def _accumulate_hip(X: torch.Tensor, idx: torch.Tensor, k: int, grid: int = 0,
                    ignore_outside: bool = False) -> torch.Tensor:
    """[k, d+1] through the cluster-sorted row list; ``idx`` int32 / int64 [n] with every value in [0, k) (or, with
    ``ignore_outside``, the other rows left out and unread)."""
    return accumulate_work(X, sorted_work(idx, k, ignore_outside), k, grid)


def accumulate(X: torch.Tensor, idx: torch.Tensor, k: int, grid: int = 0,
               ignore_outside: bool = False) -> torch.Tensor:
    """[k, d+1] fp64 ``[sum_x | count]`` of the rows' clusters ``idx`` (every value in [0, k); with ``ignore_outside``
    rows outside it add nothing and are not read on the GPU); on the GPU the same bits for every launch and every
    ``grid``."""
    k = int(k)
    if idx.dim() != 1 or int(idx.shape[0]) != int(X.shape[0]):
        raise ValueError("idx must be an [n] tensor")
    if X.shape[0] == 0:
        return torch.zeros((k, X.shape[1] + 1), dtype=torch.float64, device=X.device)
    if use_hip(X, k):
        return _accumulate_hip(X, idx.to(X.device), k, grid, ignore_outside)
    if ignore_outside:
        idx = idx.to(torch.int64)
        idx = torch.where((idx >= 0) & (idx < k), idx, torch.full_like(idx, k))
        return _accumulate_torch(X, idx, k + 1)[:k]
    return _accumulate_torch(X, idx, k)


def assign_accumulate(X: torch.Tensor, C: torch.Tensor, grid: int = 0) -> torch.Tensor:
    """The Lloyd step's ``[k, d+1]`` fp64 buffer ``[sum_x | count]`` for this rank's fp64 rows (EUCLIDEAN scores:
    COSINE callers pass normalised rows and centroids, where the order of the scores is the same)."""
    _check(X, C)
    k = C.shape[0]
    if X.shape[0] == 0:
        return torch.zeros((k, X.shape[1] + 1), dtype=torch.float64, device=X.device)
    if use_hip(X, k):
        idx, _, _ = _nearest_hip(X, C, "EUCLIDEAN", True, False, False, grid)
        return _accumulate_hip(X, idx, k, grid)
    return assign_accumulate_torch(X, C)
