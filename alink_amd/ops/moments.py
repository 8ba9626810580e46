"""Second-moment statistics and the PCA projection on the device (``csrc/moments.hip``), for contiguous fp64 GPU rows
``X [n, d]`` with ``1 <= d <= 1024``.

* ``moments(X, shift=None)`` -> ``(t [d], C [d, d])`` with ``t = sum_i (x_i - shift)`` and
  ``C = sum_i (x_i - shift)(x_i - shift)^T``: one pass that subtracts the shift in registers (no ``[n, d]``
  temporary), runs the upper tile triangle on the fp64 matrix cores and mirrors it, so ``C`` is exactly symmetric.
  Chunk partials (at most ``MOMENTS_SCRATCH_BYTES``) are merged in chunk order, no float atomics: the same bits for
  every launch and every ``grid``.  A shift near the columns' means keeps ``(C - t t^T / n) / (n - 1)`` from
  cancelling for columns whose mean is large against their spread; ``shared_shift`` picks one that all ranks share;
* ``pca_project(X, mean, scale, T, sstd)`` -> ``P [n, k]``, ``P[i, j] = sum_c ((x_ic - mean[c]) / scale[c]) T[j, c]
  / sstd[j]`` with true divisions; a column of ``scale`` 0 adds exactly nothing, whatever its cells hold;
* ``moments_torch`` / ``pca_project_torch``: the same definitions in plain torch (CPU tensors take them);
* ``shape_ok`` / ``supported`` / ``selected``: the shape rule, the rule on a GPU, and the gate
  ``sized_gate("ALINK_MOMENTS_HIP", device, n, MOMENTS_MIN_ROWS)`` for widths up to ``MOMENTS_MAX_D``;
* ``pairwise_moments(X, shift=None)`` -> ``out [4, d, d] = [N | S | Q | P]``, the pairwise-complete statistics of rows
  whose NaN cells are missing: with ``y = x - shift`` on present cells and ``m`` the presence flag,
  ``N[a,b] = sum_i m_ia m_ib``, ``S[a,b] = sum_i y_ia m_ib``, ``Q[a,b] = sum_i y_ia^2 m_ib`` and
  ``P[a,b] = sum_i y_ia y_ib m_ia m_ib``: one masked pass on the fp64 matrix cores, ``N`` and ``P`` exactly
  symmetric, the same bits for every launch and ``grid``; ``pairwise_moments_torch`` is the same in plain torch,
  ``pairwise_selected`` the callers' gate and ``pairwise_shift`` the vote and the shift all ranks share.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .kmeans_dense64 import centroid_image

__all__ = ["MOMENTS_DMAX", "MOMENTS_MAX_D", "MOMENTS_MIN_ROWS", "MOMENTS_WIDE_MIN_ROWS", "MOMENTS_SCRATCH_BYTES", "shape_ok", "supported",
           "selected", "moments_chunk_rows", "moments", "moments_torch", "pca_project", "pca_project_torch",
           "project_table", "shared_shift", "covariance", "PAIRWISE_MIN_ROWS", "PAIRWISE_WIDE_MIN_ROWS",
           "pairwise_moments", "pairwise_moments_torch", "pairwise_selected", "pairwise_shift"]

MOMENTS_DMAX = 1024                 # widest row the kernels take
MOMENTS_MAX_D = 1024                # widest row the callers send: the pass wins at every measured width (profiles/moments.txt)
MOMENTS_MIN_ROWS = 1024             # one column block (d <= 128): the former chain last wins at 256 x 128
MOMENTS_WIDE_MIN_ROWS = 65536       # more blocks: it wins up to 16384 x 512 and 16384 x 1024 (profiles/moments.txt)
MOMENTS_SCRATCH_BYTES = 256 << 20   # cap of the chunk partials [nchunk, d + d^2]
MOMENTS_CHUNKS = 512                # row chunks at most: the merge adds them one after another
MOMENTS_CHUNK_MIN_ROWS = 256        # and no chunk shorter than this, so that a small n has few partials to merge
MOMENTS_CALLS = 0                   # launches of the HIP moment / projection kernels (tests read it)
PAIRWISE_MIN_ROWS = 1024            # pairwise pass, d <= 128: the former chain last wins at 256 x 128
PAIRWISE_WIDE_MIN_ROWS = 65536      # d > 128: it wins at 16384 x 512 and 4096 x 1024 (profiles/pairwise_moments.txt)
PAIRWISE_CALLS = 0                  # launches of the pairwise-complete moment pass (tests read it)


def shape_ok(X) -> bool:
    """The shape rule of the kernels: a contiguous fp64 [n, d] tensor, 1 <= d <= MOMENTS_DMAX, n < 2^31."""
    return (isinstance(X, torch.Tensor) and X.dtype == torch.float64 and X.dim() == 2 and X.is_contiguous()
            and 1 <= X.shape[1] <= MOMENTS_DMAX and X.shape[0] < 2 ** 31)


def supported(X) -> bool:
    """Whether the kernels take these rows: ``shape_ok`` rows on a GPU."""
    return shape_ok(X) and X.is_cuda


def selected(X) -> bool:
    """The selection rule of the callers: ``supported`` rows at most ``MOMENTS_MAX_D`` wide, from
    ``MOMENTS_MIN_ROWS`` rows on (``MOMENTS_WIDE_MIN_ROWS`` for more than one block of 128 columns;
    ``ALINK_MOMENTS_HIP=1``: always, ``=0``: never); then the project's fall-back rule."""
    return (supported(X) and X.shape[1] <= MOMENTS_MAX_D
            and _lib.sized_gate("ALINK_MOMENTS_HIP", X.device, X.shape[0],
                                MOMENTS_MIN_ROWS if X.shape[1] <= 128 else MOMENTS_WIDE_MIN_ROWS))


def moments_chunk_rows(n: int, d: int) -> int:
    """Rows per chunk of the moment pass, from (n, d) alone: ``_lib.chunk_rows`` under the moment constants."""
    return _lib.chunk_rows(n, d + d * d, MOMENTS_SCRATCH_BYTES, MOMENTS_CHUNKS, MOMENTS_CHUNK_MIN_ROWS)


def moments_torch(X: torch.Tensor, shift: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``moments`` in plain torch: the shifted copy, its column sums and one product."""
    Y = X if shift is None else X - shift.to(device=X.device, dtype=X.dtype)[None, :]
    return Y.sum(0), Y.T @ Y


def pca_project_torch(X, mean, scale, T, sstd) -> torch.Tensor:
    """``pca_project`` in plain torch."""
    ok = scale != 0
    Z = torch.where(ok[None, :], (X - mean[None, :]) / torch.where(ok, scale, torch.ones_like(scale))[None, :],
                    torch.zeros_like(X))
    return Z @ T.T / sstd[None, :]


def _vec(v, size, dev, what):
    t = torch.as_tensor(v, dtype=torch.float64).to(dev).contiguous()
    if t.shape != (size,):
        raise ValueError(f"{what} must have {size} entries")
    return t


def _check(X):
    if not supported(X):
        raise ValueError(f"the moment kernels need contiguous fp64 [n, d] rows with 1 <= d <= {MOMENTS_DMAX} and "
                         "fewer than 2^31 rows")
    _lib.require()


def moments(X: torch.Tensor, shift=None, grid: int = 0, chunk_rows: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(t [d], C [d, d])`` of the rows shifted by ``shift`` ([d] or None: zero).  On the GPU the same bits for
    every launch and every ``grid`` (``chunk_rows``, a multiple of 64, overrides the chunk length, which otherwise
    follows from (n, d) alone).  CPU tensors take ``moments_torch``; GPU rows outside ``supported`` are an error
    (ask ``selected`` first)."""
    global MOMENTS_CALLS
    if not X.is_cuda:
        return moments_torch(X, None if shift is None else torch.as_tensor(shift, dtype=X.dtype))
    _check(X)
    n, d = X.shape
    dev = X.device
    if n == 0:          # nothing is launched for an empty partition
        return torch.zeros(d, dtype=torch.float64, device=dev), torch.zeros((d, d), dtype=torch.float64, device=dev)
    sh = None if shift is None else _vec(shift, d, dev, "shift")
    crows = int(chunk_rows) if chunk_rows > 0 else moments_chunk_rows(n, d)
    nchunk, part, out = _lib.chunk_buffers(n, crows, d + d * d, dev)
    _lib.call("alink_moments_f64", X.data_ptr(), n, d, sh.data_ptr() if sh is not None else None, crows, nchunk,
              part.data_ptr(), out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    MOMENTS_CALLS += 1
    return out[:d], out[d:].view(d, d)


def pca_project(X: torch.Tensor, mean, scale, T, sstd, grid: int = 0) -> torch.Tensor:
    """``P [n, k]`` of the module text for ``X [n, nx]``, ``mean`` / ``scale`` [nx], the table ``T [k, nx]`` (or its
    image, the tuple ``project_table`` returns) and ``sstd`` [k].  CPU tensors take ``pca_project_torch``."""
    global MOMENTS_CALLS
    if not X.is_cuda:
        t = lambda a: torch.as_tensor(a, dtype=torch.float64)  # noqa: E731
        return pca_project_torch(X, t(mean), t(scale), t(T), t(sstd))
    _check(X)
    n, nx = X.shape
    dev = X.device
    img, k = T if isinstance(T, tuple) else project_table(T, dev)
    if img.shape[1] != (nx + 31) // 32:
        raise ValueError("the table must have one column per column of the rows")
    P = torch.empty((n, k), dtype=torch.float64, device=dev)
    if n == 0:
        return P
    mean, scale, sstd = _vec(mean, nx, dev, "mean"), _vec(scale, nx, dev, "scale"), _vec(sstd, k, dev, "sstd")
    _lib.call("alink_pca_project_f64", X.data_ptr(), n, nx, mean.data_ptr(), scale.data_ptr(), img.data_ptr(), k,
              sstd.data_ptr(), P.data_ptr(), int(grid), _lib.stream_ptr(dev))
    MOMENTS_CALLS += 1
    return P


def project_table(T, dev):
    """``(img, k)``: the lane-ordered image (``centroid_image``) of the table ``T [k, nx]`` on ``dev``, built once
    per model."""
    T = torch.as_tensor(T, dtype=torch.float64)
    if T.dim() != 2 or T.shape[0] < 1:
        raise ValueError("the table must be [k, nx] with k >= 1")
    return centroid_image(T, 1, dev)[0], int(T.shape[0])


def shared_shift(X: torch.Tensor) -> Optional[torch.Tensor]:
    """The callers' decision and shift in one small ``all_gather_object``: None when the moment pass is not taken
    (off a GPU or with ``ALINK_MOMENTS_HIP=0`` nothing is gathered; else every rank votes ``selected``, a rank without
    rows votes by its shape alone, and one ``no`` keeps all ranks on the former path), else the shift all ranks
    share: the first row of the lowest rank that has rows, non-finite entries replaced by 0, zeros when no rank has
    rows.  fp64 [d] on the rows' device."""
    from ..parallel import comm
    if not _lib.sized_gate("ALINK_MOMENTS_HIP", X.device, MOMENTS_MIN_ROWS, MOMENTS_MIN_ROWS):
        return None
    n = X.shape[0]
    vote = selected(X) if n else supported(X) and X.shape[1] <= MOMENTS_MAX_D
    got = comm.all_gather_object((bool(vote), X[0].tolist() if n and vote else None))
    if not all(v for v, _ in got):
        return None
    rows = [r for _, r in got if r is not None]
    sh = torch.tensor(rows[0] if rows else [0.0] * X.shape[1], dtype=torch.float64)
    return torch.where(torch.isfinite(sh), sh, torch.zeros_like(sh)).to(X.device)


def covariance(X: torch.Tensor, shift: torch.Tensor):
    """``(n, mean [d], S [d, d])`` over all ranks' rows from one ``moments`` pass around ``shift`` (of
    ``shared_shift``) and one all-reduce of ``[n | t | C]``: ``mean = shift + t / n`` and the centred sums
    ``S = C - t t^T / n``, the covariance times ``n - 1``."""
    from ..parallel import comm
    d = X.shape[1]
    t, C = moments(X, shift)
    buf = torch.cat([torch.tensor([float(X.shape[0])], dtype=torch.float64, device=X.device), t, C.reshape(-1)])
    comm.all_reduce(buf, "sum")
    n = float(buf[0])
    t, C = buf[1:1 + d], buf[1 + d:].reshape(d, d)
    return n, shift + t / n, C - torch.outer(t, t) / n


def pairwise_moments_torch(X: torch.Tensor, shift: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``pairwise_moments`` in plain torch: the presence mask, the shifted values with 0 in the missing cells, three
    products with the mask and one of the values."""
    M = (~torch.isnan(X)).to(X.dtype)
    Y = X if shift is None else X - shift.to(device=X.device, dtype=X.dtype)[None, :]
    A = torch.where(torch.isnan(X), torch.zeros_like(X), Y)
    return torch.stack([M.T @ M, A.T @ M, (A * A).T @ M, A.T @ A])


def pairwise_selected(X) -> bool:
    """The callers' rule for the pairwise-complete pass: ``supported`` rows from ``PAIRWISE_MIN_ROWS`` rows on
    (``PAIRWISE_WIDE_MIN_ROWS`` above 128 columns; ``ALINK_MOMENTS_HIP=1``: always, ``=0``: never); then the
    project's fall-back rule."""
    return supported(X) and _lib.sized_gate("ALINK_MOMENTS_HIP", X.device, X.shape[0],
                                            PAIRWISE_MIN_ROWS if X.shape[1] <= 128 else PAIRWISE_WIDE_MIN_ROWS)


def pairwise_moments(X: torch.Tensor, shift=None, grid: int = 0, chunk_rows: int = 0) -> torch.Tensor:
    """``out [4, d, d] = [N | S | Q | P]`` of the module text for rows whose NaN cells are missing, shifted by
    ``shift`` ([d] or None: zero).  On the GPU the same bits for every launch and every ``grid`` (``chunk_rows``, a
    multiple of 64, overrides the chunk length, which otherwise follows from (n, d) alone).  CPU tensors take
    ``pairwise_moments_torch``; GPU rows outside ``supported`` are an error (ask ``pairwise_selected`` first)."""
    global PAIRWISE_CALLS
    if not X.is_cuda:
        return pairwise_moments_torch(X, None if shift is None else torch.as_tensor(shift, dtype=X.dtype))
    _check(X)
    n, d = X.shape
    dev = X.device
    if n == 0:          # nothing is launched for an empty partition
        return torch.zeros((4, d, d), dtype=torch.float64, device=dev)
    sh = None if shift is None else _vec(shift, d, dev, "shift")
    crows = int(chunk_rows) if chunk_rows > 0 else _lib.chunk_rows(n, 4 * d * d, MOMENTS_SCRATCH_BYTES,
                                                                   MOMENTS_CHUNKS, MOMENTS_CHUNK_MIN_ROWS)
    nchunk, part, out = _lib.chunk_buffers(n, crows, 4 * d * d, dev)
    _lib.call("alink_pairwise_moments_f64", X.data_ptr(), n, d, sh.data_ptr() if sh is not None else None, crows,
              nchunk, part.data_ptr(), out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    PAIRWISE_CALLS += 1
    return out.view(4, d, d)


def pairwise_shift(X: torch.Tensor) -> Optional[torch.Tensor]:
    """The vote and the shift of the pairwise-complete pass in one small ``all_gather_object``, as ``shared_shift``:
    None when the pass is not taken (off a GPU or with ``ALINK_MOMENTS_HIP=0`` nothing is gathered; one rank's ``no``
    keeps all ranks on the former path; a rank without rows votes by its shape), else per column the first present
    finite value among the first 64 rows of the lowest rank that has one, else 0: near the column's values at the
    cost of no pass over X.  fp64 [d] on the rows' device."""
    from ..parallel import comm
    if not _lib.sized_gate("ALINK_MOMENTS_HIP", X.device, PAIRWISE_MIN_ROWS, PAIRWISE_MIN_ROWS):
        return None
    n, d = X.shape
    vote = pairwise_selected(X) if n else supported(X)
    got = comm.all_gather_object((bool(vote), X[:64].tolist() if n and vote else None))
    if not all(v for v, _ in got):
        return None
    sh = torch.zeros(d, dtype=torch.float64)
    todo = torch.ones(d, dtype=torch.bool)
    for rows in (r for _, r in got if r is not None):
        H = torch.tensor(rows, dtype=torch.float64).reshape(-1, d)
        fin = torch.isfinite(H)
        first = fin.to(torch.int8).argmax(0)
        take = todo & fin.any(0)
        sh = torch.where(take, H[first, torch.arange(d)], sh)
        todo &= ~take
    return sh.to(X.device)
