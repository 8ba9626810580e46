"""GMM E-step (``csrc/gmm.hip``): one GEMM for all components' Mahalanobis projections plus a
fused log-density / log-sum-exp / responsibility kernel.

``estep(X0, mu0, W, logdet, rank, logw)`` -> ``(R [n, k], sum_i lse_i)`` where ``X0 = X - xbar`` and
``mu0 = mu - xbar`` (centred by one global vector so ``x W - mu W`` loses no precision), ``W [k, d, d]`` the
pseudo-inverse roots of the covariances.  ``estep_torch`` is the per-component torch formula
(``MultivariateGaussian.logpdf``); CPU tensors and k > 64 take it.

The fused EM step (``csrc/gmm_em.hip``), for contiguous fp64 GPU rows with ``1 <= d <= EM_DMAX``:

* ``em_step(X0, mu0, W, logdet, rank, logw)`` -> ``(rs [k], xs [k, d], xxs [k, d, d], ll, R [n, k])``, the moment
  sums of the CENTRED rows: one E pass on the fp64 matrix cores whose only per-row output is ``R``, and one M pass
  over (row chunk, component) units whose partials (at most ``EM_SCRATCH_BYTES``) are merged in chunk order.  No
  ``[n, k d]`` buffer, no float atomics: the same bits for every launch and every ``grid``;
* ``posterior(X0, mu0, W, logdet, rank, logw, want_prob)`` -> ``(pred int64 [n], prob [n, k] or None)``: the E pass
  alone; bit-equal log densities go to the lowest component;
* ``em_step_torch`` / ``posterior_torch``: the same results in plain torch (CPU tensors take them);
* ``em_supported`` / ``em_selected``: the shape rule, ``ALINK_GMM_HIP != "0"`` and the library.  With a GPU present a
  missing kernel library raises, unless ``ALINK_ALLOW_TORCH_FALLBACK=1``.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch

from . import _lib

__all__ = ["estep", "estep_torch", "KMAX", "EM_DMAX", "EM_SCRATCH_BYTES", "em_shape_ok", "em_supported",
           "em_selected", "em_step", "em_step_torch", "em_chunk_rows", "posterior", "posterior_torch"]

KMAX = 64
_CHUNK_BYTES = 1 << 30       # Z chunk of at most 1 GiB (rows x k*d fp64)
EM_DMAX = 128                # widest rows of the fused EM step: above it the [n, k d] traffic per flop of the GEMM
                             # path has fallen to the machine's fp64 balance
EM_SCRATCH_BYTES = 128 << 20  # cap of the M pass's chunk partials [nchunk, k, d d + d + 1]
EM_UNITS = 16384             # (chunk, component, tile row) units the M pass aims for
GMM_EM_CALLS = 0             # launches of the HIP EM kernels (tests read it)


def estep_torch(X0, mu0, W, logdet, rank, logw) -> Tuple[torch.Tensor, torch.Tensor]:
    n, k = X0.shape[0], mu0.shape[0]
    lp = torch.empty((n, k), dtype=X0.dtype, device=X0.device)
    for j in range(k):
        z = (X0 - mu0[j]) @ W[j]
        lp[:, j] = -0.5 * (rank[j] * math.log(2 * math.pi) + logdet[j]) - 0.5 * (z * z).sum(1)
    lp = lp + logw[None, :]
    lse = torch.logsumexp(lp, dim=1)
    return torch.exp(lp - lse[:, None]), lse.sum()


def estep(X0, mu0, W, logdet, rank, logw) -> Tuple[torch.Tensor, torch.Tensor]:
    k, d = mu0.shape
    if not (X0.is_cuda and X0.dtype == torch.float64 and k <= KMAX and _lib.kernels_enabled()):
        return estep_torch(X0, mu0, W, logdet, rank, logw)
    n = X0.shape[0]
    dev = X0.device
    Wcat = W.permute(1, 0, 2).reshape(d, k * d).contiguous()          # [d, k*d]: column block j is W_j
    C = torch.einsum("kd,kde->ke", mu0, W).contiguous()                # mu0_j W_j
    cst = (-0.5 * (rank * math.log(2 * math.pi) + logdet) + logw).to(torch.float64).contiguous()
    R = torch.empty((n, k), dtype=torch.float64, device=dev)
    rows = max(1, min(n, _CHUNK_BYTES // (8 * k * d)))
    total = torch.zeros((), dtype=torch.float64, device=dev)
    for s in range(0, n, rows):
        e = min(n, s + rows)
        Z = X0[s:e] @ Wcat
        part = torch.empty(_lib.query("alink_gmm_grid", e - s), dtype=torch.float64, device=dev)
        _lib.call("alink_gmm_estep_f64", Z.data_ptr(), e - s, k, d, C.data_ptr(), cst.data_ptr(), R[s:e].data_ptr(),
                  part.data_ptr(), _lib.stream_ptr(dev))
        total = total + part.sum()
    return R, total


# ---------------------------------------------------------------------------------------------------
# fused EM step (csrc/gmm_em.hip)
# ---------------------------------------------------------------------------------------------------
def _em_partial_bytes(k: int, d: int) -> int:
    """Bytes of one row chunk's partials in the M pass."""
    return 8 * int(k) * (d * d + d + 1)


def em_shape_ok(X0, k: int) -> bool:
    """The shape rule of the EM kernels: a contiguous fp64 [n, d] tensor, 1 <= d <= EM_DMAX, 1 <= n < 2^31,
    k >= 1 (and one chunk's partials within the scratch cap: k <= 1015 at d = 128)."""
    return (isinstance(X0, torch.Tensor) and X0.dtype == torch.float64 and X0.dim() == 2
            and X0.is_contiguous() and 1 <= X0.shape[1] <= EM_DMAX and 1 <= X0.shape[0] < 2 ** 31 and int(k) >= 1
            and _em_partial_bytes(k, X0.shape[1]) <= EM_SCRATCH_BYTES)


def em_supported(X0, k: int) -> bool:
    """Whether the EM kernels take these rows: ``em_shape_ok`` rows on a GPU."""
    return em_shape_ok(X0, k) and X0.is_cuda


def em_selected(X0, k: int) -> bool:
    """The selection rule: ``em_supported`` rows, unless ``ALINK_GMM_HIP=0``; then the project's fall-back rule."""
    if not em_supported(X0, k) or os.environ.get("ALINK_GMM_HIP", "") == "0":
        return False
    return _lib.kernels_enabled()


def em_chunk_rows(n: int, k: int, d: int) -> int:
    """Rows per chunk of the M pass, from (n, k, d) alone: about ``EM_UNITS`` work units, never more chunks than
    fit ``EM_SCRATCH_BYTES``, a multiple of 64 rows."""
    dt = (d + 15) // 16
    nch = max(1, min(EM_SCRATCH_BYTES // _em_partial_bytes(k, d), -(-EM_UNITS // (k * dt))))
    return max(64, -(-(-(-n // nch)) // 64) * 64)


def posterior_torch(X0, mu0, W, logdet, rank, logw, want_prob: bool):
    R, _ = estep_torch(X0, mu0, W, logdet, rank, logw)
    return R.argmax(1), (R if want_prob else None)


def em_step_torch(X0, mu0, W, logdet, rank, logw):
    """``em_step`` in plain torch on the centred rows."""
    R, ll = estep_torch(X0, mu0, W, logdet, rank, logw)
    return R.sum(0), R.T @ X0, torch.einsum("nk,nd,ne->kde", R, X0, X0), ll, R


def _em_image(mu0, W, logdet, rank, logw, dev):
    """The E pass's parameters: the columns of every W_j as a [k dpad, d] matrix (dpad = d rounded up to 16, zero
    columns behind d) in the lane order of ``kmeans_dense64.centroid_image`` at one tile per block, laid out
    img [tile, dch, u = 2, g = 4, m = 16, s = 4] (element: column ``tile * 16 + m``, dim ``dch * 32 + 16 u + 4 g + s``;
    the tile-outermost variant that the layout note of ``csrc/dense64_mfma.h`` sets apart) and padded with zero tiles
    to whole staging groups; ninit = -C_j per column (0 on the padding); cst [k]."""
    k, d = mu0.shape
    tpc = (d + 15) // 16
    ndch = (d + 31) // 32
    gt = {1: 8, 2: 4, 3: 2, 4: 2}[ndch]
    ngroup = -(-(k * tpc) // gt)
    Wd = W.to(device=dev, dtype=torch.float64)
    mu0 = mu0.to(device=dev, dtype=torch.float64)
    pad = torch.zeros((ngroup * gt * 16, ndch * 32), dtype=torch.float64, device=dev)
    pad[:k * tpc * 16].view(k, tpc * 16, ndch * 32)[:, :d, :d] = Wd.transpose(1, 2)
    img = pad.view(ngroup * gt, 16, ndch, 2, 4, 4).permute(0, 2, 3, 4, 1, 5).contiguous()
    ninit = torch.zeros(ngroup * gt * 16, dtype=torch.float64, device=dev)
    ninit[:k * tpc * 16].view(k, tpc * 16)[:, :d] = -torch.einsum("kd,kde->ke", mu0, Wd)
    cst = (-0.5 * (rank * math.log(2 * math.pi) + logdet) + logw).to(device=dev, dtype=torch.float64).contiguous()
    return img, ninit, cst, tpc, ngroup


def _em_rows(X0, mu0, W, logdet, rank, logw, want_r: bool, want_arg: bool, grid: int):
    """The E pass: (R or None, arg int32 or None, ll 0-dim or None)."""
    global GMM_EM_CALLS
    dev = X0.device
    n, d = X0.shape
    k = mu0.shape[0]
    if W.shape != (k, d, d) or mu0.shape != (k, d) or logdet.shape != (k,) or rank.shape != (k,) \
            or logw.shape != (k,):
        raise ValueError("GMM parameter shape mismatch")
    img, ninit, cst, tpc, ngroup = _em_image(mu0, W, logdet, rank, logw, dev)
    R = torch.empty((n, k), dtype=torch.float64, device=dev) if want_r else None
    arg = torch.empty(n, dtype=torch.int32, device=dev) if want_arg else None
    part = torch.empty((n + 63) // 64 + 1, dtype=torch.float64, device=dev) if want_r else None
    _lib.call("alink_gmm_em_rows_f64", X0.data_ptr(), n, d, img.data_ptr(), ninit.data_ptr(), cst.data_ptr(), k, tpc,
              ngroup, R.data_ptr() if want_r else None, arg.data_ptr() if want_arg else None,
              part.data_ptr() if want_r else None, part[-1:].data_ptr() if want_r else None, int(grid),
              _lib.stream_ptr(dev))
    GMM_EM_CALLS += 1
    return R, arg, (part[-1] if want_r else None)


def _em_moments(X0, R, grid: int, chunk_rows: int):
    """The M pass: (rs [k], xs [k, d], xxs [k, d, d]) of the rows X0 under the responsibilities R."""
    global GMM_EM_CALLS
    dev = X0.device
    n, d = X0.shape
    k = R.shape[1]
    rows = int(chunk_rows) if chunk_rows > 0 else em_chunk_rows(n, k, d)
    nchunk = -(-n // rows)
    S = d * d + d + 1
    part = torch.empty((nchunk, k, S), dtype=torch.float64, device=dev)
    out = torch.empty(k * S, dtype=torch.float64, device=dev)
    _lib.call("alink_gmm_em_moments_f64", X0.data_ptr(), R.data_ptr(), n, d, k, rows, nchunk, part.data_ptr(),
              out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    GMM_EM_CALLS += 1
    return out[:k], out[k:k + k * d].view(k, d), out[k + k * d:].view(k, d, d)


def em_step(X0, mu0, W, logdet, rank, logw, grid: int = 0, chunk_rows: int = 0):
    """One EM step's statistics of the centred rows: ``(rs [k], xs [k, d], xxs [k, d, d], ll, R [n, k])``.  On
    the GPU the same bits for every launch and every ``grid`` (``chunk_rows`` overrides the M pass's chunk length,
    which otherwise follows from (n, k, d) alone).  CPU tensors take ``em_step_torch``; GPU rows outside
    ``em_supported`` are an error (ask ``em_selected`` first)."""
    if not X0.is_cuda:
        return em_step_torch(X0, mu0, W, logdet, rank, logw)
    k, d = mu0.shape
    if X0.shape[0] == 0:        # nothing is launched for an empty partition
        z = torch.zeros
        return (z(k, dtype=torch.float64, device=X0.device), z((k, d), dtype=torch.float64, device=X0.device),
                z((k, d, d), dtype=torch.float64, device=X0.device), z((), dtype=torch.float64, device=X0.device),
                z((0, k), dtype=torch.float64, device=X0.device))
    if not em_supported(X0, k):
        raise ValueError(f"the GMM EM kernels need contiguous fp64 [n, d] rows with 1 <= d <= {EM_DMAX}, fewer than "
                         "2^31 rows and k >= 1")
    _lib.require()
    R, _, ll = _em_rows(X0, mu0, W, logdet, rank, logw, True, False, grid)
    rs, xs, xxs = _em_moments(X0, R, grid, chunk_rows)
    return rs, xs, xxs, ll, R


def posterior(X0, mu0, W, logdet, rank, logw, want_prob: bool,
              grid: int = 0) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """``(pred int64 [n], prob [n, k] or None)``: the most responsible component per row (the lowest index among
    bit-equal ones) and, with ``want_prob``, the responsibilities.  The E pass alone; without ``want_prob`` no
    [n, k] tensor is allocated."""
    if not X0.is_cuda:
        return posterior_torch(X0, mu0, W, logdet, rank, logw, want_prob)
    k = mu0.shape[0]
    if X0.shape[0] == 0:
        return (torch.zeros(0, dtype=torch.int64, device=X0.device),
                torch.zeros((0, k), dtype=torch.float64, device=X0.device) if want_prob else None)
    if not em_supported(X0, k):
        raise ValueError(f"the GMM EM kernels need contiguous fp64 [n, d] rows with 1 <= d <= {EM_DMAX}, fewer than "
                         "2^31 rows and k >= 1")
    _lib.require()
    R, arg, _ = _em_rows(X0, mu0, W, logdet, rank, logw, bool(want_prob), True, grid)
    return arg.to(torch.int64), R
