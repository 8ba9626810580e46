"""Stochastic Outlier Selection on the device (``csrc/sos.hip``): the per-row perplexity search and the ordered column
products, with the dissimilarities recomputed on the fp64 matrix cores at every evaluation and never stored.

For fp64 rows ``X [n, d]`` (2 <= n, 1 <= d <= 1024) both passes work on the rows centred by the column means
(distances are translation invariant; a large common offset would otherwise cost digits) and on ONE vector ``q`` of
squared row norms: ``D_ij = max(0, (q_i + q_j) - 2 x_i . x_j)``, the pair ``j == i`` skipped by index.

* ``search(X, perplexity, rows=None)`` -> ``(beta, s, iters)`` of the rows ``[lo, hi)``: the reference's
  ``solveForBeta`` (``SOSImpl.java:75-131``: beta0 = 1, betaMin = 0, betaMax unbounded, tol 1e-2, at most 100 updates)
  with ``logH = (sum a D) (beta / sum a) + log(sum a)``, ``a = exp(-beta D)``; ``s`` is ``sum a`` at the final beta,
  ``iters`` the updates made;
* ``products(X, beta, s, cols=None)`` -> ``p_j = prod_{i != j} (1 - exp(-beta_i D_ij) / s_i)`` of the columns
  ``[lo, hi)`` (``SOSImpl.java:133-203``);
* ``scores(X, perplexity)`` -> search then products, or ``None`` when some ``s`` is not a positive finite number or
  some ``beta`` is not finite (one host read): the caller then takes its former path and keeps that path's values;
* ``search_torch`` / ``products_torch``: the same formulas in plain torch, on any device (CPU tensors take them
  through the functions above);
* ``sos_supported`` / ``sos_selected``: the shape rule; ``ALINK_SOS_HIP != "0"``, ``d <= SOS_MAX_D`` and the library.
  With a GPU present a missing kernel library raises, unless ``ALINK_ALLOW_TORCH_FALLBACK=1``.

On the GPU no ``[n, n]`` or ``[block, n]`` buffer exists: scratch is the centred rows, their lane-ordered image
(``kmeans_dense64.centroid_image``, d padded to 32) and a few ``[n]`` vectors.  No float atomics: the same bits for
every launch, every ``grid`` and every split into ``rows=`` / ``cols=`` ranges (so a multi-rank split is an
all-gather of two vectors).
"""
from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch

from . import _lib
from .kmeans_dense64 import centroid_image

__all__ = ["SOS_MAX_D", "SOS_DMAX", "MAX_ITER", "TOL", "sos_supported", "sos_selected", "search", "products", "scores",
           "search_torch", "products_torch"]

SOS_DMAX = 1024         # widest rows the kernels take
SOS_MAX_D = 256         # widest rows for which the kernels are selected: the largest measured width up to which their
                        # median is below the former path's at n = 2e4 (profiles/sos.txt: 4.4x at d = 8, level at
                        # 256, 0.5x and 0.3x at 512 and 1024, where recomputing a dot costs more than reading a
                        # stored D)
MAX_ITER = 100
TOL = 1.0e-2
TORCH_BLOCK = 1024      # rows per block of the torch twins
SOS_CALLS = 0           # search / products passes made through search, products and scores: kernel launches on a
                        # GPU, twin passes for CPU tensors (tests read it)


def sos_supported(X) -> bool:
    """Whether the kernels take these rows: a contiguous fp64 [n, d] tensor on a GPU, 2 <= n < 2^31,
    1 <= d <= SOS_DMAX."""
    return (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float64 and X.dim() == 2
            and X.is_contiguous() and 2 <= X.shape[0] < 2 ** 31 and 1 <= X.shape[1] <= SOS_DMAX)


def sos_selected(X) -> bool:
    """The selection rule: ``sos_supported`` rows at most ``SOS_MAX_D`` wide, unless ``ALINK_SOS_HIP=0``; then the
    project's fall-back rule."""
    if not sos_supported(X) or os.environ.get("ALINK_SOS_HIP", "") == "0" or X.shape[1] > SOS_MAX_D:
        return False
    return _lib.kernels_enabled()


def _range(r, n: int) -> Tuple[int, int]:
    lo, hi = (0, n) if r is None else (int(r[0]), int(r[1]))
    if not 0 <= lo <= hi <= n:
        raise ValueError(f"range {r} outside [0, {n}]")
    return lo, hi


def _centre(X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(the rows minus the column means, their squared norms q [n]).  Rows that do not start on 16 bytes are copied
    first, so that the reductions see the same layout as for a fresh tensor and give the same bits."""
    if X.dim() != 2 or X.shape[0] < 2 or X.shape[1] < 1:
        raise ValueError("SOS needs [n, d] rows with n >= 2 and d >= 1")
    X = X.to(torch.float64)
    if X.data_ptr() % 16 != 0 or not X.is_contiguous():
        X = X.clone(memory_format=torch.contiguous_format)
    Xc = X - X.mean(0)
    return Xc, (Xc * Xc).sum(1)


# ---------------------------------------------------------------------------------------------------
# torch twins (any device; the CPU oracle of the wiring)
# ---------------------------------------------------------------------------------------------------
def _block_d(Xc, q, s: int, e: int, lo: int, hi: int):
    """D [e - s, hi - lo] of the rows [s, e) against the columns [lo, hi), and the mask of the pairs i == j."""
    D = ((q[s:e, None] + q[None, lo:hi]) - 2.0 * (Xc[s:e] @ Xc[lo:hi].T)).clamp_min(0.0)
    same = torch.arange(s, e, device=Xc.device)[:, None] == torch.arange(lo, hi, device=Xc.device)[None, :]
    return D, same


def _evaluate(D, same, beta):
    A = torch.exp(-beta[:, None] * D).masked_fill(same, 0.0)
    s = A.sum(1)
    return s, (A * D).masked_fill(same, 0.0).sum(1) * (beta / s) + torch.log(s)


def search_torch(X: torch.Tensor, perplexity: float, rows=None,
                 block: int = TORCH_BLOCK) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``search`` in plain torch: every row follows the reference's sequence of updates (vectorised state with a
    per-row mask)."""
    Xc, q = _centre(X)
    n = Xc.shape[0]
    lo, hi = _range(rows, n)
    dev = Xc.device
    logh = math.log(perplexity)
    beta_out = torch.empty(hi - lo, dtype=torch.float64, device=dev)
    s_out = torch.empty(hi - lo, dtype=torch.float64, device=dev)
    it_out = torch.empty(hi - lo, dtype=torch.int32, device=dev)
    for b in range(lo, hi, block):
        e = min(hi, b + block)
        D, same = _block_d(Xc, q, b, e, 0, n)
        beta = torch.ones(e - b, dtype=torch.float64, device=dev)
        bmin = torch.zeros_like(beta)
        bmax = torch.full_like(beta, float("inf"))
        iters = torch.zeros(e - b, dtype=torch.int32, device=dev)
        s, lh = _evaluate(D, same, beta)
        err = lh - logh
        for _ in range(MAX_ITER):
            nan = torch.isnan(err)
            active = nan | (err.abs() > TOL)
            if not bool(active.any()):
                break
            pos = active & ~nan & (err > 0)
            neg = active & ~nan & ~(err > 0)
            nb = torch.where(active & nan, beta / 10.0, beta)
            nb = torch.where(pos, torch.where(torch.isinf(bmax), beta * 2.0, 0.5 * (beta + bmax)), nb)
            nb = torch.where(neg, 0.5 * (bmin + beta), nb)
            bmin = torch.where(pos, beta, bmin)
            bmax = torch.where(neg, beta, bmax)
            beta = nb
            iters += active.to(torch.int32)
            s2, lh = _evaluate(D, same, beta)
            err = torch.where(active, lh - logh, err)
            s = torch.where(active, s2, s)
        beta_out[b - lo:e - lo], s_out[b - lo:e - lo], it_out[b - lo:e - lo] = beta, s, iters
    return beta_out, s_out, it_out


def products_torch(X: torch.Tensor, beta: torch.Tensor, s: torch.Tensor, cols=None,
                   block: int = TORCH_BLOCK) -> torch.Tensor:
    """``products`` in plain torch: the product form, row blocks multiplied in ascending order."""
    Xc, q = _centre(X)
    n = Xc.shape[0]
    lo, hi = _range(cols, n)
    beta, s = _check_state(beta, s, n, Xc.device)
    p = torch.ones(hi - lo, dtype=torch.float64, device=Xc.device)
    for b in range(0, n, block):
        e = min(n, b + block)
        D, same = _block_d(Xc, q, b, e, lo, hi)
        B = (torch.exp(-beta[b:e, None] * D) / s[b:e, None]).masked_fill(same, 0.0)
        p = p * (1.0 - B).prod(0)
    return p


def _check_state(beta, s, n: int, dev):
    if beta.shape != (n,) or s.shape != (n,):
        raise ValueError("beta and s must be [n] tensors of all the rows")
    return (beta.to(device=dev, dtype=torch.float64).contiguous(), s.to(device=dev, dtype=torch.float64).contiguous())


# ---------------------------------------------------------------------------------------------------
# HIP path
# ---------------------------------------------------------------------------------------------------
def _prepare(X: torch.Tensor):
    """(Xc, img, qpad, nt, nblk): the centred rows, the image of all n rows in the lane order of the staging loop
    (zero rows behind n) and q padded with zeros to the image's slots.  nt follows from n alone."""
    if not sos_supported(X):
        raise ValueError(f"the SOS kernels need contiguous fp64 [n, d] GPU rows with n >= 2 and 1 <= d <= {SOS_DMAX}")
    _lib.require()
    Xc, q = _centre(X)
    img, qpad, nt, nblk = centroid_image(Xc, 1, Xc.device)      # cosine = 1: the zero vector of the slots
    qpad[:q.shape[0]] = q
    return Xc, img, qpad, nt, nblk


def _search_hip(prep, perplexity: float, lo: int, hi: int, grid: int):
    global SOS_CALLS
    Xc, img, qpad, nt, nblk = prep
    n, d = Xc.shape
    dev = Xc.device
    beta = torch.empty(hi - lo, dtype=torch.float64, device=dev)
    s = torch.empty(hi - lo, dtype=torch.float64, device=dev)
    iters = torch.empty(hi - lo, dtype=torch.int32, device=dev)
    if hi > lo:
        _lib.call("alink_sos_search_f64", Xc.data_ptr(), n, d, img.data_ptr(), qpad.data_ptr(), nt, nblk, lo, hi,
                  math.log(perplexity), beta.data_ptr(), s.data_ptr(), iters.data_ptr(), int(grid),
                  _lib.stream_ptr(dev))
        SOS_CALLS += 1
    return beta, s, iters


def _products_hip(prep, beta, s, lo: int, hi: int, grid: int):
    global SOS_CALLS
    Xc, img, qpad, nt, nblk = prep
    n, d = Xc.shape
    dev = Xc.device
    beta, s = _check_state(beta, s, n, dev)
    bpad = torch.zeros_like(qpad)
    spad = torch.ones_like(qpad)
    bpad[:n] = beta
    spad[:n] = s
    p = torch.empty(hi - lo, dtype=torch.float64, device=dev)
    if hi > lo:
        _lib.call("alink_sos_products_f64", Xc.data_ptr(), n, d, img.data_ptr(), qpad.data_ptr(), bpad.data_ptr(),
                  spad.data_ptr(), nt, nblk, lo, hi, p.data_ptr(), int(grid), _lib.stream_ptr(dev))
        SOS_CALLS += 1
    return p


def search(X: torch.Tensor, perplexity: float, rows=None,
           grid: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(beta fp64, s fp64, iters int32)`` of the rows ``rows = (lo, hi)`` (all by default) against all n rows.
    CPU tensors take ``search_torch``; GPU rows outside ``sos_supported`` are an error (ask ``sos_selected``)."""
    global SOS_CALLS
    if not X.is_cuda:
        SOS_CALLS += 1
        return search_torch(X, perplexity, rows)
    lo, hi = _range(rows, X.shape[0])
    return _search_hip(_prepare(X), perplexity, lo, hi, grid)


def products(X: torch.Tensor, beta: torch.Tensor, s: torch.Tensor, cols=None, grid: int = 0) -> torch.Tensor:
    """``p [hi - lo]`` of the columns ``cols = (lo, hi)`` (all by default) from the ``beta`` and ``s`` of ALL n
    rows."""
    global SOS_CALLS
    if not X.is_cuda:
        SOS_CALLS += 1
        return products_torch(X, beta, s, cols)
    lo, hi = _range(cols, X.shape[0])
    return _products_hip(_prepare(X), beta, s, lo, hi, grid)


def scores(X: torch.Tensor, perplexity: float, grid: int = 0) -> Optional[torch.Tensor]:
    """The outlier probability of every row, or ``None`` when the search left a ``beta`` that is not finite or an
    ``s`` that is not a positive finite number (the caller's former path then decides, NaN included)."""
    n = X.shape[0]
    if not X.is_cuda:
        beta, s, _ = search(X, perplexity)
        if not _state_ok(beta, s):
            return None
        return products(X, beta, s)
    prep = _prepare(X)
    beta, s, _ = _search_hip(prep, perplexity, 0, n, grid)
    if not _state_ok(beta, s):
        return None
    return _products_hip(prep, beta, s, 0, n, grid)


def _state_ok(beta, s) -> bool:
    return bool((torch.isfinite(beta) & torch.isfinite(s) & (s > 0)).all())
