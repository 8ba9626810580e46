"""Multinomial (softmax) regression on the device (``csrc/softmax_fused.hip``): the fused gradient pass and the row
pass of ``SoftmaxObjFunc``, for contiguous fp64 GPU rows ``X [n, m]`` (``m`` includes the intercept column),
coefficients ``W [k1, m]`` (pivot class ``k1`` with logit 0, ``1 <= k1 <= SOFTMAX_FUSED_KMAX``), fp64 class indices
``y`` in ``[0, k1]`` and fp64 weights ``w``.

* ``fused_grad(X, y, w, W)`` -> ``(G [k1, m], sum w loss)`` for ``m <= SOFTMAX_FUSED_GRAD_MAX_M``: logits, softmax and
  ``G = R^T X`` on the fp64 matrix cores in one pass that reads X once and writes no ``[n, k1]`` block.  Chunk partials
  (at most ``SOFTMAX_SCRATCH_BYTES``) are merged in chunk order, no float atomics: the same bits for every launch and
  every ``grid``;
* ``search_losses(X, y, w, W, D, beta, nsteps)`` -> the ``nsteps`` weighted losses at ``W - s beta D`` from one read
  of X (``m <= SOFTMAX_FUSED_MAX_M``), in a fixed order;
* ``rows(X, y, w, W, want)`` -> a dict with ``"R"`` (``[n, k1]``, ``w (softmax - onehot)``, the right-hand side of the
  gradient GEMM of a wide ``m``) and / or ``"loss"`` (``sum w loss``);
* ``fused_grad_torch`` / ``search_losses_torch`` / ``rows_torch``: the same results by the former chain, a GEMM for the
  logits, the formulas of ``ops/softmax.py`` and ``tn_matmul`` (CPU tensors take them);
* ``shape_ok`` / ``supported`` / ``selected``: the shape rule, the rule on a GPU, and the gate
  ``sized_gate("ALINK_SOFTMAX_HIP", device, n, SOFTMAX_MIN_ROWS)``.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from . import _lib
from .gemm import tn_matmul
from .kmeans_dense64 import centroid_image
from .softmax import softmax_grad_torch, softmax_search_torch

__all__ = ["SOFTMAX_FUSED_KMAX", "SOFTMAX_FUSED_GRAD_MAX_M", "SOFTMAX_FUSED_MAX_M", "SOFTMAX_FUSED_MAX_STEPS",
           "SOFTMAX_MIN_ROWS", "SOFTMAX_SCRATCH_BYTES", "shape_ok", "supported", "selected", "softmax_chunk_rows",
           "fused_grad", "fused_grad_torch", "search_losses", "search_losses_torch", "rows", "rows_torch"]

SOFTMAX_FUSED_KMAX = 64             # four class tiles of 16
SOFTMAX_FUSED_GRAD_MAX_M = 128      # eight dim tiles: a row's dims stay in registers through the gradient pass
SOFTMAX_FUSED_MAX_M = 1024          # the row pass walks the dims in chunks of 32
SOFTMAX_FUSED_MAX_STEPS = 64
SOFTMAX_MIN_ROWS = 10000            # from here on gradient + search beat the former path at both swept shapes (profiles/softmax_fused.txt)
SOFTMAX_SCRATCH_BYTES = 128 << 20   # cap of the chunk partials [nchunk, 1 + k1 m]
SOFTMAX_CHUNKS = 1024               # row chunks of the gradient pass at most: the merge adds them one after another
SOFTMAX_CHUNK_MIN_ROWS = 256        # and no chunk shorter than this, so that a small n has few partials to merge
SOFTMAX_FUSED_CALLS = 0             # launches of the fused softmax kernels (tests read it)
_WANT = {"R": 1, "loss": 2}


def shape_ok(X, k1: int) -> bool:
    """The shape rule of the fused softmax kernels: a contiguous fp64 [n, m] tensor, 1 <= m <= SOFTMAX_FUSED_MAX_M,
    n < 2^31, 1 <= k1 <= SOFTMAX_FUSED_KMAX."""
    return (isinstance(X, torch.Tensor) and X.dtype == torch.float64 and X.dim() == 2 and X.is_contiguous()
            and 1 <= X.shape[1] <= SOFTMAX_FUSED_MAX_M and X.shape[0] < 2 ** 31 and 1 <= k1 <= SOFTMAX_FUSED_KMAX)


def supported(X, k1: int) -> bool:
    """Whether the fused softmax kernels take these rows: ``shape_ok`` rows on a GPU."""
    return shape_ok(X, k1) and X.is_cuda


def selected(X, k1: int) -> bool:
    """The selection rule: ``supported`` rows, from ``SOFTMAX_MIN_ROWS`` rows on (``ALINK_SOFTMAX_HIP=1``: always,
    ``=0``: never); then the project's fall-back rule."""
    return supported(X, k1) and _lib.sized_gate("ALINK_SOFTMAX_HIP", X.device, X.shape[0], SOFTMAX_MIN_ROWS)


def softmax_chunk_rows(n: int, k1: int, m: int) -> int:
    """Rows per chunk of the gradient pass, from (n, k1, m) alone: ``_lib.chunk_rows`` under this op's constants."""
    return _lib.chunk_rows(n, 1 + k1 * m, SOFTMAX_SCRATCH_BYTES, SOFTMAX_CHUNKS, SOFTMAX_CHUNK_MIN_ROWS)


def fused_grad_torch(X, y, w, W) -> Tuple[torch.Tensor, torch.Tensor]:
    """``fused_grad`` by the former chain: a GEMM for the logits, the softmax formulas, ``tn_matmul``."""
    R, loss = softmax_grad_torch(X @ W.T, y, w)
    return tn_matmul(X, R).T.contiguous(), loss


def search_losses_torch(X, y, w, W, D, beta: float, nsteps: int) -> torch.Tensor:
    """``search_losses`` by the former chain: two GEMMs and the search formulas."""
    return softmax_search_torch(X @ W.T, X @ D.T, y, w, beta, nsteps)


def rows_torch(X, y, w, W, want: Sequence[str]) -> Dict[str, torch.Tensor]:
    """``rows`` by the former chain."""
    R, loss = softmax_grad_torch(X @ W.T, y, w)
    return {key: val for key, val in (("R", R), ("loss", loss)) if key in want}


def _check(X, y, w, tables):
    k1 = tables[0].shape[0] if tables[0].dim() == 2 else 0
    if not supported(X, k1):
        raise ValueError(f"the fused softmax kernels need contiguous fp64 [n, m] GPU rows with 1 <= m <= "
                         f"{SOFTMAX_FUSED_MAX_M}, fewer than 2^31 rows and 1 <= k1 <= {SOFTMAX_FUSED_KMAX}")
    for t in (y, w):
        if not (t.dtype == torch.float64 and t.is_contiguous() and t.shape == (X.shape[0],) and t.device == X.device):
            raise ValueError("y and w must be contiguous fp64 [n] tensors on the rows' device")
    for t in tables:
        if not (t.dtype == torch.float64 and t.shape == (k1, X.shape[1]) and t.device == X.device):
            raise ValueError("W and D must be fp64 [k1, m] tensors on the rows' device")
    _lib.require()
    return k1


def _grad_image(W: torch.Tensor) -> torch.Tensor:
    """W [k1, m] zero-padded to whole tiles of 16 classes and whole chunks of 32 dims, tile outermost:
    img [t, dc, u = 2, g = 4, mm = 16, s = 4], element = W[16 t + mm, 32 dc + 16 u + 4 g + s]."""
    k1, m = W.shape
    nt, ndch = (k1 + 15) // 16, (m + 31) // 32
    pad = torch.zeros((nt * 16, ndch * 32), dtype=torch.float64, device=W.device)
    pad[:k1, :m] = W
    return pad.view(nt, 16, ndch, 2, 4, 4).permute(0, 2, 3, 4, 1, 5).contiguous()


def _rows_image(tables):
    """The lane-ordered image (``centroid_image``) of the tables stacked, each zero-padded to tw = 1, 2 or 4 tiles of
    16 classes, so that a class has the same lane slot in every table.  Returns ``(img, tw)``."""
    k1, m = tables[0].shape
    tw = 1 if k1 <= 16 else (2 if k1 <= 32 else 4)
    stack = torch.zeros((len(tables), tw * 16, m), dtype=torch.float64, device=tables[0].device)
    for i, t in enumerate(tables):
        stack[i, :k1] = t
    img, _, nt, nblk = centroid_image(stack.view(-1, m), 1, stack.device)
    assert nt == len(tables) * tw and nblk == 1
    return img, tw


def fused_grad(X, y, w, W, grid: int = 0, chunk_rows: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """One gradient pass: ``(G [k1, m], sum w loss (0-dim))``.  On the GPU the same bits for every launch and every
    ``grid`` (``chunk_rows``, a multiple of 64, overrides the chunk length, which otherwise follows from (n, k1, m)
    alone).  CPU tensors take ``fused_grad_torch``; GPU rows outside ``supported`` or wider than
    ``SOFTMAX_FUSED_GRAD_MAX_M`` are an error (ask ``selected`` first)."""
    global SOFTMAX_FUSED_CALLS
    if not X.is_cuda:
        return fused_grad_torch(X, y, w, W)
    k1 = _check(X, y, w, (W,))
    n, m = X.shape
    dev = X.device
    if m > SOFTMAX_FUSED_GRAD_MAX_M:
        raise ValueError(f"the fused gradient pass needs m <= {SOFTMAX_FUSED_GRAD_MAX_M}")
    if n == 0:          # nothing is launched for an empty partition
        return torch.zeros((k1, m), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    crows = int(chunk_rows) if chunk_rows > 0 else softmax_chunk_rows(n, k1, m)
    nchunk, part, out = _lib.chunk_buffers(n, crows, 1 + k1 * m, dev)
    img = _grad_image(W)
    _lib.call("alink_softmax_fused_grad_f64", X.data_ptr(), y.data_ptr(), w.data_ptr(), n, m, k1, img.data_ptr(),
              crows, nchunk, part.data_ptr(), out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    SOFTMAX_FUSED_CALLS += 1
    return out[1:].view(k1, m), out[0]


def _rows_call(X, y, w, tables, search, beta, nsteps, mask, grid):
    global SOFTMAX_FUSED_CALLS
    k1 = _check(X, y, w, tables)
    n, m = X.shape
    dev = X.device
    R = torch.empty((n, k1), dtype=torch.float64, device=dev) if mask & 1 else None
    sums = torch.zeros(nsteps, dtype=torch.float64, device=dev) if search or mask & 2 else None
    if n == 0:
        return R, sums
    img, tw = _rows_image(tables)
    part = torch.empty((nsteps, (n + 63) // 64), dtype=torch.float64, device=dev) if sums is not None else None
    _lib.call("alink_softmax_fused_rows_f64", X.data_ptr(), y.data_ptr(), w.data_ptr(), n, m, k1, img.data_ptr(), tw,
              int(search), float(beta), int(nsteps), int(mask), R.data_ptr() if R is not None else None,
              part.data_ptr() if part is not None else None, sums.data_ptr() if sums is not None else None,
              int(grid), _lib.stream_ptr(dev))
    SOFTMAX_FUSED_CALLS += 1
    return R, sums


def search_losses(X, y, w, W, D, beta: float, nsteps: int, grid: int = 0) -> torch.Tensor:
    """The weighted losses ``sum_i w_i loss_i(W - s beta D)``, ``s = 0 .. nsteps - 1`` (``nsteps <=
    SOFTMAX_FUSED_MAX_STEPS``), from one read of X; independent of ``grid``.  CPU tensors take
    ``search_losses_torch``."""
    if not X.is_cuda:
        return search_losses_torch(X, y, w, W, D, beta, nsteps)
    if not 1 <= nsteps <= SOFTMAX_FUSED_MAX_STEPS:
        raise ValueError(f"nsteps must lie in 1 .. {SOFTMAX_FUSED_MAX_STEPS}")
    return _rows_call(X, y, w, (W, D), 1, beta, nsteps, 0, grid)[1]


def rows(X, y, w, W, want: Sequence[str], grid: int = 0) -> Dict[str, torch.Tensor]:
    """The row pass at ``W``: ``"R"`` -> ``R [n, k1]``, ``"loss"`` -> ``sum w loss`` (0-dim).  CPU tensors take
    ``rows_torch``."""
    mask = sum(_WANT[key] for key in _WANT if key in want)
    if not mask or set(want) - set(_WANT):
        raise ValueError(f"want must name some of {tuple(_WANT)}")
    if not X.is_cuda:
        return rows_torch(X, y, w, W, want)
    R, sums = _rows_call(X, y, w, (W,), 0, 0.0, 1, mask, grid)
    res = {}
    if mask & 1:
        res["R"] = R
    if mask & 2:
        res["loss"] = sums[0]
    return res
