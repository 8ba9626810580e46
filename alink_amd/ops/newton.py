"""Newton's method for the linear family on the device (``csrc/newton.hip``): the fused Hessian, gradient and loss
pass of ``OptimObjFunc.calc_hessian_gradient_loss``, for contiguous fp64 GPU rows ``X [n, k]`` with
``1 <= k <= NEWTON_KMAX``.

* ``unary_sums(X, y, w, coef, code, param)`` -> ``(H [d, d], g [d], sum w, sum l)`` from one read of X:
  ``H = sum_i w_i l''(eta_i, y_i) x_i x_i^T``, ``g = sum_i w_i l'(eta_i, y_i) x_i`` and the unweighted loss sum, for
  the loss codes 0..8 of ``ops/linear.loss_code`` (``d = k``), or with ``code = AFT`` the accelerated-failure-time
  objective of ``AftRegObjFunc`` (``coef [k + 1]``, the last entry ``log sigma``, ``w`` the censor indicator,
  ``d = k + 1``, the weight sum the row count).  The Gram runs on the fp64 matrix cores; chunk partials (at most
  ``NEWTON_SCRATCH_BYTES``) are merged in chunk order, no float atomics: the same bits for every launch and ``grid``;
* ``supported`` / ``selected``: the shape rule on a GPU, and the gate
  ``sized_gate("ALINK_NEWTON_HIP", device, n, NEWTON_MIN_ROWS)``;
* ``softmax_sums(X, y, w, W)`` -> ``(H [k1 m, k1 m], G [k1, m], sum w, sum l)`` of ``SoftmaxObjFunc`` from one launch:
  ``H[(s,.),(t,.)] = sum_i w_i (delta_st phi_is - phi_is phi_it) x_i x_i^T`` in the ``[k][featDim]`` layout, for
  ``1 <= k1 <= NEWTON_SOFTMAX_KMAX`` and ``k1 m <= NEWTON_SOFTMAX_DMAX``; only the class pairs ``s <= t`` are computed
  and the merge writes the transposed blocks, so H is exactly symmetric.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib

__all__ = ["NEWTON_KMAX", "NEWTON_MIN_ROWS", "NEWTON_SCRATCH_BYTES", "AFT", "supported", "selected",
           "newton_chunk_rows", "unary_sums", "softmax_sums", "NEWTON_SOFTMAX_KMAX", "NEWTON_SOFTMAX_DMAX"]

NEWTON_KMAX = 128               # columns of X and entries of coef at most: 8 tiles of 16
NEWTON_SOFTMAX_KMAX = 64        # classes without the pivot: four class tiles of 16
NEWTON_SOFTMAX_DMAX = 1024      # k1 m at most (the reference's Newton preallocates a Hessian of 1000 features)
NEWTON_MIN_ROWS = 64            # the smallest swept size: the former path wins nowhere above (profiles/newton.txt)
NEWTON_SCRATCH_BYTES = 128 << 20    # cap of the chunk partials [nchunk, 4 + k + k^2]
NEWTON_CHUNKS = 1024            # row chunks at most: the merge adds them one after another
NEWTON_CHUNK_MIN_ROWS = 256     # and no chunk shorter than this, so that a small n has few partials to merge
NEWTON_CALLS = 0                # launches of the HIP Newton kernels (tests read it)
AFT = 9                         # the loss code of the AFT objective, behind the unary codes 0..8
_SUMS = 4                       # leading entries of the kernel's result: sum w, sum l and AFT's two corner sums


def supported(X, d: int = None, k1: int = 1) -> bool:
    """Whether the Newton kernels take these rows under a coefficient vector of ``d`` entries (default: one per
    column): a contiguous fp64 [n, k] GPU tensor, 1 <= k, d <= NEWTON_KMAX, n < 2^31; for the softmax pass with
    ``k1`` classes beside the pivot also k1 <= NEWTON_SOFTMAX_KMAX and k1 k <= NEWTON_SOFTMAX_DMAX.  Sparse rows
    have no dense tensor (``None``) and are not taken."""
    if not (isinstance(X, torch.Tensor) and X.dtype == torch.float64 and X.dim() == 2 and X.is_contiguous()
            and X.is_cuda and X.shape[0] < 2 ** 31):
        return False
    d = X.shape[1] if d is None else d
    return 1 <= X.shape[1] <= d <= NEWTON_KMAX and 1 <= k1 <= NEWTON_SOFTMAX_KMAX and \
        k1 * X.shape[1] <= NEWTON_SOFTMAX_DMAX


def selected(X, d: int = None, k1: int = 1) -> bool:
    """The selection rule: ``supported`` rows, from ``NEWTON_MIN_ROWS`` rows on (``ALINK_NEWTON_HIP=1``: always,
    ``=0``: never); then the project's fall-back rule."""
    return supported(X, d, k1) and _lib.sized_gate("ALINK_NEWTON_HIP", X.device, X.shape[0], NEWTON_MIN_ROWS)


def newton_chunk_rows(n: int, k: int) -> int:
    """Rows per chunk of the pass, from (n, k) alone: ``_lib.chunk_rows`` under the Newton constants."""
    return _lib.chunk_rows(n, _SUMS + k + k * k, NEWTON_SCRATCH_BYTES, NEWTON_CHUNKS, NEWTON_CHUNK_MIN_ROWS)


def unary_sums(X, y, w, coef, code: int, param: float = 0.0, grid: int = 0,
               chunk_rows: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """One fused Newton pass: ``(H [d, d], g [d], sum w (0-dim), sum l (0-dim))`` on the rows' device, ``d`` the
    length of ``coef`` (``k``, or ``k + 1`` with ``code = AFT``).  The same bits for every launch and every ``grid``
    (``chunk_rows``, a multiple of 64, overrides the chunk length, which otherwise follows from (n, k) alone)."""
    global NEWTON_CALLS
    n, k = X.shape
    d = k + 1 if code == AFT else k
    if not supported(X, d) or n == 0:
        raise ValueError(f"the Newton kernels need contiguous fp64 [n, k] GPU rows with n >= 1 and at most "
                         f"{NEWTON_KMAX} coefficients")
    if not 0 <= int(code) <= AFT:
        raise ValueError("code must be a loss code of ops/linear.loss_code, or AFT")
    dev = X.device
    for t, shape in ((y, (n,)), (w, (n,)), (coef, (d,))):
        if not (t.dtype == torch.float64 and t.is_contiguous() and t.shape == shape and t.device == dev):
            raise ValueError("y, w [n] and coef [d] must be contiguous fp64 tensors on the rows' device")
    _lib.require()
    crows = int(chunk_rows) if chunk_rows > 0 else newton_chunk_rows(n, k)
    nchunk, part, out = _lib.chunk_buffers(n, crows, _SUMS + k + k * k, dev)
    _lib.call("alink_newton_unary_f64", X.data_ptr(), y.data_ptr(), w.data_ptr(), coef.data_ptr(), n, k, int(code),
              float(param), crows, nchunk, part.data_ptr(), out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    NEWTON_CALLS += 1
    g, H = out[_SUMS:_SUMS + k], out[_SUMS + k:].view(k, k)
    if code == AFT:         # the row and column of log sigma: only their corner is filled, as AftRegObjFunc has it
        g = torch.cat([g, out[2:3]])
        H = torch.nn.functional.pad(H, (0, 1, 0, 1))
        H[k, k] = out[3]
    return H, g, out[0], out[1]


def softmax_sums(X, y, w, W, grid: int = 0,
                 chunk_rows: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fused softmax Newton pass at the coefficients ``W [k1, m]``: ``(H [k1 m, k1 m], G [k1, m], sum w, sum l)``
    on the rows' device, the loss sum unweighted.  The same bits for every launch and every ``grid``."""
    global NEWTON_CALLS
    from .softmax_fused import _grad_image           # the tile-outermost image the logits read
    n, m = X.shape
    k1 = W.shape[0]
    if not supported(X, m, k1) or n == 0 or W.shape != (k1, m):
        raise ValueError(f"the softmax Newton kernel needs contiguous fp64 [n, m] GPU rows with n >= 1, m <= "
                         f"{NEWTON_KMAX}, k1 <= {NEWTON_SOFTMAX_KMAX} and k1 m <= {NEWTON_SOFTMAX_DMAX}")
    dev = X.device
    for t in (y, w):
        if not (t.dtype == torch.float64 and t.is_contiguous() and t.shape == (n,) and t.device == dev):
            raise ValueError("y and w must be contiguous fp64 [n] tensors on the rows' device")
    _lib.require()
    D = k1 * m
    P = 2 + D + D * D
    crows = int(chunk_rows) if chunk_rows > 0 else \
        _lib.chunk_rows(n, P, NEWTON_SCRATCH_BYTES, NEWTON_CHUNKS, NEWTON_CHUNK_MIN_ROWS)
    nchunk, part, out = _lib.chunk_buffers(n, crows, P, dev)
    img = _grad_image(W.to(dev, torch.float64))
    _lib.call("alink_newton_softmax_f64", X.data_ptr(), y.data_ptr(), w.data_ptr(), n, m, k1, img.data_ptr(), crows,
              nchunk, part.data_ptr(), out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    NEWTON_CALLS += 1
    return out[2 + D:].view(D, D), out[2:2 + D].view(k1, m), out[0], out[1]
