"""Multinomial (softmax) regression on CSR rows (``csrc/softmax_csr.hip``): the row pass and the gradient gather of
``SoftmaxObjFunc`` for a sparse fp64 ``FeatureMatrix`` ``fm`` on the GPU (``m = fm.ncols`` columns, the intercept
column among them; int32 / int64 column indices), coefficients ``W [k1, m]`` (pivot class ``k1`` with logit 0,
``1 <= k1 <= SOFTMAX_CSR_KMAX``), fp64 class indices ``y`` in ``[0, k1]`` and fp64 weights ``w``.  The rows are never
densified, no ``[nnz, k1]`` block is formed and nothing is added by float atomics.

* ``grad(fm, y, w, W)`` -> ``(G [k1, m], sum w loss)``: the row pass writes ``R [n, k1] = w (softmax - onehot)``, the
  gather adds ``G[c, j] = sum v R[i, c]`` over the entries ``(i, j, v)`` through the CSC view and work list of
  ``kmeans_sparse.prepare`` (cached on the matrix), chunk partials of a long column merged in chunk order: the same
  bits for every launch and every ``grid``;
* ``gather(fm, R)`` -> ``Gt [m, k1]``, the second half of ``grad`` alone;
* ``search_losses(fm, y, w, W, D, beta, nsteps)`` -> the ``nsteps`` weighted losses at ``W - s beta D`` from one read
  of the rows, in a fixed order;
* ``rows(fm, y, w, W, want)`` -> a dict with ``"R"``, ``"loss"`` (``sum w loss``) and / or ``"row_loss"`` (``[n]``, the
  rows' losses without the weight);
* ``grad_torch`` / ``search_losses_torch`` / ``rows_torch``: the same results by the former chain, ``fm.mm``, the
  formulas of ``ops/softmax.py`` and ``fm.rmm`` on the guarded entries (CPU matrices take them);
* ``shape_ok`` / ``supported`` / ``selected``: the shape rule, the rule on a GPU, and the gate
  ``sized_gate("ALINK_SOFTMAX_HIP", device, n, SOFTMAX_CSR_MIN_ROWS)``.

An entry whose column is outside ``[0, m)`` adds nothing (``csrc/csr_rows.h``).
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from . import _lib, csr
from . import kmeans_sparse
from .softmax import _lin, _lse_pivot, softmax_grad_torch, softmax_search_torch

__all__ = ["SOFTMAX_CSR_KMAX", "SOFTMAX_CSR_MAX_STEPS", "SOFTMAX_CSR_TABLE_BYTES", "SOFTMAX_CSR_MIN_ROWS", "shape_ok",
           "supported", "selected", "grad", "grad_torch", "gather", "search_losses", "search_losses_torch", "rows",
           "rows_torch"]

SOFTMAX_CSR_KMAX = 64               # one class per lane
SOFTMAX_CSR_MAX_STEPS = 64          # one line-search step per lane
SOFTMAX_CSR_TABLE_BYTES = 2 << 30   # cap of the padded search table [m, 128] fp64: m <= 2^21 columns
SOFTMAX_CSR_MIN_ROWS = 64           # the smallest swept n; gradient + search win from there (profiles/softmax_csr.txt)
SOFTMAX_CSR_ROW_BLOCK = 16          # rows of one loss partial (SMC_RB of the kernel)
SOFTMAX_CSR_CALLS = 0               # launches of the CSR softmax kernels (tests read it)
_WANT = {"R": 1, "loss": 2, "row_loss": 4}


def shape_ok(fm, k1: int) -> bool:
    """The shape rule of the CSR softmax kernels: a matrix the CSR kernels take (``csr.supported``: sparse, fp64
    values, int32 / int64 columns, on a GPU, fewer than 2^31 rows), 1 <= k1 <= SOFTMAX_CSR_KMAX, at least one column
    and the padded search table ``[m, 128]`` within SOFTMAX_CSR_TABLE_BYTES."""
    return (csr.supported(fm) and 1 <= k1 <= SOFTMAX_CSR_KMAX
            and 1 <= fm.ncols and 8 * 128 * fm.ncols <= SOFTMAX_CSR_TABLE_BYTES)


def supported(fm, k1: int) -> bool:
    """Whether the CSR softmax kernels take this matrix: ``shape_ok``, which asks for a GPU matrix already."""
    return shape_ok(fm, k1)


def selected(fm, k1: int) -> bool:
    """The selection rule: a ``supported`` matrix, from ``SOFTMAX_CSR_MIN_ROWS`` rows on (``ALINK_SOFTMAX_HIP=1``:
    always, ``=0``: never); then the project's fall-back rule."""
    return supported(fm, k1) and _lib.sized_gate("ALINK_SOFTMAX_HIP", fm.val.device, fm.nrows, SOFTMAX_CSR_MIN_ROWS)


def _guarded(fm, m: int):
    """The matrix with the entries outside [0, m) turned into (0, 0.0), as the former chain needs it."""
    col, val = csr.clipped(fm, m)
    return type(fm)(crow=fm.crow, col=col, val=val, ncols=m)


def grad_torch(fm, y, w, W) -> Tuple[torch.Tensor, torch.Tensor]:
    """``grad`` by the former chain: ``fm.mm`` for the logits, the softmax formulas, ``fm.rmm``."""
    g = _guarded(fm, W.shape[1])
    R, loss = softmax_grad_torch(g.mm(W.T), y, w)
    return g.rmm(R, W.shape[1]).T.contiguous(), loss


def search_losses_torch(fm, y, w, W, D, beta: float, nsteps: int) -> torch.Tensor:
    """``search_losses`` by the former chain: two ``fm.mm`` and the search formulas."""
    g = _guarded(fm, W.shape[1])
    return softmax_search_torch(g.mm(W.T), g.mm(D.T), y, w, beta, nsteps)


def rows_torch(fm, y, w, W, want: Sequence[str]) -> Dict[str, torch.Tensor]:
    """``rows`` by the former chain; ``"row_loss"`` by the formulas of ``SoftmaxObjFunc.loss_per_sample``."""
    eta = _guarded(fm, W.shape[1]).mm(W.T)
    res = {}
    if "R" in want or "loss" in want:
        res["R"], res["loss"] = softmax_grad_torch(eta, y, w)
    if "row_loss" in want:
        res["row_loss"] = _lse_pivot(eta) - _lin(eta, y)
    return {key: res[key] for key in _WANT if key in want}


def _is_sparse(fm) -> bool:
    return not isinstance(fm, torch.Tensor) and getattr(fm, "dense", 0) is None


def _check(fm, y, w, tables) -> int:
    k1 = tables[0].shape[0] if tables[0].dim() == 2 else 0
    if not supported(fm, k1):
        raise ValueError(f"the CSR softmax kernels need a sparse fp64 GPU matrix with int32 / int64 columns, fewer "
                         f"than 2^31 rows, 1 <= m <= {SOFTMAX_CSR_TABLE_BYTES // 1024} and 1 <= k1 <= {SOFTMAX_CSR_KMAX}")
    dev = fm.val.device
    for t in (y, w):
        if not (t.dtype == torch.float64 and t.is_contiguous() and t.shape == (fm.nrows,) and t.device == dev):
            raise ValueError("y and w must be contiguous fp64 [n] tensors on the rows' device")
    for t in tables:
        if not (t.dtype == torch.float64 and t.shape == (k1, fm.ncols) and t.device == dev):
            raise ValueError("W and D must be fp64 [k1, m] tensors on the rows' device, m the matrix's columns")
    _lib.require()
    return k1


def _rows_call(fm, y, w, tables, beta, nsteps, mask, grid):
    """The row pass: ``(R, row_loss, sums)``, each None unless asked for (search: ``tables`` = (W, D), mask 0)."""
    global SOFTMAX_CSR_CALLS
    k1 = _check(fm, y, w, tables)
    search = len(tables) == 2
    n, m = fm.nrows, fm.ncols
    dev = fm.val.device
    R = torch.empty((n, k1), dtype=torch.float64, device=dev) if mask & 1 else None
    rloss = torch.empty(n, dtype=torch.float64, device=dev) if mask & 4 else None
    sums = torch.zeros(nsteps, dtype=torch.float64, device=dev) if search or mask & 2 else None
    if n == 0:          # nothing is launched for an empty partition
        return R, rloss, sums
    # lane l owns class l: W (and D behind it) transposed and padded to 64 table columns each, T [m, 64 or 128]
    T = torch.cat([csr.padded_transpose(t, 64) for t in tables], 1)
    nb = -(-n // SOFTMAX_CSR_ROW_BLOCK)
    part = torch.empty((nsteps, nb), dtype=torch.float64, device=dev) if sums is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    alive, head = csr.row_args(fm, m)      # alive: the arrays behind head's pointers
    _lib.call("alink_softmax_csr_rows", *head, y.data_ptr(), w.data_ptr(), k1, T.data_ptr(), int(search), float(beta),
              int(nsteps), int(mask), ptr(R), ptr(rloss), ptr(part), ptr(sums), int(grid), _lib.stream_ptr(dev))
    SOFTMAX_CSR_CALLS += 1
    return R, rloss, sums


def gather(fm, R, grid: int = 0) -> torch.Tensor:
    """``X^T R`` as ``Gt [m, k1]`` for ``R [n, k1]``, through the CSC view and the (column, chunk) work list of
    ``kmeans_sparse.prepare``, which is built once and cached on the matrix; columns without entries stay 0."""
    global SOFTMAX_CSR_CALLS
    n, k1 = R.shape
    m, dev = fm.ncols, fm.val.device
    if not (supported(fm, k1) and R.dtype == torch.float64 and R.is_contiguous() and n == fm.nrows and R.device == dev):
        raise ValueError("the gradient gather needs a supported matrix and a contiguous fp64 R [n, k1] on its device")
    Gt = torch.zeros((m, k1), dtype=torch.float64, device=dev)
    csc = kmeans_sparse.prepare(fm, m) if n else None
    if csc is None or csc.nwork == 0:
        return Gt
    part = torch.empty((max(csc.nslots, 1), k1), dtype=torch.float64, device=dev)
    _lib.call("alink_softmax_csr_grad", csc.rows.data_ptr(), csc.vals.data_ptr(), R.data_ptr(), k1, csc.nwork,
              csc.wcol.data_ptr(), csc.wstart.data_ptr(), csc.wlen.data_ptr(), csc.wslot.data_ptr(), csc.nmulti,
              csc.mcol.data_ptr(), csc.mfirst.data_ptr(), csc.mcount.data_ptr(), Gt.data_ptr(), part.data_ptr(),
              int(grid), _lib.stream_ptr(dev))
    SOFTMAX_CSR_CALLS += 1
    return Gt


def grad(fm, y, w, W, grid: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """One gradient pass: ``(G [k1, m], sum w loss (0-dim))``.  On the GPU the same bits for every launch and every
    ``grid``.  CPU matrices take ``grad_torch``; a GPU matrix outside ``supported`` is an error (ask ``selected``
    first)."""
    if _is_sparse(fm) and not fm.val.is_cuda:
        return grad_torch(fm, y, w, W)
    R, _, sums = _rows_call(fm, y, w, (W,), 0.0, 1, 3, grid)
    return gather(fm, R, grid).t().contiguous(), sums[0]


def search_losses(fm, y, w, W, D, beta: float, nsteps: int, grid: int = 0) -> torch.Tensor:
    """The weighted losses ``sum_i w_i loss_i(W - s beta D)``, ``s = 0 .. nsteps - 1`` (``nsteps <=
    SOFTMAX_CSR_MAX_STEPS``), from one read of the rows; independent of ``grid``.  CPU matrices take
    ``search_losses_torch``."""
    if _is_sparse(fm) and not fm.val.is_cuda:
        return search_losses_torch(fm, y, w, W, D, beta, nsteps)
    if not 1 <= nsteps <= SOFTMAX_CSR_MAX_STEPS:
        raise ValueError(f"nsteps must lie in 1 .. {SOFTMAX_CSR_MAX_STEPS}")
    return _rows_call(fm, y, w, (W, D), beta, nsteps, 0, grid)[2]


def rows(fm, y, w, W, want: Sequence[str], grid: int = 0) -> Dict[str, torch.Tensor]:
    """The row pass at ``W``: ``"R"`` -> ``R [n, k1]``, ``"loss"`` -> ``sum w loss`` (0-dim), ``"row_loss"`` -> the
    rows' losses ``[n]`` without the weight.  CPU matrices take ``rows_torch``."""
    mask = sum(_WANT[key] for key in _WANT if key in want)
    if not mask or set(want) - set(_WANT):
        raise ValueError(f"want must name some of {tuple(_WANT)}")
    if _is_sparse(fm) and not fm.val.is_cuda:
        return rows_torch(fm, y, w, W, want)
    R, rloss, sums = _rows_call(fm, y, w, (W,), 0.0, 1, mask, grid)
    res = {}
    if mask & 1:
        res["R"] = R
    if mask & 2:
        res["loss"] = sums[0]
    if mask & 4:
        res["row_loss"] = rloss
    return res
