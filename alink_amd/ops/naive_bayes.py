"""Naive Bayes for text / count vectors on one rank's rows (``models/classification/naive_bayes.py``): the per-label
sums of training and the fused score / argmax / softmax of prediction, on the row kinds of ``ops/kmeans_rows.py``.

* ``train_rows(fm, d, w)`` / ``predict_rows(fm, d)`` -> the rows object of a ``FeatureMatrix``: a sparse column as CSR
  whatever its width, a dense column as an fp64 block under ``d`` columns; ``supported(fm)`` says whether the HIP
  kernels take the column (a sparse fp64 column, or a dense fp64 one of at most 1024 columns);
* ``label_sums(rows, code, w, L)`` -> ``([L, d] feature sums, [L] weight sums)``, fp64: ``Rows.child_stats`` on the
  label codes, so no ``[n, L]`` one-hot and no ``[nnz, L]`` product; with weights the rows hold ``val * w[row]``;
* ``predict(rows, M, off, bernoulli, want_prob)`` -> ``(pred int32 [n], prob fp64 [n, L] or None, bad)``: the score
  of class c is ``off[c] + x . M[c, :]`` (Multinomial: ``M = theta``, ``off = pi``; Bernoulli:
  ``M = theta - log(1 - e^theta)``, ``off = pi + phi``), ``pred`` the first strict maximum (-1 for a row with no score
  above -inf, NaN never wins), ``prob`` the log-sum-exp softmax, ``bad`` (Bernoulli; else None) an int32 word that is
  non-zero when a value inside the model's columns is neither 0 nor 1.  Entries of a CSR row at or past the model
  width add nothing;
* ``has_duplicate_index(fm)``: whether a CSR row stores an index twice in a row of its (sorted) entries.

GPU: ``csrc/naive_bayes.hip`` — CSR rows one wave per row on the row walk of ``csrc/csr_rows.h``, fp64 rows
(1 <= d <= 1024) on the fp64 matrix cores with the table staged in LDS (``csrc/dense64_mfma.h``); the sums through
the sort-based dense accumulate and the CSC accumulate.  No float atomics: bitwise identical from run to run and for
every grid.  Every other kind (CPU rows, an empty partition): ``predict_torch``, chunked over rows; CSR rows never
become a dense matrix.

With a GPU present a missing kernel library raises, unless ``ALINK_ALLOW_TORCH_FALLBACK=1``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib, csr, kmeans_dense64 as kd64, kmeans_rows as krows
from .kmeans_sparse import DENSE_DMAX

__all__ = ["NB_MIN_ROWS", "supported", "train_rows", "predict_rows", "label_sums", "Table", "predict",
           "predict_torch", "has_duplicate_index"]

NB_MIN_ROWS = 1         # no crossover found: the device path measured faster from one row on (profiles/naive_bayes.txt)
NB_CALLS = 0            # launches of the HIP prediction kernels (tests read it)
SUM_CALLS = 0           # calls of label_sums (tests read it)
TORCH_CHUNK = 1 << 14   # dense rows per chunk of the torch path
SPARSE_CHUNK = 1 << 12  # CSR rows per chunk of the torch path (the gathered [entries, L] block sets the size)


def supported(fm) -> bool:
    """Whether the device path takes this column: sparse fp64 rows, or dense fp64 rows of 1 .. 1024 columns."""
    if fm.is_sparse:
        return fm.val.dtype == torch.float64 and fm.col.dtype in (torch.int32, torch.int64)
    return fm.dense.dtype == torch.float64 and fm.dense.dim() == 2 and 1 <= fm.ncols <= DENSE_DMAX


def _rows(fm, d: int, w: Optional[torch.Tensor] = None):
    if fm.is_sparse:
        view = krows.sparse_rows(fm, d, "EUCLIDEAN")
        if w is not None:       # rounded products, as the reference's val[i] * w
            view = krows.sparse_view(view, d, val=view.val * w[view.row_ids()])
        return krows._SparseRows(view, "EUCLIDEAN")
    X = fm.dense.to(torch.float64)
    if X.shape[1] < d:
        X = torch.nn.functional.pad(X, (0, d - X.shape[1]))
    elif X.shape[1] > d:
        X = X[:, :d]
    if w is not None:
        X = X * w[:, None]
    X = X.contiguous()
    return (krows._Dense64Rows if kd64.dense64_supported(X, 1) else krows._TorchRows)(X, "EUCLIDEAN")


def train_rows(fm, d: int, w: Optional[torch.Tensor] = None):
    """The rows of training under the global vector size ``d``, their values times the row weights ``w`` [n]."""
    return _rows(fm, int(d), w)


def predict_rows(fm, d: int):
    """The rows of prediction under the model width ``d``: dense rows padded or cut to it; CSR rows as they are (the
    entries at or past ``d`` are dropped where they are read)."""
    return _rows(fm, int(d))


def label_sums(rows, code: torch.Tensor, w: Optional[torch.Tensor], L: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``([L, d] fp64 feature sums, [L] fp64 weight sums)`` of the rows per label code (int32 / int64 [n], every
    value in [0, L)); ``rows`` are ``train_rows``, weighted already, ``w`` their weights or None."""
    global SUM_CALLS
    SUM_CALLS += 1
    L = int(L)
    feat = rows.child_stats(code, L, sqnorm=False)[:, :rows.d]
    if w is None:
        wsum = torch.bincount(code.to(torch.int64), minlength=L)[:L].to(torch.float64)
    else:
        wsum = kd64.accumulate(w.to(torch.float64)[:, None].contiguous(), code, L)[:, 0]
    return feat, wsum


def has_duplicate_index(fm) -> bool:
    """Whether two neighbouring entries of one CSR row have the same index: a row of sorted entries (what the vector
    parsers and the device feature path produce) then stores an index twice."""
    if not fm.is_sparse or fm.col.numel() < 2:
        return False
    rid = fm.row_ids()
    return bool(((fm.col[1:] == fm.col[:-1]) & (rid[1:] == rid[:-1])).any())


class Table:
    """The model operand ``M`` [L, d], ``off`` [L] with the kernels' forms of it, built once per device."""

    def __init__(self, M, off):
        self.M = torch.as_tensor(M, dtype=torch.float64).contiguous()
        self.off = torch.as_tensor(off, dtype=torch.float64).contiguous()
        if self.M.dim() != 2 or self.M.shape[0] < 1 or self.off.shape != (self.M.shape[0],):
            raise ValueError("naive Bayes table shape mismatch")
        self.L, self.d = (int(v) for v in self.M.shape)
        self._forms = {}

    def on(self, dev):
        """(M, off) on ``dev``."""
        key = ("plain", str(dev))
        if key not in self._forms:
            self._forms[key] = (self.M.to(dev), self.off.to(dev))
        return self._forms[key]

    def csr(self, dev):
        """(Mt [d, kp], off [kp] with -inf on the padded classes, kp): ``csr.padded_transpose``."""
        key = ("csr", str(dev))
        if key not in self._forms:
            M, off = self.on(dev)
            kp = csr.kp(self.L)
            offp = torch.full((kp,), float("-inf"), dtype=torch.float64, device=dev)
            offp[:self.L] = off
            self._forms[key] = (csr.padded_transpose(M, kp), offp, kp)
        return self._forms[key]

    def f64(self, dev):
        """(img, init, nt, nblk): ``kmeans_dense64.centroid_image`` of M, the accumulators starting at ``off``."""
        key = ("f64", str(dev))
        if key not in self._forms:
            M, off = self.on(dev)
            img, init, nt, nblk = kd64.centroid_image(M, 1, dev)      # the COSINE code: plain dots
            init[:self.L] = off
            self._forms[key] = (img, init, nt, nblk)
        return self._forms[key]


# ---------------------------------------------------------------------------------------------------
# torch path (CPU, an empty partition; the base of the tests' oracle)
# ---------------------------------------------------------------------------------------------------
def _finish(S: torch.Tensor, want_prob: bool):
    """(pred int32 [m], prob [m, L] or None) of the scores S [m, L]."""
    Sf = torch.where(S != S, torch.full_like(S, float("-inf")), S)
    m, idx = Sf.max(1)          # the first of equal maxima
    pred = torch.where(m > float("-inf"), idx, torch.full_like(idx, -1)).to(torch.int32)
    if not want_prob:
        return pred, None
    lse = m + torch.log(torch.exp(S - m[:, None]).sum(1))
    return pred, torch.exp(S - lse[:, None])


def _is01(v: torch.Tensor) -> torch.Tensor:
    return (v == 0.0) | (v == 1.0)


def predict_torch(rows, M, off=None, bernoulli: bool = False, want_prob: bool = False):
    """Torch implementation of ``predict``, chunked over rows."""
    table = M if isinstance(M, Table) else Table(M, off)
    dev = rows.device
    M, off = table.on(dev)
    L, d, n = table.L, table.d, rows.n
    pred = torch.zeros(n, dtype=torch.int32, device=dev)
    prob = torch.zeros((n, L), dtype=torch.float64, device=dev) if want_prob else None
    bad = torch.zeros(1, dtype=torch.int32, device=dev) if bernoulli else None
    if isinstance(rows, krows._SparseRows):
        fm = rows.X
        Mt = M.t().contiguous()
        for s in range(0, n, SPARSE_CHUNK):
            e = min(n, s + SPARSE_CHUNK)
            a, b = int(fm.crow[s]), int(fm.crow[e])
            S = off[None, :].repeat(e - s, 1)
            if b > a:
                col = fm.col[a:b].to(torch.int64)
                ok = (col >= 0) & (col < d)         # an entry outside the model adds nothing and is not checked
                col, v = col[ok], fm.val[a:b][ok].to(torch.float64)
                rid = torch.repeat_interleave(torch.arange(e - s, device=dev), fm.crow[s + 1:e + 1] - fm.crow[s:e],
                                              output_size=b - a)[ok]
                S.index_add_(0, rid, v[:, None] * Mt[col])
                if bernoulli and not bool(_is01(v).all()):
                    bad.fill_(1)
            p, q = _finish(S, want_prob)
            pred[s:e] = p
            if want_prob:
                prob[s:e] = q
        return pred, prob, bad
    X = rows.X
    if int(X.shape[1]) != d:
        raise ValueError("dense rows must have the model's width")
    for s in range(0, n, TORCH_CHUNK):
        x = X[s:s + TORCH_CHUNK].to(torch.float64)
        if bernoulli and not bool(_is01(x).all()):
            bad.fill_(1)
        p, q = _finish(x @ M.T + off[None, :], want_prob)
        pred[s:s + TORCH_CHUNK] = p
        if want_prob:
            prob[s:s + TORCH_CHUNK] = q
    return pred, prob, bad


# ---------------------------------------------------------------------------------------------------
# HIP path
# ---------------------------------------------------------------------------------------------------
def _hip_kind(rows, L: int):
    """"f64" / "csr" when the HIP kernels take these rows, else None (an empty partition launches nothing)."""
    if rows.n == 0:
        return None
    if isinstance(rows, krows._Dense64Rows):
        return "f64" if kd64.use_hip(rows.X, L) else None
    if isinstance(rows, krows._SparseRows):
        return "csr" if csr.use_hip(rows.X) else None
    return None


def predict(rows, M, off=None, bernoulli: bool = False, want_prob: bool = False, grid: int = 0):
    """``(pred int32 [n], prob fp64 [n, L] or None, bad int32 [1] or None)`` of every row against the table ``M``
    [L, d] (or a ``Table``, which keeps the kernels' operands between calls) and ``off`` [L].  On the GPU the same
    bits for every launch and every ``grid``."""
    global NB_CALLS
    table = M if isinstance(M, Table) else Table(M, off)
    kind = _hip_kind(rows, table.L)
    if kind is None:
        return predict_torch(rows, table, None, bernoulli, want_prob)
    dev, n, L, d = rows.device, rows.n, table.L, table.d
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    prob = torch.empty((n, L), dtype=torch.float64, device=dev) if want_prob else None
    bad = torch.zeros(1, dtype=torch.int32, device=dev) if bernoulli else None
    tail = (int(bool(bernoulli)), pred.data_ptr(), prob.data_ptr() if want_prob else None,
            bad.data_ptr() if bernoulli else None, int(grid), _lib.stream_ptr(dev))
    if kind == "f64":
        if rows.d != d:
            raise ValueError("dense rows must have the model's width")
        img, init, nt, nblk = table.f64(dev)
        _lib.call("alink_nb_rows_f64", rows.X.data_ptr(), n, d, img.data_ptr(), init.data_ptr(), L, nt, nblk, *tail)
    else:
        Mt, offp, kp = table.csr(dev)
        alive, head = csr.row_args(rows.X, d)      # alive: the arrays behind head's pointers
        _lib.call("alink_nb_rows_csr", *head, Mt.data_ptr(), offp.data_ptr(), L, kp, *tail)
    NB_CALLS += 1
    return pred, prob, bad
