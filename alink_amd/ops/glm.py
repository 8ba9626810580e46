"""Generalized linear models on the device (``csrc/glm.hip``): the fused IRLS statistics pass and the per-row pass,
for contiguous fp64 GPU rows ``X [n, k]`` with ``1 <= k <= GLM_KMAX``.

* ``irls_stats(X, y, w, off, beta, intercept, fam, link, vp, lp, mode)`` -> ``(sum ww^2, G [(k+2), (k+2)])`` with
  ``G = sum_i ww_i a_i a_i^T`` over the augmented rows ``a_i = [x_i | 1 | z_i]``: the working label ``z`` and weight
  ``ww`` of ``mode`` (``PLAIN``: ``y - off``, ``w``; ``INIT``: the first weighted least squares of IRLS; ``STEP``: one
  IRLS iteration at ``beta``, ``intercept``), the linear predictor, family and link arithmetic and the weighted Gram
  on the fp64 matrix cores in one pass that reads X once.  Chunk partials (at most ``GLM_SCRATCH_BYTES``) are merged
  in chunk order, no float atomics: the same bits for every launch and every ``grid``;
* ``rows(X, y, w, off, beta, intercept, fam, link, vp, lp, want)`` -> a dict of the columns asked for in ``want``
  (``"pred"``, ``"eta"``, ``"resid"`` -> ``dres, pres, wres, rres``, ``"zw"`` -> ``z, ww``) and, with ``"sums"``,
  ``sums [4] = [deviance, deviance at unlink(cnull + off), pearson^2, w]`` in a fixed order;
* ``irls_stats_torch`` / ``rows_torch``: the same results by the torch formulas of ``models/regression/glm.py`` (CPU
  tensors take them);
* ``shape_ok`` / ``supported`` / ``selected``: the shape rule, the rule on a GPU, and the gate
  ``sized_gate("ALINK_GLM_HIP", device, n, GLM_MIN_ROWS)``.

``fam`` is one of ``FAMILIES``, ``link`` one of ``LINKS`` (probit is not covered: no device ``ndtri`` has been pinned
against ``torch.special.ndtri``); ``vp`` / ``lp`` are tweedie's variance power and the power link's exponent.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from .gemm import tn_matmul

__all__ = ["GLM_KMAX", "GLM_MIN_ROWS", "GLM_SCRATCH_BYTES", "FAMILIES", "LINKS", "PLAIN", "INIT", "STEP", "shape_ok",
           "supported", "selected", "glm_chunk_rows", "irls_stats", "irls_stats_torch", "rows", "rows_torch"]

GLM_KMAX = 126                  # the augmented row [x | 1 | z] is at most 128 entries, 8 tiles of 16
GLM_MIN_ROWS = 1                # no crossover found: the sweep from 64 rows up never favours the former path (profiles/glm.txt)
GLM_SCRATCH_BYTES = 128 << 20   # cap of the chunk partials [nchunk, 1 + (k + 2)^2]
GLM_CHUNKS = 1024               # row chunks of the IRLS pass at most: the merge adds them one after another
GLM_CHUNK_MIN_ROWS = 256        # and no chunk shorter than this, so that a small n has few partials to merge
GLM_CALLS = 0                   # launches of the HIP GLM kernels (tests read it)
FAMILIES = ("gaussian", "binomial", "poisson", "gamma", "tweedie")
LINKS = ("identity", "log", "logit", "inverse", "sqrt", "cloglog", "power")
PLAIN, INIT, STEP = 0, 1, 2
_WANT = {"pred": (1, ("pred",)), "eta": (2, ("eta",)), "resid": (4, ("dres", "pres", "wres", "rres")),
         "zw": (8, ("z", "ww")), "sums": (16, ())}


def shape_ok(X, fam: str, link: str) -> bool:
    """The shape rule of the GLM kernels: a contiguous fp64 [n, k] tensor, 1 <= k <= GLM_KMAX, n < 2^31, a covered
    family and link."""
    return (isinstance(X, torch.Tensor) and X.dtype == torch.float64 and X.dim() == 2 and X.is_contiguous()
            and 1 <= X.shape[1] <= GLM_KMAX and X.shape[0] < 2 ** 31 and fam in FAMILIES and link in LINKS)


def supported(X, fam: str, link: str) -> bool:
    """Whether the GLM kernels take these rows: ``shape_ok`` rows on a GPU."""
    return shape_ok(X, fam, link) and X.is_cuda


def selected(X, fam: str, link: str) -> bool:
    """The selection rule: ``supported`` rows, from ``GLM_MIN_ROWS`` rows on (``ALINK_GLM_HIP=1``: always, ``=0``:
    never); then the project's fall-back rule."""
    return supported(X, fam, link) and _lib.sized_gate("ALINK_GLM_HIP", X.device, X.shape[0], GLM_MIN_ROWS)


def glm_chunk_rows(n: int, k: int) -> int:
    """Rows per chunk of the IRLS pass, from (n, k) alone: ``_lib.chunk_rows`` under the GLM constants."""
    return _lib.chunk_rows(n, 1 + (k + 2) ** 2, GLM_SCRATCH_BYTES, GLM_CHUNKS, GLM_CHUNK_MIN_ROWS)


def _family_link(fam, link, vp, lp):
    from ..models.regression.glm import FamilyLink          # the torch formulas live with the model
    return FamilyLink(fam, vp, link, lp)


def _working_torch(fl, X, y, w, off, beta, intercept, mode):
    if mode == PLAIN:
        return y - off, w
    if mode == INIT:
        return fl.predict(fl.family.initialize(y, w)) - off, w
    eta = X @ beta + intercept + off
    mu = fl.fitted(eta)
    deriv = fl.link.derivative(mu)
    return eta - off + (y - mu) * deriv, w / (deriv * deriv * fl.family.variance(mu))


def irls_stats_torch(X, y, w, off, beta, intercept, fam, link, vp, lp, mode) -> Tuple[torch.Tensor, torch.Tensor]:
    """``irls_stats`` in plain torch: the working label and weight, then one ``[X|1|z]^T diag(ww) [X|1|z]`` GEMM."""
    z, ww = _working_torch(_family_link(fam, link, vp, lp), X, y, w, off, beta, intercept, mode)
    Z = torch.cat([X, torch.ones((X.shape[0], 1), dtype=X.dtype, device=X.device), z[:, None]], 1)
    return (ww * ww).sum(), tn_matmul(Z, Z * ww[:, None])


def rows_torch(X, y, w, off, beta, intercept, fam, link, vp, lp, want: Sequence[str], mode: int = STEP,
               cnull: float = 0.0) -> Dict[str, torch.Tensor]:
    """``rows`` in plain torch (the formulas of ``glm_residuals`` and ``glm_summary``)."""
    fl = _family_link(fam, link, vp, lp)
    if off is None:
        off = torch.zeros(X.shape[0], dtype=X.dtype, device=X.device)
    eta = X @ beta + intercept + off
    pred = fl.fitted(eta)
    out = {}
    if "pred" in want:
        out["pred"] = pred
    if "eta" in want:
        out["eta"] = eta
    if "resid" in want or "sums" in want:
        dev = fl.family.deviance(y, pred, w)
        pr = (y - pred) * torch.sqrt(w) / torch.sqrt(fl.family.variance(pred))
    if "resid" in want:
        dr = torch.sqrt(torch.clamp(dev, min=0.0))
        out.update(dres=torch.where(y <= pred, -dr, dr), pres=pr, wres=(y - pred) * fl.link.derivative(pred),
                   rres=y - pred)
    if "zw" in want:
        out["z"], out["ww"] = _working_torch(fl, X, y, w, off, beta, intercept, mode)
    if "sums" in want:
        null_dev = fl.family.deviance(y, fl.link.unlink(cnull + off), w)
        out["sums"] = torch.stack([dev.sum(), null_dev.sum(), (pr * pr).sum(), w.sum()])
    return out


def _check(X, fam, link, others):
    if not supported(X, fam, link):
        raise ValueError(f"the GLM kernels need contiguous fp64 [n, k] rows with 1 <= k <= {GLM_KMAX}, fewer than 2^31 "
                         f"rows, a family of {FAMILIES} and a link of {LINKS}")
    for t in others:
        if t is not None and not (t.dtype == torch.float64 and t.is_contiguous() and t.shape == (X.shape[0],)
                                  and t.device == X.device):
            raise ValueError("y, w and off must be contiguous fp64 [n] tensors on the rows' device")
    _lib.require()


def _beta(beta, k, dev):
    b = torch.as_tensor(beta, dtype=torch.float64).to(dev).contiguous()
    if b.shape != (k,):
        raise ValueError("beta must have one entry per column")
    return b


def irls_stats(X, y, w, off, beta, intercept, fam, link, vp, lp, mode, grid: int = 0,
               chunk_rows: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """One IRLS statistics pass: ``(sum ww^2 (0-dim), G [(k+2), (k+2)])``.  On the GPU the same bits for every launch
    and every ``grid`` (``chunk_rows``, a multiple of 64, overrides the chunk length, which otherwise follows from
    (n, k) alone).  ``beta`` / ``intercept`` are read in mode ``STEP`` only.  CPU tensors take ``irls_stats_torch``;
    GPU rows outside ``supported`` are an error (ask ``selected`` first)."""
    global GLM_CALLS
    if not X.is_cuda:
        return irls_stats_torch(X, y, w, off, beta, intercept, fam, link, vp, lp, mode)
    n, k = X.shape
    dev = X.device
    if n == 0:          # nothing is launched for an empty partition
        return (torch.zeros((), dtype=torch.float64, device=dev),
                torch.zeros((k + 2, k + 2), dtype=torch.float64, device=dev))
    _check(X, fam, link, (y, w, off))
    b = _beta(beta, k, dev) if mode == STEP else None
    crows = int(chunk_rows) if chunk_rows > 0 else glm_chunk_rows(n, k)
    nchunk, part, out = _lib.chunk_buffers(n, crows, 1 + (k + 2) ** 2, dev)
    _lib.call("alink_glm_irls_f64", X.data_ptr(), y.data_ptr(), w.data_ptr(), off.data_ptr(), n, k,
              b.data_ptr() if b is not None else None, float(intercept), FAMILIES.index(fam), LINKS.index(link),
              float(vp), float(lp), int(mode), crows, nchunk, part.data_ptr(), out.data_ptr(), int(grid),
              _lib.stream_ptr(dev))
    GLM_CALLS += 1
    return out[0], out[1:].view(k + 2, k + 2)


def rows(X, y, w, off, beta, intercept, fam, link, vp, lp, want: Sequence[str], mode: int = STEP, cnull: float = 0.0,
         grid: int = 0) -> Dict[str, torch.Tensor]:
    """The per-row pass: the columns and sums named in ``want`` (see the module text).  ``y`` and ``w`` may be None
    when only ``"pred"`` / ``"eta"`` are asked for, ``off`` may be None (zero).  CPU tensors take ``rows_torch``."""
    global GLM_CALLS
    if not X.is_cuda:
        return rows_torch(X, y, w, off, beta, intercept, fam, link, vp, lp, want, mode, cnull)
    mask = 0
    names = []
    for key in _WANT:               # the kernel's column order
        if key in want:
            mask |= _WANT[key][0]
            names += _WANT[key][1]
    if not mask or set(want) - set(_WANT):
        raise ValueError(f"want must name some of {tuple(_WANT)}")
    if (mask & 28) and (y is None or w is None):
        raise ValueError("residuals, working values and sums need y and w")
    n, k = X.shape
    dev = X.device
    if n == 0:
        res = {name: torch.zeros(0, dtype=torch.float64, device=dev) for name in names}
        if mask & 16:
            res["sums"] = torch.zeros(4, dtype=torch.float64, device=dev)
        return res
    _check(X, fam, link, (y, w, off))
    b = _beta(beta, k, dev)
    out = torch.empty((len(names), n), dtype=torch.float64, device=dev) if names else None
    nb = (n + 63) // 64         # one partial per 64-row batch, then one per 4096 batches
    part = torch.empty((nb + -(-nb // 4096), 4), dtype=torch.float64, device=dev) if mask & 16 else None
    sums = torch.empty(4, dtype=torch.float64, device=dev) if mask & 16 else None

    def ptr(t: Optional[torch.Tensor]):
        return t.data_ptr() if t is not None else None
    _lib.call("alink_glm_rows_f64", X.data_ptr(), ptr(y), ptr(w), ptr(off), n, k, b.data_ptr(), float(intercept),
              FAMILIES.index(fam), LINKS.index(link), float(vp), float(lp), int(mode), mask, float(cnull), ptr(out),
              ptr(part), ptr(sums), int(grid), _lib.stream_ptr(dev))
    GLM_CALLS += 1
    res = {name: out[i] for i, name in enumerate(names)}
    if mask & 16:
        res["sums"] = sums
    return res
