"""Multilayer perceptron classifier on the device (``csrc/mlp_fused.hip``): the fused forward / backward pass and the
forward row pass of ``MlpObjFunc`` and ``MlpcModelMapper``, for contiguous fp64 GPU rows ``X [n, d0]``, ``layers =
[d0, h.., C]`` with 1 to 3 affine layers (sigmoid hidden layers, a softmax + cross-entropy top), the flat weights
``coef`` in the layout of ``weight_size`` (per layer ``W [in x out]`` row-major, then ``b [out]``), fp64 class indices
``y`` in ``[0, C)`` and fp64 weights ``w``.

* ``fused_grad(X, y, w, coef, layers)`` -> ``(gradient [nw], sum w loss)`` for ``d0 <= MLP_FUSED_MAX_IN``: every layer's
  products, the sigmoids, the softmax and the weight Grams on the fp64 matrix cores in one pass that reads X once and
  writes no ``[n, width]`` block.  Chunk partials (at most ``MLP_SCRATCH_BYTES``) are merged in chunk order, no float
  atomics: the same bits for every launch and every ``grid``;
* ``search_losses(X, y, w, coef, dirv, layers, beta, nsteps)`` -> the ``nsteps <= MLP_FUSED_MAX_STEPS`` weighted losses
  at ``coef - s beta dirv`` from one pass over X (``d0 <= MLP_FUSED_ROWS_MAX_IN``), in a fixed order;
* ``rows(X, y, w, coef, layers, want)`` -> a dict out of ``"loss"`` (``sum w (lse - z[y])``), ``"row_loss"`` (``[n]``,
  ``min(lse - z[y], -log(1e-300))``: the value of ``-log(max(P[y], 1e-300))`` without forming ``P[y]``; the two differ
  only by rounding, and the clamp binds in both at ``P[y] < 1e-300``), ``"P"`` (``[n, C]``) and ``"label"`` (``[n]``
  int32, the first maximum of the logits);
* ``fused_grad_torch`` / ``search_losses_torch`` / ``rows_torch``: the same results by torch formulas (CPU tensors
  take them);
* ``shape_ok`` / ``supported`` / ``selected``: the shape rule, the rule on a GPU, and the gate
  ``sized_gate("ALINK_MLP_HIP", device, n, MLP_MIN_ROWS)``.  ``grad=True`` asks for the gradient pass, which is
  narrower than the row pass.

The gradient pass has a tile budget: the tile counts of all layers, rounded as ``tile_counts`` says, add to at most
``MLP_FUSED_MAX_TILES = 40``.  The kernels with more (one hidden layer ``> 32`` with ``d0 > 64`` and ``C > 32``; two
hidden layers, one ``> 32``, with ``d0 > 64`` or with ``d0 > 32`` and ``C > 32``) spill to scratch and are not built:
``shape_ok(..., grad=True)`` is False for them and the GEMM path of ``ops/mlp.py`` keeps them.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from . import _lib

__all__ = ["MLP_FUSED_MAX_IN", "MLP_FUSED_ROWS_MAX_IN", "MLP_FUSED_MAX_HIDDEN", "MLP_FUSED_MAX_CLASSES",
           "MLP_FUSED_MAX_TILES", "MLP_FUSED_MAX_STEPS", "MLP_MIN_ROWS", "MLP_SCRATCH_BYTES", "tile_counts",
           "shape_ok", "supported", "selected", "mlp_chunk_rows", "weight_image", "weight_pack", "fused_grad",
           "fused_grad_torch", "search_losses", "search_losses_torch", "rows", "rows_torch"]

MLP_FUSED_MAX_IN = 128              # eight input tiles of 16: a row's dims stay in registers through the gradient pass
MLP_FUSED_ROWS_MAX_IN = 1024        # the row pass walks the dims in tiles of 16
MLP_FUSED_MAX_HIDDEN = 64           # four tiles
MLP_FUSED_MAX_CLASSES = 64
MLP_FUSED_MAX_TILES = 40            # Gram tiles of all layers (rounded counts): 10 accumulator tiles per wave, more spill
MLP_FUSED_MAX_STEPS = 8
MLP_MIN_ROWS = 4096                 # from here on gradient + search beat the former path at every swept shape (profiles/mlp_fused.txt)
MLP_SCRATCH_BYTES = 128 << 20       # cap of the chunk partials [nchunk, 1 + nw]
MLP_CHUNKS = 1024                   # row chunks of the gradient pass at most: the merge adds them one after another
MLP_CHUNK_MIN_ROWS = 256            # and no chunk shorter than this, so that a small n has few partials to merge
MLP_FUSED_CALLS = 0                 # launches of the fused MLP kernels (tests read it)
_WANT = {"loss": 1, "row_loss": 2, "P": 4, "label": 8}


def _round_tiles(d: int) -> int:
    t, r = (d + 15) // 16, 1
    while r < t:
        r *= 2
    return r


def tile_counts(layers: Sequence[int], grad: bool) -> Tuple[int, int, int]:
    """``(ti, th, to)``: the input, hidden and class tile counts of the kernels' images.  Hidden and class tiles are
    rounded up to 1, 2 or 4, both hidden layers to one common count; input tiles to 1, 2, 4 or 8 for the gradient
    pass and ``ceil(d0 / 16)`` for the row pass."""
    ti = _round_tiles(layers[0]) if grad else (layers[0] + 15) // 16
    th = max([_round_tiles(h) for h in layers[1:-1]], default=1)
    return ti, th, _round_tiles(layers[-1])


def _weight_size(layers) -> int:
    return sum(layers[i] * layers[i + 1] + layers[i + 1] for i in range(len(layers) - 1))


def shape_ok(X, layers: Sequence[int], grad: bool = True) -> bool:
    """The shape rule of the fused MLP kernels: a contiguous fp64 ``[n, d0]`` tensor with ``n < 2^31``, 1 to 3 affine
    layers, ``1 <= d0 <= MLP_FUSED_MAX_IN`` (``MLP_FUSED_ROWS_MAX_IN`` with ``grad=False``), hidden widths in ``1 ..
    MLP_FUSED_MAX_HIDDEN``, ``2 <= C <= MLP_FUSED_MAX_CLASSES``; for the gradient pass also at most
    ``MLP_FUSED_MAX_TILES`` Gram tiles (rounded counts)."""
    layers = [int(v) for v in layers]
    if not (isinstance(X, torch.Tensor) and X.dtype == torch.float64 and X.dim() == 2 and X.is_contiguous()
            and X.shape[0] < 2 ** 31 and 2 <= len(layers) <= 4 and X.shape[1] == layers[0]
            and 1 <= layers[0] <= (MLP_FUSED_MAX_IN if grad else MLP_FUSED_ROWS_MAX_IN)
            and all(1 <= h <= MLP_FUSED_MAX_HIDDEN for h in layers[1:-1])
            and 2 <= layers[-1] <= MLP_FUSED_MAX_CLASSES):
        return False
    if grad:
        ti, th, to = tile_counts(layers, True)
        nh = len(layers) - 2
        tiles = ti * to if nh == 0 else ti * th + (nh - 1) * th * th + th * to
        if tiles > MLP_FUSED_MAX_TILES:
            return False
    return True


def supported(X, layers: Sequence[int], grad: bool = True) -> bool:
    """Whether the fused MLP kernels take these rows: ``shape_ok`` rows on a GPU."""
    return shape_ok(X, layers, grad) and X.is_cuda


def selected(X, layers: Sequence[int], grad: bool = True) -> bool:
    """The selection rule: ``supported`` rows, from ``MLP_MIN_ROWS`` rows on (``ALINK_MLP_HIP=1``: always, ``=0``:
    never); then the project's fall-back rule."""
    return supported(X, layers, grad) and _lib.sized_gate("ALINK_MLP_HIP", X.device, X.shape[0], MLP_MIN_ROWS)


def mlp_chunk_rows(n: int, layers: Sequence[int]) -> int:
    """Rows per chunk of the gradient pass, from (n, layers) alone: ``_lib.chunk_rows`` under this op's constants."""
    return _lib.chunk_rows(n, 1 + _weight_size(layers), MLP_SCRATCH_BYTES, MLP_CHUNKS, MLP_CHUNK_MIN_ROWS)


def _unpack(coefs: torch.Tensor, layers):
    """coefs [S, nw] -> per layer (W [S, in, out], b [S, out])."""
    out, off = [], 0
    for i in range(len(layers) - 1):
        a, b = layers[i], layers[i + 1]
        out.append((coefs[:, off:off + a * b].reshape(-1, a, b), coefs[:, off + a * b:off + a * b + b]))
        off += a * b + b
    return out


def _logits(X, coef, layers):
    h = X
    params = _unpack(coef[None, :], layers)
    for W, b in params[:-1]:
        h = 1.0 / (1.0 + torch.exp(-(h @ W[0] + b[0])))
    return h @ params[-1][0][0] + params[-1][1][0]


def fused_grad_torch(X, y, w, coef, layers) -> Tuple[torch.Tensor, torch.Tensor]:
    """``fused_grad`` by torch formulas: the explicit backward pass of ``ops/mlp.py`` without its kernels."""
    from .softmax import softmax_full_grad_torch
    params = _unpack(coef[None, :], layers)
    hs = [X]
    for W, b in params[:-1]:
        hs.append(1.0 / (1.0 + torch.exp(-(hs[-1] @ W[0] + b[0]))))
    D, loss = softmax_full_grad_torch(hs[-1] @ params[-1][0][0] + params[-1][1][0], y, w)
    grads = [None] * len(params)
    for i in range(len(params) - 1, -1, -1):
        grads[i] = torch.cat([(hs[i].T @ D).reshape(-1), D.sum(0)])
        if i > 0:
            D = (D @ params[i][0][0].T) * (hs[i] * (1.0 - hs[i]))
    return torch.cat(grads), loss


def search_losses_torch(X, y, w, coef, dirv, layers, beta: float, nsteps: int) -> torch.Tensor:
    """``search_losses`` by torch formulas, one forward pass per step."""
    return torch.stack([rows_torch(X, y, w, coef - dirv * (s * beta), layers, ("loss",))["loss"]
                        for s in range(nsteps)])


def rows_torch(X, y, w, coef, layers, want: Sequence[str]) -> Dict[str, torch.Tensor]:
    """``rows`` by torch formulas."""
    z = _logits(X, coef, layers)
    lse = torch.logsumexp(z, 1)
    zy = z.gather(1, y.long()[:, None])[:, 0]
    P = torch.softmax(z, 1)
    res = {"loss": ((lse - zy) * w).sum(),
           "row_loss": -torch.log(P.gather(1, y.long()[:, None])[:, 0].clamp_min(1e-300)),
           "P": P, "label": z.argmax(1).to(torch.int32)}
    return {key: val for key, val in res.items() if key in want}


def weight_image(M: torch.Tensor, kt: int, nt: int) -> torch.Tensor:
    """``M [S, K, N]`` zero-padded to ``kt x nt`` tiles of 16 and written in the order the lanes read it:
    ``img [S][tn][tk][g = 4][mm = 16][s = 4]``, element ``= M[16 tk + 4 g + s, 16 tn + mm]``."""
    S, K, N = M.shape
    pad = torch.zeros((S, 16 * kt, 16 * nt), dtype=torch.float64, device=M.device)
    pad[:, :K, :N] = M
    return pad.view(S, kt, 4, 4, nt, 16).permute(0, 4, 1, 2, 5, 3).contiguous()


def weight_pack(coefs: torch.Tensor, layers: Sequence[int], grad: bool) -> torch.Tensor:
    """The kernels' weight pack ``[S, size]`` of the weight sets ``coefs [S, nw]``: per layer the forward image
    ``weight_image(W, in tiles, out tiles)``, the bias zero-padded to whole tiles and, for the gradient pass and every
    layer but the first, the backward image ``weight_image(W^T, out tiles, in tiles)`` (element ``= W[16 tn + mm,
    16 tk + 4 g + s]``).  Tile counts as ``tile_counts(layers, grad)``."""
    ti, th, to = tile_counts(layers, grad)
    S, nl = coefs.shape[0], len(layers) - 1
    pieces = []
    for l, (W, b) in enumerate(_unpack(coefs, layers)):
        kt, nt = (ti if l == 0 else th), (to if l == nl - 1 else th)
        bias = torch.zeros((S, 16 * nt), dtype=torch.float64, device=coefs.device)
        bias[:, :b.shape[1]] = b
        pieces += [weight_image(W, kt, nt).reshape(S, -1), bias]
        if grad and l > 0:
            pieces.append(weight_image(W.transpose(1, 2), nt, kt).reshape(S, -1))
    return torch.cat(pieces, 1).contiguous()


def _check(X, y, w, vecs, layers, grad):
    layers = [int(v) for v in layers]
    if not supported(X, layers, grad):
        raise ValueError("the fused MLP kernels need contiguous fp64 [n, d0] GPU rows and layers inside shape_ok "
                         f"(d0 <= {MLP_FUSED_MAX_IN if grad else MLP_FUSED_ROWS_MAX_IN}, hidden <= "
                         f"{MLP_FUSED_MAX_HIDDEN}, 2 <= C <= {MLP_FUSED_MAX_CLASSES}, at most 3 affine layers)")
    for t in (y, w):
        if not (t.dtype == torch.float64 and t.is_contiguous() and t.shape == (X.shape[0],) and t.device == X.device):
            raise ValueError("y and w must be contiguous fp64 [n] tensors on the rows' device")
    for t in vecs:
        if not (t.dtype == torch.float64 and t.shape == (_weight_size(layers),) and t.device == X.device):
            raise ValueError("coef and dirv must be fp64 [weight_size(layers)] tensors on the rows' device")
    _lib.require()
    return layers, layers[1:] + [0] * (4 - len(layers))


def fused_grad(X, y, w, coef, layers, grid: int = 0, chunk_rows: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """One gradient pass: ``(gradient [nw] in the coef layout, sum w loss (0-dim))``.  On the GPU the same bits for
    every launch and every ``grid`` (``chunk_rows``, a multiple of 64, overrides the chunk length, which otherwise
    follows from (n, layers) alone).  CPU tensors take ``fused_grad_torch``; GPU rows outside ``supported`` are an
    error (ask ``selected`` first)."""
    global MLP_FUSED_CALLS
    if not X.is_cuda:
        return fused_grad_torch(X, y, w, coef, layers)
    layers, rest = _check(X, y, w, (coef,), layers, True)
    n, dev, nw = X.shape[0], X.device, coef.shape[0]
    if n == 0:          # nothing is launched for an empty partition
        return torch.zeros(nw, dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    crows = int(chunk_rows) if chunk_rows > 0 else mlp_chunk_rows(n, layers)
    nchunk, part, out = _lib.chunk_buffers(n, crows, 1 + nw, dev)
    pack = weight_pack(coef[None, :], layers, True)
    _lib.call("alink_mlp_fused_grad_f64", X.data_ptr(), y.data_ptr(), w.data_ptr(), n, len(layers) - 1, layers[0],
              *rest, pack.data_ptr(), crows, nchunk, part.data_ptr(), out.data_ptr(), int(grid), _lib.stream_ptr(dev))
    MLP_FUSED_CALLS += 1
    return out[1:], out[0]


def _rows_call(X, y, w, coefs, layers, mask, grid):
    global MLP_FUSED_CALLS
    n, dev, S = X.shape[0], X.device, coefs.shape[0]
    C = layers[-1]
    sums = torch.zeros(S, dtype=torch.float64, device=dev) if mask & 1 else None
    row_loss = torch.empty(n, dtype=torch.float64, device=dev) if mask & 2 else None
    P = torch.empty((n, C), dtype=torch.float64, device=dev) if mask & 4 else None
    label = torch.empty(n, dtype=torch.int32, device=dev) if mask & 8 else None
    if n > 0:
        pack = weight_pack(coefs, layers, False)
        part = torch.empty((S, (n + 63) // 64), dtype=torch.float64, device=dev) if mask & 1 else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        _lib.call("alink_mlp_fused_rows_f64", X.data_ptr(), y.data_ptr(), w.data_ptr(), n, len(layers) - 1, layers[0],
                  *(layers[1:] + [0] * (4 - len(layers))), pack.data_ptr(), S, int(mask), ptr(part), ptr(sums),
                  ptr(row_loss), ptr(P), ptr(label), int(grid), _lib.stream_ptr(dev))
        MLP_FUSED_CALLS += 1
    return sums, row_loss, P, label


def search_losses(X, y, w, coef, dirv, layers, beta: float, nsteps: int, grid: int = 0) -> torch.Tensor:
    """The weighted losses ``sum_i w_i loss_i(coef - s beta dirv)``, ``s = 0 .. nsteps - 1`` (``nsteps <=
    MLP_FUSED_MAX_STEPS``), from one pass over X; independent of ``grid``.  CPU tensors take
    ``search_losses_torch``."""
    if not X.is_cuda:
        return search_losses_torch(X, y, w, coef, dirv, layers, beta, nsteps)
    if not 1 <= nsteps <= MLP_FUSED_MAX_STEPS:
        raise ValueError(f"nsteps must lie in 1 .. {MLP_FUSED_MAX_STEPS}")
    layers, _ = _check(X, y, w, (coef, dirv), layers, False)
    steps = torch.arange(nsteps, dtype=torch.float64, device=X.device) * beta
    return _rows_call(X, y, w, coef[None, :] - dirv[None, :] * steps[:, None], layers, 1, grid)[0]


def rows(X, y, w, coef, layers, want: Sequence[str], grid: int = 0) -> Dict[str, torch.Tensor]:
    """The forward row pass at ``coef``: ``"loss"`` -> ``sum w loss`` (0-dim), ``"row_loss"`` -> ``[n]``, ``"P"`` ->
    ``[n, C]``, ``"label"`` -> ``[n]`` int32.  CPU tensors take ``rows_torch``."""
    mask = sum(_WANT[key] for key in _WANT if key in want)
    if not mask or set(want) - set(_WANT):
        raise ValueError(f"want must name some of {tuple(_WANT)}")
    if not X.is_cuda:
        return rows_torch(X, y, w, coef, layers, want)
    layers, _ = _check(X, y, w, (coef,), layers, False)
    sums, row_loss, P, label = _rows_call(X, y, w, coef[None, :], layers, mask, grid)
    res = {"loss": sums[0] if sums is not None else None, "row_loss": row_loss, "P": P, "label": label}
    return {key: val for key, val in res.items() if key in want}
