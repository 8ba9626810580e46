"""Running top-K of query·item scores over item blocks.

``TopKState(m, K)`` holds the per-query best scores / item ids; ``merge(state, Q, T, item_base)`` folds the
item block ``T`` (global ids ``item_base + row``) into it; ``finish(state)`` returns rows sorted best first
(reference ``BlockwiseCross.findTopK`` pops its PriorityQueue into descending arrays,
``A/operator/common/dataproc/BlockwiseCross.java:221-236``).

Order: inputs are finite, and entry ``(s, id)`` ranks before ``(s', id')`` iff ``s > s'``, or ``s == s'`` and
``id < id'``.  For each query the result is the first ``min(K, N)`` of all ``(score, global id)`` pairs in that
order, returned in that order; the remaining slots are ``(-inf, -1)``.  It depends only on the queries, the
union of the items with their global ids and ``K``: not on how the items are split into blocks, the order in
which the blocks are merged, the number of slices or the number of ranks.  Ascending order is the same rule on
``-Q``.  NaN and infinite scores are out of scope.

GPU: ``alink_topk_cross_f32`` (``csrc/topk.hip``) — f32 MFMA scores against LDS-staged item chunks with the
top-K held in LDS; the score matrix never reaches HBM.  CPU (or rank > 64 / K > 128): chunked GEMM, the block's
first K by the same order, then one two-key selection over [state | block candidates].
"""
from __future__ import annotations

import torch

from . import _lib

__all__ = ["TopKState", "merge", "finish", "kernel_supported", "pad_rank"]

KMAX = 128
QB = 128            # queries per workgroup (csrc/topk.hip)
WANT_WG = 512       # 2 workgroups per CU on 256 CUs
NEG = float("-inf")


def pad_rank(r: int) -> int:
    return max(16, (r + 15) // 16 * 16)


def kernel_supported(Q: torch.Tensor, K: int) -> bool:
    return Q.is_cuda and pad_rank(Q.shape[1]) <= 64 and 1 <= K <= KMAX and _lib.kernels_enabled()


class TopKState:
    def __init__(self, m: int, K: int, device):
        self.K = int(K)
        self.val = torch.full((m, self.K), NEG, dtype=torch.float32, device=device)
        self.idx = torch.full((m, self.K), -1, dtype=torch.int32, device=device)


def _pad(x: torch.Tensor, R: int) -> torch.Tensor:
    x = x.to(torch.float32)
    if x.shape[1] == R and x.is_contiguous():
        return x
    out = torch.zeros((x.shape[0], R), dtype=torch.float32, device=x.device)
    out[:, :x.shape[1]] = x
    return out


def _first(val: torch.Tensor, idx: torch.Tensor, K: int):
    """The first ``K`` entries of every row of ``(val, idx)`` [m, w] by (score descending, id ascending), in that
    order: a stable sort by id, then a stable sort by score, so nothing rests on a library's tie order."""
    by_id = torch.sort(idx, dim=1, stable=True).indices
    by_val = torch.sort(torch.gather(val, 1, by_id), dim=1, descending=True, stable=True).indices[:, :K]
    order = torch.gather(by_id, 1, by_val)
    return torch.gather(val, 1, order), torch.gather(idx, 1, order)


def _block_first(sc: torch.Tensor, kk: int):
    """``(values, columns)`` [rows, kk] of the first ``kk`` entries of every row of the score block ``sc`` by
    (score descending, column ascending), as a set: the order inside a row is left to ``_first``.  Where no more
    than ``kk`` entries reach a row's kk-th value ``t`` the set is unique and ``torch.topk``'s is it; the other
    rows keep their entries above ``t`` and the first of those equal to ``t``, whichever ones ``torch.topk`` took."""
    v, cols = torch.topk(sc, kk, dim=1)
    t = v[:, -1:]
    tied = ((sc >= t).sum(1) > kk).nonzero().flatten()
    if tied.numel():
        sub, t = sc[tied], t[tied]
        above, equal = sub > t, sub == t
        room = kk - above.sum(1, keepdim=True, dtype=torch.int32)
        keep = above | (equal & (torch.cumsum(equal, 1, dtype=torch.int32) <= room))
        sub_cols = keep.nonzero()[:, 1].reshape(sub.shape[0], kk)       # row-major: kk per row
        v[tied], cols[tied] = torch.gather(sub, 1, sub_cols), sub_cols
    return v, cols


def merge(state: TopKState, Q: torch.Tensor, T: torch.Tensor, item_base: int = 0,
          use_kernel: bool = None) -> TopKState:
    """Fold item block ``T`` [n, r] (global ids ``item_base + row``) into the top-K of queries ``Q`` [m, r].

    The state afterwards holds the first K of (state entries ∪ block entries) in the module's order, whatever
    the order of the calls; scores are finite (NaN and ±inf are out of scope)."""
    m, n = Q.shape[0], T.shape[0]
    if m == 0 or n == 0:
        return state
    if use_kernel is None:
        use_kernel = kernel_supported(Q, state.K)
    if use_kernel:
        R = pad_rank(Q.shape[1])
        Qp, Tp = _pad(Q, R), _pad(T.to(Q.device), R)
        # split the items too when the query blocks alone cannot fill the chip (>= 2 workgroups per CU)
        qblocks = (m + QB - 1) // QB
        slices = max(1, min(WANT_WG // qblocks, (n + 4095) // 4096))
        per = ((n + slices - 1) // slices + 63) // 64 * 64
        slices = (n + per - 1) // per
        if slices == 1:
            val, idx = state.val, state.idx
        else:
            val = torch.full((slices, m, state.K), NEG, dtype=torch.float32, device=Q.device)
            idx = torch.full((slices, m, state.K), -1, dtype=torch.int32, device=Q.device)
            val[0].copy_(state.val)
            idx[0].copy_(state.idx)
        _lib.call("alink_topk_cross_f32", Qp.data_ptr(), m, Tp.data_ptr(), n, int(item_base), R, state.K,
                  val.data_ptr(), idx.data_ptr(), slices, per, _lib.stream_ptr(Q.device))
        if slices > 1:
            # by id, not by plane: plane 0 also carries the prior state, whose ids may lie above every plane's
            state.val, state.idx = _first(val.permute(1, 0, 2).reshape(m, slices * state.K),
                                          idx.permute(1, 0, 2).reshape(m, slices * state.K), state.K)
        return state
    Qf = Q.to(torch.float32)
    Tf = T.to(device=Q.device, dtype=torch.float32)
    chunk = max(1, (1 << 26) // max(1, n))
    kk = min(state.K, n)
    for s in range(0, m, chunk):
        v, i = _block_first(Qf[s:s + chunk] @ Tf.T, kk)
        state.val[s:s + chunk], state.idx[s:s + chunk] = _first(
            torch.cat([state.val[s:s + chunk], v], 1),
            torch.cat([state.idx[s:s + chunk], (i + item_base).to(torch.int32)], 1), state.K)
    return state


def finish(state: TopKState):
    """(values, ids) [m, K] in the module's order (score descending, equal scores by ascending id); unfilled
    slots (fewer than K items) are (-inf, -1) at the end."""
    return _first(state.val, state.idx, state.K)
