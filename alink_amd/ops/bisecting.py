"""Bisecting k-means on the device: the tree table and the descent kernels (``csrc/bisecting.hip``).

The one operation bisecting k-means has and KMeans does not: every row is compared with the split plane of its own
tree node.  Nodes are slots ``0 .. S-1`` of a small table built on the host, shared by training and prediction:

* ``left`` / ``right`` int32 ``[S]``: the children's slots, ``-1`` for "do not descend here" (a leaf, or in training a
  node that is not dividing).  The slots that descend come first, ``0 .. P-1``, and hold a plane;
* EUCLIDEAN: ``V [P, d] = r - l`` and ``thr [P] = (r + l)/2 . (r - l)``; a row goes left iff ``x . V[s] < thr[s]``;
* COSINE: ``A [P, d] = l/|l|``, ``B [P, d] = r/|r|``; left iff ``(1 - x . A[s]) < (1 - x . B[s])`` on rows the caller
  normalised.  Equality and any NaN go right.

``tree_table(centers, nodes, cosine, device)`` builds it; ``descend_f64`` / ``descend_csr`` launch the kernels on
fp64 rows ``[n, d]`` (``1 <= d <= 1024``) / CSR rows, moving an int32 ``slot [n]`` in place up to ``levels`` levels
(1: a training iteration; the tree depth: prediction).  A row's side depends on ``d`` and the row alone, never on
the launch or its ``grid``.  Which rows take these kernels is decided in ``ops/kmeans_rows.py`` (``Rows.descend``,
``Rows.child_stats``); the torch arithmetic of the other kinds lives there too.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from . import _lib, csr

__all__ = ["TreeTable", "tree_table", "descend_f64", "descend_csr", "BISECT_CALLS"]

BISECT_CALLS = 0        # launches of the HIP descent kernels (tests read it)


class TreeTable:
    """The tree of one descent: ``nodes`` (slot -> node id), ``slot_of`` (node id -> slot), ``S`` slots of which the
    first ``P`` descend, ``depth`` (the longest descent), the host arrays ``left_h`` / ``right_h`` and the raw child
    centres ``lc`` / ``rc`` ``[P, d]`` (the torch kinds compute from these, as the host code always did), and on
    ``device``: ``left``, ``right``, and ``V`` + ``thr`` (EUCLIDEAN) or ``A`` + ``B`` (COSINE)."""
    __slots__ = ("nodes", "slot_of", "S", "P", "d", "cosine", "depth", "device", "left_h", "right_h", "lc", "rc",
                 "left", "right", "V", "thr", "A", "B")


def tree_table(centers: Dict[int, np.ndarray], nodes: Sequence[int], cosine: bool, device) -> TreeTable:
    """The table of the tree nodes ``nodes`` (ids: root 1, children ``2 i`` and ``2 i + 1``) with the centres
    ``centers``.  A node descends iff both its children are in ``nodes``; the descending nodes take the first slots
    (in the order given), the others follow (in the order given)."""
    nodes = [int(c) for c in nodes]
    have = set(nodes)
    desc = [c for c in nodes if 2 * c in have and 2 * c + 1 in have]
    dset = set(desc)
    t = TreeTable()
    t.nodes = desc + [c for c in nodes if c not in dset]
    t.slot_of = {c: i for i, c in enumerate(t.nodes)}
    t.S, t.P, t.cosine, t.device = len(t.nodes), len(desc), bool(cosine), torch.device(device)
    t.d = int(next(iter(centers.values())).shape[0]) if centers else 0
    t.left_h = np.full(t.S, -1, dtype=np.int32)
    t.right_h = np.full(t.S, -1, dtype=np.int32)
    t.lc = np.zeros((t.P, t.d))
    t.rc = np.zeros((t.P, t.d))
    p0 = np.zeros((t.P, t.d))
    p1 = np.zeros((t.P, t.d)) if cosine else np.zeros(t.P)
    for s, c in enumerate(desc):
        t.left_h[s], t.right_h[s] = t.slot_of[2 * c], t.slot_of[2 * c + 1]
        l, r = np.asarray(centers[2 * c], dtype=np.float64), np.asarray(centers[2 * c + 1], dtype=np.float64)
        t.lc[s], t.rc[s] = l, r
        if cosine:
            p0[s], p1[s] = l / np.sqrt(l @ l), r / np.sqrt(r @ r)
        else:
            v, m = r - l, 0.5 * (r + l)
            p0[s], p1[s] = v, m @ v
    level = {}

    def depth_of(s):
        if s not in level:
            level[s] = 0 if t.left_h[s] < 0 else 1 + max(depth_of(int(t.left_h[s])), depth_of(int(t.right_h[s])))
        return level[s]
    t.depth = max((depth_of(s) for s in range(t.S)), default=0)
    dev = t.device
    t.left, t.right = torch.from_numpy(t.left_h).to(dev), torch.from_numpy(t.right_h).to(dev)
    t.device = t.left.device                # with its index, as the rows' tensors report it
    t.V = t.thr = t.A = t.B = None
    if cosine:
        t.A, t.B = torch.from_numpy(p0).to(dev), torch.from_numpy(p1).to(dev)
    else:
        t.V, t.thr = torch.from_numpy(p0).to(dev), torch.from_numpy(p1).to(dev)
    return t


def _check(table: TreeTable, slot: torch.Tensor, n: int, d: int, dev) -> None:
    if slot.dtype != torch.int32 or slot.dim() != 1 or int(slot.shape[0]) != n or not slot.is_contiguous() \
            or slot.device != dev:
        raise ValueError("slot must be a contiguous int32 [n] tensor on the rows' device")
    if table.d != d or table.device != dev:
        raise ValueError("the tree table is for another vector size or device")


def _launch(name: str, table: TreeTable, head: List, slot: torch.Tensor, levels: int, grid: int, dev) -> None:
    global BISECT_CALLS
    p0, p1, thr = (table.A, table.B, None) if table.cosine else (table.V, None, table.thr)
    _lib.call(name, *head, slot.data_ptr(), table.S, table.left.data_ptr(), table.right.data_ptr(), p0.data_ptr(),
              p1.data_ptr() if p1 is not None else None, thr.data_ptr() if thr is not None else None,
              int(table.cosine), int(levels), int(grid), _lib.stream_ptr(dev))
    BISECT_CALLS += 1


def descend_f64(X: torch.Tensor, table: TreeTable, slot: torch.Tensor, levels: int, grid: int = 0) -> torch.Tensor:
    """Move ``slot`` (int32 [n], in place) up to ``levels`` levels down ``table`` for the contiguous fp64 GPU rows
    ``X`` [n, d], 1 <= d <= 1024.  Slots outside ``[0, S)`` and slots that do not descend stay, their rows unread."""
    n, d = X.shape
    if not (X.is_cuda and X.dtype == torch.float64 and X.is_contiguous() and 1 <= d <= 1024 and n < 2 ** 31):
        raise ValueError("the dense descent needs contiguous fp64 [n, d] GPU rows with 1 <= d <= 1024, n < 2^31")
    _check(table, slot, n, d, X.device)
    if n == 0 or levels <= 0 or table.P == 0:       # nothing to launch
        return slot
    _launch("alink_bisect_descend_f64", table, [X.data_ptr(), n, d], slot, levels, grid, X.device)
    return slot


def descend_csr(fm, table: TreeTable, slot: torch.Tensor, levels: int, grid: int = 0) -> torch.Tensor:
    """The same for the CSR rows of a sparse fp64 ``FeatureMatrix`` on a GPU, which are never densified; entries
    whose column is outside ``[0, d)`` are ignored."""
    n, d = fm.nrows, int(fm.ncols)
    if not (fm.val.is_cuda and fm.val.dtype == torch.float64 and fm.col.dtype in (torch.int32, torch.int64)
            and d >= 1 and n < 2 ** 31):
        raise ValueError("the CSR descent needs fp64 values and int32/int64 columns on a GPU, n < 2^31")
    _check(table, slot, n, d, fm.val.device)
    if n == 0 or levels <= 0 or table.P == 0:
        return slot
    alive, head = csr.row_args(fm, d)      # alive: the arrays behind head's pointers
    _launch("alink_bisect_descend_csr", table, head, slot, levels, grid, fm.val.device)
    return slot
