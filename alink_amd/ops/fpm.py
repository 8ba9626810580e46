"""Frequent-itemset mining on the device: support counts on vertical bitmaps (``csrc/fpm.hip``) and the level-wise
candidate generation around them in torch.

Bit ``t`` of row ``i`` of ``B`` (int64 storage of uint64 words, ``[m, W]``, ``W = row_stride(n)`` even so rows are
16-byte aligned) says that transaction ``t`` holds frequent item ``i``; the support of an itemset is the popcount of
the AND of its rows.  The set of frequent itemsets is defined by the data and the threshold, not by the miner, so
``mine`` returns exactly the patterns of the host path ``models/associationrule/mining.fp_growth`` (the CPU path and
the oracle).  Counts are integers: every result is the same for every grid, chunk size and split into row blocks.

Three kernels, each with a torch twin of the same arguments that runs on any device (``*_twin``): ``build_bitmap``,
``pair_counts`` (level 2: the upper triangle of the bit Gram, a tiled product through LDS) and ``class_counts``
(levels >= 3, and level 2 above ``FPM_PAIR_MAX_ITEMS``: candidates grouped by prefix).  ``mine`` takes the three as
a ``Backend``, so the CPU tests drive the same level loop through the twins (``TWIN``) that the operator drives
through the kernels (``DEVICE``).  The batch loop of a level (``count_level``), the pattern columns
(``pattern_columns``) and the grouped-candidate check are shared with the sequence miner ``ops/prefixspan.py``.

``device_selected(device, n_rows)`` decides whether ``FpGrowthBatchOp`` takes this path: a CUDA device,
``ALINK_FPGROWTH_HIP`` not ``0``, at least ``FPM_MIN_ROWS`` rows (``ALINK_FPGROWTH_HIP=1`` forces it at any size) and
``_lib.kernels_enabled()`` (no quiet fall-back).
"""
from __future__ import annotations

import time
from typing import Callable, List, NamedTuple, Optional, Tuple

import torch

from ..parallel import comm
from . import _lib

__all__ = ["device_selected", "row_stride", "build_bitmap", "pair_counts", "class_counts", "build_bitmap_twin",
           "pair_counts_twin", "class_counts_twin", "u32", "Backend", "DEVICE", "TWIN", "join_siblings",
           "count_level", "pattern_columns", "mine", "FPM_CALLS", "FPM_MIN_ROWS", "FPM_PAIR_MAX_ITEMS", "FPM_BUDGET_BYTES"]

FPM_CALLS = 0                   # launches of the HIP mining kernels (tests read it)
FPM_MIN_ROWS = 512              # rows (over all ranks) from which the device path is taken: the measured crossover
#                                 against the host path, between 300 rows (host 5.2 ms, device 6.5 ms) and 1000 rows
#                                 (12.3 ms, 5.9 ms); profiles/fpgrowth.txt records the run
FPM_PAIR_MAX_ITEMS = 16384      # above this many frequent items level 2 goes through the class kernel: C uint32
#                                 [m, m] stays at 1 GiB
FPM_BUDGET_BYTES = 2 ** 31      # bytes one row block's bitmap, and one batch of candidates, may take
_CAND_BYTES = 32                # per candidate of a batch: extension, owner, position, count and the kept rows (the
#                                 level loops of this module and of ``ops/prefixspan.py``)


def device_selected(device, n_rows: int) -> bool:
    """True when ``FpGrowthBatchOp`` runs on the device: a CUDA device, not switched off by ``ALINK_FPGROWTH_HIP=0``,
    ``n_rows >= FPM_MIN_ROWS`` unless ``ALINK_FPGROWTH_HIP=1`` forces it, and the kernel library by the one
    fall-back rule (``_lib.kernels_enabled``: a missing library is an error)."""
    return _lib.sized_gate("ALINK_FPGROWTH_HIP", device, n_rows, FPM_MIN_ROWS)


def row_stride(n: int) -> int:
    """64-bit words of a bitmap row for ``n`` transactions: even (rows 16-byte aligned), at least 2."""
    return max(2, ((int(n) + 63) // 64 + 1) // 2 * 2)


def u32(C: torch.Tensor) -> torch.Tensor:
    """The uint32 counts of ``pair_counts`` (int32 storage) as int64."""
    return C.to(torch.int64) & 0xFFFFFFFF


def _ran() -> None:
    global FPM_CALLS
    FPM_CALLS += 1


# ---------------------------------------------------------------------------------------------------
# checks shared by the kernels' wrappers and the twins
# ---------------------------------------------------------------------------------------------------
def _check_csr(crow: torch.Tensor, item: torch.Tensor, m: int) -> int:
    if not (crow.dtype == torch.int64 and item.dtype == torch.int32 and crow.dim() == 1 and item.dim() == 1
            and crow.numel() >= 1 and crow.device == item.device and crow.is_contiguous() and item.is_contiguous()):
        raise ValueError("build_bitmap: crow int64 [n + 1] and item int32 [nnz], contiguous on one device, are needed")
    if int(m) < 1 or int(m) >= 2 ** 31:
        raise ValueError("build_bitmap: 1 <= m < 2^31 frequent items are needed")
    n = int(crow.numel()) - 1
    if int(crow[0]) != 0 or int(crow[-1]) != int(item.numel()) or (n and bool((crow[1:] < crow[:-1]).any())):
        raise ValueError("build_bitmap: crow must ascend from 0 to nnz")
    return n


def _check_bitmap(B: torch.Tensor, what: str) -> Tuple[int, int]:
    if not (B.dtype == torch.int64 and B.dim() == 2 and B.is_contiguous() and B.shape[0] >= 1
            and B.shape[1] >= 2 and B.shape[1] % 2 == 0):
        raise ValueError(f"{what}: a contiguous int64 [m, W] bitmap with W even is needed")
    return int(B.shape[0]), int(B.shape[1])


def _check_grouped(what: str, B, prefix, cls_ptr, ext, n_codes: int) -> Tuple[int, int, int]:
    """The candidates of a walk, grouped by parent: ``(classes, candidates, P)``.  ``n_codes``: the codes a row of
    ``prefix`` and ``ext`` may hold are ``[0, n_codes)``."""
    dev = B.device
    if not (prefix.dtype == torch.int32 and prefix.dim() == 2 and prefix.shape[1] >= 1 and prefix.is_contiguous()
            and cls_ptr.dtype == torch.int64 and cls_ptr.dim() == 1 and cls_ptr.is_contiguous()
            and ext.dtype == torch.int32 and ext.dim() == 1 and ext.is_contiguous()
            and prefix.device == dev and cls_ptr.device == dev and ext.device == dev
            and int(cls_ptr.numel()) == int(prefix.shape[0]) + 1):
        raise ValueError(f"{what}: prefix int32 [classes, P], cls_ptr int64 [classes + 1] and ext int32 [candidates], "
                         "contiguous on the bitmap's device, are needed")
    nc, ne = int(prefix.shape[0]), int(ext.numel())
    if int(cls_ptr[0]) != 0 or int(cls_ptr[-1]) != ne or (nc and bool((cls_ptr[1:] < cls_ptr[:-1]).any())):
        raise ValueError(f"{what}: cls_ptr must ascend from 0 to the number of candidates")
    for t in (prefix, ext):
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n_codes):
            raise ValueError(f"{what}: an item outside the bitmap's rows")
    return nc, ne, int(prefix.shape[1])


def _check_classes(B, prefix, cls_ptr, ext_item) -> Tuple[int, int, int]:
    m, _ = _check_bitmap(B, "class_counts")
    return _check_grouped("class_counts", B, prefix, cls_ptr, ext_item, m)


def _owner(cnt: torch.Tensor, total: int) -> torch.Tensor:
    """int64 [total]: the group of every member, for groups of ``cnt`` members back to back."""
    return torch.repeat_interleave(torch.arange(int(cnt.numel()), device=cnt.device), cnt, output_size=total)


# ---------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------
def build_bitmap(crow: torch.Tensor, item: torch.Tensor, m: int, grid: int = 0) -> torch.Tensor:
    """int64 [m, row_stride(n)] bitmap of CSR transactions on a GPU (item ranks in ``[0, m)``, unique within a row).
    Padding bits and words are zero."""
    n = _check_csr(crow, item, m)
    if not crow.is_cuda:
        raise ValueError("build_bitmap: tensors on a GPU are needed")
    dev = crow.device
    W = row_stride(n)
    B = torch.zeros((int(m), W), dtype=torch.int64, device=dev)
    if n == 0 or item.numel() == 0:
        return B
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("alink_fpm_bitmap", crow.data_ptr(), item.data_ptr(), n, int(m), W, B.data_ptr(), bad.data_ptr(),
              int(grid), _lib.stream_ptr(dev))
    _ran()
    if int(bad):
        raise ValueError("build_bitmap: an item outside [0, m)")
    return B


def pair_counts(B: torch.Tensor, chunk: int = 0, splits: int = 0) -> torch.Tensor:
    """``C[i][j] = popcount(B_i & B_j)`` for ``i < j`` (zero elsewhere) of a GPU bitmap: uint32 counts in int32
    storage ``[m, m]`` (``u32`` widens them).  ``chunk``: words staged per step, 16 or 32; ``splits``: workgroups
    that share the words of one 64 x 64 block (0: chosen from the shape).  Neither changes a count."""
    m, W = _check_bitmap(B, "pair_counts")
    if not B.is_cuda or m > 2 ** 16 or int(chunk) not in (0, 16, 32) or int(splits) < 0:
        raise ValueError("pair_counts: a GPU bitmap of at most 2^16 items, chunk 16 or 32 and splits >= 0 are needed")
    C = torch.zeros((m, m), dtype=torch.int32, device=B.device)
    if m < 2:
        return C
    _lib.call("alink_fpm_pair_counts", B.data_ptr(), m, W, C.data_ptr(), int(chunk), int(splits),
              _lib.stream_ptr(B.device))
    _ran()
    return C


def class_counts(B: torch.Tensor, prefix: torch.Tensor, cls_ptr: torch.Tensor, ext_item: torch.Tensor,
                 chunk: int = 0, grid: int = 0) -> torch.Tensor:
    """int64 [candidates] supports of candidates grouped by prefix on a GPU: candidate ``e`` of class ``c``
    (``cls_ptr[c] <= e < cls_ptr[c + 1]``) is the itemset ``prefix[c] + (ext_item[e],)``.  ``chunk``: words a wave
    owns per unit (rounded up to 128; 0: chosen from the shape); ``grid``: workgroups.  Neither changes a count."""
    nc, ne, P = _check_classes(B, prefix, cls_ptr, ext_item)
    if not B.is_cuda or int(chunk) < 0 or int(grid) < 0:
        raise ValueError("class_counts: a GPU bitmap, chunk >= 0 and grid >= 0 are needed")
    counts = torch.zeros(ne, dtype=torch.int64, device=B.device)
    if ne == 0:
        return counts
    _lib.call("alink_fpm_class_counts", B.data_ptr(), int(B.shape[1]), prefix.data_ptr(), P, cls_ptr.data_ptr(),
              ext_item.data_ptr(), nc, counts.data_ptr(), int(chunk), int(grid), _lib.stream_ptr(B.device))
    _ran()
    return counts


# ---------------------------------------------------------------------------------------------------
# torch twins: the same arguments and results on any device (the CPU path of the tests)
# ---------------------------------------------------------------------------------------------------
_POP8 = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64)


def _popcount_rows(x: torch.Tensor) -> torch.Tensor:
    """Sum over the last axis of the popcounts of int64 words, through a byte table."""
    b = x.contiguous().view(torch.uint8).reshape(*x.shape[:-1], -1)
    return _POP8.to(x.device)[b.to(torch.int64)].sum(-1)


def build_bitmap_twin(crow: torch.Tensor, item: torch.Tensor, m: int, grid: int = 0) -> torch.Tensor:
    n = _check_csr(crow, item, m)
    dev = crow.device
    W = row_stride(n)
    B = torch.zeros((int(m), W), dtype=torch.int64, device=dev)
    if n == 0 or item.numel() == 0:
        return B
    if int(item.min()) < 0 or int(item.max()) >= int(m):
        raise ValueError("build_bitmap: an item outside [0, m)")
    t = torch.repeat_interleave(torch.arange(n, device=dev), crow[1:] - crow[:-1], output_size=int(item.numel()))
    # distinct (item, transaction) pairs set distinct bits, so their two's-complement sum is their OR
    key = torch.unique(item.to(torch.int64) * n + t)
    it, t = torch.div(key, n, rounding_mode="floor"), key % n
    bit = torch.ones((), dtype=torch.int64, device=dev) << (t & 63)
    B.view(-1).index_add_(0, it * W + (t >> 6), bit)
    return B


def pair_counts_twin(B: torch.Tensor, chunk: int = 0, splits: int = 0) -> torch.Tensor:
    m, W = _check_bitmap(B, "pair_counts")
    C = torch.zeros((m, m), dtype=torch.int64, device=B.device)
    rows = max(1, (2 ** 24) // max(m * W, 1))
    for i0 in range(0, m, rows):
        C[i0:i0 + rows] = _popcount_rows(B[i0:i0 + rows, None, :] & B[None, :, :])
    return torch.triu(C, 1).to(torch.int32)


def class_counts_twin(B: torch.Tensor, prefix: torch.Tensor, cls_ptr: torch.Tensor, ext_item: torch.Tensor,
                      chunk: int = 0, grid: int = 0) -> torch.Tensor:
    nc, ne, P = _check_classes(B, prefix, cls_ptr, ext_item)
    dev = B.device
    counts = torch.zeros(ne, dtype=torch.int64, device=dev)
    if ne == 0:
        return counts
    W = int(B.shape[1])
    owner = _owner(cls_ptr[1:] - cls_ptr[:-1], ne)
    step = max(1, (2 ** 22) // W)
    for e0 in range(0, ne, step):
        o = owner[e0:e0 + step]
        acc = B[ext_item[e0:e0 + step].to(torch.int64)]
        for q in range(P):
            acc = acc & B[prefix[o, q].to(torch.int64)]
        counts[e0:e0 + step] = _popcount_rows(acc)
    return counts


class Backend(NamedTuple):
    """The three counting primitives the level loop runs on."""
    bitmap: Callable
    pair: Callable
    cls: Callable


DEVICE = Backend(build_bitmap, pair_counts, class_counts)
TWIN = Backend(build_bitmap_twin, pair_counts_twin, class_counts_twin)


# ---------------------------------------------------------------------------------------------------
# candidate generation and the level loop
# ---------------------------------------------------------------------------------------------------
def join_siblings(F: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The classes of the next level from the frequent ``L``-itemsets ``F`` int32 [k, L], sorted lexicographically:
    ``(q, a)`` and ``(q, b)`` with ``a < b`` give the candidate prefix ``(q, a)`` with extension ``b``.  Returns
    ``(cls, cnt)``: the rows of ``F`` that are a prefix with at least one extension, and how many they have; the
    extensions of row ``r`` are the last items of rows ``r + 1 .. r + cnt`` (``expand_classes``).  Candidates come
    out sorted lexicographically (classes in row order, extensions ascending)."""
    k, L = int(F.shape[0]), int(F.shape[1])
    dev = F.device
    if k < 2:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return z, z.clone()
    gid = torch.zeros(k, dtype=torch.int64, device=dev)
    if L > 1:
        new = (F[1:, :L - 1] != F[:-1, :L - 1]).any(1)
        gid[1:] = torch.cumsum(new.to(torch.int64), 0)
    gsize = torch.bincount(gid)
    gstart = torch.cumsum(gsize, 0) - gsize
    nxt = gsize[gid] - 1 - (torch.arange(k, device=dev) - gstart[gid])
    cls = torch.nonzero(nxt > 0).reshape(-1)
    return cls, nxt[cls]


def expand_classes(F: torch.Tensor, cls: torch.Tensor, cnt: torch.Tensor):
    """``(prefix int32 [classes, L], cls_ptr int64 [classes + 1], ext_item int32 [candidates], owner int64
    [candidates])`` of the classes ``cls`` / ``cnt`` of ``join_siblings``."""
    dev = F.device
    nc = int(cls.numel())
    ptr = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, 0, out=ptr[1:])
    total = int(ptr[-1])
    owner = _owner(cnt, total)
    j = torch.arange(total, device=dev) - ptr[:-1][owner]
    ext = F[cls[owner] + 1 + j, -1].contiguous()
    return F[cls].contiguous(), ptr, ext, owner


class _Blocks:
    """The transactions as row blocks whose bitmaps fit the budget; the bitmap is kept when there is one block."""

    def __init__(self, crow, item, m, backend, budget):
        self.crow, self.item, self.m, self.backend = crow, item, int(m), backend
        n = int(crow.numel()) - 1
        per = max(64, (int(budget) * 8 // max(self.m, 1)) // 64 * 64)
        self.bounds = [(lo, min(lo + per, n)) for lo in range(0, max(n, 1), per)]
        self._kept = None
        self.seconds = 0.0

    def __len__(self):
        return len(self.bounds)

    def __iter__(self):
        if self._kept is not None:
            yield self._kept
            return
        for lo, hi in self.bounds:
            t0 = time.perf_counter()
            a, b = int(self.crow[lo]), int(self.crow[hi])
            B = self.backend.bitmap((self.crow[lo:hi + 1] - a).contiguous(), self.item[a:b].contiguous(), self.m)
            if B.is_cuda:
                torch.cuda.synchronize(B.device)
            self.seconds += time.perf_counter() - t0
            if len(self.bounds) == 1:
                self._kept = B
            yield B


def count_level(cum: torch.Tensor, expand: Callable, count: Callable, blocks, budget: int, keep: int, width: int):
    """One level's candidates counted in batches that fit the budget: ``(rows int32 [kept, width], supports int64
    [kept])`` of the candidates whose support over all ranks is at least ``keep``, in candidate order.

    ``cum`` int64 [parents] holds the running total of the parents' candidates.  A batch is a run of whole parents ``c0 .. c1 - 1``
    with at most ``budget // _CAND_BYTES`` candidates (a single parent is the smallest batch):
    ``expand(c0, c1)`` gives its ``(prefix, cls_ptr, ext, owner)``, ``count(B, lo, hi, prefix, cls_ptr, ext)`` its
    supports on the bitmap ``B`` of the rows ``lo .. hi - 1`` of ``blocks``; the block counts are added and make one
    ``comm.all_reduce`` per batch."""
    dev = cum.device
    cap = max(1, int(budget) // _CAND_BYTES)
    rowsF, rowsS = [], []
    c0, nc, done = 0, int(cum.numel()), 0
    while c0 < nc:
        # the last parent that still fits the batch; a single parent is the smallest batch
        c1 = int(torch.searchsorted(cum, torch.tensor(done + cap, device=dev), right=True))
        c1 = min(max(c1, c0 + 1), nc)
        prefix, ptr, ext, owner = expand(c0, c1)
        counts = torch.zeros(int(ext.numel()), dtype=torch.int64, device=dev)
        for (lo, hi), B in zip(blocks.bounds, blocks):
            counts += count(B, lo, hi, prefix, ptr, ext)
        comm.all_reduce(counts, "sum")
        ok = counts >= keep
        rowsF.append(torch.cat([prefix[owner[ok]], ext[ok].reshape(-1, 1)], 1))
        rowsS.append(counts[ok])
        done = int(cum[c1 - 1])
        c0 = c1
    if not rowsF:
        return (torch.zeros((0, int(width)), dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.int64, device=dev))
    return torch.cat(rowsF), torch.cat(rowsS)


def pattern_columns(levels, dev):
    """``(codes int32 [sum of lens], lens int64 [P], sups int64 [P])`` of the kept ``(rows, supports)`` of every
    level: the patterns back to back, in the levels' order."""
    if not levels:
        return (torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                torch.zeros(0, dtype=torch.int64, device=dev))
    codes = torch.cat([f.reshape(-1) for f, _ in levels])
    lens = torch.cat([torch.full((int(f.shape[0]),), int(f.shape[1]), dtype=torch.int64, device=dev)
                      for f, _ in levels])
    return codes, lens, torch.cat([s for _, s in levels])


def mine(crow: torch.Tensor, item: torch.Tensor, m: int, item_sup: torch.Tensor, min_sup: int, max_len: int,
         backend: Backend, budget: Optional[int] = None, pair_max_items: Optional[int] = None,
         stats: Optional[list] = None):
    """All frequent itemsets of this rank's CSR transactions (``crow`` int64 [n + 1], ``item`` int32 [nnz]: ranks of
    the ``m`` frequent items, ascending and unique within a row), level by level on ``backend``.

    ``item_sup`` int64 [m] holds the items' supports over all ranks.  A candidate is kept when its support over all
    ranks is at least ``max(min_sup, 1)``.  Every rank generates the same candidates from the same all-reduced
    counts; a level's counts make one ``comm.all_reduce`` (one per batch when the level exceeds the budget), and
    the transactions never leave their rank.  When ``m * n / 8`` bytes exceed ``budget`` the rows are cut into
    blocks, each with its own bitmap, and the block counts are added.

    Returns ``(items int32 [sum of lens], lens int64 [P], sups int64 [P])``: the patterns back to back, by
    ``(len, tuple)`` ascending.  ``stats`` (a list) receives one dict per level: level, candidates, kept, seconds,
    path."""
    dev = crow.device
    budget = FPM_BUDGET_BYTES if budget is None else int(budget)
    pair_max = FPM_PAIR_MAX_ITEMS if pair_max_items is None else int(pair_max_items)
    keep = max(int(min_sup), 1)
    m = int(m)
    levels: List[Tuple[torch.Tensor, torch.Tensor]] = []

    if m < 1 or int(max_len) < 1:
        return pattern_columns(levels, dev)
    one = torch.nonzero(item_sup >= keep).reshape(-1)
    F = one.to(torch.int32).reshape(-1, 1)
    if F.shape[0] == 0:
        return pattern_columns(levels, dev)
    levels.append((F, item_sup[one].to(torch.int64)))
    blocks = _Blocks(crow, item, m, backend, budget)
    L = 1
    while L < int(max_len) and F.shape[0] >= 2:
        t0 = time.perf_counter()
        path = "class"
        if L == 1 and m <= pair_max:
            path = "pair"
            C = None
            for B in blocks:
                c = u32(backend.pair(B))
                C = c if C is None else C.add_(c)
            comm.all_reduce(C, "sum")
            idx = torch.nonzero(C >= keep)             # row-major: sorted by (i, j); only i < j was counted
            n_cand = m * (m - 1) // 2
            newF = idx.to(torch.int32)
            newS = C[idx[:, 0], idx[:, 1]]
            del C
        else:
            cls, cnt = join_siblings(F)
            cum = torch.cumsum(cnt, 0)
            n_cand = int(cum[-1]) if cum.numel() else 0
            newF, newS = count_level(cum, lambda c0, c1: expand_classes(F, cls[c0:c1], cnt[c0:c1]),
                                     lambda B, lo, hi, *cand: backend.cls(B, *cand), blocks, budget, keep, L + 1)
        L += 1
        if stats is not None:
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            stats.append({"level": L, "candidates": int(n_cand), "kept": int(newF.shape[0]), "path": path,
                          "seconds": time.perf_counter() - t0, "bitmap_seconds": blocks.seconds,
                          "row_blocks": len(blocks)})
        if newF.shape[0] == 0:
            break
        F = newF.contiguous()
        levels.append((F, newS))
    return pattern_columns(levels, dev)
