"""Sequential-pattern mining on the device: S-step / I-step support counts on a vertical bitmap with one field per
sequence (``alink_fpm_seq_counts`` in ``csrc/fpm.hip``) and the level-wise candidate generation around it in torch.

Every sequence of a rank gets a field of ``w`` bits, ``w`` the smallest of 8, 16, 32 and 64 that holds the rank's
longest encoded sequence; fields sit back to back in 64-bit words.  Bit ``j`` of sequence ``t``'s field in row ``i``
of ``B`` (int64 ``[m, W]``, ``W = fpm.row_stride(n_seq * w)``) says that element ``j`` of sequence ``t`` holds frequent
item ``i``.  ``B`` is ``fpm.build_bitmap`` of the "slot CSR": slot ``t * w + j`` is a transaction holding element
``j``'s items, slots past a sequence's end are empty.

A pattern is a row of step codes ``2 * item + s``: ``s = 1`` opens a new element with the item (S-step), ``s = 0``
adds it to the last element (I-step; the item is greater than the one before it).  The first code is an S code.  The
bitmap of a pattern holds bit ``j`` of a field when the pattern has a match ending at element ``j``::

    cur = B[item_0]
    S-step by i:  cur = after(cur) & B[i]     after(x): in every field, the bits strictly above the lowest set bit
    I-step by i:  cur = cur & B[i]
    support = number of fields of cur that are not zero

With ``L`` bit 0 and ``H`` the top bit of every field: ``after`` smears ``y |= (y << s) & K_s`` for ``s = 1, 2, 4, ..,
w / 2`` (``K_s``: the in-field positions ``>= s``) and returns ``(y << 1) & ~L``; the non-zero fields are
``popcount((((x & ~H) + ~H) | x) & H)``.  Left shifts, AND / OR and a wrapping add only, so the torch twin
(``seq_counts_twin``) computes the same on int64.  The supports depend on the data and the threshold, not on the
miner: ``mine`` returns exactly the patterns of the host path ``models/associationrule/mining.prefix_span`` (the CPU
path and the oracle), and every count is the same for every grid, chunk, split into row blocks and split over ranks.

``device_selected(device, n_rows)`` decides whether ``PrefixSpanBatchOp`` takes this path: a CUDA device,
``ALINK_PREFIXSPAN_HIP`` not ``0``, at least ``SPM_MIN_ROWS`` rows (``ALINK_PREFIXSPAN_HIP=1`` forces it at any
size) and ``_lib.kernels_enabled()`` (no quiet fall-back).
"""
from __future__ import annotations

import time
from typing import Callable, List, NamedTuple, Optional, Tuple

import torch

from . import _lib
from . import fpm as F

__all__ = ["device_selected", "field_width", "seq_counts", "seq_counts_twin", "seq_after_twin", "seq_fields_twin",
           "Backend", "DEVICE", "TWIN", "join_steps", "mine", "decode", "SPM_CALLS", "SPM_MIN_ROWS", "WIDTHS"]

SPM_CALLS = 0                   # launches of alink_fpm_seq_counts (tests read it)
SPM_MIN_ROWS = 512              # rows (over all ranks) from which the device path is taken: the measured crossover
#                                 against the host path, between 300 rows (host 5.7 ms, device 9.7 ms) and 1000 rows
#                                 (17.0 ms, 8.5 ms) at minSupportPercent 0.05; profiles/prefixspan.txt records the run
WIDTHS = (8, 16, 32, 64)        # bits of a sequence's field


def device_selected(device, n_rows: int) -> bool:
    """True when ``PrefixSpanBatchOp`` runs on the device: a CUDA device, not switched off by
    ``ALINK_PREFIXSPAN_HIP=0``, ``n_rows >= SPM_MIN_ROWS`` unless ``ALINK_PREFIXSPAN_HIP=1`` forces it, and the
    kernel library by the one fall-back rule (``_lib.kernels_enabled``: a missing library is an error)."""
    return _lib.sized_gate("ALINK_PREFIXSPAN_HIP", device, n_rows, SPM_MIN_ROWS)


def field_width(longest: int) -> int:
    """The smallest field width that holds a sequence of ``longest`` elements (at most 64)."""
    for w in WIDTHS:
        if int(longest) <= w:
            return w
    raise ValueError("field_width: a sequence of more than 64 elements has no field")


def _signed(x: int) -> int:
    return x - (1 << 64) if x >= 1 << 63 else x


def _low(w: int) -> int:
    """Bit 0 of every ``w``-bit field of a 64-bit word."""
    return sum(1 << k for k in range(0, 64, w))


def seq_after_twin(x: torch.Tensor, w: int) -> torch.Tensor:
    """In every ``w``-bit field of the int64 words ``x``: the bits strictly above the lowest set bit."""
    if w == 64:
        return torch.where(x != 0, ~(x ^ (x - 1)), torch.zeros_like(x))
    L = _low(w)
    y = x
    s = 1
    while s <= w // 2:
        y = y | ((y << s) & _signed(~(L * ((1 << s) - 1)) & (2 ** 64 - 1)))
        s *= 2
    return (y << 1) & _signed(~L & (2 ** 64 - 1))


def seq_fields_twin(x: torch.Tensor, w: int) -> torch.Tensor:
    """Sum over the last axis of the numbers of non-zero ``w``-bit fields of the int64 words ``x``."""
    H = _low(w) << (w - 1)
    nH = _signed(~H & (2 ** 64 - 1))
    return F._popcount_rows((((x & nH) + nH) | x) & _signed(H))


def _ran() -> None:
    global SPM_CALLS
    SPM_CALLS += 1


def _check_seq(B, n_seq, w, prefix, cls_ptr, ext) -> Tuple[int, int, int]:
    m, W = F._check_bitmap(B, "seq_counts")
    if int(w) not in WIDTHS or int(n_seq) < 0 or W != F.row_stride(int(n_seq) * int(w)):
        raise ValueError("seq_counts: w of 8, 16, 32 or 64 and a bitmap of row_stride(n_seq * w) words are needed")
    nc, ne, P = F._check_grouped("seq_counts", B, prefix, cls_ptr, ext, 2 * m)      # step codes 2 * item + s
    if nc and bool(((prefix[:, 0] & 1) == 0).any()):
        raise ValueError("seq_counts: every prefix starts with an S code")
    return nc, ne, P


def seq_counts(B: torch.Tensor, n_seq: int, w: int, prefix: torch.Tensor, cls_ptr: torch.Tensor, ext: torch.Tensor,
               chunk: int = 0, grid: int = 0) -> torch.Tensor:
    """int64 [candidates] sequence supports of candidates grouped by parent pattern on a GPU: candidate ``e`` of
    class ``c`` (``cls_ptr[c] <= e < cls_ptr[c + 1]``) is the pattern of step codes ``prefix[c] + (ext[e],)`` on the
    field bitmap ``B`` of ``n_seq`` sequences of ``w`` bits.  ``chunk``: words a wave owns per unit (rounded up to
    128; 0: chosen from the shape); ``grid``: workgroups.  Neither changes a count."""
    nc, ne, P = _check_seq(B, n_seq, w, prefix, cls_ptr, ext)
    if not B.is_cuda or int(chunk) < 0 or int(grid) < 0:
        raise ValueError("seq_counts: a GPU bitmap, chunk >= 0 and grid >= 0 are needed")
    counts = torch.zeros(ne, dtype=torch.int64, device=B.device)
    if ne == 0:
        return counts
    _lib.call("alink_fpm_seq_counts", B.data_ptr(), int(B.shape[1]), prefix.data_ptr(), P, cls_ptr.data_ptr(),
              ext.data_ptr(), nc, counts.data_ptr(), int(w), int(chunk), int(grid), _lib.stream_ptr(B.device))
    _ran()
    return counts


def seq_counts_twin(B: torch.Tensor, n_seq: int, w: int, prefix: torch.Tensor, cls_ptr: torch.Tensor,
                    ext: torch.Tensor, chunk: int = 0, grid: int = 0) -> torch.Tensor:
    nc, ne, P = _check_seq(B, n_seq, w, prefix, cls_ptr, ext)
    dev = B.device
    w = int(w)
    counts = torch.zeros(ne, dtype=torch.int64, device=dev)
    if ne == 0:
        return counts
    W = int(B.shape[1])
    owner = F._owner(cls_ptr[1:] - cls_ptr[:-1], ne)
    step = max(1, (2 ** 22) // W)
    for e0 in range(0, ne, step):
        pre = prefix[owner[e0:e0 + step]].to(torch.int64)
        cur = B[pre[:, 0] >> 1]
        for q in range(1, P):
            s = (pre[:, q] & 1).bool().reshape(-1, 1)
            cur = torch.where(s, seq_after_twin(cur, w), cur) & B[pre[:, q] >> 1]
        code = ext[e0:e0 + step].to(torch.int64)
        s = (code & 1).bool().reshape(-1, 1)
        counts[e0:e0 + step] = seq_fields_twin(torch.where(s, seq_after_twin(cur, w), cur) & B[code >> 1], w)
    return counts


class Backend(NamedTuple):
    """The two primitives the level loop runs on."""
    bitmap: Callable
    seq: Callable


DEVICE = Backend(F.build_bitmap, seq_counts)
TWIN = Backend(F.build_bitmap_twin, seq_counts_twin)


# ---------------------------------------------------------------------------------------------------
# candidate generation and the level loop
# ---------------------------------------------------------------------------------------------------
class _Steps(NamedTuple):
    cnt: torch.Tensor           # int64 [k]: candidates of parent r
    n_s: torch.Tensor           # int64 [k]: its S-extensions (the S codes of its sibling group)
    s_first: torch.Tensor       # int64 [k]: where they start in ``s_rows``
    s_rows: torch.Tensor        # int64: the rows of F whose last code is an S code, in row order
    k_pos: torch.Tensor         # int64 [k]: position of r among the rows of its kind (``k_rows[kind]``)
    k_rows: Tuple[torch.Tensor, torch.Tensor]


def join_steps(Fq: torch.Tensor) -> _Steps:
    """The candidates of the next level from the frequent patterns ``Fq`` int32 [k, L] of step codes, sorted
    lexicographically.  Siblings share all but the last code.  For a pattern ``r = (q, c_a)`` and every sibling
    ``(q, c_b)``: when ``c_b`` is an S code, the S-extension of ``r`` by ``b`` (``b = a`` included); when both codes
    have the same kind and ``b > a``, the I-extension of ``r`` by ``b``.  No other extension of ``r`` can be
    frequent (dropping ``a`` from it gives the sibling), so this only prunes.  ``expand_steps`` lists them."""
    k, L = int(Fq.shape[0]), int(Fq.shape[1])
    dev = Fq.device
    gid = torch.zeros(k, dtype=torch.int64, device=dev)
    if L > 1 and k > 1:
        new = (Fq[1:, :L - 1] != Fq[:-1, :L - 1]).any(1)
        gid[1:] = torch.cumsum(new.to(torch.int64), 0)
    kind = (Fq[:, -1] & 1).to(torch.int64)
    ng = int(gid[-1]) + 1 if k else 0
    # rows of one kind keep their order, so the siblings of a kind are a run of k_rows[kind]
    k_rows = tuple(torch.nonzero(kind == v).reshape(-1) for v in (0, 1))
    k_pos = torch.zeros(k, dtype=torch.int64, device=dev)
    n_kind = torch.zeros((2, max(ng, 1)), dtype=torch.int64, device=dev)
    for v in (0, 1):
        k_pos[k_rows[v]] = torch.arange(int(k_rows[v].numel()), device=dev)
        n_kind[v] = torch.bincount(gid[k_rows[v]], minlength=max(ng, 1))
    first = torch.cumsum(n_kind, 1) - n_kind                    # where a group's rows of a kind start in k_rows[kind]
    n_i = n_kind[kind, gid] - 1 - (k_pos - first[kind, gid])    # same kind, greater item: the rows after r
    n_s = n_kind[1][gid]
    return _Steps(n_s + n_i, n_s, first[1][gid], k_rows[1], k_pos, k_rows)


def expand_steps(Fq: torch.Tensor, st: _Steps, c0: int, c1: int):
    """``(prefix int32 [c1 - c0, L], cls_ptr int64, ext int32 [candidates], owner int64 [candidates])`` of the
    parents ``c0 .. c1 - 1`` of ``join_steps``: candidates grouped by parent, codes ascending within a parent."""
    dev = Fq.device
    nc = c1 - c0
    rows = torch.arange(c0, c1, device=dev)
    n_s = st.n_s[c0:c1]
    n_i = st.cnt[c0:c1] - n_s
    kind = (Fq[c0:c1, -1] & 1).to(torch.int64)
    last = Fq[:, -1].to(torch.int64)

    def runs(cnt):
        total = int(cnt.sum())
        o = F._owner(cnt, total)
        j = torch.arange(total, device=dev) - (torch.cumsum(cnt, 0) - cnt)[o]
        return o, j

    o_s, j_s = runs(n_s)
    code_s = last[st.s_rows[st.s_first[c0:c1][o_s] + j_s]]
    o_i, j_i = runs(n_i)
    pos = st.k_pos[rows][o_i] + 1 + j_i
    code_i = torch.zeros(int(o_i.numel()), dtype=torch.int64, device=dev)
    for v in (0, 1):
        sel = kind[o_i] == v
        code_i[sel] = last[st.k_rows[v][pos[sel]]] & ~1
    owner = torch.cat([o_s, o_i])
    code = torch.cat([code_s, code_i])
    span = 2 * (int(last.max()) // 2 + 1) if last.numel() else 2
    key = torch.sort(owner * span + code).values
    owner = torch.div(key, span, rounding_mode="floor")
    ptr = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(owner, minlength=nc), 0, out=ptr[1:])
    return Fq[c0:c1].contiguous(), ptr, (key - owner * span).to(torch.int32), owner


def mine(crow: torch.Tensor, item: torch.Tensor, m: int, n_seq: int, w: int, item_sup: torch.Tensor, min_sup: int,
         max_len: int, backend: Backend, budget: Optional[int] = None, stats: Optional[list] = None):
    """All frequent sequential patterns of this rank's sequences, level by level on ``backend``.  ``crow`` int64
    [n_seq * w + 1] and ``item`` int32 are the slot CSR (slot ``t * w + j``: the ranks of element ``j`` of sequence
    ``t`` among the ``m`` frequent items, ascending and unique); ``item_sup`` int64 [m] holds the items' sequence
    supports over all ranks.

    A pattern is kept when its support over all ranks is at least ``max(min_sup, 1)``; a level ends the loop when it
    keeps nothing or the patterns are ``max_len`` items long.  Every rank generates the same candidates from the
    same all-reduced counts (one ``comm.all_reduce`` per batch of a level); the sequences never leave their rank, and
    each rank has its own ``w``.  When ``m * n_seq * w / 8`` bytes exceed ``budget`` the sequences are cut into
    blocks, each with its own bitmap, and the block counts are added.

    Returns ``(codes int32 [sum of lens], lens int64 [P], sups int64 [P])``: the patterns' step codes back to back,
    by ``(len, codes)`` ascending.  ``stats`` (a list) receives one dict per level: level, candidates, kept, seconds,
    path, w, W."""
    dev = crow.device
    budget = F.FPM_BUDGET_BYTES if budget is None else int(budget)
    keep = max(int(min_sup), 1)
    m, n_seq, w = int(m), int(n_seq), int(w)
    levels: List[Tuple[torch.Tensor, torch.Tensor]] = []
    if m < 1:
        return F.pattern_columns(levels, dev)
    one = torch.nonzero(item_sup >= keep).reshape(-1)
    Fq = (2 * one + 1).to(torch.int32).reshape(-1, 1)
    if Fq.shape[0] == 0:
        return F.pattern_columns(levels, dev)
    levels.append((Fq, item_sup[one].to(torch.int64)))
    blocks = F._Blocks(crow, item, m, backend, budget)          # cut at multiples of 64 slots: whole fields
    L = 1
    while L < int(max_len) and Fq.shape[0] >= 1:
        t0 = time.perf_counter()
        st = join_steps(Fq)
        cum = torch.cumsum(st.cnt, 0)
        n_cand = int(cum[-1])
        newF, newS = F.count_level(cum, lambda c0, c1: expand_steps(Fq, st, c0, c1),
                                   lambda B, lo, hi, *cand: backend.seq(B, (hi - lo) // w, w, *cand),
                                   blocks, budget, keep, L + 1)
        L += 1
        if stats is not None:
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            stats.append({"level": L, "candidates": n_cand, "kept": int(newF.shape[0]), "path": "seq",
                          "seconds": time.perf_counter() - t0, "bitmap_seconds": blocks.seconds,
                          "row_blocks": len(blocks), "w": w, "W": F.row_stride(n_seq * w)})
        if newF.shape[0] == 0:
            break
        Fq = newF.contiguous()
        levels.append((Fq, newS))
    return F.pattern_columns(levels, dev)


def decode(cols):
    """``{tuple of element tuples of 1-based item ids: support}`` (the keys of ``M.prefix_span``) from the pattern
    columns of ``mine``, in their order."""
    codes, lens, sups = (t.cpu().tolist() for t in cols)
    out = {}
    p = 0
    for ln, s in zip(lens, sups):
        pat: List[List[int]] = []
        for c in codes[p:p + ln]:
            if c & 1:
                pat.append([(c >> 1) + 1])
            else:
                pat[-1].append((c >> 1) + 1)
        out[tuple(tuple(e) for e in pat)] = s
        p += ln
    return out
