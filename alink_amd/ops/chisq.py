"""Pearson chi-square tests of many columns against one label on the device: contingency counts and the statistic
(``csrc/chisq.hip``) and the sorted entry streams they read, in torch.

A block of columns is one **sorted entry stream**: ``colptr`` int64 [c + 1], ``bits`` int64 [E] (the value's
canonical bit pattern, ascending inside a column) and ``lab`` int32 [E] (the row's label code in ``[0, L)``).  A
category starts wherever ``bits`` or the column changes; ``categories`` numbers them.  ``csr_stream`` makes the stream
of CSR rows without densifying them (stored ``+0.0`` joins the implicit zero category, ``-0.0`` stays its own, every
NaN gets one pattern), ``dense_stream`` the one of dense fp64 rows, ``column_stream`` the one of a table column.

Two kernels, each with a torch twin of the same arguments that runs on any device (``*_twin``): ``counts`` (the
stream into ``cnt [G, L]``; integers, so the same for every grid, chunk and variant) and ``stat`` (per column the
statistic, the category count ``R`` and the label count ``Lc``).  ``models/statistics/chisq.chi_square_arrays``
takes the two as a ``Backend``, so the CPU tests drive the same block loop through the twins (``TWIN``) that the
operators drive through the kernels (``DEVICE``).  The host path ``models/statistics/summary.chi_square_test`` is
the CPU path and the oracle.

``device_selected(device, cells)`` decides whether the four chi-square operators take this path: a CUDA device,
``ALINK_CHISQ_HIP`` not ``0``, at least ``CHISQ_MIN_CELLS`` cells (rows x columns; ``ALINK_CHISQ_HIP=1`` forces it at
any size) and ``_lib.kernels_enabled()`` (no quiet fall-back).
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Tuple

import torch

from . import _lib

__all__ = ["device_selected", "counts", "stat", "counts_twin", "stat_twin", "u32", "Backend", "DEVICE", "TWIN",
           "canon_bits", "csr_has_duplicates", "csr_stream", "dense_stream", "column_stream", "categories",
           "column_blocks",
           "CHISQ_CALLS", "CHISQ_BUDGET_BYTES", "CHISQ_MIN_CELLS", "CHISQ_MAX_LABELS", "CHISQ_UNIT"]

CHISQ_CALLS = 0                 # launches of the HIP chi-square kernels (tests read it)
CHISQ_BUDGET_BYTES = 2 ** 31    # bytes the uint32 count table cnt [G, L] of one column block may take
CHISQ_MIN_CELLS = 2800          # cells (rows x columns, over all ranks) from which the device path is taken: the
#                                 measured crossover against the host path, between 2400 cells (300 rows x 8 integer
#                                 columns: host 2.08 ms, device 2.25 ms) and 3200 cells (2.47 ms, 2.26 ms);
#                                 profiles/chisq.txt records the run
CHISQ_MAX_LABELS = 1024         # labels the kernels hold (one LDS counter, one register slot per lane, each)
CHISQ_UNIT = 256                # categories one wave adds in ascending order (csrc/chisq.hip CQ_UNIT)
CHISQ_VARIANT = 0               # counts kernel: 0 LDS histogram for runs that fill a 64-entry step, 1 per-entry
#                                 global atomics throughout.  8.3e8 entries of Zipf-skewed counts: 3.3 ms against
#                                 43.8 ms; the same entries all distinct (both take the per-entry path): 151 ms for
#                                 the stage either way.  0 is kept (profiles/chisq.txt)
_NAN_BITS = 0x7FF8000000000000


def device_selected(device, cells) -> bool:
    """True when the chi-square operators run on the device: a CUDA device, not switched off by
    ``ALINK_CHISQ_HIP=0``, ``cells >= CHISQ_MIN_CELLS`` unless ``ALINK_CHISQ_HIP=1`` forces it, and the kernel
    library by the one fall-back rule (``_lib.kernels_enabled``: a missing library is an error).  ``cells`` may be
    a function that counts them: it is called only when the size decides (counting is a collective)."""
    return _lib.sized_gate("ALINK_CHISQ_HIP", device, cells, CHISQ_MIN_CELLS)


def u32(C: torch.Tensor) -> torch.Tensor:
    """The uint32 counts of ``counts`` (int32 storage) as int64."""
    return C.to(torch.int64) & 0xFFFFFFFF


def _ran() -> None:
    global CHISQ_CALLS
    CHISQ_CALLS += 1


# ---------------------------------------------------------------------------------------------------
# checks shared by the kernels' wrappers and the twins
# ---------------------------------------------------------------------------------------------------
def _check_counts(g, lab, G, L, chunk, grid, variant) -> int:
    if not (g.dtype == torch.int32 and lab.dtype == torch.int32 and g.dim() == 1 and g.shape == lab.shape
            and g.device == lab.device and g.is_contiguous() and lab.is_contiguous()):
        raise ValueError("counts: g int32 [E] and lab int32 [E], contiguous on one device, are needed")
    if not (0 <= int(G) < 2 ** 31 and 1 <= int(L) <= CHISQ_MAX_LABELS):
        raise ValueError(f"counts: 0 <= G < 2^31 categories and 1 <= L <= {CHISQ_MAX_LABELS} labels are needed")
    if int(chunk) < 0 or int(grid) < 0 or int(variant) not in (0, 1):
        raise ValueError("counts: chunk >= 0, grid >= 0 and variant 0 or 1 are needed")
    return int(g.numel())


def _check_stat(cnt, gptr, cs, zero) -> Tuple[int, int, int]:
    ok = (cnt.dtype == torch.int64 and cnt.dim() == 2 and cnt.is_contiguous() and gptr.dtype == torch.int64
          and gptr.dim() == 1 and gptr.numel() >= 1 and gptr.is_contiguous() and cs.dtype == torch.int64
          and cs.dim() == 2 and cs.is_contiguous() and cnt.device == gptr.device == cs.device
          and cs.shape[0] == gptr.numel() - 1 and cs.shape[1] == cnt.shape[1])
    if ok and zero is not None:
        ok = zero.dtype == torch.int64 and zero.shape == cs.shape and zero.is_contiguous() and zero.device == cs.device
    if not ok:
        raise ValueError("stat: cnt int64 [G, L], gptr int64 [C + 1], cs int64 [C, L] and zero (None or int64 "
                         "[C, L]), contiguous on one device, are needed")
    G, L, C = int(cnt.shape[0]), int(cnt.shape[1]), int(cs.shape[0])
    if not 1 <= L <= CHISQ_MAX_LABELS:
        raise ValueError(f"stat: 1 <= L <= {CHISQ_MAX_LABELS} labels are needed")
    if int(gptr[0]) != 0 or int(gptr[-1]) != G or (C and bool((gptr[1:] < gptr[:-1]).any())):
        raise ValueError("stat: gptr must ascend from 0 to the number of categories")
    return G, L, C


def _units(gptr: torch.Tensor, extra: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(uptr int64 [C + 1], ucol int32 [U])``: the units of ``CHISQ_UNIT`` categories of every column (``extra``
    = 1 when each column has a zero row after its categories)."""
    dev = gptr.device
    C = int(gptr.numel()) - 1
    per = (gptr[1:] - gptr[:-1] + int(extra) + CHISQ_UNIT - 1) // CHISQ_UNIT
    uptr = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    torch.cumsum(per, 0, out=uptr[1:])
    U = int(uptr[-1]) if C else 0
    ucol = torch.repeat_interleave(torch.arange(C, device=dev, dtype=torch.int32), per, output_size=U)
    return uptr, ucol.contiguous()


# ---------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------
def counts(g: torch.Tensor, lab: torch.Tensor, G: int, L: int, chunk: int = 0, grid: int = 0,
           variant: Optional[int] = None) -> torch.Tensor:
    """uint32 counts in int32 storage ``[G, L]`` (``u32`` widens them) of a GPU stream: entry ``e`` adds one to
    ``cnt[g[e], lab[e]]``.  ``chunk``: entries a wave owns at a time (0: 2048); ``grid``: workgroups (0: chosen from
    ``E``); ``variant``: 0 LDS histogram, 1 per-entry global atomics (default ``CHISQ_VARIANT``).  None of them
    changes a count."""
    variant = CHISQ_VARIANT if variant is None else int(variant)
    E = _check_counts(g, lab, G, L, chunk, grid, variant)
    if not g.is_cuda:
        raise ValueError("counts: tensors on a GPU are needed")
    cnt = torch.zeros((int(G), int(L)), dtype=torch.int32, device=g.device)
    if E == 0:
        return cnt
    if int(G) < 1:
        raise ValueError("counts: entries without a category")
    bad = torch.zeros(1, dtype=torch.int32, device=g.device)
    _lib.call("alink_chisq_counts", g.data_ptr(), lab.data_ptr(), E, int(G), int(L), cnt.data_ptr(), bad.data_ptr(),
              int(chunk), int(grid), variant, _lib.stream_ptr(g.device))
    _ran()
    if int(bad):
        raise ValueError("counts: an entry outside [0, G) x [0, L)")
    return cnt


def stat(cnt: torch.Tensor, gptr: torch.Tensor, cs: torch.Tensor, zero: Optional[torch.Tensor] = None,
         grid: int = 0):
    """``(value float64 [C], R int32 [C], Lc int32 [C])`` of ``C`` columns on a GPU.  Column ``c`` owns the rows
    ``gptr[c] .. gptr[c + 1]`` of ``cnt`` int64 [G, L]; ``cs`` int64 [C, L] holds the label totals of its cross table
    (the zero row included); ``zero`` int64 [C, L], when given, is one more category after them.  ``R`` counts the
    categories with a row sum > 0, ``Lc`` the labels with ``cs > 0``.  ``grid`` (workgroups) changes no bit."""
    G, L, C = _check_stat(cnt, gptr, cs, zero)
    if not cnt.is_cuda or int(grid) < 0:
        raise ValueError("stat: tensors on a GPU and grid >= 0 are needed")
    dev = cnt.device
    value = torch.zeros(C, dtype=torch.float64, device=dev)
    R = torch.zeros(C, dtype=torch.int32, device=dev)
    Lc = torch.zeros(C, dtype=torch.int32, device=dev)
    if C == 0:
        return value, R, Lc
    uptr, ucol = _units(gptr, 0 if zero is None else 1)
    U = int(ucol.numel())
    part = torch.zeros(max(U, 1), dtype=torch.float64, device=dev)
    rcat = torch.zeros(max(U, 1), dtype=torch.int32, device=dev)
    _lib.call("alink_chisq_stat", cnt.data_ptr(), gptr.data_ptr(), cs.data_ptr(),
              0 if zero is None else zero.data_ptr(), ucol.data_ptr(), uptr.data_ptr(), U, C, L, part.data_ptr(),
              rcat.data_ptr(), value.data_ptr(), R.data_ptr(), Lc.data_ptr(), int(grid), _lib.stream_ptr(dev))
    _ran()
    return value, R, Lc


# ---------------------------------------------------------------------------------------------------
# torch twins: the same arguments and results on any device (the CPU path of the tests)
# ---------------------------------------------------------------------------------------------------
def counts_twin(g: torch.Tensor, lab: torch.Tensor, G: int, L: int, chunk: int = 0, grid: int = 0,
                variant: Optional[int] = None) -> torch.Tensor:
    E = _check_counts(g, lab, G, L, chunk, grid, CHISQ_VARIANT if variant is None else int(variant))
    cnt = torch.zeros(int(G) * int(L), dtype=torch.int64, device=g.device)
    if E == 0:
        return cnt.reshape(int(G), int(L)).to(torch.int32)
    if int(G) < 1 or int(g.min()) < 0 or int(g.max()) >= int(G) or int(lab.min()) < 0 or int(lab.max()) >= int(L):
        raise ValueError("counts: an entry outside [0, G) x [0, L)")
    cnt.index_add_(0, g.to(torch.int64) * int(L) + lab.to(torch.int64), torch.ones(E, dtype=torch.int64,
                                                                                   device=g.device))
    return cnt.reshape(int(G), int(L)).to(torch.int32)         # wraps to the uint32 storage like the kernel


def stat_twin(cnt: torch.Tensor, gptr: torch.Tensor, cs: torch.Tensor, zero: Optional[torch.Tensor] = None,
              grid: int = 0):
    G, L, C = _check_stat(cnt, gptr, cs, zero)
    dev = cnt.device
    n = cs.sum(1).to(torch.float64)
    csd = cs.to(torch.float64)

    def terms(rows, col):
        """Per row of ``rows`` (a category of column ``col[i]``): the sum of its cells' terms, and rs > 0."""
        rs = rows.sum(1)
        ex = rs.to(torch.float64)[:, None] * csd[col] / n[col][:, None]
        t = rows.to(torch.float64) - ex
        keep = (rs > 0)[:, None] & (cs[col] > 0)
        one = torch.ones((), dtype=torch.float64, device=dev)
        return torch.where(keep, t * t / torch.where(keep, ex, one), torch.zeros_like(ex)).sum(1), rs > 0

    value = torch.zeros(C, dtype=torch.float64, device=dev)
    R = torch.zeros(C, dtype=torch.int64, device=dev)
    if G:
        col = torch.searchsorted(gptr, torch.arange(G, device=dev), right=True) - 1
        step = max(1, (2 ** 22) // L)
        for a in range(0, G, step):
            s, live = terms(cnt[a:a + step], col[a:a + step])
            value.index_add_(0, col[a:a + step], s)
            R.index_add_(0, col[a:a + step], live.to(torch.int64))
    if zero is not None and C:
        s, live = terms(zero, torch.arange(C, device=dev))
        value += s
        R += live.to(torch.int64)
    return value, R.to(torch.int32), (cs > 0).sum(1).to(torch.int32)


class Backend(NamedTuple):
    """The two primitives the block loop runs on."""
    counts: Callable
    stat: Callable


DEVICE = Backend(counts, stat)
TWIN = Backend(counts_twin, stat_twin)


# ---------------------------------------------------------------------------------------------------
# sorted entry streams
# ---------------------------------------------------------------------------------------------------
def canon_bits(x: torch.Tensor) -> torch.Tensor:
    """The int64 bit patterns of float64 values, every NaN as one pattern; ``-0.0`` and ``+0.0`` stay apart (the
    host keys by ``repr``)."""
    x = x.to(torch.float64).contiguous()
    b = x.view(torch.int64)
    return torch.where(x != x, torch.full_like(b, _NAN_BITS), b)


def _sort_by(col: torch.Tensor, bits: torch.Tensor, lab: torch.Tensor, c: int):
    """The entries by (column, bits), by two stable sorts as ``kmeans_sparse.prepare`` makes its CSC view."""
    bits, o1 = torch.sort(bits, stable=True)
    col, lab = col[o1], lab[o1]
    col, o2 = torch.sort(col, stable=True)
    bits, lab = bits[o2], lab[o2]
    colptr = torch.zeros(int(c) + 1, dtype=torch.int64, device=col.device)
    if col.numel():
        torch.cumsum(torch.bincount(col, minlength=int(c)), 0, out=colptr[1:])
    return colptr, bits.contiguous(), lab.contiguous()


def csr_has_duplicates(crow: torch.Tensor, col: torch.Tensor) -> bool:
    """Whether a CSR row stores a column index twice.  Rows whose indices strictly ascend (the usual case) are
    settled by one comparison; otherwise the (row, column) keys are sorted."""
    nnz = int(col.numel())
    if nnz < 2:
        return False
    col = col.to(torch.int64)
    first = torch.zeros(nnz, dtype=torch.bool, device=col.device)
    start = crow[:-1]
    first[start[start < nnz]] = True                        # an entry that opens a row
    if bool(((col[1:] > col[:-1]) | first[1:]).all()):
        return False
    n = int(crow.numel()) - 1
    row = torch.repeat_interleave(torch.arange(n, device=col.device), crow[1:] - crow[:-1], output_size=nnz)
    key = torch.sort(row * (int(col.max()) + 1) + col).values
    return bool((key[1:] == key[:-1]).any())


def csr_stream(crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor, lab_row: torch.Tensor, d: int):
    """``(colptr, bits, lab)`` of CSR rows over ``d`` columns; ``lab_row`` int32 [n] holds each row's label code,
    negative when the row takes no part.  Stored ``+0.0`` entries and indices outside ``[0, d)`` are dropped.  The
    matrix is never densified: the stream has at most ``nnz`` entries.  A row must not store an index twice
    (``csr_has_duplicates``; such a column takes the host path): both entries would count."""
    dev = val.device
    n = int(crow.numel()) - 1
    row = torch.repeat_interleave(torch.arange(n, device=dev), crow[1:] - crow[:-1], output_size=int(col.numel()))
    bits = canon_bits(val)
    col = col.to(torch.int64)
    lab = lab_row.to(device=dev, dtype=torch.int32)[row]
    keep = (bits != 0) & (col >= 0) & (col < int(d)) & (lab >= 0)
    return _sort_by(col[keep], bits[keep], lab[keep], d)


def dense_stream(X: torch.Tensor, lab_row: torch.Tensor):
    """``(colptr, bits, lab)`` of dense float64 rows ``[n, c]``: per column, a sort of the bit patterns along the
    rows; the labels are gathered with the order.  Rows with a negative label code take no part."""
    dev = X.device
    lab_row = lab_row.to(device=dev, dtype=torch.int32)
    part = lab_row >= 0
    if not bool(part.all()):
        X, lab_row = X[part], lab_row[part]
    n, c = int(X.shape[0]), int(X.shape[1])
    bits, order = torch.sort(canon_bits(X).t().contiguous(), dim=1, stable=True)
    lab = lab_row[order.reshape(-1)]
    colptr = torch.arange(c + 1, dtype=torch.int64, device=dev) * n
    return colptr, bits.reshape(-1).contiguous(), lab.contiguous()


def column_stream(codes: List[torch.Tensor], valid: List[Optional[torch.Tensor]], lab_row: torch.Tensor):
    """``(colptr, bits, lab)`` of table columns given as exact int64 codes [n] each (value bits or dictionary
    ids); a row takes no part in a column where ``valid`` is False or its label code is negative."""
    dev = lab_row.device
    lab_row = lab_row.to(torch.int32)
    bs, ls, ptr = [], [], [0]
    for code, ok in zip(codes, valid):
        keep = lab_row >= 0 if ok is None else (lab_row >= 0) & ok.to(dev)
        b, o = torch.sort(code.to(dev)[keep], stable=True)
        bs.append(b)
        ls.append(lab_row[keep][o])
        ptr.append(ptr[-1] + int(b.numel()))
    z = torch.zeros(0, dtype=torch.int64, device=dev)
    return (torch.tensor(ptr, dtype=torch.int64, device=dev), torch.cat(bs + [z]).contiguous(),
            torch.cat(ls + [z.to(torch.int32)]).contiguous())


def categories(colptr: torch.Tensor, bits: torch.Tensor):
    """``(cat int64 [E], gptr int64 [c + 1], kcol int64 [G], kbits int64 [G])``: the running category index of
    every entry (a category starts wherever ``bits`` or the column changes), the category range of every column, and
    each category's key."""
    dev = bits.device
    E, c = int(bits.numel()), int(colptr.numel()) - 1
    start = torch.ones(E, dtype=torch.bool, device=dev)
    if E > 1:
        start[1:] = bits[1:] != bits[:-1]
    first = colptr[:-1]
    start[first[first < E]] = True
    run = torch.zeros(E + 1, dtype=torch.int64, device=dev)
    torch.cumsum(start.to(torch.int64), 0, out=run[1:])
    gptr = run[colptr].contiguous()
    kbits = bits[start]
    kcol = torch.searchsorted(gptr, torch.arange(int(kbits.numel()), device=dev), right=True) - 1
    return run[1:] - 1, gptr, kcol, kbits


def column_blocks(ncat: torch.Tensor, L: int, budget: int) -> List[Tuple[int, int]]:
    """Column ranges ``(c0, c1)`` whose count tables ``[categories, L]`` uint32 stay under ``budget`` bytes; a block
    holds at least one column, even one that exceeds the budget alone.  ``ncat`` int64 [c]: categories per column
    (an upper bound will do)."""
    c = int(ncat.numel())
    cap = max(1, int(budget) // (4 * int(L)))
    cum = torch.cumsum(ncat.to(torch.int64), 0).cpu()
    out, c0, done = [], 0, 0
    while c0 < c:
        c1 = int(torch.searchsorted(cum, torch.tensor(done + cap), right=True))
        c1 = min(max(c1, c0 + 1), c)
        out.append((c0, c1))
        done = int(cum[c1 - 1])
        c0 = c1
    return out
