"""Chi-square tests of table columns or of a vector column against a label, on the sorted entry streams and the two
primitives of ``ops/chisq.py``.  ``summary.chi_square_test`` stays the CPU path and the oracle; this module returns
``None`` wherever a column cannot be coded exactly, and the operator then takes that path.

Rows never leave their rank: per column block every rank's distinct (column, bits) keys are gathered and merged, each
rank counts its entries into the merged table, and one integer all-reduce follows."""
from __future__ import annotations

import time
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ...common.linalg import DenseVector, SparseBlock, SparseVector, VectorUtil
from ...common.strings import StringBlock
from ...common.table import MTable
from ...ops import chisq as Q
from ...ops import strings as S
from ...parallel import comm

__all__ = ["chi_square_arrays", "chi_square_stream", "p_values", "global_cells"]

_SORT_ELEMS = 2 ** 27           # elements of a dense column chunk sorted at once


def p_values(value: np.ndarray, df: np.ndarray) -> np.ndarray:
    """One vectorised ``scipy.stats.chi2.sf`` over the columns (the function the host path uses); ``df == 0`` maps
    to 1."""
    from scipy.stats import chi2
    p = np.ones(value.shape, dtype=np.float64)
    m = df > 0
    if m.any():
        p[m] = chi2.sf(value[m], df[m])
    return p


class _Clock:
    """Per-stage seconds into ``stats`` (a dict) when one is given; synchronises the device only then."""

    def __init__(self, stats, dev):
        self.stats, self.dev = stats, dev
        self.t = time.perf_counter() if stats is not None else 0.0

    def restart(self) -> None:
        """Forget the time since the last lap (someone else has accounted for it)."""
        if self.stats is not None:
            self.t = time.perf_counter()

    def lap(self, stage: str) -> None:
        if self.stats is None:
            return
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        now = time.perf_counter()
        self.stats[stage] = self.stats.get(stage, 0.0) + now - self.t
        self.t = now


def chi_square_stream(colptr: torch.Tensor, bits: torch.Tensor, lab: torch.Tensor, L: int,
                      ntot: Optional[torch.Tensor], backend: Q.Backend, budget: Optional[int] = None, grid: int = 0,
                      stats: Optional[dict] = None, tables: Optional[list] = None):
    """``(value float64 [c], R int64 [c], Lc int64 [c])`` of the ``c`` columns of this rank's sorted entry stream,
    block by block on ``backend``.  ``ntot`` int64 [L] (the participating rows per label over all ranks) gives every
    column the implicit zero row ``ntot - column sums``; None: no such row.  ``budget`` (bytes of a block's count
    table) and ``grid`` change no result.  ``tables`` (a list) receives ``(c0, gptr, cnt, zero)`` of every block, after
    the ranks' sum."""
    dev = bits.device
    budget = Q.CHISQ_BUDGET_BYTES if budget is None else int(budget)
    L = int(L)
    c = int(colptr.numel()) - 1
    clock = _Clock(stats, dev)
    cat, gptr, kcol, kbits = Q.categories(colptr, bits)
    many = comm.get_world_size() > 1
    ncat = gptr[1:] - gptr[:-1]
    if many:
        ncat = comm.all_reduce(ncat.clone(), "sum")             # an upper bound of the merged count; same on all ranks
    blocks = Q.column_blocks(ncat, L, budget)
    clock.lap("coding")
    value = torch.zeros(c, dtype=torch.float64, device=dev)
    R = torch.zeros(c, dtype=torch.int64, device=dev)
    Lc = torch.zeros(c, dtype=torch.int64, device=dev)
    for c0, c1 in blocks:
        e0, e1 = int(colptr[c0]), int(colptr[c1])
        a, b = int(gptr[c0]), int(gptr[c1])
        if many:
            mine = torch.stack([kcol[a:b], kbits[a:b]], 1).cpu()
            parts = comm.all_gather_object(mine.numpy())        # keys, never rows
            allk = torch.from_numpy(np.concatenate(parts, 0))
            merged, inv = torch.unique(allk, dim=0, return_inverse=True)
            off = sum(int(p.shape[0]) for p in parts[:comm.get_rank()])
            gmap = inv[off:off + (b - a)].to(dev)
            g = gmap[cat[e0:e1] - a].to(torch.int32).contiguous() if e1 > e0 else \
                torch.zeros(0, dtype=torch.int32, device=dev)
            G = int(merged.shape[0])
            gp = torch.searchsorted(merged[:, 0].contiguous(), torch.arange(c0, c1 + 1)).to(dev)
        else:
            g = (cat[e0:e1] - a).to(torch.int32).contiguous()
            G = b - a
            gp = (gptr[c0:c1 + 1] - a).contiguous()
        clock.lap("coding")
        cnt = Q.u32(backend.counts(g, lab[e0:e1].contiguous(), G, L, grid=grid))
        clock.lap("counts")
        if many:
            comm.all_reduce(cnt, "sum")
        col_of = torch.searchsorted(gp, torch.arange(G, device=dev), right=True) - 1
        # exact integer sums; a running sum over the categories and differences at the column borders was tried and
        # dropped: torch's scan along the rows of [2.7e7, 20] int64 took 10 s a block on the MI355X against 0.07 s
        # for this add
        colsum = torch.zeros((c1 - c0, L), dtype=torch.int64, device=dev).index_add_(0, col_of, cnt)
        zero = None
        if ntot is not None:
            zero = (ntot.to(dev)[None, :] - colsum).contiguous()
            if bool((zero < 0).any()):
                raise ValueError("chi_square_stream: a column holds more entries of a label than rows")
            colsum = colsum + zero
        clock.lap("column_sums")
        if tables is not None:
            tables.append((c0, gp, cnt, zero))
        v, r, lc = backend.stat(cnt.contiguous(), gp, colsum.contiguous(), zero, grid=grid)
        value[c0:c1], R[c0:c1], Lc[c0:c1] = v, r.to(torch.int64), lc.to(torch.int64)
        clock.lap("stat")
    if stats is not None:
        stats["blocks"] = stats.get("blocks", 0) + len(blocks)
        stats["entries"] = stats.get("entries", 0) + int(bits.numel())
        stats["categories"] = stats.get("categories", 0) + int(gptr[-1])
    return value, R, Lc


# ---------------------------------------------------------------------------------------------------
# coding of labels and columns
# ---------------------------------------------------------------------------------------------------
def _tensor_codes(v: torch.Tensor) -> torch.Tensor:
    """Exact int64 codes of a numeric or boolean tensor column: distinct codes and distinct ``str(value)`` are the
    same partition once NaN is canonical."""
    return Q.canon_bits(v) if v.dtype.is_floating_point else v.to(torch.int64)


def _code_names(codes: torch.Tensor, dtype: torch.dtype) -> List[str]:
    if dtype.is_floating_point:
        vals = codes.cpu().view(torch.float64).to(torch.float64).tolist()
    elif dtype == torch.bool:
        vals = codes.cpu().to(torch.bool).tolist()
    else:
        vals = codes.cpu().tolist()
    return [str(x) for x in vals]


def _label_codes(mt: MTable, label_col: str, dev) -> Tuple[torch.Tensor, List[str]]:
    """``(lab_row int32 [n], names)``: the code of every row's label among the distinct ``str(label)`` over all
    ranks, ordered by string; -1 for a null label."""
    c = mt.col(label_col)
    v = c.values
    if isinstance(v, torch.Tensor) and v.dim() == 1:
        key = _tensor_codes(v.to(dev))
        ok = torch.ones_like(key, dtype=torch.bool) if c.nulls is None else ~c.nulls.to(dev)
        uniq, inv = torch.unique(key[ok], return_inverse=True)
        local = _code_names(uniq, v.dtype)
        local_id = torch.full(key.shape, -1, dtype=torch.int64, device=dev)
        local_id[ok] = inv
    else:
        vals = c.to_list()
        seen = {}
        ids = [-1 if x is None else seen.setdefault(str(x), len(seen)) for x in vals]
        local = list(seen)
        local_id = torch.tensor(ids, dtype=torch.int64, device=dev)
    names = sorted(set().union(*[set(x) for x in comm.all_gather_object(local)]))
    where = {s: i for i, s in enumerate(names)}
    table = torch.tensor([where[s] for s in local] + [-1], dtype=torch.int64, device=dev)
    return table[local_id].to(torch.int32), names           # local_id -1 reads the trailing -1


def _string_codes(block: StringBlock, dev):
    """``(codes int64 [n], valid bool [n])`` of a string column by the exact dictionary ids of ``ops/strings``, made
    the same on every rank through the distinct strings; None on a hash collision."""
    block = block.to(dev)
    n = len(block)
    valid = ~block.null_mask().to(dev) if block.nulls is not None else torch.ones(n, dtype=torch.bool, device=dev)
    rows = torch.nonzero(valid).reshape(-1)
    got = S.unique_ids(block if int(rows.numel()) == n else block.take(rows))     # a null hashes like ""
    if got is None:
        ok = False
        mine = []
    else:
        ok = True
        ids, rep = got
        mine = (block if int(rows.numel()) == n else block.take(rows)).take(rep).to_list() if int(rep.numel()) else []
    # the ids follow the hash; the distinct strings (never the rows) put them in string order, the same on every rank
    # and for every split of the rows
    parts = comm.all_gather_object((ok, mine))
    if not all(p[0] for p in parts):
        return None
    names = sorted(set().union(*[set(p[1]) for p in parts]))
    where = {s: i for i, s in enumerate(names)}
    codes = torch.full((n,), -1, dtype=torch.int64, device=dev)
    if mine:
        codes[rows] = torch.tensor([where[s] for s in mine], dtype=torch.int64, device=dev)[ids.to(dev)]
    return codes, valid


def _column_kind(mt: MTable, name: str) -> Optional[str]:
    """How a table column can be coded exactly, judged without communication: ``"tensor"`` (numeric or boolean value
    bits), ``"string"`` (dictionary ids) or None (the host path)."""
    v = mt.col(name).values
    if isinstance(v, torch.Tensor) and v.dim() == 1:
        return "tensor"
    if isinstance(v, StringBlock) or (isinstance(v, list) and all(x is None or isinstance(x, str) for x in v)):
        return "string"
    return None


def _column_codes(mt: MTable, name: str, kind: str, dev):
    """``(codes, valid)`` of a column of ``_column_kind`` ``kind``; a string column is a collective, so every rank
    calls this for the same columns in the same order.  None on a hash collision (agreed among the ranks)."""
    c = mt.col(name)
    v = c.values
    if kind == "tensor":
        return _tensor_codes(v.to(dev)), (None if c.nulls is None else ~c.nulls.to(dev))
    return _string_codes(v if isinstance(v, StringBlock) else StringBlock.from_list(v), dev)


def parse_vectors(mt: MTable, vector_col: str):
    """The vectors of a list-typed vector column, parsed once (None for a null row); None for a column that is
    already a ``SparseBlock`` or a dense tensor block."""
    c = mt.col(vector_col)
    v = c.values
    if isinstance(v, SparseBlock) or (isinstance(v, torch.Tensor) and v.dim() == 2):
        return None
    return [VectorUtil.getVector(x) if x is not None else None for x in (v if isinstance(v, list) else c.to_list())]


def _vector_rows(mt: MTable, vector_col: str, dev, vecs=None):
    """This rank's vector column as ``("csr", (crow, col, val), d, null rows)`` or ``("dense", X, d, null rows)``,
    ``("empty", ...)`` without rows, or None when the rows mix kinds or sizes (the host path pads those) or a CSR row
    stores an index twice (the host path densifies, where one value wins).  ``vecs``: ``parse_vectors`` of the column
    when the caller has it already.

    ``models/common/features.extract_features`` is not used here: it turns a null vector into an all-zero row (such
    a row takes no part in the test), drops the ``-0.0`` entries of dense vectors among sparse ones (a category of
    its own here) and pads rows of different sizes, which the host path keys differently."""
    c = mt.col(vector_col)
    v = c.values
    n = len(c)
    nulls = None if c.nulls is None else c.nulls.to(dev)
    if isinstance(v, SparseBlock):
        csr = (v.crow.to(dev), v.col.to(dev), v.val.to(dev))
        return None if Q.csr_has_duplicates(csr[0], csr[1]) else ("csr", csr, int(v.size), nulls)
    if isinstance(v, torch.Tensor) and v.dim() == 2:
        return "dense", v.to(device=dev, dtype=torch.float64), int(v.shape[1]), nulls
    if vecs is None:
        vecs = parse_vectors(mt, vector_col)
    nulls = torch.tensor([x is None for x in vecs], dtype=torch.bool, device=dev)
    live = [x for x in vecs if x is not None]
    if not live:
        return "empty", None, 0, nulls
    if all(isinstance(x, SparseVector) for x in live):
        if any(x.size() < 0 for x in live):
            return None
        counts = np.array([0 if x is None else len(x.indices) for x in vecs], dtype=np.int64)
        crow = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, out=crow[1:])
        col = np.concatenate([np.asarray(x.indices, dtype=np.int64) for x in live])
        val = np.concatenate([np.asarray(x.values, dtype=np.float64) for x in live])
        d = max(x.size() for x in live)
        csr = (torch.from_numpy(crow).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(val).to(dev))
        return None if Q.csr_has_duplicates(csr[0], csr[1]) else ("csr", csr, d, nulls)
    if all(isinstance(x, DenseVector) for x in live) and len({x.size() for x in live}) == 1:
        d = live[0].size()
        X = np.zeros((n, d), dtype=np.float64)
        for i, x in enumerate(vecs):
            if x is not None:
                X[i] = x.data
        return "dense", torch.from_numpy(X).to(dev), d, nulls
    return None


def global_cells(mt: MTable, selected_cols: Optional[Sequence[str]], vector_col: Optional[str], vecs=None) -> int:
    """Rows x columns over all ranks, the size ``ops.chisq.device_selected`` judges.  ``vecs``: ``parse_vectors`` of
    the vector column."""
    if vector_col:
        v = mt.col(vector_col).values
        if isinstance(v, SparseBlock):
            d = int(v.size)
        elif isinstance(v, torch.Tensor) and v.dim() == 2:
            d = int(v.shape[1])
        else:
            vecs = parse_vectors(mt, vector_col) if vecs is None else vecs
            d = max([x.size() for x in vecs if x is not None] + [0])
    else:
        d = len(selected_cols or [])
    got = comm.all_gather_object((int(mt.num_rows), d))
    return sum(x[0] for x in got) * max([x[1] for x in got] + [0])


def chi_square_arrays(mt: MTable, selected_cols: Optional[Sequence[str]], vector_col: Optional[str], label_col: str,
                      backend: Q.Backend, device=None, budget: Optional[int] = None, grid: int = 0,
                      stats: Optional[dict] = None, vecs=None):
    """The chi-square test of every column of ``selected_cols``, or of every coordinate of ``vector_col``, against
    ``label_col``: ``(names, value float64 [c], df float64 [c], p float64 [c])`` as numpy arrays, or None when the
    host path has to be taken (a column type that cannot be coded exactly, vectors of mixed kinds, more than
    ``CHISQ_MAX_LABELS`` labels, 2^31 rows on a rank, a CSR row that stores an index twice).  Every rank takes the same
    decision, and agrees on it before any collective that only some ranks would enter.  ``vecs``: ``parse_vectors`` of
    the vector column when the caller has parsed it already."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    clock = _Clock(stats, dev)
    lab_row, names = _label_codes(mt, label_col, dev)
    L = max(len(names), 1)
    n_local = int(mt.num_rows)
    if vector_col:
        got = _vector_rows(mt, vector_col, dev, vecs)
        coded = None if got is None else (got[0], got[2], n_local)
    else:
        col_kinds = [_column_kind(mt, name) for name in selected_cols]
        coded = None if any(k is None for k in col_kinds) else ("table", len(col_kinds), n_local)
    if coded is not None and (len(names) > Q.CHISQ_MAX_LABELS or n_local >= 2 ** 31):
        coded = None
    everyone = comm.all_gather_object(coded)
    kinds = {x[0] for x in everyone if x is not None and x[0] != "empty"}
    if any(x is None for x in everyone) or len(kinds) > 1:
        return None
    if not vector_col:
        # every rank codes the same columns in the same order: a string column gathers its distinct strings
        got = [_column_codes(mt, name, k, dev) for name, k in zip(selected_cols, col_kinds)]
        if any(x is None for x in got):
            return None
    if vector_col:
        kind = kinds.pop() if kinds else "dense"
        d = max(x[1] for x in everyone)
        if kind == "dense" and any(x[1] != d for x in everyone if x[0] != "empty"):
            return None
        _, data, _, nulls = got
        if nulls is not None:
            lab_row = torch.where(nulls, torch.full_like(lab_row, -1), lab_row)
        out_names = [str(j) for j in range(d)]
        if kind == "csr":
            ntot = torch.bincount(lab_row[lab_row >= 0].to(torch.int64), minlength=L)
            comm.all_reduce(ntot, "sum")
            if data is None:
                z = torch.zeros(0, dtype=torch.int64, device=dev)
                data = (torch.zeros(mt.num_rows + 1, dtype=torch.int64, device=dev), z, z.to(torch.float64))
            colptr, bits, lab = Q.csr_stream(*data, lab_row, d)
            clock.lap("coding")
            res = chi_square_stream(colptr, bits, lab, L, ntot, backend, budget, grid, stats)
        else:
            X = data if data is not None else torch.zeros((0, d), dtype=torch.float64, device=dev)
            # the chunk width comes from the largest share of the rows: every rank cuts the same column ranges, since
            # each chunk's block loop is a sequence of collectives
            step = max(1, _SORT_ELEMS // max(max(x[2] for x in everyone), 1))
            parts = []
            for j0 in range(0, d, step):
                colptr, bits, lab = Q.dense_stream(X[:, j0:j0 + step], lab_row)
                clock.lap("coding")
                parts.append(chi_square_stream(colptr, bits, lab, L, None, backend, budget, grid, stats))
                clock.restart()
            res = tuple(torch.cat([p[i] for p in parts]) if parts else torch.zeros(0, device=dev) for i in range(3))
    else:
        out_names = list(selected_cols)
        colptr, bits, lab = Q.column_stream([x[0] for x in got], [x[1] for x in got], lab_row)
        clock.lap("coding")
        res = chi_square_stream(colptr, bits, lab, L, None, backend, budget, grid, stats)
    value = res[0].cpu().numpy().astype(np.float64)
    R, Lc = res[1].cpu().numpy().astype(np.int64), res[2].cpu().numpy().astype(np.int64)
    df = np.where((R > 1) & (Lc > 1), (R - 1) * (Lc - 1), 0).astype(np.float64)
    clock = _Clock(stats, dev)
    p = p_values(value, df)
    clock.lap("p_values")
    return out_names, value, df, p
