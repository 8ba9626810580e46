"""Generators and oracles of the chi-square tests (tests/test_chisq_device.py on the CPU through the torch twins,
tests/test_chisq_gpu.py through the kernels).

The oracles know nothing of streams: a column is a list of (canonical bits, label) pairs; its cross table comes from
``np.unique`` and ``np.add.at``, its statistic from the terms ``E = rs * cs / n``, ``t = O - E``, ``t * t / E`` in numpy
fp64, summed with ``math.fsum``."""
import math
import struct

import numpy as np

NAN_BITS = 0x7FF8000000000000
NAN_A = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000001))[0]       # two NaNs of different payload
NAN_B = struct.unpack("<d", struct.pack("<Q", 0xFFF0000000000123))[0]


def bits_of(x: np.ndarray) -> np.ndarray:
    """Canonical int64 bit patterns of float64 values: every NaN one pattern, -0.0 and +0.0 apart."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.int64).copy()
    b[np.isnan(x)] = NAN_BITS
    return b


def table_oracle(bits: np.ndarray, lab: np.ndarray, L: int):
    """``(keys int64 [R] ascending, cnt int64 [R, L])`` of one column's (bits, label) pairs."""
    keys, inv = np.unique(np.asarray(bits, dtype=np.int64), return_inverse=True)
    cnt = np.zeros((len(keys), L), dtype=np.int64)
    np.add.at(cnt, (inv.reshape(-1), np.asarray(lab, dtype=np.int64)), 1)
    return keys, cnt


def stat_oracle(cnt: np.ndarray):
    """``(value, R, Lc, df, T)`` of a cross table of integer counts: rows with a row sum > 0, columns with a column
    sum > 0, every cell of those a term; T = R * Lc cells."""
    cnt = np.asarray(cnt, dtype=np.int64)
    cnt = cnt[cnt.sum(1) > 0][:, cnt.sum(0) > 0] if cnt.size else cnt.reshape(0, 0)
    R, Lc = (int(cnt.shape[0]), int(cnt.shape[1])) if cnt.size else (0, 0)
    if R == 0:
        return 0.0, 0, 0, 0, 0
    rs, cs = cnt.sum(1).astype(np.float64), cnt.sum(0).astype(np.float64)
    n = float(cnt.sum())
    E = np.outer(rs, cs) / n
    t = cnt.astype(np.float64) - E
    value = math.fsum((t * t / E).ravel().tolist())
    df = (R - 1) * (Lc - 1) if R > 1 and Lc > 1 else 0
    return value, R, Lc, df, R * Lc


def dense_columns(X: np.ndarray, lab: np.ndarray):
    """Per column of dense rows, the (bits, label) pairs of the rows whose label is >= 0."""
    ok = lab >= 0
    return [(bits_of(X[ok, j]), lab[ok]) for j in range(X.shape[1])]


def csr_columns(crow, col, val, lab, d):
    """Per column of CSR rows, the (bits, label) pairs: the stored entries that are not +0.0, and +0.0 for every
    other participating row (the implicit zero category)."""
    n = len(crow) - 1
    row = np.repeat(np.arange(n), np.diff(crow))
    b = bits_of(val)
    out = []
    for j in range(d):
        m = (col == j) & (b != 0) & (lab[row] >= 0)
        rest = np.ones(n, dtype=bool)
        rest[row[m]] = False
        rest &= lab >= 0
        out.append((np.concatenate([b[m], np.zeros(int(rest.sum()), dtype=np.int64)]),
                    np.concatenate([lab[row[m]], lab[rest]])))
    return out


def random_dense(seed, n, d, L, distinct=5, null_labels=True):
    """Dense rows with ``distinct`` values per column (so categories have runs) and labels in [0, L), some -1."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, distinct, size=(n, d)).astype(np.float64) * 0.5 - 1.0
    lab = rng.integers(0, L, size=n).astype(np.int32)
    if null_labels and n > 4:
        lab[rng.integers(0, n, size=max(1, n // 17))] = -1
    return X, lab


def special_csr(n=4097, L=3, seed=5):
    """CSR rows over 6 columns that hold the edge cases: 0 one value in every row (one run over many chunks, no
    implicit zero), 1 ``n`` distinct values, 2 no stored entry, 3 a stored +0.0, a -0.0 and two NaNs of different
    payload among 2.0s, 4 random sparse counts, 5 one of two values in every row; index 9 >= d is dropped."""
    rng = np.random.default_rng(seed)
    d = 6
    rows, cols, vals = [], [], []

    def put(r, c, v):
        rows.append(r), cols.append(c), vals.append(v)

    for r in range(n):
        put(r, 0, 1.0)
        put(r, 1, float(r + 1) * 0.25)
        if r % 5 == 0:
            put(r, 3, [0.0, -0.0, NAN_A, NAN_B, 2.0][(r // 5) % 5])
        if rng.random() < 0.3:
            put(r, 4, float(rng.integers(1, 4)))
        if r % 97 == 0:
            put(r, 9, 3.0)
        put(r, 5, 1.0 if (r * 7 + r // 3) % 2 else 2.0)
    rows, cols, vals = np.array(rows), np.array(cols, dtype=np.int64), np.array(vals, dtype=np.float64)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=crow[1:])
    lab = rng.integers(0, L, size=n).astype(np.int32)
    lab[::53] = -1
    return crow, cols, vals, lab, d


def balanced_column(n_cat=7, L=4, reps=3):
    """A column independent of the label by construction: every category holds every label ``reps`` times."""
    x = np.repeat(np.arange(n_cat, dtype=np.float64), L * reps)
    lab = np.tile(np.repeat(np.arange(L, dtype=np.int32), reps), n_cat)
    return x.reshape(-1, 1), lab


def rel_bound(T: int) -> float:
    """``|value - ref| <= T * 2**-52 * ref``: any order of adding T non-negative, identically computed terms is within
    (T - 1) * 2**-53 relative of the exact sum, fsum within 2**-53; that total, doubled."""
    return T * 2.0 ** -52


# ---------------------------------------------------------------------------------------------------
# checks shared by the CPU tests (twins) and the GPU tests (kernels): ``backend`` is ops.chisq.TWIN or DEVICE
# ---------------------------------------------------------------------------------------------------
def check_value(value, ref, T):
    assert abs(value - ref) <= rel_bound(T) * ref, (value, ref, T, abs(value - ref) / max(ref, 1e-300))


def check_columns(columns, L, value, R, Lc):
    """The statistic arrays of a run against the oracle of every column's (bits, label) pairs."""
    for j, (b, lab) in enumerate(columns):
        ref, r, lc, _, T = stat_oracle(table_oracle(b, lab, L)[1])
        assert (int(R[j]), int(Lc[j])) == (r, lc), (j, int(R[j]), int(Lc[j]), r, lc)
        check_value(float(value[j]), ref, T)


def check_dense_shape(backend, dev, n, d, L, grids=(0, 1, 3)):
    """Counts (exact) and statistic (bounded, bitwise equal across grids) of random dense rows at one shape."""
    import torch
    from alink_amd.ops import chisq as Q
    X, lab = random_dense(n * 1000 + d * 10 + L, n, d, L)
    colptr, bits, slab = Q.dense_stream(torch.from_numpy(X).to(dev), torch.from_numpy(lab).to(dev))
    cat, gptr, kcol, kbits = Q.categories(colptr, bits)
    G = int(gptr[-1])
    g = cat.to(torch.int32).contiguous()
    columns = dense_columns(X, lab)
    want = np.concatenate([table_oracle(b, l, L)[1] for b, l in columns]) if G else np.zeros((0, L), dtype=np.int64)
    tables, values = [], []
    for grid in grids:
        cnt = Q.u32(backend.counts(g, slab, G, L, grid=grid))
        assert np.array_equal(cnt.cpu().numpy(), want), (n, d, L, grid)
        tables.append(cnt)
        col_of = torch.searchsorted(gptr, torch.arange(G, device=dev), right=True) - 1
        cs = torch.zeros((d, L), dtype=torch.int64, device=dev).index_add_(0, col_of, cnt)
        value, R, Lc = backend.stat(cnt.contiguous(), gptr, cs, None, grid=grid)
        check_columns(columns, L, value.cpu().numpy(), R.cpu().numpy(), Lc.cpu().numpy())
        values.append(value.cpu().numpy())
    for other in (backend.counts(g, slab, G, L, chunk=64, grid=2), backend.counts(g, slab, G, L, variant=1)):
        assert np.array_equal(Q.u32(other).cpu().numpy(), want)
    for v in values[1:]:
        assert np.array_equal(v.view(np.int64), values[0].view(np.int64))


def run_special(backend, dev, budget=None, grid=0, L=3):
    """The edge-case CSR rows through the block loop: ``(columns, value, R, Lc, tables, blocks)``."""
    import torch
    from alink_amd.models.statistics import chisq as CQ
    from alink_amd.ops import chisq as Q
    crow, col, val, lab, d = special_csr(L=L)
    t = lambda a: torch.from_numpy(a).to(dev)           # noqa: E731
    colptr, bits, slab = Q.csr_stream(t(crow), t(col), t(val), t(lab), d)
    ntot = torch.from_numpy(np.bincount(lab[lab >= 0], minlength=L).astype(np.int64)).to(dev)
    tables, stats = [], {}
    value, R, Lc = CQ.chi_square_stream(colptr, bits, slab, L, ntot, backend, budget=budget, grid=grid, stats=stats,
                                        tables=tables)
    return (csr_columns(crow, col, val, lab, d), value.cpu().numpy(), R.cpu().numpy(), Lc.cpu().numpy(), tables,
            stats["blocks"])


def special_tables(tables, d, L):
    """Per column, the count table a run produced: its stored categories, then the zero row."""
    out = [None] * d
    for c0, gp, cnt, zero in tables:
        gp, cnt, zero = gp.cpu().numpy(), cnt.cpu().numpy(), zero.cpu().numpy()
        for k in range(len(gp) - 1):
            out[c0 + k] = np.concatenate([cnt[gp[k]:gp[k + 1]], zero[k:k + 1]])
    return out


def check_special(backend, dev):
    """Every edge case, every budget and grid: exact tables, bounded values, bitwise equal values."""
    L, d = 3, 6
    runs = [run_special(backend, dev), run_special(backend, dev, budget=4 * L, grid=1),
            run_special(backend, dev, budget=4 * L * 6, grid=3), run_special(backend, dev)]
    columns = runs[0][0]
    assert runs[0][5] == 1 and runs[1][5] == d and 1 < runs[2][5] < d   # one block; one per column; borders between
    for _, value, R, Lc, tables, _ in runs:
        check_columns(columns, L, value, R, Lc)
        got = special_tables(tables, d, L)
        for j, (b, lab) in enumerate(columns):
            keys, cnt = table_oracle(b, lab, L)
            # the oracle's zero category (bits 0) comes first when -0.0 or NaN follow it in int64 order; the run's
            # zero row comes last: compare as multisets of rows keyed by the category
            z = cnt[keys == 0] if (keys == 0).any() else np.zeros((1, L), dtype=np.int64)
            assert np.array_equal(got[j][:-1], cnt[keys != 0]), j
            assert np.array_equal(got[j][-1:], z), j
        assert np.array_equal(value.view(np.int64), runs[0][1].view(np.int64))
    R = runs[0][2]
    assert R[0] == 1 and R[1] == 4097 - len(range(0, 4097, 53)) and R[2] == 1 and R[5] == 2
    assert R[3] == 4                                            # -0.0, NaN, 2.0 and the zeros (stored +0.0 among them)
