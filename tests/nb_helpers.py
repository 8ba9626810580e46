"""The fp64 numpy oracle and the case generators of the naive Bayes prediction tests (``ops/naive_bayes.py``,
``ops/csrc/naive_bayes.hip``).

The model operand is a table ``M`` [L, d] and offsets ``pi``, ``phi`` [L] (``phi = 0`` for Multinomial); the score of
class c is ``s_c = pi[c] + phi[c] + x . M[c, :]``, ``pred`` the first strict maximum (NaN never wins, -1 when no score
is above -inf) and ``prob_c = exp(s_c - lse)``, ``lse = m + log sum_c exp(s_c - m)``, m the row maximum.

Bounds, derived here and not tuned (``U = 2^-53``, 4x the project's margin):

* score: a dot of T products accumulated in any order and by fma or not, plus the two offset additions, is T + 2
  roundings at most, each relative U of a partial sum that ``A = sum|v M| + |pi| + |phi|`` bounds:
  ``|ds| <= (T + 2) U A`` to first order, for the kernel and for this oracle alike; ``E = 4 (T + 2) U A``.  T is the
  number of stored entries inside ``[0, d)`` for CSR rows and d for dense rows.
* probability: ``log p_c = s_c - lse``.  ``m`` is exact for given scores; each ``exp(s_c - m)`` has a relative error
  ``|ds_c| + |dm| <= 2 E_max`` from its argument plus 2 U from the subtraction and the exp; the sum of L such
  positive terms adds L U; the log, the addition ``m + log`` and the final subtraction and exp add a few U relative
  and ``U (|lse| + |s_c - lse|)`` through the rounding of ``lse`` and of ``s_c - lse``.  Together
  ``|dp| / p <= 2 E_max + (L + 8) U + U (|lse| + |s_c - lse|)``, times 4.

Conditions the generators keep and ``reference`` asserts: the gap between the top two distinct scores of a row exceeds
``2 E`` (so rounding cannot change the winner; the bit-identical twin classes are the deliberate exception), and every
finite-score class has ``p >= 1e-200`` (no denormal probabilities).

Every case holds, as far as its L allows: two bit-identical classes (L >= 2) that win a good share of the rows and must
go to the lower index; a class (L >= 3) whose table row holds a -inf, so that its score is -inf on the rows that touch
that column and which must never win; one row whose scores are all -inf, which must give ``pred = -1`` (its ``prob``
is not checked).  On dense rows a zero against the -inf gives a NaN score, which must not win either; the ``prob`` of
such a row is not checked (non-finite inputs are not guaranteed beyond this).
"""
import numpy as np

U = 2.0 ** -53
NCOLS = 1 << 18


def special_classes(L):
    """(a, b, c0): the twin classes a < b and the class with a -inf in its table row; None where L has no room."""
    if L < 2:
        return None, None, None
    if L == 2:
        return 0, 1, None
    return max(1, L // 3), L - 1, 0


def make_table(L, d, rng, j0, j1=None):
    """(M [L, d], pi, phi): negative log-probability-like entries, a common column profile plus small class terms (so
    the classes' scores stay within a few units of each other), the twins, -inf at (c0, j0) and, with ``j1``, a column
    of -inf on every class."""
    base = -(1.0 + 3.0 * rng.random(d))
    M = base[None, :] + 0.05 * rng.standard_normal((L, d))
    pi = -1.0 - rng.random(L)
    phi = -0.5 * rng.random(L)
    a, b, c0 = special_classes(L)
    if a is not None:
        pi[a] += 0.5
        M[b], pi[b], phi[b] = M[a], pi[a], phi[a]
    if c0 is not None:
        M[c0, j0] = -np.inf
    if j1 is not None:
        M[:, j1] = -np.inf
    return M, pi, phi


def reference(S, A, T, L):
    """The oracle's outputs from the scores S [n, L], the magnitudes A [n, L] and the term counts T [n]:
    dict(S, E, pred, prob, ptol, prob_rows); asserts the generators' conditions."""
    n = S.shape[0]
    E = 4.0 * (T[:, None] + 2) * U * A
    Sf = np.where(np.isnan(S), -np.inf, S)
    pred = Sf.argmax(1).astype(np.int64)
    top = Sf[np.arange(n), pred]
    pred[top == -np.inf] = -1
    finite = np.isfinite(S)
    Emax = np.where(finite, E, 0.0).max(1)
    for r in range(n):
        vals = np.unique(Sf[r][np.isfinite(Sf[r])])
        if len(vals) >= 2:
            assert vals[-1] - vals[-2] > 2.0 * Emax[r], ("gap condition", r, vals[-1] - vals[-2], Emax[r])
    prob_rows = ~np.isnan(S).any(1) & finite.any(1)
    with np.errstate(all="ignore"):
        lse = top + np.log(np.exp(S - top[:, None]).sum(1))
        prob = np.exp(S - lse[:, None])
        ptol = 4.0 * (2.0 * Emax[:, None] + (L + 8) * U + U * (np.abs(lse)[:, None] + np.abs(S - lse[:, None])))
    ptol = np.where(finite, ptol, 0.0)
    assert (prob[prob_rows][finite[prob_rows]] >= 1e-200).all(), "denormal probability condition"
    return {"S": S, "E": E, "pred": pred, "prob": prob, "ptol": ptol, "prob_rows": prob_rows}


def check(ref, pred, prob=None):
    """``pred`` exactly; ``prob`` within ``ptol`` relative on the rows whose scores hold no NaN and one finite value."""
    pred = np.asarray(pred)
    assert pred.dtype == np.int32 and pred.shape == ref["pred"].shape
    bad = np.nonzero(pred != ref["pred"])[0]
    assert bad.size == 0, ("pred", bad[:5], pred[bad[:5]], ref["pred"][bad[:5]])
    if prob is None:
        return
    prob = np.asarray(prob)
    rows = ref["prob_rows"]
    want, tol = ref["prob"][rows], ref["ptol"][rows]
    err = np.abs(prob[rows] - want)
    over = err > tol * want
    assert not over.any(), ("prob", np.argwhere(over)[:5], (err / np.maximum(want, 1e-300)).max(), tol.max())


# ------------------------------------------------------------------------------------------------------ CSR rows

def csr_case(L, d, bernoulli, n=200, seed=0, ncols=None, max_entries=130):
    """CSR rows under ``ncols >= d`` columns against a model of d columns: empty rows, rows of 1 .. ``max_entries``
    entries in random stored order, entries at -1, d and d + 7 (they add nothing and are never checked for 0 / 1).
    Returns dict(crow, col int64, val, ncols, d, L, M, pi, phi, off, bernoulli, ref)."""
    rng = np.random.default_rng(1000 * L + 7 * (d % 1009) + 2 * seed + int(bernoulli))
    ncols = d + 64 if ncols is None else ncols
    j0, j1 = 3 % d, d - 1
    M, pi, phi = make_table(L, d, rng, j0, j1)
    if not bernoulli:
        phi[:] = 0.0
    cols, vals = [], []
    for r in range(n):
        m = 0 if r % 17 == 5 else int(rng.integers(1, max_entries + 1))
        if r == 0:
            m = max_entries
        if r == 1:
            m = 1
        c = rng.choice(d - 1, size=min(m, d - 1), replace=False).astype(np.int64)     # never j1 = d - 1
        v = np.ones(len(c)) if bernoulli else 0.5 + 2.5 * rng.random(len(c))
        if bernoulli and len(c) > 2:
            v[0], v[1] = 0.0, -0.0
        if r % 5 == 2 and len(c):       # entries outside the model, anywhere in the stored order
            out = np.array([-1, d, d + 7], dtype=np.int64)
            pos = rng.permutation(len(c) + 3)
            c = np.concatenate([c, out])[pos]
            v = np.concatenate([v, [2.0, 0.5, 3.0]])[pos]
        if r % 4 == 1 and j0 not in c and len(c):       # rows that touch the -inf of class c0
            c[0], v[0] = j0, 1.0
        cols.append(c)
        vals.append(v)
    rinf = n // 2
    cols[rinf] = np.concatenate([cols[rinf][cols[rinf] != j0][:3], [j1]]).astype(np.int64)      # the all -inf row
    vals[rinf] = np.ones(len(cols[rinf]))
    crow = np.zeros(n + 1, dtype=np.int64)
    crow[1:] = np.cumsum([len(c) for c in cols])
    col, val = np.concatenate(cols), np.concatenate(vals)
    off = pi + phi
    S = np.empty((n, L))
    A = np.empty((n, L))
    T = np.empty(n)
    with np.errstate(all="ignore"):
        for r in range(n):
            c, v = cols[r], vals[r]
            ok = (c >= 0) & (c < d)
            prod = v[ok][None, :] * M[:, c[ok]]
            S[r] = off + prod.sum(1)
            A[r] = np.nan_to_num(np.abs(prod), nan=0.0, posinf=0.0).sum(1) + np.abs(pi) + np.abs(phi)
            T[r] = ok.sum()
    assert np.isneginf(S[rinf]).all()
    return {"crow": crow, "col": col, "val": val, "ncols": ncols, "d": d, "L": L, "M": M, "pi": pi, "phi": phi,
            "off": off, "bernoulli": bernoulli, "ref": reference(S, A, T, L)}


def csr_rows(case, device="cpu", idx_dtype=None):
    """The case's rows as ``ops.naive_bayes.predict_rows`` makes them (the model narrower than the rows)."""
    import torch
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import naive_bayes as nb
    fm = FeatureMatrix(crow=torch.from_numpy(case["crow"]).to(device),
                       col=torch.from_numpy(case["col"]).to(device, idx_dtype or torch.int64),
                       val=torch.from_numpy(case["val"]).to(device), ncols=case["ncols"])
    return nb.predict_rows(fm, case["d"])


# ------------------------------------------------------------------------------------------------------ dense rows

def dense_case(d, L, bernoulli, n=200, seed=0):
    """Dense fp64 rows [n, d].  Column j0 = 0 meets the -inf of class c0: positive on most rows (score -inf), zero on
    a few (score NaN).  The all -inf row holds a +inf in column d - 1, against a table that is negative there.
    Returns dict(X, d, L, M, pi, phi, off, bernoulli, ref)."""
    rng = np.random.default_rng(1000 * L + d + 2 * seed + int(bernoulli))
    j0 = 0
    M, pi, phi = make_table(L, d, rng, j0)
    if not bernoulli:
        phi[:] = 0.0
    if bernoulli:
        X = (rng.random((n, d)) < 0.5).astype(np.float64)
        X = np.where((rng.random((n, d)) < 0.1) & (X == 0.0), -0.0, X)      # -0.0 passes the 0 / 1 rule
    else:
        X = np.floor(4.0 * rng.random((n, d))) * (rng.random((n, d)) < 0.7) + 0.25 * rng.random((n, d))
    _, _, c0 = special_classes(L)
    if c0 is not None:
        X[:, j0] = 1.0
        X[np.arange(n) % 9 == 4, j0] = 0.0
    rinf = n // 2
    X[rinf, d - 1] = np.inf
    off = pi + phi
    with np.errstate(all="ignore"):
        prod = X[:, None, :] * M[None, :, :] if n * L * d <= (1 << 24) else None
        if prod is not None:
            S = off[None, :] + prod.sum(2)
            A = np.nan_to_num(np.abs(prod), nan=0.0, posinf=0.0).sum(2)
        else:
            S = off[None, :] + X @ M.T
            A = np.nan_to_num(np.abs(X), posinf=0.0) @ np.nan_to_num(np.abs(M), posinf=0.0).T
    A = A + (np.abs(pi) + np.abs(phi))[None, :]
    assert (np.isnan(S[rinf]) | np.isneginf(S[rinf])).all()
    return {"X": X, "d": d, "L": L, "M": M, "pi": pi, "phi": phi, "off": off, "bernoulli": bernoulli,
            "ref": reference(S, A, np.full(n, float(d)), L)}


def dense_rows(case, device="cpu", unaligned=False):
    """The case's rows as a rows object; ``unaligned``: a contiguous view that starts 8 bytes into its allocation."""
    import torch
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import naive_bayes as nb
    X = torch.from_numpy(case["X"]).to(device)
    if unaligned:
        flat = torch.empty(X.numel() + 1, dtype=torch.float64, device=device)
        Xo = flat[1:].view(X.shape)
        Xo.copy_(X)
        assert Xo.data_ptr() % 16 == 8 and Xo.is_contiguous()
        X = Xo
    return nb.predict_rows(FeatureMatrix(X), case["d"])


# ------------------------------------------------------------------------------------------------------ operators

def count_docs(n=400, L=3, seed=0, size=NCOLS, vocab=60, bernoulli=False):
    """Documents of integer counts (0 / 1 values for Bernoulli) over ``vocab`` columns spread through ``size``:
    (crow, col int64 sorted inside a row, val, label int64 [n], the columns used)."""
    rng = np.random.default_rng(seed)
    used = np.sort(rng.choice(size, vocab, replace=False)).astype(np.int64)
    label = rng.integers(0, L, n)
    cols, vals = [], []
    for r in range(n):
        lo = (label[r] * vocab) // (2 * L)
        pick = np.sort(rng.choice(np.arange(lo, lo + vocab // 2), size=int(rng.integers(3, 12)), replace=False))
        cols.append(used[pick])
        vals.append(np.ones(len(pick)) if bernoulli else rng.integers(1, 5, len(pick)).astype(np.float64))
    crow = np.zeros(n + 1, dtype=np.int64)
    crow[1:] = np.cumsum([len(c) for c in cols])
    return crow, np.concatenate(cols), np.concatenate(vals), label.astype(np.int64), used


def sparse_table(crow, col, val, size, label, device="cpu", weight=None):
    import torch
    from alink_amd.common.linalg.block import SparseBlock
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    blk = SparseBlock(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), int(size)).to(device)
    names, types, cols = ["v", "label"], [Types.SPARSE_VECTOR, Types.LONG], [Column(blk),
                                                                             Column(torch.from_numpy(label))]
    if weight is not None:
        names, types, cols = names + ["w"], types + [Types.DOUBLE], cols + [Column(torch.from_numpy(weight))]
    return MTable(TableSchema(names, types), cols)


def dense_table(X, label, device="cpu"):
    import torch
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    return MTable(TableSchema(["v", "label"], [Types.DENSE_VECTOR, Types.LONG]),
                  [Column(torch.from_numpy(X).to(device)), Column(torch.from_numpy(label))])
