"""Shared by ``test_sos_device.py`` (CPU) and ``test_sos_gpu.py``: seeded rows, the numpy ``longdouble`` oracle of
``SOSImpl`` (the perplexity search and the column products) with its rounding bounds, and the operator calls.

The oracle takes the raw fp64 rows.  ``D_ij = sum_a (x_ia - x_ja)^2`` directly, in ``longdouble`` (u_ld = 2^-64 on
x86, whose own error is 2^-11 of every bound below and is ignored).  The scalar state ``beta, betaMin, betaMax`` is
fp64 with fp64 arithmetic, as in Java; every ``exp`` result is rounded through fp64, so underflow happens where it
does in double; all sums are ``longdouble``.

Bounds (u = 2^-53; first-order error of one fp64 evaluation of the code under test against the exact value; the tests
allow ``MARGIN`` = 4x, the project's margin).  The code under test centres the rows (x0 = x - mean, one rounding of
relative size u per element; an inexact mean moves every row alike and no distance) and forms
``D = max(0, (q_i + q_j) - 2 x0_i . x0_j)`` with ``M2 = max_i |x0_i|^2``:

* dissimilarity: the two norms and the dot are d-term sums in any order, fused or not, of at most ``(d + 1) u M2``
  each (the dot twice), the centring adds ``2 u (|x0_i| + |x0_j|)^2 <= 8 u M2``, the two additions and the
  subtraction ``2 u (q_i + q_j + 2 |dot|) <= 8 u M2``:  ``eD = (4 d + 20) u M2``, the same for every pair;
* affinity ``a = exp(-beta D)``: the exponent moves by ``beta eD`` and by the product's rounding ``u beta D``, and
  ``exp`` is within 1 ulp (2 u): relative ``rho_j = beta eD + (min(beta D_j, 746) + 2) u`` (beyond 746 the affinity
  is zero on both sides);
* ``s = sum_j a_j`` (n - 1 nonnegative terms in any order): relative ``rs = R + n u`` with ``R = sum_j w_j rho_j``,
  ``w_j = a_j / s``;
* ``t = sum_j a_j D_j``: ``|dt| <= sum_j a_j D_j rho_j + eD s + (n + 1) u t``;
* ``err = t (beta / s) + log(s) - log(h)``: with ``H = beta t / s``
  ``|d err| <= sum_j w_j beta D_j rho_j + beta eD + (n + 1) u H + (H + 1) rs + 4 u (H + |log s| + |log h|)``
  (the division, the product, ``log`` within 1 ulp, the two additions).  ``slack`` is MARGIN times this, per row and
  evaluation; it depends on n, d and ``beta eD`` only through the terms above.

A row is FRAGILE if at any evaluation of its search ``| |err| - tol | < slack`` (a branch within rounding of the
threshold) or ``0 < s < 1e-300`` (the sums are subnormal).  On every other row the code under test must take the
oracle's branches, and since the updates of beta are exact fp64 operations, reach its ``beta`` and ``iters`` bit for
bit.  At most ``FRAGILE_CAP`` = 5 % of a case's rows may be fragile; a case over the cap gets another seed.

* ``s`` at the final beta: ``|ds| <= MARGIN rs s``;
* products for GIVEN ``(beta, s)``: a factor ``f_ij = 1 - a_ij / s_i`` moves by ``df_ij = b_ij (rho_ij + u) + u`` with
  ``b = a / s`` (the division and the subtraction), and the product of n - 1 factors by
  ``sum_i df_ij prod_{k != i} f_kj + 2 n u p_j``; the test allows MARGIN times that plus 1e-300 for results below
  the normal range.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -53
MARGIN = 4.0
LD = np.longdouble
TOL = 1.0e-2
MAX_ITER = 100
FRAGILE_CAP = 0.05
P_FLOOR = 1e-300

# (seed, n, d, scale, perplexity, extra): the cases of the issue, checked on the CPU with the oracle alone
CASES = (
    (0, 300, 5, 1.0, 10.0, None),
    (1, 257, 33, 1.0, 30.0, None),
    (3, 200, 16, 0.01, 20.0, None),          # a long doubling phase
    (4, 130, 128, 1.0, 4.5, None),
    (5, 17, 1, 1.0, 3.0, None),
    (6, 65, 7, 1.0, 8.0, "dup"),             # rows 10..13 equal row 9
    (7, 3, 2, 1.0, 1.5, None),
    (9, 200, 8, 1.0, 10.0, "offset"),        # 1e4 added to every value
    (2, 300, 3, 60.0, 5.0, None),            # 70 rows start in the NaN branch
)
ZERO_FRAGILE = CASES[:8]

# the GPU sweep: every d of D_ALL and every n of N_ALL at least once, perplexity below (n - 1) / 3
D_ALL = (1, 3, 16, 17, 31, 32, 33, 64, 65, 127, 128, 129, 1024)
N_ALL = (2, 3, 15, 16, 17, 63, 64, 65, 129, 257, 300)
SWEEP = (
    (11, 300, 1, 1.0, 10.0, None),
    (12, 257, 3, 1.0, 30.0, None),
    (13, 129, 16, 1.0, 30.0, None),
    (14, 65, 17, 1.0, 20.0, None),
    (15, 64, 31, 1.0, 15.0, None),
    (16, 63, 32, 1.0, 10.0, None),
    (17, 17, 33, 1.0, 5.0, None),
    (18, 16, 64, 1.0, 4.5, None),
    (19, 15, 65, 1.0, 4.0, None),
    # perplexity below 1 is never reached: at scale 1 every row would double beta into the subnormal range and be
    # fragile; at 1e-15 the 100 doublings end at beta D of about 320, all sums normal, iters = 100 (the cap)
    (20, 3, 127, 1e-15, 0.6, None),
    (21, 2, 128, 1e-15, 0.3, None),
    (22, 64, 129, 1.0, 12.0, None),
    (23, 65, 1024, 1.0, 20.0, None),
)


def rows(seed, n, d, scale, extra=None):
    X = np.random.default_rng(seed).standard_normal((n, d)) * scale
    if extra == "dup":
        X[10:14] = X[9]
    elif extra == "offset":
        X = X + 1e4
    return np.ascontiguousarray(X)


class Case:
    """X (numpy fp64), perplexity; the oracle's beta / iters / s / scores, ``fragile`` [n] bool, ``tol_s`` [n],
    ``tol_scores`` [n] and, for the bounds, D (longdouble) and eD."""


def dissimilarity(X):
    Xl = X.astype(LD)
    n = X.shape[0]
    D = np.empty((n, n), dtype=LD)
    for i in range(n):
        diff = Xl - Xl[i]
        D[i] = (diff * diff).sum(1)
    return D


def _e_d(X):
    Xl = X.astype(LD)
    x0 = Xl - Xl.mean(0)
    return (4 * X.shape[1] + 20) * U * float((x0 * x0).sum(1).max())


def _affinity(D, beta):
    """exp(-beta D) rounded through fp64, the diagonal zero, as longdouble."""
    with np.errstate(under="ignore"):
        A = np.exp(-(beta.astype(LD)[:, None]) * D).astype(np.float64).astype(LD)
    np.fill_diagonal(A, 0)
    return A


def _rho(D, beta, eD):
    bd = np.minimum((beta[:, None] * D).astype(np.float64), 746.0)
    return beta[:, None] * eD + (bd + 2.0) * U


def oracle(X, perplexity):
    n, d = X.shape
    c = Case()
    c.X, c.perplexity = X, perplexity
    D = dissimilarity(X)
    eD = _e_d(X)
    c.D, c.eD = D, eD
    logh = np.log(LD(perplexity))
    beta = np.ones(n)
    bmin = np.zeros(n)
    bmax = np.full(n, np.inf)
    iters = np.zeros(n, dtype=np.int32)
    active = np.ones(n, dtype=bool)
    fragile = np.zeros(n, dtype=bool)
    s_fin = np.zeros(n, dtype=LD)
    Df = D.astype(np.float64)
    while active.any():
        A = _affinity(D, beta)
        s = A.sum(1)
        t = (A * D).sum(1)
        with np.errstate(all="ignore"):
            H = t * (beta.astype(LD) / s)
            err = H + np.log(s) - logh
            # the bound of the docstring, per row
            w = (A / s[:, None]).astype(np.float64)
            rho = _rho(D, beta, eD)
            R = (w * rho).sum(1)
            rs = R + n * U
            Hf = H.astype(np.float64)
            bound = ((w * (beta[:, None] * Df) * rho).sum(1) + beta * eD + (n + 1) * U * Hf + (Hf + 1.0) * rs
                     + 4 * U * (Hf + np.abs(np.log(s)).astype(np.float64) + abs(float(logh))))
            slack = MARGIN * bound
            errf = err.astype(np.float64)
            near = np.abs(np.abs(errf) - TOL) < slack
        sub = (s > 0) & (s < LD(1e-300))
        fragile |= active & ((near & ~np.isnan(errf)) | sub)
        s_fin = np.where(active, s, s_fin)
        nan = np.isnan(errf)
        go = active & (iters < MAX_ITER) & (nan | (np.abs(err) > TOL))
        pos = go & ~nan & (err > 0)
        neg = go & ~nan & ~(err > 0)
        nb = np.where(go & nan, beta / 10.0, beta)
        nb = np.where(pos, np.where(np.isinf(bmax), beta * 2.0, 0.5 * (beta + bmax)), nb)
        nb = np.where(neg, 0.5 * (bmin + beta), nb)
        bmin = np.where(pos, beta, bmin)
        bmax = np.where(neg, beta, bmax)
        beta = nb
        iters = iters + go.astype(np.int32)
        active = go
    c.beta, c.iters, c.fragile = beta, iters, fragile
    c.s = s_fin.astype(np.float64)
    with np.errstate(all="ignore"):
        A = _affinity(D, beta)
        w = (A / s_fin[:, None]).astype(np.float64)
        c.tol_s = MARGIN * ((w * _rho(D, beta, eD)).sum(1) + n * U) * c.s
        c.scores, c.tol_scores = products_oracle(c, beta, c.s)
    return c


def products_oracle(c, beta, s):
    """(p [n] fp64, tol [n]) of the longdouble products prod_{i != j} (1 - exp(-beta_i D_ij) / s_i) for the given
    fp64 ``beta`` and ``s`` of all rows."""
    n = c.D.shape[0]
    with np.errstate(all="ignore"):
        A = _affinity(c.D, beta)
        B = A / s.astype(LD)[:, None]
        F = 1 - B
        np.fill_diagonal(F, 1)
        p = F.prod(0)
        dF = B.astype(np.float64) * (_rho(c.D, beta, c.eD) + U) + U
        np.fill_diagonal(dF, 0.0)
        excl = np.empty((n, n), dtype=LD)
        for i in range(n):
            for j in np.nonzero(F[i] == 0)[0]:
                excl[i, j] = np.delete(F[:, j], i).prod()
        nz = F != 0
        excl[nz] = (np.broadcast_to(p, (n, n))[nz] / F[nz])
        tol = MARGIN * ((dF * excl.astype(np.float64)).sum(0) + 2 * n * U * p.astype(np.float64)) + P_FLOOR
    return p.astype(np.float64), tol


@functools.lru_cache(maxsize=None)
def case(seed, n, d, scale, perplexity, extra=None):
    return oracle(rows(seed, n, d, scale, extra), perplexity)


def fragile_share(c):
    return float(c.fragile.mean())


def check_search(c, beta, s, iters):
    """``beta`` and ``iters`` bit-equal to the oracle on the rows that are not fragile, ``s`` within its bound there;
    returns the number of rows compared.  Prints the figures first."""
    beta, s, iters = (t.detach().cpu().numpy() for t in (beta, s, iters))
    ok = ~c.fragile
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(s[ok] == c.s[ok], 0.0, np.abs(s[ok] - c.s[ok]) / c.tol_s[ok])
    print("fragile", int(c.fragile.sum()), "of", len(ok), "iters", int(c.iters.min()), "-", int(c.iters.max()),
          "beta mismatches", int((beta[ok] != c.beta[ok]).sum()), "iters mismatches",
          int((iters[ok] != c.iters[ok]).sum()), "err/tol s", float(ratio.max()) if ratio.size else 0.0)
    assert fragile_share(c) <= FRAGILE_CAP
    assert iters.dtype == np.int32 and beta.dtype == np.float64
    assert np.array_equal(beta[ok], c.beta[ok])
    assert np.array_equal(iters[ok], c.iters[ok])
    assert np.all(np.abs(s[ok] - c.s[ok]) <= c.tol_s[ok])
    return int(ok.sum())


def check_products(c, beta, s, p):
    """``p`` against the longdouble products from the same ``(beta, s)`` (torch tensors of all rows)."""
    want, tol = products_oracle(c, beta.detach().cpu().numpy(), s.detach().cpu().numpy())
    p = p.detach().cpu().numpy()
    err = np.abs(p - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("err/tol p", float(np.max(np.where(err == 0, 0.0, err / tol))))
    assert p.shape == want.shape
    assert np.all(err <= tol)


def check_scores(c, p):
    """Scores of a whole run against the oracle's, on a case without fragile rows."""
    assert not c.fragile.any()
    p = p.detach().cpu().numpy()
    err = np.abs(p - c.scores)
    # the run's own s differs from the oracle's by tol_s, which moves every factor of that row: b_ij by b_ij tol_s_i/s_i
    n = len(p)
    with np.errstate(all="ignore"):
        A = _affinity(c.D, c.beta)
        B = (A / c.s.astype(LD)[:, None]).astype(np.float64)
        F = 1.0 - B
        np.fill_diagonal(F, 1.0)
        extra = (B * (c.tol_s / c.s)[:, None] / np.where(F == 0, 1.0, F)).sum(0) * c.scores
    tol = c.tol_scores + extra
    print("err/tol scores", float(np.max(np.where(err == 0, 0.0, err / tol))))
    assert np.all(err <= tol)


# ---------------------------------------------------------------------------------------------------- operators

def vector_table(X, device="cpu"):
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    return MTable(TableSchema(["v"], [Types.DENSE_VECTOR]), [Column(torch.from_numpy(X).to(device))])


def csr_table(X, device="cpu"):
    """The rows as a CSR vector column (the zeros of X left out)."""
    from alink_amd.common.linalg.block import SparseBlock
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    nz = X != 0
    crow = np.concatenate([[0], np.cumsum(nz.sum(1))]).astype(np.int64)
    col = np.nonzero(nz)[1].astype(np.int64)
    blk = SparseBlock(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(X[nz]), X.shape[1]).to(device)
    return MTable(TableSchema(["v"], [Types.SPARSE_VECTOR]), [Column(blk)])


def run_op(mt, perplexity, device):
    """The score column of ``SosBatchOp`` on the table ``mt`` as a numpy array."""
    from alink_amd import SosBatchOp, useLocalEnv
    from alink_amd.operator.batch.source import TableSourceBatchOp
    useLocalEnv(1, device=device)
    op = SosBatchOp().setVectorCol("v").setPredictionCol("score").setPerplexity(perplexity)
    out = op.linkFrom(TableSourceBatchOp(mt)).collect()
    return np.array([float(r[-1]) for r in out])
