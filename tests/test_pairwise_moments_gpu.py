"""The pairwise-complete moment pass (ops/csrc/moments.hip, ``pairwise_moments``) on the GPU against longdouble oracles
and itself (grids, alignment), and ``CorrelationBatchOp`` on columns with NULL cells against a two-pass pairwise
longdouble oracle and against ``ALINK_MOMENTS_HIP=0``."""
import functools
import itertools

import numpy as np
import pytest
import torch

from alink_amd.ops import _lib, moments as M

pytestmark = pytest.mark.gpu
L = np.longdouble
U = L(2) ** -53
DS, NS = (1, 2, 15, 16, 17, 63, 64, 65, 81, 97, 129, 1024), (1, 3, 63, 64, 65, 200)
# d and n taken in turn (one tile, a ragged tile, a full block of 64, a last block of 1 .. 4 tiles), then several
# chunks over a full and a ragged block, their off-diagonal unit, and 177: two full blocks and a last one of 4 tiles;
# at chunk_rows = 64, n = 513 and 641 are 9 and 11 chunks: the merge's round of eight loads in flight
CASES = list(zip(DS, itertools.cycle(NS))) + [(65, 200), (129, 200), (177, 200), (17, 513), (17, 641)]
# at d = 1024 two combinations that share nothing; the others repeat them at the cost of a longdouble oracle each
COMBOS = [(d, n, c, s, p) for (d, n), c, s, p in itertools.product(CASES, (0, 64), (False, True),
                                                                  ("none", "random", "structured"))
          if d < 1024 or (c, s, p) in ((64, True, "random"), (0, False, "structured"))]


@functools.lru_cache(maxsize=None)
def pairwise_case(d, n, shifted, pattern):
    """X with NaN in the missing cells, the shift, and the longdouble N, S, Q, P with the sums of |terms| of S and P
    (Q's terms are not negative)."""
    rng = np.random.default_rng(1000 * d + n)
    X = rng.standard_normal((n, d)) + 3.0
    miss = np.zeros((n, d), dtype=bool)
    if pattern == "random":
        miss = rng.random((n, d)) < 0.3
    elif pattern == "structured":
        miss[:, 0] = True                           # a column without a present cell
        if d >= 3:
            miss[0::2, 1], miss[1::2, 2] = True, True       # present on disjoint rows: N[1, 2] = 0
        miss[n - 1 if n > 1 else n:, :] = True      # the last row
        miss[63::64, d - 1] = True                  # the last column in the last staged row of a batch
    X[miss] = np.nan
    shift = 3.0 + rng.standard_normal(d) if shifted else None
    K = (~miss).astype(L)
    Y = np.where(miss, L(0), X.astype(L) - (shift.astype(L) if shifted else 0))
    return X, shift, K.T @ K, Y.T @ K, (Y * Y).T @ K, Y.T @ Y, np.abs(Y).T @ K, np.abs(Y).T @ np.abs(Y)


def run_pairwise(X, shift, **kw):
    calls = M.PAIRWISE_CALLS
    out = M.pairwise_moments(X, None if shift is None else torch.from_numpy(shift), **kw)
    assert M.PAIRWISE_CALLS == calls + 1 and out.shape == (4, X.shape[1], X.shape[1])
    return out


@pytest.mark.parametrize("d,n,chunk_rows,shifted,pattern", COMBOS)
def test_pairwise_moments_against_the_oracle(d, n, chunk_rows, shifted, pattern):
    """N equals the integer counts.  S and P against the longdouble sums of y = x - shift over the pair's rows, bound
    per element (n + 4) 2^-53 sum |terms|: one rounding of y (two factors in P), then any order of n fused products,
    as in test_moments_against_the_oracle.  Q's bound is (n + 5) 2^-53 Q: its square is rounded once more before the
    instruction.  N and P are exactly symmetric.  A dropped tile family, S_AB for S_BA or a NaN in a sum exceeds these
    by many orders."""
    _lib.require()
    X, shift, rN, rS, rQ, rP, aS, aP = pairwise_case(d, n, shifted, pattern)
    N, S, Q, P = run_pairwise(torch.from_numpy(X).cuda(), shift, chunk_rows=chunk_rows).cpu().numpy()
    assert np.array_equal(N, rN.astype(np.float64))
    assert (np.abs(S.astype(L) - rS) <= (n + 4) * U * aS).all()
    assert (np.abs(Q.astype(L) - rQ) <= (n + 5) * U * rQ).all()
    assert (np.abs(P.astype(L) - rP) <= (n + 4) * U * aP).all()
    assert np.array_equal(N, N.T) and np.array_equal(P, P.T)


@pytest.mark.parametrize("d", [16, 17, 81, 129])
def test_same_bits_for_every_grid_and_alignment(d):
    _lib.require()
    X, shift = pairwise_case(d, 200, True, "random")[:2]
    Xd = torch.from_numpy(X).cuda()
    base = torch.empty(200 * d + 1, dtype=torch.float64, device="cuda")
    off8 = base[1:].view(200, d)
    off8.copy_(Xd)
    assert Xd.data_ptr() % 16 == 0 and off8.data_ptr() % 16 == 8
    out0 = run_pairwise(Xd, shift, chunk_rows=64)
    assert not torch.isnan(out0).any()
    for rows, grid in ((Xd, 1), (Xd, 7), (Xd, 7), (off8, 0)):
        assert torch.equal(run_pairwise(rows, shift, grid=grid, chunk_rows=64), out0)


def pair_oracle(X):
    """Two-pass pairwise-complete Pearson correlation in longdouble (NaN: missing); NaN below two common rows."""
    d = X.shape[1]
    C = np.full((d, d), np.nan, dtype=L)
    for a, b in itertools.product(range(d), repeat=2):
        both = ~np.isnan(X[:, a]) & ~np.isnan(X[:, b])
        if both.sum() >= 2:
            xa, xb = X[both, a].astype(L), X[both, b].astype(L)
            xa, xb = xa - xa.mean(), xb - xb.mean()
            C[a, b] = (xa * xb).sum() / np.sqrt((xa * xa).sum() * (xb * xb).sum())
    np.fill_diagonal(C, 1)
    return C


def err(a, b):
    """Largest error of a against b over b's finite entries (correlations: the largest entry is 1); the NaN entries
    must be the same."""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.nanmax(np.abs(a - b)))


def test_operator_on_columns_with_nulls(monkeypatch):
    """CorrelationBatchOp on 200 x 5 device columns with None in about 20 % of the cells (columns 0 and 1 correlated,
    column 4 with one present value: its correlations are NaN).  Pearson at mean 1e8 and unit spread against the
    two-pass pairwise longdouble oracle; tolerance: 8 x the error of ``pairwise_moments_torch`` (fp64, CPU, the same
    shift and epilogue) against that oracle, at least 2^-46.  Then Pearson and SPEAMAN at mean 0 under
    ``ALINK_MOMENTS_HIP=1`` against ``=0`` by the same tolerance; the pass runs exactly under ``=1``."""
    _lib.require()
    from alink_amd import CorrelationBatchOp, MemSourceBatchOp, useLocalEnv
    from alink_amd.models.statistics.summary import _corr_of_pairwise
    rng = np.random.default_rng(11)
    E = rng.standard_normal((200, 5))
    E[:, 1] = 0.8 * E[:, 0] + 0.6 * E[:, 1]
    E[rng.random((200, 5)) < 0.2] = np.nan
    E[0, 4], E[1:, 4] = 0.5, np.nan
    names = ["a", "b", "c", "d", "e"]

    def op(X, flag, method="PEARSON"):
        monkeypatch.setenv("ALINK_MOMENTS_HIP", flag)
        calls = M.PAIRWISE_CALLS
        rows = [tuple(None if v != v else v for v in r) for r in X.tolist()]
        src = MemSourceBatchOp(rows, ", ".join(f"{c} double" for c in names))
        corr = CorrelationBatchOp().setSelectedCols(names).setMethod(method).linkFrom(src).collectCorrelation()
        assert M.PAIRWISE_CALLS - calls == (1 if flag == "1" else 0)
        return np.asarray(corr.getCorrelation())
    big = E + 1e8
    ref = pair_oracle(big)
    assert np.isnan(ref[4, :4]).all() and np.isfinite(ref[:4, :4]).all()
    shift = torch.tensor([col[~np.isnan(col)][0] for col in big.T])     # what pairwise_shift picks
    tol = max(8 * err(_corr_of_pairwise(M.pairwise_moments_torch(torch.from_numpy(big), shift)), ref), 2.0 ** -46)
    try:
        useLocalEnv(1, device="cuda:0")
        got = op(big, "1")
        between = [err(op(E, "1", m), op(E, "0", m)) for m in ("PEARSON", "SPEAMAN")]
    finally:
        useLocalEnv(1, device="cpu")
    print("tol %.3e" % tol, "error %.3e" % err(got, ref), "against the former path", between)
    assert err(got, ref) <= tol and max(between) <= tol
