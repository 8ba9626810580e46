"""Exact oracle and integer data for the top-K cross tests (ops/topk.py, csrc/topk.hip, parallel/cross.py).

The contract under test: entry (s, id) ranks before (s', id') iff s > s', or s == s' and id < id'; a query's
result is the first min(K, N) of all (score, global id) pairs in that order, then (-inf, -1) fillers; it
depends only on the queries, the items with their global ids and K.

Integer inputs make every score exact in fp32 (|score| < 2^24), so values compare bitwise and ids exactly.
"""
import numpy as np
import torch


def topk_oracle(Q, T, K, ids=None):
    """(values float64 [m, K], ids int64 [m, K]) of the contract.  Integer inputs are scored in int64, float
    inputs in fp64; ``ids`` are the global ids of T's rows (default 0..n-1)."""
    Q, T = np.asarray(Q), np.asarray(T)
    wide = np.int64 if np.issubdtype(Q.dtype, np.integer) and np.issubdtype(T.dtype, np.integer) else np.float64
    S = Q.astype(wide) @ T.astype(wide).T
    n = T.shape[0]
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    kk = min(K, n)
    val = np.full((Q.shape[0], K), -np.inf)
    idx = np.full((Q.shape[0], K), -1, dtype=np.int64)
    for q in range(Q.shape[0]):
        order = np.lexsort((ids, -S[q]))[:kk]
        val[q, :kk] = S[q, order]
        idx[q, :kk] = ids[order]
    return val, idx


def ints(rng, shape, lo, hi):
    """Integer matrix with entries in [lo, hi], as int64."""
    return rng.integers(lo, hi + 1, size=shape).astype(np.int64)


def tie_rich(seed, m, n, r):
    """Entries in [-3, 3]: |score| <= 9 r, so a few hundred items give every query many equal scores."""
    rng = np.random.default_rng(seed)
    return ints(rng, (m, r), -3, 3), ints(rng, (n, r), -3, 3)


def magnitude(seed, m, n):
    """Entries in [-500, 500] at r = 64: |score| <= 64 * 250000 = 1.6e7 < 2^24, still exact in fp32."""
    rng = np.random.default_rng(seed)
    return ints(rng, (m, 64), -500, 500), ints(rng, (n, 64), -500, 500)


def f32(a, device="cpu"):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=device)


def merged(Q, T, K, blocks, device="cpu", use_kernel=False, state=None):
    """``finish`` of the blocks ``[(lo, hi), ...]`` of ``T`` merged in the order given, each at base ``lo``."""
    from alink_amd.ops import topk as ops
    Qd = Q if torch.is_tensor(Q) else f32(Q, device)
    Td = T if torch.is_tensor(T) else f32(T, device)
    st = ops.TopKState(Qd.shape[0], K, device) if state is None else state
    for lo, hi in blocks:
        ops.merge(st, Qd, Td[lo:hi], lo, use_kernel=use_kernel)
    return ops.finish(st)


def assert_exact(got, want, what=""):
    """Values bitwise (== on fp32, fillers included) and ids exactly equal to the oracle's."""
    v, i = got
    rv, ri = want
    v, i = v.detach().cpu(), i.detach().cpu().to(torch.int64)
    rv32 = torch.as_tensor(np.asarray(rv, dtype=np.float32))
    ri = torch.as_tensor(np.asarray(ri, dtype=np.int64))
    bad = (i != ri).any(1).nonzero().flatten().tolist()
    assert not bad, f"{what}: ids differ in rows {bad[:5]}: got {i[bad[0]].tolist()} want {ri[bad[0]].tolist()}"
    assert torch.equal(v, rv32), f"{what}: values differ"


def partitions(n):
    """The four ways the partition tests split n items: one block, two in order, three in ring order (last
    first), and a one-row block in the middle."""
    a, b = n // 3, (2 * n) // 3
    h = n // 2
    return {
        "one": [(0, n)],
        "two": [(0, h), (h, n)],
        "ring3": [(b, n), (0, a), (a, b)],
        "one_row_middle": [(0, h), (h, h + 1), (h + 1, n)],
    }


# the tie and partition cases shared by the CPU (fallback) and GPU (kernel) tests: name -> (Q, T, K)
def tie_cases():
    cases = {}
    for K in (5, 6, 10):
        Qz, Tz = tie_rich(K, 3, 300, 8)
        Qz[0] = 0                                             # an all-zero query: ids 0..K-1
        cases[f"zero_query_K{K}"] = (Qz, Tz, K)
    Q, T = tie_rich(11, 9, 130, 5)
    for i in (4, 16, 20, 63, 64, 65):                         # duplicates of row 3 across lane groups and chunks
        T[i] = T[3]
    cases["duplicate_rows"] = (Q, T, 6)
    Q, T = tie_rich(12, 40, 200, 3)
    cases["dense_ties"] = (Q, T, 10)
    Q, T = magnitude(13, 20, 150)
    T[70:75] = T[5]
    cases["magnitude"] = (Q, T, 7)
    return cases
