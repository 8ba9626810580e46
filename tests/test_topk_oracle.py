"""The top-K oracle against a naive loop, and the torch path of ops/topk.py and the one-rank ring against the
oracle on integer data: values bitwise, ids exact, for every tie and partition case the GPU tests use."""
import numpy as np
import pytest
import torch

import topk_helpers as H
from alink_amd.ops import topk as ops


def _naive(Q, T, K, ids):
    """One query at a time: every (score, id) pair into a Python list, sorted by the contract's key."""
    val, idx = [], []
    for q in Q:
        pairs = sorted(((int(np.dot(q, t)), int(i)) for t, i in zip(T, ids)), key=lambda p: (-p[0], p[1]))[:K]
        pairs += [(-np.inf, -1)] * (K - len(pairs))
        val.append([p[0] for p in pairs])
        idx.append([p[1] for p in pairs])
    return np.array(val, dtype=np.float64), np.array(idx, dtype=np.int64)


@pytest.mark.parametrize("m,n,r,K", [(1, 1, 1, 1), (3, 7, 2, 3), (4, 5, 3, 8), (5, 40, 2, 6)])
def test_oracle_matches_naive_loop(m, n, r, K):
    Q, T = H.tie_rich(m + n, m, n, r)
    ids = np.arange(n) * 3 + 5
    v, i = H.topk_oracle(Q, T, K, ids)
    nv, ni = _naive(Q, T, K, ids)
    assert np.array_equal(i, ni) and np.array_equal(v, nv)
    # ties exist in these inputs (or the oracle's second key is not exercised)
    if n >= 40:
        S = Q @ T.T
        assert any(len(set(row.tolist())) < n for row in S)


def test_oracle_float_inputs_score_in_fp64():
    rng = np.random.default_rng(0)
    Q, T = rng.normal(size=(3, 4)).astype(np.float32), rng.normal(size=(9, 4)).astype(np.float32)
    v, i = H.topk_oracle(Q, T, 4)
    S = Q.astype(np.float64) @ T.astype(np.float64).T
    for q in range(3):
        assert i[q].tolist() == np.argsort(-S[q], kind="stable")[:4].tolist()
        assert v[q].tolist() == S[q, i[q]].tolist()


@pytest.mark.parametrize("name", sorted(H.tie_cases()))
def test_fallback_ties_and_partitions(name):
    Q, T, K = H.tie_cases()[name]
    want = H.topk_oracle(Q, T, K)
    for how, blocks in H.partitions(T.shape[0]).items():
        H.assert_exact(H.merged(Q, T, K, blocks), want, f"{name}/{how}")


@pytest.mark.parametrize("n,K", [(1, 1), (1, 4), (63, 128), (65, 5), (129, 128), (129, 129)])
def test_fallback_negative_scores_and_short_blocks(n, K):
    """Every real score is below 0 and K may exceed n: the tail is (-inf, -1)."""
    rng = np.random.default_rng(n + K)
    Q, T = H.ints(rng, (6, 5), 1, 3), -H.ints(rng, (n, 5), 1, 3)
    want = H.topk_oracle(Q, T, K)
    H.assert_exact(H.merged(Q, T, K, [(0, n)]), want)
    H.assert_exact(H.merged(Q, T, K, [(n // 2, n), (0, n // 2)]), want, "reversed halves")


def test_fallback_boundary_tie_arrives_later_with_smaller_id():
    """The K-th score is tied between an id in the second half (merged first) and ids in the first half (merged
    later): the smaller ids win; and a strictly better item evicts the tied minimum with the largest id."""
    Q = np.array([[1, 0], [0, 1]], dtype=np.int64)
    T = np.zeros((140, 2), dtype=np.int64)
    T[[2, 66, 70, 130], 0] = 5                                 # four tied at 5 for query 0, K = 3
    T[100, 0] = 9
    T[:, 1] = -np.arange(140) // 50                            # query 1: long runs of equal scores
    h = 69
    want = H.topk_oracle(Q, T, 3)
    assert want[1][0].tolist() == [100, 2, 66]
    H.assert_exact(H.merged(Q, T, 3, [(h, 140), (0, h)]), want)
    # state {2, 66, 70} tied at 5, then the 9 arrives alone: 70 leaves
    st = ops.TopKState(2, 3, "cpu")
    Tt = H.f32(T)
    for lo, hi in ((0, 100), (101, 130)):
        ops.merge(st, H.f32(Q), Tt[lo:hi], lo, use_kernel=False)
    assert sorted(st.idx[0].tolist()) == [2, 66, 70]
    ops.merge(st, H.f32(Q), Tt[100:101], 100, use_kernel=False)
    assert ops.finish(st)[1][0].tolist() == [100, 2, 66]


def test_fallback_item_base_near_int32_limit():
    Q, T = H.tie_rich(21, 4, 90, 3)
    base = 2 ** 31 - 1 - 90
    st = ops.TopKState(4, 12, "cpu")
    ops.merge(st, H.f32(Q), H.f32(T), base, use_kernel=False)
    H.assert_exact(ops.finish(st), H.topk_oracle(Q, T, 12, base + np.arange(90)))


def test_blockwise_topk_one_rank_both_orders():
    from alink_amd.parallel.cross import blockwise_topk
    Q, T = H.tie_rich(31, 12, 150, 4)
    Q[3] = 0
    for desc in (True, False):
        v, i = blockwise_topk(H.f32(Q), H.f32(T), 9, descending=desc)
        rv, ri = H.topk_oracle(Q if desc else -Q, T, 9)
        assert i.dtype == torch.int64
        H.assert_exact((v, i), (rv if desc else -rv, ri), f"descending={desc}")
