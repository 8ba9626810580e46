"""The fused score + top-K kernel (ops/csrc/topk.hip) against the exact oracle of tests/topk_helpers.py.

Integer data makes every fp32 score exact, so values are compared bitwise and ids exactly: the (score, id)
order, the item and query edges, every rank instantiation and its k permutation, state carried across
launches in any order, item slices (grid.y > 1) with their host merge, ids up to 2^31 - 1, and the torch path
on the device.  One test with random normal data checks the kernel's rounding against a derived bound."""
import functools

import numpy as np
import pytest
import torch

import topk_helpers as H
from alink_amd.ops import topk as ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _kernel(Q, T, K, blocks=None, state=None):
    return H.merged(Q, T, K, blocks or [(0, np.asarray(T).shape[0])], DEV, True, state)


@pytest.fixture
def launches(monkeypatch):
    """The (n, item_base, slices, per_slice) of every kernel launch made through ``_lib.call``."""
    seen = []
    real = ops._lib.call

    def spy(name, *a, **kw):
        if name == "alink_topk_cross_f32":
            seen.append((a[3], a[4], a[9], a[10]))
        return real(name, *a, **kw)
    monkeypatch.setattr(ops._lib, "call", spy)
    return seen


# ---- item edges: padding rows of the last chunk score 0 and must not beat negative scores -------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129])
def test_item_edges_negative_scores(n):
    rng = np.random.default_rng(n)
    Q, T = H.ints(rng, (20, 5), 1, 3), -H.ints(rng, (n, 5), 1, 3)
    for K in (1, 3, 4, 5, 128):
        want = H.topk_oracle(Q, T, K)
        assert (want[0][:, :min(K, n)] < 0).all()
        H.assert_exact(_kernel(Q, T, K), want, f"K={K}")
        if K > n:
            v, i = _kernel(Q, T, K)
            assert bool((i[:, n:] == -1).all()) and bool((v[:, n:] == float("-inf")).all())


# ---- query edges: partial waves and workgroups; every row has its own answer -------------------------------

@pytest.mark.parametrize("m", [1, 15, 16, 17, 127, 128, 129])
def test_query_edges_distinct_rows(m):
    n = 130
    i = np.arange(n, dtype=np.int64)
    T = np.stack([i, -i * i], 1)
    Q = np.stack([2 * np.arange(m, dtype=np.int64), np.ones(m, dtype=np.int64)], 1)   # score = q^2 - (i - q)^2
    want = H.topk_oracle(Q, T, 5)
    assert len({tuple(r) for r in want[1].tolist()}) == m
    assert want[1][:, 0].tolist() == list(range(m))
    H.assert_exact(_kernel(Q, T, 5), want)


# ---- rank: each of the four instantiations, with and without zero padding, and the k permutation ------------

@pytest.mark.parametrize("r", [1, 3, 16, 17, 32, 33, 48, 49, 64])
def test_rank_identity_queries_pick_their_column(r):
    """Q = 3 I_r: query d must return the top-K of column d of T, so a dim that reaches the wrong MFMA step
    shows as another column's ranking."""
    rng = np.random.default_rng(r)
    T = H.ints(rng, (200, r), -500, 500)
    Q = 3 * np.eye(r, dtype=np.int64)
    want = H.topk_oracle(Q, T, 7)
    for d in range(r):
        col = np.lexsort((np.arange(200), -T[:, d]))[:7]
        assert want[1][d].tolist() == col.tolist()
    H.assert_exact(_kernel(Q, T, 7), want)


@pytest.mark.parametrize("r", [1, 3, 16, 17, 32, 33, 48, 49, 64])
def test_rank_dense_integer_queries(r):
    rng = np.random.default_rng(100 + r)
    Q, T = H.ints(rng, (33, r), -500, 500), H.ints(rng, (300, r), -500, 500)
    H.assert_exact(_kernel(Q, T, 9, [(0, 100), (100, 300)]), H.topk_oracle(Q, T, 9))


# ---- ties and partition invariance ----------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(H.tie_cases()))
def test_ties_and_partitions(name):
    """One block, two in order, three in ring order, a one-row block in the middle: identical values and ids,
    equal to the oracle, and bitwise the same when run again."""
    Q, T, K = H.tie_cases()[name]
    want = H.topk_oracle(Q, T, K)
    if name.startswith("zero_query"):
        assert want[1][0].tolist() == list(range(K))
    for how, blocks in H.partitions(T.shape[0]).items():
        first = _kernel(Q, T, K, blocks)
        H.assert_exact(first, want, f"{name}/{how}")
        again = _kernel(Q, T, K, blocks)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_boundary_tie_arrives_later_with_smaller_id():
    """The K-th score is tied between ids of the block merged first (T[h:]) and smaller ids of the block merged
    later (T[:h]): the smaller ids win, in both launch orders."""
    Q = np.array([[1, 0], [0, 1]], dtype=np.int64)
    T = np.zeros((140, 2), dtype=np.int64)
    T[[2, 66, 70, 130], 0] = 5
    T[100, 0] = 9
    T[:, 1] = -np.arange(140) // 50
    h = 69
    want = H.topk_oracle(Q, T, 3)
    assert want[1][0].tolist() == [100, 2, 66]
    H.assert_exact(_kernel(Q, T, 3, [(h, 140), (0, h)]), want, "later block has the smaller ids")
    H.assert_exact(_kernel(Q, T, 3, [(0, h), (h, 140)]), want, "in order")


def test_better_item_evicts_tied_minimum_with_largest_id():
    Q = np.array([[1, 0]], dtype=np.int64)
    T = np.zeros((140, 2), dtype=np.int64)
    T[[2, 66, 70], 0] = 5
    T[100, 0] = 9
    st = ops.TopKState(1, 3, DEV)
    Qd, Td = H.f32(Q, DEV), H.f32(T, DEV)
    ops.merge(st, Qd, Td[:100], 0, use_kernel=True)
    assert sorted(st.idx[0].tolist()) == [2, 66, 70]
    ops.merge(st, Qd, Td[100:], 100, use_kernel=True)
    v, i = ops.finish(st)
    assert i[0].tolist() == [100, 2, 66] and v[0].tolist() == [9.0, 5.0, 5.0]


# ---- item slices: blockIdx.y > 0, per-plane states, item_base + i0, the host merge of planes ------------------

@functools.lru_cache(maxsize=None)
def _slice_case(n, m):
    """Tie-rich rank-16 data with n + 150 items (the sliced block is rows 50 .. n + 50) and the K = 128 oracles,
    of which every smaller K is a prefix.  Query 0 and the rows around both candidate slice boundaries are all
    threes: the duplicates on either side of the boundary are that query's best items."""
    Q, T = H.tie_rich(n + m, m, n + 150, 16)
    Q[0] = 3
    for per in _pers(n, m):
        T[50 + per - 2:50 + per + 2] = 3
    whole = H.topk_oracle(Q, T, 128)
    block = H.topk_oracle(Q, T[50:n + 50], 128, 50 + np.arange(n))
    return Q, T, whole, block


def _pers(n, m):
    """per_slice of the plan merge() makes for n items and m queries (recomputed, then checked by the spy)."""
    slices = max(1, min(ops.WANT_WG // ((m + ops.QB - 1) // ops.QB), (n + 4095) // 4096))
    return [((n + slices - 1) // slices + 63) // 64 * 64]


@pytest.mark.parametrize("n", [4097, 8193])
@pytest.mark.parametrize("m", [5, 129])
def test_sliced_launches(n, m, launches):
    Q, T, whole, block = _slice_case(n, m)
    per = _pers(n, m)[0]
    Qd, Td = H.f32(Q, DEV), H.f32(T, DEV)
    for K in (1, 10, 128):
        # the block alone, at item_base 50, into an empty state
        del launches[:]
        got = H.merged(Qd, Td, K, [(50, n + 50)], DEV, True)
        assert launches == [(n, 50, (n + per - 1) // per, per)] and launches[0][2] >= 2
        H.assert_exact(got, (block[0][:, :K], block[1][:, :K]), f"K={K} empty state")
        # into a state that already holds the items below and above the block (plane 0 carries larger ids)
        del launches[:]
        got = H.merged(Qd, Td, K, [(0, 50), (n + 50, n + 150), (50, n + 50)], DEV, True)
        assert [l[2] for l in launches] == [1, 1, (n + per - 1) // per]
        H.assert_exact(got, (whole[0][:, :K], whole[1][:, :K]), f"K={K} prior state")
    # the duplicates on either side of the slice boundary are query 0's best, smallest id first
    assert block[1][0, :4].tolist() == [50 + per - 2, 50 + per - 1, 50 + per, 50 + per + 1]


# ---- ids up to 2^31 - 1 ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n,sliced", [(130, False), (4097, True)])
def test_item_base_near_int32_limit(n, sliced, launches):
    Q, T = H.tie_rich(n, 5, n, 16)
    base = 2 ** 31 - 1 - n
    st = ops.TopKState(5, 10, DEV)
    ops.merge(st, H.f32(Q, DEV), H.f32(T, DEV), base, use_kernel=True)
    assert (launches[0][2] >= 2) == sliced
    want = H.topk_oracle(Q, T, 10, base + np.arange(n))
    assert want[1].max() <= 2 ** 31 - 2
    H.assert_exact(ops.finish(st), want)


# ---- the torch path on the device keeps the same contract -----------------------------------------------------

@pytest.mark.parametrize("r,K", [(5, 129), (65, 10)])
def test_device_fallback_same_contract(r, K, launches):
    Q, T = H.tie_rich(r + K, 9, 300, r)
    Q[0] = 0
    Qd = H.f32(Q, DEV)
    assert not ops.kernel_supported(Qd, K)
    want = H.topk_oracle(Q, T, K)
    for how, blocks in H.partitions(300).items():
        H.assert_exact(H.merged(Qd, H.f32(T, DEV), K, blocks, DEV, None), want, how)
    assert launches == []


# ---- non-integer data: the kernel's rounding against the bound of a length-R fp32 dot product ----------------

@pytest.mark.parametrize("r,m,n", [(10, 130, 1000), (64, 130, 1000), (10, 5, 5000)])
def test_random_normal_within_derived_bound(r, m, n):
    """B[q, i] = gamma_R sum_d |q_d| |t_d| with gamma_R = R u / (1 - R u), u = 2^-24 and R the padded rank (the
    length of the kernel's fused-multiply-add chain; the padded products are exact zeros).  Every returned value
    is within B of the fp64 score of its id, and no item left out beats the smallest returned fp64 score by more
    than 2 max_i B[q, i] (its computed score lost to a computed score, each within its own B)."""
    g = torch.Generator().manual_seed(r + n)
    Q, T = torch.randn(m, r, generator=g), torch.randn(n, r, generator=g)
    K = 10
    v, i = H.merged(Q.to(DEV), T.to(DEV), K, [(0, n // 3), (n // 3, n)], DEV, True)
    v, i = v.cpu().double(), i.cpu().long()
    S = Q.double() @ T.double().T
    R = ops.pad_rank(r)
    u = 2.0 ** -24
    B = (R * u / (1 - R * u)) * (Q.double().abs() @ T.double().abs().T)
    assert bool((i >= 0).all()) and all(len(set(row)) == K for row in i.tolist())
    err = (v - torch.gather(S, 1, i)).abs()
    print("max err / bound:", float((err / torch.gather(B, 1, i)).max()))
    assert bool((err <= torch.gather(B, 1, i)).all())
    assert bool((v[:, :-1] >= v[:, 1:]).all())
    left = S.clone()
    left.scatter_(1, i, float("-inf"))
    smallest = torch.gather(S, 1, i).min(1).values
    slack = 2 * B.max(1).values
    print("max (left out - smallest returned) / slack:", float(((left.max(1).values - smallest) / slack).max()))
    assert bool((left.max(1).values <= smallest + slack).all())


# ---- the ring wrapper, ascending ------------------------------------------------------------------------

def test_blockwise_topk_ascending_integer_ties():
    from alink_amd.parallel.cross import blockwise_topk
    Q, T = H.tie_rich(41, 130, 500, 4)
    Q[7] = 0
    v, i = blockwise_topk(H.f32(Q, DEV), H.f32(T, DEV), 12, descending=False, use_kernel=True)
    rv, ri = H.topk_oracle(-Q, T, 12)
    assert i.dtype == torch.int64 and ri[7].tolist() == list(range(12))
    H.assert_exact((v, i), (-rv, ri))
