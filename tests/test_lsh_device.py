"""The torch and host parts of the device LSH path (``ops/lsh.py``, ``JavaRandom.nextGaussians``) against the host
path of ``models/similarity/lsh.py``; no GPU needed.  The kernels themselves are in ``test_lsh_gpu.py``."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lsh_helpers as H  # noqa: E402

from alink_amd.common.jrandom import JavaRandom  # noqa: E402
from alink_amd.models.common.features import FeatureMatrix  # noqa: E402
from alink_amd.models.similarity import lsh as L  # noqa: E402
from alink_amd.ops import lsh as K  # noqa: E402


def _pairs_equal(ha, hb, budget=None):
    wa, wb = L._candidates(ha, hb)
    ga, gb = K.candidate_pairs(torch.from_numpy(ha), torch.from_numpy(hb), budget=budget)
    assert ga.dtype == torch.int64 and gb.dtype == torch.int64
    assert np.array_equal(ga.numpy(), wa) and np.array_equal(gb.numpy(), wb)
    return len(wa)


@pytest.mark.parametrize("n,m,T", [(1, 1, 1), (50, 70, 3), (300, 200, 5), (64, 64, 2)])
def test_candidate_pairs_equal_the_host_join(n, m, T):
    rng = np.random.default_rng(n + m + T)
    for buckets in (1, 7, 40):                      # 1: every row in one bucket
        ha = rng.integers(-buckets, buckets, size=(n, T)).astype(np.int64) // 2
        hb = rng.integers(-buckets, buckets, size=(m, T)).astype(np.int64) // 2
        _pairs_equal(ha, hb)
    one = np.zeros((n, T), dtype=np.int64), np.zeros((m, T), dtype=np.int64)
    assert _pairs_equal(*one) == n * m
    # no two rows share a bucket
    assert _pairs_equal(np.arange(n * T).reshape(n, T), -1 - np.arange(m * T).reshape(m, T)) == 0
    # int32 hashes, as the kernels write them, negative ones included
    ha = rng.integers(-3, 3, size=(n, T)).astype(np.int32)
    hb = rng.integers(-3, 3, size=(m, T)).astype(np.int32)
    wa, wb = L._candidates(ha, hb)
    ga, gb = K.candidate_pairs(torch.from_numpy(ha), torch.from_numpy(hb))
    assert np.array_equal(ga.numpy(), wa) and np.array_equal(gb.numpy(), wb)


def test_candidate_pairs_stitch_chunks():
    rng = np.random.default_rng(5)
    ha = rng.integers(0, 6, size=(300, 5)).astype(np.int64)
    hb = rng.integers(0, 6, size=(200, 5)).astype(np.int64)
    total = _pairs_equal(ha, hb, budget=64)         # every query alone expands more than 64 pairs
    assert total > 64 * 10
    ha[::3] = -1                                    # queries without a candidate between the chunks
    _pairs_equal(ha, hb, budget=64)
    _pairs_equal(ha, hb, budget=1000)
    assert K.candidate_pairs(torch.zeros((0, 2), dtype=torch.int64), torch.zeros((4, 2), dtype=torch.int64))[0] \
        .numel() == 0
    assert K.candidate_pairs(torch.zeros((4, 2), dtype=torch.int64), torch.zeros((0, 2), dtype=torch.int64))[0] \
        .numel() == 0


def _host_top_n(qi, di, d, n):
    """The loop of ``approx_nearest_neighbors``."""
    from collections import defaultdict
    per = defaultdict(list)
    for a, b, x in zip(qi.tolist(), di.tolist(), d.tolist()):
        per[a].append((x, b))
    out = []
    for a in sorted(per):
        for rank, (x, b) in enumerate(sorted(per[a], key=lambda t: t[0])[:n], start=1):
            out.append((a, b, x, rank))
    return out


@pytest.mark.parametrize("n", [1, 3, 10])
def test_top_n_equals_the_host_loop(n):
    rng = np.random.default_rng(n)
    ha = rng.integers(0, 4, size=(40, 2)).astype(np.int64)
    ha[5] = 99                                      # a query without candidates
    hb = rng.integers(0, 4, size=(30, 2)).astype(np.int64)
    hb[:2] = 77
    ha[7] = 77                                      # a query with 2 candidates, fewer than n = 3 and 10
    qi, di = L._candidates(ha, hb)
    d = rng.integers(0, 4, size=len(qi)).astype(np.float64) / 4.0      # exact ties inside every query
    want = _host_top_n(qi, di, d, n)
    got = K.top_n(torch.from_numpy(qi), torch.from_numpy(di), torch.from_numpy(d), n)
    assert [tuple(t) for t in zip(*(x.tolist() for x in got))] == want
    assert got[3].dtype == torch.int64 and int(got[3].min()) == 1
    counts = np.bincount(got[0].numpy(), minlength=40)
    assert counts[5] == 0 and counts[7] == min(n, 2) and counts.max() == n


def test_canonical_csr():
    crow = torch.tensor([0, 3, 3, 5], dtype=torch.int64)
    # explicit zeros are dropped
    fm = FeatureMatrix(crow=crow, col=torch.tensor([1, 4, 9, 0, 2]), val=torch.tensor([1.0, 0.0, 2.0, 0.0, 3.0],
                                                                                      dtype=torch.float64), ncols=10)
    r = K.canonical_csr(fm)
    assert r.crow.tolist() == [0, 2, 2, 3] and r.col.tolist() == [1, 9, 2] and r.val.tolist() == [1.0, 2.0, 3.0]
    assert r.col.dtype == torch.int64 and r.ncols == 10 and r.nrows == 3 and r.nnz == 3
    # unsorted rows are sorted, the values move with their columns
    fm = FeatureMatrix(crow=crow, col=torch.tensor([9, 1, 4, 2, 0]), val=torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0],
                                                                                      dtype=torch.float64), ncols=10)
    r = K.canonical_csr(fm)
    assert r.crow.tolist() == [0, 3, 3, 5] and r.col.tolist() == [1, 4, 9, 0, 2]
    assert r.val.tolist() == [2.0, 3.0, 1.0, 5.0, 4.0]
    # a column twice in a row: not device-eligible (a dropped zero does not count)
    fm = FeatureMatrix(crow=crow, col=torch.tensor([4, 1, 4, 0, 2]), val=torch.ones(5, dtype=torch.float64), ncols=10)
    assert K.canonical_csr(fm) is None
    fm = FeatureMatrix(crow=crow, col=torch.tensor([4, 1, 4, 0, 2]), val=torch.tensor([0.0, 1.0, 1.0, 1.0, 1.0],
                                                                                      dtype=torch.float64), ncols=10)
    assert K.canonical_csr(fm).col.tolist() == [1, 4, 0, 2]
    # more columns than MinHash's 32-bit arithmetic takes
    fm = FeatureMatrix(crow=crow, col=torch.tensor([1, 4, 9, 0, 2]), val=torch.ones(5, dtype=torch.float64),
                       ncols=2 ** 31)
    assert K.canonical_csr(fm) is None
    # a dense block through nonzero; NaN != 0 stays
    X = torch.tensor([[0.0, 1.5, 0.0, float("nan")], [0.0, 0.0, 0.0, 0.0], [-2.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    r = K.canonical_csr(FeatureMatrix(X))
    assert r.crow.tolist() == [0, 2, 2, 3] and r.col.tolist() == [1, 3, 0] and r.ncols == 4
    assert r.val[0] == 1.5 and bool(torch.isnan(r.val[1])) and r.val[2] == -2.0
    # the same rows as the host path's
    left, _ = H.near_duplicates()
    rows = L._Rows(H.vectors(left))
    r = K.canonical_csr(H.csr(left))
    assert np.array_equal(r.crow.numpy(), rows.ptr) and np.array_equal(r.col.numpy(), rows.idx)
    assert np.array_equal(r.val.numpy(), rows.val)


@pytest.mark.parametrize("n", [1, 2, 3, 1000])
def test_next_gaussians_bit_equal(n):
    for burn in (0, 1):                             # 1: a cached second value waits when the batch starts
        a, b = JavaRandom(42 + n), JavaRandom(42 + n)
        for _ in range(burn):
            assert a.nextGaussian() == b.nextGaussian()
        want = np.asarray([a.nextGaussian() for _ in range(n)])
        got = b.nextGaussians(n)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64))
        assert a.nextDouble() == b.nextDouble()
        assert a.nextGaussian() == b.nextGaussian()
        assert a.nextGaussian() == b.nextGaussian() and a._seed == b._seed
    assert JavaRandom(1).nextGaussians(0).shape == (0,)


def test_brp_directions_unchanged():
    """``BucketRandomProjectionLSH(0, 5, 2, 2, 1.0)`` draws through ``nextGaussians`` what the loop of single calls
    drew (``tests/test_distance.py`` pins its hashes)."""
    brp = L.BucketRandomProjectionLSH(0, 5, 2, 2, 1.0)
    rnd = JavaRandom(0)
    for i in range(2):
        for j in range(2):
            d = np.asarray([rnd.nextGaussian() for _ in range(5)])
            assert np.array_equal(brp.R[i, j], d / np.linalg.norm(d))
            assert brp.r[i, j] == rnd.nextDouble() * 1.0


def test_device_selected_rule(monkeypatch):
    assert K.device_selected("cpu") is False
    monkeypatch.setenv("ALINK_LSH_HIP", "0")
    assert K.device_selected("cuda:0") is False     # switched off before the library is asked for


def _env_device():
    from alink_amd.common.mlenv import MLEnvironmentFactory
    return MLEnvironmentFactory.getDefault().device


def _host_join(left, right, distance, thr, P=2, T=3, width=2.0):
    res = L.approx_similarity_join(left, right, distance, 7, P, T, width, thr, _env_device())
    return [(a, b, d) for a, b, d in res]


def _host_topn(left, right, distance, n, P=2, T=3, width=2.0):
    return [(q, d, x, r) for q, d, x, r in
            L.approx_nearest_neighbors(right, left, distance, 7, P, T, width, n, _env_device(),
                                       lsh_basis_vecs=left)]


@pytest.mark.parametrize("how", ["cpu_env", "switched_off"])
def test_operators_keep_the_host_path(how, monkeypatch):
    """On the CPU device, or with ``ALINK_LSH_HIP=0``, the operators return what the host functions return: the
    rows, their order and every bit of the distances."""
    from alink_amd import useLocalEnv
    if how == "cpu_env":
        useLocalEnv(1, device="cpu")
    else:
        monkeypatch.setenv("ALINK_LSH_HIP", "0")
    calls = K.LSH_CALLS
    left, right = H.near_duplicates()
    lv, rv = H.vectors(left), H.vectors(right)
    got = H.run_join(H.table(lv), H.table(rv, 1000), "JACCARD", 0.5)
    want = _host_join(lv, rv, "JACCARD", 0.5)
    assert len(want) > 50 and got == [(a, 1000 + b, d) for a, b, d in want]
    got = H.run_topn(H.table(lv), H.table(rv, 1000), "JACCARD", 3)
    want = _host_topn(lv, rv, "JACCARD", 3)
    assert len(want) > 50 and got == [(1000 + q, d, x, r) for q, d, x, r in want]
    dl, dr = H.noisy_copies(33)
    got = H.run_join(H.table(dl), H.table(dr, 1000), "EUCLIDEAN", 0.5)
    want = _host_join(list(dl), list(dr), "EUCLIDEAN", 0.5)
    assert len(want) > 50 and got == [(a, 1000 + b, d) for a, b, d in want]
    got = H.run_topn(H.table(dl), H.table(dr, 1000), "EUCLIDEAN", 2)
    want = _host_topn(list(dl), list(dr), "EUCLIDEAN", 2)
    assert len(want) > 50 and got == [(1000 + q, d, x, r) for q, d, x, r in want]
    assert K.LSH_CALLS == calls
