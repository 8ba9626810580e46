"""The cluster evaluation kernels (``ops/csrc/evalcluster.hip`` through ``ops/evalcluster.py``) and
``EvalClusterBatchOp`` on the GPU.

Kernel level: the oracle is the fp64 numpy reference of ``evalcluster_helpers.py`` on the host.  Tolerances are
derived there, not tuned: a dot of d terms ``2 d 2^-53 sum|x_j m_j|``; the direct EUCLIDEAN / CITYBLOCK ``own``
``(d + 4) 2^-53`` relative; the COSINE ``own`` from the dot's bound over ``|x| |m|``; the CSR rearranged forms an
absolute ``T 2^-53 (|x|^2 + |m|^2)`` on ``own^2`` (CITYBLOCK: the 1-norms on ``own``) with the term count
``T = s + 8 nz + 8``; the silhouette from the ``dis`` bound through ``|d sil| <= E / (max(cur, nb) - E)``; 4x each,
the project's margin.  The generators keep ``own^2 >= 1e-3 (|x|^2 + |m|^2)`` and a well-conditioned silhouette, and
the helper asserts it.  Every case holds a cluster of one row and cids outside ``[0, k)`` (-1, k, k + 5), which must
give zero rows.  The 8-byte-aligned rows are a contiguous view that starts one element into its allocation.
Blocks of different grids, and sums of different runs, are compared with ``torch.equal``.
Non-finite rows are not guaranteed by the kernels and are not tested.

Operator level: ``EvalClusterBatchOp`` under a GPU env against the ``ALINK_EVALCLUSTER_HIP=0`` path run on the CPU,
every numeric metric within the operator's own figures (``rel=1e-9, abs=1e-12``), counts, k and the cluster array
exactly.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import evalcluster_helpers as H  # noqa: E402
from evalcluster_helpers import DISTS, NCOLS  # noqa: E402

pytestmark = pytest.mark.gpu

DS = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 128, 131, 300, 1024)
KS = (1, 2, 15, 16, 17, 64, 65, 130)
GRIDS = (0, 1, 7)


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _dense_rows(Xg):
    from alink_amd.ops.kmeans_rows import _Dense64Rows, rows
    r = rows(Xg, "EUCLIDEAN")
    assert isinstance(r, _Dense64Rows)
    return r


def _check_dense(d, k, dist, unaligned=False):
    from alink_amd.ops import evalcluster as ev
    X, cid, mean, cnt, n2, ref = H.dense_case(d, k, dist)
    Xg = _t(X)
    if unaligned:
        flat = torch.empty(X.size + 1, dtype=torch.float64, device="cuda")
        Xo = flat[1:].view(X.shape)
        Xo.copy_(Xg)
        assert Xo.data_ptr() % 16 == 8 and Xo.is_contiguous()
        Xg = Xo
    r = _dense_rows(Xg)
    ct = _t(cid, torch.int32)
    args = (_t(mean), _t(cnt), _t(n2), dist)
    calls = ev.EVALCLUSTER_CALLS
    block = ev.row_pass(r, ct, *args)
    assert ev.EVALCLUSTER_CALLS == calls + 1
    assert block.dtype == torch.float64 and tuple(block.shape) == (len(X), 3)
    H.check_block(block.cpu().numpy(), ref)
    for grid in GRIDS[1:]:
        assert torch.equal(ev.row_pass(r, ct, *args, grid=grid), block), (d, k, dist, grid)


@pytest.mark.parametrize("d", DS)
def test_dense_row_pass_equals_numpy(d):
    for k in KS:
        for dist in DISTS:
            _check_dense(d, k, dist)


@pytest.mark.parametrize("d", [2, 64, 130])
def test_dense_row_pass_unaligned_rows(d):
    """Even d on rows that start 8 bytes into an allocation: the 16-byte loads must not be taken."""
    for dist in DISTS:
        _check_dense(d, 17, dist, unaligned=True)


def _csr_rows(case, idx_dtype):
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops.kmeans_rows import _SparseRows, rows
    crow, col, val = case[:3]
    r = rows(FeatureMatrix(crow=_t(crow), col=_t(col, idx_dtype), val=_t(val), ncols=NCOLS), "EUCLIDEAN")
    assert isinstance(r, _SparseRows)
    return r


def _wide_mean(case):
    cols, mean_n = case[4], case[6]
    mean = torch.zeros((mean_n.shape[0], NCOLS), dtype=torch.float64, device="cuda")
    mean[:, _t(cols)] = _t(mean_n)
    return mean


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("k", [1, 64, 65, 129, 256, 300])
def test_csr_row_pass_equals_numpy(k, idx_dtype):
    """d = 2^18, empty rows, rows of 1 .. 130 entries in random stored order, entries outside [0, d) (-1, d,
    d + 7) that must add nothing; one, two, three (k = 129: the tail guard in the first pass of four blocks), four
    (k = 256: an exactly full pass) and (k = 300) five cluster blocks of 64."""
    from alink_amd.ops import evalcluster as ev
    for dist in DISTS:
        case = H.csr_case(k, dist)
        crow, col, cid, cnt, n2, ref = case[0], case[1], case[3], case[7], case[8], case[9]
        assert (np.diff(crow) == 0).any() and (col < 0).any() and (col >= NCOLS).any()
        r = _csr_rows(case, idx_dtype)
        ct = _t(cid, torch.int32)
        args = (_wide_mean(case), _t(cnt), _t(n2), dist)
        calls = ev.EVALCLUSTER_CALLS
        block = ev.row_pass(r, ct, *args)
        assert ev.EVALCLUSTER_CALLS == calls + 1
        H.check_block(block.cpu().numpy(), ref, rearranged_euclid=dist == "EUCLIDEAN")
        for grid in GRIDS[1:]:
            assert torch.equal(ev.row_pass(r, ct, *args, grid=grid), block), (k, dist, grid)


def test_cluster_sums_are_reproducible():
    """Two runs and every grid give ``torch.equal`` sums, for both kinds and for the block's sums; the values are
    those of numpy within the bound of a sum of n terms; the one sorted work list serves all of them."""
    from alink_amd.ops import evalcluster as ev
    X, cid, mean, cnt, n2, ref = H.dense_case(131, 17, "EUCLIDEAN")
    d, k = 131, 17
    r = _dense_rows(_t(X))
    ct = _t(cid, torch.int32)
    work = ev.sorted_work(r, ct, k)
    assert work is not None
    sums = ev.cluster_sums(r, ct, k, work)
    assert torch.equal(ev.cluster_sums(r, ct, k, work), sums) and torch.equal(ev.cluster_sums(r, ct, k), sums)
    for grid in GRIDS[1:]:
        assert torch.equal(ev.cluster_sums(r, ct, k, work, grid=grid), sums)
    s = sums.cpu().numpy()
    tol = 4 * 2 * len(X) * H.EPS * np.abs(X).max() * np.maximum(cnt, 1.0)[:, None]
    assert np.all(np.abs(s[:, :d] - mean * cnt[:, None]) <= tol) and np.array_equal(s[:, d], cnt)
    assert np.allclose(s[:, d + 1], n2, rtol=4 * 2 * (len(X) + d) * H.EPS, atol=0)
    block = ev.row_pass(r, ct, _t(mean), _t(cnt), _t(n2), "EUCLIDEAN")
    rs = ev.cluster_row_sums(block, ct, k, work)
    assert tuple(rs.shape) == (k, 3)
    assert torch.equal(ev.cluster_row_sums(block, ct, k, work), rs) and torch.equal(ev.cluster_row_sums(block, ct, k), rs)
    want = np.zeros((k, 3))
    np.add.at(want, cid[ref.ok], block.cpu().numpy()[ref.ok])
    assert np.allclose(rs.cpu().numpy(), want, rtol=4 * 2 * len(X) * H.EPS, atol=4 * 2 * len(X) * H.EPS)
    # CSR rows
    case = H.csr_case(65, "EUCLIDEAN")
    r = _csr_rows(case, torch.int64)
    ct = _t(case[3], torch.int32)
    work = ev.sorted_work(r, ct, 65)
    sums = ev.cluster_sums(r, ct, 65, work)
    assert torch.equal(ev.cluster_sums(r, ct, 65, work), sums) and torch.equal(ev.cluster_sums(r, ct, 65), sums)
    assert torch.equal(ev.cluster_sums(r, ct, 65, work, grid=7), sums)
    cols = _t(case[4])
    assert np.allclose(sums[:, cols].cpu().numpy(), case[6] * case[7][:, None], rtol=1e-12, atol=1e-13)
    assert np.array_equal(sums[:, NCOLS].cpu().numpy(), case[7])
    assert np.allclose(sums[:, NCOLS + 1].cpu().numpy(), case[8], rtol=1e-12)


def test_empty_partition_launches_nothing():
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import evalcluster as ev
    from alink_amd.ops.kmeans_rows import rows
    z = torch.zeros(0, dtype=torch.int64, device="cuda")
    fm = FeatureMatrix(crow=torch.zeros(1, dtype=torch.int64, device="cuda"), col=z,
                       val=torch.zeros(0, dtype=torch.float64, device="cuda"), ncols=37)
    mean = torch.ones((4, 37), dtype=torch.float64, device="cuda")
    one = torch.ones(4, dtype=torch.float64, device="cuda")
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    calls = ev.EVALCLUSTER_CALLS
    for r in (rows(torch.zeros((0, 37), dtype=torch.float64, device="cuda"), "EUCLIDEAN"), rows(fm, "EUCLIDEAN")):
        assert ev.sorted_work(r, empty, 4) is None
        assert torch.equal(ev.cluster_sums(r, empty, 4), torch.zeros((4, 39), dtype=torch.float64, device="cuda"))
        block = ev.row_pass(r, empty, mean, one, one, "COSINE")
        assert tuple(block.shape) == (0, 3)
        assert torch.equal(ev.cluster_row_sums(block, empty, 4), torch.zeros((4, 3), dtype=torch.float64, device="cuda"))
    assert ev.EVALCLUSTER_CALLS == calls


# ---------------------------------------------------------------------------------------------------- operator

@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("d", [3, 130])
def test_operator_dense_equals_host_path(d, dist, monkeypatch):
    from alink_amd.ops import evalcluster as ev
    monkeypatch.delenv("ALINK_KMEANS_DENSE64", raising=False)
    X, cid = H.separated(n=600, d=d)
    monkeypatch.setenv("ALINK_EVALCLUSTER_HIP", "0")
    want = H.evaluate(H.dense_table(X, cid), dist, "cpu")
    calls = ev.EVALCLUSTER_CALLS
    still = H.evaluate(H.dense_table(X, cid, "cuda"), dist, "cuda:0")       # =0 on the GPU: the host path, no launch
    assert ev.EVALCLUSTER_CALLS == calls
    H.assert_metrics_equal(still, want)
    monkeypatch.delenv("ALINK_EVALCLUSTER_HIP")
    got = H.evaluate(H.dense_table(X, cid, "cuda"), dist, "cuda:0")
    assert ev.EVALCLUSTER_CALLS == calls + 1
    assert got["k"] == "3" and got["count"] == "600" and got["clusterArray"] == '["0","1","2"]'
    H.assert_metrics_equal(got, want)


@pytest.mark.parametrize("dist", DISTS)
def test_operator_csr_equals_host_path_on_the_narrow_copy(dist, monkeypatch):
    """A CSR column of 2^18 features on the GPU; the oracle is the same rows at a vector size of 600 with the columns
    remapped, evaluated by the ``=0`` path on the CPU."""
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import evalcluster as ev
    monkeypatch.delenv("ALINK_KMEANS_SPARSE", raising=False)
    crow, col, val, cid, cols = H.sparse_docs()
    label = (cid + (np.arange(len(cid)) % 7 == 0)) % 4
    monkeypatch.setenv("ALINK_EVALCLUSTER_HIP", "0")
    want = H.evaluate(H.sparse_table(crow, np.searchsorted(cols, col), val, 600, cid, label=label), dist, "cpu",
                      label=True)
    monkeypatch.delenv("ALINK_EVALCLUSTER_HIP")

    def no_dense(self, d=None):
        raise AssertionError("the sparse column was densified")
    monkeypatch.setattr(FeatureMatrix, "to_dense", no_dense)
    calls = ev.EVALCLUSTER_CALLS
    got = H.evaluate(H.sparse_table(crow, col, val, NCOLS, cid, "cuda", label=label), dist, "cuda:0", label=True)
    assert ev.EVALCLUSTER_CALLS == calls + 1
    H.assert_metrics_equal(got, want)
