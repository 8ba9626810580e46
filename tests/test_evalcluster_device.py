"""Cluster evaluation on the row kinds (``ops/evalcluster.py``, ``models/evaluation/cluster.py``), on the CPU: the
torch implementation of the three passes against the numpy reference of ``evalcluster_helpers.py`` (its bounds are
derived in that module's docstring), the operator on a sparse column that is never densified, and the columnar
prediction / label path against the per-row one.  ``ALINK_EVALCLUSTER_HIP=0`` is the oracle of the operator tests.
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


def _csr_rows(case, device="cpu", idx_dtype=torch.int64):
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops.kmeans_rows import rows
    crow, col, val = case[:3]
    fm = FeatureMatrix(crow=torch.from_numpy(crow).to(device), col=torch.from_numpy(col).to(device, idx_dtype),
                       val=torch.from_numpy(val).to(device), ncols=NCOLS)
    return rows(fm, "EUCLIDEAN")


def _wide_mean(case, device="cpu"):
    cols, mean_n = case[4], case[6]
    mean = torch.zeros((mean_n.shape[0], NCOLS), dtype=torch.float64, device=device)
    mean[:, torch.from_numpy(cols).to(device)] = torch.from_numpy(mean_n).to(device)
    return mean


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("d,k", [(1, 2), (5, 1), (33, 17), (131, 65)])
def test_torch_passes_equal_numpy_dense(d, k, dist):
    from alink_amd.ops import evalcluster as ev
    from alink_amd.ops.kmeans_rows import rows
    X, cid, mean, cnt, n2, ref = H.dense_case(d, k, dist)
    r = rows(torch.from_numpy(X), "EUCLIDEAN")
    ct = torch.from_numpy(cid).to(torch.int32)
    assert ev.sorted_work(r, ct, k) is None                 # no sort on the torch kinds
    sums = ev.cluster_sums(r, ct, k).numpy()
    tol = 4 * 2 * len(X) * H.EPS * np.abs(X).max() * np.maximum(cnt, 1.0)[:, None]
    assert np.all(np.abs(sums[:, :d] - mean * cnt[:, None]) <= tol)
    assert np.array_equal(sums[:, d], cnt) and np.allclose(sums[:, d + 1], n2, rtol=1e-12, atol=0)
    block = ev.row_pass(r, ct, torch.from_numpy(mean), torch.from_numpy(cnt), torch.from_numpy(n2), dist)
    assert block.dtype == torch.float64 and tuple(block.shape) == (len(X), 3)
    H.check_block(block.numpy(), ref)
    rs = ev.cluster_row_sums(block, ct, k).numpy()
    want = np.zeros((k, 3))
    np.add.at(want, cid[ref.ok], block.numpy()[ref.ok])
    assert np.allclose(rs, want, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("k", [1, 65])
def test_torch_passes_equal_numpy_csr(k, dist, monkeypatch):
    """CSR rows of 2^18 columns on the CPU: chunked products, never a dense matrix."""
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import evalcluster as ev
    monkeypatch.setattr(FeatureMatrix, "to_dense", lambda *a, **kw: pytest.fail("densified"))
    monkeypatch.setattr(ev, "SPARSE_CHUNK", 100)            # several chunks
    case = H.csr_case(k, dist)
    cid, Xn, mean_n, cnt, n2, ref = case[3], case[5], case[6], case[7], case[8], case[9]
    r = _csr_rows(case)
    ct = torch.from_numpy(cid).to(torch.int32)
    sums = ev.cluster_sums(r, ct, k)
    cols = torch.from_numpy(case[4])
    assert np.allclose(sums[:, cols].numpy(), mean_n * cnt[:, None], rtol=1e-12, atol=1e-13)
    assert float(sums[:, :NCOLS].abs().sum() - sums[:, cols].abs().sum()) == 0.0     # nothing outside the pool
    assert np.array_equal(sums[:, NCOLS].numpy(), cnt) and np.allclose(sums[:, NCOLS + 1].numpy(), n2, rtol=1e-12)
    block = ev.row_pass(r, ct, _wide_mean(case), torch.from_numpy(cnt), torch.from_numpy(n2), dist)
    H.check_block(block.numpy(), ref, rearranged_euclid=dist == "EUCLIDEAN")


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("dist", DISTS)
def test_operator_equals_reference_formulas(dist, sparse, monkeypatch):
    """The operator through the torch passes against the reference's formulas in numpy, on dense rows and on the
    same rows taken as CSR (``ALINK_KMEANS_SPARSE=1``)."""
    from alink_amd.models.evaluation.metrics import ClusterMetrics  # noqa: F401
    monkeypatch.delenv("ALINK_EVALCLUSTER_HIP", raising=False)
    X, cid = H.separated(n=60, d=3)
    if sparse:
        monkeypatch.setenv("ALINK_KMEANS_SPARSE", "1")
        n, d = X.shape
        mt = H.sparse_table(np.arange(n + 1, dtype=np.int64) * d, np.tile(np.arange(d), n), X.reshape(-1).copy(), d,
                            cid)
    else:
        mt = H.dense_table(X, cid)
    got = H.evaluate(mt, dist)
    names = {"Ssb": "SSB", "Ssw": "SSW", "Compactness": "compactness", "SilhouetteCoefficient": "silhouetteCoefficient"}
    for name, v in H.ref_cluster_metrics(X, cid, dist).items():
        assert float(got[names[name]]) == pytest.approx(v, rel=1e-9, abs=1e-12), name


@pytest.mark.parametrize("dist", DISTS)
def test_sparse_column_of_2_18_features_is_not_densified(dist, monkeypatch):
    """300 documents of about 20 entries under 2^18 features, k = 4: the operator takes them as CSR rows
    (``FeatureMatrix.to_dense`` raises here) and gives the metrics of the same rows at a vector size of 600 with the
    columns remapped, evaluated by the ``ALINK_EVALCLUSTER_HIP=0`` path."""
    from alink_amd.models.common.features import FeatureMatrix
    crow, col, val, cid, cols = H.sparse_docs()
    narrow = H.sparse_table(crow, np.searchsorted(cols, col), val, 600, cid)
    monkeypatch.setenv("ALINK_EVALCLUSTER_HIP", "0")
    want = H.evaluate(narrow, dist)
    monkeypatch.delenv("ALINK_EVALCLUSTER_HIP")

    def no_dense(self, d=None):
        raise AssertionError("the sparse column was densified")
    monkeypatch.setattr(FeatureMatrix, "to_dense", no_dense)
    got = H.evaluate(H.sparse_table(crow, col, val, NCOLS, cid), dist)
    assert got["k"] == "4" and got["count"] == "300"
    H.assert_metrics_equal(got, want)


def _id_tables(pred, pnull, label, lnull, X):
    """The same table twice: tensor columns with null masks, and plain lists with None."""
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    n = len(pred)
    s = TableSchema(["v", "p", "l"], [Types.DENSE_VECTOR, Types.LONG, Types.LONG])
    to_list = lambda v, m: [None if m[i] else int(v[i]) for i in range(n)]  # noqa: E731
    vec = Column(torch.from_numpy(X))
    return (MTable(s, [vec, Column(pred, pnull if pnull.any() else None), Column(label, lnull if lnull.any() else None)]),
            MTable(s, [vec, Column(to_list(pred, pnull)), Column(to_list(label, lnull))]))


@pytest.mark.parametrize("nulls", ["none", "pred", "label", "both"])
def test_columnar_ids_equal_the_python_loop(nulls, monkeypatch):
    """Integer tensor columns take the device path (``torch.unique``, a lookup, one ``bincount``); lists take the
    per-row loop.  Ids 2 and 10 check the string order ("10" < "2"); null fill values (0 and 99) are no ids."""
    monkeypatch.delenv("ALINK_EVALCLUSTER_HIP", raising=False)
    g = torch.Generator().manual_seed(5)
    n = 400
    ids = torch.tensor([2, 10, 7, 33])
    pred = ids[torch.randint(0, 4, (n,), generator=g)]
    label = torch.tensor([1, 20, 3])[torch.randint(0, 3, (n,), generator=g)]
    pnull = (torch.rand(n, generator=g) < 0.1) & torch.tensor(nulls in ("pred", "both"))
    lnull = (torch.rand(n, generator=g) < 0.1) & torch.tensor(nulls in ("label", "both"))
    pred = torch.where(pnull, torch.tensor(99), pred)       # what a null holds must not become an id
    label = torch.where(lnull, torch.tensor(0), label)
    X = np.random.default_rng(2).normal(size=(n, 4)) + 3.0 * np.eye(4)[np.searchsorted([2, 7, 10, 33], pred.clamp_max(33).numpy())]
    tensors, lists = _id_tables(pred, pnull, label, lnull, X)
    got = H.evaluate(tensors, "EUCLIDEAN", label=True)
    loop = H.evaluate(lists, "EUCLIDEAN", label=True)
    assert got == loop
    assert got["clusterArray"] == '["10","2","33","7"]' and got["count"] == str(int((~pnull).sum()))
    monkeypatch.setenv("ALINK_EVALCLUSTER_HIP", "0")
    H.assert_metrics_equal(got, H.evaluate(lists, "EUCLIDEAN", label=True))
    # without a vector column: counts and the contingency metrics alone
    from alink_amd import EvalClusterBatchOp
    from alink_amd.operator.batch.source import TableSourceBatchOp
    monkeypatch.delenv("ALINK_EVALCLUSTER_HIP")
    outs = [EvalClusterBatchOp().setPredictionCol("p").setLabelCol("l").linkFrom(TableSourceBatchOp(t)).collect()[0][0]
            for t in (tensors, lists)]
    assert outs[0] == outs[1]


def test_flag_and_counter(monkeypatch):
    """On the CPU nothing is launched, whatever the flag says."""
    from alink_amd.ops import evalcluster as ev
    X, cid = H.separated(n=60, d=3)
    calls = ev.EVALCLUSTER_CALLS
    for flag in ("0", "1"):
        monkeypatch.setenv("ALINK_EVALCLUSTER_HIP", flag)
        H.evaluate(H.dense_table(X, cid), "EUCLIDEAN")
    assert ev.EVALCLUSTER_CALLS == calls
