"""Sparse-vector KMeans without a GPU: the torch path of ``ops/kmeans_sparse.py`` (the oracle of the GPU tests),
``train_kmeans`` on CSR rows, the operators and the selection rule.

Tolerance (derived, not tuned): two fp64 evaluations of a sum over ``m`` terms differ by at most
``2 m 2^-53 sum|terms|``; the tests allow 4x that, computed from the data.  For a distance ``m = nnz_row + 2`` with
the terms ``x_j c_j``, ``|x|^2`` and ``|c|^2``; for a column sum ``m`` is the column's entry count.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kmeans_sparse_dist import blob_init, sparse_blobs
from test_distributed import _free_port

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -53


def _fm(crow, col, val, d, col_dtype=torch.int64):
    from alink_amd.models.common.features import FeatureMatrix
    return FeatureMatrix(crow=torch.from_numpy(crow), col=torch.from_numpy(col).to(col_dtype),
                         val=torch.from_numpy(val), ncols=d)


def _densify(crow, col, val, d):
    out = np.zeros((len(crow) - 1, d))
    rid = np.repeat(np.arange(len(crow) - 1), np.diff(crow))
    ok = col < d
    out[rid[ok], col[ok]] = val[ok]
    return out


def _edge_rows(integer, n=257, d=1500, seed=4):
    """Row 0 empty, row 1 one entry, every fifth row stores column d - 1, every seventh an entry past d."""
    rng = np.random.default_rng(seed)
    cols, cnt = [], []
    for r in range(n):
        ln = 0 if r == 0 else 1 if r == 1 else int(rng.integers(2, 40))
        c = set(rng.choice(d - 1, size=ln, replace=False).tolist())
        if r % 5 == 2:
            c.add(d - 1)
        if r % 7 == 3:
            c.add(d + 11)
        cols.append(np.sort(np.fromiter(c, dtype=np.int64, count=len(c))))
        cnt.append(len(c))
    crow = np.zeros(n + 1, np.int64)
    crow[1:] = np.cumsum(cnt)
    col = np.concatenate(cols)
    val = rng.integers(-4, 5, size=col.size).astype(np.float64) if integer else rng.normal(size=col.size)
    return crow, col, val


@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
@pytest.mark.parametrize("k", [1, 3, 65])
def test_torch_reference_against_densified(k, dist):
    from alink_amd.ops import kmeans_sparse as ksp
    n, d = 257, 1500
    crow, col, val = _edge_rows(False)
    X = _densify(crow, col, val, d)
    C = np.random.default_rng(k).normal(size=(k, d)) * 0.5
    if dist == "COSINE":
        nrm = np.linalg.norm(X, axis=1, keepdims=True)
        safe = np.where(nrm > 0, nrm, 1)
        X = X / safe
        val = val / safe[np.repeat(np.arange(n), np.diff(crow)), 0]
        C = C / np.linalg.norm(C, axis=1, keepdims=True)
        ref = 1.0 - np.stack([(X * c[None]).sum(1) for c in C], 1)
    else:
        ref = np.stack([((X - c[None]) ** 2).sum(1) for c in C], 1)
    terms = np.abs(X) @ np.abs(C).T + (X * X).sum(1, keepdims=True) + (C * C).sum(1)[None, :]
    bound = 4.0 * 2.0 * (np.diff(crow) + 2.0)[:, None] * EPS * terms
    if k > 1:       # the data is away from ties beyond the bound; under COSINE the empty row is equidistant from all
        two = np.sort(ref, 1)[:, :2]
        sure = np.diff(crow) > 0 if dist == "COSINE" else np.ones(n, bool)
        assert ((two[:, 1] - two[:, 0]) > 2.0 * bound.max(1))[sure].all()
    for col_dtype in (torch.int32, torch.int64):
        fm = _fm(crow, col, val, d, col_dtype)
        idx, best = ksp.nearest(fm, torch.from_numpy(C), dist)
        idx, best = idx.numpy(), best.numpy()
        rows = np.arange(n)
        assert (ref[rows, idx] - ref.min(1) <= bound[rows, idx]).all()                 # the assignment is optimal
        assert (np.abs(best - ref.min(1)) <= bound[rows, ref.argmin(1)]).all()
        assert np.array_equal(ksp.nearest_counts(fm, torch.from_numpy(C), dist).numpy(), np.bincount(idx, minlength=k))
    assert idx[0] == ((C * C).sum(1).argmin() if dist == "EUCLIDEAN" else 0)            # the empty row
    buf = ksp.assign_accumulate(fm, torch.from_numpy(C), dist).numpy()
    want = np.zeros((k, d))
    np.add.at(want, idx, X)
    absum = np.zeros((k, d))
    np.add.at(absum, idx, np.abs(X))
    m = np.bincount(col[col < d], minlength=d).astype(np.float64)
    assert (np.abs(buf[:, :d] - want) <= 4.0 * 2.0 * m[None, :] * EPS * absum).all()
    assert np.array_equal(buf[:, d], np.bincount(idx, minlength=k).astype(np.float64))


@pytest.mark.parametrize("k", [1, 3, 65])
def test_torch_sums_of_integer_data_are_exact(k):
    from alink_amd.ops import kmeans_sparse as ksp
    d = 1500
    crow, col, val = _edge_rows(True)
    X = _densify(crow, col, val, d)
    C = torch.from_numpy(np.random.default_rng(k).normal(size=(k, d)))
    fm = _fm(crow, col, val, d)
    idx = ksp.nearest(fm, C, "EUCLIDEAN")[0].numpy()
    buf = ksp.assign_accumulate(fm, C, "EUCLIDEAN").numpy()
    want = np.zeros((k, d + 1))
    np.add.at(want[:, :d], idx, X)
    want[:, d] = np.bincount(idx, minlength=k)
    assert np.array_equal(buf, want)                # sums of small integers are exact in fp64: bit for bit


def test_take_dense_and_row_norms():
    from alink_amd.ops import kmeans_sparse as ksp
    d = 1500
    crow, col, val = _edge_rows(False)
    X = _densify(crow, col, val, d)
    fm = _fm(crow, col, val, d, torch.int32)
    pick = torch.tensor([5, 0, 1, 256, 5])
    assert np.array_equal(ksp.take_dense(fm, pick).numpy(), X[pick.numpy()])
    sq = (X * X).sum(1)
    assert (np.abs(ksp.row_sqnorm(fm).numpy() - sq) <= 4.0 * 2.0 * np.diff(crow) * EPS * sq).all()


@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
def test_train_sparse_matches_densified(dist):
    from alink_amd import useLocalEnv
    from alink_amd.models.clustering.kmeans import KMeansModelDataConverter, train_kmeans
    n, d, k = 300, 5000, 3
    crow, col, val = sparse_blobs(n, d, k)
    X = _densify(crow, col, val, d)
    init = torch.from_numpy(blob_init(col, d, k))
    if dist == "COSINE":
        init = init / init.norm(dim=1, keepdim=True)
    env = useLocalEnv(1, device="cpu")
    rows_s, qs = train_kmeans(_fm(crow, col, val, d), k, 20, 1e-6, dist, "RANDOM", 2, "v", env,
                              init_centroids=init.clone())
    rows_d, qd = train_kmeans(torch.from_numpy(X), k, 20, 1e-6, dist, "RANDOM", 2, "v", env,
                              init_centroids=init.clone())
    assert qs.step_no == qd.step_no                                  # the same number of supersteps
    a, b = KMeansModelDataConverter().load(rows_s), KMeansModelDataConverter().load(rows_d)
    assert a.centroids.shape == (k, d) and np.array_equal(a.weights, b.weights)
    assert sorted(a.weights.tolist()) == [100.0, 100.0, 100.0]
    # every centroid coordinate is a mean of at most n terms of size <= max(1, max|x|), or that mean normalised
    atol = 4.0 * 2.0 * n * EPS * max(1.0, float(np.abs(val).max()))
    assert np.abs(a.centroids - b.centroids).max() <= atol


def _limit_densify(monkeypatch, limit=4096):
    """vector_block / to_dense raise when asked for more than ``limit`` rows x columns."""
    from alink_amd.common.linalg.block import SparseBlock
    from alink_amd.common.table import MTable
    from alink_amd.models.common.features import FeatureMatrix
    vb, sb, fd = MTable.vector_block, SparseBlock.to_dense, FeatureMatrix.to_dense

    def vector_block(self, *a, **k):
        out = vb(self, *a, **k)
        if out.numel() > limit:
            raise AssertionError(f"MTable.vector_block densified {tuple(out.shape)}")
        return out

    def block_to_dense(self, *a, **k):
        if len(self) * self.size > limit:
            raise AssertionError(f"SparseBlock.to_dense asked for {len(self)} x {self.size}")
        return sb(self, *a, **k)

    def fm_to_dense(self, d=None):
        if self.nrows * (self.ncols if d is None else d) > limit:
            raise AssertionError(f"FeatureMatrix.to_dense asked for {self.nrows} x {d or self.ncols}")
        return fd(self, d)

    monkeypatch.setattr(MTable, "vector_block", vector_block)
    monkeypatch.setattr(SparseBlock, "to_dense", block_to_dense)
    monkeypatch.setattr(FeatureMatrix, "to_dense", fm_to_dense)


def _column(kind, crow, col, val, d):
    from alink_amd.common.linalg.block import SparseBlock
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    if kind == "block":
        c = Column(SparseBlock(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), d))
        return MTable(TableSchema(["v"], [Types.SPARSE_VECTOR]), [c])
    strs = ["$%d$" % d + " ".join("%d:%r" % (int(j), float(v)) for j, v in
                                   zip(col[crow[r]:crow[r + 1]], val[crow[r]:crow[r + 1]]))
            for r in range(len(crow) - 1)]
    return MTable(TableSchema(["v"], [Types.STRING]), [Column(strs)])


@pytest.mark.parametrize("kind", ["block", "strings"])
def test_operators_at_2_18_columns_never_densify(kind, monkeypatch):
    """Fails on a tree without the sparse path: training and prediction densify the column there."""
    from alink_amd import useLocalEnv, KMeansPredictBatchOp, KMeansTrainBatchOp
    from alink_amd.models.clustering.kmeans import KMeansModelDataConverter
    from alink_amd.operator.batch.source import TableSourceBatchOp
    n, d, k = 300, 1 << 18, 3
    crow, col, val = sparse_blobs(n, d, k)
    _limit_densify(monkeypatch)
    useLocalEnv(1, device="cpu")
    src = TableSourceBatchOp(_column(kind, crow, col, val, d))
    model = KMeansTrainBatchOp().setVectorCol("v").setK(k).setMaxIter(10).linkFrom(src)
    pred = KMeansPredictBatchOp().setPredictionCol("p").setPredictionDistanceCol("dist").linkFrom(model, src)
    md = KMeansModelDataConverter().load(model.getOutputTable().rows())
    assert int(md.params.get("vectorSize", int)) == d and md.centroids.shape[1] == d
    got = np.asarray(pred.getOutputTable().col("p").to_list())
    dist = np.asarray(pred.getOutputTable().col("dist").to_list())
    C = md.centroids
    cn = (C * C).sum(1)
    for r in range(n):
        j, v = col[crow[r]:crow[r + 1]], val[crow[r]:crow[r + 1]]
        d2 = (v * v).sum() + cn - 2.0 * (C[:, j] * v[None, :]).sum(1)          # sparse: the stored entries only
        assert md.ids[int(np.argmin(d2))] == got[r]
        # m = nnz + 2 terms, sum|terms| <= |x|^2 + |c|^2 + sum|x_j c_j|, compared as squared distances
        b = 4.0 * 2.0 * (len(j) + 2) * EPS * ((v * v).sum() + cn.max() + np.abs(C[:, j] * v[None, :]).sum(1).max())
        assert abs(dist[r] ** 2 - d2.min()) <= b


def _train_rows(mt, dist, init, flag, monkeypatch):
    from alink_amd import useLocalEnv, KMeansTrainBatchOp
    from alink_amd.models.clustering.kmeans import KMeansModelDataConverter
    from alink_amd.operator.batch.source import TableSourceBatchOp
    from alink_amd.ops import kmeans_sparse as ksp
    monkeypatch.setenv("ALINK_KMEANS_SPARSE", flag)
    useLocalEnv(1, device="cpu")
    seen = []
    orig = ksp.assign_accumulate
    monkeypatch.setattr(ksp, "assign_accumulate", lambda *a, **k: (seen.append(1), orig(*a, **k))[1])
    op = KMeansTrainBatchOp().setVectorCol("v").setK(3).setMaxIter(20).setDistanceType(dist).setInitMode(init) \
        .linkFrom(TableSourceBatchOp(mt))
    monkeypatch.setattr(ksp, "assign_accumulate", orig)
    assert bool(seen) == (flag == "1")
    return KMeansModelDataConverter().load(op.getOutputTable().rows())


@pytest.mark.parametrize("init", ["RANDOM", "K_MEANS_PARALLEL"])
@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
def test_forced_sparse_equals_densified_model(dist, init, monkeypatch):
    """d = 1000 is below the rule's threshold: ``ALINK_KMEANS_SPARSE=1`` forces the sparse path, ``=0`` densifies."""
    n, d = 300, 1000
    crow, col, val = sparse_blobs(n, d)
    mt = _column("block", crow, col, val, d)
    a = _train_rows(mt, dist, init, "1", monkeypatch)
    b = _train_rows(mt, dist, init, "0", monkeypatch)
    assert a.centroids.shape == b.centroids.shape and np.array_equal(a.weights, b.weights)
    atol = 4.0 * 2.0 * n * EPS * max(1.0, float(np.abs(val).max()))
    assert np.abs(a.centroids - b.centroids).max() <= atol


def test_forced_sparse_at_5000_columns(monkeypatch):
    n, d = 300, 5000
    crow, col, val = sparse_blobs(n, d)
    mt = _column("strings", crow, col, val, d)
    a = _train_rows(mt, "EUCLIDEAN", "K_MEANS_PARALLEL", "1", monkeypatch)
    b = _train_rows(mt, "EUCLIDEAN", "K_MEANS_PARALLEL", "0", monkeypatch)
    assert np.array_equal(a.weights, b.weights)
    assert np.abs(a.centroids - b.centroids).max() <= 4.0 * 2.0 * n * EPS * max(1.0, float(np.abs(val).max()))


def test_predict_detail_distance_and_null_rows(monkeypatch):
    """Sparse prediction with every output column equals the densified prediction; a null row stays null."""
    from alink_amd import useLocalEnv, KMeansPredictBatchOp
    from alink_amd.common.linalg import VectorUtil
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    from alink_amd.models.clustering.kmeans import KMeansModelDataConverter, train_kmeans
    from alink_amd.operator.batch.source import TableSourceBatchOp
    from alink_amd.ops import kmeans_sparse as ksp
    n, d, k = 60, 1000, 3
    crow, col, val = sparse_blobs(n, d, k)
    strs = _column("strings", crow, col, val, d).col("v").to_list()
    strs[7] = None
    mt = MTable(TableSchema(["v"], [Types.STRING]), [Column(strs)])
    outs = {}
    for dist in ("EUCLIDEAN", "COSINE"):
        env = useLocalEnv(1, device="cpu")
        rows, _ = train_kmeans(_fm(crow, col, val, d), k, 5, 1e-6, dist, "RANDOM", 2, "v", env,
                               init_centroids=torch.from_numpy(blob_init(col, d, k)))
        model = TableSourceBatchOp(MTable.from_rows(rows, KMeansModelDataConverter().getModelSchema(), replicated=True))
        for flag in ("1", "0"):
            monkeypatch.setenv("ALINK_KMEANS_SPARSE", flag)
            calls = []
            orig = ksp.nearest
            monkeypatch.setattr(ksp, "nearest", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
            t = KMeansPredictBatchOp().setPredictionCol("p").setPredictionDetailCol("det") \
                .setPredictionDistanceCol("dist").linkFrom(model, TableSourceBatchOp(mt)).getOutputTable()
            monkeypatch.setattr(ksp, "nearest", orig)
            assert bool(calls) == (flag == "1")
            outs[flag] = (t.col("p").to_list(), t.col("det").to_list(), t.col("dist").to_list())
        (p1, det1, dist1), (p0, det0, dist0) = outs["1"], outs["0"]
        assert p1 == p0 and p1[7] is None and det1[7] is None and dist1[7] is None
        for i in range(n):
            if i == 7:
                continue
            # distances of size <= 10 and probabilities in [0, 1] from sums of at most 12 terms of size <= 4
            assert abs(dist1[i] - dist0[i]) <= 4.0 * 2.0 * 12 * EPS * 4 * 10
            np.testing.assert_allclose(VectorUtil.getVector(det1[i]).data, VectorUtil.getVector(det0[i]).data,
                                       rtol=0, atol=4.0 * 2.0 * 12 * EPS * 4 * 10)


def test_selection_rule(monkeypatch):
    from alink_amd.ops import kmeans_sparse as ksp
    monkeypatch.delenv("ALINK_KMEANS_SPARSE", raising=False)
    assert ksp.sparse_selected(True, 1025) and not ksp.sparse_selected(True, 1024)
    assert not ksp.sparse_selected(False, 1 << 18)
    monkeypatch.setenv("ALINK_KMEANS_SPARSE", "1")
    assert ksp.sparse_selected(True, 8) and not ksp.sparse_selected(False, 8)
    monkeypatch.setenv("ALINK_KMEANS_SPARSE", "0")
    assert not ksp.sparse_selected(True, 1 << 18)


def test_text_pipeline_both_ways(monkeypatch):
    """DocHashCountVectorizer(numFeatures=2048) -> KMeans(COSINE): sparse and densified runs predict alike."""
    import alink_amd as A
    from alink_amd.operator.batch.source import MemSourceBatchOp
    rng = np.random.default_rng(8)
    topics = [["gpu", "kernel", "wave", "lane", "register"], ["river", "forest", "mountain", "lake", "trail"],
              ["violin", "piano", "chord", "melody", "tempo"]]
    docs = [(i, " ".join(rng.choice(topics[i % 3], size=8).tolist())) for i in range(90)]
    preds = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("ALINK_KMEANS_SPARSE", flag)
        A.useLocalEnv(1, device="cpu")
        data = MemSourceBatchOp(docs, ["id", "text"])
        vec = A.DocHashCountVectorizer().setSelectedCol("text").setNumFeatures(2048).setOutputCol("v").fit(data) \
            .transform(data)
        out = A.KMeans().setVectorCol("v").setK(3).setDistanceType("COSINE").setPredictionCol("p").fit(vec) \
            .transform(vec).select(["id", "p"]).collect()
        preds[flag] = [int(r[1]) for r in sorted(out, key=lambda r: r[0])]
    assert preds["1"] == preds["0"]
    assert len({(i % 3, p) for i, p in enumerate(preds["1"])}) == 3      # the three topics are recovered


def _run(world, tmp_path, dist):
    port = _free_port()
    env = dict(os.environ)
    env.update({"ALINK_TEST_TMP": str(tmp_path), "ALINK_TEST_DIST": dist})
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("ALINK_KMEANS_SPARSE", None)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "kmeans_sparse_dist.py"), str(r), str(world),
                               str(port), "kmeans_sparse", str(tmp_path)], env=env) for r in range(world)]
    for p in procs:
        p.wait(timeout=300)
    outs = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), f"kmeans_sparse_{world}_{r}.json")) as f:
            o = json.load(f)
        assert "error" not in o, o.get("error")
        outs.append(o)
    return outs


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    return _run(1, tmp_path_factory.mktemp("sparse_one"), "EUCLIDEAN")[0]       # shared, read-only


@pytest.mark.parametrize("world", [2, 3])
def test_sparse_kmeans_ranks_equal_single(world, one_rank, tmp_path):
    """2 ranks, and 3 ranks of which the last holds no rows, give the 1-rank sparse model."""
    one = one_rank
    many = _run(world, tmp_path, "EUCLIDEAN")
    assert one["sparse_steps"] > 0 and all(o["sparse_steps"] > 0 for o in many if o["rows"])
    assert all(o["model"] == many[0]["model"] for o in many)
    c1 = [json.loads(r[1]) for r in one["model"][1:]]
    c2 = [json.loads(r[1]) for r in many[0]["model"][1:]]
    assert len(c1) == len(c2) == 3
    for a, b in zip(c1, c2):
        np.testing.assert_allclose(a["vec"]["data"], b["vec"]["data"], atol=1e-9)
        assert a["weight"] == b["weight"]
