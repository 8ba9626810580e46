"""Sparse-vector KMeans on the GPU (``ops/csrc/kmeans_sparse.hip`` through ``ops/kmeans_sparse.py``).

Tolerance (derived, not tuned): two fp64 evaluations of a sum over ``m`` terms differ by at most
``2 m 2^-53 sum|terms|``; the tests allow 4x that, computed from the data.  For a distance ``m = nnz_row + 2`` with
the terms ``x_j c_j``, ``|x|^2`` and ``|c|^2``; for a column sum ``m`` is the column's entry count.  The data is
generated away from ties beyond that bound (checked), the duplicated centroid being the deliberate exception.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
N, D = 1003, 1500               # 1003 rows: not a multiple of the 4 waves of a workgroup
ROW_LENS = (0, 1, 63, 64, 65, 200)
KS = (1, 3, 64, 65, 100, 129, 256, 300)


def _fm(crow, col, val, d, device, col_dtype=torch.int64):
    from alink_amd.models.common.features import FeatureMatrix
    return FeatureMatrix(crow=torch.from_numpy(crow).to(device), col=torch.from_numpy(col).to(device, col_dtype),
                         val=torch.from_numpy(val).to(device), ncols=d)


@functools.lru_cache(maxsize=None)
def _rows():
    """CSR rows of lengths 0, 1, 63, 64, 65, 200 (cycled) over D columns; every tenth row also stores column
    D - 1, and every seventh row two columns past D (ignored)."""
    rng = np.random.default_rng(11)
    cols, vals, cnt = [], [], []
    for r in range(N):
        ln = ROW_LENS[r % len(ROW_LENS)]
        c = set(rng.choice(D - 1, size=ln, replace=False).tolist())
        if r % 10 == 3 and ln:
            c.add(D - 1)
        if r % 7 == 2 and ln:
            c.update((D + 5, D + 30))
        c = np.sort(np.fromiter(c, dtype=np.int64, count=len(c)))
        cols.append(c)
        vals.append(rng.normal(size=c.size))
        cnt.append(c.size)
    crow = np.zeros(N + 1, np.int64)
    crow[1:] = np.cumsum(cnt)
    col, val = np.concatenate(cols), np.concatenate(vals)
    dense = np.zeros((N, D))
    rid = np.repeat(np.arange(N), cnt)
    ok = col < D
    dense[rid[ok], col[ok]] = val[ok]
    return crow, col, val, dense


@functools.lru_cache(maxsize=None)
def _case(k, dist):
    """(crow, col, val, C, reference distances [N, k] on the GPU, bounds [N, k]); computed once per (k, dist)."""
    crow, col, val, dense = _rows()
    rng = np.random.default_rng(100 + k)
    C = rng.normal(size=(k, D)) * 0.5
    if k >= 3:
        C[0] *= 0.8                          # the smallest norm: the centroid most of the sparse rows choose
        C[k - 1] = C[0]                      # an exact duplicate: index 0 must win
    X = dense.copy()
    if dist == "COSINE":
        nrm = np.linalg.norm(X, axis=1, keepdims=True)
        X = np.where(nrm > 0, X / np.where(nrm > 0, nrm, 1), X)
        val = val / np.where(nrm > 0, nrm, 1)[np.repeat(np.arange(N), np.diff(crow)), 0]
        C = C / np.linalg.norm(C, axis=1, keepdims=True)
    Xg = torch.from_numpy(X).cuda()
    Cg = torch.from_numpy(C).cuda()
    ref = torch.empty((N, k), dtype=torch.float64, device="cuda")
    absdot = Xg.abs() @ Cg.abs().T                                  # sum_j |x_j c_j|
    for s in range(0, N, 64):
        xc = Xg[s:s + 64]
        if dist == "COSINE":
            ref[s:s + 64] = 1.0 - (xc[:, None, :] * Cg[None]).sum(2)
        else:
            ref[s:s + 64] = ((xc[:, None, :] - Cg[None]) ** 2).sum(2)
    m = torch.from_numpy(np.diff(crow) + 2.0).cuda()
    terms = absdot + (Xg * Xg).sum(1, keepdim=True) + (Cg * Cg).sum(1)[None, :]
    bound = 4.0 * 2.0 * m[:, None] * EPS * terms                    # [N, k]: per (row, centroid)
    # the data is away from ties beyond the bound; the two deliberate exceptions are the duplicated centroid and,
    # under COSINE, the empty rows (every centroid at distance 1: the lowest index takes them)
    distinct = ref[:, :k - 1] if k >= 3 else ref
    if distinct.shape[1] > 1:
        two = distinct.topk(2, dim=1, largest=False).values
        sure = m > 2 if dist == "COSINE" else torch.ones_like(m, dtype=torch.bool)
        assert bool(((two[:, 1] - two[:, 0]) > 2.0 * bound.max(1).values)[sure].all())
    return crow, col, val, C, ref, bound


@pytest.mark.parametrize("col_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
@pytest.mark.parametrize("k", KS)
def test_nearest(k, dist, col_dtype):
    from alink_amd.ops import kmeans_sparse as ksp
    crow, col, val, C, ref, bound = _case(k, dist)
    fm = _fm(crow, col, val, D, "cuda", col_dtype)
    assert ksp.sparse_supported(fm)
    Cg = torch.from_numpy(C).cuda()
    calls = ksp.SPARSE_CALLS
    idx, best = ksp.nearest(fm, Cg, dist)
    assert ksp.SPARSE_CALLS == calls + 1
    assert idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < k
    rmin, rarg = ref.min(1)
    chosen = ref.gather(1, idx[:, None])[:, 0]
    b_chosen = bound.gather(1, idx[:, None])[:, 0]
    b_min = bound.gather(1, rarg[:, None])[:, 0]
    print("nearest", k, dist, "max excess over the row minimum", float((chosen - rmin).max()),
          "max distance error", float((best - rmin).abs().max()), "min bound", float(b_min.min()))
    assert bool((chosen - rmin <= b_chosen).all())
    assert bool(((best - rmin).abs() <= b_min).all())
    if dist == "COSINE":
        empty = torch.from_numpy(np.diff(crow) == 0).cuda()
        assert bool((idx[empty] == 0).all()) and bool((best[empty] == 1.0).all())
    if k >= 3:
        assert not bool((idx == k - 1).any())           # the duplicate of centroid 0 never wins
        assert bool((idx == 0).any())
    counts = ksp.nearest_counts(fm, Cg, dist)
    assert counts.dtype == torch.int64
    assert torch.equal(counts, torch.bincount(idx, minlength=k))


def _accum_rows(integer):
    from alink_amd.ops import kmeans_sparse as ksp
    n, d = 2 * ksp.ACCUM_CHUNK + 17, 300
    rng = np.random.default_rng(5 + int(integer))
    cols, cnt = [], []
    for r in range(n):
        c = np.concatenate([[0], 1 + np.sort(rng.choice(d - 1, size=int(rng.integers(0, 9)), replace=False))])
        cols.append(c.astype(np.int64))
        cnt.append(c.size)
    crow = np.zeros(n + 1, np.int64)
    crow[1:] = np.cumsum(cnt)
    col = np.concatenate(cols)
    val = rng.integers(-3, 4, size=col.size).astype(np.float64) if integer else rng.normal(size=col.size)
    dense = np.zeros((n, d))
    dense[np.repeat(np.arange(n), cnt), col] = val
    return n, d, crow, col, val, dense


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("k", [3, 100, 300])
def test_accumulate(k, integer):
    from alink_amd.ops import kmeans_sparse as ksp
    n, d, crow, col, val, dense = _accum_rows(integer)
    fm = _fm(crow, col, val, d, "cuda")
    csc = ksp.prepare(fm)
    assert csc.nmulti >= 1 and int(csc.mcount.max()) == 3           # column 0 spans three chunks
    assert ksp.prepare(fm) is csc                                    # built once
    C = torch.from_numpy(np.random.default_rng(k).normal(size=(k, d))).cuda()
    idx, _, counts = ksp.nearest_hip(fm, C, "EUCLIDEAN", True, False, True)
    buf = ksp.accumulate_hip(fm, idx, k, d, counts)
    idx_h = idx.cpu().to(torch.int64)
    Xd = torch.from_numpy(dense)
    ref = torch.zeros((k, d), dtype=torch.float64).index_add_(0, idx_h, Xd)
    got = buf[:, :d].cpu()
    if integer:
        assert torch.equal(got, ref)
    else:
        m = torch.from_numpy(np.bincount(col, minlength=d).astype(np.float64))
        bound = 4.0 * 2.0 * m[None, :] * EPS * torch.zeros((k, d), dtype=torch.float64).index_add_(0, idx_h, Xd.abs())
        print("accumulate", k, "max error", float((got - ref).abs().max()), "max bound", float(bound.max()))
        assert bool(((got - ref).abs() <= bound).all())
    assert torch.equal(buf[:, d].cpu(), torch.bincount(idx_h, minlength=k).to(torch.float64))
    assert torch.equal(ksp.accumulate_hip(fm, idx, k, d, counts), buf)          # launch to launch
    for grid in (1, 7):                                                          # and for every grid
        assert torch.equal(ksp.accumulate_hip(fm, idx, k, d, counts, grid=grid), buf)
    assert torch.equal(ksp.assign_accumulate(fm, C, "EUCLIDEAN"), buf)


def test_empty_inputs():
    from alink_amd.ops import kmeans_sparse as ksp
    d, k = 40, 5
    C = torch.from_numpy(np.random.default_rng(2).normal(size=(k, d))).cuda()
    z = np.zeros(0)
    fm0 = _fm(np.zeros(1, np.int64), z.astype(np.int64), z, d, "cuda")
    calls = ksp.SPARSE_CALLS
    idx, dist = ksp.nearest(fm0, C, "EUCLIDEAN")
    assert idx.shape == (0,) and dist.shape == (0,)
    assert torch.equal(ksp.nearest_counts(fm0, C, "EUCLIDEAN"), torch.zeros(k, dtype=torch.int64, device="cuda"))
    assert torch.equal(ksp.assign_accumulate(fm0, C, "COSINE"), torch.zeros((k, d + 1), dtype=torch.float64,
                                                                            device="cuda"))
    assert ksp.SPARSE_CALLS == calls                       # n = 0: nothing is launched
    n = 130
    fme = _fm(np.zeros(n + 1, np.int64), z.astype(np.int64), z, d, "cuda")
    want = int((C * C).sum(1).argmin())
    idx, dist = ksp.nearest(fme, C, "EUCLIDEAN")
    assert bool((idx == want).all())
    assert torch.equal(dist, (C * C).sum(1)[want].expand(n))
    buf = ksp.assign_accumulate(fme, C, "EUCLIDEAN")
    assert float(buf[:, :d].abs().sum()) == 0.0 and float(buf[want, d]) == n and float(buf[:, d].sum()) == n


def _blobs(n=600, d=5000, k=4):
    """Well-separated sparse blobs over disjoint column ranges, and initial centroids (one per blob)."""
    from kmeans_sparse_dist import blob_init, sparse_blobs
    crow, col, val = sparse_blobs(n, d, k, nnz=12, seed=3)
    return crow, col, val, blob_init(col, d, k, nnz=12)


@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
def test_train_takes_sparse_path_and_matches_cpu(dist):
    from alink_amd import useLocalEnv
    from alink_amd.models.clustering.kmeans import KMeansModelDataConverter, train_kmeans
    from alink_amd.ops import kmeans_sparse as ksp
    n, d, k = 600, 5000, 4
    crow, col, val, init = _blobs(n, d, k)
    init_t = torch.from_numpy(init)
    if dist == "COSINE":
        init_t = init_t / init_t.norm(dim=1, keepdim=True)
    models = {}
    for dev in ("cpu", "cuda:0"):
        env = useLocalEnv(1, device=dev)
        calls = ksp.SPARSE_CALLS
        rows, q = train_kmeans(_fm(crow, col, val, d, dev), k, 10, 1e-6, dist, "RANDOM", 2, "v", env,
                               init_centroids=init_t.clone())
        if dev != "cpu":
            assert ksp.SPARSE_CALLS >= calls + 2 * q.step_no        # nearest + accumulate per superstep
        else:
            assert ksp.SPARSE_CALLS == calls
        models[dev] = (KMeansModelDataConverter().load(rows), q.step_no)
    (a, sa), (b, sb) = models["cpu"], models["cuda:0"]
    assert sa == sb and a.centroids.shape == (k, d)
    assert np.array_equal(a.weights, b.weights)
    # a centroid coordinate is a mean of at most n terms of size <= max|x| (or that mean normalised): two fp64
    # evaluations differ by at most 2 n 2^-53 max|x|; 4x that, as everywhere in this file
    atol = 4.0 * 2.0 * n * EPS * max(1.0, float(np.abs(val).max()))
    print("train", dist, "max centroid difference", float(np.abs(a.centroids - b.centroids).max()), "atol", atol)
    assert np.abs(a.centroids - b.centroids).max() <= atol


def test_predict_on_device_block_matches_cpu():
    from alink_amd import useLocalEnv, KMeansPredictBatchOp, KMeansTrainBatchOp
    from alink_amd.common.linalg.block import SparseBlock
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    from alink_amd.operator.batch.source import TableSourceBatchOp
    from alink_amd.ops import kmeans_sparse as ksp
    n, d, k = 600, 5000, 4
    crow, col, val, _ = _blobs(n, d, k)
    blk = SparseBlock(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), d)
    schema = TableSchema(["v"], [Types.SPARSE_VECTOR])
    useLocalEnv(1, device="cpu")
    src = TableSourceBatchOp(MTable(schema, [Column(blk)]))
    model = KMeansTrainBatchOp().setVectorCol("v").setK(k).setMaxIter(10).linkFrom(src)
    pred = KMeansPredictBatchOp().setPredictionCol("p").setPredictionDistanceCol("dist").linkFrom(model, src)
    cpu_ids = pred.getOutputTable().col("p").to_list()
    cpu_d2 = np.asarray(pred.getOutputTable().col("dist").to_list()) ** 2
    useLocalEnv(1, device="cuda:0")
    calls = ksp.SPARSE_CALLS
    gsrc = TableSourceBatchOp(MTable(schema, [Column(blk.to("cuda:0"))]))
    gmodel = TableSourceBatchOp(model.getOutputTable())
    gpred = KMeansPredictBatchOp().setPredictionCol("p").setPredictionDistanceCol("dist").linkFrom(gmodel, gsrc)
    assert gpred.getOutputTable().col("p").to_list() == cpu_ids
    assert ksp.SPARSE_CALLS > calls
    # squared distances are sums of m = 12 + 2 terms x_j c_j, |x|^2, |c|^2 with 12 entries in [1, 2) per row and
    # centroids that are means of such rows: sum|terms| <= 3 * 12 * 4
    gpu_d2 = np.asarray(gpred.getOutputTable().col("dist").to_list()) ** 2
    assert np.abs(gpu_d2 - cpu_d2).max() <= 4.0 * 2.0 * 14 * EPS * 3 * 12 * 4
