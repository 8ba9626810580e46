"""Dense fp64 KMeans on the GPU (``ops/csrc/kmeans_dense64.hip`` through ``ops/kmeans_dense64.py``).

Tolerance (derived, not tuned; the rule of ``test_kmeans_sparse_gpu.py``): two fp64 evaluations of a sum over ``m``
terms differ by at most ``2 m 2^-53 sum|terms|``; the tests allow 4x that, computed from the data.  For a distance
``m = d + 2`` with the terms ``x_j c_j``, ``|x|^2`` and ``|c|^2``; for a cluster sum ``m`` is the cluster's row count
with the terms ``x_rj``.  The data is away from ties beyond that bound (asserted on the reference alone), the
duplicated centroid being the deliberate exception.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
N = 1003                        # not a multiple of 16 or of a workgroup's 64 rows
DS = (1, 3, 4, 5, 63, 64, 65, 128, 131, 300, 1024)
KS = (1, 3, 15, 16, 17, 100, 257, 300)


def _data(d, k, dist):
    """X [N, d], C [k, d] as numpy: every 17th row (r % 17 == 5) is far out (x -2^12), centroid 0 is shrunk and
    centroid k - 1 duplicates it."""
    X = np.random.default_rng(11 + d).normal(size=(N, d))
    X[np.arange(N) % 17 == 5] *= -(2.0 ** 12)
    C = np.random.default_rng(100 + k + 1000 * d).normal(size=(k, d)) * 0.5
    if k >= 3:
        C[0] *= 0.8
        C[k - 1] = C[0]
    if dist == "COSINE":
        X = X / np.linalg.norm(X, axis=1, keepdims=True)
        C = C / np.linalg.norm(C, axis=1, keepdims=True)
    return X, C


def _reference(Xg, Cg, dist):
    """(reference distances [n, k] by the direct formula in 64-row blocks, bounds [n, k])."""
    n, d = Xg.shape
    k = Cg.shape[0]
    ref = torch.empty((n, k), dtype=torch.float64, device=Xg.device)
    for s in range(0, n, 64):
        xc = Xg[s:s + 64]
        if dist == "COSINE":
            ref[s:s + 64] = 1.0 - (xc[:, None, :] * Cg[None]).sum(2)
        else:
            ref[s:s + 64] = ((xc[:, None, :] - Cg[None]) ** 2).sum(2)
    terms = Xg.abs() @ Cg.abs().T + (Xg * Xg).sum(1, keepdim=True) + (Cg * Cg).sum(1)[None, :]
    return ref, 4.0 * 2.0 * (d + 2) * EPS * terms


@functools.lru_cache(maxsize=None)
def _case(d, k, dist):
    """(X, C, reference distances, bounds) on the GPU; computed once per case and left unchanged."""
    X, C = _data(d, k, dist)
    Xg, Cg = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    ref, bound = _reference(Xg, Cg, dist)
    distinct = ref[:, :k - 1] if k >= 3 else ref
    if distinct.shape[1] > 1:
        two = distinct.topk(2, dim=1, largest=False).values
        assert bool(((two[:, 1] - two[:, 0]) > 2.0 * bound.max(1).values).all())
    return Xg, Cg, ref, bound


def _check_nearest(d, k, dist):
    from alink_amd.ops import kmeans_dense64 as kd
    Xg, Cg, ref, bound = _case(d, k, dist)
    assert kd.dense64_selected(Xg, k)
    calls = kd.DENSE64_CALLS
    idx, best = kd.nearest(Xg, Cg, dist)
    assert kd.DENSE64_CALLS == calls + 1
    assert idx.dtype == torch.int64 and idx.shape == (N,) and int(idx.min()) >= 0 and int(idx.max()) < k
    assert best.dtype == torch.float64 and best.shape == (N,)
    rmin, rarg = ref.min(1)
    chosen = ref.gather(1, idx[:, None])[:, 0]
    b_chosen = bound.gather(1, idx[:, None])[:, 0]
    b_min = bound.gather(1, rarg[:, None])[:, 0]
    print("nearest", d, k, dist, "max excess over the row minimum", float((chosen - rmin).max()),
          "max distance error / bound", float(((best - rmin).abs() / b_min).max()))
    assert bool((chosen - rmin <= b_chosen).all())
    assert bool(((best - rmin).abs() <= b_min).all())
    if dist == "EUCLIDEAN":
        assert float(best.min()) >= 0.0
    if k >= 3:
        assert not bool((idx == k - 1).any())           # the duplicate of centroid 0 never wins
        # ... and centroid 0 takes every row that the reference gives to it or to its duplicate.  In a few
        # low-dimensional cases with many centroids (d = 1, 4, 5 at k = 257, d = 3, 5 at k = 300, d = 5 at k = 1025)
        # the reference itself has no such row, so "index 0 wins" is asserted wherever the reference has one
        mine = (rarg == 0) | (rarg == k - 1)
        assert bool((idx[mine] == 0).all()) and bool((idx == 0).any()) == bool(mine.any())
        if d > 5 or k <= 100:
            assert bool((idx == 0).any())
    counts = kd.nearest_counts(Xg, Cg, dist)
    assert counts.dtype == torch.int64 and counts.shape == (k,)
    assert torch.equal(counts, torch.bincount(idx, minlength=k))


# COSINE at d = 1 is left out: every normalised 1-d row ties
@pytest.mark.parametrize("d,k,dist", [(d, k, dist) for dist in ("EUCLIDEAN", "COSINE") for d in DS for k in KS
                                      if not (dist == "COSINE" and d == 1)])
def test_nearest(d, k, dist):
    _check_nearest(d, k, dist)


def test_nearest_many_centroid_blocks():
    _check_nearest(5, 1025, "EUCLIDEAN")


def test_unaligned_rows():
    """A view that starts 8 bytes into an allocation (even d): the 16-byte loads must not be taken."""
    from alink_amd.ops import kmeans_dense64 as kd
    Xg, Cg, ref, bound = _case(64, 17, "EUCLIDEAN")
    flat = torch.empty(N * 64 + 1, dtype=torch.float64, device="cuda")
    Xo = flat[1:].view(N, 64)
    Xo.copy_(Xg)
    assert Xo.data_ptr() % 16 == 8 and kd.dense64_supported(Xo, 17)
    idx, best = kd.nearest(Xo, Cg, "EUCLIDEAN")
    idx0, best0 = kd.nearest(Xg, Cg, "EUCLIDEAN")
    assert torch.equal(idx, idx0) and torch.equal(best, best0)


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("k", [3, 100, 300])
def test_accumulate(k, integer, monkeypatch):
    from alink_amd.ops import kmeans as kops, kmeans_dense64 as kd
    monkeypatch.delenv("ALINK_KMEANS_DENSE64", raising=False)
    d, n = 131, 2 * kd.ACCUM_ROWS + 17
    rng = np.random.default_rng(5 + int(integer) + 10 * k)
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float64) if integer else rng.normal(size=(n, d))
    C = rng.integers(-3, 4, size=(k, d)).astype(np.float64) if integer else rng.normal(size=(k, d))
    planted = np.arange(n) % 40 != 0            # all but 14 rows sit on centroid 1: its cluster spans three chunks
    X[planted] = C[1]
    Xg, Cg = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    idx, _ = kd.nearest(Xg, Cg, "EUCLIDEAN")
    cnt = torch.bincount(idx, minlength=k)
    big = int(cnt.max())
    assert 2 * kd.ACCUM_ROWS < big <= 3 * kd.ACCUM_ROWS
    buf = kd.accumulate(Xg, idx, k)
    assert buf.shape == (k, d + 1) and buf.dtype == torch.float64
    ref = torch.zeros((k, d), dtype=torch.float64).index_add_(0, idx.cpu(), torch.from_numpy(X))
    got = buf[:, :d].cpu()
    if integer:
        assert torch.equal(got, ref)
    else:
        sabs = torch.zeros((k, d), dtype=torch.float64).index_add_(0, idx.cpu(), torch.from_numpy(np.abs(X)))
        bound = 4.0 * 2.0 * cnt.cpu().to(torch.float64)[:, None] * EPS * sabs
        print("accumulate", k, "max error", float((got - ref).abs().max()), "max bound", float(bound.max()))
        assert bool(((got - ref).abs() <= bound).all())
    assert torch.equal(buf[:, d], cnt.to(torch.float64))
    assert torch.equal(kd.accumulate(Xg, idx, k), buf)                      # launch to launch
    for grid in (1, 7):                                                     # and for every grid
        assert torch.equal(kd.accumulate(Xg, idx, k, grid=grid), buf)
    assert torch.equal(kd.accumulate(Xg, idx.to(torch.int32), k), buf)
    assert torch.equal(kd.assign_accumulate(Xg, Cg), buf)
    for grid in (1, 7):
        assert torch.equal(kd.assign_accumulate(Xg, Cg, grid=grid), buf)
    calls = kd.DENSE64_CALLS
    assert torch.equal(kops.assign_accumulate(Xg, Cg), buf)
    assert kd.DENSE64_CALLS > calls
    monkeypatch.setenv("ALINK_KMEANS_DENSE64", "0")
    calls = kd.DENSE64_CALLS
    off = kops.assign_accumulate(Xg, Cg)
    assert kd.DENSE64_CALLS == calls
    assert torch.equal(off[:, d], buf[:, d])


def test_nan_and_inf_rows():
    from alink_amd.ops import kmeans_dense64 as kd
    d, k, n = 5, 17, 200
    rng = np.random.default_rng(3)
    X = rng.normal(size=(n, d))
    C = rng.normal(size=(k, d))
    X[37, 2] = np.nan
    X[150, 4] = np.inf
    keep = np.ones(n, bool)
    keep[[37, 150]] = False
    Xg, Cg = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    clean = torch.from_numpy(X[keep]).cuda()
    for dist in ("EUCLIDEAN", "COSINE"):
        idx, best = kd.nearest(Xg, Cg, dist)
        assert int(idx.min()) >= 0 and int(idx.max()) < k
        assert int(idx[37]) == 0
        idx_c, best_c = kd.nearest(clean, Cg, dist)
        km = torch.from_numpy(keep).cuda()
        assert torch.equal(idx[km], idx_c) and torch.equal(best[km], best_c)
        counts = kd.nearest_counts(Xg, Cg, dist)
        assert int(counts.sum()) == n and torch.equal(counts, torch.bincount(idx, minlength=k))
    buf = kd.assign_accumulate(Xg, Cg)
    assert float(buf[:, d].sum()) == n


def test_no_n_by_k_buffer():
    from alink_amd.ops import kmeans_dense64 as kd
    n, d, k = 2 ** 18, 8, 512
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((n, d), dtype=torch.float64, device="cuda", generator=g)
    C = torch.randn((k, d), dtype=torch.float64, device="cuda", generator=g)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    idx, best = kd.nearest(X, C, "EUCLIDEAN")
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("nearest peak rise", rise / 2 ** 20, "MiB")
    assert rise < 64 * 2 ** 20            # the outputs are 4 MiB; an [n, k] fp64 matrix would be 1 GiB
    assert idx.shape == (n,) and best.shape == (n,)


def test_empty_inputs():
    from alink_amd.ops import kmeans_dense64 as kd
    d, k = 40, 5
    C = torch.from_numpy(np.random.default_rng(2).normal(size=(k, d))).cuda()
    X0 = torch.zeros((0, d), dtype=torch.float64, device="cuda")
    calls = kd.DENSE64_CALLS
    idx, dist = kd.nearest(X0, C, "EUCLIDEAN")
    assert idx.shape == (0,) and idx.dtype == torch.int64 and dist.shape == (0,)
    assert torch.equal(kd.nearest_counts(X0, C, "EUCLIDEAN"), torch.zeros(k, dtype=torch.int64, device="cuda"))
    zero = torch.zeros((k, d + 1), dtype=torch.float64, device="cuda")
    assert torch.equal(kd.assign_accumulate(X0, C), zero)
    assert torch.equal(kd.accumulate(X0, torch.zeros(0, dtype=torch.int64, device="cuda"), k), zero)
    assert kd.DENSE64_CALLS == calls                       # n = 0: nothing is launched
    n = 130
    Xz = torch.zeros((n, d), dtype=torch.float64, device="cuda")
    cn = (C * C).sum(1)
    want = int(cn.argmin())
    idx, dist = kd.nearest(Xz, C, "EUCLIDEAN")
    assert bool((idx == want).all())
    assert torch.equal(dist, cn[want].expand(n))
    buf = kd.assign_accumulate(Xz, C)
    assert float(buf[:, :d].abs().sum()) == 0.0 and float(buf[want, d]) == n and float(buf[:, d].sum()) == n


def _blobs(n=600, d=37, k=4):
    rng = np.random.default_rng(3)
    centers = rng.normal(size=(k, d)) * 10.0 + 3.0        # well separated, away from the origin (COSINE too)
    lab = np.arange(n) % k
    X = centers[lab] + rng.normal(size=(n, d)) * 0.3
    init = centers + rng.normal(size=(k, d)) * 0.5
    return X, init


@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
def test_train_matches_cpu(dist):
    from alink_amd import useLocalEnv
    from alink_amd.models.clustering.kmeans import KMeansModelDataConverter, train_kmeans
    from alink_amd.ops import kmeans_dense64 as kd
    n, d, k = 600, 37, 4
    X, init = _blobs(n, d, k)
    init_t = torch.from_numpy(init)
    if dist == "COSINE":
        init_t = init_t / init_t.norm(dim=1, keepdim=True)
    models = {}
    for dev in ("cpu", "cuda:0"):
        env = useLocalEnv(1, device=dev)
        calls = kd.DENSE64_CALLS
        rows, q = train_kmeans(torch.from_numpy(X).to(dev), k, 10, 1e-6, dist, "RANDOM", 2, "v", env,
                               init_centroids=init_t.clone())
        if dev != "cpu":
            assert kd.DENSE64_CALLS >= calls + q.step_no
        else:
            assert kd.DENSE64_CALLS == calls
        models[dev] = (KMeansModelDataConverter().load(rows), q.step_no)
    (a, sa), (b, sb) = models["cpu"], models["cuda:0"]
    assert sa == sb and a.centroids.shape == (k, d)
    assert np.array_equal(a.weights, b.weights)
    # a centroid coordinate is a mean of at most n terms of size <= max|x| (or that mean normalised): two fp64
    # evaluations differ by at most 2 n 2^-53 max|x|; 4x that
    atol = 4.0 * 2.0 * n * EPS * max(1.0, float(np.abs(X).max()))
    print("train", dist, "max centroid difference", float(np.abs(a.centroids - b.centroids).max()), "atol", atol)
    assert np.abs(a.centroids - b.centroids).max() <= atol


def test_init_passes_take_kernel():
    from alink_amd import useLocalEnv
    from alink_amd.models.clustering.kmeans import kmeans_init
    from alink_amd.ops import kmeans_dense64 as kd
    from alink_amd.ops.kmeans_rows import rows
    n, d, k = 600, 37, 4
    X, init = _blobs(n, d, k)
    Xc, Cc = torch.from_numpy(X), torch.from_numpy(init)
    Xg, Cg = Xc.cuda(), Cc.cuda()
    calls = kd.DENSE64_CALLS
    cpu = rows(Xc, "EUCLIDEAN").nearest(Cc)[1]
    assert kd.DENSE64_CALLS == calls
    gpu = rows(Xg, "EUCLIDEAN").nearest(Cg)[1]
    assert kd.DENSE64_CALLS == calls + 1
    # |sqrt(a) - sqrt(b)| <= sqrt|a - b| for two evaluations a, b of the squared distance to the nearest centroid
    ref, bound = _reference(Xg, Cg, "EUCLIDEAN")
    tol = torch.sqrt(bound.gather(1, ref.argmin(1)[:, None])[:, 0])
    print("min_dist max difference", float((gpu.cpu() - cpu).abs().max()), "min tol", float(tol.min()))
    assert bool(((gpu - cpu.cuda()).abs() <= tol).all())
    useLocalEnv(1, device="cuda:0")
    calls = kd.DENSE64_CALLS
    init_c = kmeans_init(Xg, k, "K_MEANS_PARALLEL", 2, "EUCLIDEAN", seed=1)
    assert kd.DENSE64_CALLS > calls
    assert init_c.shape == (k, d) and bool(torch.isfinite(init_c).all())


def test_predict_device_block():
    from alink_amd import useLocalEnv, KMeansPredictBatchOp, KMeansTrainBatchOp
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    from alink_amd.operator.batch.source import TableSourceBatchOp
    from alink_amd.ops import kmeans_dense64 as kd
    n, d, k = 600, 37, 4
    X, _ = _blobs(n, d, k)
    Xt = torch.from_numpy(X)
    schema = TableSchema(["v"], [Types.DENSE_VECTOR])
    useLocalEnv(1, device="cpu")
    src = TableSourceBatchOp(MTable(schema, [Column(Xt)]))
    model = KMeansTrainBatchOp().setVectorCol("v").setK(k).setMaxIter(10).linkFrom(src)

    def predict(source, model_op, detail):
        op = KMeansPredictBatchOp().setPredictionCol("p").setPredictionDistanceCol("dist")
        if detail:
            op = op.setPredictionDetailCol("det")
        return op.linkFrom(model_op, source).getOutputTable()

    cpu = predict(src, model, False)
    cpu_det = predict(src, model, True)
    useLocalEnv(1, device="cuda:0")
    gsrc = TableSourceBatchOp(MTable(schema, [Column(Xt.cuda())]))
    gmodel = TableSourceBatchOp(model.getOutputTable())
    calls = kd.DENSE64_CALLS
    gpu = predict(gsrc, gmodel, False)
    assert gpu.col("p").to_list() == cpu.col("p").to_list()
    assert kd.DENSE64_CALLS > calls
    # squared distances: m = d + 2 terms; sum|terms| <= |x|^2 + |c|^2 + |x||c| <= 3 max|x|^2 d (the centroids are
    # means of rows)
    cpu_d2 = np.asarray(cpu.col("dist").to_list()) ** 2
    gpu_d2 = np.asarray(gpu.col("dist").to_list()) ** 2
    bound = 4.0 * 2.0 * (d + 2) * EPS * 3.0 * float(np.abs(X).max()) ** 2 * d
    print("predict max dist^2 difference", float(np.abs(gpu_d2 - cpu_d2).max()), "bound", bound)
    assert np.abs(gpu_d2 - cpu_d2).max() <= bound
    calls = kd.DENSE64_CALLS
    gpu_det = predict(gsrc, gmodel, True)
    assert kd.DENSE64_CALLS == calls                      # the detail column needs every distance: left as it was
    assert gpu_det.col("p").to_list() == cpu_det.col("p").to_list()
    # The detail strings print every probability 1/(k-1) - d/s/(k-1) to the last digit, and nothing in that chain is
    # the same on both devices for general data: the [n, k] distances come from torch's GEMM (on the blobs above one
    # string in 600 differs in its last digit, 0.2062833060352597 against ...25968, with or without this path), the
    # sum s of a row's distances rounds by its order, and a division by the scalar k - 1 is a multiplication by
    # its reciprocal on the GPU.  String equality is therefore asserted where every step is exact or correctly
    # rounded on any device: integer points on one line (x = offset + t e_0) with 128 rows per cluster, so every
    # centroid coordinate is an integer over 2^7 and every distance |t - mean| and every sum of distances a small
    # dyadic number; and ki = 5 clusters, so k - 1 is a power of two.  What is left is one IEEE division d/s
    ki = 5
    rng = np.random.default_rng(9)
    lab = np.arange(128 * ki) % ki
    Xi = np.tile(rng.integers(-30, 31, size=(1, d)), (128 * ki, 1)).astype(np.float64)
    Xi[:, 0] = np.array([0, 40, 100, 170, 250])[lab] + np.concatenate([np.zeros(ki),
                                                                       rng.integers(-2, 3, size=128 * ki - ki)])
    Xit = torch.from_numpy(Xi)
    from alink_amd.models.clustering.kmeans import KMeansModelDataConverter, train_kmeans
    env = useLocalEnv(1, device="cpu")
    isrc = TableSourceBatchOp(MTable(schema, [Column(Xit)]))
    rows, _ = train_kmeans(Xit, ki, 10, 1e-6, "EUCLIDEAN", "RANDOM", 2, "v", env, init_centroids=Xit[:ki].clone())
    imodel = MTable.from_rows(rows, KMeansModelDataConverter().getModelSchema(), replicated=True)
    icpu = predict(isrc, TableSourceBatchOp(imodel), True)
    assert np.bincount(icpu.col("p").to_list(), minlength=ki).tolist() == [128] * ki
    useLocalEnv(1, device="cuda:0")
    calls = kd.DENSE64_CALLS
    igpu = predict(TableSourceBatchOp(MTable(schema, [Column(Xit.cuda())])), TableSourceBatchOp(imodel), True)
    assert kd.DENSE64_CALLS == calls
    assert igpu.col("p").to_list() == icpu.col("p").to_list()
    assert igpu.col("det").to_list() == icpu.col("det").to_list()
