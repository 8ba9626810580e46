"""KMeans end to end (reference T/pipeline/clustering/KMeansTest.java, KMeansModelMapperTest.java)."""
import numpy as np
import pytest

from alink_amd import *
from alink_amd.common.types import TableSchema, Types
from tests.test_core_formats import KMEANS_ROWS

ROWS = [["0 0 0"], ["0.1 0.1 0.1"], ["0.2 0.2 0.2"], ["9 9 9"], ["9.1 9.1 9.1"], ["9.2 9.2 9.2"]]


def test_kmeans_pipeline_distances():
    data = MemSourceBatchOp(ROWS, ["vector"])
    km = KMeans().setVectorCol("vector").setPredictionCol("pred").setPredictionDistanceCol("distance").setK(2)
    model = Pipeline().add(km).fit(data)
    res = model.transform(data).select("distance").collect()
    expect = [0.173, 0, 0.173, 0.173, 0, 0.173]
    for r, e in zip(res, expect):
        assert abs(r[0] - e) < 0.01


def test_kmeans_model_mapper_detail():
    from alink_amd.models.clustering.kmeans import KMeansModelMapper, KMeansModelDataConverter
    from alink_amd.common.params import Params
    ds = TableSchema(["Y"], [Types.STRING])
    p = Params().set("predictionCol", "pred").set("predictionDetailCol", "detail").set("predictionDistanceCol",
                                                                                         "distance")
    m = KMeansModelMapper(KMeansModelDataConverter().getModelSchema(), ds, p)
    m.loadModel(KMEANS_ROWS)
    r = m.map(("0 0 0",))
    assert r[1] == 1
    assert r[2] == "0.010869565217391353 0.9891304347826086"
    assert abs(r[3] - 0.173) < 0.001
    assert m.getOutputSchema() == TableSchema(["Y", "pred", "detail", "distance"],
                                              [Types.STRING, Types.LONG, Types.STRING, Types.DOUBLE])


def test_kmeans_train_op_model_rows_format():
    data = MemSourceBatchOp(ROWS, ["vector"])
    model = KMeansTrainBatchOp().setVectorCol("vector").setK(2).linkFrom(data)
    rows = model.collect()
    assert rows[0][0] == 0 and rows[1][0] == 1048576
    meta = rows[0][1]
    assert meta.startswith('{"vectorCol":"\\"vector\\"","latitudeCol":null')
    pred = KMeansPredictBatchOp().setPredictionCol("p").linkFrom(model, data).collect()
    assert len({r[1] for r in pred[:3]}) == 1 and pred[0][1] != pred[5][1]


def test_kmeans_blobs_converges_and_recovers_centers():
    rng = np.random.default_rng(0)
    centers = rng.normal(size=(5, 4)) * 10
    lab = rng.integers(0, 5, 2000)
    X = centers[lab] + rng.normal(size=(2000, 4)) * 0.3
    rows = [[" ".join(map(str, x))] for x in X]
    op = KMeansTrainBatchOp().setVectorCol("v").setK(5).setMaxIter(50).setInitSteps(5).linkFrom(MemSourceBatchOp(rows, ["v"]))
    from alink_amd.models.clustering.kmeans import KMeansModelDataConverter
    m = KMeansModelDataConverter().load(op.collect())
    got = m.centroids
    d = np.linalg.norm(got[:, None, :] - centers[None, :, :], axis=2).min(0)
    assert d.max() < 0.2
    assert op.getTrainInfo()["iterations"] < 50


@pytest.mark.parametrize("init", ["RANDOM", "K_MEANS_PARALLEL"])
def test_kmeans_init_modes_and_cosine(init):
    rng = np.random.default_rng(1)
    X = np.abs(rng.normal(size=(300, 3)))
    rows = [[" ".join(map(str, x))] for x in X]
    data = MemSourceBatchOp(rows, ["v"])
    for dt in ["EUCLIDEAN", "COSINE"]:
        op = KMeansTrainBatchOp().setVectorCol("v").setK(3).setInitMode(init).setDistanceType(dt).linkFrom(data)
        out = KMeansPredictBatchOp().setPredictionCol("p").setPredictionDetailCol("d").linkFrom(op, data).collect()
        assert len(out) == 300 and all(0 <= r[1] < 3 for r in out)


def test_reference_seeding_rule_flag(monkeypatch):
    """Default (reference) rule: one sampled candidate per pick (LocalKmeansFunc); greedy opt-in; both give k
    distinct centroids from the candidate set."""
    import torch
    from alink_amd.models.clustering.kmeans import _local_kmeans
    g = torch.Generator().manual_seed(0)
    pts = torch.cat([torch.randn(50, 4, generator=g, dtype=torch.float64) + 10 * i for i in range(5)])
    w = torch.ones(pts.shape[0], dtype=torch.float64)
    for rule in ("greedy", "reference"):
        monkeypatch.setenv("ALINK_KMEANS_SEEDING", rule)
        C = _local_kmeans(pts, w, 5, "EUCLIDEAN", seed=3)
        assert C.shape == (5, 4)
        assert len({tuple(torch.round(c / 10).tolist()) for c in C}) >= 4


def test_predict_columnar_inputs_and_detail_match_row_formatting():
    import json
    import pandas as pd
    import torch
    """KMeans predict on dense-vector strings (C++ parser), sparse vector strings / SparseBlock columns and the
    detail column (C++ Double.toString rows) equals the per-row formatting of the same values."""
    import numpy as np
    from alink_amd import BatchOperator, KMeansTrainBatchOp, KMeansPredictBatchOp
    from alink_amd.common.linalg import DenseVector, VectorUtil
    from alink_amd.models.clustering.kmeans import prob_from_distances
    rng = np.random.default_rng(4)
    X = np.concatenate([rng.normal(size=(40, 3)) + 5 * i for i in range(3)])
    dense = [" ".join(repr(float(v)) for v in r) for r in X]
    sparse = ["$3$" + " ".join(f"{j}:{float(v)!r}" for j, v in enumerate(r) if j != 1) for r in X]
    df = pd.DataFrame({"v": dense, "s": sparse})
    src = BatchOperator.fromDataframe(df, schemaStr="v string, s string")
    model = KMeansTrainBatchOp().setVectorCol("v").setK(3).linkFrom(src)
    out = KMeansPredictBatchOp().setPredictionCol("p").setPredictionDetailCol("d").setPredictionDistanceCol("dist") \
        .linkFrom(model, src).collect()
    C = np.array([[float(x) for x in json.loads(r[1])["vec"]["data"]] for r in model.collect() if r[0] > 0])
    D = np.sqrt(((X[:, None, :] - C[None]) ** 2).sum(-1))
    probs = prob_from_distances(torch.from_numpy(D)).numpy()
    for r, row in enumerate(out):
        assert row[2] == int(np.argmin(D[r]))
        got = np.array([float(x) for x in row[3].split(" ")])
        np.testing.assert_allclose(got, probs[r], rtol=1e-12, atol=1e-14)
        assert row[3] == VectorUtil.toString(DenseVector(got))          # Java Double.toString layout
        assert abs(row[4] - D[r].min()) < 1e-9
    # sparse strings (index 1 missing) through the row path
    ms = KMeansTrainBatchOp().setVectorCol("s").setK(3).linkFrom(src)
    outs = KMeansPredictBatchOp().setPredictionCol("p").linkFrom(ms, src).collect()
    Cs = np.array([[float(x) for x in json.loads(r[1])["vec"]["data"]] for r in ms.collect() if r[0] > 0])
    Xs = X.copy()
    Xs[:, 1] = 0.0
    Ds = ((Xs[:, None, :] - Cs[None]) ** 2).sum(-1)
    assert [row[2] for row in outs] == [int(i) for i in Ds.argmin(1)]


def test_native_java_double_rows_equals_vector_tostring():
    import numpy as np
    from alink_amd import _native
    from alink_amd.common.linalg import DenseVector, VectorUtil
    rng = np.random.default_rng(9)
    a = rng.normal(size=(50, 7)) * 10.0 ** rng.integers(-8, 9, size=(50, 7))
    a[0, :] = [0.0, -0.0, 1e-3, 9.999999e6, 1e7, -1e-4, 123456789.0]
    rows = _native.java_double_rows(a, " ")
    assert rows == [VectorUtil.toString(DenseVector(r)) for r in a]


OLD_META = ('{"vectorCol":"\\"Y\\"","latitudeCol":null,"longitudeCol":null,"distanceType":"\\"EUCLIDEAN\\"",'
            '"k":"2","modelSchema":"\\"model_id bigint,model_info string\\"","isNewFormat":"true",'
            '"vectorSize":"3"}')
HAV_META = ('{"vectorCol":null,"latitudeCol":"\\"f1\\"","longitudeCol":"\\"f0\\"","distanceType":"\\"HAVERSINE\\"",'
            '"k":"2","modelSchema":"\\"model_id bigint,model_info string\\"","isNewFormat":"true",'
            '"vectorSize":"2"}')


@pytest.mark.parametrize("rows", [
    # KMeansOldModelMapper1Test: OldClusterSummary with the center as a DenseVector JSON string
    [(0, OLD_META), (1048576, '{"center":"{\\"data\\":[9.1,9.1,9.1]}","clusterId":0,"weight":3.0}'),
     (2097152, '{"center":"{\\"data\\":[0.1,0.1,0.1]}","clusterId":1,"weight":3.0}')],
    # KMeansOldModelMapper2Test: no modelSchema / isNewFormat in the meta, center as "[x, y, z]", vec null
    [(0, '{"vectorCol":"\\"Y\\"","latitudeCol":null,"longitudeCol":null,"distanceType":"\\"EUCLIDEAN\\"",'
         '"k":"2","vectorSize":"3"}'),
     (1048576, '{"clusterId":0,"weight":3.0,"center":"[9.1, 9.1, 9.1]","vec":null}'),
     (2097152, '{"clusterId":1,"weight":3.0,"center":"[0.1, 0.1, 0.1]","vec":null}')]])
def test_kmeans_old_model_formats(rows):
    from alink_amd.models.clustering.kmeans import KMeansModelMapper, KMeansModelDataConverter
    from alink_amd.common.params import Params
    m = KMeansModelMapper(KMeansModelDataConverter().getModelSchema(), TableSchema(["Y"], [Types.STRING]),
                          Params().set("predictionCol", "pred"))
    m.loadModel(rows)
    assert m.map(("0 0 0",))[1] == 1
    assert m.getOutputSchema() == TableSchema(["Y", "pred"], [Types.STRING, Types.LONG])


def test_kmeans_old_model_haversine():
    from alink_amd.models.clustering.kmeans import KMeansModelMapper, KMeansModelDataConverter
    from alink_amd.common.params import Params
    rows = [(0, HAV_META), (1048576, '{"center":"{\\"data\\":[8.33,9.0]}","clusterId":0,"weight":3.0}'),
            (2097152, '{"center":"{\\"data\\":[1.0,1.33]}","clusterId":1,"weight":3.0}')]
    m = KMeansModelMapper(KMeansModelDataConverter().getModelSchema(),
                          TableSchema(["f0", "f1"], [Types.DOUBLE, Types.DOUBLE]), Params().set("predictionCol", "pred"))
    m.loadModel(rows)
    assert m.map((0.0, 0.0))[2] == 1
    assert m.getOutputSchema() == TableSchema(["f0", "f1", "pred"], [Types.DOUBLE, Types.DOUBLE, Types.LONG])


def test_update_sum_matrix_reference():
    """KMeansUtilTest.updateSumMatrix{,Sparse}Test: k=2 centroids (9.1, 9.1, 9.1) / (0.1, 0.1, 0.1); rows i * (1,1,1)
    and the sparse rows with i^2 at index i % 3 (i < 10) give the [k][d + 1] sums + counts
    [35,35,35,5, 10,10,10,5] and [117,65,89,6, 9,1,4,4]."""
    import torch
    from alink_amd.ops.kmeans import assign_accumulate_torch
    C = torch.tensor([[9.1] * 3, [0.1] * 3], dtype=torch.float64)
    X = torch.stack([torch.full((3,), float(i), dtype=torch.float64) for i in range(10)])
    assert assign_accumulate_torch(X, C).flatten().tolist() == [35.0, 35.0, 35.0, 5.0, 10.0, 10.0, 10.0, 5.0]
    X = torch.zeros(10, 3, dtype=torch.float64)
    for i in range(10):
        X[i, i % 3] = i * i
    assert assign_accumulate_torch(X, C).flatten().tolist() == [117.0, 65.0, 89.0, 6.0, 9.0, 1.0, 4.0, 4.0]


def _host_loop_local_kmeans(samples, weights, k, dist_type, max_iter=30, seed=0):
    """The per-pick / per-centroid host loop _local_kmeans replaced (reference seeding rule), kept verbatim as the
    oracle of the device-resident version."""
    import torch
    from alink_amd.models.clustering.kmeans import pairwise_distance, _normalize_rows
    rng = np.random.default_rng(seed)
    n = samples.shape[0]
    w = weights.to(torch.float64)
    D = pairwise_distance(samples, samples, dist_type)
    cum = torch.cumsum(w, 0).cpu().numpy()
    idx = int(min(np.searchsorted(cum, rng.random() * cum[-1], side="left"), n - 1))
    chosen = [idx]
    costs = D[idx].clone()
    for _ in range(1, k):
        cw = torch.cumsum(w * costs, 0).cpu().numpy()
        tot = cw[-1]
        if tot <= 0:
            cand = rng.integers(n, size=1)
        else:
            cand = np.minimum(np.searchsorted(cw, rng.random(1) * tot, side="left"), n - 1)
        cand_t = torch.as_tensor(cand, device=samples.device)
        newc = torch.minimum(costs[None, :], D[cand_t])
        b = int((newc * w[None, :]).sum(1).argmin().item())
        chosen.append(int(cand[b]))
        costs = newc[b]
    C = samples[chosen].clone()
    assign = torch.full((n,), -1, dtype=torch.int64, device=samples.device)
    for _ in range(max_iter):
        a = pairwise_distance(samples, C, dist_type).argmin(1)
        converged = bool(torch.equal(a, assign))
        assign = a
        S = torch.zeros_like(C)
        S.index_add_(0, a, samples * w[:, None])
        cnt = torch.zeros(k, dtype=torch.float64, device=samples.device).index_add_(0, a, w)
        for c in range(k):
            if cnt[c] > 0:
                C[c] = S[c] / cnt[c]
            else:
                C[c] = samples[int(rng.integers(n))]
        if dist_type.upper() == "COSINE":
            C = _normalize_rows(C)
        if converged:
            break
    return C


@pytest.mark.parametrize("n,k,dist,dup", [(220, 20, "EUCLIDEAN", False), (60, 25, "EUCLIDEAN", True),
                                          (150, 10, "COSINE", False), (12, 12, "EUCLIDEAN", True)])
def test_local_kmeans_device_resident_equals_host_loop(n, k, dist, dup, monkeypatch):
    """The device-resident reference-rule seeding + Lloyd (no per-pick / per-centroid host reads) returns exactly
    the centroids of the old host loop, including when picks exhaust the distinct candidates (all-zero totals:
    duplicated rows) and when Lloyd empties clusters (refilled from the same generator draws)."""
    import torch
    from alink_amd.models.clustering import kmeans as km
    monkeypatch.delenv("ALINK_KMEANS_SEEDING", raising=False)
    g = torch.Generator().manual_seed(n + k)
    X = torch.randn(n, 6, generator=g, dtype=torch.float64)
    if dup:
        X = torch.cat([X[: n // 3]] * 3 + [X[: n - 3 * (n // 3)]])
    if dist == "COSINE":
        X = km._normalize_rows(X)
    w = torch.randint(1, 9, (n,), generator=g).to(torch.float64)
    got = km._local_kmeans(X, w, k, dist, seed=3)
    ref = _host_loop_local_kmeans(X, w, k, dist, seed=3)
    assert torch.equal(got, ref)


def test_kmeans_predict_detail_packed_with_nulls():
    """Prediction detail strings come back packed (C++ Double.toString rows); a null vector row reads None."""
    import numpy as np
    import pandas as pd
    from alink_amd import BatchOperator, KMeansPredictBatchOp, KMeansTrainBatchOp
    from alink_amd.common.linalg import DenseVector, VectorUtil
    rng = np.random.default_rng(1)
    X = np.concatenate([rng.standard_normal((30, 2)), rng.standard_normal((30, 2)) + 8])
    vs = [" ".join(map(str, r)) for r in X]
    b = BatchOperator.fromDataframe(pd.DataFrame({"v": vs}), schemaStr="v string")
    m = KMeansTrainBatchOp().setVectorCol("v").setK(2).linkFrom(b)
    t = BatchOperator.fromDataframe(pd.DataFrame({"v": vs[:5] + [None]}), schemaStr="v string")
    rows = KMeansPredictBatchOp().setPredictionCol("p").setPredictionDetailCol("d").linkFrom(m, t).collect()
    assert rows[-1][1] is None and rows[-1][2] is None
    for r in rows[:-1]:
        p = np.array([float(x) for x in r[2].split(" ")])
        assert r[2] == VectorUtil.toString(DenseVector(p)) and abs(p.sum() - 1) < 1e-12


def _numpy_lloyd(X, C, dist, tol, max_iter):
    """Plain Lloyd with the update rule of KMeansUpdateCentroids: empty clusters are dropped, the shift is compared
    only when the previous and the new centroids have the same shape, COSINE renormalises the rows."""
    for _ in range(max_iter):
        idx = (X @ C.T - 0.5 * (C * C).sum(1)).argmax(1)
        cnt = np.bincount(idx, minlength=len(C)).astype(np.float64)
        S = np.zeros_like(C)
        np.add.at(S, idx, X)
        keep = cnt > 0
        new, cnt = S[keep] / cnt[keep, None], cnt[keep]
        if dist == "COSINE":
            new = new / np.linalg.norm(new, axis=1, keepdims=True)
        done = False
        if new.shape == C.shape:
            shift = (1.0 - (new * C).sum(1)) if dist == "COSINE" else np.sqrt(((new - C) ** 2).sum(1))
            done = shift.max() < tol
        C = new
        if done:
            break
    return C, cnt


@pytest.mark.parametrize("dist,tol", [("EUCLIDEAN", 1e-6), ("COSINE", 1e-9)])
def test_generic_update_compacts_empty_cluster(dist, tol):
    """The generic torch update (fp64 rows on the CPU) drops a cluster that no row joins: k shrinks to 3, the
    weights still cover every row, and the centroids equal a numpy Lloyd with the same rule.  Tolerance: the fp64
    sum of 200 O(1) terms carries about 4e-14 of rounding, so 1e-12 absolute."""
    import torch
    from alink_amd.models.clustering.kmeans import train_kmeans
    env = useLocalEnv(1)
    rng = np.random.default_rng(7)
    centres = rng.standard_normal((4, 4)) * 5
    if dist == "COSINE":
        centres = np.abs(centres) + 0.1
    X = centres[rng.integers(0, 4, 200)] + 0.1 * rng.standard_normal((200, 4))
    init = centres + 0.05 * rng.standard_normal((4, 4))
    if dist == "COSINE":
        X = np.abs(X) + 1e-3                                        # positive orthant
        init = np.abs(init)
        init /= np.linalg.norm(init, axis=1, keepdims=True)
        init[1] = -init[0]                                          # farthest from every row
        Xn = X / np.linalg.norm(X, axis=1, keepdims=True)           # train_kmeans normalises the rows
    else:
        init[1] = 1e4                                               # no row joins it
        Xn = X
    _, q = train_kmeans(torch.from_numpy(X), 4, 20, tol, dist, "RANDOM", 2, "v", env,
                        init_centroids=torch.from_numpy(init))
    ctx = q.final_contexts[0]
    assert ctx.getObj("k") == 3
    w = ctx.getObj("lastWeights").numpy()
    assert w.sum() == 200
    c1, c2 = ctx.getObj("centroid1"), ctx.getObj("centroid2")
    got = (c1 if c1[0] > c2[0] else c2)[1][:3].numpy()
    want, cnt = _numpy_lloyd(Xn, init, dist, tol, 20)
    assert want.shape == (3, 4) and np.array_equal(cnt, w)
    err = np.abs(got - want).max()
    print(f"{dist}: {len(q.stats)} supersteps, max |centroid - numpy| = {err:.3e}")
    assert err <= 1e-12
