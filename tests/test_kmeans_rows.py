"""The KMeans rows object (``ops/kmeans_rows.py``) without a GPU: the kind is chosen when the object is built, and every
operation is the expression it replaced in ``models/clustering/kmeans.py``, bit for bit."""
import pytest
import torch

N, D, K = 53, 7, 5
LOW = (torch.bfloat16, torch.float16)


def _normalize(X):
    from alink_amd.models.clustering.kmeans import _normalize_rows
    return _normalize_rows(X.to(torch.float64)) if X.dtype == torch.float64 else _normalize_rows(X.float()).to(X.dtype)


def _centroids(dist):
    C = torch.randn((K, D), dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    C[K - 1] = C[1]                                 # one duplicated centroid: the tie goes to the lower index
    return _normalize(C) if dist == "COSINE" else C


def _tensor(dtype, dist, n=N):
    X = torch.randn((n, D), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(dtype)
    return _normalize(X) if dist == "COSINE" else X


def _sparse(dist, n=N):
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops.kmeans_rows import sparse_rows
    g = torch.Generator().manual_seed(3)
    X = torch.randn((n, D), dtype=torch.float64, generator=g) * (torch.rand((n, D), generator=g) < 0.4)
    nz = X != 0
    crow = torch.zeros(n + 1, dtype=torch.int64)
    crow[1:] = nz.sum(1).cumsum(0)
    fm = FeatureMatrix(crow=crow, col=nz.nonzero()[:, 1], val=X[nz], ncols=D)
    return sparse_rows(fm, D, dist)


def _spy(monkeypatch, mod, name):
    calls, orig = [], getattr(mod, name)
    monkeypatch.setattr(mod, name, lambda *a, **k: (calls.append(name), orig(*a, **k))[1])
    return calls


@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16])
def test_tensor_rows_are_the_torch_expressions(dtype, dist):
    from alink_amd.models.clustering.kmeans import pairwise_distance
    from alink_amd.ops import kmeans as kops, kmeans_rows as kr
    X, C = _tensor(dtype, dist), _centroids(dist)
    r = kr.rows(X, dist.lower())
    assert type(r) is kr._TorchRows and (r.n, r.d, r.device) == (N, D, X.device) and r.fused_update
    cd = torch.float32 if dtype in LOW else dtype
    want = pairwise_distance(X.to(cd), C.to(cd), dist)
    idx, dist_v = r.nearest(C)
    assert idx.dtype == torch.int64 and torch.equal(idx, want.argmin(1))
    assert dist_v.dtype == torch.float64 and torch.equal(dist_v, want.min(1).values.to(torch.float64))
    assert not bool((idx == K - 1).any())
    idx2, dist2 = r.nearest(C, r.distances(C))      # what the mapper does when it holds every distance
    assert torch.equal(idx2, idx) and torch.equal(dist2, want.double().min(1).values)
    cost, total = r.first_cost(C[:1])
    one = pairwise_distance(X.to(cd), C[:1].to(cd), dist).min(1).values.to(torch.float64)
    assert torch.equal(cost, one) and torch.equal(total, one.sum())
    assert torch.equal(r.nearest_counts(C), torch.bincount(want.argmin(1), minlength=K))
    for step in (1, 2):
        assert torch.equal(r.assign_accumulate(C, step),
                           kops.assign_accumulate(X, C, reverse=kops.serpentine_reverse(step)))
    pick = torch.tensor([5, 0, 52, 5])
    assert torch.equal(r.take(pick), X[pick].to(torch.float64))
    assert r.queue_assign(K) is None                 # nothing to queue ahead without the fused kernel


@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
def test_sparse_rows_are_the_sparse_calls(dist, monkeypatch):
    from alink_amd.ops import kmeans_rows as kr, kmeans_sparse as ksp
    fm, C = _sparse(dist), _centroids(dist)
    r = kr.rows(fm, dist)
    assert type(r) is kr._SparseRows and (r.n, r.d) == (N, D) and not r.fused_update and r.queue_assign(K) is None
    idx_w, d2 = ksp.nearest(fm, C, dist)
    dist_w = d2.sqrt() if dist == "EUCLIDEAN" else d2
    counts_w = ksp.nearest_counts(fm, C, dist)
    buf_w = ksp.assign_accumulate(fm, C, dist)
    one = ksp.nearest(fm, C[:1], dist)[1]
    one = one.sqrt() if dist == "EUCLIDEAN" else one
    near = _spy(monkeypatch, ksp, "nearest")
    accum = _spy(monkeypatch, ksp, "assign_accumulate")
    idx, dist_v = r.nearest(C)
    assert near == ["nearest"] and torch.equal(idx, idx_w) and torch.equal(dist_v, dist_w)
    assert not bool((idx == K - 1).any())
    cost, total = r.first_cost(C[:1])
    assert near == ["nearest"] * 2 and torch.equal(cost, one) and torch.equal(total, one.sum())
    assert torch.equal(r.nearest_counts(C), counts_w) and near == ["nearest"] * 2
    assert torch.equal(r.assign_accumulate(C, 1), buf_w) and accum == ["assign_accumulate"]
    pick = torch.tensor([5, 0, 52, 5])
    assert torch.equal(r.take(pick), ksp.take_dense(fm, pick))
    # the [n, k] distances of the detail column: their row minimum is the kernel's distance within the tests' slack
    # (4 x 2 m 2^-53 sum|terms| with m = d + 2 terms, each of size <= (|x| + |c|)^2)
    every = r.distances(C)
    xc = (fm.to_dense().norm(dim=1)[:, None] + C.norm(dim=1)[None, :]) ** 2
    sq = (lambda t: t * t) if dist == "EUCLIDEAN" else (lambda t: t)
    assert every.shape == (N, K) and every.dtype == torch.float64
    assert bool(((sq(every.min(1).values) - sq(dist_v)).abs() <= 8.0 * (D + 2) * 2.0 ** -53 * xc.max(1).values).all())


def test_sparse_rows_refuse_other_distances():
    from alink_amd.ops import kmeans_rows as kr
    with pytest.raises(ValueError):
        kr.rows(_sparse("EUCLIDEAN"), "HAVERSINE")


@pytest.mark.parametrize("kind", ["sparse", torch.float64, torch.float32, torch.bfloat16])
def test_empty_partition_gives_shaped_zeros_and_launches_nothing(kind, monkeypatch):
    from alink_amd.ops import _lib, kmeans_rows as kr
    launched = _spy(monkeypatch, _lib, "call")
    C = _centroids("EUCLIDEAN")
    r = kr.rows(_sparse("EUCLIDEAN", 0) if kind == "sparse" else _tensor(kind, "EUCLIDEAN", 0), "EUCLIDEAN")
    assert (r.n, r.d) == (0, D)
    idx, dist = r.nearest(C)
    assert idx.shape == (0,) and idx.dtype == torch.int64 and dist.shape == (0,) and dist.dtype == torch.float64
    cost, total = r.first_cost(C[:1])
    assert cost.shape == (0,) and cost.dtype == torch.float64 and float(total) == 0.0
    assert torch.equal(r.nearest_counts(C), torch.zeros(K, dtype=torch.int64))
    assert torch.equal(r.assign_accumulate(C, 1), torch.zeros((K, D + 1), dtype=torch.float64))
    assert r.take(torch.zeros(0, dtype=torch.int64)).shape == (0, D)
    assert r.distances(C).shape == (0, K) and r.queue_assign(K) is None
    assert launched == []


def test_dense64_flag_is_read_when_the_object_is_built(monkeypatch):
    """On a CPU ``dense64_supported`` is patched to accept the rows, so the flag alone decides; ``kd64.nearest`` then
    runs its torch body."""
    from alink_amd.ops import kmeans_dense64 as kd64, kmeans_rows as kr
    monkeypatch.setattr(kd64, "dense64_supported", lambda X, k: True)
    X, C = _tensor(torch.float64, "EUCLIDEAN"), _centroids("EUCLIDEAN")
    monkeypatch.delenv("ALINK_KMEANS_DENSE64", raising=False)
    on = kr.rows(X, "EUCLIDEAN")
    monkeypatch.setenv("ALINK_KMEANS_DENSE64", "0")
    off = kr.rows(X, "EUCLIDEAN")
    assert type(on) is kr._Dense64Rows and type(off) is kr._TorchRows
    monkeypatch.delenv("ALINK_KMEANS_DENSE64")
    near = _spy(monkeypatch, kd64, "nearest")
    counts = _spy(monkeypatch, kd64, "nearest_counts")
    off.nearest(C), off.first_cost(C[:1]), off.nearest_counts(C)
    assert near == [] and counts == []               # built with the flag off: stays on torch
    monkeypatch.setenv("ALINK_KMEANS_DENSE64", "0")
    idx, dist = on.nearest(C)                        # built with the flag on: stays on the dense fp64 family
    on.first_cost(C[:1]), on.nearest_counts(C)
    assert near == ["nearest"] * 2 and counts == ["nearest_counts"]
    want = kd64.nearest_torch(X, C, "EUCLIDEAN")
    assert torch.equal(idx, want[0]) and torch.equal(dist, want[1].sqrt())
    assert near == ["nearest"] * 2                   # nearest_torch is not the spied entry point


def test_column_kind():
    from alink_amd.common.linalg import SparseVector
    from alink_amd.common.linalg.block import SparseBlock
    from alink_amd.ops.kmeans_rows import DENSE, SPARSE, UNDECIDED, column_kind
    z = torch.zeros(0, dtype=torch.int64)
    assert column_kind(torch.zeros((2, 3))) == DENSE
    assert column_kind(SparseBlock(torch.zeros(1, dtype=torch.int64), z, z.double(), 4)) == SPARSE
    assert column_kind([None, "$4$1:2.0"]) == SPARSE and column_kind(["0:1.0 3:2.0"]) == SPARSE
    assert column_kind([None, SparseVector(4, [1], [2.0])]) == SPARSE
    assert column_kind(["1.0 2.0"]) == DENSE and column_kind([None, None]) == UNDECIDED and column_kind([]) == UNDECIDED
