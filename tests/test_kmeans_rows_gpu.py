"""The KMeans rows object (``ops/kmeans_rows.py``) on the GPU: every kind launches its own kernel family and nothing
else, and every operation is the direct ``ops`` call it stands for.

Equality is ``torch.equal`` except where the direct call itself sums with float atomics, so that two calls of it
may differ:

* the two-pass bf16 path away from d = 128 (``assign_accumulate_general_hip``): counts exact, sums within the
  ``rtol = 2e-5, atol = 2e-3`` of ``test_kmeans_general_gpu.py``;
* the fp32 path (``alink_kmeans_accum_f32`` adds into an fp64 LDS table by atomics): counts exact, and two fp64
  evaluations of a sum over the m rows of a cluster differ by at most ``2 m 2^-53 sum|x|``; 4x that, from the data.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, K = 1027, 5          # no tile, wave or 32-row group divides n
EPS = 2.0 ** -53
COUNTERS = ("HIP_CALLS", "GENERAL_CALLS", "F32_CALLS", "DENSE64_CALLS", "SPARSE_CALLS")
CASES = ("bf16_64", "bf16_128", "bf16_256", "fp64_37", "fp32_128", "csr_2000")
INDEPENDENT = {"alink_kmeans_par_pick", "alink_kmeans_seed_ref", "alink_kmeans_local_lloyd"}
FAMILY = {"bf16": {"alink_kmeans_cost1_bf16", "alink_kmeans_nearest_bf16"}, "fp64": {"alink_kmeans_dense64_nearest"},
          "fp32": set(), "csr": {"alink_kmeans_sparse_nearest"}}


def _counters():
    from alink_amd.ops import kmeans as kops, kmeans_dense64 as kd64, kmeans_sparse as ksp
    return {"HIP_CALLS": kops.HIP_CALLS, "GENERAL_CALLS": kops.GENERAL_CALLS, "F32_CALLS": kops.F32_CALLS,
            "DENSE64_CALLS": kd64.DENSE64_CALLS, "SPARSE_CALLS": ksp.SPARSE_CALLS}


def _moved(before):
    return {c: v - before[c] for c, v in _counters().items() if v != before[c]}


@functools.lru_cache(maxsize=None)
def _case(case):
    """(rows as ``rows()`` takes them, centroids [K, d] fp64 with centroid K - 1 a copy of centroid 1), on the GPU;
    built once per case and left unchanged."""
    kind, d = case.split("_")
    d = int(d)
    g = torch.Generator().manual_seed(17 + d)
    cen = torch.randn((K, d), generator=g, dtype=torch.float64) * 3.0
    X = cen[torch.arange(N) % (K - 1)] + torch.randn((N, d), generator=g, dtype=torch.float64)
    if kind == "csr":
        from alink_amd.models.common.features import FeatureMatrix
        X = X * (torch.rand((N, d), generator=g) < 0.01)
        nz = X != 0
        crow = torch.zeros(N + 1, dtype=torch.int64)
        crow[1:] = nz.sum(1).cumsum(0)
        X = FeatureMatrix(crow=crow.cuda(), col=nz.nonzero()[:, 1].cuda(), val=X[nz].cuda(), ncols=d)
        cen = cen * 0.05
    else:
        X = X.to({"bf16": torch.bfloat16, "fp64": torch.float64, "fp32": torch.float32}[kind]).cuda().contiguous()
    if kind == "bf16":
        cen = cen.to(torch.bfloat16).double()           # candidates are rows: exactly representable
    cen[K - 1] = cen[1]
    return X, cen.cuda()


def _direct(case, X, C):
    """The direct ``ops`` calls the four operations stand for, and the counter each may move."""
    from alink_amd.models.clustering.kmeans import pairwise_distance
    from alink_amd.ops import kmeans as kops, kmeans_dense64 as kd64, kmeans_sparse as ksp
    kind, d = case.split("_")

    def lloyd(step):
        return kops.assign_accumulate(X, C, reverse=kops.serpentine_reverse(step))

    if kind == "bf16":
        def nearest(Cc):
            idx, d2 = kops.nearest_hip(X, Cc)
            return idx.to(torch.int64), d2.to(torch.float64).sqrt()

        def first(c):
            cost, psum = kops.cost1_hip(X, c[0], with_sum=True)
            return cost, psum.sum()
        return nearest, first, lambda Cc: kops.nearest_counts_hip(X, Cc), lloyd, \
            (None, None, None, "HIP_CALLS" if d == "128" else "GENERAL_CALLS")
    if kind == "fp32":
        def nearest(Cc):
            best = pairwise_distance(X, Cc.float(), "EUCLIDEAN").min(1)
            return best.indices, best.values.double()
        move = (None, None, None, "F32_CALLS")
    else:
        mod, name = (kd64, "DENSE64_CALLS") if kind == "fp64" else (ksp, "SPARSE_CALLS")

        def nearest(Cc):
            idx, d2 = mod.nearest(X, Cc, "EUCLIDEAN")
            return idx, d2.sqrt()
        move = (name,) * 4
        if kind == "csr":
            return nearest, lambda c: (nearest(c)[1], nearest(c)[1].sum()), \
                lambda Cc: ksp.nearest_counts(X, Cc, "EUCLIDEAN"), \
                lambda step: ksp.assign_accumulate(X, C, "EUCLIDEAN"), move
    counts = (lambda Cc: kd64.nearest_counts(X, Cc, "EUCLIDEAN")) if kind == "fp64" else \
        (lambda Cc: torch.bincount(nearest(Cc)[0], minlength=Cc.shape[0]))
    return nearest, lambda c: (nearest(c)[1], nearest(c)[1].sum()), counts, lloyd, move


@pytest.mark.parametrize("case", CASES)
def test_operations_are_the_direct_calls_of_one_family(case, monkeypatch):
    from alink_amd.ops import kmeans_rows as kr
    monkeypatch.setenv("ALINK_KMEANS_SPARSE", "1")
    X, C = _case(case)
    kind = case.split("_")[0]
    r = kr.rows(X, "EUCLIDEAN")
    assert type(r) is {"bf16": kr._Bf16Rows, "fp64": kr._Dense64Rows, "fp32": kr._TorchRows,
                       "csr": kr._SparseRows}[kind]
    assert (r.n, r.d) == (N, int(case.split("_")[1])) and r.device == C.device
    nearest, first, counts, lloyd, move = _direct(case, X, C)
    want = (nearest(C), first(C[:1]), counts(C), lloyd(2))
    torch.cuda.synchronize()
    ops = (lambda: r.nearest(C), lambda: r.first_cost(C[:1]), lambda: r.nearest_counts(C),
           lambda: r.assign_accumulate(C, 2))
    got = []
    for op, name in zip(ops, move):
        before = _counters()
        got.append(op())
        assert set(_moved(before)) == ({name} if name else set()), (case, _moved(before))
    torch.cuda.synchronize()
    assert torch.equal(got[0][0], want[0][0]) and torch.equal(got[0][1], want[0][1])
    assert got[0][0].dtype == torch.int64 and got[0][1].dtype == torch.float64
    assert not bool((got[0][0] == K - 1).any())                 # the duplicated centroid loses the tie
    assert torch.equal(got[1][0], want[1][0]) and torch.equal(got[1][1], want[1][1])
    assert torch.equal(got[2], want[2]) and int(got[2].sum()) == N
    buf, ref = got[3], want[3]
    assert torch.equal(buf[:, -1], ref[:, -1]) and float(buf[:, -1].sum()) == N
    if case in ("bf16_64", "bf16_256"):
        print(case, "max |sum difference|", float((buf - ref).abs().max()))
        torch.testing.assert_close(buf, ref, rtol=2e-5, atol=2e-3)
    elif kind == "fp32":
        absum = torch.zeros_like(ref[:, :-1]).index_add_(0, got[0][0], X.double().abs())
        bound = 4.0 * 2.0 * ref[:, -1:] * EPS * absum
        print(case, "max |sum difference|", float((buf - ref).abs().max()), "min bound", float(bound.min()))
        assert bool(((buf[:, :-1] - ref[:, :-1]).abs() <= bound).all())
    else:
        assert torch.equal(buf, ref)
    pick = torch.tensor([5, 0, N - 1, 5], device=C.device)
    dense = X.to_dense() if kind == "csr" else X
    assert torch.equal(r.take(pick), dense[pick].to(torch.float64))
    # only the fused bf16 kernel (d = 128, k <= 128) has a next superstep to queue ahead
    assert (r.queue_assign(K) is not None) == (case == "bf16_128") and r.fused_update == (kind != "csr")


@pytest.mark.parametrize("case", CASES)
def test_kmeans_parallel_init_stays_in_its_family(case, monkeypatch):
    from alink_amd import useLocalEnv
    from alink_amd.models.clustering.kmeans import kmeans_init
    from alink_amd.ops import _lib
    monkeypatch.setenv("ALINK_KMEANS_SPARSE", "1")
    useLocalEnv(1, device="cuda:0")
    X, _ = _case(case)
    names, orig = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
    init = kmeans_init(X, K, "K_MEANS_PARALLEL", 2, "EUCLIDEAN", seed=3)
    torch.cuda.synchronize()
    family = FAMILY[case.split("_")[0]]
    assert set(names) <= family | INDEPENDENT, sorted(set(names))
    assert family <= set(names), sorted(set(names))              # the cost pass and the weights pass both ran
    assert init.shape == (K, int(case.split("_")[1])) and bool(torch.isfinite(init).all())
