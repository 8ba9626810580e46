"""The v10 KMeans kernel's tile pipeline at its edges: ring wraps, short and odd tile counts, rows past N, uneven
regions -- checked EXACTLY.  X is integer-valued bf16 in [-3, 3], so every fp32 partial sum is exact in any order and
the returned [k, 129] must equal the fp64 sums of X by the kernel's own assignment bit for bit: a wrong register
index, a row read before its DMA landed, or a row dropped or doubled at a ring wrap is an exact mismatch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# grid = 1: fewer tiles than are staged ahead (7), odd tile counts (a pair's second tile missing), one and two wraps
# of the 9-slot ring, and one row short of / past a tile edge; then uneven regions and a full grid
_TILES = (1, 2, 3, 6, 7, 8, 9, 10, 17, 18, 19)
_SHAPES = [(64 * t + o, 1) for t in _TILES for o in (-1, 0, 1)] + [(1217, 2), (1217, 3), (300001, None)]
_KS = (1, 16, 17, 96, 97, 100, 112)

_X = {}


def _x(n):
    """Integer-valued rows, generated once per n and never modified."""
    if n not in _X:
        g = torch.Generator(device="cuda").manual_seed(1000 + n)
        _X[n] = torch.randint(-3, 4, (n, 128), device="cuda", generator=g).to(torch.bfloat16)
    return _X[n]


def _c(k):
    g = torch.Generator(device="cuda").manual_seed(77 + k)
    return torch.randn(k, 128, device="cuda", generator=g, dtype=torch.float64) * 1.5


def _exact(X, ids, k):
    a = ids.long()
    ref = torch.zeros((k, 129), dtype=torch.float64, device=X.device)
    ref[:, :128].index_add_(0, a, X.double())
    ref[:, 128].index_add_(0, a, torch.ones(X.shape[0], dtype=torch.float64, device=X.device))
    return ref


@pytest.mark.parametrize("k", _KS)
@pytest.mark.parametrize("n,grid", _SHAPES)
def test_v10_pipeline_exact_sums(n, grid, k, monkeypatch):
    from alink_amd.ops import kmeans as K
    X, C = _x(n), _c(k)
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v7")
    ids7 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids7)
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v10")
    assert K.kernel_version(k) == "v10"
    ref = None
    for rev in (False, True):
        ids = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        got = K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids, reverse=rev)
        bare = K.assign_accumulate_hip(X, C, grid=grid, reverse=rev)
        ids2 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        again = K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids2, reverse=rev)
        assert int(ids.min()) >= 0 and int(ids.max()) < k, (n, grid, k, rev)
        assert torch.equal(ids, ids7), (n, grid, k, rev, "v10 ids differ from v7")
        if ref is None:
            ref = _exact(X, ids, k)
        assert torch.equal(got, ref), (n, grid, k, rev, "sums differ from the fp64 sums of the kernel's own ids")
        assert torch.equal(bare, got), (n, grid, k, rev, "result depends on assign_out")
        assert torch.equal(again.view(torch.int64), got.view(torch.int64)) and torch.equal(ids2, ids), \
            (n, grid, k, rev, "two launches differ")
