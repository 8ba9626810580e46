"""The v10 KMeans kernel's 9-slot tile ring -- checked EXACTLY at the tile counts where its lookahead (and a deeper one:
the shapes are those at which staging tiles 2j+7 and 2j+8 in iteration j, by the slot's owning accumulate wave, can
go wrong) meets the ring's wraps.  X is integer-valued bf16 in [-3, 3], so every fp32 partial sum is exact in any
order and the returned [k, 129] must equal the fp64 sums of X by the kernel's own assignment bit for bit: a slot
refilled before its last reader was done, a tile staged twice, out of order or not at all, or a row read before its
DMA landed is an exact mismatch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# grid = 1, n = 64 t + o.  t = 8, 9: fewer tiles than / exactly as many as the ring has slots (all staged before the
# first slot is reused); 10..12: the first refilled slots; 18..20, 27..29, 37: two, three and four wraps of the ring.
# Then uneven regions of 2 and 3 workgroups.
_TILES = (8, 9, 10, 11, 12, 18, 19, 20, 27, 28, 29, 37)
_SHAPES = [(64 * t + o, 1) for t in _TILES for o in (-1, 0, 1)] + [(1217, 2), (1217, 3), (2369, 2), (2369, 3)]
_KS = (1, 17, 97, 100, 112)

_X = {}


def _x(n):
    """Integer-valued rows, generated once per n and never modified."""
    if n not in _X:
        g = torch.Generator(device="cuda").manual_seed(5000 + n)
        _X[n] = torch.randint(-3, 4, (n, 128), device="cuda", generator=g).to(torch.bfloat16)
    return _X[n]


def _c(k):
    g = torch.Generator(device="cuda").manual_seed(177 + k)
    return torch.randn(k, 128, device="cuda", generator=g, dtype=torch.float64) * 1.5


def _exact(X, ids, k):
    a = ids.long()
    ref = torch.zeros((k, 129), dtype=torch.float64, device=X.device)
    ref[:, :128].index_add_(0, a, X.double())
    ref[:, 128].index_add_(0, a, torch.ones(X.shape[0], dtype=torch.float64, device=X.device))
    return ref


@pytest.mark.parametrize("k", _KS)
@pytest.mark.parametrize("n,grid", _SHAPES)
def test_v10_ring_exact_sums(n, grid, k, monkeypatch):
    from alink_amd.ops import kmeans as K
    X, C = _x(n), _c(k)
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v7")
    ids7 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids7)
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v10")
    assert K.kernel_version(k) == "v10"
    ref = _exact(X, ids7, k)
    for rev in (False, True):
        ids = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        got = K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids, reverse=rev)
        bare = K.assign_accumulate_hip(X, C, grid=grid, reverse=rev)
        ids2 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        again = K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids2, reverse=rev)
        assert torch.equal(ids, ids7), (n, grid, k, rev, "v10 ids differ from v7")
        assert torch.equal(got, _exact(X, ids, k)), \
            (n, grid, k, rev, "sums differ from the fp64 sums of the kernel's own ids")
        assert torch.equal(got, ref), (n, grid, k, rev)
        assert torch.equal(bare, got), (n, grid, k, rev, "result depends on assign_out")
        assert torch.equal(again.view(torch.int64), got.view(torch.int64)) and torch.equal(ids2, ids), \
            (n, grid, k, rev, "two launches differ")
