"""The v10 KMeans kernel's accumulate role after its trim: one generated body per tile pair (paired row reads,
tile B's reads refilled into the registers tile A's rows have just left, the pair's ids read as one dword per lane)
and a main loop split into iteration 0, the steady iterations 1 <= j < np - 3 (np = tile pairs of the workgroup) and
the last ones.

grid 1, n = 64 t + o: t = 1 a lone tile; 2 one pair; 3 an odd tail tile; 4, 5 no steady iteration yet (np <= 3);
9, 10 the first steady iteration (np = 5); 11 an odd tail behind it (np = 6); 19 steady iterations that wrap the 9-slot
ring, the last steady iteration and the first of the tail loop.  Then uneven regions of 2 and 3 workgroups.

Everything is exact: C is integer-valued with |c| <= 45, a row is its centroid plus a vector in {-1, 0, 1}, so rows
differ from each other, every score and every fp32 partial sum is an exactly representable number in any order, and
the margin between the best and the second-best centroid is in the thousands.  The ids must equal the fp64 argmax
and the returned [k, 129] the fp64 sums of X by them, bit for bit: a row read refilled into a register before its
last reader, paired with the wrong partner row, or added under another row's id is an exact mismatch.  Row
arrangements (labels by row number r, as far as k allows):
  each   r mod k through a stride: every row of a pair goes to a different centroid (k = 112: 112 of 128 rows)
  run4   runs of 4 consecutive rows share a centroid -- one accumulate wave's m = 0..3 of one q
  run16  runs of 16 consecutive rows share one -- a whole q of all four waves
  split  tile A and tile B of every pair use disjoint halves of the centroids
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

_TILES = (1, 2, 3, 4, 5, 9, 10, 11, 19)
_SHAPES = [(64 * t + o, 1) for t in _TILES for o in (-1, 0, 1)] + [(1217, 2), (1217, 3)]
_KS = (1, 17, 100, 112)
_ARR = ("each", "run4", "run16", "split")

_C = {}
_E = {}


def _c(k):
    """Distinct integer-valued centroids, generated once per k and never modified."""
    if k not in _C:
        g = torch.Generator(device="cuda").manual_seed(8200 + k)
        _C[k] = torch.round(torch.randn(k, 128, device="cuda", generator=g, dtype=torch.float64) * 8).clamp_(-45, 45)
    return _C[k]


def _e(n):
    if n not in _E:
        g = torch.Generator(device="cuda").manual_seed(8300 + n)
        _E[n] = torch.randint(-1, 2, (n, 128), device="cuda", generator=g).double()
    return _E[n]


def _labels(arr, n, k):
    r = torch.arange(n, device="cuda")
    if arr == "each":
        return (r * 37) % k                      # 37 is coprime to every k here: k consecutive rows all differ
    if arr == "run4":
        return (r // 4 * 37) % k
    if arr == "run16":
        return (r // 16 * 37) % k
    half = max(k // 2, 1)
    odd = (r // 64) % 2                          # tile B of its pair
    return torch.where(odd == 0, (r * 37) % half, (half + (r * 37) % (k - half)) % k if k > 1 else r * 0)


def _exact(X, ids, k):
    a = ids.long()
    ref = torch.zeros((k, 129), dtype=torch.float64, device=X.device)
    ref[:, :128].index_add_(0, a, X.double())
    ref[:, 128].index_add_(0, a, torch.ones(X.shape[0], dtype=torch.float64, device=X.device))
    return ref


@pytest.mark.parametrize("k", _KS)
@pytest.mark.parametrize("n,grid", _SHAPES)
def test_v10_accumulate_pair_exact(n, grid, k, monkeypatch):
    from alink_amd.ops import kmeans as K
    C = _c(k)
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v10")
    assert K.kernel_version(k) == "v10"
    for arr in _ARR:
        lab = _labels(arr, n, k)
        X64 = C[lab] + _e(n)
        X = X64.to(torch.bfloat16)
        assert torch.equal(X.double(), X64)
        score = X64 @ C.T - 0.5 * (C * C).sum(1)[None, :]
        want = score.argmax(1).int()
        assert torch.equal(want.long(), lab), "the arrangement's rows must go to their own centroid"
        if k > 1:
            top = score.topk(2, dim=1).values
            assert float((top[:, 0] - top[:, 1]).min()) > 100.0      # no ties anywhere near
        ref = _exact(X, want, k)
        for flags in (0, 1):
            monkeypatch.setattr(K, "V10_FLAGS", flags)
            for rev in (False, True):
                where = (n, grid, k, arr, flags, rev)
                ids = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                got = K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids, reverse=rev)
                bare = K.assign_accumulate_hip(X, C, grid=grid, reverse=rev)
                ids2 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                again = K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids2, reverse=rev)
                assert torch.equal(ids, want), (where, "ids differ from the fp64 argmax")
                assert torch.equal(got, ref), (where, "sums differ from the fp64 sums")
                assert torch.equal(bare, got), (where, "result depends on assign_out")
                assert torch.equal(again.view(torch.int64), got.view(torch.int64)) and torch.equal(ids2, ids), \
                    (where, "two launches differ")
