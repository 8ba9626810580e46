"""The v10 KMeans kernel's static split over several workgroups, checked EXACTLY at the shapes where the split, the
pair logic and the buffer bounds meet: fewer tiles than workgroups, as many, one more; unequal and odd tile counts,
also in a workgroup that is not the last one (its phantom second tile lies inside X, in the next workgroup's rows,
and must still read as zeros); a partial last tile; and enough tiles per workgroup for the 9-slot ring to wrap.
tests/test_kmeans_v10_ring_gpu.py walks the ring with one workgroup; this file is about the grid.  It is a regression
test of the split the kernel has always had (contiguous runs of `per` tiles), run under both cache policies of the
X stream; it came with the measurement of a swept tile order that was not built (profiles/kmeans_v10_sweep.txt).

Everything is exact, as in tests/test_kmeans_v10_pairmax_gpu.py: C and X are integer-valued with |c|, |x| <= 45, so
they are exact in bf16, every score is exact in fp32 in any order, and every fp32 partial sum of X is an integer far
below 2^24.  Ids, counts and sums must therefore equal the fp64 oracle (ties to the lowest index) bit for bit,
whatever the grouping of rows into workgroups, forward and serpentine; no row may stay unwritten, and two launches
must agree bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

K_ = 100
# (rows, grid): tiles 3 < 7 | 4 == 4 | 5 = 4 + 1 (a last tile of one row) | 5 = 4 + 1 whole tiles |
# 165 tiles on 7 workgroups of 24 (the last: 21, partial last tile) | 67 on 3 of 23 (odd; the last: 21, partial) |
# 86 on 4 of 22 (the last: 20), whole tiles | 23 on 3 of 8 (the last: 7, one row in its last tile)
_SHAPES = [(133, 7), (253, 4), (257, 4), (320, 4), (10513, 7), (4248, 3), (5504, 4), (1409, 3)]

_DATA = {}


def _case(n):
    """(X bf16 [n, 128], C fp64 [100, 128], fp64 argmax ids, fp64 sums|counts) -- made once, never modified."""
    if n not in _DATA:
        g = torch.Generator(device="cuda").manual_seed(7100 + n)
        C = torch.round(torch.randn(K_, 128, device="cuda", generator=g, dtype=torch.float64) * 8).clamp_(-45, 45)
        lab = torch.randint(0, K_, (n,), device="cuda", generator=g)
        noise = torch.randint(-2, 3, (n, 128), device="cuda", generator=g).double()
        X64 = (C[lab] + noise).clamp_(-45, 45)
        X = X64.to(torch.bfloat16)
        assert torch.equal(X.double(), X64) and torch.equal(C.to(torch.bfloat16).double(), C)
        score = X64 @ C.T - 0.5 * (C * C).sum(1)[None, :]
        best = score.max(1, keepdim=True).values
        cols = torch.arange(K_, device="cuda")[None, :].expand(n, K_)
        want = torch.where(score == best, cols, torch.full_like(cols, K_)).min(1).values.int()
        ref = torch.zeros((K_, 129), dtype=torch.float64, device="cuda")
        ref[:, :128].index_add_(0, want.long(), X64)
        ref[:, 128].index_add_(0, want.long(), torch.ones(n, dtype=torch.float64, device="cuda"))
        _DATA[n] = (X, C, want, ref)
    return _DATA[n]


@pytest.mark.parametrize("flags", (0, 1))
@pytest.mark.parametrize("n,grid", _SHAPES)
def test_v10_grid_exact(n, grid, flags, monkeypatch):
    """flags: 0 = non-temporal X loads (the production launch), 1 = default-policy loads."""
    from alink_amd.ops import kmeans as K
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v10")
    monkeypatch.setattr(K, "V10_FLAGS", flags)
    assert K.kernel_version(K_) == "v10"
    X, C, want, ref = _case(n)
    for rev in (False, True):
        ids = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        got = K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids, reverse=rev)
        ids2 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        again = K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids2, reverse=rev)
        tag = (n, grid, flags, rev)
        assert int((ids < 0).sum()) == 0, (tag, "rows never written")
        assert float(got[:, 128].sum()) == float(n), (tag, "counts do not sum to N")
        assert torch.equal(ids, want), (tag, "ids differ from the fp64 argmax")
        assert torch.equal(got, ref), (tag, "sums or counts differ from the fp64 oracle")
        assert torch.equal(ids2, ids) and torch.equal(again.view(torch.int64), got.view(torch.int64)), \
            (tag, "two launches differ")
