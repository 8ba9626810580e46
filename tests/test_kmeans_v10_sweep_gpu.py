"""The v10 KMeans kernel on the swept tile order (alink_amd/ops/csrc/kmeans_v10_map.h), checked EXACTLY where the
mapping, the pair logic, the windowed buffer resource and the buffer bounds meet.  tests/test_kmeans_v10_map.py checks
the index arithmetic on the CPU; this file runs the kernel on it.

Workgroup b of G owns the tiles b, b + G, ... (chunks of S of them), and addresses them through a buffer resource per
window of owned tiles.  The production window is hundreds of tiles long, so a small launch never leaves its first one;
mode bits 8-23 set the window, and 3 and 4 owned tiles make the kernel re-base every other pair, in both directions,
on the first tile of a pair (4; 3 at every second window) and on the last (3).  The shapes: fewer tiles than
workgroups, as many, one more; tile counts that are no multiple of G or G * S, so that workgroups own unequal counts
and the last chunk is short; odd owned counts in workgroups that are not the last (their phantom second tile must
count for nothing, wherever its index falls); a last tile of one row; more than 20 owned tiles per workgroup, so that
the 9-slot ring wraps.

Everything is exact, as in tests/test_kmeans_v10_grids_gpu.py: C and X are integer-valued with |c|, |x| <= 45, so
they are exact in bf16, every score is exact in fp32 in any order, and every fp32 partial sum of X is an integer far
below 2^24.  Ids, counts and sums must equal the fp64 oracle (ties to the lowest index) bit for bit, whatever the
grouping of rows into workgroups, with and without the id output; no row may stay unwritten, the counts sum to N, and
two launches agree bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (rows, grid); the grid is the one asked for, the launch clamps it to the chunk count.  Owned tiles per workgroup with
# the chunk that ships, S = 1:
#   3 tiles on 7 (fewer than workgroups) | 4 on 4 (as many) | 5 on 4 (one more; a last tile of one row at 257 rows)
#   10 on 3 (4 3 3) | 23 on 3 (8 8 7; one row in the last tile) | 27 on 3 (9 9 9: odd everywhere; one row in the last)
#   85 on 4 (22 21 21 21) | 165 on 7 (24 x 4, 23 x 3: odd counts in workgroups that are not the last; partial last tile)
#   67 on 3 (23 22 22) | 86 on 4 (22 22 21 21) | 188 on 7 (27 x 6, 26): the ring wraps
# and with the A/B chunk S = 8 (tiles -> chunks): 3, 4, 5 tiles: one chunk, one workgroup | 10 on 3: 2 chunks < 3 |
#   23 on 3: 3 == 3 (8 8 7) | 27 on 3: 4 = 3 + 1 (11 8 8: workgroup 0 owns the short last chunk) | 85 on 4: 11 chunks
#   (24 24 21 16: the short chunk of 5 makes workgroup 2, not the last, odd) | 165 on 7: 21 chunks (24 x 6, 21) |
#   188 on 7: 24 chunks (32 32 28, 24 x 4)
_SHAPES = [(133, 7), (253, 4), (257, 4), (320, 4), (640, 3), (1409, 3), (1665, 3), (5440, 4), (10513, 7), (4248, 3),
           (5504, 4), (11969, 7)]
_WINDOWS = (0, 3, 4)        # 0 = the production window

_DATA = {}


def _case(n, k):
    """(X bf16 [n, 128], C fp64 [k, 128], fp64 argmax ids, fp64 sums|counts) -- made once, never modified."""
    if (n, k) not in _DATA:
        g = torch.Generator(device="cuda").manual_seed(9100 + n + 131 * k)
        C = torch.round(torch.randn(k, 128, device="cuda", generator=g, dtype=torch.float64) * 8).clamp_(-45, 45)
        lab = torch.randint(0, k, (n,), device="cuda", generator=g)
        noise = torch.randint(-2, 3, (n, 128), device="cuda", generator=g).double()
        X64 = (C[lab] + noise).clamp_(-45, 45)
        X = X64.to(torch.bfloat16)
        assert torch.equal(X.double(), X64) and torch.equal(C.to(torch.bfloat16).double(), C)
        score = X64 @ C.T - 0.5 * (C * C).sum(1)[None, :]
        best = score.max(1, keepdim=True).values
        cols = torch.arange(k, device="cuda")[None, :].expand(n, k)
        want = torch.where(score == best, cols, torch.full_like(cols, k)).min(1).values.int()
        ref = torch.zeros((k, 129), dtype=torch.float64, device="cuda")
        ref[:, :128].index_add_(0, want.long(), X64)
        ref[:, 128].index_add_(0, want.long(), torch.ones(n, dtype=torch.float64, device="cuda"))
        _DATA[(n, k)] = (X, C, want, ref)
    return _DATA[(n, k)]


def _check(n, grid, k, flags, window, monkeypatch):
    from alink_amd.ops import kmeans as K
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v10")
    monkeypatch.setattr(K, "V10_FLAGS", flags)
    monkeypatch.setattr(K, "V10_POOL", 0.0)
    assert K.kernel_version(k) == "v10"
    X, C, want, ref = _case(n, k)
    mode = (flags << 4) | (window << 8)
    for rev in (False, True):
        tag = (n, grid, k, flags, window, rev)
        ids = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        got = K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids, reverse=rev, mode=mode)
        ids2 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        again = K.assign_accumulate_hip(X, C, grid=grid, assign_out=ids2, reverse=rev, mode=mode)
        bare = K.assign_accumulate_hip(X, C, grid=grid, reverse=rev, mode=mode)
        assert int((ids < 0).sum()) == 0, (tag, "rows never written")
        assert float(got[:, 128].sum()) == float(n), (tag, "counts do not sum to N")
        assert torch.equal(ids, want), (tag, "ids differ from the fp64 argmax")
        assert torch.equal(got, ref), (tag, "sums or counts differ from the fp64 oracle")
        assert torch.equal(bare, ref), (tag, "without the id output: sums or counts differ from the fp64 oracle")
        assert torch.equal(ids2, ids) and torch.equal(again.view(torch.int64), got.view(torch.int64)), \
            (tag, "two launches differ")


@pytest.mark.parametrize("window", _WINDOWS)
@pytest.mark.parametrize("flags", (0, 1))
@pytest.mark.parametrize("n,grid", _SHAPES)
def test_v10_sweep_exact(n, grid, flags, window, monkeypatch):
    """flags: 0 = non-temporal X loads (the production launch), 1 = default-policy loads."""
    _check(n, grid, 100, flags, window, monkeypatch)


@pytest.mark.parametrize("n,grid,k", [(4248, 3, 17), (5440, 4, 112)])
def test_v10_sweep_exact_other_k(n, grid, k, monkeypatch):
    """Two and seven blocks of 16 centroids, the window of 3 owned tiles, both directions."""
    _check(n, grid, k, 0, 3, monkeypatch)
