"""The v10 KMeans kernel's pair-pipelined argmax (both tiles of a distance pair in one software pipeline,
lane-independent packed fields with the lane's 4g taken off once) at its seam and sign cases, one workgroup,
n = 128 + o: rows whose best score is negative (the rare_neg recompute), all-zero rows, and exact ties between
duplicated centroids in different blocks and lane groups -- each placed in the pair's first tile only, its second
tile only, and both.

Everything here is exact.  C is integer- or half-integer-valued with |c| <= 45 and X integer-valued with |x| <= 45:
both are exact in bf16, and every product and partial sum of a score x.c - |c|^2/2 is a multiple of 1/8 far below
2^14 in magnitude, so it is exact in fp32 in any order and needs at most the 17 significant bits that the packed
compare keeps.  The kernel's id must therefore equal the fp64 argmax with ties to the LOWEST index on every row, and
the returned sums the fp64 sums of X by those ids bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

_KS = (97, 100, 112)
_OFFS = (-1, 0, 1)
_CASES = ("neg", "zero", "tie16", "tie4", "tie95")
_PLACES = ("A", "B", "AB")
_DUP = {"zero": (7, 23), "tie16": (37, 53), "tie4": (41, 45), "tie95": (95, 96)}

_DATA = {}


def _case(case, k, n):
    """(X bf16 [n, 128], C fp64 [k, 128], special-row template [128, 128]) -- generated once, never modified."""
    key = (case, k, n)
    if key not in _DATA:
        g = torch.Generator(device="cuda").manual_seed(9000 + 31 * k + _CASES.index(case))
        C = torch.round(torch.randn(k, 128, device="cuda", generator=g, dtype=torch.float64) * 8).clamp_(-45, 45)
        lab = torch.randint(0, k, (n,), device="cuda", generator=g)
        X = C[lab].clone()                       # a row equal to its centroid: best score +|c|^2/2 > 0
        if case == "neg":
            # small rows against large-norm centroids: every score is negative
            S = torch.randint(-1, 2, (128, 128), device="cuda", generator=g).double()
        else:
            lo, hi = _DUP[case]
            C[lo] = torch.round(C[lo]) * 0.5     # the smallest norm by far: the best centroid of the special rows
            C[hi] = C[lo]                        # ... and an exact duplicate at a higher index
            if case == "zero":
                S = torch.zeros((128, 128), device="cuda", dtype=torch.float64)          # score -|c|^2/2: tie < 0
            else:
                S = torch.empty((128, 128), device="cuda", dtype=torch.float64)
                S[0::2] = torch.round(2 * C[lo])            # x.c - |c|^2/2 = 3|c|^2/2 > 0: a tie of positive scores
                S[1::2] = torch.sign(C[lo])                 # sum|c| - |c|^2/2 < 0: a tie of negative scores
        _DATA[key] = (X, C, S)
    return _DATA[key]


def _rows(place, n):
    r = torch.arange(n, device="cuda")
    tile = r // 64
    inside = (tile == 0) if place == "A" else (tile == 1) if place == "B" else (tile <= 1)
    return inside & (r % 3 != 0)                 # special and ordinary rows mixed inside every wave's 16 rows


def _exact(X, ids, k):
    a = ids.long()
    ref = torch.zeros((k, 129), dtype=torch.float64, device=X.device)
    ref[:, :128].index_add_(0, a, X.double())
    ref[:, 128].index_add_(0, a, torch.ones(X.shape[0], dtype=torch.float64, device=X.device))
    return ref


@pytest.mark.parametrize("place", _PLACES)
@pytest.mark.parametrize("case", _CASES)
@pytest.mark.parametrize("o", _OFFS)
@pytest.mark.parametrize("k", _KS)
def test_v10_pairmax_seam_and_sign(k, o, case, place, monkeypatch):
    from alink_amd.ops import kmeans as K
    n = 128 + o
    X0, C, S = _case(case, k, n)
    sel = _rows(place, n)
    X64 = torch.where(sel[:, None], S[torch.arange(n, device="cuda") % 128], X0)
    X = X64.to(torch.bfloat16)
    assert torch.equal(X.double(), X64) and torch.equal(C.to(torch.bfloat16).double(), C)
    # fp64 argmax, ties to the lowest index
    score = X64 @ C.T - 0.5 * (C * C).sum(1)[None, :]
    best = score.max(1, keepdim=True).values
    cols = torch.arange(k, device="cuda")[None, :].expand(n, k)
    want = torch.where(score == best, cols, torch.full_like(cols, k)).min(1).values.int()
    if case == "neg":
        assert bool((best[sel] < 0).all())
    else:
        lo, hi = _DUP[case]
        assert bool((want[sel] == lo).all()) and bool((score[sel, lo] == score[sel, hi]).all())
        if case == "zero":
            assert bool((best[sel] < 0).all())
        else:
            assert bool((best[sel] < 0).any()) and bool((best[sel] > 0).any())
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v7")
    ids7 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    K.assign_accumulate_hip(X, C, grid=1, assign_out=ids7)
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v10")
    assert K.kernel_version(k) == "v10"
    for rev in (False, True):
        ids = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        got = K.assign_accumulate_hip(X, C, grid=1, assign_out=ids, reverse=rev)
        bare = K.assign_accumulate_hip(X, C, grid=1, reverse=rev)
        assert torch.equal(ids, ids7), (k, n, case, place, rev, "v10 ids differ from v7")
        assert torch.equal(ids, want), \
            (k, n, case, place, rev, "ids differ from the fp64 argmax (lowest index at ties)")
        assert torch.equal(got, _exact(X, ids, k)), (k, n, case, place, rev, "sums differ from the fp64 sums")
        assert torch.equal(bare, got), (k, n, case, place, rev, "result depends on assign_out")
