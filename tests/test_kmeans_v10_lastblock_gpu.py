"""The v10 KMeans kernel's last, partly filled centroid block: k on both sides of every boundary of its live count
L = k mod 16 at 4, 8 and 12, and k = 1, 4, 5 where the last block is the only one.  One workgroup, n around two and
three tiles.  The kernel treats the last block like every other one today; these cases guard that path -- dead slots
that must never win, ties that cross into the last block, the negative-score recompute ending there -- and are the
cases at which a variant that loads a last block of few live centroids transposed (measured, not built:
profiles/kmeans_v10_trim.txt) would switch paths.

Everything here is exact.  C is integer- or half-integer-valued with |c| <= 45 and X integer-valued with |x| <= 45:
both are exact in bf16, and every product and partial sum of a score x.c - |c|^2/2 is a multiple of 1/8 far below
2^14 in magnitude, so it is exact in fp32 in any order and needs at most the 17 significant bits that the packed
compare keeps.  The kernel's id must therefore equal the fp64 argmax with ties to the LOWEST index on every row, and
the returned [k, 129] the fp64 sums of X by those ids bit for bit.

Cases (special rows are two of every three rows of every tile, mixed with rows that sit on a centroid):
  cross  an exact duplicate pair, the higher copy the LAST centroid (in the last block), the lower copy in the block
         before it; rows that tie on it with a positive and with a negative score.  With one block (k <= 16) the
         lower copy is centroid 0; with k = 1 there is nothing to duplicate and the rows are ordinary.
  inside both copies in the last block (its first and last centroid; L = 1 has no second one: ordinary rows).
  neg    rows whose every score is negative (the rare_neg recompute) and whose winner is in the last block.
  zero   all-zero rows: score -|c|^2/2, the winner (smallest norm) in the last block.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

_KS = (1, 4, 5, 17, 20, 21, 97, 100, 101, 104, 105, 112)
_NS = (128, 129, 191, 192, 193)
_CASES = ("cross", "inside", "neg", "zero")

_DATA = {}


def _pair(case, k):
    """(lo, hi) of the duplicate pair, or None where k has no room for it."""
    first = 16 * ((k - 1) // 16)             # first centroid of the last block
    if case == "cross":
        return None if k == 1 else (first - 11 if first else 0, k - 1)
    if case == "inside":
        return None if k - 1 == first else (first, k - 1)
    return None


def _case(case, k):
    """(C fp64 [k, 128], special rows [192, 128] or None, ordinary labels [193]) -- generated once, never modified."""
    key = (case, k)
    if key not in _DATA:
        g = torch.Generator(device="cuda").manual_seed(7100 + 37 * k + _CASES.index(case))
        C = torch.round(torch.randn(k, 128, device="cuda", generator=g, dtype=torch.float64) * 8).clamp_(-45, 45)
        lab = torch.randint(0, k, (max(_NS),), device="cuda", generator=g)
        S = None
        pr = _pair(case, k)
        if pr is not None:
            lo, hi = pr
            C[lo] = torch.round(C[lo]) * 0.5     # the smallest norm by far: the best centroid of the special rows
            C[hi] = C[lo]                        # ... and an exact duplicate in the last block
            S = torch.empty((192, 128), device="cuda", dtype=torch.float64)
            S[0::2] = torch.round(2 * C[lo])     # x.c - |c|^2/2 = 3|c|^2/2 > 0: a tie of positive scores
            S[1::2] = torch.sign(C[lo])          # sum|c| - |c|^2/2 < 0: a tie of negative scores
        elif case in ("neg", "zero"):
            w = k - 1                            # the smallest norm by far, in the last block
            C[w] = torch.round(C[w]) * 0.5
            if case == "zero":
                S = torch.zeros((192, 128), device="cuda", dtype=torch.float64)
            else:
                keep = torch.randint(0, 4, (192, 128), device="cuda", generator=g) > 0
                S = torch.sign(C[w])[None, :] * keep          # sum of most |c_w| - |c_w|^2/2 < 0, far above the rest
        _DATA[key] = (C, S, lab)
    return _DATA[key]


def _exact(X, ids, k):
    a = ids.long()
    ref = torch.zeros((k, 129), dtype=torch.float64, device=X.device)
    ref[:, :128].index_add_(0, a, X.double())
    ref[:, 128].index_add_(0, a, torch.ones(X.shape[0], dtype=torch.float64, device=X.device))
    return ref


@pytest.mark.parametrize("case", _CASES)
@pytest.mark.parametrize("k", _KS)
def test_v10_last_block_exact(k, case, monkeypatch):
    from alink_amd.ops import kmeans as K
    C, S, lab = _case(case, k)
    assert torch.equal(C.to(torch.bfloat16).double(), C)
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v10")
    assert K.kernel_version(k) == "v10"
    first = 16 * ((k - 1) // 16)
    cols = torch.arange(k, device="cuda")[None, :]
    for n in _NS:
        r = torch.arange(n, device="cuda")
        X64 = C[lab[:n]].clone()                 # a row equal to its centroid: best score +|c|^2/2 > 0
        sel = torch.zeros(n, dtype=torch.bool, device="cuda")
        if S is not None:
            sel = r % 3 != 0
            X64 = torch.where(sel[:, None], S[r % 192], X64)
        X = X64.to(torch.bfloat16)
        assert torch.equal(X.double(), X64)
        # fp64 argmax, ties to the lowest index
        score = X64 @ C.T - 0.5 * (C * C).sum(1)[None, :]
        best = score.max(1, keepdim=True).values
        want = torch.where(score == best, cols.expand(n, k), torch.full((n, k), k, device="cuda")).min(1).values.int()
        pr = _pair(case, k)
        if pr is not None:
            lo, hi = pr
            assert bool((want[sel] == lo).all()) and bool((score[sel, lo] == score[sel, hi]).all())
            assert bool((best[sel] < 0).any()) and bool((best[sel] > 0).any())
        elif S is not None:
            assert bool((best[sel] < 0).all()) and bool((want[sel] >= first).all())
        for flags in (0, 1):
            monkeypatch.setattr(K, "V10_FLAGS", flags)
            for rev in (False, True):
                ids = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                got = K.assign_accumulate_hip(X, C, grid=1, assign_out=ids, reverse=rev)
                bare = K.assign_accumulate_hip(X, C, grid=1, reverse=rev)
                where = (k, n, case, flags, rev)
                assert torch.equal(ids, want), (where, "ids differ from the fp64 argmax (lowest index at ties)")
                assert torch.equal(got, _exact(X, ids, k)), (where, "sums differ from the fp64 sums")
                assert torch.equal(bare, got), (where, "result depends on assign_out")


@pytest.mark.parametrize("k", (97, 100))
def test_v10_last_block_matches_v7_on_gaussian_centroids(k, monkeypatch):
    """On Gaussian fp64 centroids (scores that are NOT exact in fp32) the ids equal v7's, at a size that runs the
    steady loop and the last iterations as well as at a small one.  It would also hold a transposed last block to the
    rule that an MFMA row's result does not depend on the row's position in its block."""
    from alink_amd.ops import kmeans as K
    g = torch.Generator(device="cuda").manual_seed(177 + k)
    C = torch.randn(k, 128, device="cuda", generator=g, dtype=torch.float64) * 1.5
    for n in (193, 1217):
        X = torch.randint(-3, 4, (n, 128), device="cuda", generator=g).to(torch.bfloat16)
        monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v7")
        ids7 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        K.assign_accumulate_hip(X, C, grid=1, assign_out=ids7)
        monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v10")
        assert K.kernel_version(k) == "v10"
        assert n < 1217 or bool((ids7 >= 16 * ((k - 1) // 16)).any()), "no row is won by the last block"
        for flags in (0, 1):
            monkeypatch.setattr(K, "V10_FLAGS", flags)
            for rev in (False, True):
                ids = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                got = K.assign_accumulate_hip(X, C, grid=1, assign_out=ids, reverse=rev)
                assert torch.equal(ids, ids7), (k, n, flags, rev, "v10 ids differ from v7")
                assert torch.equal(got, _exact(X, ids, k)), (k, n, flags, rev, "sums differ from the fp64 sums")
