"""The HIP nearest-centroid kernels held to the exact fp64 oracle of ``tests/kmeans_oracle.py`` on the inputs the
blob tests never produce: bit-exact ties of both signs, winners next to the padded slots, scores far from O(1)
and one cluster summed in fp32 by a single workgroup.  Every tolerance is the oracle's (derived in its module
docstring); ``tests/test_kmeans_oracle.py`` validates the oracle itself on the CPU paths.

Tie rule, every path: a bit-equal best score goes to the LOWEST index, whatever its sign.  The fused kernels pack
an index field into the low mantissa bits and take a float max; a fixed field gets one sign wrong (a larger
mantissa is the larger number only when positive) -- ``kmeans_v10.hip`` ``pack`` describes what they do instead.

Non-finite rows are not run here: docs/kmeans_numerics.md says why."""
import pytest
import torch

import kmeans_oracle as KO

pytestmark = pytest.mark.gpu

PAD_K = (1, 15, 16, 17, 111, 112, 113, 127, 128)
PAD_N = (1, 63, 64, 65, 127, 128, 129, 257)


@pytest.fixture(params=["v7", "v10"])
def kernel(request, monkeypatch):
    """Both fused kernels (v10 serves k <= 112; above that the call runs v7 either way)."""
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", request.param)
    return request.param


def _fused(X, C, k, grid=None, reverse=False):
    from alink_amd.ops import kmeans as K
    asg = torch.full((X.shape[0],), -1, dtype=torch.int32, device=X.device)
    got = K.assign_accumulate_hip(X, C, grid=grid, assign_out=asg, reverse=reverse)
    torch.cuda.synchronize()
    return asg, got


def _check_fused(family, args, what, grid=None, reverse=False):
    Xc, Cc = getattr(KO, family + "_family")(*args)
    o = KO.cached_oracle(family, *args)
    k = Cc.shape[0]
    asg, got = _fused(Xc.cuda(), Cc.cuda(), k, grid, reverse)
    KO.check_assignment(o, asg, k, what)
    KO.check_sums(Xc, asg, got, k, what)
    return asg


TIES = [(20,), (100,), (100, True), (20, True)]


@pytest.mark.parametrize("args", TIES + [(128,)], ids=str)
def test_fused_kernels_give_exact_ties_to_the_lowest_index(args, kernel):
    """v7 and v10 (default grid and one workgroup, forward and serpentine-reversed): duplicated centroids at
    (0, k-1), inside a 16-block, across a 16-block boundary and a triple; best scores positive (rows 2c), negative
    (rows c/4, -c), and +-0 (zero rows on a centroid pair at the origin: packed, a denormal bit pattern);
    -0.0 in rows and centroids."""
    a = _check_fused("tie", args, f"{kernel} ties {args}")
    for grid, rev in ((1, False), (None, True), (2, True)):
        b = _check_fused("tie", args, f"{kernel} ties {args} grid={grid} reverse={rev}", grid, rev)
        assert torch.equal(a, b)


@pytest.mark.parametrize("args", TIES, ids=str)
def test_v10_work_stealing_tail_gives_exact_ties_to_the_lowest_index(args, monkeypatch):
    from alink_amd.ops import kmeans as K
    monkeypatch.setenv("ALINK_KMEANS_KERNEL", "v10")
    monkeypatch.setattr(K, "V10_POOL", 0.5)
    _check_fused("tie", args, f"v10 pool ties {args}")
    _check_fused("tie", args, f"v10 pool ties {args} (second launch: the other counter)")


def _csr(Xd):
    from alink_amd.models.common.features import FeatureMatrix
    nz = Xd != 0
    crow = torch.zeros(Xd.shape[0] + 1, dtype=torch.int64)
    crow[1:] = nz.sum(1).cumsum(0)
    r, c = nz.nonzero(as_tuple=True)
    return FeatureMatrix(crow=crow.cuda(), col=c.cuda(), val=Xd[r, c].cuda(), ncols=Xd.shape[1])


@pytest.mark.parametrize("args", TIES + [(128,)], ids=str)
def test_two_pass_paths_give_exact_ties_to_the_lowest_index(args, monkeypatch):
    """The paths that never packed (nearest_hip, the default counts mode, assign_f32, the general path, the sparse
    nearest kernel on the same rows as CSR) and the packed counts mode, whose field used to favour the higher
    index on a negative tie."""
    from alink_amd.ops import kmeans as K
    from alink_amd.ops import kmeans_sparse as KS
    Xc, Cc = KO.tie_family(*args)
    o = KO.cached_oracle("tie", *args)
    k = Cc.shape[0]
    X, C = Xc.cuda(), Cc.cuda()
    want_counts = torch.bincount(o.expected, minlength=k)     # every row of a tie family is decided or a tie
    assert bool(o.pinned.all())
    idx, _ = K.nearest_hip(X, C)
    KO.check_assignment(o, idx, k, "nearest_hip")
    for flag in ("0", "1"):
        monkeypatch.setenv("ALINK_KMEANS_COUNTS_PACKED", flag)
        for rg in (1, 2, 3):
            monkeypatch.setattr(K, "NEAREST_RG", rg)
            cnt = K.nearest_counts_hip(X, C)
            assert torch.equal(cnt.cpu(), want_counts), f"nearest_counts_hip packed={flag} rg={rg}"
    KO.check_assignment(o, K.assign_f32(X.float(), C), k, "assign_f32")
    buf = K.assign_accumulate_general_hip(X, C.to(torch.bfloat16))
    torch.cuda.synchronize()
    KO.check_sums(Xc, o.expected, buf, k, "general path")
    sidx, _ = KS.nearest(_csr(Xc.double()), C, "EUCLIDEAN")
    KO.check_assignment(o, sidx, k, "sparse nearest")


@pytest.mark.parametrize("k", PAD_K)
def test_padding_and_block_edges(k, kernel):
    """k at and around the 16-centroid block edges with the winner at index k-1, rows whose every real score is
    about -8e6 (a -3e38 pad slot must never win), row counts around the 64-row tile, one workgroup and the default
    grid: indices in [0, k), counts summing to n, the oracle's sets and sums."""
    for n in PAD_N:
        for grid in (None, 1):
            a = _check_fused("padding", (k, n), f"{kernel} padding k={k} n={n} grid={grid}", grid)
            kind = torch.arange(n) % 3
            assert bool((a.cpu()[kind != 2] == k - 1).all())


@pytest.mark.parametrize("family,args", [("blob", (1500, 37, 0)), ("blob", (1500, 37, 10)), ("blob", (1500, 37, -20)),
                                         ("blob", (1500, 37, -70)), ("offset", (1500, 37))], ids=str)
def test_magnitudes_away_from_one(family, args, kernel):
    """Scores of about 1e9, 1e-9 and 1e-39 (under the smallest fp32 normal: the oracle's absolute floor accepts
    every centroid there, so range, counts and sums are what is checked), and un-centred blobs whose scores cancel
    to 1 part in 4000: membership on all rows, equality on decided rows."""
    _check_fused(family, args, f"{kernel} {family} {args}")
    _check_fused(family, args, f"{kernel} {family} {args} grid=1", 1)
    if family == "blob":
        from alink_amd.ops import kmeans as K
        Xc, Cc = KO.blob_family(*args)
        idx, _ = K.nearest_hip(Xc.cuda(), Cc.cuda())
        KO.check_assignment(KO.cached_oracle(family, *args), idx, Cc.shape[0], f"nearest_hip {args}")


@pytest.mark.parametrize("grid", [1, None])
def test_one_cluster_takes_everything(grid, kernel):
    """70 001 rows of magnitude 2^8, all of one cluster: with one workgroup its four accumulate waves each add
    17 500 rows in fp32.  Sums within m_c 2^-24 sum|x|, nothing added."""
    _check_fused("one_cluster", (70001, 100), f"{kernel} one cluster grid={grid}", grid)
