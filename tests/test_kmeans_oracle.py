"""The exact KMeans oracle (``tests/kmeans_oracle.py``) checked without a GPU: the torch paths
(``assign_accumulate_torch``, ``assign``) must pass every check on every input family -- lowest index on bit-exact
ties included -- and the derived slack must leave at least 99 % of the rows of every non-tie family decided, so
that the GPU tests built on it pin the kernels down instead of waving them through.  Every tolerance is the
oracle's (derivation in its module docstring)."""
import pytest
import torch

import kmeans_oracle as KO

PAD_K = (1, 15, 16, 17, 111, 112, 113, 127, 128)
PAD_N = (1, 63, 64, 65, 127, 128, 129, 257)
# (family, args, decided-row cap applies).  The 2^-70 blobs have scores of about 2^-129, under the oracle's absolute
# floor of 2^-126: there every centroid is acceptable by construction and no row can be decided.
FAMILIES = [("tie", (20,), False), ("tie", (100,), False), ("tie", (128,), False), ("tie", (100, True), False),
            ("tie", (20, True), False),
            ("blob", (1500, 37, 0), True), ("blob", (1500, 37, 10), True), ("blob", (1500, 37, -20), True),
            ("blob", (1500, 37, -70), False), ("offset", (1500, 37), True), ("one_cluster", (70001, 100), True)]
FAMILIES += [("padding", (k, 257), True) for k in PAD_K] + [("padding", (17, n), True) for n in PAD_N]


def _torch_paths(X, C):
    from alink_amd.ops import kmeans as K
    idx, d2 = K.assign(X, C)
    buf = K.assign_accumulate_torch(X, C)
    return idx, buf


@pytest.mark.parametrize("family,args,cap", FAMILIES, ids=lambda v: str(v).replace(" ", ""))
def test_torch_paths_pass_the_oracle(family, args, cap):
    X, C = getattr(KO, family + "_family")(*args)
    k = C.shape[0]
    o = KO.cached_oracle(family, *args)
    idx, buf = _torch_paths(X, C)
    KO.check_assignment(o, idx, k, "assign")
    # assign_accumulate_torch takes the same argmax: its counts are the bincount of assign's indices
    KO.check_sums(X, idx, buf, k, "assign_accumulate_torch")
    KO.check_counts(o, buf[:, -1], k, "assign_accumulate_torch")
    if family == "tie":
        assert bool(o.pinned.all()), "every row of a tie family is decided or a bit-exact tie"
        assert int(o.tie.sum()) >= 2 * sum(len(g) for g in KO.dup_groups(k)), "too few tie rows"
        neg = o.tie & (o.s.max(1).values < 0)
        pos = o.tie & (o.s.max(1).values > 0)
        assert int(pos.sum()) >= len(KO.dup_groups(k))
        if len(args) > 1 and args[1]:
            # a centroid pair at the origin scores exactly 0 on every row: no best score is negative, and the
            # zero rows (and every row that nothing else attracts) tie on the pair at +-0
            assert int((o.tie & (o.s.max(1).values == 0)).sum()) >= 4
        else:
            assert int(neg.sum()) >= len(KO.dup_groups(k))
    elif family == "padding":
        kind = torch.arange(X.shape[0]) % 3
        want = kind != 2
        assert bool(o.decided[want].all()) and bool((o.expected[want] == k - 1).all())
    if cap:
        frac = float(o.decided.double().mean())
        assert frac >= 0.99, f"only {frac:.4f} of the rows are decided under the oracle alone"


def test_oracle_accepts_and_rejects_what_it_should():
    """The checks fail when they must: a higher tied index, an index outside the acceptable set, a count moved
    between clusters and a sum off by more than the bound are all caught."""
    X, C = KO.tie_family(20)
    o = KO.cached_oracle("tie", 20)
    k = 20
    good = o.expected.clone()
    KO.check_assignment(o, good, k)
    r = int(o.tie.nonzero()[0])
    other = int((o.s[r] == o.s[r].max()).nonzero()[-1])
    assert other != int(good[r])
    bad = good.clone()
    bad[r] = other                                           # a tied index, but not the lowest
    with pytest.raises(AssertionError, match="decided / tied"):
        KO.check_assignment(o, bad, k)
    bad = good.clone()
    bad[r] = int(o.s[r].argmin())
    with pytest.raises(AssertionError, match="outside the acceptable set"):
        KO.check_assignment(o, bad, k)
    buf = torch.zeros((k, 129), dtype=torch.float64)
    buf[:, :128].index_add_(0, good, X.double())
    buf[:, 128] = torch.bincount(good, minlength=k).double()
    KO.check_sums(X, good, buf, k)
    c = int(good[0])
    off = buf.clone()
    off[c, 3] += 2.0 * float(buf[c, 128]) * KO.U * float(X.double().abs()[good == c, 3].sum()) + 1e-30
    with pytest.raises(AssertionError, match="sums outside"):
        KO.check_sums(X, good, off, k)
    off = buf.clone()
    off[c, 128] -= 1
    off[(c + 1) % k, 128] += 1
    with pytest.raises(AssertionError, match="counts differ"):
        KO.check_sums(X, good, off, k)
    with pytest.raises(AssertionError):
        KO.check_counts(o, off[:, 128], k)


def test_sign_dependent_packing_is_what_the_tie_rows_catch():
    """Why the tie rows exist: a float max over (score & ~127) | index gives a bit-equal pair to the HIGHER index
    when the score is positive and to the lower when it is negative; with 127 - index it is the other way round.
    Emulated here in integer arithmetic on the fp32 bit patterns, the rule the fused kernels now follow -- field
    127 - c for a best score with the sign bit clear, c for one with it set -- returns the lowest index on every
    tie row of the family, and either fixed field fails rows of one sign."""
    X, C = KO.tie_family(100)
    o = KO.cached_oracle("tie", 100)
    s32 = o.s.float()
    assert torch.equal(s32.double(), o.s)                    # the tie family's scores are exact in fp32
    bits = s32.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    cidx = torch.arange(100)[None, :]

    def packed_argmax(field):
        p = (bits & 0xFFFFFF80) | field                      # int64 holding the uint32 pattern
        val = torch.where(p >= 2 ** 31, p - 2 ** 32, p).to(torch.int32).view(torch.float32)
        return val.max(1).values.view(torch.int32).to(torch.int64) & 127

    hi_wins = packed_argmax(cidx.expand_as(bits))                           # field c
    lo_field = 127 - packed_argmax((127 - cidx).expand_as(bits))            # field 127 - c
    best_neg = o.s.max(1).values.view(torch.int64) < 0                      # sign bit of the best score
    rule = torch.where(best_neg, hi_wins, lo_field)      # main pass 127 - c; rows with a negative best redone with c
    t = o.tie
    assert torch.equal(rule[t], o.expected[t])
    pos_t = t & ~best_neg
    neg_t = t & best_neg
    assert bool((hi_wins[pos_t] != o.expected[pos_t]).all()) and torch.equal(hi_wins[neg_t], o.expected[neg_t])
    assert bool((lo_field[neg_t] != o.expected[neg_t]).all()) and torch.equal(lo_field[pos_t], o.expected[pos_t])
