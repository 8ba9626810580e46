"""The oracles of tests/tree_helpers.py, checked on the CPU: the fixed-point histogram oracle against the fp64
reference within its own quantisation step, the host-side plan of the fp32-atomic kernels, and every split-search case
of tests/test_tree_kernels_gpu.py (enough compared nodes, a real tie in every tie case)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tree_helpers as T  # noqa: E402

from alink_amd.ops import tree as tops  # noqa: E402


@pytest.mark.parametrize("n,F,B,S,nslots", [(1000, 3, 9, 4, 3), (1000, 1, 1, 3, 1), (257, 33, 5, 1, 5)])
def test_hist_fm_oracle_within_quantisation_step(n, F, B, S, nslots):
    """Every statistic is rounded to the nearest multiple of inv[k], so a bin's fixed-point sum is within
    rows_in_bin * inv[k] / 2 of the fp64 sum (both taken before the one rounding to fp32 of the result)."""
    rng = np.random.default_rng(n + F)
    bins = rng.integers(0, B, size=(n, F)).astype(np.uint8)
    slot = rng.integers(-1, nslots + 2, size=n).astype(np.int32)
    stats = rng.normal(size=(n, S)).astype(np.float32)
    acc, inv = T.hist_fm_exact(bins, slot, stats, nslots, B)
    ref = tops.histogram_torch(torch.as_tensor(bins), torch.as_tensor(slot), torch.as_tensor(stats).double(), nslots,
                               B).numpy()
    rows = tops.histogram_torch(torch.as_tensor(bins), torch.as_tensor(slot), torch.ones((n, 1), dtype=torch.float64),
                                nslots, B).numpy()
    diff = np.abs(acc.astype(np.float64) * inv - ref)
    assert (diff <= rows * inv / 2).all()
    assert float(rows.sum()) == float(((slot >= 0) & (slot < nslots)).sum()) * F
    got = T.hist_fm_oracle(bins, slot, stats, nslots, B)
    assert got.dtype == np.float32 and np.array_equal(got, (acc.astype(np.float64) * inv).astype(np.float32))


def test_hist_fm_oracle_unit_count_is_exact():
    """A unit count column quantises to a power of two: the oracle's statistic 2 is the exact row count."""
    rng = np.random.default_rng(3)
    n, F, B, nslots = 700, 2, 4, 2
    bins = rng.integers(0, B, size=(n, F)).astype(np.uint8)
    slot = rng.integers(-1, nslots + 1, size=n).astype(np.int32)
    stats = rng.normal(size=(n, 3)).astype(np.float32)
    stats[:, 2] = 1.0
    got = T.hist_fm_oracle(bins, slot, stats, nslots, B)
    cnt = np.zeros((nslots, F, B))
    for r in range(n):
        if 0 <= slot[r] < nslots:
            for f in range(F):
                cnt[slot[r], f, bins[r, f]] += 1
    assert np.array_equal(got[..., 2].astype(np.float64), cnt)


def test_slots_with_populations_counts():
    slot = T.slots_with_populations(np.random.default_rng(0), [5, 0, 17], [-1, 3, 6])
    assert slot.dtype == np.int32 and slot.size == 22 + 21
    assert [int((slot == s).sum()) for s in (0, 1, 2, -1, 3, 6)] == [5, 0, 17, 7, 7, 7]


def test_int_stats_sums_stay_exact_in_fp32():
    rng = np.random.default_rng(0)
    a = T.int_stats(rng, 5000, 5, False)
    assert a.dtype == np.float32 and np.array_equal(a, np.round(a)) and float(np.abs(a).max()) <= 8
    assert float(np.abs(a).sum(0).max()) < 2 ** 24
    b = T.int_stats(rng, 5000, 6, True)
    assert (b[:, :5].sum(1) == 1).all() and (b[:, 5] == 1).all() and set(np.unique(b)) == {0.0, 1.0}
    assert (T.int_stats(rng, 10, 1, True) == 1).all()


@pytest.mark.parametrize("kind,ncls", T.SPLIT_KINDS)
@pytest.mark.parametrize("tie", [None] + T.TIE_MODES)
def test_split_cases_compare_half_their_nodes_and_hold_ties(kind, ncls, tie):
    for B in (T.SPLIT_B if tie is None else T.TIE_B):
        case = T.split_case(kind, ncls, B, tie)
        assert case.H.shape == (3, 4, B, ncls + 1 if ncls else 4)
        ref = T.search(case, "cpu")
        assert ref[5] is not None                        # the torch scan ran
        cmp_ = T.compared_nodes(case, ref)
        if not T.has_candidates(case):
            assert not bool(ref[4].any()) and bool(torch.isinf(ref[0]).all())
            continue
        assert 2 * len(cmp_) >= case.H.shape[0], (B, cmp_)
        if tie is not None:
            assert T.tied_nodes(case, ref), B


@pytest.mark.parametrize("tie", T.TIE_MODES)
@pytest.mark.parametrize("B", T.GBDT_B)
def test_gbdt_cases_compare_half_their_nodes_and_hold_ties(B, tie):
    case = T.gbdt_case(B, tie)
    ref = T.search(case, "cpu")
    assert T.compared_nodes(case, ref) == [0, 1]         # node 2 has no allowed feature
    assert not bool(ref[4][2]) and float(ref[0][2]) == float("-inf")
    if B > 2:
        assert T.tied_nodes(case, ref)


def test_make_ties_layout():
    H = np.arange(1, 1 + 2 * 2 * 10 * 3, dtype=np.float64).reshape(2, 2, 10, 3)
    out = T.make_ties(H, [True, False], "lanes")
    assert np.array_equal(out[:, 0, 1:8:2], out[:, 0, 0:8:2]) and np.array_equal(out[:, 0, 8:], H[:, 0, 8:])
    zero = [b for b in range(10) if not out[:, 1, b].any()]
    assert zero == [1, 3, 4, 5, 7, 8]                     # the missing bin 9 and bins 0, 2, 6 keep their statistics
    pairs = T.make_ties(H, [True, False], "pairs")
    assert [b for b in range(10) if not pairs[:, 1, b].any()] == [1, 3, 5, 7]


def test_hist_f32_branch_arithmetic():
    assert T.hist_f32_branch(70, 9, 3, 5) == dict(kernel="lds", max_units=292, FG=48, spg=5, groups=1)
    assert T.hist_f32_branch(4, 256, 4, 10) == dict(kernel="lds", max_units=7, FG=1, spg=7, groups=2)
    assert T.hist_f32_branch(2, 256, 11, 16)["groups"] == 8 and T.hist_f32_branch(2, 256, 11, 16)["kernel"] == "lds"
    assert T.hist_f32_branch(2, 256, 11, 17) == dict(kernel="global", max_units=2, FG=1, spg=2, groups=9)
    assert T.hist_f32_branch(2, 256, 32, 2)["max_units"] == 0 and T.hist_f32_branch(2, 256, 32, 2)["kernel"] == "global"
