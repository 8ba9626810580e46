"""The tree-training kernels (ops/csrc/tree_hist.hip, the split search of ops/csrc/tree_split.hip) against the exact
oracles of tests/tree_helpers.py at their edges: slot populations around the wave / batch / pair sizes, feature and bin
counts around the 32-feature groups and 8-bin reduce tiles, forced chunk plans, every host-side branch of the
fp32-atomic launcher, the LDS / global switch of the node sums, and split searches over all 64 lanes with ties."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tree_helpers as T  # noqa: E402

from alink_amd.ops import tree as tops  # noqa: E402

pytestmark = pytest.mark.gpu


def _cu(x):
    return torch.as_tensor(x).cuda()


def _fm(bins, slot, stats, nslots, B, **kw):
    return tops.histogram(_cu(bins), _cu(slot), _cu(stats), nslots, B, variant=2, **kw)


def _stats(rng, n, S):
    """fp32 normal statistics; S == "3p": three columns, the last a unit count (the packed build)."""
    st = rng.normal(size=(n, 3 if S == "3p" else S)).astype(np.float32)
    if S == "3p":
        st[:, 2] = 1.0
    return st


def _fm_fits(B, S):
    return B * (2 if S == "3p" else S) * 256 <= 160 * 1024


def _check_fm(bins, slot, stats, nslots, B, S, monkeypatch, **kw):
    """Bitwise equality with the integer oracle; packed build: exact counts, and equal to the unpacked build where
    that fits the fixed-point kernel too."""
    assert _fm_fits(B, S) and tops.fm_eligible(_cu(bins), stats.shape[1], B, 2, pack=S == "3p")
    ref = torch.from_numpy(T.hist_fm_oracle(bins, slot, stats, nslots, B))
    monkeypatch.setattr(tops, "FM_PACK", True)
    got = _fm(bins, slot, stats, nslots, B, **kw).cpu()
    assert got.shape == ref.shape and torch.equal(got, ref)
    if S == "3p":
        assert tops.FmStats(_cu(stats)).pack
        ok = (slot >= 0) & (slot < nslots)
        cnt = np.zeros(ref.shape[:3], dtype=np.int64)
        for f in range(bins.shape[1]):
            np.add.at(cnt[:, f], (slot[ok], bins[ok, f]), 1)
        assert torch.equal(got[..., 2].long(), torch.from_numpy(cnt))
        if _fm_fits(B, 3):
            monkeypatch.setattr(tops, "FM_PACK", False)
            plain = tops.FmStats(_cu(stats))
            assert not plain.pack
            assert torch.equal(_fm(bins, slot, stats, nslots, B, prep=plain, **kw).cpu(), got)
    return got


# ---------------------------------------------------------------------------------------------------
# 1. fixed-point histogram (variant 2): bitwise equal to the integer oracle
# ---------------------------------------------------------------------------------------------------
POPS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 255, 256, 257, 600]


@pytest.mark.parametrize("S", ["3p", 4])
@pytest.mark.parametrize("nslots", [1, 5])
@pytest.mark.parametrize("p", POPS)
def test_fm_slot_populations(p, nslots, S, monkeypatch):
    """One chunk per slot, p rows over 16 waves: the tail loop alone (p <= 255: at most 16 rows per wave, the last
    wave short, an odd last pair for odd p), exactly one 16-row batch per wave (256), batch plus tail (257, 600);
    an empty slot in the middle, rows of slots -1, nslots and nslots + 3 left out."""
    rng = np.random.default_rng(100 * p + nslots)
    pops = [p] if nslots == 1 else [p, 3, 0, 17, p]
    slot = T.slots_with_populations(rng, pops, [-1, nslots, nslots + 3])
    n, F, B = slot.size, 33, 9
    plan, slot_chunk = tops.fm_plan(pops, 2, tops.FM_PACK_MAX_ROWS - 1 if S == "3p" else None)
    assert (plan[:, 1] - plan[:, 0]).tolist() == [c for c in pops if c]
    assert np.diff(slot_chunk).tolist() == [int(c > 0) for c in pops]
    bins = rng.integers(0, B, size=(n, F)).astype(np.uint8)
    _check_fm(bins, slot, _stats(rng, n, S), nslots, B, S, monkeypatch)


# B = 256 with 3 or 4 int64 statistics per bin is past the kernel's LDS (the packed S = 3 build fits)
@pytest.mark.parametrize("F,B,S", [(F, B, S) for F in (1, 31, 32, 33, 128, 129, 257) for B in (1, 2, 8, 9, 256)
                                   for S in (1, 2, 3, "3p", 4) if _fm_fits(B, S)])
def test_fm_feature_groups_bins_and_stats(F, B, S, monkeypatch):
    """nfg = 1, 1, 1, 2, 4, 5, 9 feature groups (the quad / pos block mapping, blocks that exit early, lanes past F in
    the last group), B around the 8-bin reduce tiles, every statistic count."""
    rng = np.random.default_rng(F * 1000 + B)
    n, nslots = 600, 3
    bins = rng.integers(0, B, size=(n, F)).astype(np.uint8)
    slot = rng.integers(-1, nslots + 1, size=n).astype(np.int32)
    _check_fm(bins, slot, _stats(rng, n, S), nslots, B, S, monkeypatch)


@pytest.mark.parametrize("S", ["3p", 4])
@pytest.mark.parametrize("min_rows,identity", [(1, True), (1, False), (600, True), (600, False)])
def test_fm_many_chunks_per_slot(min_rows, identity, S, monkeypatch):
    """Forced chunk plans at n = 3000: ~8-row chunks (a row pair or none per wave), and ~600-row chunks (two 16-row
    batches plus a tail per wave); identity row order (one slot, every row active) and the sorted order."""
    monkeypatch.setattr(tops, "FM_MIN_ROWS", min_rows)
    rng = np.random.default_rng(min_rows + identity)
    F, B = 129, 8
    nfg = (F + 31) // 32
    if identity:
        nslots, pops = 1, [3000]
        slot = np.zeros(3000, dtype=np.int32)
    else:
        nslots, pops = 3, [1200, 0, 1701]
        slot = T.slots_with_populations(rng, pops, [-1, 3, 6], n_extra=33)
    n = slot.size
    plan, slot_chunk = tops.fm_plan(pops, nfg, tops.FM_PACK_MAX_ROWS - 1 if S == "3p" else None)
    lens = plan[:, 1] - plan[:, 0]
    if min_rows == 1:
        assert lens.max() <= 8 and lens.min() >= 4 and plan.shape[0] >= sum(pops) // 8
    elif identity:
        assert lens.tolist() == [600] * 5
    else:
        assert lens.tolist() == [600, 600, 567, 567, 567] and slot_chunk.tolist() == [0, 2, 2, 5]
    bins = rng.integers(0, B, size=(n, F)).astype(np.uint8)
    _check_fm(bins, slot, _stats(rng, n, S), nslots, B, S, monkeypatch)


@pytest.mark.parametrize("S", [3, "3p", 2])
def test_fm_histogram_groups_padding_repeats_and_order(S, monkeypatch):
    """Feature-major build of a group list with a padding group, a repeated group and groups out of order."""
    monkeypatch.setattr(tops, "FM_PACK", True)
    rng = np.random.default_rng(11)
    n, F, B, nslots = 1500, 100, 9, 4
    bins = rng.integers(0, B, size=(n, F)).astype(np.uint8)
    slot = rng.integers(-1, nslots + 2, size=n).astype(np.int32)
    slot[slot == 2] = -1                                      # an empty slot
    stats = _stats(rng, n, S)
    groups = [2, tops.PAD_GROUP, 0, 2, 3, 1]
    got = tops.histogram_groups(_cu(bins), _cu(slot), _cu(stats), nslots, B, groups).cpu()
    ref = T.hist_fm_oracle(bins, slot, stats, nslots, B).transpose(1, 0, 2, 3)          # [F, nslots, B, S]
    assert got.shape == (len(groups) * 32, nslots, B, ref.shape[3])
    for i, g in enumerate(groups):
        exp = np.zeros((32,) + ref.shape[1:], dtype=np.float32)
        if g != tops.PAD_GROUP:
            part = ref[g * 32:(g + 1) * 32]
            exp[:part.shape[0]] = part
        assert torch.equal(got[i * 32:(i + 1) * 32], torch.from_numpy(exp)), (i, g)
    assert not bool(got[32:64].any()) and not bool(got[4 * 32 + 4:5 * 32].any())       # padding: exactly zero


@pytest.mark.parametrize("S", ["3p", 4])
@pytest.mark.parametrize("min_rows", [8192, 100])
def test_fm_row_order_segments_in_place(min_rows, S, monkeypatch):
    """RowOrder at kernel level: build nodes a subset of the level's nodes, out of order, with skipped segments
    between them (chunk starts with gaps); a second level regrouped from the first."""
    monkeypatch.setattr(tops, "FM_PACK", True)
    monkeypatch.setattr(tops, "FM_MIN_ROWS", min_rows)
    rng = np.random.default_rng(21)
    n, F, B = 3000, 40, 9
    bins = rng.integers(0, B, size=(n, F)).astype(np.uint8)
    stats = _stats(rng, n, S)
    active = rng.random(n) < 0.7
    node = rng.integers(-1, 8, size=n).astype(np.int32)          # 6 level nodes; -1, 6 and 7 are out
    node[node == 2] = 3                                           # node 2 has no rows
    prep = tops.FmStats(_cu(stats))
    assert prep.pack == (S == "3p")
    tro = tops.RowOrder(prep, _cu(active))

    def check_level(node_l, nn, inside, slot_nodes, tag):
        tro.regroup(_cu(node_l), nn, tag)
        order = tro.order.cpu().numpy()
        assert tro.seg.shape == (nn + 1,) and tro.seg[0] == 0 and tro.seg[nn] == order.size
        for k in range(nn):
            # ascending row ids inside every segment
            assert np.array_equal(order[tro.seg[k]:tro.seg[k + 1]], np.flatnonzero(inside & (node_l == k)))
        assert torch.equal(tro.q.cpu(), prep.q.cpu()[torch.from_numpy(order).long()])
        counts = [int(tro.seg[k + 1] - tro.seg[k]) for k in slot_nodes]
        plan, _ = tops.fm_plan(counts, (F + 31) // 32, tops.FM_PACK_MAX_ROWS - 1 if prep.pack else None,
                               [int(tro.seg[k]) for k in slot_nodes])
        assert plan[0, 0] == tro.seg[slot_nodes[0]] and plan[0, 0] > 0          # the first chunk skips rows
        assert plan.shape[0] == len(slot_nodes) if min_rows == 8192 else plan.shape[0] > len(slot_nodes)
        slot = np.full(n, -1, dtype=np.int32)
        for s, k in enumerate(slot_nodes):
            slot[inside & (node_l == k)] = s
        got = tops.histogram(_cu(bins), _cu(np.full(n, -1, dtype=np.int32)), _cu(stats), len(slot_nodes), B, variant=2,
                             prep=prep, tro=tro, slot_nodes=slot_nodes).cpu()
        assert torch.equal(got, torch.from_numpy(T.hist_fm_oracle(bins, slot, stats, len(slot_nodes), B)))

    inside = active & (node >= 0) & (node < 6)
    check_level(node, 6, inside, [4, 1], 1)
    node2 = np.where(inside, 2 * node + rng.integers(0, 2, size=n), -1).astype(np.int32)
    node2[rng.random(n) < 0.1] = -7                               # finished rows leave the order
    check_level(node2, 12, inside & (node2 >= 0), [7, 0, 11], 2)


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("n", [65535, 65536])
def test_fm_packed_worst_case_carry_margin(n, sign, monkeypatch):
    """kPackBits against FM_PACK_MAX_ROWS: 65535 rows of one bin in ONE chunk, statistic 0 the same power of two
    (the largest quantised value the scales give, |q0| = 2^29) and of one sign in every row: count and sum exact;
    65536 rows: two chunks."""
    monkeypatch.setattr(tops, "FM_PACK", True)
    monkeypatch.setattr(tops, "FM_MIN_ROWS", 1 << 20)
    plan, _ = tops.fm_plan([n], 1, tops.FM_PACK_MAX_ROWS - 1)
    assert (plan[:, 1] - plan[:, 0]).tolist() == ([65535] if n == 65535 else [32768, 32768])
    B = 2
    bins = np.ones((n, 1), dtype=np.uint8)
    slot = np.zeros(n, dtype=np.int32)
    stats = np.empty((n, 3), dtype=np.float32)
    stats[:, 0] = sign * 2.0
    stats[:, 1] = 0.5
    stats[:, 2] = 1.0
    prep = tops.FmStats(_cu(stats))
    assert prep.pack and int(prep.q[0, 0]) == int(sign) * 2 ** 29
    got = _check_fm(bins, slot, stats, 1, B, "3p", monkeypatch)
    assert float(got[0, 0, 1, 2]) == n
    assert float(got[0, 0, 1, 0]) == n * float(stats[0, 0])
    assert not bool(got[0, 0, 0].any())


@pytest.mark.parametrize("S", ["3p", 4])
def test_fm_deterministic_and_row_order_independent(S, monkeypatch):
    monkeypatch.setattr(tops, "FM_PACK", True)
    monkeypatch.setattr(tops, "FM_MIN_ROWS", 64)
    rng = np.random.default_rng(31)
    n, F, B, nslots = 4000, 33, 9, 5
    bins = rng.integers(0, B, size=(n, F)).astype(np.uint8)
    slot = rng.integers(-1, nslots + 1, size=n).astype(np.int32)
    stats = _stats(rng, n, S)
    a = _fm(bins, slot, stats, nslots, B)
    b = _fm(bins, slot, stats, nslots, B)
    p = rng.permutation(n)
    c = _fm(bins[p], slot[p], stats[p], nslots, B)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))          # bit patterns, signed zeros included


# ---------------------------------------------------------------------------------------------------
# 2. fp32-atomic kernels (variants 0 and 1, tree_hist_global): exact on integer-valued statistics
# ---------------------------------------------------------------------------------------------------
# name: (F, B, S, nslots, one-hot statistics, expected plan of alink_tree_hist_f32) with unit = (B*S+1)*8 bytes and
# max_units = 65536 // unit.  S = 1 and S > 4 run tree_hist_lds under both variants; S in 2..4 run tree_hist_rows<S>
# under variant 0.
F32_CASES = {
    # unit 224, max_units 292 >= 5: one group, FG = 292 // 5 = 58 -> 48 (< F, 16-aligned); F % 16 != 0: byte loads
    "one_group_FG_lt_F_bytes": (70, 9, 3, 5, False, dict(kernel="lds", max_units=292, FG=48, spg=5, groups=1)),
    # unit 152, max_units 431: FG = 431 // 6 = 71 -> 64 < F = 80; F % 16 == 0, f0 in {0, 64}: uint4 bin loads, rows<2>
    "one_group_uint4_S2": (80, 9, 2, 6, False, dict(kernel="lds", max_units=431, FG=64, spg=6, groups=1)),
    # unit 296, max_units 221: FG = 44 -> 32 < F = 64; uint4 bin loads, rows<4>
    "one_group_uint4_S4": (64, 9, 4, 5, True, dict(kernel="lds", max_units=221, FG=32, spg=5, groups=1)),
    # unit 144, max_units 455: FG = min(151, F) = 7 = F: one feature group, run-time-S loop with S = 1
    "one_group_all_features_S1": (7, 17, 1, 3, True, dict(kernel="lds", max_units=455, FG=7, spg=3, groups=1)),
    # unit 1328, max_units 49: FG = 12 (< 16: not rounded) < F = 20
    "one_group_S5": (20, 33, 5, 4, True, dict(kernel="lds", max_units=49, FG=12, spg=4, groups=1)),
    # unit 12296, max_units 5 >= 3: FG = 1, five feature groups
    "one_group_FG1_S6": (5, 256, 6, 3, False, dict(kernel="lds", max_units=5, FG=1, spg=3, groups=1)),
    # unit 8200, max_units 7 < 10: spg 7, 2 groups covering 14 > 10 slots
    "two_groups_S4": (4, 256, 4, 10, False, dict(kernel="lds", max_units=7, FG=1, spg=7, groups=2)),
    # unit 6152, max_units 10 < 12: spg 10, 2 groups covering 20 > 12 slots; rows<3>
    "two_groups_S3": (3, 256, 3, 12, True, dict(kernel="lds", max_units=10, FG=1, spg=10, groups=2)),
    # unit 16392, max_units 3 < 7: spg 3, 3 groups covering 9 > 7 slots
    "three_groups_S8": (3, 256, 8, 7, True, dict(kernel="lds", max_units=3, FG=1, spg=3, groups=3)),
    # unit 22536, max_units 2 < 5: spg 2, 3 groups covering 6 > 5 slots
    "three_groups_S11": (2, 256, 11, 5, True, dict(kernel="lds", max_units=2, FG=1, spg=2, groups=3)),
    # max_units 2, nslots 15: 8 groups covering 16 > 15 slots: the last plan that stays in LDS
    "eight_groups_S11": (2, 256, 11, 15, False, dict(kernel="lds", max_units=2, FG=1, spg=2, groups=8)),
    # max_units 2, nslots 17: 9 groups > 8 -> tree_hist_global
    "global_nine_groups_S11": (2, 256, 11, 17, True, dict(kernel="global", max_units=2, FG=1, spg=2, groups=9)),
    # unit 65544 > 64 KiB: max_units 0 -> tree_hist_global (one (slot, feature) row does not fit LDS)
    "global_no_unit_fits_S32": (2, 256, 32, 2, False, dict(kernel="global", max_units=0, FG=1, spg=1, groups=2)),
}
F32_ROWS = [1, 2047, 2048, 2049, 5000]      # rows per block >= 2048: 1, 1, 1, 2 and 3 blocks in x


@functools.lru_cache(maxsize=None)
def _f32_case(name, n):
    F, B, S, nslots, onehot, plan = F32_CASES[name]
    assert T.hist_f32_branch(F, B, S, nslots) == plan
    rng = np.random.default_rng([n, F, B, S, nslots])
    bins = rng.integers(0, B, size=(n, F)).astype(np.uint8)
    bins[n // 2:, 0] = B - 1                                      # the last bin is hit for sure
    slot = rng.integers(-1, nslots, size=n).astype(np.int32)
    if nslots > 2:
        slot[slot == 1] = -1                                      # an empty slot
    out = rng.random(n) < 0.2
    # slots past the end, those the last group's LDS range covers among them: skipped rows
    hi = max(plan["groups"] * plan["spg"], nslots + 4)
    slot[out] = rng.integers(nslots, hi, size=int(out.sum()))
    if n == 1:
        slot[0] = nslots - 1
    stats = T.int_stats(rng, n, S, onehot)
    ref = tops.histogram_torch(torch.as_tensor(bins), torch.as_tensor(slot), torch.as_tensor(stats).double(), nslots, B)
    assert float(ref.abs().max()) < 2 ** 24
    return bins, slot, stats, ref


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n", F32_ROWS)
@pytest.mark.parametrize("name", list(F32_CASES))
def test_f32_atomic_histograms_exact_on_integers(name, n, variant):
    F, B, S, nslots, _, plan = F32_CASES[name]
    bins, slot, stats, ref = _f32_case(name, n)
    assert not tops.fm_eligible(_cu(bins), S, B, variant)
    got = tops.histogram(_cu(bins), _cu(slot), _cu(stats), nslots, B, variant=variant).cpu()
    assert got.dtype == torch.float32 and torch.equal(got.double(), ref)


# ---------------------------------------------------------------------------------------------------
# 3. node sums
# ---------------------------------------------------------------------------------------------------
def _node_case(rng, n, nnodes, S, ints):
    node = rng.integers(-1, nnodes, size=n).astype(np.int32)
    if nnodes > 2:
        node[node == nnodes // 2] = 0                             # a node without rows
    out = rng.random(n) < 0.1
    node[out] = rng.choice([nnodes, nnodes + 5], size=int(out.sum()))
    sample = rng.random(n) >= 1 / 3
    stats = T.int_stats(rng, n, S, False) if ints else rng.normal(size=(n, S)).astype(np.float32)
    return torch.as_tensor(node), torch.as_tensor(sample), torch.as_tensor(stats)


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 20000])
@pytest.mark.parametrize("nnodes,S", [(1, 1), (7, 3), (2048, 4), (2049, 4), (300, 11)])
def test_node_sums_exact_on_integers(nnodes, S, n):
    """tree_node_sums up to nnodes * S * 8 == 64 KiB of LDS ((2048, 4) exactly), tree_node_sums_global past it
    ((2049, 4)); 4096 rows per block: 1, 1, 1, 2 and 5 blocks."""
    node, sample, stats = _node_case(np.random.default_rng([n, nnodes, S]), n, nnodes, S, True)
    ref = tops.node_sums_torch(node, sample, stats, nnodes)
    got = tops.node_sums(node.cuda(), sample.cuda(), stats.cuda(), nnodes).cpu()
    assert got.dtype == torch.float64 and got.shape == (nnodes, S) and torch.equal(got, ref)
    if n == 20000 and nnodes > 2:
        assert not bool(ref[nnodes // 2].any()) and bool(ref.any())


def test_node_sums_lds_launch_at_exactly_64_kib():
    """(2048, 4) asks for 65536 bytes of dynamic LDS: the launch itself must succeed and reach the last node."""
    n, nnodes, S = 5000, 2048, 4
    node = torch.full((n,), nnodes - 1, dtype=torch.int32)
    node[::2] = 0
    stats = torch.ones((n, S))
    got = tops.node_sums(node.cuda(), torch.ones(n, dtype=torch.bool).cuda(), stats.cuda(), nnodes).cpu()
    assert got[0].tolist() == [2500.0] * S and got[nnodes - 1].tolist() == [2500.0] * S and float(got.sum()) == n * S


def test_node_sums_no_nodes():
    node, sample, stats = _node_case(np.random.default_rng(0), 100, 4, 3, True)
    got = tops.node_sums(node.cuda(), sample.cuda(), stats.cuda(), 0)
    assert got.shape == (0, 3) and got.dtype == torch.float64


@pytest.mark.parametrize("nnodes,S", [(7, 3), (2049, 4)])
def test_node_sums_fp32_normals_within_summation_bound(nnodes, S):
    """One case per kernel.  Both sides sum the same fp64 values in some order: per entry
    |got - ref| <= rows_in_node * 2^-53 * sum |x| (recursive fp64 summation, any order)."""
    n = 20000
    node, sample, stats = _node_case(np.random.default_rng(nnodes), n, nnodes, S, False)
    ref = torch.zeros((nnodes, S), dtype=torch.float64)
    keep = sample & (node >= 0) & (node < nnodes)
    ref.index_add_(0, node[keep].long(), stats[keep].double())
    rows = torch.zeros(nnodes, dtype=torch.float64).index_add_(0, node[keep].long(), torch.ones(int(keep.sum()),
                                                                                              dtype=torch.float64))
    mag = torch.zeros((nnodes, S), dtype=torch.float64).index_add_(0, node[keep].long(), stats[keep].double().abs())
    got = tops.node_sums(node.cuda(), sample.cuda(), stats.cuda(), nnodes).cpu()
    assert bool(((got - ref).abs() <= rows[:, None] * 2.0 ** -53 * mag).all())


# ---------------------------------------------------------------------------------------------------
# 4. gather_rows
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["permutation", "subset", "repeats"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70001])
def test_gather_rows_equals_indexing(n, mode):
    rng = np.random.default_rng(n)
    src = max(n, 1) if mode == "permutation" else 2 * n + 3
    q = torch.as_tensor(rng.integers(-2 ** 31, 2 ** 31, size=(src, 4), dtype=np.int64).astype(np.int32))
    order = torch.as_tensor(rng.integers(0, 2 ** 31, size=src, dtype=np.int64).astype(np.int32))
    if mode == "permutation":
        p = rng.permutation(src)[:n]
    elif mode == "subset":
        p = np.sort(rng.choice(src, size=n, replace=False))
    else:
        p = rng.integers(0, 3, size=n)
    p = torch.as_tensor(p, dtype=torch.int64)
    qo, oo = tops.gather_rows(q.cuda(), p.cuda(), order.cuda())
    assert qo.dtype == torch.int32 and torch.equal(qo.cpu(), q[p]) and torch.equal(oo.cpu(), order[p])
    qo, oo = tops.gather_rows(q.cuda(), p.cuda())
    assert oo is None and qo.shape == (n, 4) and torch.equal(qo.cpu(), q[p])


# ---------------------------------------------------------------------------------------------------
# 5. route
# ---------------------------------------------------------------------------------------------------
def _route_both(bins, node, feat, base, tab):
    exp = tops.route_torch(bins, node, feat, base, tab)
    got = tops.route(bins.cuda(), node.cuda().clone(), feat.cuda(), base.cuda(), tab.cuda()).cpu()
    assert got.dtype == torch.int32 and torch.equal(got, exp.to(torch.int32))
    return got


@pytest.mark.parametrize("n", [1, 257])
def test_route_one_feature_one_node(n):
    """F = 1 and nnodes = 1, once a leaf only and once a split only; route offsets up to 255 in the int16 table;
    rows whose node is outside [0, nnodes) keep it."""
    rng = np.random.default_rng(n)
    bins = torch.as_tensor(rng.integers(0, 256, size=(n, 1)).astype(np.uint8))
    bins[0, 0] = 255
    node = torch.as_tensor(rng.choice([0, 0, 0, -1, 1, 6, -9], size=n).astype(np.int32))
    node[0] = 0
    if n > 1:
        bins[1, 0], node[1] = 0, 0
    tab = torch.arange(256, dtype=torch.int16)[None, :].flip(1).contiguous()        # bin b -> offset 255 - b
    split = _route_both(bins, node, torch.tensor([0], dtype=torch.int32), torch.tensor([10], dtype=torch.int32), tab)
    act = node == 0
    assert torch.equal(split[act], 10 + 255 - bins[act, 0].int()) and torch.equal(split[~act], node[~act])
    assert int(split[0]) == 10 and (n == 1 or int(split[1]) == 265)
    leaf = _route_both(bins, node, torch.tensor([-1], dtype=torch.int32), torch.tensor([-5], dtype=torch.int32), tab)
    assert bool((leaf[act] == -5).all()) and torch.equal(leaf[~act], node[~act])


def test_route_mixed_nodes_wide_offsets():
    rng = np.random.default_rng(5)
    n, F = 257, 3
    bins = torch.as_tensor(rng.integers(0, 256, size=(n, F)).astype(np.uint8))
    node = torch.as_tensor(rng.integers(-3, 7, size=n).astype(np.int32))
    feat = torch.tensor([2, -1, 0, 1], dtype=torch.int32)
    base = torch.tensor([0, -7, 300, 1000], dtype=torch.int32)
    tab = torch.as_tensor(rng.integers(0, 256, size=(4, 256)).astype(np.int16))
    got = _route_both(bins, node, feat, base, tab)
    assert torch.equal(got[(node < 0) | (node >= 4)], node[(node < 0) | (node >= 4)])


# ---------------------------------------------------------------------------------------------------
# 6. split search
# ---------------------------------------------------------------------------------------------------
def _check_search(case):
    """The comparisons of test_hip_general_split_search_matches_torch; the position is compared for every node that is
    not a multi-way split, the left set for every accepted one."""
    ref = T.search(case, "cpu")
    g0, f0, j0, mb0, a0, perm = ref
    assert tops.gpu_kernels_ok()
    g1, f1, j1, mb1, a1, perm1 = T.search(case, "cuda")
    assert perm1 is None                                  # the HIP search ran (no bin order back)
    np.testing.assert_allclose(g1.cpu().numpy(), g0.numpy(), rtol=1e-9, atol=1e-12)
    assert f1.cpu().tolist() == f0.tolist() and mb1.cpu().tolist() == mb0.tolist()
    assert a1.cpu().tolist() == a0.tolist()
    compared = T.compared_nodes(case, ref)
    for r in range(case.H.shape[0]):
        if bool(mb0[r]):
            continue
        assert int(j1[r]) == int(j0[r]), r
        if r in compared:
            f = int(f0[r])
            po = tops.split_order_key(case.H[r, f].numpy(), case.kind, case.ncls, case.is_cat[f])
            assert sorted(po[:int(j0[r]) + 1].tolist()) == sorted(perm[r, f, :int(j0[r]) + 1].tolist())
    if T.has_candidates(case):
        assert 2 * len(compared) >= case.H.shape[0]
    else:                                                 # one candidate with an empty right side: nothing to accept
        assert not compared and not bool(a1.any()) and bool(torch.isinf(g1).all())
    return ref


@pytest.mark.parametrize("B", T.SPLIT_B)
@pytest.mark.parametrize("kind,ncls", T.SPLIT_KINDS)
def test_tree_split_all_lanes(kind, ncls, B):
    """B - 1 = 1, 4, 64, 65, 129, 255 and 256 candidates: one lane, one wave exactly, a second and a fourth stride of
    the categorical rank sort, every lane of the scan and the arg-max holding data."""
    case = T.split_case(kind, ncls, B)
    assert case.H.shape[3] in tops.SPLIT_S
    _check_search(case)


@pytest.mark.parametrize("B", T.TIE_B)
@pytest.mark.parametrize("tie", T.TIE_MODES)
@pytest.mark.parametrize("kind,ncls", T.SPLIT_KINDS)
def test_tree_split_ties_first_position_wins(kind, ncls, tie, B):
    """Equal gains at neighbouring positions (inside a lane, and across two lanes) and equal categorical keys: the
    lower position and the stable order by bin, as in the oracle."""
    case = T.split_case(kind, ncls, B, tie)
    ref = _check_search(case)
    assert T.tied_nodes(case, ref)


@pytest.mark.parametrize("tie", T.TIE_MODES)
@pytest.mark.parametrize("B", T.GBDT_B)
def test_gbdt_split_lanes_ties_and_masked_node(B, tie):
    case = T.gbdt_case(B, tie)
    ref = _check_search(case)
    assert T.compared_nodes(case, ref) == [0, 1]
    if B > 2:
        assert T.tied_nodes(case, ref)


@pytest.mark.parametrize("kind,ncls", T.SPLIT_KINDS)
def test_tree_split_empty_histogram(kind, ncls):
    """A node whose histogram is all zero: gain -inf and position 0 for every feature, not accepted.  Three features:
    9 waves, so the last block has three idle waves."""
    case = T.split_case(kind, ncls, 66)
    case.H = case.H[:, :3].contiguous()
    case.H[1] = 0.0
    case.is_cat, case.ok, case.order = case.is_cat[:3], case.ok[:, :3].contiguous(), case.order[:, :3].contiguous()
    g0, f0, j0, mb0, a0, _ = T.search(case, "cpu")
    g1, f1, j1, mb1, a1, _ = T.search(case, "cuda")
    np.testing.assert_allclose(g1.cpu().numpy(), g0.numpy(), rtol=1e-9, atol=1e-12)
    assert a1.cpu().tolist() == a0.tolist() and f1.cpu().tolist() == f0.tolist()
    assert float(g1[1]) == float("-inf") and int(j1[1]) == 0 and not bool(a1[1])
    assert float(g0[1]) == float("-inf") and int(j0[1]) == 0 and not bool(a0[1])
    cfg = case.cfg
    gain, pos = tops.tree_split(case.H.cuda(), kind, torch.tensor(case.is_cat), ncls, cfg.min_samples_per_leaf,
                                cfg.min_sum_hessian_per_leaf, cfg.min_sample_ratio_per_child, cfg.min_info_gain)
    assert bool(torch.isinf(gain[1]).all()) and bool((gain[1] < 0).all()) and pos[1].tolist() == [0, 0, 0]
    assert bool(torch.isfinite(gain[0]).any())


def test_gbdt_split_empty_histogram():
    case = T.gbdt_case(65)
    case.H[0] = 0.0
    g0, f0, j0, _, a0, _ = T.search(case, "cpu")
    g1, f1, j1, _, a1, _ = T.search(case, "cuda")
    np.testing.assert_allclose(g1.cpu().numpy(), g0.numpy(), rtol=1e-9, atol=1e-12)
    assert a1.cpu().tolist() == a0.tolist() == [False, True, False]
    assert float(g1[0]) == float("-inf") and int(j1[0]) == int(j0[0]) == 0 and int(j1[1]) == int(j0[1])
    gain, pos = tops.gbdt_split(case.H.cuda(), case.cfg.min_samples_per_leaf, case.cfg.min_sum_hessian_per_leaf)
    assert bool((gain[0] == float("-inf")).all()) and pos[0].tolist() == [0, 0, 0]
