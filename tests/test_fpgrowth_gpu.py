"""The frequent-itemset kernels (``ops/csrc/fpm.hip`` through ``ops/fpm.py``) and ``FpGrowthBatchOp`` on the GPU.
Bitmaps are compared bit for bit with ``numpy.packbits``, counts with dense integer oracles, the operator with its own
host path.  Every compared value is an integer: exact equality, no tolerance.  Every case is a valid input."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fpm_helpers as H  # noqa: E402

from alink_amd.ops import fpm as F  # noqa: E402

pytestmark = pytest.mark.gpu


def _c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------- bitmap

@pytest.mark.parametrize("n,m", [(1, 1), (63, 3), (64, 5), (65, 5), (4097, 7), (4097, 1)])
@pytest.mark.parametrize("grid", [0, 1, 3])
def test_bitmap_equals_packbits(n, m, grid):
    D = H.random_bits(n * 31 + m, n, m, density=0.4, empty_rows=0.25)          # a quarter of the rows hold nothing
    crow, item = H.csr_of(D)
    calls = F.FPM_CALLS
    B = F.build_bitmap(_c(crow), _c(item), m, grid=grid)
    assert F.FPM_CALLS == calls + (1 if len(item) else 0)
    assert B.dtype == torch.int64 and tuple(B.shape) == (m, H.row_stride(n))
    assert np.array_equal(B.cpu().numpy(), H.packed(D))


def test_bitmap_of_full_rows_leaves_the_padding_zero():
    D = np.ones((4097, 3), dtype=bool)
    B = F.build_bitmap(*map(_c, H.csr_of(D)), 3)
    assert np.array_equal(B.cpu().numpy(), H.packed(D))


# ---------------------------------------------------------------------------------------------------- pairs

@pytest.mark.parametrize("m", [2, 63, 64, 65, 130])
@pytest.mark.parametrize("n,chunk,splits", [(1000, 0, 0), (4097, 16, 1), (4097, 32, 3), (2111, 16, 0)])
def test_pair_counts_equal_the_oracle(m, n, chunk, splits):
    D = H.random_bits(m * 7 + n, n, m, density=0.3)
    calls = F.FPM_CALLS
    C = F.pair_counts(_c(H.packed(D)), chunk=chunk, splits=splits)
    assert F.FPM_CALLS == calls + 1
    assert np.array_equal(F.u32(C).cpu().numpy(), H.pair_oracle(D))


@pytest.mark.parametrize("m,n", [(65, 4097), (130, 1000)])
def test_pair_counts_of_the_all_ones_table_are_n(m, n):
    D = np.ones((n, m), dtype=bool)
    B = F.build_bitmap(*map(_c, H.csr_of(D)), m)
    for chunk, splits in ((32, 0), (16, 2)):
        C = F.u32(F.pair_counts(B, chunk=chunk, splits=splits)).cpu().numpy()
        assert np.array_equal(C, np.triu(np.full((m, m), n, dtype=np.int64), 1))     # a padding bit that counts shows


# ---------------------------------------------------------------------------------------------------- classes

def _class_case(P, n=4097, m=40, n_classes=37, sizes=(1, 3, 20, 0, 35, 2), seed=0):
    D = H.random_bits(seed + P, n, m, density=0.7)
    return (D,) + H.random_classes(seed + P, m, P, n_classes, sizes)


def _zero_half_case(n=40000, m=40, n_classes=12, sizes=(1, 17, 5)):
    """Every second run of 128 words' worth of transactions holds none of the first four items, and every prefix
    holds one of them: its AND is zero in all lanes there."""
    D = H.random_bits(77, n, m, density=0.7)
    D[(np.arange(n) // 8192) % 2 == 1, :4] = False
    prefix = np.array([[c % 4, 4 + c % 7] for c in range(n_classes)], dtype=np.int32)
    ptr = np.zeros(n_classes + 1, dtype=np.int64)
    ext = []
    for c in range(n_classes):
        k = sizes[c % len(sizes)]
        ext.append(np.arange(12, 12 + k, dtype=np.int32))
        ptr[c + 1] = ptr[c] + k
    return D, prefix, ptr, np.concatenate(ext)


@pytest.mark.parametrize("P", [2, 3, 4])           # levels 3 to 5
@pytest.mark.parametrize("chunk,grid", [(0, 0), (128, 2), (256, 5)])
def test_class_counts_equal_the_oracle(P, chunk, grid):
    # classes with 1 extension, with none, and with more than one extension tile (16); more classes than the grid
    D, prefix, ptr, ext = _class_case(P)
    calls = F.FPM_CALLS
    got = F.class_counts(_c(H.packed(D)), _c(prefix), _c(ptr), _c(ext), chunk=chunk, grid=grid)
    assert F.FPM_CALLS == calls + 1
    assert np.array_equal(got.cpu().numpy(), H.class_oracle(D, prefix, ptr, ext))


def test_class_counts_with_all_zero_prefix_chunks():
    D, prefix, ptr, ext = _zero_half_case()
    B = _c(H.packed(D))
    zero = (B[int(prefix[0, 0]), 128:256] == 0).all() and (B[int(prefix[0, 0]), 0:128] != 0).any()
    assert bool(zero)                                                   # whole steps whose prefix AND is zero
    got = F.class_counts(B, _c(prefix), _c(ptr), _c(ext), chunk=128)
    assert np.array_equal(got.cpu().numpy(), H.class_oracle(D, prefix, ptr, ext))


@pytest.mark.parametrize("m,n", [(65, 2111), (130, 4097)])
def test_level_two_through_the_class_kernel_equals_the_pair_kernel(m, n):
    D = H.random_bits(m + n, n, m, density=0.3)
    B = _c(H.packed(D))
    C = F.u32(F.pair_counts(B))
    Fq = torch.arange(m, dtype=torch.int32, device="cuda").reshape(-1, 1)
    prefix, ptr, ext, owner = F.expand_classes(Fq, *F.join_siblings(Fq))
    got = F.class_counts(B, prefix, ptr, ext)
    assert int(ext.numel()) == m * (m - 1) // 2
    assert torch.equal(got, C[prefix[owner, 0].long(), ext.long()])
    assert np.array_equal(got.cpu().numpy(), H.pair_oracle(D)[np.triu_indices(m, 1)])


def test_grids_and_chunks_give_identical_counts():
    D, prefix, ptr, ext = _class_case(3, n=20000, seed=9)
    B, args = _c(H.packed(D)), [_c(prefix), _c(ptr), _c(ext)]
    a = F.class_counts(B, *args, chunk=128, grid=3)
    b = F.class_counts(B, *args, chunk=512, grid=64)
    assert torch.equal(a, b) and torch.equal(a, F.class_counts_twin(B, *args))
    Bm = _c(H.packed(H.random_bits(4, 20000, 70)))
    assert torch.equal(F.pair_counts(Bm, chunk=16, splits=1), F.pair_counts(Bm, chunk=32, splits=5))
    assert torch.equal(F.pair_counts(Bm), F.pair_counts_twin(Bm))


# ---------------------------------------------------------------------------------------------------- operator

def _run(rows, monkeypatch, flag, **kw):
    from alink_amd import FpGrowthBatchOp, MemSourceBatchOp, useLocalEnv
    monkeypatch.setenv("ALINK_FPGROWTH_HIP", flag)
    useLocalEnv(1, device="cuda:0")
    op = FpGrowthBatchOp().setItemsCol("items")
    for k, v in kw.items():
        getattr(op, "set" + k)(v)
    op.linkFrom(MemSourceBatchOp([(s,) for s in rows], "items string"))
    return [tuple(r) for r in op.collect()], [tuple(r) for r in op.getSideOutput(0).collect()]


def test_operator_on_the_device_equals_its_host_path(monkeypatch):
    vocab = ["i%02d" % i for i in range(30)] + ["été", "中文"]
    rows = H.gen_rows(11, 2000, vocab, max_len=8, zipf=0.9) + [None, "", "  ", ",i01"]
    kw = dict(MinSupportCount=12, MinConfidence=0.2)
    calls = F.FPM_CALLS
    want_p, want_r = _run(rows, monkeypatch, "0", **kw)
    assert F.FPM_CALLS == calls
    got_p, got_r = _run(rows, monkeypatch, "1", **kw)
    assert F.FPM_CALLS > calls
    assert max(r[2] for r in want_p) >= 3 and len(want_r) > 0
    assert got_p == want_p
    assert got_r == want_r


def test_operator_on_the_device_gives_the_documented_rows(monkeypatch):
    rows = ["A,B,C,D", "B,C,E", "A,B,C,E", "B,D,E", "A,B,C,D"]
    calls = F.FPM_CALLS
    pats, rules = _run(rows, monkeypatch, "1", MinSupportPercent=0.4, MinConfidence=0.6)
    assert F.FPM_CALLS > calls
    doc = {"E": 3, "B,E": 3, "C,E": 2, "B,C,E": 2, "D": 3, "B,D": 3, "C,D": 2, "B,C,D": 2, "A,D": 2, "B,A,D": 2,
           "C,A,D": 2, "B,C,A,D": 2, "A": 3, "B,A": 3, "C,A": 3, "B,C,A": 3, "C": 4, "B,C": 4, "B": 5}
    assert {r[0]: r[1] for r in pats} == doc and all(r[2] == r[0].count(",") + 1 for r in pats)
    by = {r[0]: r[1:] for r in rules}
    assert len(by) == 27 and by["C,D=>A"][4] == 2 and by["B,C=>A"][1] == 1.25 and by["B,C=>A"][3] == 0.75
