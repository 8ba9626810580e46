"""The sequence count kernel (``alink_fpm_seq_counts`` in ``ops/csrc/fpm.hip`` through ``ops/prefixspan.py``) and
``PrefixSpanBatchOp`` on the GPU.  Counts are compared with a brute-force oracle that knows no bitmap
(``spm_helpers.support``), the operator with its own host path.  Every compared value is an integer or a string built
from integers: exact equality, no tolerance.  Every case is a valid input."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import spm_helpers as H  # noqa: E402

from alink_amd.ops import prefixspan as S  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (8, 16, 32, 64)
SHAPES = [(0, 0), (128, 2), (256, 5)]               # (chunk, grid)


def _c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _n_seq(W, w):
    """Sequences that fill ``W`` words but for one padding field."""
    n = W * 64 // w - 1
    assert H.row_stride(n * w) == W
    return n


_CASES = {}


def _case(w, W, P):
    """Table, classes and oracle counts, computed once per shape and shared (never written to)."""
    key = (w, W, P)
    if key not in _CASES:
        n_seq, m = _n_seq(W, w), 6
        D = H.random_table(w * 1000 + W + P, n_seq, w, m, density=0.6)
        # more classes than the waves of the small grids; classes with 0, 1 and 35 extensions (three tiles of 16)
        prefix, ptr, ext = H.random_seq_classes(W + P, m, P, 25, [1, 3, 35, 0, 2])
        _CASES[key] = (n_seq, H.packed_fields(D), prefix, ptr, ext, H.seq_oracle(D, prefix, ptr, ext))
    return _CASES[key]


# one partial step, exactly one step, a step plus a tail, two steps plus a tail
@pytest.mark.parametrize("P", [1, 3, 9])
@pytest.mark.parametrize("W", [2, 128, 130, 258])
@pytest.mark.parametrize("w", WIDTHS)
def test_seq_counts_equal_the_oracle(w, W, P):
    n_seq, B, prefix, ptr, ext, want = _case(w, W, P)
    assert want.max() > 0 or W == 2
    B, args = _c(B), [_c(prefix), _c(ptr), _c(ext)]
    for chunk, grid in SHAPES:
        calls = S.SPM_CALLS
        got = S.seq_counts(B, n_seq, w, *args, chunk=chunk, grid=grid)
        assert S.SPM_CALLS == calls + 1
        assert np.array_equal(got.cpu().numpy(), want), (chunk, grid)


@pytest.mark.parametrize("w", WIDTHS)
def test_kernel_at_the_edges_of_a_field(w):
    D, prefix, ptr, ext, want = H.edge_table(w)
    got = S.seq_counts(_c(H.packed_fields(D)), 4, w, _c(prefix), _c(ptr), _c(ext))
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("w", WIDTHS)
def test_kernel_on_the_all_ones_table_counts_lengths_and_no_padding(w):
    n_seq = 130 * 64 // w - 3                                   # a step plus a tail, padding fields at the end
    D, lens = H.ones_table(w, n_seq)
    B = _c(H.packed_fields(D))
    ptr, ext = _c(np.array([0, 2], np.int64)), _c(np.array([1, 3], np.int32))
    for k in range(2, 11):
        prefix = _c(np.full((1, k - 1), 1, dtype=np.int32))
        for chunk, grid in ((0, 0), (128, 1)):
            got = S.seq_counts(B, n_seq, w, prefix, ptr, ext, chunk=chunk, grid=grid)
            assert got.tolist() == [int((lens >= k).sum())] * 2


@pytest.mark.parametrize("w", WIDTHS)
def test_grids_and_chunks_give_the_counts_of_the_twin(w):
    n_seq = 20000 * 8 // w
    D = H.random_table(w + 9, n_seq, w, 8, density=0.5)
    prefix, ptr, ext = H.random_seq_classes(w, 8, 3, 30, [1, 17, 5, 0, 35])
    B, args = _c(H.packed_fields(D)), [_c(prefix), _c(ptr), _c(ext)]
    a = S.seq_counts(B, n_seq, w, *args, chunk=128, grid=3)
    b = S.seq_counts(B, n_seq, w, *args, chunk=512, grid=64)
    assert int(a.sum()) > 0 and torch.equal(a, b)
    assert torch.equal(a, S.seq_counts_twin(B, n_seq, w, *args))


# ---------------------------------------------------------------------------------------------------- operator

def _run(rows, monkeypatch, flag, **kw):
    from alink_amd import MemSourceBatchOp, PrefixSpanBatchOp, useLocalEnv
    monkeypatch.setenv("ALINK_PREFIXSPAN_HIP", flag)
    useLocalEnv(1, device="cuda:0")
    op = PrefixSpanBatchOp().setItemsCol("s")
    for k, v in kw.items():
        getattr(op, "set" + k)(v)
    op.linkFrom(MemSourceBatchOp([(s,) for s in rows], "s string"))
    return [tuple(r) for r in op.collect()], [tuple(r) for r in op.getSideOutput(0).collect()]


def test_operator_on_the_device_equals_its_host_path(monkeypatch):
    vocab = ["i%02d" % i for i in range(30)] + ["été", "中文"]
    rows = H.gen_rows(11, 2000, vocab, max_elements=5, max_items=3, zipf=0.9) + [None, "", "  "]
    kw = dict(MinSupportCount=40, MinConfidence=0.2)
    calls = S.SPM_CALLS
    want_p, want_r = _run(rows, monkeypatch, "0", **kw)
    assert S.SPM_CALLS == calls
    got_p, got_r = _run(rows, monkeypatch, "1", **kw)
    assert S.SPM_CALLS > calls
    assert max(r[2] for r in want_p) >= 3 and len(want_r) > 0
    assert any("," in r[0] for r in want_p)                     # an I-step pattern
    assert got_p == want_p
    assert got_r == want_r


def test_operator_on_the_device_gives_the_documented_rows(monkeypatch):
    rows = ["a;a,b,c;a,c;d;c,f", "a,d;c;b,c;a,e", "e,f;a,b;d,f;c;b", "e;g;a,f;c;b;c"]
    calls = S.SPM_CALLS
    pats, rules = _run(rows, monkeypatch, "1", MinSupportCount=3)
    assert S.SPM_CALLS > calls
    assert {r[0]: r[1] for r in pats} == {"a": 4, "a;c": 4, "a;c;c": 3, "a;c;b": 3, "a;b": 4, "b": 4, "b;c": 3,
                                          "c": 4, "c;c": 3, "c;b": 3, "d": 3, "d;c": 3, "e": 3, "f": 3}
    assert {r[0]: r[1:] for r in rules} == {
        "a=>c": (2, 1.0, 1.0, 4), "a;c=>c": (3, 0.75, 0.75, 3), "a;c=>b": (3, 0.75, 0.75, 3),
        "a=>b": (2, 1.0, 1.0, 4), "b=>c": (2, 0.75, 0.75, 3), "c=>c": (2, 0.75, 0.75, 3),
        "c=>b": (2, 0.75, 0.75, 3), "d=>c": (2, 0.75, 1.0, 3)}
