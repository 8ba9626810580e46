"""The device path of PrefixSpanBatchOp on the CPU: the torch twin of the sequence count kernel against a brute-force
oracle that knows no bitmap, and the level loop of ``ops.prefixspan.mine`` through the twins against the host path
``M.prefix_span``.  Every compared value is an integer (or a string built from equal integers by the same host code):
exact equality throughout."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import spm_helpers as H  # noqa: E402

from alink_amd import MemSourceBatchOp, PrefixSpanBatchOp  # noqa: E402
from alink_amd.common.strings import StringBlock  # noqa: E402
from alink_amd.models.associationrule import mining as M  # noqa: E402
from alink_amd.ops import fpm as F  # noqa: E402
from alink_amd.ops import prefixspan as S  # noqa: E402

WIDTHS = (8, 16, 32, 64)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WIDTHS)
def test_after_and_field_count_twins_equal_per_field_arithmetic(w):
    rng = np.random.default_rng(w)
    x = rng.integers(0, 2 ** 63, size=50, dtype=np.int64) * rng.choice([1, -1], size=50)
    x[:3] = [0, -1, np.iinfo(np.int64).min]
    x[3:10] &= x[10:17] & x[17:24]                              # sparse words: fields that are zero
    after = S.seq_after_twin(_t(x), w).numpy()
    fields = S.seq_fields_twin(_t(x).reshape(-1, 1), w).numpy()
    mask = (1 << w) - 1
    for v, a, c in zip(x.tolist(), after.tolist(), fields.tolist()):
        v, a = v & (2 ** 64 - 1), a & (2 ** 64 - 1)
        want, n = 0, 0
        for k in range(0, 64, w):
            f = (v >> k) & mask
            if f:
                n += 1
                want |= (mask & ~(((f & -f) << 1) - 1)) << k
        assert a == want and c == n


@pytest.mark.parametrize("P", [1, 2, 4, 9])
@pytest.mark.parametrize("w", WIDTHS)
def test_seq_twin_equals_oracle(w, P):
    n_seq, m = 3 * 64 // w + 70, 7                              # several words, a last word with padding fields
    D = H.random_table(w * 10 + P, n_seq, w, m, density=0.6)
    prefix, ptr, ext = H.random_seq_classes(P, m, P, 9, [1, 3, 18, 0, 2])
    got = S.seq_counts_twin(_t(H.packed_fields(D)), n_seq, w, _t(prefix), _t(ptr), _t(ext))
    want = H.seq_oracle(D, prefix, ptr, ext)
    assert want.max() > 0
    assert np.array_equal(got.numpy(), want)


@pytest.mark.parametrize("w", WIDTHS)
def test_twin_at_the_edges_of_a_field(w):
    D, prefix, ptr, ext, want = H.edge_table(w)
    assert np.array_equal(H.seq_oracle(D, prefix, ptr, ext), want)
    got = S.seq_counts_twin(_t(H.packed_fields(D)), 4, w, _t(prefix), _t(ptr), _t(ext))
    assert np.array_equal(got.numpy(), want)


@pytest.mark.parametrize("w", WIDTHS)
def test_twin_on_the_all_ones_table_counts_lengths_and_no_padding(w):
    n_seq = 2 * (w + 1) + 3
    D, lens = H.ones_table(w, n_seq)
    B = _t(H.packed_fields(D))
    assert (n_seq * w) % 128 != 0                               # padding fields, and for w < 64 inside a word
    for k in range(2, 11):
        prefix = np.full((1, k - 1), 1, dtype=np.int32)
        got = S.seq_counts_twin(B, n_seq, w, _t(prefix), _t(np.array([0, 2])), _t(np.array([1, 3], np.int32)))
        assert got.tolist() == [int((lens >= k).sum())] * 2


def test_bitmap_of_the_slot_csr_is_the_field_layout():
    for w in WIDTHS:
        D = H.random_table(w, 37, w, 5)
        crow, item = H.slot_csr(D)
        assert np.array_equal(F.build_bitmap_twin(_t(crow), _t(item), 5).numpy(), H.packed_fields(D))


def test_wrappers_refuse_bad_arguments():
    D = H.random_table(1, 10, 8, 3)
    B = _t(H.packed_fields(D))
    pre, ptr, ext = _t(np.array([[1]], np.int32)), _t(np.array([0, 1], np.int64)), _t(np.array([3], np.int32))
    assert S.seq_counts_twin(B, 10, 8, pre, ptr, ext).shape == (1,)
    bad = [
        (B, 10, 12, pre, ptr, ext),                             # no such field width
        (B, 10, 16, pre, ptr, ext),                             # W does not match n_seq * w
        (B, 10, 8, _t(np.array([[2]], np.int32)), ptr, ext),    # a prefix that starts with an I code
        (B, 10, 8, pre, ptr, _t(np.array([6], np.int32))),      # item 3 of 3
        (B, 10, 8, pre, ptr, _t(np.array([-1], np.int32))),
        (B, 10, 8, pre, _t(np.array([0, 2], np.int64)), ext),   # cls_ptr does not end at the candidates
        (B, 10, 8, pre, _t(np.array([1, 1], np.int64)), ext),   # nor start at 0
        (B, 10, 8, pre.to(torch.int64), ptr, ext),
        (B, 10, 8, pre, ptr.to(torch.int32), ext),
        (B[:, :1], 10, 8, pre, ptr, ext),
        (B.t(), 10, 8, pre, ptr, ext),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            S.seq_counts_twin(*args)
        with pytest.raises(ValueError):
            S.seq_counts(*args)
    with pytest.raises(ValueError):
        S.seq_counts(B, 10, 8, pre, ptr, ext)                   # the kernel wrapper wants GPU tensors
    with pytest.raises(ValueError):
        S.field_width(65)
    assert [S.field_width(k) for k in (0, 8, 9, 16, 17, 33, 64)] == [8, 8, 16, 16, 32, 64, 64]


def test_join_steps_makes_the_candidates_of_the_next_level():
    # siblings under (S0): I1, I2, S0, S2 (codes 2, 4, 1, 5 sorted: 1, 2, 4, 5); a lone pattern under (S1)
    Fq = torch.tensor([[1, 1], [1, 2], [1, 4], [1, 5], [3, 3]], dtype=torch.int32)
    st = S.join_steps(Fq)
    prefix, ptr, ext, owner = S.expand_steps(Fq, st, 0, 5)
    cands = [tuple(prefix[o].tolist()) + (int(e),) for o, e in zip(owner.tolist(), ext.tolist())]
    assert cands == [(1, 1, 1), (1, 1, 4), (1, 1, 5),           # (S0 S0): S0, S2, and S2's item joins: I2
                     (1, 2, 1), (1, 2, 4), (1, 2, 5),           # (S0 I1): S0, S2, I2
                     (1, 4, 1), (1, 4, 5),                      # (S0 I2): S0, S2
                     (1, 5, 1), (1, 5, 5),                      # (S0 S2): S0, S2
                     (3, 3, 3)]
    assert ptr.tolist() == [0, 3, 6, 8, 10, 11] and st.cnt.tolist() == [3, 3, 2, 2, 1]
    a, b = S.expand_steps(Fq, st, 1, 3), S.expand_steps(Fq, st, 3, 5)
    assert torch.equal(torch.cat([a[2], b[2]]), ext[3:])


# ---------------------------------------------------------------------------------------------------
# the level loop through the twins against the host path
# ---------------------------------------------------------------------------------------------------
VOCAB = ["a", "b", "c", "d", "e", "f", "été", "中文"]


def _tables():
    gen = H.gen_rows(5, 90, VOCAB, max_elements=5, max_items=4, zipf=0.7)
    gen += [None, "", "   ", "\t", " \x1c\x1f ", " a ; b,c\t", "a,a,a;a,a", "été;中文", "中文,été;a",
            ";".join(["a", "b"] * 5)]
    # q occurs four times in one sequence and nowhere else: it qualifies at 3 by occurrences, not by sequences
    occ = ["q,q;q;q,a", "a;b", "a;b", "b;a", None]
    return {"doc": ["a;a,b,c;a,c;d;c,f", "a,d;c;b,c;a,e", "e,f;a,b;d,f;c;b", "e;g;a,f;c;b;c"],
            "itemset": ["a,b;c", "a,b;c", "a;b,c"], "gen": gen, "occ": occ}


TABLES = _tables()
_HOST = {}


def _host(name, cnt, pct, max_len):
    """``M.prefix_span`` on the table, computed once per case and shared."""
    key = (name, cnt, pct, max_len)
    if key not in _HOST:
        _HOST[key] = M.prefix_span([H.parse_row(s) for s in TABLES[name]], cnt, pct, max_len)
    return _HOST[key]


def _device(name, cnt, pct, max_len, **kw):
    res = M.prefix_span_device(StringBlock.from_list(TABLES[name]), cnt, pct, max_len, backend=S.TWIN, **kw)
    assert res is not None
    return res


CASES = [("doc", 3, 0.0, 10), ("doc", 2, 0.0, 4), ("itemset", 2, 0.0, 10), ("itemset", 1, 0.0, 10),
         ("gen", 12, 0.0, 10), ("gen", 30, 0.0, 10), ("gen", 8, 0.0, 1), ("gen", 8, 0.0, 2), ("gen", 0, 0.0, 2),
         ("gen", -1, 0.15, 10), ("gen", -1, 0.0, 2), ("occ", 3, 0.0, 10), ("occ", 1, 0.0, 3)]


@pytest.mark.parametrize("name,cnt,pct,max_len", CASES)
def test_level_loop_equals_host_path(name, cnt, pct, max_len):
    names_h, pats_h, n_h = _host(name, cnt, pct, max_len)
    names_d, cols, n_d = _device(name, cnt, pct, max_len)
    assert names_d == names_h and n_d == n_h
    assert S.decode(cols) == pats_h and len(pats_h) > 0
    assert cols[0].dtype == torch.int32 and cols[1].dtype == torch.int64 and cols[2].dtype == torch.int64
    assert cols[1].tolist() == sorted(cols[1].tolist()) and int(cols[1].sum()) == cols[0].numel()


def test_tables_hold_what_the_cases_are_about():
    pats = _host("gen", 12, 0.0, 10)[1]
    assert max(sum(len(e) for e in p) for p in pats) >= 3 and any(len(e) > 1 for p in pats for e in p)
    names, pats, _ = _host("occ", 3, 0.0, 10)
    assert "q" in names and ((names.index("q"),),) not in pats          # qualified, yet no pattern
    assert M._min_support(len(TABLES["gen"]), -1, 0.15) == 15
    assert _host("gen", -1, 0.15, 10)[1] == _host("gen", 15, 0.0, 10)[1]


def test_percent_equals_count():
    a, b = _device("gen", -1, 0.15, 10), _device("gen", 15, 0.0, 10)
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_row_blocks_and_candidate_batches_add_to_the_whole():
    whole = _device("gen", 12, 0.0, 10)
    stats = []
    cut = _device("gen", 12, 0.0, 10, budget=64, stats=stats)       # 64-slot blocks, two candidates per batch
    assert stats[0]["stage"] == "encode" and stats[0]["w"] == 16
    assert stats[1]["row_blocks"] == len(TABLES["gen"]) * 16 // 64 > 1 and stats[1]["candidates"] > 2
    assert stats[1]["w"] == 16 and stats[1]["W"] == F.row_stride(len(TABLES["gen"]) * 16)
    assert [s["level"] for s in stats[1:]] == list(range(2, 2 + len(stats) - 1))
    for x, y in zip(whole[1], cut[1]):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------
# the parse
# ---------------------------------------------------------------------------------------------------
def _parsed(rows, cnt=1):
    return M.prefix_span_device(StringBlock.from_list(rows), cnt, 0.0, 10, backend=S.TWIN)


def test_accepted_rows_equal_the_host_parse():
    rows = [None, "", "  \t ", " a ; b,c\t", "\x1fa,b\x1c;c", "été;中文", "a,été ;中文,b", "x y, z;a", "é", "a, ,c;b"]
    res = _parsed(rows)
    assert res is not None
    names, pats, n = M.prefix_span([H.parse_row(s) for s in rows], 1, 0.0, 10)
    assert res[0] == names and res[2] == n == len(rows) and S.decode(res[1]) == pats
    assert " z" in names and "été" in names and " " in names          # items are not stripped one by one


@pytest.mark.parametrize("row", ["a,,b", "a;;b", ";a", "a;", "\u00a0a", "a\u3000", "a; ;b", ",a", "a,", "a ,;b",
                                 "\u00a0", "a;b\u0085", "a;\u2003b", "\u1680a;b", ";".join(["a"] * 65)])
def test_rows_the_bytes_cannot_decide_take_the_host_path(row):
    assert _parsed(["a;b", row, "b"]) is None
    assert _parsed(["a;b", "b"]) is not None


def test_a_row_of_64_elements_gets_the_widest_field():
    rows = [";".join(["a", "b"] * 32), "a;b"]
    stats = []
    res = M.prefix_span_device(StringBlock.from_list(rows), 2, 0.0, 3, backend=S.TWIN, stats=stats)
    assert stats[0]["w"] == 64 and stats[1]["W"] == 2
    assert S.decode(res[1]) == M.prefix_span([H.parse_row(s) for s in rows], 2, 0.0, 3)[1]


def test_hash_collision_takes_the_host_path(monkeypatch):
    from alink_amd.ops import strings as OS
    monkeypatch.setattr(OS, "unique_ids", lambda block: None)
    assert _parsed(["a;b", "b"]) is None


# ---------------------------------------------------------------------------------------------------
# the operator, the selection rule
# ---------------------------------------------------------------------------------------------------
def _op(rows, **kw):
    op = PrefixSpanBatchOp().setItemsCol("s")
    for k, v in kw.items():
        getattr(op, "set" + k)(v)
    op.linkFrom(MemSourceBatchOp([(s,) for s in rows], "s string"))
    return [tuple(r) for r in op.collect()], [tuple(r) for r in op.getSideOutput(0).collect()]


@pytest.mark.parametrize("name,kw", [("doc", {"MinSupportCount": 3}), ("itemset", {"MinSupportCount": 2}),
                                     ("gen", {"MinSupportCount": 12, "MinConfidence": 0.3}),
                                     ("gen", {"MinSupportPercent": 0.2, "MaxPatternLength": 3})])
def test_operator_through_the_twins_equals_the_host_operator(monkeypatch, name, kw):
    want = _op(TABLES[name], **kw)
    assert len(want[0]) > 0 and len(want[1]) > 0
    seen = []
    real = M.prefix_span_device

    def spy(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]

    monkeypatch.setattr(S, "device_selected", lambda device, n_rows: True)      # a CPU block runs on the twins
    monkeypatch.setattr(M, "prefix_span_device", spy)
    monkeypatch.setattr(M, "prefix_span", None)                                 # the host path is not taken
    assert _op(TABLES[name], **kw) == want
    assert len(seen) == 1 and seen[0] is not None


def test_operator_falls_back_to_the_host_rows_when_declined(monkeypatch):
    rows = ["a;b", "a;;b", "a;b"]
    want = _op(rows, MinSupportCount=2)
    monkeypatch.setattr(S, "device_selected", lambda device, n_rows: True)
    assert _op(rows, MinSupportCount=2) == want and len(want[0]) > 0


def test_small_tables_stay_on_the_host_by_default(monkeypatch):
    monkeypatch.delenv("ALINK_PREFIXSPAN_HIP", raising=False)
    monkeypatch.setattr(S._lib, "kernels_enabled", lambda: True)
    assert S.SPM_MIN_ROWS >= 64 and not S.device_selected("cuda:0", 16)


def test_selection_rule(monkeypatch):
    monkeypatch.delenv("ALINK_PREFIXSPAN_HIP", raising=False)
    assert not S.device_selected("cpu", 10 ** 9)
    monkeypatch.setenv("ALINK_PREFIXSPAN_HIP", "1")
    assert not S.device_selected("cpu", 10 ** 9)                 # a CPU device is never selected
    monkeypatch.setattr(S._lib, "kernels_enabled", lambda: True)
    monkeypatch.setattr(S, "SPM_MIN_ROWS", 100)
    assert S.device_selected("cuda:0", 5)                        # 1 forces the device path at any size
    monkeypatch.setenv("ALINK_PREFIXSPAN_HIP", "0")
    assert not S.device_selected("cuda:0", 10 ** 9)
    monkeypatch.delenv("ALINK_PREFIXSPAN_HIP")
    assert not S.device_selected("cuda:0", 99) and S.device_selected("cuda:0", 100)
    monkeypatch.setattr(S._lib, "kernels_enabled", lambda: False)       # the allowed fall-back: the host path
    assert not S.device_selected("cuda:0", 100)

    def missing():
        raise RuntimeError("alink_amd HIP kernels unavailable")
    monkeypatch.setattr(S._lib, "kernels_enabled", missing)      # no quiet fall-back: a missing library is an error
    with pytest.raises(RuntimeError):
        S.device_selected("cuda:0", 100)


# ---------------------------------------------------------------------------------------------------
# two processes over gloo
# ---------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, tmp_path):
    port = _free_port()
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "spm_dist_helpers.py"), str(r), str(world),
                               str(port), str(tmp_path)], env=env) for r in range(world)]
    for p in procs:
        p.wait(timeout=300)
    outs = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), f"spm_{world}_{r}.json")) as f:
            o = json.load(f)
        assert "error" not in o, o.get("error")
        outs.append(o)
    return outs


def test_two_processes_with_different_fields_equal_one(tmp_path):
    one = _run(1, tmp_path)[0]
    two = _run(2, tmp_path)
    assert len(one["patterns"]) > 20 and max(sum(len(e) for e in p) for p, _ in one["patterns"]) >= 3
    assert [o["w"] for o in two] == [8, 16] and one["w"] == 16
    for o in two:
        assert o["names"] == one["names"] and o["patterns"] == one["patterns"] and o["n"] == one["n"]
        assert len(o["gather_sizes"]) == 1 and max(o["gather_sizes"]) < o["database_size"] // 4
