"""The chi-square kernels (ops/csrc/chisq.hip) against the oracles of tests/chisq_helpers.py, and the four operators
on the device against their own host path in the same process."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import chisq_helpers as H  # noqa: E402

from alink_amd.models.statistics import chisq as CQ  # noqa: E402
from alink_amd.ops import chisq as Q  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------
# counts (exact) and statistic (bounded; bitwise equal across grids) at every shape
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 64, 65, 130])
@pytest.mark.parametrize("d", [1, 3, 130])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_kernels_equal_the_oracles(n, d, L):
    calls = Q.CHISQ_CALLS
    H.check_dense_shape(Q.DEVICE, _dev(), n, d, L, grids=(0, 1, 3))
    assert Q.CHISQ_CALLS >= calls + 8                   # three grids of both kernels, two more count variants


def test_edge_cases_budgets_and_grids():
    """One value in all 4097 rows, 4044 distinct values, a column without entries, one without implicit zeros, stored
    +0.0 / -0.0 / two NaN payloads; one block, a block per column (one of them over the budget alone) and borders
    between columns: the same tables and the same bits."""
    H.check_special(Q.DEVICE, _dev())


def test_long_run_and_distinct_values_with_many_labels():
    """L above one pass of the flush (65 and 1024 labels): a run over many chunks and an all-distinct column."""
    dev = _dev()
    for L in (65, 1024):
        n = 4097
        rng = np.random.default_rng(L)
        X = np.stack([np.ones(n), np.arange(n, dtype=np.float64), rng.integers(0, 3, size=n).astype(np.float64)], 1)
        lab = rng.integers(0, L, size=n).astype(np.int32)
        colptr, bits, slab = Q.dense_stream(torch.from_numpy(X).to(dev), torch.from_numpy(lab).to(dev))
        tables = []
        value, R, Lc = CQ.chi_square_stream(colptr, bits, slab, L, None, Q.DEVICE, tables=tables)
        want = np.concatenate([H.table_oracle(b, l, L)[1] for b, l in H.dense_columns(X, lab)])
        assert np.array_equal(tables[0][2].cpu().numpy(), want)
        H.check_columns(H.dense_columns(X, lab), L, value.cpu().numpy(), R.cpu().numpy(), Lc.cpu().numpy())


def test_value_repeats_bitwise_and_p_is_the_host_function():
    from scipy.stats import chi2
    a = H.run_special(Q.DEVICE, _dev())
    b = H.run_special(Q.DEVICE, _dev())
    assert np.array_equal(a[1].view(np.int64), b[1].view(np.int64))
    R, Lc = a[2].astype(np.int64), a[3].astype(np.int64)
    df = np.where((R > 1) & (Lc > 1), (R - 1) * (Lc - 1), 0).astype(np.float64)
    p = CQ.p_values(a[1], df)
    for j in range(len(df)):
        assert p[j] == (float(chi2.sf(a[1][j], df[j])) if df[j] > 0 else 1.0)
    assert df[0] == 0 and df[2] == 0 and p[0] == 1.0 and p[2] == 1.0


def test_identity_matrix_and_independent_column():
    dev = _dev()
    k, m = 8, 32                                        # the cross table is m times the k x k identity
    lab = np.repeat(np.arange(k, dtype=np.int32), m)
    X = lab.astype(np.float64).reshape(-1, 1)
    colptr, bits, slab = Q.dense_stream(torch.from_numpy(X).to(dev), torch.from_numpy(lab).to(dev))
    tables = []
    value, R, Lc = CQ.chi_square_stream(colptr, bits, slab, k, None, Q.DEVICE, tables=tables)
    assert np.array_equal(tables[0][2].cpu().numpy(), m * np.eye(k, dtype=np.int64))
    df = np.array([(int(R[0]) - 1) * (int(Lc[0]) - 1)], dtype=np.float64)
    assert df[0] == (k - 1) ** 2 and CQ.p_values(value.cpu().numpy(), df)[0] < 1e-10
    H.check_columns(H.dense_columns(X, lab), k, value.cpu().numpy(), R.cpu().numpy(), Lc.cpu().numpy())
    X, lab = H.balanced_column()
    colptr, bits, slab = Q.dense_stream(torch.from_numpy(X).to(dev), torch.from_numpy(lab).to(dev))
    value, R, Lc = CQ.chi_square_stream(colptr, bits, slab, 4, None, Q.DEVICE)
    assert float(value[0]) == 0.0 and int(R[0]) == 7 and int(Lc[0]) == 4


# ---------------------------------------------------------------------------------------------------
# the four operators: ALINK_CHISQ_HIP=1 against their own host path (flag 0) in this process
# ---------------------------------------------------------------------------------------------------
LC = 3          # labels of every operator input; every column sees all of them


def _table_rows(n=500, seed=3):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        y = int(rng.integers(0, LC))
        s = None if i % 23 == 0 else "uvwxé"[(y if rng.random() < 0.25 else int(rng.integers(0, 5)))]
        k = None if i % 31 == 0 else (y + 4 if rng.random() < 0.15 else int(rng.integers(0, 4)))
        x = None if i % 19 == 0 else ([float("nan"), -0.0, 0.0][y] if rng.random() < 0.2
                                      else [float("nan"), -0.0, 0.0, 7.25][int(rng.integers(0, 4))])
        b = None if i % 17 == 0 else bool(rng.random() < 0.4 + 0.07 * y)
        rows.append((s, k, x, b, int(rng.integers(0, 7)), float(int(rng.integers(0, 4))),
                     None if i % 13 == 0 else "label%d" % y))
    return rows


TABLE_SCHEMA = "s string, k long, x double, b boolean, noise long, noise2 double, label string"
TABLE_COLS = ["s", "k", "x", "b", "noise", "noise2"]


def _vector_rows(kind, n=500, d=12, seed=11):
    from alink_amd.common.linalg import DenseVector, SparseVector
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        y = int(rng.integers(0, LC))
        strength = [0.03 * max(j - 3, 0) for j in range(d)]    # four columns of noise, then ever stronger
        vals = [float(y + 1) if rng.random() < strength[j] else float(int(rng.integers(0, 3))) for j in range(d)]
        if kind == "dense":
            v = DenseVector(vals)
        else:
            idx = [j for j in range(d) if vals[j] != 0.0 or rng.random() < 0.05]      # some stored +0.0
            v = SparseVector(d, idx, [vals[j] for j in idx])
        rows.append((None if i % 29 == 0 else v, None if i % 11 == 0 else y))
    return rows


def _run_op(op_cls, rows, schema, flag, monkeypatch, **kw):
    from alink_amd import MemSourceBatchOp, useLocalEnv
    from alink_amd.common.mlenv import resetEnv
    resetEnv()
    monkeypatch.setenv("ALINK_CHISQ_HIP", flag)
    useLocalEnv(1, device="cuda:0")
    op = op_cls()
    for k, v in kw.items():
        getattr(op, "set" + k)(v)
    calls = Q.CHISQ_CALLS
    op.linkFrom(MemSourceBatchOp(rows, schema))
    assert (Q.CHISQ_CALLS > calls) == (flag == "1")
    return op


def _results(op, only=None):
    rows = op.collect()
    out = []
    for j in (range(len(rows)) if only is None else only):
        d = json.loads(rows[j][1])
        out.append((rows[j][0], d["df"], d["value"], d["p"]))
    return out


def _compare(dev_res, host_res, names=None):
    for j, (d, h) in enumerate(zip(dev_res, host_res)):
        assert d[0] == (h[0] if names is None else names[j])
        assert d[1] == h[1], (j, d, h)
        T = (h[1] / (LC - 1) + 1) * LC if h[1] > 0 else 1       # T = R * Lc cells
        assert abs(d[2] - h[2]) <= 2 * T * 2.0 ** -52 * h[2], (j, d, h)


def test_table_operator_equals_its_host_path(monkeypatch):
    from alink_amd import ChiSquareTestBatchOp
    kw = dict(SelectedCols=TABLE_COLS, LabelCol="label")
    dev = _run_op(ChiSquareTestBatchOp, _table_rows(), TABLE_SCHEMA, "1", monkeypatch, **kw)
    host = _run_op(ChiSquareTestBatchOp, _table_rows(), TABLE_SCHEMA, "0", monkeypatch, **kw)
    assert dev.getOutputTable().schema.names == host.getOutputTable().schema.names
    assert set(json.loads(dev.collect()[0][1])) == set(json.loads(host.collect()[0][1]))
    _compare(_results(dev), _results(host))
    assert all(r[1] > 0 for r in _results(host))


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_vector_operator_equals_its_host_path(kind, monkeypatch):
    from alink_amd import VectorChiSquareTestBatchOp
    kw = dict(SelectedCol="vec", LabelCol="label")
    schema = "vec %s_vector, label long" % kind
    dev = _run_op(VectorChiSquareTestBatchOp, _vector_rows(kind), schema, "1", monkeypatch, **kw)
    host = _run_op(VectorChiSquareTestBatchOp, _vector_rows(kind), schema, "0", monkeypatch, **kw)
    _compare(_results(dev), _results(host))
    assert all(r[1] > 0 for r in _results(host))


def test_sparse_vectors_of_hashed_size_equal_the_host_path_on_a_slice(monkeypatch):
    """Vectors of size 2^18 on the device; the host path runs on 64 of the columns re-indexed to size 64."""
    from alink_amd import VectorChiSquareTestBatchOp
    from alink_amd.common.linalg import SparseVector
    d, n = 2 ** 18, 300
    rng = np.random.default_rng(7)
    hot = np.unique(np.concatenate([[0, d - 1], rng.integers(0, d, size=80)]))[:64]
    hot[-1] = d - 1
    hot = np.unique(hot)
    assert len(hot) == 64
    wide, narrow = [], []
    for i in range(n):
        y = int(rng.integers(0, LC))
        pick = np.unique(rng.integers(0, 64, size=12))
        vals = [float(y + 1) if rng.random() < 0.3 else float(int(rng.integers(0, 3))) for _ in pick]
        label = None if i % 11 == 0 else y
        wide.append((SparseVector(d, [int(hot[q]) for q in pick], vals), label))
        narrow.append((SparseVector(64, [int(q) for q in pick], vals), label))
    kw = dict(SelectedCol="vec", LabelCol="label")
    schema = "vec sparse_vector, label long"
    dev = _run_op(VectorChiSquareTestBatchOp, wide, schema, "1", monkeypatch, **kw)
    host = _run_op(VectorChiSquareTestBatchOp, narrow, schema, "0", monkeypatch, **kw)
    assert dev.getOutputTable().num_rows == d
    _compare(_results(dev, only=[int(c) for c in hot]), _results(host), names=[str(int(c)) for c in hot])
    cold = [int(c) for c in (1, 2, d // 2) if c not in set(hot.tolist())]
    assert all(r[1] == 0 and r[2] == 0 and r[3] == 1.0 for r in _results(dev, only=cold))


SELECTORS = [dict(SelectorType="NumTopFeatures", NumTopFeatures=3), dict(SelectorType="percentile", Percentile=0.5),
             dict(SelectorType="fpr", Fpr=0.05), dict(SelectorType="fdr", Fdr=0.05), dict(SelectorType="fwe", Fwe=0.05)]


def _cuts_are_clear(pvals, kw):
    """Neighbouring p-values at every cut differ by more than 1e-6 relative (on the host path's values): no two
    p-values that close anywhere in the order, and none that close to a threshold the selector compares with."""
    p = np.sort(np.asarray(pvals, dtype=np.float64))
    n = len(p)
    assert np.all(np.diff(p) > 1e-6 * p[1:]), p
    marks = []
    if "Fpr" in kw:
        marks = [kw["Fpr"]]
    if "Fwe" in kw:
        marks = [kw["Fwe"] / n]
    if "Fdr" in kw:
        marks = [kw["Fdr"] * (k + 1) / n for k in range(n)]
    for m in marks:
        assert np.all(np.abs(p - m) > 1e-6 * m), (p, m)


@pytest.mark.parametrize("kw", SELECTORS, ids=[s["SelectorType"] for s in SELECTORS])
@pytest.mark.parametrize("kind", ["table", "dense", "sparse"])
def test_selectors_choose_what_their_host_path_chooses(kind, kw, monkeypatch):
    from alink_amd import (ChiSqSelectorBatchOp, ChiSquareTestBatchOp, VectorChiSqSelectorBatchOp,
                           VectorChiSquareTestBatchOp)
    if kind == "table":
        rows, schema, sel_cls, test_cls = _table_rows(), TABLE_SCHEMA, ChiSqSelectorBatchOp, ChiSquareTestBatchOp
        base = dict(SelectedCols=TABLE_COLS, LabelCol="label")
    else:
        rows, schema = _vector_rows(kind), "vec %s_vector, label long" % kind
        sel_cls, test_cls = VectorChiSqSelectorBatchOp, VectorChiSquareTestBatchOp
        base = dict(SelectedCol="vec", LabelCol="label")
    host_test = _run_op(test_cls, rows, schema, "0", monkeypatch, **base)
    _cuts_are_clear([r[3] for r in _results(host_test)], kw)
    dev = _run_op(sel_cls, rows, schema, "1", monkeypatch, **base, **kw)
    host = _run_op(sel_cls, rows, schema, "0", monkeypatch, **base, **kw)
    assert dev.selectedIndices() == host.selectedIndices()
    assert dev.collect() == host.collect()
    assert 0 < len(host.selectedIndices()) < len(_results(host_test))
