"""The CSR softmax passes (ops/csrc/softmax_csr.hip) against a numpy longdouble reference on the host, computed from
the same CSR arrays.

Tolerance, the rule of tests/test_softmax_fused_gpu.py: per element the larger of four times the error of the former
torch chain (fm.mm, softmax formulas, fm.rmm) on the same inputs, and the summation bound count * eps * sum |term|.
For a logit, count is the row's stored entries and the terms are x_ij W_cj; R_ic moves by at most w_i times the
largest logit error (the softmax has slope at most 1), a row's loss lse - eta[y] by at most twice that error.  For
G_cj, count is the column's entries and the terms are x_ij r_ic, and G inherits sum_i |x_ij| (bound of R_i).  A loss
sum has the n terms w_i loss_i.  Every case prints its errors before it asserts.
"""
import functools
import json

import numpy as np
import pytest
import torch

from alink_amd.models.common.features import FeatureMatrix
from alink_amd.ops import softmax_csr as S

pytestmark = pytest.mark.gpu
L = np.longdouble
EPS = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def _data(kind, k1, idx64):
    """Seeded CSR rows on the device and their longdouble reference.  "merge": 1100 rows with a prefixed intercept
    column (3 chunks of 512 in the CSC view) and column 7 left empty.  Otherwise 37 rows of 0, 1, 64, 65 and 129 stored
    entries in turn, one entry moved outside [0, m); "zero_w": every third weight 0; "big": logits to +-700."""
    rng = np.random.default_rng(100 * k1 + len(kind))
    if kind == "merge":
        n, m = 1100, 50
        cols = [np.concatenate([[0], np.sort(rng.choice(np.setdiff1d(np.arange(1, m), [7]), 3, replace=False))])
                for _ in range(n)]
    else:
        n, m = 37, 300
        cols = [np.sort(rng.choice(m, (0, 1, 64, 65, 129)[i % 5], replace=False)) for i in range(n)]
    crow = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    col = np.concatenate(cols).astype(np.int64)
    val = rng.normal(size=col.size)
    if kind == "merge":
        val[crow[:-1]] = 1.0
    else:
        col[crow[3] - 2] = m + 5                # inside a 64-entry row: the entry guard drops it
    ok = (col >= 0) & (col < m)
    X = np.zeros((n, m), L)
    np.add.at(X, (np.repeat(np.arange(n), np.diff(crow))[ok], col[ok]), val[ok].astype(L))
    W = rng.normal(size=(k1, m)) * 0.5
    if kind == "big":
        W *= 700.0 / np.abs(X.astype(np.float64) @ W.T).max()
    D = rng.normal(size=(k1, m)) * 0.3
    y = rng.integers(0, k1 + 1, size=n).astype(np.float64)
    y[0] = k1                                   # the pivot class is always among the labels
    w = rng.random(n) + 0.25
    if kind == "zero_w":
        w[::3] = 0.0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fm = FeatureMatrix(crow=dev(crow), col=dev(col if idx64 else col.astype(np.int32)), val=dev(val), ncols=m)
    yi = y.astype(int)

    def ref(Wm):        # r [n, k1], the rows' losses and the largest sum_j |x_ij W_cj| per row, at the coefficients Wm
        full = np.concatenate([X @ Wm.T, np.zeros((n, 1), L)], 1)
        mx = full.max(1)
        lse = mx + np.log(np.exp(full - mx[:, None]).sum(1))
        r = w[:, None] * (np.exp(full[:, :k1] - lse[:, None]) - (yi[:, None] == np.arange(k1)))
        return r, lse - full[np.arange(n), yi], (np.abs(X) @ np.abs(Wm).T).max(1)
    r, loss, terms = ref(W.astype(L))
    return dict(fm=fm, y=dev(y), w=dev(w), W=dev(W), D=dev(D), X=X, r=r, loss=loss, ref=ref, Wn=W, Dn=D, wn=w,
                eta_bound=np.diff(crow) * EPS * terms, col_count=np.bincount(col[ok], minlength=m))


def _check(name, got, old, want, bound):
    got, old = got.detach().cpu().numpy().astype(L), old.detach().cpu().numpy().astype(L)
    err, err_old = np.abs(got - want), np.abs(old - want)
    tol = np.maximum(4 * err_old, bound)
    print(f"{name}: max err csr {float(np.max(err, initial=0)):.3e} former {float(np.max(err_old, initial=0)):.3e} "
          f"worst err/tol {float(np.max(err / np.maximum(tol, 1e-300), initial=0)):.3f}")
    assert np.isfinite(got.astype(np.float64)).all() and (err <= tol).all(), name


@pytest.mark.parametrize("kind,k1,idx64", [
    ("edges", 1, False), ("edges", 3, True), ("edges", 16, False), ("edges", 17, True), ("edges", 64, False),
    ("merge", 3, False), ("merge", 17, True), ("merge", 64, True), ("zero_w", 3, False), ("big", 17, False)])
def test_grad_and_rows_match_reference(kind, k1, idx64):
    d = _data(kind, k1, idx64)
    fm, y, w, W = d["fm"], d["y"], d["w"], d["W"]
    tag = f"{kind} k1={k1} idx64={idx64}"
    r_bound = (d["wn"] * d["eta_bound"])[:, None]
    wloss = d["wn"] * d["loss"]
    G, loss = S.grad(fm, y, w, W)
    G0, loss0 = S.grad_torch(fm, y, w, W)
    assert G.shape == W.shape
    ax = np.abs(d["X"])
    _check(tag + " G", G, G0, d["r"].T @ d["X"],
           d["col_count"][None, :] * EPS * (np.abs(d["r"]).T @ ax) + (r_bound * np.ones((1, k1))).T @ ax)
    _check(tag + " loss", loss, loss0, wloss.sum(), len(wloss) * EPS * np.abs(wloss).sum())
    got, old = S.rows(fm, y, w, W, ("R", "loss", "row_loss")), S.rows_torch(fm, y, w, W, ("R", "loss", "row_loss"))
    _check(tag + " R", got["R"], old["R"], d["r"], r_bound)
    _check(tag + " row_loss", got["row_loss"], old["row_loss"], d["loss"], 2 * d["eta_bound"])
    assert torch.equal(got["loss"], loss) and torch.equal(S.rows(fm, y, w, W, ("loss",))["loss"], loss)


@pytest.mark.parametrize("kind,k1,idx64,nsteps", [
    ("edges", 3, False, 1), ("edges", 17, True, 11), ("edges", 1, True, 11), ("merge", 64, False, 11),
    ("big", 17, False, 11)])
def test_search_matches_reference(kind, k1, idx64, nsteps):
    d = _data(kind, k1, idx64)
    args, beta = (d["fm"], d["y"], d["w"], d["W"], d["D"]), 0.37
    want = np.stack([d["wn"] * d["ref"](d["Wn"].astype(L) - s * (beta * d["Dn"].astype(L)))[1] for s in range(nsteps)])
    _check(f"search {kind} k1={k1} nsteps={nsteps}", S.search_losses(*args, beta, nsteps),
           S.search_losses_torch(*args, beta, nsteps), want.sum(1), want.shape[1] * EPS * np.abs(want).sum(1))


def test_same_bits_for_every_grid_and_run():
    d = _data("merge", 17, True)
    args = (d["fm"], d["y"], d["w"], d["W"])
    G, loss = S.grad(*args)
    Ss = S.search_losses(*args, d["D"], 0.5, 11)
    for grid in (1, 3, 0, 0):
        G1, loss1 = S.grad(*args, grid=grid)
        assert torch.equal(G, G1) and torch.equal(loss, loss1)
        assert torch.equal(Ss, S.search_losses(*args, d["D"], 0.5, 11, grid=grid))


def operator_rows(n=600, d=30, K=4, seed=3):
    """Sparse-vector rows whose label is a noise-free argmax with a margin of 1 between the two best scores."""
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(d, K)) * 2.0
    rows = []
    while len(rows) < n:
        idx = np.sort(rng.choice(d, 5, replace=False))
        v = rng.normal(size=5)
        sc = np.sort(v @ B[idx])
        if sc[-1] - sc[-2] > 1.0:
            rows.append([f"${d}$" + " ".join(f"{j}:{x!r}" for j, x in zip(idx.tolist(), v.tolist())),
                         int(np.argmax(v @ B[idx]))])
    return rows


def train_and_predict(rows, device):
    """(predictions, top-two probability gaps) of a softmax model trained and applied on ``device``."""
    from alink_amd import useLocalEnv, SoftmaxTrainBatchOp, SoftmaxPredictBatchOp
    from alink_amd.operator.batch.source import MemSourceBatchOp
    useLocalEnv(1, device=device)
    try:
        src = MemSourceBatchOp(rows, "vec string, label int")
        model = SoftmaxTrainBatchOp().setVectorCol("vec").setLabelCol("label").setMaxIter(30).linkFrom(src)
        out = SoftmaxPredictBatchOp().setPredictionCol("p").setPredictionDetailCol("d").linkFrom(model, src).collect()
    finally:
        useLocalEnv(1, device="cpu")
    probs = [sorted(float(v) for v in json.loads(r[-1]).values()) for r in out]
    return [r[-2] for r in out], np.array([p[-1] - p[-2] for p in probs])


def test_operator_takes_csr_path(monkeypatch):
    rows = operator_rows()
    preds, calls = {}, {}
    for flag in ("1", "0"):
        monkeypatch.setenv("ALINK_SOFTMAX_HIP", flag)
        before = S.SOFTMAX_CSR_CALLS
        preds[flag], gap = train_and_predict(rows, "cuda:0")
        calls[flag] = S.SOFTMAX_CSR_CALLS - before
    assert calls["1"] > 0 and calls["0"] == 0, calls
    keep = gap > 1e-6                           # the gaps of the former path (the last run)
    assert keep.mean() >= 0.99
    assert [p for p, k in zip(preds["1"], keep) if k] == [p for p, k in zip(preds["0"], keep) if k]


@pytest.mark.parametrize("bad", ["k1", "fp32", "dense"])
def test_rejects_what_the_kernels_do_not_take(bad):
    d = _data("edges", 3, False)
    fm, y, w = d["fm"], d["y"], d["w"]
    W = torch.zeros(65 if bad == "k1" else 3, fm.ncols, device="cuda", dtype=torch.float64)
    if bad == "fp32":
        fm = FeatureMatrix(crow=fm.crow, col=fm.col, val=fm.val.float(), ncols=fm.ncols)
    if bad == "dense":
        fm = torch.zeros(fm.nrows, fm.ncols, device="cuda", dtype=torch.float64)
    assert not S.supported(fm, W.shape[0])
    for call in (lambda: S.grad(fm, y, w, W), lambda: S.search_losses(fm, y, w, W, W, 1.0, 3),
                 lambda: S.rows(fm, y, w, W, ("R",))):
        with pytest.raises(ValueError):
            call()
