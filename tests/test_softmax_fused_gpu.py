"""The fused softmax passes (ops/csrc/softmax_fused.hip) against a numpy longdouble reference on the host.

Tolerance, per element: the larger of four times the error of the former torch fp64 chain (GEMM, softmax formulas,
tn_matmul) on the same inputs, and the textbook summation bound count * eps * sum |term| of the reference terms: for
G the n terms r_ic x_ij, for a loss sum the n terms w_i loss_i, for an element of R the m terms x_ij W_cj of its logit
(the softmax has slope at most 1 in every logit, so R_ic moves by at most w_i times the largest logit error).
Every case prints its errors before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

from alink_amd.ops import softmax_fused as F

pytestmark = pytest.mark.gpu
L = np.longdouble
EPS = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def _data(n, m, k1, kind=""):
    """Seeded inputs on the device and their longdouble reference; |eta| <~ 10 unless kind is "big" (logits to +-700).
    kind "offset": X starts one double past a 16-byte boundary; "zero_w": every third weight is 0."""
    rng = np.random.default_rng(1000 * n + 10 * m + k1)
    X = rng.normal(size=(n, m))
    W = rng.normal(size=(k1, m)) * (3.0 if kind != "big" else 200.0) / np.sqrt(m)
    D = rng.normal(size=(k1, m)) / np.sqrt(m)
    y = rng.integers(0, k1 + 1, size=n).astype(np.float64)
    y[0] = k1                                   # the pivot class is always among the labels
    w = rng.random(n) + 0.25
    if kind == "zero_w":
        w[::3] = 0.0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Xd = dev(X)
    if kind == "offset":
        Xd = torch.cat([Xd.new_zeros(1), Xd.reshape(-1)])[1:].view(n, m)
        assert Xd.data_ptr() % 16 == 8 and Xd.is_contiguous()
    Xl, yi = X.astype(L), y.astype(int)

    def ref(Wm):        # r [n, k1] and the rows' w loss at the coefficients Wm
        full = np.concatenate([Xl @ Wm.T, np.zeros((n, 1), L)], 1)
        mx = full.max(1)
        lse = mx + np.log(np.exp(full - mx[:, None]).sum(1))
        r = w[:, None] * (np.exp(full[:, :k1] - lse[:, None]) - (yi[:, None] == np.arange(k1)))
        return r, w * (lse - full[np.arange(n), yi])
    r, wloss = ref(W.astype(L))
    return dict(X=Xd, y=dev(y), w=dev(w), W=dev(W), D=dev(D), Xl=Xl, r=r, wloss=wloss, ref=ref, Wn=W, Dn=D, wn=w)


def _check(name, got, old, want, bound):
    got, old = got.detach().cpu().numpy().astype(L), old.detach().cpu().numpy().astype(L)
    err, err_old = np.abs(got - want), np.abs(old - want)
    tol = np.maximum(4 * err_old, bound)
    print(f"{name}: max err fused {float(err.max()):.3e} former {float(err_old.max()):.3e} "
          f"worst err/tol {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
    assert np.isfinite(got.astype(np.float64)).all() and (err <= tol).all(), name


@pytest.mark.parametrize("n,m,k1,kind", [
    (1, 1, 1, ""), (63, 16, 16, ""), (65, 17, 17, ""), (257, 33, 64, ""), (257, 128, 64, ""), (65, 128, 1, ""),
    (63, 1, 64, ""), (257, 17, 16, ""), (257, 33, 17, ""), (257, 16, 17, "offset"), (257, 33, 16, "zero_w")])
def test_fused_grad_matches_reference(n, m, k1, kind, chunk_rows=256):
    d = _data(n, m, k1, kind)
    G, loss = F.fused_grad(d["X"], d["y"], d["w"], d["W"], chunk_rows=chunk_rows)
    G0, loss0 = F.fused_grad_torch(d["X"], d["y"], d["w"], d["W"])
    assert G.shape == (k1, m)
    tag = f"grad n={n} m={m} k1={k1} {kind}"
    _check(tag + " G", G, G0, d["r"].T @ d["Xl"], n * EPS * (np.abs(d["r"]).T @ np.abs(d["Xl"])))
    _check(tag + " loss", loss, loss0, d["wloss"].sum(), n * EPS * np.abs(d["wloss"]).sum())


@pytest.mark.parametrize("n", [513, 641])
def test_fused_grad_merges_nine_and_eleven_chunks(n):
    """chunk_rows = 64: the merge's round of eight loads in flight, without a tail (9 chunks) and with one of two (11)."""
    test_fused_grad_matches_reference(n, 17, 17, "", chunk_rows=64)


@pytest.mark.parametrize("n", [64 * 1024 + 1, 64 * 8192 + 1])
def test_loss_sums_of_many_batches_match_reference(n):
    """nb = 1025 and 8193 batch partials per series: a thread of the batch sums adds a second partial, and a first
    round of eight loads in flight with one partial behind it."""
    d = _data(n, 1, 1)
    X, y, w, W, D = d["X"], d["y"], d["w"], d["W"], d["D"]
    beta, nsteps = 0.37, 3
    want = np.stack([d["ref"](d["Wn"].astype(L) - s * (beta * d["Dn"].astype(L)))[1] for s in range(nsteps)])
    _check(f"sums n={n} search", F.search_losses(X, y, w, W, D, beta, nsteps),
           F.search_losses_torch(X, y, w, W, D, beta, nsteps), want.sum(1), n * EPS * np.abs(want).sum(1))
    _check(f"sums n={n} loss", F.rows(X, y, w, W, ("loss",))["loss"], F.rows_torch(X, y, w, W, ("loss",))["loss"],
           d["wloss"].sum(), n * EPS * np.abs(d["wloss"]).sum())


@pytest.mark.parametrize("n,m,k1,nsteps,kind", [
    (257, 17, 1, 1, ""), (257, 129, 17, 11, ""), (129, 1024, 64, 11, ""), (257, 17, 64, 11, ""),
    (65, 1024, 1, 1, ""), (257, 129, 64, 1, ""), (257, 17, 17, 11, "big")])
def test_search_and_rows_match_reference(n, m, k1, nsteps, kind):
    d = _data(n, m, k1, kind)
    X, y, w, W, D = d["X"], d["y"], d["w"], d["W"], d["D"]
    tag = f"rows n={n} m={m} k1={k1} nsteps={nsteps} {kind}"
    beta = 0.37
    want = np.stack([d["ref"](d["Wn"].astype(L) - s * (beta * d["Dn"].astype(L)))[1] for s in range(nsteps)])
    _check(tag + " search", F.search_losses(X, y, w, W, D, beta, nsteps),
           F.search_losses_torch(X, y, w, W, D, beta, nsteps), want.sum(1), n * EPS * np.abs(want).sum(1))
    got, old = F.rows(X, y, w, W, ("R", "loss")), F.rows_torch(X, y, w, W, ("R", "loss"))
    logit_terms = (np.abs(d["Xl"]) @ np.abs(d["Wn"].astype(L)).T).max(1)
    _check(tag + " R", got["R"], old["R"], d["r"], (m * EPS * d["wn"] * logit_terms)[:, None])
    _check(tag + " loss", got["loss"], old["loss"], d["wloss"].sum(), n * EPS * np.abs(d["wloss"]).sum())
    assert torch.equal(F.rows(X, y, w, W, ("loss",))["loss"], got["loss"])


def test_same_bits_for_every_grid_and_run():
    d = _data(1000, 33, 10)
    args = (d["X"], d["y"], d["w"], d["W"])
    G, loss = F.fused_grad(*args, chunk_rows=256)
    S = F.search_losses(*args, d["D"], 0.5, 11)
    for grid in (1, 3, 0, 0):
        G1, loss1 = F.fused_grad(*args, grid=grid, chunk_rows=256)
        assert torch.equal(G, G1) and torch.equal(loss, loss1)
        assert torch.equal(S, F.search_losses(*args, d["D"], 0.5, 11, grid=grid))


def test_operator_takes_fused_path(monkeypatch):
    from alink_amd import useLocalEnv, SoftmaxTrainBatchOp, SoftmaxPredictBatchOp
    from alink_amd.operator.batch.source import MemSourceBatchOp
    rng = np.random.default_rng(1)
    X = rng.normal(size=(600, 3))
    lab = np.argmax(X @ rng.normal(size=(3, 4)) + 0.3 * rng.normal(size=(600, 4)), 1)
    data = [[float(a), float(b), float(c), int(l)] for (a, b, c), l in zip(X, lab)]
    preds, calls = {}, {}
    useLocalEnv(1, device="cuda:0")
    try:
        for flag in ("1", "0"):
            monkeypatch.setenv("ALINK_SOFTMAX_HIP", flag)
            before = F.SOFTMAX_FUSED_CALLS
            src = MemSourceBatchOp(data, "f0 double, f1 double, f2 double, label int")
            model = SoftmaxTrainBatchOp().setFeatureCols(["f0", "f1", "f2"]).setLabelCol("label").setMaxIter(30) \
                .linkFrom(src)
            preds[flag] = [r[-1] for r in SoftmaxPredictBatchOp().setPredictionCol("p").linkFrom(model, src).collect()]
            calls[flag] = F.SOFTMAX_FUSED_CALLS - before
    finally:
        useLocalEnv(1, device="cpu")
    assert calls["1"] > 0 and calls["0"] == 0, calls
    assert preds["1"] == preds["0"]


@pytest.mark.parametrize("n,m,k1,bad", [(8, 4, 65, ""), (8, 1025, 3, ""), (8, 4, 3, "fp32"), (8, 4, 3, "strided")])
def test_rejects_what_the_kernels_do_not_take(n, m, k1, bad):
    X = torch.randn(n, 2 * m if bad == "strided" else m, device="cuda",
                    dtype=torch.float32 if bad == "fp32" else torch.float64)[:, :m]
    y, w = torch.zeros(n, device="cuda", dtype=torch.float64), torch.ones(n, device="cuda", dtype=torch.float64)
    W = torch.zeros(k1, m, device="cuda", dtype=torch.float64)
    assert not F.supported(X, k1)
    for call in (lambda: F.fused_grad(X, y, w, W), lambda: F.search_losses(X, y, w, W, W, 1.0, 3),
                 lambda: F.rows(X, y, w, W, ("R",))):
        with pytest.raises(ValueError):
            call()
