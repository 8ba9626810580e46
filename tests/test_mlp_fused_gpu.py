"""The fused MLP kernels (ops/csrc/mlp_fused.hip) against a numpy.longdouble forward / backward pass of the network,
at the smallest shapes that reach each mechanism, and their wiring into MlpObjFunc and the predict mapper.

Measured on an MI355X (profiles/mlp_fused.txt): the gradient within 1.5e-14 of the reference, 8.1e-13 under saturation
(bound 1e-10); P within 5.9e-15 (bound 1e-12) and its row sums within 7.8e-16 of 1 (bound 1e-14)."""
import json

import numpy as np
import pytest
import torch

from alink_amd.models.classification.mlp import weight_size
from alink_amd.ops import mlp_fused as F
from tests.test_mlp_fused import problem, reference

pytestmark = pytest.mark.gpu

SHAPES = [[1, 2], [17, 3], [F.MLP_FUSED_MAX_IN, F.MLP_FUSED_MAX_CLASSES], [5, 7, 3], [16, 17, 2],
          [33, F.MLP_FUSED_MAX_HIDDEN, 17], [15, 16, 33, 5], [4, 3, 3, 2]]


def check_grad(X, y, w, coef, layers, **kw):
    loss0, grad0, _ = reference(X, y, w, coef, layers)
    assert np.isfinite(grad0).all() and np.isfinite(loss0)
    grad, loss = F.fused_grad(X, y, w, coef, layers, **kw)
    err = np.abs(grad.cpu().numpy() - grad0.astype(np.float64))
    print("grad", layers, X.shape[0], "max abs err", err.max(), "loss rel", abs(float(loss) / float(loss0) - 1))
    assert torch.isfinite(grad).all() and torch.isfinite(loss)
    np.testing.assert_allclose(grad.cpu().numpy(), grad0.astype(np.float64), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(float(loss), float(loss0), rtol=1e-11)


@pytest.mark.parametrize("layers", SHAPES, ids=str)
@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_gradient_and_loss_match_the_reference(n, layers):
    check_grad(*problem(n, layers, n + sum(layers), "cuda"), layers, chunk_rows=64)


@pytest.mark.parametrize("n", [513, 641])
def test_gradient_merges_nine_and_eleven_chunks(n):
    """chunk_rows = 64: the merge's round of eight loads in flight, without a tail (9 chunks) and with one of two (11)."""
    layers = [5, 7, 3]
    check_grad(*problem(n, layers, n + sum(layers), "cuda"), layers, chunk_rows=64)


@pytest.mark.parametrize("layers", [[17, 3], [5, 7, 3]], ids=str)
def test_gradient_on_8_byte_aligned_rows_and_zero_weights(layers):
    X, y, w, coef = problem(131, layers, 3, "cuda")
    X = X[1:]                      # an odd d0: rows that are only 8-byte aligned
    assert X.data_ptr() % 16 == 8 and X.is_contiguous()
    w[::3] = 0.0
    y[::2] = layers[-1] - 1
    check_grad(X, y[1:].contiguous(), w[1:].contiguous(), coef, layers, chunk_rows=64)


def test_gradient_under_saturation():
    layers = [4, 6, 3]
    X, y, w, coef = problem(129, layers, 5, "cuda")
    coef[:24] *= 800.0              # hidden pre-activations past +-800
    coef[30:48] *= 1000.0           # logits more than 700 apart
    z1 = X @ coef[:24].reshape(4, 6) + coef[24:30]
    z2 = torch.sigmoid(z1) @ coef[30:48].reshape(6, 3) + coef[48:]
    assert z1.max() > 800 and z1.min() < -800 and (z2.max(1).values - z2.min(1).values).max() > 700
    check_grad(X, y, w, coef, layers, chunk_rows=64)


@pytest.mark.parametrize("layers", [[17, 3], [15, 16, 33, 5]], ids=str)
def test_same_bits_on_every_grid(layers):
    X, y, w, coef = problem(1000, layers, 7, "cuda")
    dirv = torch.randn_like(coef)
    g0, l0 = F.fused_grad(X, y, w, coef, layers, chunk_rows=64)
    s0 = F.search_losses(X, y, w, coef, dirv, layers, 0.5, 4)
    for grid in (1, 7):
        g1, l1 = F.fused_grad(X, y, w, coef, layers, grid=grid, chunk_rows=64)
        assert torch.equal(g0, g1) and torch.equal(l0, l1)
        assert torch.equal(s0, F.search_losses(X, y, w, coef, dirv, layers, 0.5, 4, grid=grid))


@pytest.mark.parametrize("layers", [[5, 7, 3], [200, 16, 4], [130, 40, 20, 33]], ids=str)
@pytest.mark.parametrize("nsteps", [1, 4, F.MLP_FUSED_MAX_STEPS])
def test_search_losses_match_the_reference(nsteps, layers):
    X, y, w, coef = problem(129, layers, 11, "cuda")
    dirv = torch.randn_like(coef) * 0.1
    got = F.search_losses(X, y, w, coef, dirv, layers, 0.25, nsteps).cpu().numpy()
    want = [float(reference(X, y, w, coef - dirv * (s * 0.25), layers)[0]) for s in range(nsteps)]
    np.testing.assert_allclose(got, want, rtol=1e-11)


@pytest.mark.parametrize("layers", [[17, 2], [5, 7, 17], [15, 16, 33, 5], [200, 64]], ids=str)
def test_rows_probabilities_labels_and_losses(layers):
    n = 129
    X, y, w, coef = problem(n, layers, 13, "cuda")
    _, _, P0 = reference(X, y, w, coef, layers)
    res = F.rows(X, y, w, coef, layers, ("row_loss", "P", "label"))
    P = res["P"].cpu().numpy()
    print("rows", layers, "max abs P err", np.abs(P - P0.astype(np.float64)).max(), "row sum err", np.abs(P.sum(1) - 1).max())
    np.testing.assert_allclose(P, P0.astype(np.float64), rtol=0, atol=1e-12)
    assert np.abs(P.sum(1) - 1).max() <= 1e-14
    assert np.array_equal(res["label"].cpu().numpy(), P.argmax(1))       # numpy's argmax is the first maximum
    np.testing.assert_allclose(res["row_loss"].cpu().numpy(),
                               -np.log(P0[np.arange(n), y.long().cpu().numpy()]).astype(np.float64), rtol=1e-11)


@pytest.mark.parametrize("C,lo,hi", [(2, 0, 1), (17, 3, 16)])
def test_tied_logits_give_the_lower_class(C, lo, hi):
    layers = [5, 7, C]
    X, y, w, coef = problem(129, layers, 17, "cuda")
    Wt, bt = coef[42:42 + 7 * C].view(7, C), coef[42 + 7 * C:]
    Wt[:, hi] = Wt[:, lo]
    bt[lo] = bt[hi] = 50.0          # the tied pair is the maximum of every row
    label = F.rows(X, y, w, coef, layers, ("label",))["label"]
    assert (label == lo).all()


def test_objfunc_and_predict_take_the_fused_kernels(monkeypatch):
    from alink_amd import MultilayerPerceptronPredictBatchOp, MultilayerPerceptronTrainBatchOp, useLocalEnv
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    from alink_amd.models.classification.mlp import MlpObjFunc, MlpcModelDataConverter
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.models.linear.objfunc import LabeledData
    from alink_amd.operator.batch.source import TableSourceBatchOp
    layers = [6, 5, 3]
    X, y, w, coef = problem(300, layers, 19, "cuda")
    dirv = torch.randn_like(coef) * 0.1
    data, obj = LabeledData(FeatureMatrix(dense=X), y, w), MlpObjFunc(layers)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("ALINK_MLP_HIP", flag)
        calls = F.MLP_FUSED_CALLS
        out[flag] = (obj.calc_gradient(data, coef)[0], obj.calc_search_values(data, coef, dirv, 0.5, 3),
                     obj.calc_obj_value(data, coef)[0])
        assert F.MLP_FUSED_CALLS - calls == (3 if flag == "1" else 0)
    torch.testing.assert_close(out["1"][0], out["0"][0], rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(out["1"][1], out["0"][1], rtol=1e-10, atol=1e-10)
    assert abs(out["1"][2] - out["0"][2]) <= 1e-10 * abs(out["0"][2])

    def table(device):
        return MTable(TableSchema(["v", "label"], [Types.DENSE_VECTOR, Types.LONG]),
                      [Column(X.to(device)), Column(y.long().cpu())])
    useLocalEnv(1, device="cpu")
    model = MultilayerPerceptronTrainBatchOp().setVectorCol("v").setLabelCol("label").setLayers(layers).setMaxIter(5) \
        .linkFrom(TableSourceBatchOp(table("cpu")))
    _, wm, labels = MlpcModelDataConverter(Types.LONG).load(model.collect())
    P0 = np.sort(reference(X, y, w, torch.as_tensor(wm), layers)[2], 1)
    assert (P0[:, -1] - P0[:, -2]).min() > 1e-6
    pred = MultilayerPerceptronPredictBatchOp().setVectorCol("v").setPredictionCol("p").setPredictionDetailCol("d")
    want = pred.linkFrom(model, TableSourceBatchOp(table("cpu"))).collect()
    monkeypatch.setenv("ALINK_MLP_HIP", "1")
    calls = F.MLP_FUSED_CALLS
    got = pred.linkFrom(model, TableSourceBatchOp(table("cuda"))).collect()
    assert F.MLP_FUSED_CALLS == calls + 1 and len(got) == 300
    for a, b in zip(got, want):
        assert a[-2] == b[-2]
        da, db = json.loads(a[-1]), json.loads(b[-1])
        assert da.keys() == db.keys() and all(abs(da[k] - db[k]) <= 1e-12 for k in da)
