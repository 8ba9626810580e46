"""ops/mlp_fused.py without a GPU: the torch twins against a numpy.longdouble forward / backward pass, the weight images
element by element, and the selection rule at the edges of every constant."""
import numpy as np
import pytest
import torch

from alink_amd.models.classification.mlp import weight_size
from alink_amd.ops import mlp_fused as F


def reference(X, y, w, coef, layers):
    """(sum w loss, gradient in the coef layout, P [n, C]) of the network in numpy.longdouble."""
    X, w, coef = (np.asarray(t.detach().cpu().numpy(), dtype=np.longdouble) for t in (X, w, coef))
    y, rows = y.detach().cpu().numpy().astype(np.int64), np.arange(X.shape[0])
    params, off = [], 0
    for a, b in zip(layers[:-1], layers[1:]):
        params.append((coef[off:off + a * b].reshape(a, b), coef[off + a * b:off + a * b + b]))
        off += a * b + b
    assert off == weight_size(layers)
    hs = [X]
    for W, b in params[:-1]:
        hs.append(1 / (1 + np.exp(-(hs[-1] @ W + b))))
    z = hs[-1] @ params[-1][0] + params[-1][1]
    mx = z.max(1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(1))
    P = np.exp(z - lse[:, None])
    loss = (w * (lse - z[rows, y])).sum()
    D = P.copy()
    D[rows, y] -= 1
    D *= w[:, None]
    grads = [None] * len(params)
    for i in range(len(params) - 1, -1, -1):
        grads[i] = np.concatenate([(hs[i].T @ D).ravel(), D.sum(0)])
        if i:
            D = (D @ params[i][0].T) * hs[i] * (1 - hs[i])
    return loss, np.concatenate(grads), P


def problem(n, layers, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, layers[0], dtype=torch.float64, generator=g)
    y = torch.randint(0, layers[-1], (n,), generator=g).double()
    w = torch.rand(n, dtype=torch.float64, generator=g) + 0.5
    coef = torch.randn(weight_size(layers), dtype=torch.float64, generator=g) * 0.5
    return [t.to(device) for t in (X, y, w, coef)]


@pytest.mark.parametrize("layers", [[17, 3], [5, 7, 3], [15, 16, 33, 5]])
def test_torch_twins_match_the_reference(layers):
    X, y, w, coef = problem(65, layers, 1)
    loss0, grad0, P0 = reference(X, y, w, coef, layers)
    grad, loss = F.fused_grad(X, y, w, coef, layers)
    np.testing.assert_allclose(grad.numpy(), grad0.astype(np.float64), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(float(loss), float(loss0), rtol=1e-11)
    res = F.rows(X, y, w, coef, layers, ("loss", "row_loss", "P", "label"))
    np.testing.assert_allclose(float(res["loss"]), float(loss0), rtol=1e-11)
    np.testing.assert_allclose(res["P"].numpy(), P0.astype(np.float64), rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["row_loss"].numpy(), -np.log(P0[np.arange(65), y.long().numpy()]).astype(np.float64),
                               rtol=1e-11)
    assert np.array_equal(res["label"].numpy(), P0.argmax(1))
    dirv = torch.randn_like(coef)
    got = F.search_losses(X, y, w, coef, dirv, layers, 0.25, 3)
    want = [float(reference(X, y, w, coef - dirv * (s * 0.25), layers)[0]) for s in range(3)]
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-11)


@pytest.mark.parametrize("layers", [[17, 3], [5, 18, 2]])
def test_weight_pack_places_every_element(layers):
    coef = torch.arange(1, weight_size(layers) + 1, dtype=torch.float64)
    ti, th, to = F.tile_counts(layers, True)
    pack = F.weight_pack(coef[None, :], layers, True)[0]
    nl, off, coff = len(layers) - 1, 0, 0
    for l in range(nl):
        a, b = layers[l], layers[l + 1]
        W, bias = coef[coff:coff + a * b].reshape(a, b), coef[coff + a * b:coff + a * b + b]
        coff += a * b + b
        kt, nt = (ti if l == 0 else th), (to if l == nl - 1 else th)
        fwd = pack[off:off + kt * nt * 256].reshape(nt, kt, 4, 16, 4)
        off += kt * nt * 256
        assert torch.equal(pack[off:off + b], bias) and not pack[off + b:off + 16 * nt].any()
        off += 16 * nt
        bwd = pack[off:off + kt * nt * 256].reshape(kt, nt, 4, 16, 4) if l else None
        off += kt * nt * 256 if l else 0
        for i in range(16 * kt):
            for j in range(16 * nt):
                want = float(W[i, j]) if i < a and j < b else 0.0
                assert float(fwd[j // 16, i // 16, (i % 16) // 4, j % 16, i % 4]) == want, (l, i, j)
                if l:
                    assert float(bwd[i // 16, j // 16, (j % 16) // 4, i % 16, j % 4]) == want, (l, i, j)
    assert off == pack.numel()


def test_selected_is_false_on_cpu_and_outside_every_constant():
    X = torch.zeros(8, 4, dtype=torch.float64)
    assert F.shape_ok(X, [4, 3]) and not F.selected(X, [4, 3]) and not F.supported(X, [4, 3])
    wide = lambda d: torch.zeros(1, d, dtype=torch.float64)
    for bad, grad in [([F.MLP_FUSED_MAX_IN + 1, 3], True), ([F.MLP_FUSED_ROWS_MAX_IN + 1, 3], False),
                      ([4, F.MLP_FUSED_MAX_HIDDEN + 1, 3], True), ([4, F.MLP_FUSED_MAX_CLASSES + 1], True),
                      ([4, 1], True), ([4, 3, 3, 3, 3], True), ([128, 64, 64], True), ([64, 64, 8, 33], True)]:
        assert not F.shape_ok(wide(bad[0]), bad, grad), bad
    for good, grad in [([F.MLP_FUSED_MAX_IN, F.MLP_FUSED_MAX_CLASSES], True), ([F.MLP_FUSED_ROWS_MAX_IN, 3], False),
                       ([128, 64, 32], True), ([64, 64, 8, 32], True), ([128, 64, 64], False)]:
        assert F.shape_ok(wide(good[0]), good, grad), good
    assert not F.shape_ok(wide(4).float(), [4, 3]) and not F.shape_ok(wide(5), [4, 3])
