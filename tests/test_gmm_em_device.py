"""The fused GMM EM step's torch twin and its wiring, on the CPU: ``em_step_torch`` against the longdouble oracle
of ``gmm_helpers``, ``train_gmm`` and the mapper forced onto the centred update / the ``posterior`` route, and the
selection rule."""
import numpy as np
import pytest
import torch

import gmm_helpers as H
from alink_amd.models.clustering import gmm as M
from alink_amd.ops import _lib
from alink_amd.ops import gmm as G


@pytest.mark.parametrize("n,k,d", [(65, 2, 3), (200, 17, 16), (200, 16, 33), (60, 3, 128)])
def test_em_step_torch_matches_the_oracle(n, k, d):
    c = H.case(n, k, d)
    H.check_step(c, *G.em_step_torch(*H.tensors(c)))
    # CPU tensors go to the same function through the public entry points
    rs, xs, xxs, ll, R = G.em_step(*H.tensors(c))
    assert torch.equal(R, G.em_step_torch(*H.tensors(c))[4])
    H.check_posterior(c, *G.posterior(*H.tensors(c), True))
    assert G.posterior(*H.tensors(c), False)[1] is None


def test_train_gmm_centred_update_equals_the_raw_one(monkeypatch):
    X = H.blobs()
    w0, mu0, cv0 = H.model_arrays(H.train(X, 3, "cpu").collect())
    calls = []
    real = G.em_step

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(G, "em_selected", lambda X0, k: True)
    monkeypatch.setattr(G, "em_step", counted)
    w1, mu1, cv1 = H.model_arrays(H.train(X, 3, "cpu").collect())
    assert len(calls) == 5
    np.testing.assert_allclose(w1, w0, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(mu1, mu0, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(cv1, cv0, rtol=1e-9, atol=1e-12)


def test_mapper_posterior_route_equals_the_numpy_route(monkeypatch):
    X = H.blobs()
    model = H.train(X, 3, "cpu")
    p0, det0 = H.predict(model, X, "cpu")
    calls = []
    real = G.posterior

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(G, "em_selected", lambda X0, k: True)
    monkeypatch.setattr(G, "posterior", counted)
    p1, det1 = H.predict(model, X, "cpu")
    assert calls
    assert np.array_equal(p0, p1)
    np.testing.assert_allclose(det1, det0, rtol=1e-9, atol=1e-12)
    assert len(set(p0)) == 3


def test_selection_rule(monkeypatch):
    monkeypatch.delenv("ALINK_GMM_HIP", raising=False)
    ok = torch.zeros((10, 128), dtype=torch.float64)
    assert G.em_shape_ok(ok, 3) and G.em_shape_ok(ok[:, :1].contiguous(), 1)
    assert not G.em_shape_ok(torch.zeros((10, 129), dtype=torch.float64), 3)
    assert not G.em_shape_ok(ok.float(), 3)
    assert not G.em_shape_ok(ok[:, ::2], 3)
    assert not G.em_shape_ok(ok[:0], 3)
    assert not G.em_shape_ok(ok, 0)
    # CPU rows are never selected
    assert not G.em_supported(ok, 3) and not G.em_selected(ok, 3)
    # with supported rows and a library, the flag alone decides
    monkeypatch.setattr(G, "em_supported", lambda X0, k: True)
    monkeypatch.setattr(_lib, "kernels_enabled", lambda: True)
    assert G.em_selected(ok, 3)
    monkeypatch.setenv("ALINK_GMM_HIP", "0")
    assert not G.em_selected(ok, 3)
    monkeypatch.setenv("ALINK_GMM_HIP", "1")
    assert G.em_selected(ok, 3)


def test_chunk_rows_depend_on_the_shape_alone_and_fit_the_cap():
    for n, k, d in [(10 ** 7, 10, 32), (2 * 10 ** 6, 16, 128), (2 * 10 ** 7, 5, 8), (4 * 10 ** 6, 100, 16),
                    (200, 130, 17), (10 ** 5, 32, 64), (1, 1, 1)]:
        rows = G.em_chunk_rows(n, k, d)
        assert rows % 64 == 0 and rows >= 64
        nchunk = -(-n // rows)
        assert nchunk * k * (d * d + d + 1) * 8 <= G.EM_SCRATCH_BYTES <= 256 << 20
