"""Stochastic Outlier Selection through ``ops/sos.py`` on the CPU: the torch twins against the longdouble oracle of
``sos_helpers``, the range arguments, the selection rule and the wiring into ``sos_scores`` / ``SosBatchOp``."""
import numpy as np
import pytest
import torch

import sos_helpers as H
from alink_amd.models.outlier import sos as M
from alink_amd.ops import sos as S


def _x(c):
    return torch.from_numpy(c.X)


@pytest.mark.parametrize("spec", H.CASES + H.SWEEP, ids=lambda s: f"seed{s[0]}-n{s[1]}-d{s[2]}")
def test_fragile_share_within_cap(spec):
    c = H.case(*spec)
    print("fragile", int(c.fragile.sum()), "of", len(c.fragile), "iters", int(c.iters.min()), int(c.iters.max()))
    assert H.fragile_share(c) <= H.FRAGILE_CAP
    if spec in H.ZERO_FRAGILE:
        assert not c.fragile.any()


def test_sweep_covers_every_size():
    assert {s[2] for s in H.SWEEP} == set(H.D_ALL) and {s[1] for s in H.SWEEP} == set(H.N_ALL)
    assert all(s[4] < (s[1] - 1) / 3 for s in H.SWEEP)


@pytest.mark.parametrize("spec", H.CASES, ids=lambda s: f"seed{s[0]}-n{s[1]}-d{s[2]}")
def test_search_torch_matches_oracle(spec):
    c = H.case(*spec)
    H.check_search(c, *S.search_torch(_x(c), c.perplexity))


@pytest.mark.parametrize("spec", H.CASES, ids=lambda s: f"seed{s[0]}-n{s[1]}-d{s[2]}")
def test_products_torch_matches_oracle(spec):
    c = H.case(*spec)
    beta, s = torch.from_numpy(c.beta), torch.from_numpy(c.s)
    H.check_products(c, beta, s, S.products_torch(_x(c), beta, s))


def test_ranges_concatenate_exactly():
    c = H.case(*H.CASES[0])
    X = _x(c)
    n = X.shape[0]
    full = S.search(X, c.perplexity)
    a, b = S.search(X, c.perplexity, rows=(0, 131)), S.search(X, c.perplexity, rows=(131, n))
    for f, u, v in zip(full, a, b):
        assert torch.equal(f, torch.cat([u, v]))
    p = S.products(X, full[0], full[1])
    assert torch.equal(p, torch.cat([S.products(X, full[0], full[1], cols=(0, 131)),
                                     S.products(X, full[0], full[1], cols=(131, n))]))
    with pytest.raises(ValueError):
        S.search(X, c.perplexity, rows=(5, n + 1))


def test_selection_rule(monkeypatch):
    X = torch.zeros((8, 4), dtype=torch.float64)
    assert not S.sos_supported(X) and not S.sos_selected(X)               # a CPU tensor
    # the rest of the rule on a stand-in for a GPU tensor
    monkeypatch.setattr(S._lib, "kernels_enabled", lambda: True)

    class Dev(torch.Tensor):
        is_cuda = True
    def dev(t):
        return t.as_subclass(Dev)
    assert S.sos_selected(dev(X))
    assert not S.sos_selected(dev(X.float()))
    assert not S.sos_selected(dev(torch.zeros((8, 8), dtype=torch.float64)[:, :4]))
    assert not S.sos_selected(dev(torch.zeros((4, 1025), dtype=torch.float64)))
    assert S.sos_selected(dev(torch.zeros((4, 1024), dtype=torch.float64))) == (S.SOS_MAX_D >= 1024)
    assert not S.sos_selected(dev(torch.zeros((1, 4), dtype=torch.float64)))
    assert S.sos_selected(dev(torch.zeros((2, 1), dtype=torch.float64)))
    monkeypatch.setattr(S, "SOS_MAX_D", 3)
    assert not S.sos_selected(dev(X)) and S.sos_supported(dev(X))
    monkeypatch.setattr(S, "SOS_MAX_D", 1024)
    monkeypatch.setenv("ALINK_SOS_HIP", "0")
    assert not S.sos_selected(dev(X))


@pytest.mark.parametrize("spec", H.ZERO_FRAGILE, ids=lambda s: f"seed{s[0]}-n{s[1]}-d{s[2]}")
def test_sos_scores_goes_through_ops(monkeypatch, spec):
    c = H.case(*spec)
    calls = []
    real = S.scores
    monkeypatch.setattr(S, "sos_selected", lambda X: True)
    monkeypatch.setattr(S, "scores", lambda X, p: calls.append(1) or real(X, p))
    before = S.SOS_CALLS
    H.check_scores(c, M.sos_scores(_x(c), c.perplexity))
    assert calls == [1] and S.SOS_CALLS == before + 2


def test_operator_goes_through_ops(monkeypatch):
    c = H.case(*H.CASES[0])
    calls = []
    real = S.scores
    monkeypatch.setattr(S, "sos_selected", lambda X: True)
    monkeypatch.setattr(S, "scores", lambda X, p: calls.append(1) or real(X, p))
    before = S.SOS_CALLS
    got = H.run_op(H.vector_table(c.X), c.perplexity, "cpu")
    assert calls == [1] and S.SOS_CALLS == before + 2
    H.check_scores(c, torch.from_numpy(got))


def test_not_selected_keeps_former_path(monkeypatch):
    c = H.case(*H.CASES[0])
    monkeypatch.setattr(S, "scores", lambda X, p: pytest.fail("ops.sos.scores must not run for CPU rows"))
    before = S.SOS_CALLS
    got = M.sos_scores(_x(c), c.perplexity)
    assert S.SOS_CALLS == before
    assert got.shape == (len(c.scores),) and bool(torch.isfinite(got).all())


def test_none_falls_back_to_former_path(monkeypatch):
    X = torch.tensor([[0.0], [1e60]], dtype=torch.float64)
    want = M.sos_scores(X, 1.5)
    assert S.scores(X, 1.5) is None
    calls = []
    real = S.scores
    monkeypatch.setattr(S, "sos_selected", lambda X: True)
    monkeypatch.setattr(S, "scores", lambda X, p: calls.append(1) or real(X, p))
    got = M.sos_scores(X, 1.5)
    assert calls == [1]
    assert np.array_equal(got.numpy(), want.numpy(), equal_nan=True)
