"""``pairwise_moments_torch`` and the shared epilogue ``_corr_of_pairwise`` on the CPU against a two-pass pairwise
oracle: a column without a present cell, two columns present on disjoint rows, a row without a present cell."""
import numpy as np
import torch

from alink_amd.models.statistics.summary import _corr_of_pairwise
from alink_amd.ops import moments as M


def test_torch_moments_and_epilogue_on_the_structured_pattern():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 5)) + 1e6
    X[:, 0], X[0::2, 1], X[1::2, 2], X[39, :] = np.nan, np.nan, np.nan, np.nan
    shift = torch.tensor([0.0, X[1, 1], X[0, 2], X[0, 3], X[0, 4]])
    mom = M.pairwise_moments(torch.from_numpy(X), shift)        # a CPU tensor takes pairwise_moments_torch
    K = ~np.isnan(X)
    assert np.array_equal(mom[0].numpy(), K.T.astype(float) @ K.astype(float)) and mom[0, 1, 2] == 0
    assert torch.equal(mom, M.pairwise_moments_torch(torch.from_numpy(X), shift))
    corr = _corr_of_pairwise(mom)
    for a in range(5):
        for b in range(5):
            both = K[:, a] & K[:, b]
            if a == b:
                assert corr[a, b] == 1.0
            elif both.sum() < 2:
                assert np.isnan(corr[a, b])
            else:
                assert abs(corr[a, b] - np.corrcoef(X[both, a] - X[both, a][0], X[both, b] - X[both, b][0])[0, 1]) < 1e-12
