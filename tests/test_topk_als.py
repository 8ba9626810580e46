"""als_topk end to end on a hand-built model with duplicated item factors and a zero user: the recommendation
strings equal the top-K oracle's in the cpu environment and in the cuda:0 environment, so the two agree."""
import numpy as np
import pytest

import topk_helpers as H
from alink_amd.common.javafmt import java_float_str
from alink_amd.models.recommendation.als import AlsModelData, als_topk

K = 6


def _model():
    U, V = H.tie_rich(51, 9, 90, 6)
    U[4] = 0                                                   # a cold user: every score 0, items in id order
    for i in (4, 16, 20, 63, 64, 65):                          # duplicated item factors
        V[i] = V[3]
    user_ids = np.arange(9) * 5 + 2
    item_ids = 1000 - 3 * np.arange(90)                        # row order, not item-id order, breaks the ties
    return AlsModelData(user_ids, U, item_ids, V), U, V


def _expected(model, U, V):
    val, idx = H.topk_oracle(U, V, K)
    return [(int(u), ",".join(f"{int(model.item_ids[i])}:{java_float_str(float(s))}" for s, i in zip(vr, ir)))
            for u, vr, ir in zip(model.user_ids, val, idx)]


def test_als_topk_cpu_equals_oracle():
    model, U, V = _model()
    want = _expected(model, U, V)
    assert want[4][1].split(",")[0] == "1000:0.0"
    assert als_topk(model, model.user_ids.tolist(), K, "cpu") == want


@pytest.mark.gpu
def test_als_topk_cuda_equals_cpu_and_oracle():
    from alink_amd.ops import topk as ops
    model, U, V = _model()
    import torch
    assert ops.kernel_supported(torch.zeros(1, 6, device="cuda:0"), K)
    got = als_topk(model, model.user_ids.tolist(), K, "cuda:0")
    assert got == als_topk(model, model.user_ids.tolist(), K, "cpu") == _expected(model, U, V)
