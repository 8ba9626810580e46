"""The fused Newton pass (ops/csrc/newton.hip) on the GPU against the longdouble oracle of tests/newton_helpers.py,
against itself (grids, chunk lengths, repeats), and three trainers under ``optimMethod = "Newton"`` against
``ALINK_NEWTON_HIP=0``.

Bound per element: (n + 4) 2^-53 S + eps_c S, S = sum_i |c_i x_ia x_ib|: the worst case for any order of n rounded or
fused products, plus the per-row coefficient's own error, eps_c = max(4 x the relative error of the torch derivative /
second_derivative against the oracle on the same inputs on the CPU, 2^-50); at most 7.8e-15 over the cases of
test_sums_against_the_oracle (profiles/newton.txt).  A dropped or doubled row exceeds the bound by ten orders."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newton_helpers as H  # noqa: E402

from alink_amd.ops import _lib, newton as N  # noqa: E402

pytestmark = pytest.mark.gpu
DS, NS = (1, 2, 15, 16, 17, 33, 47, 48, 64, 65, 113, 128), (1, 3, 63, 64, 65, 200)
# d and n taken in turn: every tile count 1 .. 8, the row-split rule at one and two tiles, odd d (scalar loads) and the
# ragged deal of the tiles to the waves; the widest rows and 7 tiles over several chunks as well; at chunk_rows = 64,
# n = 513 and 641 are 9 and 11 chunks: the merge's round of eight loads in flight without a tail and with one of two
CASES = list(zip(DS, itertools.cycle(NS))) + [(128, 200), (97, 65), (17, 513), (17, 641)]


SM_CASES = [(1, 1), (2, 3), (3, 16), (4, 17), (9, 33), (7, 128), (8, 128), (16, 64), (63, 16), (64, 16)]


def run(case, grid=0, chunk_rows=0):
    t = [torch.from_numpy(case[key]).cuda() for key in ("X", "y", "w", "W" if "W" in case else "coef")]
    calls = N.NEWTON_CALLS
    out = N.softmax_sums(*t, grid, chunk_rows) if "W" in case else \
        N.unary_sums(*t, case["code"], case["p"], grid, chunk_rows)
    assert N.NEWTON_CALLS == calls + 1
    return [o.cpu().numpy() for o in out]


def check(got, ref):
    for name, v in zip(("H", "g", "ws", "loss"), got):
        err = np.abs(v.astype(H.L) - ref[name])
        print(name, "eps_c", ref["eps"], "err / bound", float(np.max(err / np.maximum(ref[name + "_bound"], 1e-300))))
        assert np.isfinite(v).all() and (err <= ref[name + "_bound"]).all(), name
    assert np.array_equal(got[0], got[0].T)
    assert not (ref["zero_hessian"] and got[0].any())


@pytest.mark.parametrize("chunk_rows", [0, 64])
@pytest.mark.parametrize("d,n", CASES)
def test_sums_against_the_oracle(d, n, chunk_rows):
    """H, g, the weight sum and the loss sum of the log loss (labels +-1, every fifth weight 0); H exactly symmetric."""
    _lib.require()
    case = H.make_case(0, n, d, seed=d)
    check(run(case, chunk_rows=chunk_rows), H.oracle(case))


@pytest.mark.parametrize("code,k", [(c, 3) for c in range(9)] + [(H.AFT, k) for k in (3, 1, 16, 127)]
                         + [(c, 17) for c in (1, 2, 4, 6, 7)])
def test_every_loss(code, k):
    """All nine loss codes and AFT at n = 65; at k = 3 on rows that take every branch of the loss (asserted on the
    oracle's own masks; the branch rows of the log losses have eps_c = 0.17, profiles/newton.txt), at k = 17 the
    losses with l'' != 0 on random rows, where eps_c is a few 2^-53.  The losses with l'' = 0 give H = 0 exactly."""
    _lib.require()
    case = H.make_case(code, 65, k, seed=100 + code, branches=k == 3)
    check(run(case), H.oracle(case))


@pytest.mark.parametrize("k1,m,n,chunk_rows", [c + (65, 0) for c in SM_CASES]
                         + [(9, 33, 200, 64), (9, 33, 513, 64), (9, 33, 641, 64)])
def test_softmax_sums_against_the_oracle(k1, m, n, chunk_rows):
    """H (every block, exactly symmetric as a whole), G and the sums of the softmax pass: one to four class tiles, one
    to eight dim tiles, one pair and many pairs per unit, a last group that is not full, several chunks (4, and 9 and
    11: the merge's round of eight loads in flight)."""
    _lib.require()
    case = H.softmax_case(n, m, k1, seed=100 * k1 + m)
    check(run(case, chunk_rows=chunk_rows), H.softmax_oracle(case))


@pytest.mark.parametrize("softmax", [False, True])
def test_same_bits_for_every_grid_and_run(softmax):
    """grid = 1, the default grid and a repeated call give the same bits at either chunk length; across chunk
    lengths the sums differ within the oracle's bound only."""
    _lib.require()
    case = H.softmax_case(200, 33, 9, seed=933) if softmax else H.make_case(0, 200, 65, seed=65)
    ref = H.softmax_oracle(case) if softmax else H.oracle(case)
    for chunk_rows in (64, 128):
        a, b, c = run(case, 1, chunk_rows), run(case, 0, chunk_rows), run(case, 0, chunk_rows)
        assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c))
        check(a, ref)


def test_operators_against_the_former_path(monkeypatch):
    """The LogisticRegression, Softmax (3 classes) and AftSurvivalReg trainers (n = 300, 4 features) under Newton with the fused
    pass against ``ALINK_NEWTON_HIP=0``: Newton corrects itself, so the fixed point moves by about cond(H) 2^-53, far
    inside the 1e-9 of tests/test_glm_gpu.py's operator comparison; a wrong coefficient or row moves it by 1e-3."""
    _lib.require()
    from alink_amd import (AftSurvivalRegTrainBatchOp, LogisticRegressionTrainBatchOp, MemSourceBatchOp,
                           SoftmaxTrainBatchOp, useLocalEnv)
    rng = np.random.default_rng(5)
    X = rng.normal(size=(300, 4))
    eta = X @ np.array([1.0, -0.5, 0.25, 0.5])
    lab = (eta + 0.5 * rng.normal(size=300) > 0).astype(int)
    lab3 = np.digitize(eta + 0.5 * rng.normal(size=300), [-0.5, 0.5])
    t, cen = np.exp(0.3 * eta + 0.2 * rng.normal(size=300)), (rng.random(300) < 0.8).astype(float)
    rows = [tuple(x) + (int(a), float(b), float(c), int(d)) for x, a, b, c, d in zip(X.tolist(), lab, t, cen, lab3)]

    def coefs(op):
        op.getParams().set("optimMethod", "Newton")         # the AFT trainer reads the parameter and has no setter
        model = op.setFeatureCols(["a", "b", "c", "d"]).setMaxIter(30).linkFrom(src).collect()
        found = [json.loads(f)["coefVector"]["data"] for r in model for f in r
                 if isinstance(f, str) and '"coefVector"' in f]
        assert len(found) == 1
        return np.array(found[0])
    try:
        useLocalEnv(1, device="cuda:0")
        src = MemSourceBatchOp(rows, "a double, b double, c double, d double, y int, t double, cen double, y3 int")
        for make in (lambda: LogisticRegressionTrainBatchOp().setLabelCol("y"),
                     lambda: SoftmaxTrainBatchOp().setLabelCol("y3"),
                     lambda: AftSurvivalRegTrainBatchOp().setLabelCol("t").setCensorCol("cen")):
            got = {}
            for flag in ("1", "0"):
                monkeypatch.setenv("ALINK_NEWTON_HIP", flag)
                calls = N.NEWTON_CALLS
                got[flag] = coefs(make())
                assert (N.NEWTON_CALLS > calls) == (flag == "1")
            np.testing.assert_allclose(got["1"], got["0"], rtol=1e-9)
    finally:
        useLocalEnv(1, device="cpu")
