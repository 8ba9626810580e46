"""The GLM device path on the CPU: the torch twins of ops/glm.py against the longdouble oracle of tests/glm_helpers.py
for every covered (family, link) pair, and the shape rule."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import glm_helpers as H  # noqa: E402

from alink_amd.ops import glm as G  # noqa: E402

COLS = ("eta", "pred", "z", "ww", "dres", "pres", "wres", "rres", "sums")
# fp64 formulas against longdouble at n = 65, k = 3: a few roundings per output, amplified where y - mu or
# ylogy - (y - mu) or the tweedie powers cancel: up to four digits on these draws, so 1e4 x 2^-53 x a few roundings
# (measured: at most 1.6e-12, profiles/glm.txt)
TWIN_TOL = 1e-11


def tensors(case):
    return [torch.from_numpy(case[key]) for key in ("X", "y", "w", "off", "beta")]


def twin_rows(case, fam, lnk, mode, cnull):
    X, y, w, off, beta = tensors(case)
    return G.rows_torch(X, y, w, off, beta, case["intercept"], fam, lnk, H.VP, H.LP,
                        ("pred", "eta", "resid", "zw", "sums"), G.INIT if mode == "init" else G.STEP, cnull)


@pytest.mark.parametrize("mode", ["init", "step"])
@pytest.mark.parametrize("fam,lnk", H.PAIRS)
def test_torch_twins_match_the_longdouble_oracle(fam, lnk, mode):
    case = H.make_case(fam, lnk, 65, 3)
    cnull = case["intercept"]
    ref = H.oracle(case, fam, lnk, mode, cnull)
    got = twin_rows(case, fam, lnk, mode, cnull)
    for name in COLS:
        assert H.rel_err(got[name].numpy(), ref[name]) <= TWIN_TOL, name
    # the statistics: [sum ww^2 | G] of the augmented rows under the oracle's z and ww, over the rows whose z is finite
    # (in init mode link(initialize(y)) leaves a link's domain for some families: logit or cloglog of y >= 1)
    fin = np.isfinite(ref["z"])
    assert mode == "init" or fin.all()
    assert fin.sum() >= (20 if fam in ("gaussian", "binomial") or lnk not in ("logit", "cloglog") else 1)
    X, y, w, off, beta = (v[torch.from_numpy(fin)] if v.shape[0] == 65 else v for v in tensors(case))
    wwsum, gram = G.irls_stats(X, y, w, off, beta, case["intercept"], fam, lnk, H.VP, H.LP,
                               G.INIT if mode == "init" else G.STEP)
    A = np.concatenate([case["X"].astype(H.L), np.ones((65, 1), H.L), ref["z"][:, None]], 1)[fin]
    assert H.rel_err(gram.numpy(), (A * ref["ww"][fin, None]).T @ A) <= TWIN_TOL
    assert H.rel_err(wwsum.numpy(), (ref["ww"][fin] ** 2).sum()) <= TWIN_TOL


def test_shape_rule():
    X = torch.zeros((8, 126), dtype=torch.float64)
    assert G.shape_ok(X, "poisson", "log") and not G.supported(X, "poisson", "log")      # a CPU tensor
    assert not G.shape_ok(X, "binomial", "probit")
    assert not G.shape_ok(torch.zeros((8, 127), dtype=torch.float64), "poisson", "log")
    assert not G.shape_ok(X.float(), "poisson", "log")
    assert not G.shape_ok(torch.zeros((8, 252), dtype=torch.float64)[:, ::2], "poisson", "log")
    assert not G.shape_ok(X[:, :0], "poisson", "log")
    assert G.glm_chunk_rows(10 ** 7, 126) % 64 == 0
    assert -(-10 ** 7 // G.glm_chunk_rows(10 ** 7, 126)) * 8 * (1 + 128 ** 2) <= G.GLM_SCRATCH_BYTES
