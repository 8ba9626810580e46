"""The GLM kernels (ops/csrc/glm.hip) on the GPU against the longdouble oracle of tests/glm_helpers.py, the former
torch path and themselves (grids, alignment), and the three operators against ``ALINK_GLM_HIP=0``."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import glm_helpers as H  # noqa: E402

from alink_amd.ops import _lib, glm as G  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = ("pred", "eta", "resid", "zw", "sums")
COLS = ("eta", "pred", "z", "ww", "dres", "pres", "wres", "rres", "sums")
KS, NS = (1, 2, 13, 14, 15, 30, 31, 126), (1, 3, 63, 64, 65, 200)
# k and n taken in turn, the widest rows over several chunks as well, and k + 2 = 48, 64, 65, 96, 112: 3 .. 7 tiles,
# where the deal of the tiles to the waves (t mod 4) is ragged; at chunk_rows = 64, n = 513 and 641 are 9 and 11
# chunks: the merge's round of eight loads in flight without a tail and with one of two
GRAM_CASES = list(zip(KS, itertools.cycle(NS))) + [(126, 200), (31, 65), (46, 65), (62, 200), (63, 64), (94, 65),
                                                    (110, 200), (14, 513), (14, 641)]


def dev_case(case):
    return [torch.from_numpy(case[key]).cuda() for key in ("X", "y", "w", "off", "beta")]


def run_rows(t, case, fam, lnk, want=ALL, mode=G.STEP, cnull=0.0, grid=0, fn=None):
    calls = G.GLM_CALLS
    out = (fn or G.rows)(*t, case["intercept"], fam, lnk, H.VP, H.LP, want, mode, cnull, *(() if fn else (grid,)))
    assert fn is not None or G.GLM_CALLS > calls
    return out


def run_stats(t, case, fam, lnk, mode=G.STEP, grid=0, chunk_rows=0):
    calls = G.GLM_CALLS
    out = G.irls_stats(*t, case["intercept"], fam, lnk, H.VP, H.LP, mode, grid, chunk_rows)
    assert G.GLM_CALLS > calls
    return out


@pytest.mark.parametrize("mode", [G.PLAIN, G.INIT, G.STEP])
@pytest.mark.parametrize("chunk_rows", [0, 64])
@pytest.mark.parametrize("k,n", GRAM_CASES)
def test_gram_against_the_oracle(k, n, chunk_rows, mode):
    """G and sum ww^2 of every mode against the longdouble Gram of [X | 1 | z] under ww, z and ww the row kernel's own
    outputs for that mode, so only the sums are under test.  Bound per element: (n + 4) 2^-53 sum_i |ww_i a_ia a_ib|,
    the worst case for any order of n rounded or fused products; a dropped or doubled row exceeds it by ten orders."""
    _lib.require()
    case = H.make_case("poisson", "log", n, k, seed=k)
    t = dev_case(case)
    r = run_rows(t, case, "poisson", "log", ("zw",), mode)
    wwsum, gram = run_stats(t, case, "poisson", "log", mode, chunk_rows=chunk_rows)
    z, ww = r["z"].cpu().numpy().astype(H.L), r["ww"].cpu().numpy().astype(H.L)
    assert np.isfinite(z).all() and np.isfinite(ww).all()
    A = np.concatenate([case["X"].astype(H.L), np.ones((n, 1), H.L), z[:, None]], 1)
    ref = (A * ww[:, None]).T @ A
    bound = (n + 4) * H.L(2) ** -53 * ((np.abs(A) * ww[:, None]).T @ np.abs(A))
    got = gram.cpu().numpy()
    assert (np.abs(got.astype(H.L) - ref) <= bound).all()
    assert np.array_equal(got, got.T)
    assert abs(H.L(float(wwsum)) - (ww * ww).sum()) <= (n + 4) * H.L(2) ** -53 * (ww * ww).sum()


@pytest.mark.parametrize("mode", ["init", "step"])
@pytest.mark.parametrize("fam,lnk", H.PAIRS)
def test_row_values_against_the_oracle(fam, lnk, mode):
    """Every row output and the four sums at n = 65, k = 3.  Tolerance: 4 x the former torch path's largest
    relative error against the same oracle on the same inputs on the CPU (the margin covers differing exp / log / pow
    implementations), at least 2^-50.  Measured torch errors (profiles/glm.txt): 2.9e-16 .. 1.6e-12, the large ones
    where the deviance or y - mu cancels."""
    _lib.require()
    case = H.make_case(fam, lnk, 65, 3)
    cnull, m = case["intercept"], (G.INIT if mode == "init" else G.STEP)
    ref = H.oracle(case, fam, lnk, mode, cnull)
    cpu = run_rows([torch.from_numpy(case[key]) for key in ("X", "y", "w", "off", "beta")], case, fam, lnk, ALL, m,
                   cnull, fn=G.rows_torch)
    tol = max(4 * max(H.rel_err(cpu[c].numpy(), ref[c]) for c in COLS), 2.0 ** -50)
    got = run_rows(dev_case(case), case, fam, lnk, ALL, m, cnull)
    errs = {c: H.rel_err(got[c].cpu().numpy(), ref[c]) for c in COLS}
    print(fam, lnk, mode, "tol %.3e" % tol, {c: "%.2e" % e for c, e in errs.items()})
    assert max(errs.values()) <= tol, errs


NOT_FINITE = {("gaussian", "dres"): [0, 4], ("poisson", "dres"): [0, 4], ("gaussian", "wres"): [1, 5]}


@pytest.mark.parametrize("fam,lnk", [("gaussian", "log"), ("binomial", "logit"), ("binomial", "cloglog"),
                                      ("poisson", "log"), ("gamma", "log"), ("tweedie", "log")])
def test_clamps(fam, lnk):
    """eta = +-800 drives unlink to inf, 0 and 1 (rows 0, 1, 4, 5; rows 2, 3 are moderate, with y = 0 among them for
    poisson, tweedie and binomial).  pred must be ``project``'s constant, bit for bit what the former path gives.
    Every output is finite on every row but the two that cannot be, on either path (``NOT_FINITE``): the deviance
    residual at mu = JAVA_MAX_VALUE for gaussian and poisson, whose deviance (w (y - MAX)^2, 2 w (.. + MAX))
    overflows, and gaussian's working residual at eta = -800, where exp underflows to mu = 0, gaussian's ``project``
    has no lower clamp and log's derivative is 1 / 0.  All four residuals agree with the former path on all six rows
    (the same inf where not finite) within 128 x 2^-53: mu has the same bits on both paths at the clamp rows, so what
    differs is the log / exp / sqrt implementation (a few ulp each), through at most ten-fold cancellation in y - mu
    on the moderate rows and a handful of operations."""
    _lib.require()
    eta = np.array([800.0, -800.0, -0.5, -1.0, 800.0, -800.0])
    y = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]) if fam in ("binomial", "poisson", "tweedie") else np.full(6, 0.7)
    case = {"X": eta[:, None].copy(), "y": y, "w": np.ones(6), "off": np.zeros(6), "beta": np.ones(1),
            "intercept": 0.0}
    t = dev_case(case)
    got = {c: v.cpu().numpy() for c, v in run_rows(t, case, fam, lnk, ("pred", "eta", "resid")).items()}
    old = {c: v.cpu().numpy() for c, v in run_rows(t, case, fam, lnk, ("pred", "eta", "resid"),
                                                   fn=G.rows_torch).items()}
    hi = float(H.JMAX) if fam != "binomial" else 1.0 - 1e-16
    lo = 0.0 if fam == "gaussian" else 1e-16
    assert np.array_equal(got["pred"][[0, 1, 4, 5]], [hi, lo, hi, lo])
    assert np.array_equal(got["pred"][[0, 1, 4, 5]], old["pred"][[0, 1, 4, 5]])
    for c in ("pred", "eta", "dres", "pres", "wres", "rres"):
        finite = np.ones(6, dtype=bool)
        finite[NOT_FINITE.get((fam, c), [])] = False
        assert np.array_equal(np.isfinite(got[c]), finite) and np.array_equal(np.isfinite(old[c]), finite), c
    for c in ("dres", "pres", "wres", "rres"):
        print(fam, lnk, c, got[c], old[c])
        np.testing.assert_allclose(got[c], old[c], rtol=128 * 2.0 ** -53, atol=0, err_msg=c)


@pytest.mark.parametrize("n,k", [(200, 14), (200, 126), (65, 31), (200, 62), (200, 94)])
def test_same_bits_for_every_grid(n, k):
    _lib.require()
    case = H.make_case("poisson", "log", n, k, seed=n + k)
    t = dev_case(case)
    runs = [(run_stats(t, case, "poisson", "log", grid=g, chunk_rows=64), run_rows(t, case, "poisson", "log", grid=g))
            for g in (0, 1, 7, 7)]
    for (s, r) in runs[1:]:
        assert torch.equal(s[0], runs[0][0][0]) and torch.equal(s[1], runs[0][0][1])
        assert all(torch.equal(r[c], runs[0][1][c]) for c in COLS)


@pytest.mark.parametrize("k", [2, 15, 126])
def test_rows_at_an_8_byte_offset_give_the_same_bits(k):
    _lib.require()
    case = H.make_case("poisson", "log", 70, k, seed=k)
    t = dev_case(case)
    base = torch.empty(70 * k + 1, dtype=torch.float64, device="cuda")
    shifted = base[1:].view(70, k)
    shifted.copy_(t[0])
    assert t[0].data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 8
    t8 = [shifted] + t[1:]
    a, b = run_stats(t, case, "poisson", "log"), run_stats(t8, case, "poisson", "log")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ra, rb = run_rows(t, case, "poisson", "log"), run_rows(t8, case, "poisson", "log")
    assert all(torch.equal(ra[c], rb[c]) for c in COLS)


def test_operators_against_the_former_path(monkeypatch):
    """GlmTrainBatchOp (poisson, n = 300, k = 3) with the kernels against ``ALINK_GLM_HIP=0``: IRLS corrects itself,
    so the fixed point moves by about cond(M) 2^-53, and cond(M) <= 291 over the iterations on this table (computed on
    the CPU): far inside 1e-9, while a wrong weight, row or link moves a coefficient by more than 1e-3.  Then
    GlmPredictBatchOp and GlmEvaluationBatchOp of one model under both settings: columns by the row tolerance rule
    (4 x the former path's error against the oracle, at least 2^-50); the sums have positive terms only, so either
    path is within that plus (n + 4) 2^-53 of the truth, and the two within twice that of each other."""
    _lib.require()
    from alink_amd import GlmEvaluationBatchOp, GlmPredictBatchOp, GlmTrainBatchOp, MemSourceBatchOp, useLocalEnv
    rng = np.random.default_rng(3)
    X = rng.uniform(0.1, 1.0, size=(300, 3))
    y = rng.poisson(np.exp(X @ np.array([0.8, -0.5, 0.3]) + 0.2)).astype(float)
    rows = [tuple(x) + (float(v),) for x, v in zip(X.tolist(), y)]

    def conf(op):
        return op.setFamily("poisson").setFeatureCols(["a", "b", "c"]).setLabelCol("y").setMaxIter(25)

    def under(flag, fn):
        monkeypatch.setenv("ALINK_GLM_HIP", flag)
        calls = G.GLM_CALLS
        out = fn()
        assert (G.GLM_CALLS > calls) == (flag == "1")
        return out
    try:
        useLocalEnv(1, device="cuda:0")
        src = MemSourceBatchOp(rows, "a double, b double, c double, y double")
        train = {f: under(f, lambda: conf(GlmTrainBatchOp()).linkFrom(src)) for f in ("1", "0")}
        fit = {f: [json.loads(r[1]) for r in sorted(t.collect(), key=lambda r: r[0])[1:4]] for f, t in train.items()}
        for a, b in zip(fit["1"], fit["0"]):            # coefficients, intercept, diagInvAtWA
            np.testing.assert_allclose(a, b, rtol=1e-9)
        out = {}
        for f in ("1", "0"):
            pred = under(f, lambda: GlmPredictBatchOp().setPredictionCol("p").setLinkPredResultCol("e")
                         .linkFrom(train["0"], src).collect())
            ev = under(f, lambda: conf(GlmEvaluationBatchOp()).linkFrom(train["0"], src))
            out[f] = (np.array([r[-2:] for r in pred]), np.array([r[-5:] for r in ev.getSideOutput(0).collect()]),
                      json.loads(ev.collect()[0][0]))
    finally:
        useLocalEnv(1, device="cpu")
    case = {"X": X, "y": y, "w": np.ones(300), "off": np.zeros(300), "beta": np.array(fit["0"][0]),
            "intercept": fit["0"][1]}
    ref = H.oracle(case, "poisson", "log", "step")
    want = [ref[c] for c in ("pred", "eta", "pred", "dres", "pres", "wres", "rres")]
    errs = {f: [H.rel_err(col, r) for col, r in zip(list(o[0].T) + list(o[1].T), want)] for f, o in out.items()}
    tol = max(4 * max(errs["0"]), 2.0 ** -50)
    print("operator columns: tol %.3e" % tol, errs)
    assert max(errs["1"]) <= tol
    for key in ("deviance", "nullDeviance", "dispersion"):
        np.testing.assert_allclose(out["1"][2][key], out["0"][2][key], rtol=2 * (tol + 304 * 2.0 ** -53))
