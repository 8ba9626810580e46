"""Shared by ``test_gmm_em_device.py`` (CPU) and ``test_gmm_em_gpu.py``: seeded mixtures and rows, the numpy
``longdouble`` oracle of one EM step with its rounding bounds, and the operator calls.

The oracle starts from the same fp64 ``X0, mu0, W, logdet, rank, log w`` that the code under test gets and works
in ``longdouble`` (u_ld = 2^-64 on x86, whose own error is 2^-11 of every bound below and is ignored).

Bounds (u = 2^-53; first-order error of one fp64 evaluation against the exact value; the tests allow 4x, the
project's margin):

* projection ``z_c = sum_a x0_a W_ac - sum_a mu0_a W_ac``: two dots of d terms (in any order, fused or not, at most
  ``d u sum|.|`` each), the subtraction and the stored ``C`` add two more roundings:
  ``e_c = (d + 2) u (sum_a |x0_a| |W_ac| + sum_a |mu0_a| |W_ac|)``;
* ``q = sum_c z_c^2``: the squares of the perturbed z move by ``2 |z_c| e_c + e_c^2``, and a square, d - 1 additions
  of nonnegative terms in any order and one more rounding give ``(d + 2) u q``:
  ``E_q = sum_c (2 |z_c| e_c + e_c^2) + (d + 2) u q``;
* log density ``lp = cst - q / 2``, ``cst = -(rank log 2 pi)/2 - logdet/2 + log w``: the halving is exact, the three
  terms of cst, their two additions and the final subtraction are at most 4 roundings of values no larger than
  ``|lp|`` plus the magnitudes of the terms: ``E_lp = E_q / 2 + 4 u (|lp| + |rank log 2 pi / 2| + |logdet / 2| +
  |log w|)``;
* responsibilities ``r_j = exp(lp_j - lse)``: lse moves by at most ``max_j E_lp`` (it is a weighted mean of the lp
  perturbations) plus the k - 1 additions, the subtraction of the maximum, ``exp`` and ``log`` (about 1 ulp each):
  the exponent moves by ``2 max_j E_lp + (k + 8) u`` in all, so the relative bound is
  ``rho_i = expm1(2 max_j E_lp + (k + 8) u)``; where the oracle's r is below the fp64 normal range the result may be
  flushed, hence an absolute floor of 1e-290;
* moment sums: every term ``r_ij x0_a x0_b`` carries ``rho_i`` and the n-term sum in any order (products included)
  ``(n + 2) u``: ``|d xxs_j[a, b]| <= sum_i (rho_i + (n + 2) u) r_ij |x0_a x0_b|``, and the same form for ``xs``
  (``|x0_a|``) and ``rs`` (1);
* log likelihood ``sum_i lse_i``: ``sum_i (max_j E_lp + (k + 8) u + u |lse_i|)`` for the terms and
  ``n u sum_i |lse_i|`` for the n-term sum.

Inputs that keep these meaningful: covariance eigenvalues in [0.25, 4] on a random orthogonal basis (so |W| <= 2),
component 0 rank-deficient (eigenvalues 1, 1, 1, 0, ...) whenever d > 3, rows and means from 2 N(0, 1), weights from
U(0.5, 1.5), normalised.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -53
MARGIN = 4.0
R_FLOOR = 1e-290
LD = np.longdouble

D_ALL = (1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 127, 128)
K_ALL = (1, 2, 15, 16, 17, 64, 65, 130)
N_ALL = (1, 15, 16, 17, 63, 64, 65, 200)


class Case:
    """The fp64 inputs (numpy: X0, mu0, W, logdet, rank, logw), the oracle's r / rs / xs / xxs / ll / arg and the
    tolerances tol_* (already 4x the bound); ``sure`` = rows whose argmax is decided beyond 4x the bound."""


def mixture(k, d, rng, twin=False):
    """(w [k], mu [k, d], cov [k, d, d]) of the docstring; with ``twin`` component 1 repeats component 0's mean and
    covariance and the weights are all equal."""
    w = rng.uniform(0.5, 1.5, size=k)
    w = w / w.sum()
    mu = 2.0 * rng.normal(size=(k, d))
    cov = np.empty((k, d, d))
    for j in range(k):
        Q, _ = np.linalg.qr(rng.normal(size=(d, d)))
        lam = rng.uniform(0.25, 4.0, size=d)
        if j == 0 and d > 3:
            lam = np.array([1.0, 1.0, 1.0] + [0.0] * (d - 3))
        cov[j] = (Q * lam) @ Q.T
        cov[j] = 0.5 * (cov[j] + cov[j].T)
    if twin:
        w = np.full(k, 1.0 / k)
        mu[1], cov[1] = mu[0], cov[0]
    return w, mu, cov


def factors(w, mu, cov, centre):
    """The fp64 inputs of the step from the project's own ``_root_inv``: (mu0, W, logdet, rank, logw) as numpy."""
    from alink_amd.models.clustering.gmm import _root_inv
    W, logdet, rank = _root_inv(torch.as_tensor(cov))
    if len(w) > 1 and np.array_equal(cov[0], cov[1]):      # the twins get the same factors bit for bit
        W[1], logdet[1] = W[0], logdet[0]
    return mu - centre, W.numpy(), logdet.numpy(), rank.numpy(), np.log(w)


def oracle(X0, mu0, W, logdet, rank, logw, twin=False):
    n, d = X0.shape
    k = mu0.shape[0]
    c = Case()
    c.X0, c.mu0, c.W, c.logdet, c.rank, c.logw = X0, mu0, W, logdet, rank, logw
    Xl, ml, Wl = X0.astype(LD), mu0.astype(LD), W.astype(LD)
    aX, am, aW = np.abs(X0), np.abs(mu0), np.abs(W)
    half_log2pi = LD(0.5) * np.log(LD(8) * np.arctan(LD(1)))      # 2 pi = 8 atan(1), in longdouble
    lp = np.empty((n, k), dtype=LD)
    E_lp = np.empty((n, k))
    for j in range(k):
        z = Xl @ Wl[j] - ml[j] @ Wl[j]
        q = (z * z).sum(1)
        e = (d + 2) * U * (aX @ aW[j] + am[j] @ aW[j])
        az, qf = np.abs(z).astype(np.float64), q.astype(np.float64)
        E_q = (2 * az * e + e * e).sum(1) + (d + 2) * U * qf
        t1, t2, t3 = half_log2pi * LD(rank[j]), LD(0.5) * LD(logdet[j]), LD(logw[j])
        lp[:, j] = -t1 - t2 + t3 - q / 2
        E_lp[:, j] = E_q / 2 + 4 * U * (np.abs(lp[:, j]).astype(np.float64) + float(abs(t1)) + float(abs(t2))
                                        + float(abs(t3)))
    m = lp.max(1)
    lse = m + np.log(np.exp(lp - m[:, None]).sum(1))
    r = np.exp(lp - lse[:, None])
    Emax = E_lp.max(1)
    rho = np.expm1(2 * Emax + (k + 8) * U)
    rf = r.astype(np.float64)
    c.r, c.tol_r = rf, MARGIN * rho[:, None] * rf + R_FLOOR
    c.rho = rho
    lsef = lse.astype(np.float64)
    c.ll = float(lse.sum())
    c.tol_ll = MARGIN * ((Emax + (k + 8) * U + U * np.abs(lsef)).sum() + n * U * np.abs(lsef).sum())
    wt = (rho + (n + 2) * U)[:, None] * rf                        # [n, k]
    c.rs = r.sum(0).astype(np.float64)
    c.tol_rs = MARGIN * wt.sum(0)
    c.xs = (r.T @ Xl).astype(np.float64)
    c.tol_xs = MARGIN * (wt.T @ aX)
    c.xxs = np.empty((k, d, d))
    c.tol_xxs = np.empty((k, d, d))
    for j in range(k):
        c.xxs[j] = ((r[:, j:j + 1] * Xl).T @ Xl).astype(np.float64)
        c.tol_xxs[j] = MARGIN * ((wt[:, j:j + 1] * aX).T @ aX)
    c.arg = r.argmax(1)
    if k > 1:
        # twins: component 1 equals component 0 bit for bit and must never win; the margin is among the others
        top = np.sort(np.delete(rf, 1, axis=1) if twin and k > 2 else rf, axis=1)[:, -2:]
        c.sure = (top[:, 1] - top[:, 0]) > MARGIN * 2 * rho * top[:, 1]
    else:
        c.sure = np.ones(n, dtype=bool)
    return c


@functools.lru_cache(maxsize=None)
def case(n, k, d, twin=False):
    """Seeded rows around a seeded mixture, centred by the rows' mean, and their oracle."""
    assert n * k * d * d <= 1e8
    rng = np.random.default_rng(100000 * n + 1000 * k + d)
    w, mu, cov = mixture(k, d, rng, twin)
    X = 2.0 * rng.normal(size=(n, d))
    xbar = X.mean(0)
    return oracle(X - xbar, *factors(w, mu, cov, xbar), twin=twin)


def tensors(c, device="cpu", offset8=False):
    """The case's inputs as torch tensors on ``device``; with ``offset8`` the rows start 8 bytes into a 16-byte
    aligned allocation."""
    X0 = torch.from_numpy(c.X0).to(device)
    if offset8:
        flat = torch.empty(X0.numel() + 2, dtype=torch.float64, device=device)
        base = 1 if flat.data_ptr() % 16 == 0 else 2
        X0 = flat[base:base + X0.numel()].view(X0.shape).copy_(X0)
        assert X0.data_ptr() % 16 == 8 and X0.is_contiguous()
    return (X0,) + tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                         for a in (c.mu0, c.W, c.logdet, c.rank, c.logw))


def _ratio(got, want, tol):
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):        # 0 / 0 where both the error and the bound are 0
        return float(np.max(np.where(err == 0, 0.0, err / tol))) if got.size else 0.0


def check_step(c, rs, xs, xxs, ll, R, mirrored=False):
    """Asserts the five results of a step (torch tensors) against the oracle; prints the error / tolerance ratios
    first.  ``mirrored``: xxs must be symmetric bit for bit (the kernels compute one triangle)."""
    rs, xs, xxs, R = (t.detach().cpu().numpy() for t in (rs, xs, xxs, R))
    ll = float(ll)
    print("err/tol r", _ratio(R, c.r, c.tol_r), "rs", _ratio(rs, c.rs, c.tol_rs), "xs", _ratio(xs, c.xs, c.tol_xs),
          "xxs", _ratio(xxs, c.xxs, c.tol_xxs), "ll", abs(ll - c.ll) / c.tol_ll)
    assert R.shape == c.r.shape and xxs.shape == c.xxs.shape and xs.shape == c.xs.shape and rs.shape == c.rs.shape
    assert np.all(np.abs(R - c.r) <= c.tol_r)
    assert np.all(np.abs(rs - c.rs) <= c.tol_rs)
    assert np.all(np.abs(xs - c.xs) <= c.tol_xs)
    assert np.all(np.abs(xxs - c.xxs) <= c.tol_xxs)
    assert abs(ll - c.ll) <= c.tol_ll
    assert not mirrored or np.array_equal(xxs, xxs.transpose(0, 2, 1)), "xxs must be mirrored exactly"


def check_posterior(c, pred, prob=None):
    """``pred`` equals the oracle's argmax on the rows decided beyond 4x the bound, which must be 99 % of them."""
    pred = pred.detach().cpu().numpy()
    assert pred.dtype == np.int64 and pred.shape == c.arg.shape
    left_out = 1.0 - c.sure.mean()
    print("rows left out of the argmax check", left_out)
    assert left_out <= 0.01
    assert np.array_equal(pred[c.sure], c.arg[c.sure])
    assert pred.min() >= 0 and pred.max() < c.r.shape[1]
    if prob is not None:
        prob = prob.detach().cpu().numpy()
        print("err/tol prob", _ratio(prob, c.r, c.tol_r))
        assert np.all(np.abs(prob - c.r) <= c.tol_r)


# ---------------------------------------------------------------------------------------------------- operators

def blobs(n=600, d=5, k=3, seed=3):
    """Three blobs within a few units of the origin."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-3.0, 3.0, size=(k, d))
    return centres[np.arange(n) % k] + 0.5 * rng.normal(size=(n, d))


def vector_table(X, device="cpu"):
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    return MTable(TableSchema(["v"], [Types.DENSE_VECTOR]), [Column(torch.from_numpy(X).to(device))])


def train(X, k, device, max_iter=5):
    """``GmmTrainBatchOp`` linked to the rows X (``collect()`` gives the model rows)."""
    from alink_amd import GmmTrainBatchOp, useLocalEnv
    from alink_amd.operator.batch.source import TableSourceBatchOp
    useLocalEnv(1, device=device)
    op = GmmTrainBatchOp().setVectorCol("v").setK(k).setMaxIter(max_iter).setTol(0.0)
    return op.linkFrom(TableSourceBatchOp(vector_table(X, device)))


def model_arrays(rows):
    """(weights [k], means [k, d], packed covariances [k, d (d + 1) / 2]) of the model rows, by cluster id."""
    import json
    cl = []
    for row in rows:
        for v in row:
            if isinstance(v, str) and v.startswith("{") and "clusterId" in v:
                cl.append(json.loads(v))
    cl.sort(key=lambda c: c["clusterId"])
    return (np.array([c["weight"] for c in cl]), np.stack([np.array(c["mean"]["data"]) for c in cl]),
            np.stack([np.array(c["cov"]["data"]) for c in cl]))


def predict(model_op, X, device, detail=True):
    """(pred [n], detail [n, k] or None) of ``GmmPredictBatchOp``."""
    from alink_amd import GmmPredictBatchOp, useLocalEnv
    from alink_amd.operator.batch.source import TableSourceBatchOp
    useLocalEnv(1, device=device)
    op = GmmPredictBatchOp().setPredictionCol("p")
    if detail:
        op = op.setPredictionDetailCol("det")
    out = op.linkFrom(model_op, TableSourceBatchOp(vector_table(X, device))).collect()
    pred = np.array([int(r[1]) for r in out])
    det = np.array([[float(t) for t in r[2].split(" ")] for r in out]) if detail else None
    return pred, det
