"""A numpy longdouble oracle of the Newton sums (H, g, the weight sum and the unweighted loss sum) for the nine unary
losses and AFT, written from the formulas of alink_amd/models/linear/objfunc.py, with seeded inputs and the bounds
that tests/test_newton_gpu.py holds the kernel to."""
import numpy as np
import torch

from alink_amd.models.common.features import FeatureMatrix
from alink_amd.models.linear import objfunc as O

L = np.longdouble
U = L(2) ** -53
AFT = 9
PARAM = {7: 1.0, 8: 0.5}        # Huber's delta, SVR's epsilon
LOSSES = {0: O.LogLossFunc, 1: O.LogisticLossFunc, 2: O.SquareLossFunc, 3: O.HingeLossFunc,
          4: O.SmoothHingeLossFunc, 5: O.PerceptronLossFunc, 6: O.ExponentialLossFunc,
          7: lambda: O.HuberLossFunc(PARAM[7]), 8: lambda: O.SvrLossFunc(PARAM[8])}


def row_terms(code, p, eta, y, w):
    """(l, l', l'') per row in longdouble; the branches each loss can take, as masks, come fourth."""
    d, x, z, one = eta * y, eta - y, np.zeros_like(eta), np.ones_like(eta)
    if code in (0, 1):
        ln2 = np.log(L(2)) if code == 1 else L(1)
        lo, hi = d < -37, d > 34
        dm = np.clip(d, -37, 34)
        l = np.where(lo, -d, np.where(hi, z, np.log1p(np.exp(-dm)))) / ln2
        t = y / (1 + np.exp(np.minimum(d, 700)))
        if code == 0:
            d1 = np.where(lo, -y, np.where(hi, z, -y / (np.exp(dm) + 1)))
        else:
            d1 = np.where(lo, -y, -y / (np.exp(np.minimum(d, 700)) + 1)) / ln2
        return l, d1, t * (y - t) / ln2, [lo, hi, d > 700, ~lo & ~hi]
    if code == 2:
        return x * x / 2, x, one, []
    if code == 3:
        return np.maximum(1 - d, 0), np.where(d < 1, -y, z), z, [d < 1, d >= 1]
    if code == 4:
        l = np.where(d <= 0, 0.5 - d, np.where(d >= 1, z, (1 - d) ** 2 / 2))
        d1 = np.where(d <= 0, -y, np.where(d >= 1, z, (1 - d) * -y))
        return l, d1, np.where((d >= 1) | (d <= 0), z, y * y), [d == 0, d == 1, d < 0, d > 1, (d > 0) & (d < 1)]
    if code == 5:
        return np.maximum(-d, 0), np.where(d < 0, -y, z), z, [d < 0, d >= 0]
    if code == 6:
        e = np.exp(-d)
        return e, -y * e, y * y * e, []
    out = np.abs(x) > p
    if code == 7:
        return (np.where(out, p * (np.abs(x) - p / 2), x * x / 2), np.where(out, np.sign(x) * p, x),
                np.where(out, z, one), [out, np.abs(x) < p])
    return np.maximum(np.abs(x) - p, 0), np.where(out, np.sign(x), z), z, [out, np.abs(x) < p]


def make_case(code, n, k, seed, branches=False):
    """Seeded X [n, k], y, w (every fifth 0; AFT: the censor indicator) and coef (AFT: k + 1 entries, the last log
    sigma).  ``branches``: dyadic rows (eta exact in fp64) whose first rows put eta y below -37, above 34 and 700, at
    0 and 1 exactly and between, or eta - y on both sides of delta and epsilon (moderate where exp would overflow)."""
    rng = np.random.default_rng(seed)
    cls = code in (0, 1, 3, 4, 5, 6)
    if branches:
        X = rng.integers(-8, 9, size=(n, k)) / 8.0
        coef = np.array([1.0, 0.5, -2.0, 0.25][:k] + [0.25] * (code == AFT))
        eta0 = [-40.0, 36.0, 800.0, 0.0, 1.0, 0.5, -0.5] if code in (0, 1, 3, 4, 5) else \
            [0.0, 1.0, 0.5, -0.5, 2.0, -3.0, 0.25]
        X[:len(eta0)] = 0.0
        X[:len(eta0), 0] = eta0
        y = np.where(np.arange(n) < len(eta0), 1.0, rng.choice([-1.0, 1.0], n)) if cls else \
            rng.integers(-8, 9, n) / 4.0
        y[len(eta0):2 * len(eta0)] = -1.0 if cls else 0.75
        X[len(eta0):2 * len(eta0)] = X[:len(eta0)]
    else:
        X = rng.normal(size=(n, k))
        coef = rng.normal(size=k + (code == AFT)) / np.sqrt(k)
        y = rng.choice([-1.0, 1.0], n) if cls else rng.normal(size=n)
    w = rng.uniform(0.5, 2.0, n)
    w[::5] = 0.0
    if code == AFT:
        w = (rng.random(n) < 0.7).astype(float)
    return {"X": X, "y": y, "w": w, "coef": coef, "code": code, "p": PARAM.get(code, 0.0), "branches": branches}


def torch_coefs(case):
    X, y, w, coef = (torch.from_numpy(case[key]) for key in ("X", "y", "w", "coef"))
    if case["code"] == AFT:
        obj = O.AftRegObjFunc()
        data = O.LabeledData(FeatureMatrix(X), y, w)
        _, sigma, eps = obj._parts(data, coef)
        return obj.loss_per_sample(data, coef), (w - torch.exp(eps)) / sigma, torch.exp(eps) / (sigma * sigma)
    u = LOSSES[case["code"]]()
    eta = X @ coef
    return u.loss(eta, y), w * u.derivative(eta, y), u.second_derivative(eta, y) * w


def rel_err(got, want):
    nz = want != 0
    assert (got[~nz] == 0).all()
    return float(np.max(np.abs(got[nz].astype(L) - want[nz]) / np.abs(want[nz]), initial=0.0))


def oracle(case):
    """The exact sums and their bounds: per element (n + 4) 2^-53 S + eps S with S = sum_i |c_i x_ia x_ib| (|c_i x_ia|
    for g, |l_i| for the loss), eps = max(4 x the relative error of the torch coefficients on the CPU, 2^-50)."""
    X, y, w, coef = (case[key].astype(L) for key in ("X", "y", "w", "coef"))
    n, k = X.shape
    code = case["code"]
    tail = []
    if code == AFT:
        ls, sigma = coef[-1], np.exp(coef[-1])
        eps = (y - X @ coef[:k]) / sigma
        ee = np.exp(eps)
        l, gc, hc, ws = w * (ls - eps) + ee, (w - ee) / sigma, ee / (sigma * sigma), L(n)
        tail = [w + (w - ee) * eps, eps * (ee * (1 + eps) - w)]
    else:
        l, d1, d2, masks = row_terms(code, L(case["p"]), X @ coef, y, w)
        if case["branches"]:    # a condition on the inputs: every branch of the loss holds at least one row
            assert all(m.any() for m in masks), (code, [int(m.sum()) for m in masks])
        gc, hc, ws = w * d1, w * d2, w.sum()
    eps_c = [max(4 * rel_err(t.numpy(), want), 2.0 ** -50) for t, want in zip(torch_coefs(case), (l, gc, hc))]
    rnd = (n + 4) * U
    g, gs = X.T @ gc, np.abs(X).T @ np.abs(gc)
    H, Hs = (X * hc[:, None]).T @ X, (np.abs(X) * np.abs(hc)[:, None]).T @ np.abs(X)
    gb, Hb = (rnd + eps_c[1]) * gs, (rnd + eps_c[2]) * Hs
    if tail:        # the row and column of log sigma: the corner sums, every other entry zero
        g, H = np.append(g, tail[0].sum()), np.pad(H, (0, 1))
        H[k, k] = tail[1].sum()
        # The corner terms are products of at most three factors out of eps, exp(eps), 1 + eps.  exp(eps) has the
        # relative error e of the Hessian coefficient, so eps the absolute error e: a term moves by at most 4 e times
        # its majorant with |eps| -> 1 + |eps|.
        ae, e4 = 1 + np.abs(eps), rnd + 4 * eps_c[2]
        gb, Hb = np.append(gb, e4 * (np.abs(w) + (np.abs(w) + ee) * ae).sum()), np.pad(Hb, (0, 1))
        Hb[k, k] = e4 * (ae * (ee * (1 + ae) + np.abs(w))).sum()
    return {"H": H, "g": g, "ws": ws, "loss": l.sum(), "H_bound": Hb, "g_bound": gb, "ws_bound": rnd * np.abs(ws),
            "loss_bound": (rnd + eps_c[0]) * np.abs(l).sum(), "eps": eps_c, "zero_hessian": not hc.any()}


def softmax_case(n, m, k1, seed):
    """Seeded X [n, m], W [k1, m], labels 0 .. k1 (the pivot included) and weights, every fifth 0."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 2.0, n)
    w[::5] = 0.0
    return {"X": rng.normal(size=(n, m)), "W": rng.normal(size=(k1, m)) / np.sqrt(m),
            "y": (np.arange(n) % (k1 + 1)).astype(float), "w": w}


def softmax_oracle(case):
    """H, G and the sums of SoftmaxObjFunc in longdouble.  H: the unary bound with c = w (delta phi_s - phi_s phi_t),
    eps_c from the torch phi on the CPU.  G and the loss: the rule of tests/test_softmax_fused_gpu.py, the larger of
    4 x the error of the torch chain on the CPU and (n + 4) 2^-53 sum |term|."""
    X, W, y, w = (case[key].astype(L) for key in ("X", "W", "y", "w"))
    (n, m), k1, yi = X.shape, W.shape[0], case["y"].astype(int)
    full = np.concatenate([X @ W.T, np.zeros((n, 1), L)], 1)
    mx = full.max(1)
    lse = mx + np.log(np.exp(full - mx[:, None]).sum(1))
    phi, loss = np.exp(full[:, :k1] - lse[:, None]), lse - full[np.arange(n), yi]
    R = (phi - np.eye(k1 + 1, dtype=L)[yi][:, :k1]) * w[:, None]
    dg = (phi - phi * phi) * w[:, None]                             # the coefficients of the diagonal blocks
    Z, Za, rnd = (phi[:, :, None] * X[:, None, :]).reshape(n, -1), \
        (phi[:, :, None] * np.abs(X)[:, None, :]).reshape(n, -1), (n + 4) * U
    H, Hs = -(Z * w[:, None]).T @ Z, (Za * w[:, None]).T @ Za
    for s in range(k1):
        sl = slice(s * m, (s + 1) * m)
        H[sl, sl], Hs[sl, sl] = (X * dg[:, s, None]).T @ X, (np.abs(X) * np.abs(dg[:, s, None])).T @ np.abs(X)
    obj, t = O.SoftmaxObjFunc(k1 + 1), {key: torch.from_numpy(case[key]) for key in case}
    data, coef = O.LabeledData(FeatureMatrix(t["X"]), t["y"], t["w"]), t["W"].reshape(-1)
    tp = obj._phi(obj._eta(data, coef))
    off = (-tp[:, :, None] * tp[:, None, :] * t["w"][:, None, None]).numpy()
    off[:, np.arange(k1), np.arange(k1)] = ((tp - tp ** 2) * t["w"][:, None]).numpy()
    want = -phi[:, :, None] * phi[:, None, :] * w[:, None, None]
    want[:, np.arange(k1), np.arange(k1)] = dg
    eps = max(4 * rel_err(off, want), 2.0 ** -50)
    G, ls = R.T @ X, loss.sum()
    Gt, lt = obj.grad_sum(data, coef).numpy().reshape(k1, m).astype(L), L(float(obj.loss_per_sample(data, coef).sum()))
    return {"H": H, "g": G, "ws": w.sum(), "loss": ls, "H_bound": (rnd + eps) * Hs, "ws_bound": rnd * w.sum(),
            "g_bound": np.maximum(4 * np.abs(Gt - G), rnd * (np.abs(R).T @ np.abs(X))),
            "loss_bound": max(4 * abs(lt - ls), rnd * np.abs(loss).sum()), "eps": eps, "zero_hessian": False}
