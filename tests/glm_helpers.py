"""The numpy ``longdouble`` oracle of the GLM formulas (``models/regression/glm.py``) and one small case builder, shared
by ``test_glm_device.py`` and ``test_glm_gpu.py``."""
import numpy as np

L = np.longdouble
EPS, DELTA = L(np.float64(1e-16)), L(np.float64(0.1))
JMAX, JMIN = L(np.float64(1.7976931348623157e308)), L(np.float64(4.9e-324))
FAMILIES = ("gaussian", "binomial", "poisson", "gamma", "tweedie")
LINKS = ("identity", "log", "logit", "inverse", "sqrt", "cloglog", "power")
VP, LP = 1.5, -0.5          # tweedie's variance power and the power link's exponent (tweedie's default link)
PAIRS = [(f, l) for f in FAMILIES for l in LINKS]
# intercepts that put mu = unlink(x . beta + b0 + off) inside (0.2, 0.85) for X in [0.1, 1], beta = 0.15, off <= 0.05:
# inside every link's domain and a valid mean for every family
INTERCEPT = {"identity": 0.2, "log": -1.5, "logit": -0.3, "inverse": 1.5, "sqrt": 0.4, "cloglog": -1.5, "power": 1.2}


def link(name, mu):
    return {"identity": lambda: mu, "log": lambda: np.log(mu), "logit": lambda: np.log(mu / (1 - mu)),
            "inverse": lambda: 1 / mu, "sqrt": lambda: np.sqrt(mu), "cloglog": lambda: np.log(-np.log(1 - mu)),
            "power": lambda: np.power(mu, L(LP))}[name]()


def unlink(name, eta):
    return {"identity": lambda: eta, "log": lambda: np.exp(eta), "logit": lambda: 1 / (1 + np.exp(-eta)),
            "inverse": lambda: 1 / eta, "sqrt": lambda: eta * eta, "cloglog": lambda: 1 - np.exp(-np.exp(eta)),
            "power": lambda: np.power(eta, 1 / L(LP))}[name]()


def deriv(name, mu):
    return {"identity": lambda: np.ones_like(mu), "log": lambda: 1 / mu, "logit": lambda: 1 / (mu * (1 - mu)),
            "inverse": lambda: -1 / (mu * mu), "sqrt": lambda: 1 / (2 * np.sqrt(mu)),
            "cloglog": lambda: 1 / ((mu - 1) * np.log(1 - mu)),
            "power": lambda: L(LP) * np.power(mu, L(LP) - 1)}[name]()


def project(fam, mu):
    if fam == "gaussian":
        return np.where(mu == -np.inf, JMIN, np.where(mu == np.inf, JMAX, mu))
    if fam == "binomial":
        return np.where(mu < EPS, EPS, np.where(mu > 1 - EPS, 1 - EPS, mu))
    mu = np.where(mu < EPS, EPS, mu)
    return np.where(np.isinf(mu), JMAX, mu)


def variance(fam, mu):
    return {"gaussian": lambda: np.ones_like(mu), "binomial": lambda: mu * (1 - mu), "poisson": lambda: mu,
            "gamma": lambda: mu * mu, "tweedie": lambda: np.power(mu, L(VP))}[fam]()


def initialize(fam, y, w):
    return {"gaussian": lambda: y, "gamma": lambda: y, "binomial": lambda: (w * y + L(0.5)) / (w + 1),
            "poisson": lambda: np.where(y < DELTA, DELTA, y), "tweedie": lambda: np.where(y == 0, DELTA, y)}[fam]()


def deviance(fam, y, mu, w):
    def ylogy(a, b):
        return np.where(a == 0, L(0), a * np.log(np.where(a == 0, L(1), a) / b))
    if fam == "gaussian":
        return w * (y - mu) * (y - mu)
    if fam == "binomial":
        return 2 * w * (ylogy(y, mu) + ylogy(1 - y, 1 - mu))
    if fam == "poisson":
        return 2 * w * (ylogy(y, mu) - (y - mu))
    if fam == "gamma":
        return -2 * w * (np.log(y / mu) - (y - mu) / mu)
    y1 = np.where(y == 0, L(1), y)
    p1, p2 = 1 - L(VP), 2 - L(VP)
    d = 2 * w * (y * (np.power(y1, p1) - np.power(mu, p1)) / p1 - (np.power(y, p2) - np.power(mu, p2)) / p2)
    return np.where(d < EPS, EPS, d)


def oracle(case, fam, lnk, mode, cnull=0.0):
    """Every row output and the four sums of one (family, link) in longdouble; ``mode`` "init" or "step"."""
    X, y, w, off, beta = (case[key].astype(L) for key in ("X", "y", "w", "off", "beta"))
    with np.errstate(all="ignore"):
        eta = X @ beta + L(case["intercept"]) + off
        mu = project(fam, unlink(lnk, eta))
        g = deriv(lnk, mu)
        dev = deviance(fam, y, mu, w)
        pr = (y - mu) * np.sqrt(w) / np.sqrt(variance(fam, mu))
        dr = np.sqrt(np.maximum(dev, 0))
        if mode == "init":
            z, ww = link(lnk, project(fam, initialize(fam, y, w))) - off, w
        else:
            z, ww = eta - off + (y - mu) * g, w / (g * g * variance(fam, mu))
        null = deviance(fam, y, unlink(lnk, L(cnull) + off), w)
    return {"eta": eta, "pred": mu, "z": z, "ww": ww, "dres": np.where(y <= mu, -dr, dr), "pres": pr,
            "wres": (y - mu) * g, "rres": y - mu,
            "sums": np.array([dev.sum(), null.sum(), (pr * pr).sum(), w.sum()], dtype=L)}


def make_case(fam, lnk, n, k, seed=0, beta=None):
    """fp64 numpy inputs: X uniform in [0.1, 1], positive beta, the link's intercept, y drawn from the family."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.1, 1.0, size=(n, k))
    beta = np.full(k, 0.45 / k) * (1 + 0.1 * (np.arange(k) % 3 - 1)) if beta is None else beta
    off = rng.uniform(0.0, 0.05, size=n)
    w = rng.uniform(0.5, 2.0, size=n)
    b0 = INTERCEPT[lnk]
    mu = np.asarray(unlink(lnk, (X @ beta + b0 + off).astype(L)), dtype=np.float64)
    if fam == "gaussian":
        y = mu + 0.03 * rng.normal(size=n)
    elif fam == "binomial":
        y = (rng.random(n) < mu).astype(np.float64)
    elif fam == "poisson":
        y = rng.poisson(mu).astype(np.float64)
    else:
        y = mu * rng.gamma(2.0, 0.5, size=n)
        if fam == "tweedie":
            y[rng.random(n) < 0.3] = 0.0
    return {"X": X, "y": y, "w": w, "off": off, "beta": beta, "intercept": b0}


def rel_err(got, ref):
    """Largest elementwise relative error of ``got`` (fp64) against ``ref`` (longdouble) over the finite entries of
    ``ref``; where ``ref`` is not finite ``got`` must be the same inf or a NaN too."""
    got, ref = np.asarray(got, dtype=L).reshape(-1), np.asarray(ref, dtype=L).reshape(-1)
    fin = np.isfinite(ref)
    bad = np.asarray(ref[~fin], dtype=np.float64)
    np.testing.assert_array_equal(np.asarray(got[~fin], dtype=np.float64), bad)
    if not fin.any():
        return 0.0
    den = np.where(ref[fin] == 0, L(1), np.abs(ref[fin]))
    return float(np.max(np.abs(got[fin] - ref[fin]) / den))
