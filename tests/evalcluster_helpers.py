"""Shared by ``test_evalcluster_device.py`` (CPU) and ``test_evalcluster_gpu.py``: seeded rows and clusterings, the
fp64 numpy reference of the row pass with its rounding bounds, the reference formulas of the operator's metrics, and
the operator call.

Bounds (u = 2^-53; one evaluation's first-order error, a comparison of two evaluations gets twice that, and the
tests allow 4x the result, the project's margin):

* a dot of m terms: ``m u sum|x_j m_j|`` (so two evaluations differ by at most ``2 m u sum|x_j m_j|``); m is d for
  dense rows and the row's entry count for CSR rows (absent terms add exactly 0);
* the direct EUCLIDEAN / CITYBLOCK ``own`` of dense rows: two evaluations differ by at most ``(m + 4) u`` relative
  (3 roundings per squared term, m - 1 additions of nonnegative terms, the root halves and adds one);
* COSINE ``own = 1 - q``, ``q = x.m / (|x| |m|)``: the dot's bound over the cross, plus ``(T + 5) u |q|`` for the
  two norms, their product and the quotient (T = the larger term count of the two norms), plus ``u |own|``;
* the CSR rearranged forms: ``own^2 = |m|^2 + sum_nz((x - m)^2 - m^2)`` has an absolute error of at most
  ``T u (|x|^2 + |m|^2)`` with the term count ``T = s + 8 nz + 8`` (s = the stored-nonzero count of the mean behind
  ``|m|^2``, every entry's term is at most ``3 (x_j^2 + m_j^2)`` after 4 roundings, and the running sum stays below
  ``4 (|x|^2 + |m|^2)``); ``own`` then moves by at most that over ``own``.  CITYBLOCK is the same with the 1-norms:
  ``T u (|x|_1 + |m|_1)``;
* the silhouette follows from the ``dis`` bound: EUCLIDEAN ``dis_j = cnt_j |x|^2 - 2 cnt_j x.m_j + n2_j`` errs by at
  most ``u (cnt_j |x|^2 (m + 5) + 2 cnt_j (m + 4) sum|x m_j| + 3 n2_j)``, otherwise ``dis_j = 1 - x.m_j`` by
  ``u (m sum|x m_j| + 1 + |dis_j|)``; ``cur`` and the neighbour candidates inherit it through their divisions (one
  more ``u`` relative for ``cur``, two for a candidate, which the kernels multiply by a rounded ``1 / cnt_j``), the
  minimum moves by at most the largest candidate error, and
  ``sil(cur, nb)`` has slope at most ``1 / max(cur, nb)`` in either argument: ``|d sil| <= E / (M - E) + 4 u`` with
  ``E`` the two errors added and ``M = max(cur, nb)``.

So that no bound is vacuous the generators only keep rows (outside one-row clusters, whose ``own`` is 0) with
``own^2 >= 1e-3 (|x|^2 + |m|^2)``, for CITYBLOCK also ``own >= 1e-3 (|x|_1 + |m|_1)``, and ``E <= M / 2``; rows
that miss are drawn again, and ``reference`` asserts all three.  The one exception is COSINE at d = 1, where ``own``
is 0, 1 or 2 whatever the rows are; its bound is absolute in ``|q| <= 1`` and not vacuous there either.
"""
import functools

import numpy as np
import torch

EPS = 2.0 ** -53
N = 257
NCOLS = 2 ** 18
DISTS = ("EUCLIDEAN", "COSINE", "CITYBLOCK")
ROW_LENS = (0, 1, 2, 5, 63, 64, 65, 130)


class Ref:
    """own / sil fp64 [n] with the absolute tolerances tol_own / tol_sil (already 4x the bound); ``ok`` = the rows
    whose cid is inside [0, k) (the others expect zeros); own2 / tol_own2 for the rearranged EUCLIDEAN form."""


def _sums(X, cid, k):
    ok = (cid >= 0) & (cid < k)
    cnt = np.bincount(cid[ok], minlength=k).astype(np.float64)
    s = np.zeros((k, X.shape[1]))
    np.add.at(s, cid[ok], X[ok])
    n2 = np.zeros(k)
    np.add.at(n2, cid[ok], (X[ok] ** 2).sum(1))
    return s / np.maximum(cnt, 1.0)[:, None], cnt, n2


def reference(X, cid, mean, cnt, n2, dist, terms=None, rearranged=False, check=True):
    """The row pass in fp64 numpy for the dense rows ``X`` [n, D] (CSR rows: their narrow dense copy, with ``terms``
    = the entry count per row and ``rearranged`` = the kernel's own-distance forms).  With ``check`` the input
    properties of the module docstring are asserted; ``bad`` lists the rows that miss them either way."""
    n, D = X.shape
    k = len(cnt)
    u = EPS
    ok = (cid >= 0) & (cid < k)
    cs = np.where(ok, cid, 0)
    m = np.full(n, float(D)) if terms is None else np.maximum(np.asarray(terms, dtype=np.float64), 1.0)
    dot = X @ mean.T
    S = np.abs(X) @ np.abs(mean).T
    xn = (X * X).sum(1)
    mo = mean[cs]
    m2 = (mo * mo).sum(1)
    sm = np.maximum((mean != 0).sum(1)[cs].astype(np.float64), 1.0)
    cn = cnt[cs]
    rows = np.arange(n)
    r = Ref()
    r.ok = ok
    single = cn <= 1
    x1, mo1 = np.abs(X).sum(1), np.abs(mo).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        if dist == "EUCLIDEAN":
            own = np.sqrt(((X - mo) ** 2).sum(1))
            if rearranged:
                eq = (sm + 8 * m + 8) * u * (xn + m2)
                r.own2, r.tol_own2 = own * own, 4 * 2 * (eq + 2 * u * own * own)
                b_own = np.where(own > 0, eq / own + u * own, np.sqrt(2 * eq))
            else:
                b_own = 0.5 * (m + 4) * u * own
        elif dist == "CITYBLOCK":
            own = np.abs(X - mo).sum(1)
            b_own = (sm + 8 * m + 8) * u * (x1 + mo1) if rearranged else 0.5 * (m + 4) * u * own
        else:
            cross = np.sqrt(xn) * np.sqrt(m2)
            q = np.where(cross > 0, dot[rows, cs] / np.where(cross > 0, cross, 1.0), 0.0)
            own = 1.0 - q
            T = np.maximum(m, sm)
            b_own = np.where(cross > 0, m * u * S[rows, cs] / np.where(cross > 0, cross, 1.0), 0.0) \
                + (T + 5) * u * np.abs(q) + u * np.abs(own)
        r.own, r.tol_own = own, 4 * 2 * b_own
        if dist == "EUCLIDEAN":
            dis = cnt[None, :] * xn[:, None] - 2 * cnt[None, :] * dot + n2[None, :]
            e_dis = u * (cnt[None, :] * xn[:, None] * (m[:, None] + 5) + 2 * cnt[None, :] * (m[:, None] + 4) * S
                         + 3 * n2[None, :])
            div = np.maximum(cnt, 1.0)[None, :]
            nbv, e_nbv = dis / div, e_dis / div + 2 * u * np.abs(dis / div)     # a division, or a rounded reciprocal
            cur = np.where(cn > 1, dis[rows, cs] / np.maximum(cn - 1, 1.0), 0.0)
            e_cur = np.where(cn > 1, e_dis[rows, cs] / np.maximum(cn - 1, 1.0) + u * np.abs(cur), 0.0)
        else:
            dis = 1.0 - dot
            e_dis = u * (m[:, None] * S + 1 + np.abs(dis))
            nbv, e_nbv = dis, e_dis
            f = cn / np.where(cn > 1, cn - 1, 1.0)
            cur = np.where(cn > 1, dis[rows, cs] * f, 0.0)
            e_cur = np.where(cn > 1, (e_dis[rows, cs] + 2 * u * np.abs(dis[rows, cs])) * f, 0.0)
        if k > 1:
            nbv, e_nbv = nbv.copy(), e_nbv.copy()
            nbv[rows, cs] = np.inf
            e_nbv[rows, cs] = 0.0
            nb, e_nb = nbv.min(1), e_nbv.max(1)
        else:
            nb, e_nb = np.full(n, np.inf), np.zeros(n)
        sil = np.where(cur < nb, 1 - cur / nb, nb / cur - 1)
        sil = np.where(np.isnan(sil), 0.0, sil)
        E, M = 2 * (e_cur + e_nb), np.maximum(cur, nb)
        r.sil = sil
        r.tol_sil = 4 * (np.where(np.isinf(M), 0.0, E / np.where(M - E > 0, M - E, np.nan)) + 4 * u)
    # the input properties (of the reference alone)
    bad = ok & ~(E <= 0.5 * M)
    if not (dist == "COSINE" and D == 1):       # a COSINE own at d = 1 is 0, 1 or 2 whatever the rows are
        bad |= ok & ~single & ~(own * own >= 1e-3 * (xn + m2))
    if dist == "CITYBLOCK":
        bad |= ok & ~single & ~(own >= 1e-3 * (x1 + mo1))
    r.bad = np.flatnonzero(bad)
    if check:
        assert len(r.bad) == 0, (dist, r.bad[:10])
        assert np.isfinite(r.tol_sil[ok]).all() and np.isfinite(r.tol_own[ok]).all()
    return r


def clusters(n, k, rng):
    """cids of n rows over k clusters: every cluster has a row, cluster k - 1 (k > 1) has exactly one, and three rows
    lie outside [0, k): -1, k and k + 5."""
    cid = rng.permutation(np.arange(n) % k).astype(np.int64)
    if k > 1:
        last = np.flatnonzero(cid == k - 1)
        cid[last[1:]] = 0
    for v in (-1, k, k + 5):        # each taken from the cluster that is the largest at that moment
        inside = (cid >= 0) & (cid < k)
        big = int(np.bincount(cid[inside], minlength=k).argmax())
        cid[np.flatnonzero(cid == big)[0]] = v
    assert len(set(cid[(cid >= 0) & (cid < k)])) == k and (k == 1 or (cid == k - 1).sum() == 1)
    return cid


def _settle(draw, X, cid, k, dist, terms=None, rearranged=False):
    """Rows that miss the input properties are drawn again (``draw(i)``) until none does."""
    for _ in range(200):
        mean, cnt, n2 = _sums(X, cid, k)
        ref = reference(X, cid, mean, cnt, n2, dist, terms, rearranged, check=False)
        if len(ref.bad) == 0:
            return mean, cnt, n2
        for i in ref.bad:
            X[i] = draw(i)
    raise AssertionError(("no well-conditioned rows", dist, k))


@functools.lru_cache(maxsize=None)
def dense_case(d, k, dist, n=N):
    """(X [n, d], cid [n], mean, cnt, n2, reference): seeded normal rows (for the non-Euclidean types scaled to
    norms in (0.2, 0.9): inside the unit ball like the operator's unit rows, so every ``1 - x.m`` stays above 0.19)
    with the clustering of ``clusters`` and the cluster sums of exactly these rows."""
    rng = np.random.default_rng(1000 * d + k)
    unit = dist != "EUCLIDEAN"

    def draw(i):
        x = rng.normal(size=d)
        return x / np.linalg.norm(x) * rng.uniform(0.2, 0.9) if unit else x
    X = np.stack([draw(i) for i in range(n)])
    cid = clusters(n, k, rng)
    mean, cnt, n2 = _settle(draw, X, cid, k, dist)
    return X, cid, mean, cnt, n2, reference(X, cid, mean, cnt, n2, dist)


@functools.lru_cache(maxsize=None)
def csr_case(k, dist, n=None, ncols=NCOLS, pool=400):
    """n = max(257, 2 k + 40) (no cluster is empty) CSR rows of the lengths ``ROW_LENS`` (in turn) over ``pool`` columns spread over [0, ncols), first and last
    included, stored in random order, every fifth row with three more entries outside [0, ncols) that must not
    count.  Returns (crow, col, val, cid, cols = the pool, Xn = the narrow dense copy [n, pool], mean_n [k, pool], cnt,
    n2, reference)."""
    rng = np.random.default_rng(77 + k)
    n = n or max(N, 2 * k + 40)
    cols = np.unique(np.concatenate([[0, ncols - 1], rng.integers(0, ncols, size=pool - 2)]))
    P = len(cols)
    unit = dist != "EUCLIDEAN"
    lens = [ROW_LENS[i % len(ROW_LENS)] for i in range(n)]
    cid = clusters(n, k, rng)
    for c in range(k):      # two stored rows per cluster (one in a one-row cluster): a cluster of empty rows has the
        mine = np.flatnonzero(cid == c)     # mean 0, and a single stored row is parallel to its cluster's mean
        for i in mine[:2]:
            if sum(lens[j] > 0 for j in mine) < min(2, len(mine)) and lens[i] == 0:
                lens[i] = 5

    def draw(i):
        x = np.zeros(P)
        pos = rng.choice(P, size=lens[i], replace=False)
        x[pos] = rng.normal(size=lens[i]) + np.sign(rng.normal(size=lens[i])) * 0.25      # no stored zero
        return x / np.linalg.norm(x) * rng.uniform(0.2, 0.9) if unit and lens[i] else x
    Xn = np.stack([draw(i) for i in range(n)])
    terms = np.array(lens, dtype=np.float64)
    mean, cnt, n2 = _settle(draw, Xn, cid, k, dist, terms, True)
    crow, col, val = [0], [], []
    for i in range(n):
        pos = np.flatnonzero(Xn[i])
        pos = pos[rng.permutation(len(pos))]
        c, v = cols[pos], Xn[i, pos]
        if i % 5 == 0:      # entries outside [0, ncols): ignored by the dots and the norms alike
            c = np.concatenate([c, [-1, ncols, ncols + 7]])
            v = np.concatenate([v, [3.0, -2.0, 5.0]])
            q = rng.permutation(len(c))
            c, v = c[q], v[q]
        col.append(c)
        val.append(v)
        crow.append(crow[-1] + len(c))
    return (np.array(crow, dtype=np.int64), np.concatenate(col).astype(np.int64), np.concatenate(val), cid, cols, Xn,
            mean, cnt, n2, reference(Xn, cid, mean, cnt, n2, dist, terms, True))


def check_block(block, ref, rearranged_euclid=False):
    """Asserts an [n, 3] block (numpy) against ``ref``; prints the largest error / tolerance ratios first."""
    ok = ref.ok
    assert np.array_equal(block[~ok], np.zeros(((~ok).sum(), 3))), "rows outside [0, k) must be zero"
    own, sil = block[ok, 0], block[ok, 2]
    with np.errstate(divide="ignore", invalid="ignore"):        # 0 / 0 where both the error and the bound are 0
        ro = np.abs(own - ref.own[ok]) / ref.tol_own[ok]
        rs = np.abs(sil - ref.sil[ok]) / ref.tol_sil[ok]
    print("own err/tol", np.nanmax(ro), "sil err/tol", np.nanmax(rs))
    assert np.all(np.abs(own - ref.own[ok]) <= ref.tol_own[ok])
    assert np.all(np.abs(sil - ref.sil[ok]) <= ref.tol_sil[ok])
    if rearranged_euclid:
        assert np.all(np.abs(block[ok, 1] - ref.own2[ok]) <= ref.tol_own2[ok])
    else:
        assert np.array_equal(block[ok, 1], own * own)


# ---------------------------------------------------------------------------------------------------- operator

def ref_cluster_metrics(X, cid, dist):
    """The reference ClusterEvaluationUtil / ClusterMetricsSummary formulas, written out in numpy."""
    ks = sorted(set(cid))
    if dist != "EUCLIDEAN":
        X = X / np.linalg.norm(X, axis=1, keepdims=True)

    def d(a, b):
        if dist == "COSINE":
            return 1.0 - a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
        if dist == "CITYBLOCK":
            return np.abs(a - b).sum()
        return np.linalg.norm(a - b)
    mean = {k: X[cid == k].mean(0) for k in ks}
    cnt = {k: int((cid == k).sum()) for k in ks}
    dsum = {k: sum(d(mean[k], x) for x in X[cid == k]) for k in ks}
    d2 = {k: sum(d(mean[k], x) ** 2 for x in X[cid == k]) for k in ks}
    n2 = {k: float((X[cid == k] ** 2).sum()) for k in ks}
    gmean = sum(mean[k] * cnt[k] for k in ks) / len(X)
    ssb = sum(d(mean[k], gmean) ** 2 * cnt[k] for k in ks)
    ssw = sum(d2.values())
    comp = {k: dsum[k] / cnt[k] for k in ks}
    sil = 0.0
    for x, c in zip(X, cid):
        cur, nb = 0.0, np.inf
        for k in ks:
            if dist == "EUCLIDEAN":
                dis = cnt[k] * (x @ x) - 2 * cnt[k] * (x @ mean[k]) + n2[k]
                if k == c:
                    cur = dis / (cnt[k] - 1) if cnt[k] > 1 else 0.0
                else:
                    nb = min(nb, dis / cnt[k])
            else:
                dis = 1.0 - x @ mean[k]
                if k == c:
                    cur = dis * cnt[k] / (cnt[k] - 1) if cnt[k] > 1 else 0.0
                else:
                    nb = min(nb, dis)
        sil += 1 - cur / nb if cur < nb else nb / cur - 1
    return {"Ssb": ssb, "Ssw": ssw, "Compactness": sum(comp.values()) / len(ks),
            "SilhouetteCoefficient": sil / len(X)}


def separated(n=600, d=3, k=3):
    """The fixture of ``test_evaluation.py`` (positive noise plus 3 on the cluster's own axis) at n rows, d dims."""
    rng = np.random.default_rng(4)
    cid = np.repeat(np.arange(k), n // k)
    X = np.abs(rng.normal(size=(n, d)))
    X[np.arange(n), cid] += 3.0
    return X, cid


def sparse_docs(n=300, ncols=NCOLS, per_row=20, k=4, pool=600):
    """(crow, col, val, cid, cols): n documents of about ``per_row`` entries over ``pool`` columns of [0, ncols)."""
    rng = np.random.default_rng(9)
    cols = np.unique(np.concatenate([[0, ncols - 1], rng.integers(0, ncols, size=pool - 2)]))
    cid = np.arange(n) % k
    crow, col, val = [0], [], []
    for i in range(n):
        m = int(rng.integers(per_row - 4, per_row + 5))
        # a cluster prefers its own quarter of the pool, so the clustering is not arbitrary
        lo = (cid[i] * len(cols)) // (2 * k)
        pos = np.unique(np.concatenate([rng.integers(lo, lo + len(cols) // 2, size=m - 4),
                                        rng.integers(0, len(cols), size=4)]))
        col.append(cols[pos])
        val.append(rng.integers(1, 6, size=len(pos)).astype(np.float64))
        crow.append(crow[-1] + len(pos))
    return np.array(crow, dtype=np.int64), np.concatenate(col), np.concatenate(val), cid, cols


def sparse_table(crow, col, val, size, pred, device="cpu", label=None):
    from alink_amd.common.linalg.block import SparseBlock
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    blk = SparseBlock(torch.from_numpy(crow), torch.from_numpy(np.asarray(col, dtype=np.int64)),
                      torch.from_numpy(val), int(size)).to(device)
    names, types, colsl = ["v", "p"], [Types.SPARSE_VECTOR, Types.LONG], [Column(blk), Column(torch.from_numpy(pred))]
    if label is not None:
        names, types, colsl = names + ["l"], types + [Types.LONG], colsl + [Column(torch.from_numpy(label))]
    return MTable(TableSchema(names, types), colsl)


def dense_table(X, pred, device="cpu"):
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    return MTable(TableSchema(["v", "p"], [Types.DENSE_VECTOR, Types.LONG]),
                  [Column(torch.from_numpy(X).to(device)), Column(torch.from_numpy(pred).to(device))])


def evaluate(mt, dist, device="cpu", label=False):
    """The ``Params`` dict of ``EvalClusterBatchOp`` on the table ``mt`` (columns v, p and, with ``label``, l)."""
    import json
    from alink_amd import EvalClusterBatchOp, useLocalEnv
    from alink_amd.operator.batch.source import TableSourceBatchOp
    useLocalEnv(1, device=device)
    op = EvalClusterBatchOp().setVectorCol("v").setPredictionCol("p").setDistanceType(dist)
    if label:
        op = op.setLabelCol("l")
    return json.loads(op.linkFrom(TableSourceBatchOp(mt)).collect()[0][0])


def assert_metrics_equal(got, want):
    """Every numeric metric within the operator's own figures (rel 1e-9, abs 1e-12); counts, k and the cluster
    array exactly."""
    import pytest
    assert set(got) == set(want)
    for key, w in want.items():
        if key in ("k", "count", "clusterArray", "countArray"):
            assert got[key] == w, key
        else:
            assert float(got[key]) == pytest.approx(float(w), rel=1e-9, abs=1e-12, nan_ok=True), (key, got[key], w)
