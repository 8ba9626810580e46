"""The LSH kernels (``ops/csrc/lsh.hip`` through ``ops/lsh.py``) and the two similarity operators on the GPU.  The
oracle is always the host path of ``models/similarity/lsh.py``, run on the CPU.

Hashes and Jaccard distances are compared exactly.  Euclidean tolerance (derived, not tuned): each term
``(a - b)^2`` carries at most 3 roundings, ``m`` nonnegative terms add at most ``m - 1`` more, the square root halves
the relative error and adds one rounding, so two such evaluations differ by at most ``(m + 4) 2^-53`` relative, with
``m`` the size of the union of the two rows' entries (CSR) or ``d`` (dense); the tests allow 4x that, the rule of
``test_bisecting_gpu.py``.  A projection of ``d`` terms is bounded as there: ``2 d 2^-53 sum|x_j r_j|``.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lsh_helpers as H  # noqa: E402
from lsh_helpers import EPS, NCOLS, ROW_LENS  # noqa: E402

from alink_amd.models.similarity import lsh as L  # noqa: E402
from alink_amd.ops import lsh as K  # noqa: E402

pytestmark = pytest.mark.gpu

DS = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 128, 131, 300, 1024)
GRIDS = (0, 1, 7)


def _cuda_rows(rows, ncols=NCOLS):
    """CsrRows on the GPU of (indices, values) rows as they are (zeros kept, nothing sorted)."""
    fm = H.csr(rows, ncols, "cuda")
    return K.CsrRows(fm.crow, fm.col, fm.val, ncols)


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).cuda()


# ---------------------------------------------------------------------------------------------------- MinHash

@pytest.mark.parametrize("P,T", [(1, 1), (2, 3), (3, 4), (7, 10)])
def test_minhash_tables_equal_the_host_hash(P, T):
    rng = np.random.default_rng(P * 31 + T)
    top = 2 ** 31 - 1
    rows = []
    for i in range(257):
        idx = H.sparse_row(rng, ROW_LENS[i % len(ROW_LENS)], hi=top)
        if len(idx) >= 2:
            idx[-1] = top - 1                       # the largest index the 32-bit arithmetic takes
        val = rng.integers(1, 5, size=len(idx)).astype(np.float64)
        val[rng.random(len(idx)) < 0.2] = 0.0       # explicit zeros: not hashed
        rows.append((idx, val))
    rows[3] = (rows[3][0], np.zeros(len(rows[3][0])))       # a row of zeros only hashes as an empty one
    lsh = L.MinHashLSH(11, P, T)
    host = L._Rows([H.SparseVector(top, i.astype(np.int32), v) for i, v in rows])
    assert host.idx.size < sum(len(i) for i, _ in rows) and int(host.idx.max()) == top - 1
    want = lsh.hash(host)
    assert (want < 0).any() and (want > 0).any()
    dev = _cuda_rows(rows, top)
    calls = K.LSH_CALLS
    got = K.minhash_tables(dev, lsh.A, lsh.B)
    assert K.LSH_CALLS == calls + 1
    assert got.dtype == torch.int32 and tuple(got.shape) == (257, T)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    assert np.array_equal(want[3], want[0])         # row 0 is empty
    for grid in (1, 7):
        assert torch.equal(K.minhash_tables(dev, lsh.A, lsh.B, grid=grid), got)


def test_minhash_of_empty_rows_launches_nothing():
    lsh = L.MinHashLSH(11, 2, 3)
    empty = [(np.zeros(0, dtype=np.int64), np.zeros(0))] * 5
    calls = K.LSH_CALLS
    got = K.minhash_tables(_cuda_rows(empty), lsh.A, lsh.B)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), lsh.hash(L._Rows(H.vectors(empty))))
    assert tuple(K.minhash_tables(_cuda_rows([]), lsh.A, lsh.B).shape) == (0, 3)
    assert K.LSH_CALLS == calls


# ---------------------------------------------------------------------------------------------------- BRP hash

@pytest.mark.parametrize("P,T", [(1, 1), (2, 3), (7, 10)])
def test_brp_tables_equal_numpy(P, T):
    rng = np.random.default_rng(P + T)
    n, F, w = 300, P * T, 0.5
    r = rng.integers(0, 4, size=F) / 8.0            # offsets in [0, w), multiples of 1/8
    dots = rng.normal(size=(n, F)) * 50.0           # negative values included
    k = rng.integers(-1000, 1000, size=(n // 2, F))
    dots[: n // 2] = k * w - r                      # dot + r is an exact multiple of w
    dots[0] = (2.0 ** 31 - 3) * w                   # the ends of the int32 range
    dots[1] = -(2.0 ** 31 - 3) * w
    q = np.floor((dots + r) / w)
    assert np.abs(q).max() < 2 ** 31 and (q < 0).any() and np.array_equal(q[2: n // 2], k[2:].astype(np.float64))
    hv = q.astype(np.int64).reshape(n, T, P)
    want = np.stack([L.murmur3_32_words(hv[:, t, :]) for t in range(T)], 1)
    calls = K.LSH_CALLS
    got = K.brp_tables(torch.from_numpy(dots).cuda(), r, w, T)
    assert K.LSH_CALLS == calls + 1 and got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    for grid in (1, 7):
        assert torch.equal(K.brp_tables(torch.from_numpy(dots).cuda(), r, w, T, grid=grid), got)


# ---------------------------------------------------------------------------------------------------- pairs

def _pair_cases():
    """(a rows, b rows) as (indices, values): pair i is (a[i], b[i]).  Every combination of ``ROW_LENS`` on both
    sides with a random overlap, then identical rows, disjoint rows, and one common entry at the first or last
    position of either row."""
    rng = np.random.default_rng(3)
    val = lambda k: rng.normal(size=k) + np.where(rng.random(k) < 0.5, -3.0, 3.0)       # noqa: E731  never zero
    a, b = [], []
    for la in ROW_LENS:
        for lb in ROW_LENS:
            pool = rng.choice(NCOLS, size=la + lb, replace=False).astype(np.int64)
            k = int(rng.integers(0, min(la, lb) + 1))
            ia, ib = np.sort(pool[:la]), np.sort(np.concatenate([pool[:k], pool[la:la + lb - k]]))
            a.append((ia, val(la)))
            b.append((ib, val(lb)))
    for la in ROW_LENS:                             # identical rows (empty against empty among them)
        ia = H.sparse_row(rng, la)
        va = val(la)
        a.append((ia, va))
        b.append((ia.copy(), va.copy()))
    for la in ROW_LENS[1:]:
        for lb in ROW_LENS[1:]:
            lo = np.sort(rng.choice(1000, size=lb - 1, replace=False)).astype(np.int64)             # below a
            hi = np.sort(rng.choice(1000, size=lb - 1, replace=False)).astype(np.int64) + 200000    # above a
            ia = np.sort(rng.choice(100000, size=la, replace=False)).astype(np.int64) + 1000
            for ib in (np.concatenate([lo, hi[:1]]),                   # disjoint
                       np.concatenate([ia[:1], hi]),                   # first of a, first of b
                       np.concatenate([lo, ia[:1]]),                   # first of a, last of b
                       np.concatenate([ia[-1:], hi]),                  # last of a, first of b
                       np.concatenate([lo, ia[-1:]])):                 # last of a, last of b
                a.append((ia, val(la)))
                assert len(ib) == lb or (lb == 1 and len(ib) == 0)
                b.append((ib, val(len(ib))))
    return a, b


def _union_dense(ra, rb):
    (ia, va), (ib, vb) = ra, rb
    u = np.union1d(ia, ib)
    x, y = np.zeros(len(u)), np.zeros(len(u))
    x[np.searchsorted(u, ia)] = va
    y[np.searchsorted(u, ib)] = vb
    return x, y


@pytest.fixture(scope="module")
def pair_case():
    a, b = _pair_cases()
    m = len(a)
    jac = L.MinHashLSH.distance(L._Rows(H.vectors(a)), np.arange(m), L._Rows(H.vectors(b)), np.arange(m))
    euc, union = np.zeros(m), np.zeros(m)
    for i in range(m):
        x, y = _union_dense(a[i], b[i])
        euc[i] = np.sqrt(np.sum((x - y) ** 2))
        union[i] = len(x)
    return a, b, jac, euc, union


def test_pair_jaccard_bit_equal(pair_case):
    a, b, want, _, _ = pair_case
    m = len(a)
    assert m > 256 and (want == 0.0).any() and (want == 1.0).any() and ((want > 0) & (want < 1)).any()
    A, B = _cuda_rows(a), _cuda_rows(b)
    idx = _t(np.arange(m))
    calls = K.LSH_CALLS
    got = K.pair_jaccard(A, B, idx, idx)
    assert K.LSH_CALLS == calls + 1
    assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64))
    for grid in (1, 7):
        assert torch.equal(K.pair_jaccard(A, B, idx, idx, grid=grid), got)
    # both orders of the two sides, and pairs out of order
    perm = _t(np.random.default_rng(0).permutation(m))
    assert torch.equal(K.pair_jaccard(B, A, perm, perm), got[perm])
    # an index outside its matrix reads nothing
    bad = K.pair_jaccard(A, B, _t([0, m, -1]), _t([0, 0, 0])).cpu().numpy()
    assert bad[0] == want[0] and np.isnan(bad[1]) and np.isnan(bad[2])


def test_pair_euclidean_csr(pair_case):
    a, b, _, want, union = pair_case
    m = len(a)
    A, B = _cuda_rows(a), _cuda_rows(b)
    idx = _t(np.arange(m))
    calls = K.LSH_CALLS
    got = K.pair_euclidean(A, B, idx, idx)
    assert K.LSH_CALLS == calls + 1
    g = got.cpu().numpy()
    err = np.abs(g - want)
    tol = 4 * (union + 4) * EPS * want
    print("csr euclid: max err / tol", float(np.max(err / np.maximum(tol, 1e-300))))
    assert (err <= tol).all()
    same = np.asarray([np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b)])
    assert same.sum() >= len(ROW_LENS) and (g[same] == 0.0).all() and not np.signbit(g[same]).any()
    for grid in (1, 7):
        assert torch.equal(K.pair_euclidean(A, B, idx, idx, grid=grid), got)
    h = m // 2 + 3
    two = torch.cat([K.pair_euclidean(A, B, idx[:h], idx[:h]), K.pair_euclidean(A, B, idx[h:], idx[h:])])
    assert torch.equal(two, got)
    # equal rows give equal bits: the same pair twice, far apart in the list
    rep = _t(np.concatenate([np.arange(m), np.arange(m)[::-1]]))
    twice = K.pair_euclidean(A, B, rep, rep)
    assert torch.equal(twice[:m], got) and torch.equal(twice[m:].flip(0), got)


@pytest.mark.parametrize("d", DS)
def test_pair_euclidean_dense(d):
    rng = np.random.default_rng(d)
    na, nb, m = 70, 64, 600
    A, B = rng.normal(size=(na, d)), rng.normal(size=(nb, d)) * 3.0
    A[1] = A[2]
    B[3] = B[4]
    A[5] = B[7]
    pa, pb = rng.integers(0, na, size=m), rng.integers(0, nb, size=m)
    pa[:6], pb[:6] = [1, 2, 9, 9, 5, 5], [6, 6, 3, 4, 7, 7]
    want = np.sqrt(np.sum((A[pa] - B[pb]) ** 2, axis=1))
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    ta, tb = _t(pa), _t(pb)
    calls = K.LSH_CALLS
    got = K.pair_euclidean(Ad, Bd, ta, tb)
    assert K.LSH_CALLS == calls + 1
    g = got.cpu().numpy()
    err, tol = np.abs(g - want), 4 * (d + 4) * EPS * want
    print("dense euclid d", d, "max err / tol", float(np.max(err / np.maximum(tol, 1e-300))))
    assert (err <= tol).all()
    assert g[0] == g[1] and g[2] == g[3] and g[4] == 0.0 and g[5] == 0.0 and g[0] > 0
    for grid in (1, 7):
        assert torch.equal(K.pair_euclidean(Ad, Bd, ta, tb, grid=grid), got)
    two = torch.cat([K.pair_euclidean(Ad, Bd, ta[:301], tb[:301]), K.pair_euclidean(Ad, Bd, ta[301:], tb[301:])])
    assert torch.equal(two, got)
    if d % 2 == 0:
        # views that start 8 bytes into an allocation: the 16-byte loads must not be taken, the bits stay
        fa = torch.empty(na * d + 1, dtype=torch.float64, device="cuda")
        fb = torch.empty(nb * d + 1, dtype=torch.float64, device="cuda")
        Ao, Bo = fa[1:].view(na, d), fb[1:].view(nb, d)
        Ao.copy_(Ad)
        Bo.copy_(Bd)
        assert Ao.data_ptr() % 16 == 8 and Bo.data_ptr() % 16 == 8
        assert torch.equal(K.pair_euclidean(Ao, Bo, ta, tb), got)
        assert torch.equal(K.pair_euclidean(Ao, Bd, ta, tb), got)
    bad = K.pair_euclidean(Ad, Bd, _t([0, na, 0]), _t([0, 0, -1])).cpu().numpy()
    assert np.isfinite(bad[0]) and np.isnan(bad[1]) and np.isnan(bad[2])


# ---------------------------------------------------------------------------------------------------- operators

def _both(run, monkeypatch):
    """(oracle rows, device rows, kernel launches of the device run): the same operator call on the CPU
    environment with ``ALINK_LSH_HIP=0`` and on ``cuda:0``."""
    from alink_amd import useLocalEnv
    monkeypatch.setenv("ALINK_LSH_HIP", "0")
    useLocalEnv(1, device="cpu")
    calls = K.LSH_CALLS
    want = run()
    assert K.LSH_CALLS == calls
    monkeypatch.delenv("ALINK_LSH_HIP")
    useLocalEnv(1, device="cuda:0")
    got = run()
    return want, got, K.LSH_CALLS - calls


def _mid_threshold(dists):
    """Midway between the two adjacent distinct distances around the median: the oracle keeps and drops pairs."""
    u = np.unique(dists)
    assert len(u) >= 2
    i = max(1, len(u) // 2)
    return 0.5 * (u[i - 1] + u[i])


def test_jaccard_operators_equal_the_host_path(monkeypatch):
    left, right = H.near_duplicates()
    lt, rt = H.table(H.vectors(left)), H.table(H.vectors(right), 1000)
    every, got, ran = _both(lambda: H.run_topn(lt, rt, "JACCARD", 10 ** 6, P=2, T=4), monkeypatch)
    assert 0.01 * 144 * 102 <= len(every) <= 0.5 * 144 * 102
    assert got == every and ran >= 3
    dist = np.asarray([r[2] for r in every])
    assert len(np.unique(dist)) >= 10
    thr = _mid_threshold(dist)
    want, got, ran = _both(lambda: H.run_join(lt, rt, "JACCARD", thr, P=2, T=4), monkeypatch)
    assert 0 < len(want) < len(every) and ran >= 3
    assert got == want
    want, got, _ = _both(lambda: H.run_topn(lt, rt, "JACCARD", 2, P=2, T=4), monkeypatch)
    assert got == want and max(r[3] for r in want) == 2


def _projection_margin(rows, ncols, P, T, width, sparse):
    """The smallest distance of any ``(dot + r) / w`` of the oracle to an integer, less twice its fp64 bound."""
    lsh = L.BucketRandomProjectionLSH(7, ncols, P, T, width)
    R, r = lsh.R.reshape(T * P, ncols), lsh.r.reshape(-1)
    worst = np.inf
    for row in rows:
        if sparse:
            idx, val = row
            terms = val[None, :] * R[:, idx]
            m = max(len(idx), 1)
        else:
            terms = row[None, :] * R
            m = ncols
        q = (terms.sum(1) + r) / width
        bound = (2 * m * EPS * np.abs(terms).sum(1) + 4 * EPS * (np.abs(q) * width + r)) / width
        worst = min(worst, float(np.min(np.abs(q - np.round(q)) - 2 * bound)))
    return worst


@pytest.mark.parametrize("kind", [2, 33, 131, "csr"])
def test_euclidean_operators_equal_the_host_path(kind, monkeypatch):
    P, T, width = 2, 3, 2.0
    sparse = kind == "csr"
    if sparse:
        # the documents over 2^13 columns (the host oracle densifies both sides for its GEMM and its distances),
        # their values scaled by 32 so that projections on unit directions of that size spread over buckets of 2.0
        ncols, total = 2 ** 13, 144 * 102
        left, right = H.near_duplicates(1, ncols, 32.0)
        left[1] = left[0]                           # duplicated dictionary rows on purpose
        lt, rt = H.table(H.vectors(left, ncols)), H.table(H.vectors(right, ncols), 1000)
        size = lambda i, j: len(np.union1d(left[i][0], right[j - 1000][0]))        # noqa: E731
    else:
        left, right = H.noisy_copies(kind)
        lt, rt = H.table(left), H.table(right, 1000)
        ncols, total = kind, 96 * 60
        size = lambda i, j: kind                                                   # noqa: E731
    # preconditions, on the oracle alone
    assert _projection_margin(list(left) + list(right), ncols, P, T, width, sparse) > 0
    every, got_every, ran = _both(lambda: H.run_topn(lt, rt, "EUCLIDEAN", 10 ** 6, P, T, width), monkeypatch)
    assert 0.01 * total <= len(every) <= 0.5 * total and ran >= 3
    dist = np.asarray([r[2] for r in every])
    tol = np.asarray([4 * (size(r[1], r[0]) + 4) * EPS * r[2] for r in every])
    thr = _mid_threshold(dist)
    assert (np.abs(dist - thr) > 2 * tol).all()
    q = np.asarray([r[0] for r in every])
    ties = 0
    for i in range(1, len(every)):
        if q[i] == q[i - 1]:
            if dist[i] == dist[i - 1]:
                ties += 1
            else:
                assert dist[i] - dist[i - 1] > 2 * (tol[i] + tol[i - 1])
    assert ties > 0

    def same(want, got):
        assert [r[:2] + r[3:] for r in got] == [r[:2] + r[3:] for r in want]
        for w, g in zip(want, got):
            i, j = (w[0], w[1]) if len(w) == 3 else (w[1], w[0])
            assert abs(g[2] - w[2]) <= 4 * (size(i, j) + 4) * EPS * w[2]
            if w[2] == 0.0:
                assert g[2] == 0.0
    same(every, got_every)
    want, got, ran = _both(lambda: H.run_join(lt, rt, "EUCLIDEAN", thr, P, T, width), monkeypatch)
    assert 0 < len(want) < len(every) and ran >= 3
    same(want, got)
    want, got, _ = _both(lambda: H.run_topn(lt, rt, "EUCLIDEAN", 2, P, T, width), monkeypatch)
    same(want, got)


@pytest.mark.parametrize("distance", ["JACCARD", "EUCLIDEAN"])
def test_empty_sides(distance, monkeypatch):
    ncols = 2 ** 13
    left, _ = H.near_duplicates(0, ncols)
    full = H.table(H.vectors(left[:20], ncols))
    none = H.table(H.vectors([]), 1000)
    blank = H.table(H.vectors([(np.zeros(0, dtype=np.int64), np.zeros(0))] * 4, ncols), 1000)
    for lt, rt in ((full, none), (none, full)):
        want, got, ran = _both(lambda: H.run_join(lt, rt, distance, 10.0), monkeypatch)
        assert want == [] and got == [] and ran == 0
        want, got, ran = _both(lambda: H.run_topn(lt, rt, distance, 3), monkeypatch)
        assert want == [] and got == [] and ran == 0
    want, got, ran = _both(lambda: H.run_join(blank, blank, distance, 10.0), monkeypatch)
    assert len(want) == 16 and got == want
    if distance == "JACCARD":
        assert ran == 0                             # only empty vectors: no kernel reads a row
    want, got, _ = _both(lambda: H.run_join(full, blank, distance, 10.0), monkeypatch)
    assert got == want
    want, got, _ = _both(lambda: H.run_topn(blank, full, distance, 2), monkeypatch)
    assert got == want
