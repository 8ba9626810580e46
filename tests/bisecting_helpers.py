"""Shared by ``test_bisecting_rows.py`` (CPU) and ``test_bisecting_gpu.py``: the seeded data and trees, the per-row
numpy reference of the descent with its rounding bound, and the trainer call.

Tolerance (the rule of ``test_kmeans_dense64_gpu.py``): two fp64 evaluations of a sum of ``m`` terms differ by at most
``2 m 2^-53 sum|terms|``; the tests allow 4x that.
"""
import functools

import numpy as np
import torch

EPS = 2.0 ** -53
N = 1003


def blobs(n=600, d=37, k=4):
    """The ``_blobs`` recipe of ``test_kmeans_dense64_gpu.py``: 4 separated blobs away from the origin."""
    rng = np.random.default_rng(3)
    centers = rng.normal(size=(k, d)) * 10.0 + 3.0
    lab = np.arange(n) % k
    return centers[lab] + rng.normal(size=(n, d)) * 0.3


def heap_tree(d, cosine):
    """A complete tree of 15 internal nodes (ids 1 .. 15) and 16 leaves: centres of the children of node ``i`` are
    rows ``2 i - 1`` and ``2 i`` of ``default_rng(100 + d).normal((31, d)) * 0.5`` (row 0 is the root's own)."""
    C = np.random.default_rng(100 + d).normal(size=(31, d)) * 0.5
    if cosine:
        C = C / np.linalg.norm(C, axis=1, keepdims=True)
    return {i + 1: C[i] for i in range(31)}


def data(d, cosine):
    X = np.random.default_rng(11 + d).normal(size=(N, d))
    X[np.arange(N) % 17 == 5] *= -(2.0 ** 12)
    if cosine:
        X = X / np.linalg.norm(X, axis=1, keepdims=True)
    return X


class DenseRef:
    """Rows [n, d] for the host reference: ``dots(i, W)`` = (x_i . w, |x_i| . |w|) per row w of W, ``m`` terms."""

    def __init__(self, X):
        self.X, self.n = X, X.shape[0]

    def dots(self, i, W):
        x = self.X[i]
        return np.array([x @ w for w in W]), np.array([np.abs(x) @ np.abs(w) for w in W]), self.X.shape[1]


class CsrRef:
    """CSR rows (entries outside [0, d) dropped) for the host reference: the dense row's dot without its zero terms."""

    def __init__(self, crow, col, val, d):
        self.crow, self.col, self.val, self.d, self.n = crow, col, val, d, len(crow) - 1

    def dots(self, i, W):
        c, v = self.col[self.crow[i]:self.crow[i + 1]], self.val[self.crow[i]:self.crow[i + 1]]
        ok = (c >= 0) & (c < self.d)
        c, v = c[ok], v[ok]
        return (np.array([v @ w[c] for w in W]), np.array([np.abs(v) @ np.abs(w[c]) for w in W]), max(len(c), 1))


def planes(centers, table, cosine):
    """Per descending slot: (a, b, thr) with the side ``1 - x.a < 1 - x.b`` (COSINE) or (v, None, thr) with
    ``x.v < thr``, computed as ``BisectingKMeansModelMapper._leaf_of`` does."""
    out = []
    for s in range(table.P):
        c = table.nodes[s]
        l, r = centers[2 * c], centers[2 * c + 1]
        if cosine:
            out.append((l / np.sqrt(l @ l), r / np.sqrt(r @ r), None))
        else:
            v, m = r - l, 0.5 * (r + l)
            out.append((v, None, m @ v))
    return out


def side(ref, i, plane, cosine):
    """(goes left, |gap| / bound) of row ``i`` at ``plane``; the bound is 4 x 2 m 2^-53 sum|x_j v_j| (COSINE: both
    dots' bounds added, plus 4 x 2^-53 for the two subtractions from 1)."""
    a, b, thr = plane
    if cosine:
        (da, db), (ta, tb), m = ref.dots(i, [a, b])
        bound = 4.0 * (2.0 * m * EPS * (ta + tb) + 4.0 * EPS)
        return (1 - da) < (1 - db), abs((1 - da) - (1 - db)) / bound
    (p,), (t,), m = ref.dots(i, [a])
    bound = 4.0 * 2.0 * m * EPS * t
    return p < thr, (abs(p - thr) / bound if bound > 0 else np.inf)


def separation(ref, centers, table, cosine):
    """The smallest |gap| / bound over every row and EVERY plane of the table."""
    pl = planes(centers, table, cosine)
    return min(side(ref, i, q, cosine)[1] for i in range(ref.n) for q in pl)


def reference_descend(ref, centers, table, slot, levels, cosine):
    """Per row and per level on the host: the new slots."""
    pl = planes(centers, table, cosine)
    out = np.array(slot, dtype=np.int64)
    for i in range(ref.n):
        s = out[i]
        for _ in range(levels):
            if not (0 <= s < table.S) or table.left_h[s] < 0:
                break
            s = table.left_h[s] if side(ref, i, pl[s], cosine)[0] else table.right_h[s]
        out[i] = s
    return out


def check_table(table):
    assert table.S == 31 and table.P == 15 and table.depth == 4 and table.nodes == list(range(1, 32))


def start_slots(seed):
    """Random starting slots of the heap tree that include -1 and leaf slots."""
    start = np.random.default_rng(seed).integers(-1, 31, size=N).astype(np.int32)
    assert (start == -1).any() and (start >= 15).any() and (start < 15).any()
    return start


@functools.lru_cache(maxsize=None)
def descend_case(d, cosine, device="cpu"):
    """(X, centers, table, random starting slots, reference after 1 level from them, reference after 4 levels from
    the root); asserted on the reference alone: every row is more than twice the bound from every plane."""
    from alink_amd.ops.bisecting import tree_table
    X = data(d, cosine)
    centers = heap_tree(d, cosine)
    table = tree_table(centers, list(range(1, 32)), cosine, device)
    check_table(table)
    ref = DenseRef(X)
    sep = separation(ref, centers, table, cosine)
    print("separation", d, "COSINE" if cosine else "EUCLIDEAN", sep, "bounds")
    assert sep > 2.0, (d, cosine, sep)
    start = start_slots(7 + d)
    one = reference_descend(ref, centers, table, start, 1, cosine)
    full = reference_descend(ref, centers, table, np.zeros(N, np.int32), 4, cosine)
    return X, centers, table, start, one, full


def train(X, dist, device, sparse_size=None, max_iter=None):
    """Model rows of ``train_bisecting_kmeans`` at k = 4 for the rows ``X`` as a dense vector column, or with
    ``sparse_size`` as a sparse vector column of that vector size."""
    from alink_amd import useLocalEnv
    from alink_amd.common.linalg.block import SparseBlock
    from alink_amd.common.params import Params
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import TableSchema, Types
    from alink_amd.models.clustering.bisecting import train_bisecting_kmeans
    env = useLocalEnv(1, device=device)
    if sparse_size is None:
        mt = MTable(TableSchema(["v"], [Types.DENSE_VECTOR]), [Column(torch.from_numpy(X).to(device))])
    else:
        n, d = X.shape
        blk = SparseBlock(torch.arange(n + 1, dtype=torch.int64) * d, torch.arange(d, dtype=torch.int64).repeat(n),
                          torch.from_numpy(X.reshape(-1).copy()), sparse_size)
        mt = MTable(TableSchema(["v"], [Types.SPARSE_VECTOR]), [Column(blk.to(device))])
    p = Params().set("vectorCol", "v").set("k", 4).set("distanceType", dist)
    if max_iter is not None:
        p.set("maxIter", max_iter)
    return train_bisecting_kmeans(mt, p, env)
