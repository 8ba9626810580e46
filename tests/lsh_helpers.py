"""Data shared by ``test_lsh_device.py`` and ``test_lsh_gpu.py``: sparse rows of the lengths at which the LSH kernels
change path, near-duplicate documents, noisy copies of cluster centres, and tables of them."""
import numpy as np
import torch

from alink_amd.common.linalg import SparseVector
from alink_amd.common.table import Column, MTable
from alink_amd.common.types import Types

ROW_LENS = (0, 1, 2, 63, 64, 65, 130, 513)
NCOLS = 2 ** 18
EPS = 2.0 ** -53


def sparse_row(rng, length, ncols=NCOLS, hi=None):
    """A strictly ascending int64 index row of ``length`` entries below ``hi`` (default ``ncols``)."""
    u = np.zeros(0, dtype=np.int64)
    while len(u) < length:                          # no permutation of the whole range: hi goes up to 2^31 - 1
        u = np.unique(np.concatenate([u, rng.integers(0, hi or ncols, size=length + 16)]))
    return np.sort(rng.choice(u, size=length, replace=False)).astype(np.int64)


def near_duplicates(seed=0, ncols=NCOLS, scale=1.0):
    """(left, right): 144 and 102 documents as (indices, values) rows.  36 shared base documents of the lengths
    ``ROW_LENS`` (in turn) give 4 left and 2 right copies each; 18 more base documents give 30 right rows (2 copies
    of the first 12, 1 of the rest).  A copy replaces up to 3 entries of its base by fresh columns; its values are
    ``scale`` times a multiple of 1/4 in [1/4, 2]."""
    rng = np.random.default_rng(seed)
    bases = [sparse_row(rng, ROW_LENS[i % len(ROW_LENS)], ncols) for i in range(54)]

    def copy(b):
        b = b.copy()
        k = int(rng.integers(0, 4))
        if len(b) and k:
            drop = rng.choice(len(b), size=min(k, len(b)), replace=False)
            b[drop] = rng.integers(0, ncols, size=len(drop))
            b = np.unique(b)
        return b, rng.integers(1, 9, size=len(b)).astype(np.float64) / 4.0 * scale

    left = [copy(bases[i]) for i in range(36) for _ in range(4)]
    right = [copy(bases[i]) for i in range(36) for _ in range(2)]
    right += [copy(bases[36 + i]) for i in range(18) for _ in range(2 if i < 12 else 1)]
    return left, right


def noisy_copies(d, seed=0):
    """(left [96, d], right [60, d]) fp64: 12 centres, 8 and 5 noisy copies; the left side, the dictionary of the
    top-N operator, repeats a row of every group bit for bit (duplicated rows are there on purpose).  Values are
    multiples of 2^-10."""
    rng = np.random.default_rng(100 + d + seed)
    centres = np.round(rng.normal(size=(12, d)) * 4.0 * 1024) / 1024
    q = lambda x: np.round(x * 1024) / 1024                                          # noqa: E731
    left = q(np.repeat(centres, 8, 0) + 0.05 * rng.normal(size=(96, d)))
    right = q(np.repeat(centres, 5, 0) + 0.05 * rng.normal(size=(60, d)))
    left[1::8] = left[0::8]                                                          # a duplicate in every group
    return left, right


def vectors(rows, ncols=NCOLS):
    return [SparseVector(ncols, i.astype(np.int32), v) for i, v in rows]


def csr(rows, ncols=NCOLS, device="cpu"):
    """A sparse ``FeatureMatrix`` of (indices, values) rows."""
    from alink_amd.models.common.features import FeatureMatrix
    crow = np.zeros(len(rows) + 1, dtype=np.int64)
    crow[1:] = np.cumsum([len(i) for i, _ in rows])
    col = np.concatenate([i for i, _ in rows]) if rows else np.zeros(0, dtype=np.int64)
    val = np.concatenate([v for _, v in rows]) if rows else np.zeros(0)
    return FeatureMatrix(crow=torch.from_numpy(crow).to(device), col=torch.from_numpy(col.astype(np.int64)).to(device),
                         val=torch.from_numpy(val.astype(np.float64)).to(device), ncols=ncols)


def table(vecs, first_id=0):
    """``id long, vec`` table: ``vecs`` is a list of vectors or a dense [n, d] array."""
    n = len(vecs)
    ids = torch.arange(first_id, first_id + n, dtype=torch.int64)
    col = Column(torch.from_numpy(np.ascontiguousarray(vecs))) if isinstance(vecs, np.ndarray) else Column(list(vecs))
    return MTable.from_columns(["id", "vec"], [Types.LONG, Types.VECTOR], [Column(ids), col])


def run_join(left, right, distance, threshold, P=2, T=3, width=2.0, env=None):
    from alink_amd import ApproxVectorSimilarityJoinLSHBatchOp, TableSourceBatchOp
    op = ApproxVectorSimilarityJoinLSHBatchOp().setLeftIdCol("id").setRightIdCol("id").setLeftCol("vec") \
        .setRightCol("vec").setDistanceType(distance).setDistanceThreshold(threshold) \
        .setNumProjectionsPerTable(P).setNumHashTables(T).setProjectionWidth(width).setSeed(7)
    return [tuple(r) for r in op.linkFrom(TableSourceBatchOp(left), TableSourceBatchOp(right)).collect()]


def run_topn(left, right, distance, top_n, P=2, T=3, width=2.0):
    from alink_amd import ApproxVectorSimilarityTopNLSHBatchOp, TableSourceBatchOp
    op = ApproxVectorSimilarityTopNLSHBatchOp().setLeftIdCol("id").setRightIdCol("id").setLeftCol("vec") \
        .setRightCol("vec").setDistanceType(distance).setTopN(top_n) \
        .setNumProjectionsPerTable(P).setNumHashTables(T).setProjectionWidth(width).setSeed(7)
    return [tuple(r) for r in op.linkFrom(TableSourceBatchOp(left), TableSourceBatchOp(right)).collect()]
