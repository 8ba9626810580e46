"""BisectingKMeans on the rows objects of ``ops/kmeans_rows.py``, CPU: the torch ``descend`` / ``child_stats`` against
per-row numpy on seeded trees, and the trainer against the model rows recorded before it moved onto them.

Tolerance (the rule of ``test_kmeans_dense64_gpu.py``): two fp64 evaluations of a sum of ``m`` terms differ by at most
``2 m 2^-53 sum|terms|``; the tests allow 4x that.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bisecting_helpers import EPS, N, DenseRef, blobs, descend_case, reference_descend, train  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bisecting_parent_models.json")


DS = (1, 3, 5, 32, 37, 131)


@pytest.mark.parametrize("d,cosine", [(d, c) for c in (False, True) for d in DS if not (c and d == 1)])
def test_torch_descend_matches_numpy(d, cosine):
    from alink_amd.ops.kmeans_rows import _TorchRows, rows
    X, centers, table, start, one, full = descend_case(d, cosine)
    r = rows(torch.from_numpy(X), "COSINE" if cosine else "EUCLIDEAN")
    assert type(r) is _TorchRows
    got = r.descend(table, torch.from_numpy(start.copy()), 1)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), one)
    keep = (start < 0) | (start >= 15)
    assert np.array_equal(got.numpy()[keep], start[keep])
    got = r.descend(table, torch.zeros(N, dtype=torch.int32), 4)
    assert np.array_equal(got.numpy(), full) and int(got.min()) >= 15


@pytest.mark.parametrize("integer", [True, False])
def test_torch_child_stats_matches_numpy(integer):
    from alink_amd.ops.kmeans_rows import rows
    n, d, nslots = 700, 37, 6
    rng = np.random.default_rng(5 + int(integer))
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float64) if integer else rng.normal(size=(n, d))
    slot = rng.integers(-1, nslots + 1, size=n).astype(np.int32)      # -1 and nslots are outside
    slot[slot == 4] = 3                                               # slot 4 stays empty
    ok = (slot >= 0) & (slot < nslots)
    r = rows(torch.from_numpy(X), "EUCLIDEAN")
    buf = r.child_stats(torch.from_numpy(slot), nslots)
    assert buf.shape == (nslots, d + 2) and buf.dtype == torch.float64
    ref = np.zeros((nslots, d + 2))
    for i in np.flatnonzero(ok):
        ref[slot[i], :d] += X[i]
        ref[slot[i], d] += 1.0
        ref[slot[i], d + 1] += X[i] @ X[i]
    cnt = ref[:, d]
    assert np.array_equal(buf[:, d].numpy(), cnt) and cnt[4] == 0 and cnt.sum() == ok.sum() < n
    if integer:
        assert np.array_equal(buf.numpy(), ref)
    else:
        sabs = np.zeros((nslots, d + 2))
        np.add.at(sabs[:, :d], slot[ok], np.abs(X[ok]))
        np.add.at(sabs[:, d + 1], slot[ok], (X[ok] * X[ok]).sum(1))
        bound = 4.0 * 2.0 * np.maximum(cnt, d)[:, None] * EPS * sabs   # |x|^2 is itself a sum of d terms
        assert (np.abs(buf.numpy() - ref) <= bound).all()
    empty = rows(torch.zeros((0, d), dtype=torch.float64), "EUCLIDEAN")
    assert torch.equal(empty.child_stats(torch.zeros(0, dtype=torch.int32), nslots),
                       torch.zeros((nslots, d + 2), dtype=torch.float64))


def test_sparse_torch_rows_match_dense():
    """CSR rows on the CPU (the chunked CSR product) give the dense torch kind's slots and sums."""
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops.kmeans_rows import rows
    d = 37
    X, centers, table, start, one, full = descend_case(d, False)
    Xs = X.copy()
    Xs[:, 5:] = np.where(np.random.default_rng(1).random((N, d - 5)) < 0.5, 0.0, Xs[:, 5:])
    Xs[17] = 0.0                                                     # an empty row
    nz = Xs != 0
    crow = np.zeros(N + 1, np.int64)
    crow[1:] = np.cumsum(nz.sum(1))
    fm = FeatureMatrix(crow=torch.from_numpy(crow), col=torch.from_numpy(np.nonzero(nz)[1].astype(np.int64)),
                       val=torch.from_numpy(Xs[nz]), ncols=d)
    sp, de = rows(fm, "EUCLIDEAN"), rows(torch.from_numpy(Xs), "EUCLIDEAN")
    want = reference_descend(DenseRef(Xs), centers, table, np.zeros(N, np.int32), 4, False)
    a = sp.descend(table, torch.zeros(N, dtype=torch.int32), 4)
    b = de.descend(table, torch.zeros(N, dtype=torch.int32), 4)
    # rows within the bound of a plane may differ between two orders of summation; on this data none is
    assert np.array_equal(a.numpy(), want) and np.array_equal(b.numpy(), want)
    sa, sb = sp.child_stats(a - 15, 16), de.child_stats(b - 15, 16)
    assert torch.equal(sa[:, d], sb[:, d]) and float(sa[:, d].sum()) == N
    atol = 4.0 * 2.0 * N * EPS * float(np.abs(Xs).max()) ** 2 * d
    assert float((sa - sb).abs().max()) <= atol


@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
def test_cpu_training_is_unchanged(dist):
    """Byte-identical model rows to those recorded from the trainer before it moved onto the rows objects."""
    with open(GOLDEN) as f:
        want = json.load(f)[dist]
    got = train(blobs(), dist, "cpu")
    assert [[int(r[0]), r[1]] + list(r[2:]) for r in got] == want
    assert len(got) == 8 and json.loads(got[1][1])["size"] == 600


def test_bulk_noise_draw_is_the_scalar_draw():
    """``JavaRandom.nextDoubles(n)`` (the trainer's noise) gives ``nextDouble`` n times and leaves the same state."""
    from alink_amd.common.jrandom import JavaRandom
    for seed in (0, 12345, -7):
        a, b = JavaRandom(seed), JavaRandom(seed)
        for n in (1, 2, 3, 37, 1000, 0, 5):
            assert np.array_equal(np.array([a.nextDouble() for _ in range(n)]), b.nextDoubles(n))
            assert a.nextInt() == b.nextInt()
