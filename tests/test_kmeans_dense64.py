"""Dense fp64 KMeans (``ops/kmeans_dense64.py``): the selection rule and the torch paths, on the CPU."""
import numpy as np
import pytest
import torch


class _FakeCuda:
    """Stands in for a device tensor in the selection rule, which reads attributes only."""

    def __init__(self, n, d, dtype=torch.float64, contiguous=True, dim=2):
        self.shape, self.dtype, self.is_cuda, self._c, self._dim = (n, d), dtype, True, contiguous, dim

    def dim(self):
        return self._dim

    def is_contiguous(self):
        return self._c


def test_selection_rule(monkeypatch):
    from alink_amd.ops import kmeans_dense64 as kd
    from alink_amd.ops.kmeans_sparse import DENSE_DMAX
    monkeypatch.delenv("ALINK_KMEANS_DENSE64", raising=False)
    monkeypatch.setattr(kd, "isinstance", lambda o, t: True, raising=False)   # let the stand-in pass for a tensor
    assert kd.dense64_supported(_FakeCuda(10, 37), 3)
    assert kd.dense64_supported(_FakeCuda(0, 1), 1)
    assert kd.dense64_supported(_FakeCuda(10, DENSE_DMAX), 4096)
    assert not kd.dense64_supported(_FakeCuda(10, DENSE_DMAX + 1), 3)
    assert not kd.dense64_supported(_FakeCuda(10, 0), 3)
    assert not kd.dense64_supported(_FakeCuda(2 ** 31, 4), 3)
    assert not kd.dense64_supported(_FakeCuda(10, 37), 0)
    assert not kd.dense64_supported(_FakeCuda(10, 37, dtype=torch.float32), 3)
    assert not kd.dense64_supported(_FakeCuda(10, 37, dtype=torch.bfloat16), 3)
    assert not kd.dense64_supported(_FakeCuda(10, 37, contiguous=False), 3)
    assert not kd.dense64_supported(_FakeCuda(10, 37, dim=1), 3)
    assert kd.dense64_selected(_FakeCuda(10, 37), 3)
    monkeypatch.setenv("ALINK_KMEANS_DENSE64", "0")
    assert not kd.dense64_selected(_FakeCuda(10, 37), 3)
    monkeypatch.setenv("ALINK_KMEANS_DENSE64", "1")
    assert kd.dense64_selected(_FakeCuda(10, 37), 3)


def test_cpu_tensors_are_never_selected(monkeypatch):
    from alink_amd.ops import kmeans_dense64 as kd
    monkeypatch.delenv("ALINK_KMEANS_DENSE64", raising=False)
    X = torch.zeros((10, 37), dtype=torch.float64)
    assert not kd.dense64_supported(X, 3) and not kd.dense64_selected(X, 3)
    assert not kd.dense64_supported(None, 3)


def _small():
    rng = np.random.default_rng(7)
    X = rng.normal(size=(50, 7))
    C = rng.normal(size=(5, 7))
    C[3] = C[1]                     # an exact duplicate: the lower index wins
    return X, C


@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
def test_torch_paths_against_direct_loop(dist):
    from alink_amd.ops import kmeans_dense64 as kd
    X, C = _small()
    if dist == "COSINE":
        X = X / np.linalg.norm(X, axis=1, keepdims=True)
        C = C / np.linalg.norm(C, axis=1, keepdims=True)
    n, d = X.shape
    k = C.shape[0]
    ref = np.empty((n, k))
    for r in range(n):
        for c in range(k):
            ref[r, c] = 1.0 - float(np.dot(X[r], C[c])) if dist == "COSINE" else float(((X[r] - C[c]) ** 2).sum())
    idx, best = kd.nearest_torch(torch.from_numpy(X), torch.from_numpy(C), dist)
    idx, best = idx.numpy(), best.numpy()
    assert idx.dtype == np.int64 and not (idx == 3).any() and (idx == 1).any()
    # m = d + 2 terms of size at most |x|^2 + |c|^2 + |x||c| <= 2 (|x|^2 + |c|^2): 4 x 2 m 2^-53 sum|terms|
    tol = 4.0 * 2.0 * (d + 2) * 2.0 ** -53 * 2.0 * ((X * X).sum(1).max() + (C * C).sum(1).max())
    assert (ref[np.arange(n), idx] - ref.min(1) <= tol).all()
    assert (np.abs(best - ref.min(1)) <= tol).all()
    if dist == "EUCLIDEAN":
        buf = kd.assign_accumulate_torch(torch.from_numpy(X), torch.from_numpy(C)).numpy()
        want = np.zeros((k, d + 1))
        for r in range(n):
            want[idx[r], :d] += X[r]
            want[idx[r], d] += 1.0
        assert np.array_equal(buf, want)            # the CPU sums run in ascending row order
        assert np.array_equal(kd.accumulate(torch.from_numpy(X), torch.from_numpy(idx), k).numpy(), want)
        assert np.array_equal(kd.nearest_counts(torch.from_numpy(X), torch.from_numpy(C), dist).numpy(), want[:, d])


def test_only_euclidean_and_cosine():
    from alink_amd.ops import kmeans_dense64 as kd
    X, C = (torch.from_numpy(a) for a in _small())
    for fn in (kd.nearest, kd.nearest_counts, kd.nearest_torch):
        with pytest.raises(ValueError):
            fn(X, C, "CITYBLOCK")


def test_empty_rows_give_shaped_zeros():
    from alink_amd.ops import kmeans_dense64 as kd
    C = torch.from_numpy(_small()[1])
    X0 = torch.zeros((0, 7), dtype=torch.float64)
    idx, dist = kd.nearest(X0, C, "EUCLIDEAN")
    assert idx.shape == (0,) and idx.dtype == torch.int64 and dist.shape == (0,) and dist.dtype == torch.float64
    assert torch.equal(kd.nearest_counts(X0, C, "COSINE"), torch.zeros(5, dtype=torch.int64))
    assert torch.equal(kd.assign_accumulate(X0, C), torch.zeros((5, 8), dtype=torch.float64))
    assert torch.equal(kd.accumulate(X0, torch.zeros(0, dtype=torch.int64), 5), torch.zeros((5, 8), dtype=torch.float64))


def test_cpu_rows_keep_the_torch_result_bit_for_bit():
    from alink_amd.ops import kmeans as kops, kmeans_dense64 as kd
    X, C = (torch.from_numpy(a) for a in _small())
    calls = kd.DENSE64_CALLS
    got = kops.assign_accumulate(X, C)
    assert kd.DENSE64_CALLS == calls
    assert torch.equal(got, kops.assign_accumulate_torch(X, C))


# (k, d) -> the documented (nt, nblk): nt the power of two whose 16 nt rows cover k, at most 8; nblk blocks of 16 nt.
# nt = 1, 2, 4, 8, more than one block, an odd d and a dim chunk edge (d = 32 fills a chunk, d = 34 spills over)
@pytest.mark.parametrize("k,d,nt_doc,nblk_doc", [(1, 1, 1, 1), (5, 7, 1, 1), (17, 32, 2, 1), (40, 34, 4, 1),
                                                 (300, 64, 8, 3)])
def test_centroid_image_layout(k, d, nt_doc, nblk_doc):
    """The Python end of the image contract of ``csrc/dense64_mfma.h``: element [blk, dch, u, t, g, m, s] of the
    image is C[(blk * nt + t) * 16 + m, dch * 32 + 16 u + 4 g + s], or 0 outside C — checked index by index, not by the
    permute that builds it; ninit is -|c|^2 / 2 summed over the padded rows, bit for bit, and 0 on padded slots and
    for COSINE."""
    import math
    from alink_amd.ops import kmeans_dense64 as kd
    rng = np.random.default_rng(100 * k + d)
    C = rng.normal(size=(k, d))
    if k > 3:
        C[2] = C[3] = C[1]          # duplicate rows, odd and even: the same bits of |c|^2 wherever a row starts
    ndch = (d + 31) // 32
    for cosine in (0, 1):
        img, ninit, nt, nblk = kd.centroid_image(torch.from_numpy(C), cosine, "cpu")
        assert kd.tiles(k) == nt == nt_doc and nblk == nblk_doc
        assert img.dtype == torch.float64 and img.is_contiguous()
        assert tuple(img.shape) == (nblk, ndch, 2, nt, 4, 16, 4)
        got = img.numpy()
        pad = np.full((nblk * nt * 16, ndch * 32), np.nan)          # the padded rows, built by the same index loop
        for blk, dch, u, t, g, m, s in np.ndindex(*got.shape):
            r, j = (blk * nt + t) * 16 + m, dch * 32 + 16 * u + 4 * g + s
            want = C[r, j] if r < k and j < d else 0.0
            assert got[blk, dch, u, t, g, m, s] == want, (blk, dch, u, t, g, m, s)
            pad[r, j] = want
        ni = ninit.numpy()
        assert ni.dtype == np.float64 and ni.shape == (nblk * nt * 16,)
        assert not ni[k:].any()                                     # exactly 0 on the padded slots
        if cosine:
            assert not ni.any()
            continue
        # -|c|^2 / 2 taken from the padded rows, bit for bit: the summation order is that of a padded row, whatever
        # the alignment of the row in C
        padt = torch.from_numpy(pad)
        assert np.array_equal(ni, (-0.5 * (padt * padt).sum(1)).numpy())
        for r in range(k):
            # independently: any order of the d (+ zero padding) fp64 additions is within d ulp-halves of the exact
            # sum of squares
            exact = math.fsum(float(v) * float(v) for v in C[r])
            assert abs(ni[r] + 0.5 * exact) <= 0.5 * exact * (d + 1) * 2.0 ** -53, r
        if k > 3:
            assert ni[2] == ni[1] and ni[3] == ni[1]
