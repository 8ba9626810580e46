"""BisectingKMeans on the GPU: the descent kernels (``ops/csrc/bisecting.hip``), ``Rows.descend`` /
``Rows.child_stats`` of ``ops/kmeans_rows.py``, the trainer and the mapper.

Tolerance (derived, not tuned; the rule of ``test_kmeans_dense64_gpu.py``): two fp64 evaluations of a sum of ``m``
terms differ by at most ``2 m 2^-53 sum|terms|``; the tests allow 4x that.  For a projection ``m = d`` (the row's
entry count for CSR rows) with the terms ``x_j v_j``; COSINE adds both dots' bounds and ``4 x 2^-53`` for the two
subtractions from 1.  For a child sum ``m`` is the child's row count.  The descent data is away from every plane by
more than twice that bound (asserted on the host reference alone), so the kernel's slots must equal the reference's.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bisecting_helpers as BH  # noqa: E402
from bisecting_helpers import EPS, N  # noqa: E402

pytestmark = pytest.mark.gpu

DS = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 128, 131, 300, 1024)
MIB = 2 ** 20


def _rows(X, cosine):
    from alink_amd.ops.kmeans_rows import _Dense64Rows, rows
    r = rows(X, "COSINE" if cosine else "EUCLIDEAN")
    assert type(r) is _Dense64Rows
    return r


def _slots(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int32)).cuda()


# COSINE at d = 1 is left out: every normalised 1-d row ties
@pytest.mark.parametrize("d,cosine", [(d, c) for c in (False, True) for d in DS if not (c and d == 1)])
def test_descend_dense(d, cosine):
    from alink_amd.ops import bisecting as bops
    X, centers, table, start, one, full = BH.descend_case(d, cosine, "cuda")
    r = _rows(torch.from_numpy(X).cuda(), cosine)
    calls = bops.BISECT_CALLS
    slot = _slots(start)
    got = r.descend(table, slot, 1)
    assert bops.BISECT_CALLS == calls + 1
    assert got.data_ptr() == slot.data_ptr() and got.dtype == torch.int32       # in place
    assert np.array_equal(got.cpu().numpy(), one)
    keep = (start < 0) | (start >= 15)                      # no slot and leaf slots come back unchanged
    assert np.array_equal(got.cpu().numpy()[keep], start[keep])
    got4 = r.descend(table, _slots(np.zeros(N)), 4)
    assert np.array_equal(got4.cpu().numpy(), full) and int(got4.min()) >= 15
    for grid in (1, 7):
        assert torch.equal(r.descend(table, _slots(start), 1, grid=grid), got)
        assert torch.equal(r.descend(table, _slots(np.zeros(N)), 4, grid=grid), got4)
    if d % 2 == 0:
        # a view that starts 8 bytes into an allocation: the 16-byte loads must not be taken, the sides stay
        flat = torch.empty(N * d + 1, dtype=torch.float64, device="cuda")
        Xo = flat[1:].view(N, d)
        Xo.copy_(r.X)
        assert Xo.data_ptr() % 16 == 8
        ro = _rows(Xo, cosine)
        assert torch.equal(ro.descend(table, _slots(start), 1), got)
        assert torch.equal(ro.descend(table, _slots(np.zeros(N)), 4), got4)


def _integer_tree(d):
    """The heap tree with integer centres whose sibling pairs differ by an even vector: every plane ``x . v < thr``
    has an integer ``v``, its midpoint ``m`` is an integer point on it, and every dot is exact in any order."""
    rng = np.random.default_rng(40 + d)
    centers = {1: rng.integers(-3, 4, size=d).astype(np.float64)}
    for c in range(1, 16):
        l = rng.integers(-3, 4, size=d).astype(np.float64)
        delta = rng.integers(-2, 3, size=d).astype(np.float64)
        delta[0] = 1.0                                      # never the zero vector
        centers[2 * c], centers[2 * c + 1] = l, l + 2.0 * delta
    return centers


@pytest.mark.parametrize("d", [5, 64])
def test_ties_go_right(d):
    from alink_amd.ops.bisecting import tree_table
    centers = _integer_tree(d)
    table = tree_table(centers, list(range(1, 32)), False, "cuda")
    BH.check_table(table)
    X = np.random.default_rng(50 + d).integers(-3, 4, size=(N, d)).astype(np.float64)
    start = BH.start_slots(60 + d)
    planted = np.flatnonzero(start < 15)[::3]               # every third row that descends sits on its own plane
    planted = planted[start[planted] >= 0]
    for i in planted:
        c = table.nodes[start[i]]
        X[i] = 0.5 * (centers[2 * c] + centers[2 * c + 1])
        v = centers[2 * c + 1] - centers[2 * c]
        assert X[i] @ v == (0.5 * (centers[2 * c] + centers[2 * c + 1])) @ v
    assert len(planted) > 100
    ref = BH.DenseRef(X)
    one = BH.reference_descend(ref, centers, table, start, 1, False)
    full = BH.reference_descend(ref, centers, table, np.zeros(N, np.int32), 4, False)
    assert np.array_equal(one[planted], table.right_h[start[planted]])          # the reference sends them right
    r = _rows(torch.from_numpy(X).cuda(), False)
    got = r.descend(table, _slots(start), 1).cpu().numpy()
    assert np.array_equal(got[planted], table.right_h[start[planted]])
    assert np.array_equal(got, one)                                             # every row, exactly
    assert np.array_equal(r.descend(table, _slots(np.zeros(N)), 4).cpu().numpy(), full)


@pytest.mark.parametrize("cosine", [False, True])
def test_nan_rows_go_right(cosine):
    d = 37
    X, centers, table, start, one, full = BH.descend_case(d, cosine, "cuda")
    Xn = X.copy()
    bad = [37, 150, 1002]
    Xn[37, 2] = np.nan
    Xn[150, :] = np.nan
    Xn[1002, d - 1] = np.nan
    got = _rows(torch.from_numpy(Xn).cuda(), cosine).descend(table, _slots(np.zeros(N)), 4).cpu().numpy()
    assert (got[bad] == 30).all()                           # right at every level of the heap tree: the last slot
    keep = np.ones(N, bool)
    keep[bad] = False
    clean = _rows(torch.from_numpy(Xn[keep]).cuda(), cosine).descend(table, _slots(np.zeros(N - 3)), 4)
    assert np.array_equal(got[keep], clean.cpu().numpy()) and np.array_equal(got[keep], full[keep])


D_CSR = 2 ** 18


@functools.lru_cache(maxsize=None)
def _csr_rows():
    """CSR rows over 2^18 columns, 0 to 200 entries each (every 13th row empty), row 7 with 300 entries (more than
    4 x 64); every 7th row also stores two columns past the vector size, which are ignored."""
    rng = np.random.default_rng(21)
    cols, vals = [], []
    for i in range(N):
        ln = 300 if i == 7 else 0 if i % 13 == 0 else int(rng.integers(1, 201))
        c = set(rng.choice(D_CSR, size=ln, replace=False).tolist())
        if i % 7 == 2 and ln:
            c.update((D_CSR, D_CSR + 31))
        c = np.sort(np.fromiter(c, dtype=np.int64, count=len(c)))
        cols.append(c)
        vals.append(rng.normal(size=c.size) * (-(2.0 ** 12) if i % 17 == 5 else 1.0))
    crow = np.zeros(N + 1, np.int64)
    crow[1:] = np.cumsum([c.size for c in cols])
    assert (np.diff(crow) == 0).any() and np.diff(crow).max() > 256
    return crow, np.concatenate(cols), np.concatenate(vals)


@functools.lru_cache(maxsize=None)
def _csr_case(cosine):
    from alink_amd.ops.bisecting import tree_table
    crow, col, val = _csr_rows()
    if cosine:
        inside = np.where(col < D_CSR, val, 0.0)
        nrm = np.sqrt(np.add.reduceat(np.append(inside * inside, 0.0), crow[:-1]) * (np.diff(crow) > 0))
        val = val / np.where(nrm > 0, nrm, 1.0)[np.repeat(np.arange(N), np.diff(crow))]
    centers = BH.heap_tree(D_CSR, cosine)
    table = tree_table(centers, list(range(1, 32)), cosine, "cuda")
    BH.check_table(table)
    ref = BH.CsrRef(crow, col, val, D_CSR)
    # an empty row has the projection 0 exactly in every order (and ties under COSINE): it is held to the
    # reference's side, not to a distance from the plane
    rows_with = [i for i in range(N) if crow[i + 1] > crow[i]]
    pl = BH.planes(centers, table, cosine)
    sep = min(BH.side(ref, i, q, cosine)[1] for i in rows_with for q in pl)
    print("csr separation", "COSINE" if cosine else "EUCLIDEAN", sep, "bounds")
    assert sep > 2.0
    start = BH.start_slots(9)
    one = BH.reference_descend(ref, centers, table, start, 1, cosine)
    full = BH.reference_descend(ref, centers, table, np.zeros(N, np.int32), 4, cosine)
    return crow, col, val, table, start, one, full


@pytest.mark.parametrize("col_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("cosine", [False, True])
def test_descend_csr(cosine, col_dtype):
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import bisecting as bops
    from alink_amd.ops.kmeans_rows import _SparseRows, rows
    crow, col, val, table, start, one, full = _csr_case(cosine)
    fm = FeatureMatrix(crow=torch.from_numpy(crow).cuda(), col=torch.from_numpy(col).to("cuda", col_dtype),
                       val=torch.from_numpy(val).cuda(), ncols=D_CSR)
    r = rows(fm, "COSINE" if cosine else "EUCLIDEAN")
    assert type(r) is _SparseRows and r.d == D_CSR
    s1, s4 = _slots(start), _slots(np.zeros(N))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    calls = bops.BISECT_CALLS
    got = r.descend(table, s1, 1)
    got4 = r.descend(table, s4, 4)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert bops.BISECT_CALLS == calls + 2
    print("csr descend peak rise", rise / MIB, "MiB")
    assert rise < 64 * MIB                                  # the dense matrix would be 2 GiB
    assert got.data_ptr() == s1.data_ptr()
    assert np.array_equal(got.cpu().numpy(), one)
    keep = (start < 0) | (start >= 15)
    assert np.array_equal(got.cpu().numpy()[keep], start[keep])
    assert np.array_equal(got4.cpu().numpy(), full)
    for grid in (1, 7):
        assert torch.equal(r.descend(table, _slots(start), 1, grid=grid), got)
        assert torch.equal(r.descend(table, _slots(np.zeros(N)), 4, grid=grid), got4)


def _stats_slots(n, nslots):
    """Slots for ``child_stats``: 100 rows without one (-1), child 2 with more than 2 ACCUM_ROWS rows (three
    chunks), child 4 empty, the other rows spread over children 0, 1, 3, 5."""
    rng = np.random.default_rng(8)
    slot = np.full(n, 2, dtype=np.int32)
    perm = rng.permutation(n)
    slot[perm[:100]] = -1
    slot[perm[100:102]] = nslots + 3                        # past the last child: ignored as well
    rest = perm[102:102 + 12]
    slot[rest] = np.array([0, 1, 3, 5])[np.arange(12) % 4]
    return slot


def _stats_reference(X, slot, nslots):
    ok = (slot >= 0) & (slot < nslots)
    idx = torch.from_numpy(slot[ok].astype(np.int64))
    Xt = torch.from_numpy(X[ok])
    d = X.shape[1]
    ref = torch.zeros((nslots, d + 2), dtype=torch.float64)
    ref[:, :d].index_add_(0, idx, Xt)
    ref[:, d] = torch.bincount(idx, minlength=nslots).to(torch.float64)
    ref[:, d + 1].index_add_(0, idx, (Xt * Xt).sum(1))
    sabs = torch.zeros((nslots, d + 2), dtype=torch.float64)
    sabs[:, :d].index_add_(0, idx, Xt.abs())
    sabs[:, d + 1].index_add_(0, idx, (Xt * Xt).sum(1))
    # a child sum has count terms; sum |x|^2 has count terms that are themselves sums of d terms
    m = ref[:, d][:, None].repeat(1, d + 2)
    m[:, d + 1] += float(d)
    return ref, 4.0 * 2.0 * m * EPS * sabs, int(ok.sum())


def _check_stats(r, X, slot, nslots, integer):
    d = X.shape[1]
    ref, bound, inside = _stats_reference(np.nan_to_num(X), slot, nslots)
    sg = _slots(slot)
    buf = r.child_stats(sg, nslots)
    assert buf.shape == (nslots, d + 2) and buf.dtype == torch.float64
    got = buf.cpu()
    assert torch.equal(got[:, d], ref[:, d]) and float(got[:, d].sum()) == inside      # ignored rows: nowhere
    assert float(got[4].abs().sum()) == 0.0                                            # the empty child
    if integer:
        assert torch.equal(got, ref)
    else:
        print("child_stats max error / bound", float(((got - ref).abs() / bound.clamp_min(1e-300)).max()))
        assert bool(((got - ref).abs() <= bound).all())
    assert torch.equal(r.child_stats(sg, nslots), buf)                      # launch to launch
    for grid in (1, 7):                                                     # and for every grid
        assert torch.equal(r.child_stats(sg, nslots, grid=grid), buf)
    nosq = r.child_stats(sg, nslots, sqnorm=False)
    assert torch.equal(nosq[:, :d + 1], buf[:, :d + 1])


@pytest.mark.parametrize("integer", [True, False])
def test_child_stats_dense(integer):
    from alink_amd.ops import kmeans_dense64 as kd
    d, nslots = 131, 6
    n = 2 * kd.ACCUM_ROWS + 17 + 100
    rng = np.random.default_rng(5 + int(integer))
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float64) if integer else rng.normal(size=(n, d))
    slot = _stats_slots(n, nslots)
    assert 2 * kd.ACCUM_ROWS < int((slot == 2).sum()) <= 3 * kd.ACCUM_ROWS and int((slot == -1).sum()) == 100
    X[(slot < 0) | (slot >= nslots)] = np.nan               # a row without a slot is not read: a NaN would show
    calls = kd.DENSE64_CALLS
    _check_stats(_rows(torch.from_numpy(X).cuda(), False), X, slot, nslots, integer)
    assert kd.DENSE64_CALLS > calls


@pytest.mark.parametrize("integer", [True, False])
def test_child_stats_csr(integer):
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import kmeans_dense64 as kd, kmeans_sparse as ksp
    from alink_amd.ops.kmeans_rows import _SparseRows, rows
    d, nslots = 40, 6
    n = 2 * kd.ACCUM_ROWS + 17 + 100
    rng = np.random.default_rng(15 + int(integer))
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float64) if integer else rng.normal(size=(n, d))
    X[rng.random((n, d)) < 0.6] = 0.0
    X[:, 0] = 1.0 + np.arange(n) % 3                        # column 0 holds n > ACCUM_CHUNK entries
    assert n > ksp.ACCUM_CHUNK
    slot = _stats_slots(n, nslots)
    nz = X != 0
    crow = np.zeros(n + 1, np.int64)
    crow[1:] = np.cumsum(nz.sum(1))
    fm = FeatureMatrix(crow=torch.from_numpy(crow).cuda(), col=torch.from_numpy(np.nonzero(nz)[1]).cuda(),
                       val=torch.from_numpy(X[nz]).cuda(), ncols=d)
    r = rows(fm, "EUCLIDEAN")
    assert type(r) is _SparseRows
    calls = ksp.SPARSE_CALLS
    _check_stats(r, X, slot, nslots, integer)
    assert ksp.SPARSE_CALLS > calls


def test_no_n_by_m_buffer():
    from alink_amd.ops.bisecting import tree_table
    n, d, m = 2 ** 18, 8, 64
    rng = np.random.default_rng(2)
    centers = {c: rng.normal(size=d) for c in range(64, 256)}      # 64 dividing nodes 64 .. 127 and their children
    split = list(range(64, 128))
    table = tree_table(centers, split + [x for c in split for x in (2 * c, 2 * c + 1)], False, "cuda")
    assert table.P == m and table.S == 3 * m
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((n, d), dtype=torch.float64, device="cuda", generator=g)
    r = _rows(X, False)
    r.row_sqnorm()                                          # once per run, as in training
    slot = torch.randint(0, m, (n,), device="cuda", generator=g).to(torch.int32)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    slot = r.descend(table, slot, 1)
    stats = r.child_stats(slot - m, 2 * m)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("descend + child_stats peak rise", rise / MIB, "MiB")
    assert rise < 64 * MIB                  # the one-hot [n, 2m] of the torch chain alone is 256 MiB
    assert stats.shape == (2 * m, d + 2) and float(stats[:, d].sum()) == n


def _model(rows):
    from alink_amd.common.model.converter import SimpleModelDataConverter
    _, data = SimpleModelDataConverter.split_rows(rows)
    nodes = [json.loads(s) for s in data]
    return ([(s["clusterId"], s["size"]) for s in nodes], np.array([s["center"]["data"] for s in nodes]))


@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
def test_train_matches_cpu(dist):
    from alink_amd.ops import bisecting as bops
    X = BH.blobs()
    n = X.shape[0]
    calls = bops.BISECT_CALLS
    cpu = BH.train(X, dist, "cpu")
    assert bops.BISECT_CALLS == calls
    gpu = BH.train(X, dist, "cuda:0")
    assert bops.BISECT_CALLS > calls
    (ids_c, cen_c), (ids_g, cen_g) = _model(cpu), _model(gpu)
    assert ids_c == ids_g and len(ids_c) == 7               # node ids and sizes
    # a centre coordinate is a mean of at most n terms of size <= max|x| (or that mean normalised): two fp64
    # evaluations differ by at most 2 n 2^-53 max|x|; 4x that (the rule of test_kmeans_dense64_gpu.py)
    atol = 4.0 * 2.0 * n * EPS * max(1.0, float(np.abs(X).max()))
    print("train", dist, "max centre difference", float(np.abs(cen_c - cen_g).max()), "atol", atol)
    assert np.abs(cen_c - cen_g).max() <= atol
    again = BH.train(X, dist, "cuda:0")
    assert [tuple(r) for r in again] == [tuple(r) for r in gpu]             # byte-identical model rows


@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
def test_train_sparse_column(dist):
    """The blobs as a sparse vector column under vectorSize = 2^18: CSR rows all the way, never an [n, 2^18] matrix
    (1.2 GiB).  What the run does allocate at this size is the CSC accumulate's transposed sums [2^18, 64] fp64 =
    128 MiB and the [2m + 1, 2^18 + 2] statistics beside it, so the peak is held under 512 MiB."""
    from alink_amd.ops import bisecting as bops, kmeans_sparse as ksp
    X = BH.blobs()
    cpu = BH.train(X, dist, "cpu", sparse_size=D_CSR, max_iter=3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    calls, scalls = bops.BISECT_CALLS, ksp.SPARSE_CALLS
    gpu = BH.train(X, dist, "cuda:0", sparse_size=D_CSR, max_iter=3)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("sparse train peak rise", rise / MIB, "MiB")
    assert rise < 512 * MIB
    assert bops.BISECT_CALLS > calls and ksp.SPARSE_CALLS > scalls
    assert _model(cpu)[0] == _model(gpu)[0] and len(_model(gpu)[0]) == 7


def _predict(model_table, col):
    from alink_amd import BisectingKMeansPredictBatchOp
    from alink_amd.common.table import MTable
    from alink_amd.common.types import TableSchema
    from alink_amd.operator.batch.source import TableSourceBatchOp
    src = TableSourceBatchOp(MTable(TableSchema(["v"], [col[0]]), [col[1]]))
    op = BisectingKMeansPredictBatchOp().setPredictionCol("p").setReservedCols([])
    return op.linkFrom(TableSourceBatchOp(model_table), src).getOutputTable().col("p").to_list()


@pytest.mark.parametrize("dist", ["EUCLIDEAN", "COSINE"])
def test_predict_device_columns(dist, monkeypatch):
    from alink_amd import useLocalEnv
    from alink_amd.common.linalg.block import SparseBlock
    from alink_amd.common.model.converter import SimpleModelDataConverter
    from alink_amd.common.table import Column, MTable
    from alink_amd.common.types import Types
    from alink_amd.ops import bisecting as bops
    monkeypatch.delenv("ALINK_KMEANS_DENSE64", raising=False)
    monkeypatch.delenv("ALINK_KMEANS_SPARSE", raising=False)
    X = BH.blobs()
    n, d = X.shape
    model = MTable.from_rows(BH.train(X, dist, "cpu"), SimpleModelDataConverter().getModelSchema(), replicated=True)
    Xt = torch.from_numpy(X)
    useLocalEnv(1, device="cpu")
    cpu = _predict(model, (Types.DENSE_VECTOR, Column(Xt)))
    assert len(set(cpu)) == 4
    useLocalEnv(1, device="cuda:0")
    calls = bops.BISECT_CALLS
    assert _predict(model, (Types.DENSE_VECTOR, Column(Xt.cuda()))) == cpu
    assert bops.BISECT_CALLS == calls + 1                   # one descend launch over the whole tree
    # a sparse block on the device, taken as CSR (ALINK_KMEANS_SPARSE=1 takes every sparse column)
    monkeypatch.setenv("ALINK_KMEANS_SPARSE", "1")
    blk = SparseBlock(torch.arange(n + 1, dtype=torch.int64) * d, torch.arange(d, dtype=torch.int64).repeat(n),
                      torch.from_numpy(X.reshape(-1).copy()), d)
    calls = bops.BISECT_CALLS
    assert _predict(model, (Types.SPARSE_VECTOR, Column(blk.to("cuda:0")))) == cpu
    assert bops.BISECT_CALLS == calls + 1
    monkeypatch.delenv("ALINK_KMEANS_SPARSE")
    monkeypatch.setenv("ALINK_KMEANS_DENSE64", "0")         # the torch kind: no launch, the same clusters
    calls = bops.BISECT_CALLS
    assert _predict(model, (Types.DENSE_VECTOR, Column(Xt.cuda()))) == cpu
    assert bops.BISECT_CALLS == calls


def test_empty_partition():
    from alink_amd.models.common.features import FeatureMatrix
    from alink_amd.ops import bisecting as bops, kmeans_dense64 as kd, kmeans_sparse as ksp
    from alink_amd.ops.kmeans_rows import rows
    d = 37
    X, centers, table, start, one, full = BH.descend_case(d, False, "cuda")
    calls = (bops.BISECT_CALLS, kd.DENSE64_CALLS, ksp.SPARSE_CALLS)
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    z = torch.zeros(0, dtype=torch.int64, device="cuda")
    fm = FeatureMatrix(crow=torch.zeros(1, dtype=torch.int64, device="cuda"), col=z,
                       val=torch.zeros(0, dtype=torch.float64, device="cuda"), ncols=d)
    for r in (rows(torch.zeros((0, d), dtype=torch.float64, device="cuda"), "EUCLIDEAN"), rows(fm, "EUCLIDEAN")):
        assert r.descend(table, empty, 4).shape == (0,)
        assert torch.equal(r.child_stats(empty, 6), torch.zeros((6, d + 2), dtype=torch.float64, device="cuda"))
    assert bops.descend_f64(torch.zeros((0, d), dtype=torch.float64, device="cuda"), table, empty, 4).shape == (0,)
    assert (bops.BISECT_CALLS, kd.DENSE64_CALLS, ksp.SPARSE_CALLS) == calls     # n = 0: nothing is launched
