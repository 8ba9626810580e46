"""Bisecting k-means (reference ``A/operator/batch/clustering/BisectingKMeansTrainBatchOp.java``,
``A/operator/common/clustering/BisectingKMeansModel{Data,DataConverter,Mapper}.java``).

Semantics kept: clusters are nodes of a binary tree (root 1, children ``2i`` / ``2i + 1``); every bisecting
step splits the leaves with ``size > max(1, minDivisibleClusterSize)`` of largest cost (as many as needed to
reach ``k`` leaves), the two children start at ``c -/+ noise`` (``noise_j = 1e-4 |c| U[0,1)``, drawn with
``java.util.Random(0)``), and ``maxIter`` 2-means iterations move them (Euclidean: the half-space of the
middle plane ``x.(r - l) < (r + l)/2.(r - l)``; cosine: nearest child).  Cluster summaries hold ``size``,
``center`` and ``cost`` (``sum |x|^2 - n |c|^2``, or ``n - c.sum/|c|`` for cosine).  Prediction descends the
tree; leaves are numbered in BFS order and the detail vector turns tree distances into probabilities
(``KMeansUtil.getProbArrayFromDistanceArray``).

MI355X design: the samples stay on the device as the rows object of ``ops/kmeans_rows.py`` (fp64 rows or CSR rows
that are never densified, normalised once for COSINE) with an int32 tree slot per row; an inner iteration is one
``descend`` (``ops/csrc/bisecting.hip``: every row against the plane of its own node, one pass over the rows) and
one ``child_stats`` (the exact sort-based sums of the KMeans kernels, no float atomics), then one all-reduce of
``[#children, d + 2]`` statistics.  Prediction is one ``descend`` launch over the whole tree.  CPU rows and the
other row kinds keep the torch arithmetic (a projection on every dividing plane, a one-hot GEMM).
"""
from __future__ import annotations

import json
from typing import Dict, List

import numpy as np
import torch

from ...ops import bisecting as bops, kmeans_rows as krows
from ...common.javafmt import gson_dumps
from ...common.jrandom import JavaRandom
from ...common.linalg import DenseVector
from ...common.mapper import RichModelMapper
from ...common.model.converter import SimpleModelDataConverter
from ...common.params import Params
from ...common.table import Column, MTable
from ...common.types import Types
from ...parallel import comm
from ..common.features import extract_features, global_vector_size

__all__ = ["train_bisecting_kmeans", "BisectingKMeansModelMapper"]


def _pget(p: Params, name, default=None):
    try:
        if p.contains(name):
            v = p.get(name)
            return default if v is None else v
    except KeyError:
        pass
    return default


class _Summary:
    __gson_fields__ = ("clusterId", "size", "center", "cost")

    def __init__(self, cid, size, center, cost):
        self.clusterId, self.size, self.center, self.cost = int(cid), int(size), center, float(cost)


def _summaries(stats: torch.Tensor, ids: List[int], cosine: bool):
    """Global (size, center, cost) per tree node in ``ids`` from this rank's ``[len(ids), d + 2]`` statistics
    ``[sum_x | count | sum |x|^2]`` (``Rows.child_stats``)."""
    d = stats.shape[1] - 2
    comm.all_reduce(stats, "sum")
    out = {}
    S = stats.cpu().numpy()
    for i, cid in enumerate(ids):
        s, cnt, ss = S[i, :d], S[i, d], S[i, d + 1]
        c = s / cnt if cnt > 0 else np.zeros(d)
        if cosine and cnt > 0:
            c = c / np.sqrt(c @ c)
            cost = max(cnt - (c @ s) / np.sqrt(c @ c), 0.0)
        else:
            cost = max(ss - cnt * (c @ c), 0.0)
        out[cid] = (int(cnt), c, float(cost))
    return out


def _normalize_rows(X: torch.Tensor) -> torch.Tensor:
    return X / torch.sqrt((X * X).sum(1, keepdim=True))


def bisecting_rows(fm, d: int, dist: str):
    """One rank's rows for BisectingKMeans (training and prediction): CSR where ``sparse_selected`` takes the column,
    else a dense fp64 block under ``d`` columns; normalised once for COSINE."""
    if fm.is_sparse and krows.sparse_selected(True, d):
        return krows.rows(krows.sparse_rows(fm, d, dist), dist)
    if fm.is_sparse:
        fm.set_ncols(d)
    X = fm.to_dense().to(torch.float64)
    if X.shape[1] < d:
        X = torch.nn.functional.pad(X, (0, d - X.shape[1]))
    if dist == "COSINE":
        X = _normalize_rows(X)
    return krows.rows(X.contiguous(), dist)


def train_bisecting_kmeans(mt: MTable, params: Params, env) -> List[tuple]:
    dev = env.device
    vcol = params.get("vectorCol")
    k = int(_pget(params, "k", 4))
    max_iter = int(_pget(params, "maxIter", 10))
    min_div = int(_pget(params, "minDivisibleClusterSize", 1))
    dist = str(getattr(_pget(params, "distanceType", "EUCLIDEAN"), "name", _pget(params, "distanceType",
                                                                                "EUCLIDEAN"))).upper()
    cosine = dist == "COSINE"
    fm = extract_features(mt, None, vcol, dev)
    d = global_vector_size(fm)
    rows = bisecting_rows(fm, d, "COSINE" if cosine else "EUCLIDEAN")
    n = rows.n
    # a row's node is an index into ``nodes``, the list of every tree node so far (the host keeps the ids)
    nodes: List[int] = [1]
    node = torch.zeros(n, dtype=torch.int32, device=dev)
    summ: Dict[int, tuple] = _summaries(rows.child_stats(node, 1, sqnorm=not cosine), [1], cosine)
    rnd = JavaRandom(0)
    while True:
        ids = set(summ)
        leaves = [c for c in sorted(ids) if 2 * c not in ids and 2 * c + 1 not in ids]
        cand = [c for c in leaves if summ[c][0] > 1 and summ[c][0] > min_div]
        cand.sort(key=lambda c: -summ[c][2])          # stable: ties keep ascending id
        split = sorted(cand[:max(0, k - len(leaves))])
        if not split:
            break
        should_stop = len(split) + len(leaves) >= k
        centers = {}
        for c in split:
            ctr = summ[c][1]
            level = 1.0e-4 * np.sqrt(ctr @ ctr)
            noise = level * rnd.nextDoubles(d)
            centers[2 * c], centers[2 * c + 1] = ctr - noise, ctr + noise
        m = len(split)
        kids = [x for c in split for x in (2 * c, 2 * c + 1)]
        # this round's slots: the dividing nodes 0 .. m-1, then their children m .. 3m-1; every other row has -1
        to_slot = torch.full((len(nodes),), -1, dtype=torch.int32)
        for i, c in enumerate(split):
            to_slot[nodes.index(c)] = i
        start = to_slot.to(dev)[node.to(torch.int64)]
        slot, stats = start, None
        for it in range(max_iter):
            table = bops.tree_table(centers, split + kids, cosine, dev)
            slot = rows.descend(table, start.clone(), 1)
            # sum |x|^2 only feeds the EUCLIDEAN cost, which is read after the round's last iteration
            stats = rows.child_stats(slot - m, 2 * m, sqnorm=not cosine and it == max_iter - 1)
            s = _summaries(stats, kids, cosine)
            for cid in kids:
                if s[cid][0] > 0:
                    centers[cid] = s[cid][1]
        if max_iter < 1:
            s = _summaries(rows.child_stats(slot - m, 2 * m, sqnorm=not cosine), kids, cosine)
        summ.update(s)
        # the rows that moved now sit in a child: slot m + j is node ``kids[j]``
        first = len(nodes)
        nodes.extend(kids)
        node = torch.where(slot >= m, slot - m + first, node)
        if should_stop:
            break
    meta = Params().set("distanceType", dist).set("k", k).set("vectorSize", d).set("vectorCol", vcol)
    data = [gson_dumps(_Summary(cid, summ[cid][0], DenseVector(summ[cid][1]), summ[cid][2]), java_map_order=False)
            for cid in sorted(summ)]
    return SimpleModelDataConverter.rows_from(meta, data)


class BisectingKMeansModelMapper(RichModelMapper):
    def predResultType(self):
        return Types.LONG

    def loadModel(self, rows):
        meta, data = SimpleModelDataConverter.split_rows(rows)
        self.d = int(meta.get("vectorSize"))
        self.cosine = str(getattr(meta.get("distanceType"), "name", meta.get("distanceType"))).upper() == "COSINE"
        self.vcol = meta.get("vectorCol")
        self.centers = {int(s["clusterId"]): np.asarray(s["center"]["data"]) for s in map(json.loads, data)}
        order, queue = [], [1]
        while queue:                       # BFS leaf numbering
            c = queue.pop(0)
            kids = [x for x in (2 * c, 2 * c + 1) if x in self.centers]
            if not kids:
                order.append(c)
            queue.extend(kids)
        self.leaf_ids = order
        self.leaf_index = {c: i for i, c in enumerate(order)}
        self._tables = {}                   # the tree table per device, built on first use

    @staticmethod
    def _level(n):
        lv = 0
        while n > 1:
            n //= 2
            lv += 1
        return lv

    def _tree_dist(self, a, b):
        la, lb, dd = self._level(a), self._level(b), 0
        while la > lb:
            a //= 2
            la -= 1
            dd += 1
        while lb > la:
            b //= 2
            lb -= 1
            dd += 1
        while a != b:
            a //= 2
            b //= 2
            dd += 2
        return float(dd)

    def _leaf_of(self, x):
        c = 1
        while 2 * c in self.centers and 2 * c + 1 in self.centers:
            l, r = self.centers[2 * c], self.centers[2 * c + 1]
            if self.cosine:
                xn = x / np.sqrt(x @ x)
                left = (1 - xn @ (l / np.sqrt(l @ l))) < (1 - xn @ (r / np.sqrt(r @ r)))
            else:
                v, m = r - l, 0.5 * (r + l)
                left = x @ v < m @ v
            c = 2 * c if left else 2 * c + 1
        return c

    def _leaves_of(self, X: np.ndarray) -> np.ndarray:
        """``_leaf_of`` for every row at once: rows descend level by level, each internal node's rows split by
        one matrix-vector product (the row path's per-row dot to rounding)."""
        c = np.ones(X.shape[0], dtype=np.int64)
        while True:
            moved = False
            for node in np.unique(c).tolist():
                if not (2 * node in self.centers and 2 * node + 1 in self.centers):
                    continue
                rows = np.flatnonzero(c == node)
                x = X[rows]
                l, r = self.centers[2 * node], self.centers[2 * node + 1]
                if self.cosine:
                    xn = x / np.sqrt(np.einsum("ij,ij->i", x, x))[:, None]
                    left = (1 - xn @ (l / np.sqrt(l @ l))) < (1 - xn @ (r / np.sqrt(r @ r)))
                else:
                    v, m = r - l, 0.5 * (r + l)
                    left = x @ v < m @ v
                c[rows] = np.where(left, 2 * node, 2 * node + 1)
                moved = True
            if not moved:
                return c

    def _tree(self, dev):
        """(tree table, leaf slot -> BFS leaf index int64 [S]) on ``dev``, built once per loaded model and device."""
        cache, key = self._tables, str(dev)
        if key not in cache:
            order, queue = [], [1]
            while queue:                    # the nodes a row can reach from the root
                c = queue.pop(0)
                order.append(c)
                if 2 * c in self.centers and 2 * c + 1 in self.centers:
                    queue.extend((2 * c, 2 * c + 1))
            table = bops.tree_table(self.centers, order, self.cosine, dev)
            lut = torch.tensor([self.leaf_index.get(c, -1) for c in table.nodes], dtype=torch.int64)
            cache[key] = (table, lut.to(dev))
        return cache[key]

    def _leaves_device(self, fm) -> torch.Tensor:
        """BFS leaf index (int64 [n], on the device) of a device column: one ``descend`` over the whole tree."""
        dev = fm.device
        table, lut = self._tree(dev)
        rows = bisecting_rows(fm, self.d, "COSINE" if self.cosine else "EUCLIDEAN")
        slot = torch.full((rows.n,), table.slot_of[1], dtype=torch.int32, device=dev)
        return lut[rows.descend(table, slot, table.depth).to(torch.int64)]

    def _map_row_values(self, row):
        mt = MTable.from_rows([tuple(row)], self.dataSchema)
        return [c.to_list()[0] for c in self._map_columns(mt)]

    def _map_columns(self, mt):
        from ...common.linalg import VectorUtil
        vcol = self.params.get("vectorCol") if self.params.contains("vectorCol") and \
            self.params.get("vectorCol") else self.vcol
        from ..linear.model import _dev
        dev = _dev(mt)
        v = mt.col(vcol).values
        if not isinstance(v, torch.Tensor) and getattr(getattr(v, "val", None), "is_cuda", False):
            dev = v.val.device                      # a sparse block on the device
        if self.detail_col:
            dev = torch.device("cpu")
        fm = extract_features(mt, None, vcol, dev)
        if dev.type == "cuda":
            if (fm.ncols > self.d) if fm.is_sparse else (fm.ncols != self.d):
                raise RuntimeError(f"Dim of predict data not equal to vectorSize of training data: {self.d}")
            return [Column(self._leaves_device(fm).cpu())]
        if fm.is_sparse:
            fm.set_ncols(self.d)
        X = fm.to_dense().double()
        X = X.numpy()
        if X.shape[1] != self.d:
            raise RuntimeError(f"Dim of predict data not equal to vectorSize of training data: {self.d}")
        if not self.detail_col:
            leaves = self._leaves_of(X)
            ids = np.unique(leaves)
            idx = np.array([self.leaf_index[int(i)] for i in ids], dtype=np.int64)
            return [Column(torch.from_numpy(idx[np.searchsorted(ids, leaves)]))]
        preds, details = [], []
        nl = len(self.leaf_ids)
        for x in X:
            leaf = self._leaf_of(x)
            preds.append(self.leaf_index[leaf])
            if self.detail_col:
                dists = np.array([self._tree_dist(leaf, o) for o in self.leaf_ids])
                if nl > 1:
                    prob = np.full(nl, 1.0 / (nl - 1)) - dists / dists.sum() / (nl - 1)
                else:
                    prob = np.ones(1)
                details.append(VectorUtil.toString(DenseVector(prob)))
        cols = [Column.from_values(preds, Types.LONG)]
        if self.detail_col:
            cols.append(Column.from_values(details, Types.STRING))
        return cols
