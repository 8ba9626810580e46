"""Association rules, sequential patterns, outlier selection and LSH similarity batch ops.

Reference: ``A/operator/batch/associationrule/{FpGrowthBatchOp,PrefixSpanBatchOp}.java`` (output = patterns,
side output 0 = rules), ``A/operator/batch/outlier/SosBatchOp.java``,
``A/operator/batch/similarity/{ApproxVectorSimilarityJoinLSHBatchOp,ApproxVectorSimilarityTopNLSHBatchOp}.java``.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from ...common.linalg import VectorUtil
from ...common.table import Column, MTable
from ...common.types import TableSchema, Types
from ...models.associationrule import mining as M
from ...models.outlier.sos import sos_scores
from ...models.similarity import lsh as L
from ...ops import lsh as K
from ...parallel import comm
from ..base import BatchOperator, gather_table, partition_bounds

__all__ = ["FpGrowthBatchOp", "PrefixSpanBatchOp", "SosBatchOp", "ApproxVectorSimilarityJoinLSHBatchOp",
           "ApproxVectorSimilarityTopNLSHBatchOp"]

ITEM_SEP, ELEMENT_SEP, RULE_SEP = ",", ";", "=>"


def _own_block(rows, schema, env, replicated_in):
    mt = MTable.from_rows(rows, schema)
    if comm.get_world_size() > 1 and not replicated_in:
        lo, hi = partition_bounds(mt.num_rows, env)
        mt = mt.slice(lo, hi)
    return mt


def _fpgrowth_device_rows(mt, p, device, backend=None):
    """``(patterns columns, rule rows)`` of ``FpGrowthBatchOp`` through ``M.fp_growth_device`` on ``device``, or None
    when the rows send the operator down the host path.  The patterns come as columns (itemset strings assembled from
    the names' bytes, no per-pattern Python); the rules are ``M.association_rules`` on a dict built from them."""
    from ...common.strings import StringBlock
    from ...models.nlp.text import _string_block
    from ...ops.strings import join_tokens
    res = M.fp_growth_device(_string_block(mt, p.get("itemsCol"), device), int(p.get("minSupportCount")),
                             float(p.get("minSupportPercent")), int(p.get("maxPatternLength")), backend=backend)
    if res is None:
        return None
    names, (items, lens, sups), n, _ = res
    dev = items.device
    P = int(lens.numel())
    if P:
        tok = StringBlock.from_list(names, device=dev).take(items.to(torch.int64))
        doc = torch.repeat_interleave(torch.arange(P, device=dev), lens, output_size=int(items.numel()))
        sets = join_tokens(tok, doc, torch.ones(int(items.numel()), dtype=torch.bool, device=dev), P,
                           sep=ord(ITEM_SEP)).to("cpu")
    else:
        sets = StringBlock.empty()
    pcols = [Column(sets), Column(sups.cpu()), Column(lens.cpu())]
    pats = M.patterns_dict((items, lens, sups))
    rules = M.association_rules(pats, n, float(p.get("minConfidence")), float(p.get("minLift")),
                                int(p.get("maxConsequentLength")))
    rules.sort(key=lambda r: (len(r[0]) + len(r[1]), r[0], r[1]))
    rrow = [(ITEM_SEP.join(names[i] for i in a) + RULE_SEP + ITEM_SEP.join(names[i] for i in c), len(a) + len(c),
             float(lift), float(sup), float(conf), int(cnt)) for a, c, cnt, lift, sup, conf in rules]
    return pcols, rrow


class FpGrowthBatchOp(BatchOperator):
    """Frequent itemsets (output) and association rules (side output 0).  On a GPU the itemsets are mined by
    ``M.fp_growth_device`` (``ops.fpm.device_selected``; ``ALINK_FPGROWTH_HIP=0`` turns it off); the host path below
    is the CPU path and the fallback for rows the device path cannot decide."""

    PATTERN_SCHEMA = "itemset string, supportcount bigint, itemcount bigint"
    RULE_SCHEMA = ("rule string, itemcount bigint, lift double, support_percent double, confidence_percent double, "
                   "transaction_count bigint")

    def linkFrom(self, *inputs):
        mt = self.checkAndGetFirst(inputs).getOutputTable()
        p = self.resolvedParams()
        from ...ops import fpm as FPM
        n_rows = mt.num_rows
        if comm.get_world_size() > 1 and torch.device(self.env.device).type == "cuda":
            n_rows = sum(comm.all_gather_object(n_rows))        # every rank takes the same path
        if FPM.device_selected(self.env.device, n_rows):
            res = _fpgrowth_device_rows(mt, p, self.env.device)
            if res is not None:         # None: rows that cannot be decided from bytes take the host path below
                from ...common.table import schema_str_to_schema
                pcols, rrow = res
                rep = mt.replicated
                out = MTable(schema_str_to_schema(self.PATTERN_SCHEMA), pcols)
                if comm.get_world_size() > 1 and not rep:
                    out = out.slice(*partition_bounds(out.num_rows, self.env))
                self.setOutputTable(out)
                self.setSideOutputTables([_own_block(rrow, self.RULE_SCHEMA, self.env, rep)])
                return self
        items = mt.col(p.get("itemsCol")).to_list()
        tx = [s.split(ITEM_SEP) if s is not None and s.strip() else [] for s in items]
        names, pats, n, _ = M.fp_growth(tx, int(p.get("minSupportCount")), float(p.get("minSupportPercent")),
                                        int(p.get("maxPatternLength")))
        order = sorted(pats, key=lambda t: (len(t), t))
        prow = [(ITEM_SEP.join(names[i] for i in pat), int(pats[pat]), len(pat)) for pat in order]
        rules = M.association_rules(pats, n, float(p.get("minConfidence")), float(p.get("minLift")),
                                    int(p.get("maxConsequentLength")))
        rules.sort(key=lambda r: (len(r[0]) + len(r[1]), r[0], r[1]))
        rrow = [(ITEM_SEP.join(names[i] for i in a) + RULE_SEP + ITEM_SEP.join(names[i] for i in c), len(a) + len(c),
                 float(lift), float(sup), float(conf), int(cnt)) for a, c, cnt, lift, sup, conf in rules]
        rep = mt.replicated
        self.setOutputTable(_own_block(prow, "itemset string, supportcount bigint, itemcount bigint", self.env, rep))
        self.setSideOutputTables([_own_block(
            rrow, "rule string, itemcount bigint, lift double, support_percent double, confidence_percent double, "
                  "transaction_count bigint", self.env, rep)])
        return self


def _encode_seq(names, elements) -> str:
    return ELEMENT_SEP.join(ITEM_SEP.join(names[i] for i in el) for el in elements)


def _prefixspan_device_patterns(mt, p, device, backend=None):
    """``(names, patterns dict, N)`` as ``M.prefix_span`` gives them, through ``M.prefix_span_device`` on ``device``,
    or None when the rows send the operator down the host path."""
    from ...models.nlp.text import _string_block
    from ...ops import prefixspan as SPM
    res = M.prefix_span_device(_string_block(mt, p.get("itemsCol"), device), int(p.get("minSupportCount")),
                               float(p.get("minSupportPercent")), int(p.get("maxPatternLength")), backend=backend)
    if res is None:
        return None
    names, cols, n = res
    return names, SPM.decode(cols), n


class PrefixSpanBatchOp(BatchOperator):
    """Sequential patterns (output) and sequence rules (side output 0).  On a GPU the patterns are mined by
    ``M.prefix_span_device`` (``ops.prefixspan.device_selected``; ``ALINK_PREFIXSPAN_HIP=0`` turns it off); the host
    path is the CPU path and the fallback for columns the device path declines.  Rows, order and strings are built
    from the pattern dict by the same code on both paths."""

    def linkFrom(self, *inputs):
        mt = self.checkAndGetFirst(inputs).getOutputTable()
        p = self.resolvedParams()
        from ...ops import prefixspan as SPM
        n_rows = mt.num_rows
        if comm.get_world_size() > 1 and torch.device(self.env.device).type == "cuda":
            n_rows = sum(comm.all_gather_object(n_rows))        # every rank takes the same path
        res = None
        if SPM.device_selected(self.env.device, n_rows):
            res = _prefixspan_device_patterns(mt, p, self.env.device)
        if res is None:                 # not selected, or a column the device path declines
            seqs = []
            for s in mt.col(p.get("itemsCol")).to_list():
                if s is None or not s.strip():
                    seqs.append([])
                    continue
                seqs.append([el.strip().split(ITEM_SEP) for el in s.split(ELEMENT_SEP)])
            res = M.prefix_span(seqs, int(p.get("minSupportCount")), float(p.get("minSupportPercent")),
                                int(p.get("maxPatternLength")))
        names, pats, n = res
        order = sorted(pats, key=lambda t: (sum(len(e) for e in t), t))
        prow = [(_encode_seq(names, pat), int(pats[pat]), sum(len(e) for e in pat)) for pat in order]
        rules = M.sequence_rules(pats, n, float(p.get("minConfidence")))
        rules.sort(key=lambda r: (len(r[0]) + 1, r[0], r[1]))
        rrow = [(_encode_seq(names, a) + RULE_SEP + _encode_seq(names, c), len(a) + len(c), float(sup), float(conf),
                 int(cnt)) for a, c, cnt, sup, conf in rules]
        rep = mt.replicated
        self.setOutputTable(_own_block(prow, "itemset string, supportcount bigint, itemcount bigint", self.env, rep))
        self.setSideOutputTables([_own_block(
            rrow, "rule string, chain_length bigint, support double, confidence double, transaction_count bigint",
            self.env, rep)])
        return self


def _dense_block(values, device) -> torch.Tensor:
    vecs = [VectorUtil.getVector(v) for v in values]
    d = max((v.size() for v in vecs), default=0)
    X = np.zeros((len(vecs), d))
    for i, v in enumerate(vecs):
        X[i] = v.toDense().getData()[:d] if v.size() == d else np.pad(v.toDense().getData(), (0, d - v.size()))
    return torch.as_tensor(X, device=device)


def _sos_device_block(table, col, device):
    """The vector column as fp64 rows on a GPU device without a pass through Python vectors: a dense block as it
    is, a CSR block at most ``ops.sos.SOS_DMAX`` wide densified on the device.  None for CPU devices, fp32 blocks,
    wider sparse columns and ``ALINK_SOS_HIP=0``: those keep ``_dense_block``."""
    from ...common.linalg import SparseBlock
    from ...ops import sos as S
    if torch.device(device).type != "cuda" or os.environ.get("ALINK_SOS_HIP", "") == "0":
        return None
    v = table.col(col).values
    if isinstance(v, SparseBlock):
        if v.size > S.SOS_DMAX:
            return None
    elif isinstance(v, torch.Tensor) and v.dim() == 2:
        if v.dtype != torch.float64:
            return None
    fm = _lsh_columns(table, col, device)
    if fm.is_sparse and fm.ncols > S.SOS_DMAX:
        return None
    return fm.to_dense().contiguous()


class SosBatchOp(BatchOperator):
    """Outlier probability per row; the n x n affinity work is split by row blocks across ranks and the
    per-column log-products are all-reduced."""

    def linkFrom(self, *inputs):
        mt = self.checkAndGetFirst(inputs).getOutputTable()
        p = self.resolvedParams()
        full = gather_table(mt)
        X = _sos_device_block(full, p.get("vectorCol"), self.env.device)
        if X is None:
            X = _dense_block(full.col(p.get("vectorCol")).to_list(), self.env.device)
        scores = sos_scores(X, float(p.get("perplexity")))
        lo, hi = (0, full.num_rows) if mt.replicated or comm.get_world_size() == 1 else \
            partition_bounds(full.num_rows, self.env)
        own = full.slice(lo, hi) if (lo, hi) != (0, full.num_rows) else full
        out = own.with_columns([p.get("predictionCol")], [Types.DOUBLE], [Column(scores[lo:hi].cpu())])
        # each rank keeps its own row block of the gathered table: a partitioned output (collect gathers it)
        out.replicated = bool(mt.replicated or comm.get_world_size() == 1)
        self.setOutputTable(out)
        return self


def _lsh_args(p):
    dt = p.get("distanceType")
    return (getattr(dt, "name", str(dt)), int(p.get("seed")), int(p.get("numProjectionsPerTable")),
            int(p.get("numHashTables")), float(p.get("projectionWidth")))


def _own_columns(schema, cols, env):
    """``_own_block`` for an output that is already columns (the device path: no per-row Python tuples)."""
    mt = MTable(schema, cols)
    if comm.get_world_size() > 1:
        lo, hi = partition_bounds(mt.num_rows, env)
        mt = mt.slice(lo, hi)
    return mt


def _lsh_columns(table, col, device):
    from ...models.common.features import extract_features
    return extract_features(table, None, col, device)


class ApproxVectorSimilarityJoinLSHBatchOp(BatchOperator):
    def linkFrom(self, *inputs):
        self.checkOpSize(2, inputs)
        p = self.resolvedParams()
        left, right = gather_table(inputs[0].getOutputTable()), gather_table(inputs[1].getOutputTable())
        lid, rid = p.get("leftIdCol"), p.get("rightIdCol")
        if K.device_selected(self.env.device):
            dev = self.env.device
            res = L.approx_similarity_join_columns(
                _lsh_columns(left, p.get("leftCol"), dev), _lsh_columns(right, p.get("rightCol"), dev),
                *_lsh_args(p), float(p.get("distanceThreshold")))
            if res is not None:         # None: rows that are not device-eligible take the host path below
                ai, bi, d = res
                ln, rn = (lid + "_left", rid + "_right") if lid.lower() == rid.lower() else (lid, rid)
                dcol = p.get("outputCol") if p.contains("outputCol") and p.get("outputCol") else "distance"
                schema = TableSchema([ln, rn, dcol], [left.col_type(lid), right.col_type(rid), Types.DOUBLE])
                self.setOutputTable(_own_columns(
                    schema, [left.col(lid).take(ai), right.col(rid).take(bi), Column(d.cpu())], self.env))
                return self
        res = L.approx_similarity_join(left.col(p.get("leftCol")).to_list(), right.col(p.get("rightCol")).to_list(),
                                       *_lsh_args(p), float(p.get("distanceThreshold")), self.env.device)
        lids, rids = left.col(lid).to_list(), right.col(rid).to_list()
        ln, rn = (lid + "_left", rid + "_right") if lid.lower() == rid.lower() else (lid, rid)
        dcol = p.get("outputCol") if p.contains("outputCol") and p.get("outputCol") else "distance"
        schema = TableSchema([ln, rn, dcol], [left.col_type(lid), right.col_type(rid), Types.DOUBLE])
        rows = [(lids[a], rids[b], d) for a, b, d in res]
        self.setOutputTable(_own_block(rows, schema, self.env, False))
        return self


class ApproxVectorSimilarityTopNLSHBatchOp(BatchOperator):
    def linkFrom(self, *inputs):
        self.checkOpSize(2, inputs)
        p = self.resolvedParams()
        left, right = gather_table(inputs[0].getOutputTable()), gather_table(inputs[1].getOutputTable())
        lid, rid = p.get("leftIdCol"), p.get("rightIdCol")
        if K.device_selected(self.env.device):
            dev = self.env.device
            dict_fm = _lsh_columns(left, p.get("leftCol"), dev)         # the left table is the dictionary and basis
            res = L.approx_nearest_neighbors_columns(_lsh_columns(right, p.get("rightCol"), dev), dict_fm,
                                                     *_lsh_args(p), int(p.get("topN")), dict_fm.ncols)
            if res is not None:         # None: rows that are not device-eligible take the host path below
                qi, di, d, rank = res
                ln, rn = (lid + "_left", rid + "_right") if lid.lower() == rid.lower() else (lid, rid)
                dcol = p.get("outputCol") if p.contains("outputCol") and p.get("outputCol") else "distance"
                schema = TableSchema([rn, ln, dcol, "rank"], [right.col_type(rid), left.col_type(lid), Types.DOUBLE,
                                                             Types.LONG])
                self.setOutputTable(_own_columns(
                    schema, [right.col(rid).take(qi), left.col(lid).take(di), Column(d.cpu()),
                             Column(rank.to(torch.int64).cpu())], self.env))
                return self
        lv = left.col(p.get("leftCol")).to_list()
        res = L.approx_nearest_neighbors(right.col(p.get("rightCol")).to_list(), lv, *_lsh_args(p),
                                         int(p.get("topN")), self.env.device, lsh_basis_vecs=lv)
        lids, rids = left.col(lid).to_list(), right.col(rid).to_list()
        ln, rn = (lid + "_left", rid + "_right") if lid.lower() == rid.lower() else (lid, rid)
        dcol = p.get("outputCol") if p.contains("outputCol") and p.get("outputCol") else "distance"
        schema = TableSchema([rn, ln, dcol, "rank"], [right.col_type(rid), left.col_type(lid), Types.DOUBLE,
                                                     Types.LONG])
        rows = [(rids[q], lids[d], dist, rank) for q, d, dist, rank in res]
        self.setOutputTable(_own_block(rows, schema, self.env, False))
        return self
