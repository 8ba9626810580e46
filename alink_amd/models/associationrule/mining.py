"""Frequent-pattern mining: FP-Growth (itemsets + association rules) and PrefixSpan (sequential patterns +
sequence rules).

Reference: ``A/operator/batch/associationrule/FpGrowthBatchOp.java`` (item order = support desc, name asc
:153-178; min support count = ``floor(N * percent)`` unless given :268-281; pattern strings in item-index
order :283-320), ``A/operator/common/associationrule/{ParallelFpGrowth,FpTree,AssociationRule}.java``
(rules: ``lift = supXY*N/(supX*supY)``, ``lift >= minLift && confidence >= minConfidence``),
``PrefixSpanBatchOp.java`` (item support counted per occurrence :104-139, sequences encoded with 0 between
elements :166-203, ``encodeSequence`` :273-293), ``ParallelPrefixSpan.java``, ``SequenceRule.java``
(antecedent = all but the last element, consequent = last element).

Parallel scheme (PFP): transactions/sequences are encoded once, identical ones are de-duplicated with
counts, and the distinct encoded database is shared; rank r mines the patterns whose *last* item (FP-Growth:
the least frequent item of the pattern; PrefixSpan: the first item) belongs to its item group, and the
pattern lists are all-gathered — the same partition-by-item decomposition as the reference's parallel
FP-growth, with no pattern mined twice.

Device path (``fp_growth_device``, ``ops/fpm.py``): the same frequent itemsets counted level by level on vertical
bitmaps by HIP kernels.  Each rank keeps its own transactions; only the distinct items with their counts, and each
level's integer candidate counts, cross ranks.  ``fp_growth`` stays the CPU path, the fallback and the oracle.
Known difference: the device path splits the items column as Java's ``String.split`` does, which drops trailing empty
items (``"A,B,"`` holds A and B, as in the reference); ``FpGrowthBatchOp``'s host path uses Python's ``split``, which
keeps them (A, B and the empty item).

``prefix_span_device`` (``ops/prefixspan.py``) is the same for sequences: one bit field per sequence, S-step and
I-step support counts by ``alink_fpm_seq_counts``, candidates level by level.  It returns the pattern set and the
supports of ``prefix_span`` exactly, and declines (None) every column it cannot prove it parses as the host does;
``prefix_span`` stays the CPU path, the fallback and the oracle.
"""
from __future__ import annotations

import math
from collections import Counter, defaultdict
from typing import Dict, List, Sequence, Tuple

from ...parallel import comm

__all__ = ["fp_growth", "fp_growth_device", "patterns_dict", "association_rules", "prefix_span", "prefix_span_device",
           "sequence_rules"]


def _min_support(n: int, count: int, percent: float) -> int:
    return int(count) if count is not None and count >= 0 else int(math.floor(n * percent))


# ---------------------------------------------------------------------------------------------------
# shared by the two device paths
# ---------------------------------------------------------------------------------------------------
def _ascii_ws(d):
    """The bytes of ``d`` that are ASCII whitespace to Python's ``strip()``: 0x09-0x0d and 0x1c-0x20."""
    return ((d >= 0x09) & (d <= 0x0d)) | ((d >= 0x1c) & (d <= 0x20))


def _vote_items(undecided: bool, names_local, counts_local, n_local: int, min_support_count, min_support_percent):
    """The one ``all_gather_object`` of a device path: every rank's verdict, distinct items with their counts, and
    row count.  None when any rank is undecided; else ``(qualified, n, min_sup)``: the ``(item, count)`` over all
    ranks that reach the minimum support, by ``(-count, name)``, the rows of all ranks and the minimum support."""
    gathered = comm.all_gather_object((undecided, names_local, counts_local, n_local))
    if any(g[0] for g in gathered):
        return None
    counts = Counter()
    n = 0
    for _, nm, ct, nl in gathered:
        for k, c in zip(nm, ct):
            counts[k] += c
        n += nl
    min_sup = _min_support(n, min_support_count, min_support_percent)
    qualified = [(it, c) for it, c in counts.items() if c >= min_sup]
    qualified.sort(key=lambda t: (-t[1], t[0]))
    return qualified, n, min_sup


def _rank_lut(qualified, names_local, dev):
    """int64 [local ids]: the 0-based place of every local item among ``qualified``, -1 when it did not qualify."""
    import torch
    index = {it: i for i, (it, _) in enumerate(qualified)}
    return torch.tensor([index.get(s, -1) for s in names_local], dtype=torch.int64, device=dev)


# ---------------------------------------------------------------------------------------------------
# FP-Growth
# ---------------------------------------------------------------------------------------------------
def _mine(db: List[Tuple[Tuple[int, ...], int]], suffix: Tuple[int, ...], min_sup: int, max_len: int,
          out: Dict[Tuple[int, ...], int], allowed_last=None):
    """Conditional-pattern-base recursion.  ``db`` holds (sorted item tuple, count); patterns grow by
    prepending items that precede the current suffix in the global order."""
    counts = Counter()
    for items, c in db:
        for it in items:
            counts[it] += c
    for it, c in counts.items():
        if c < min_sup:
            continue
        if allowed_last is not None and it not in allowed_last:
            continue
        pat = (it,) + suffix
        out[pat] = c
        if len(pat) >= max_len:
            continue
        cond = []
        for items, cc in db:
            if it in items:
                pre = items[:items.index(it)]
                if pre:
                    cond.append((pre, cc))
        if cond:
            _mine(cond, pat, min_sup, max_len, out)


def fp_growth(transactions: Sequence[Sequence[str]], min_support_count: int, min_support_percent: float,
              max_pattern_length: int):
    """Returns (item names by index, patterns {sorted index tuple: support}, N, item supports)."""
    local_counts = Counter()
    local_tx = Counter()
    for t in transactions:
        s = frozenset(t)
        local_tx[s] += 1
        for it in s:
            local_counts[it] += 1
    counts = Counter()
    for c in comm.all_gather_object(dict(local_counts)):
        counts.update(c)
    n = sum(comm.all_gather_object(len(transactions)))
    min_sup = _min_support(n, min_support_count, min_support_percent)
    qualified = [(it, c) for it, c in counts.items() if c >= min_sup]
    qualified.sort(key=lambda t: (-t[1], t[0]))
    names = [it for it, _ in qualified]
    index = {it: i for i, it in enumerate(names)}
    db_counter = Counter()
    for part in comm.all_gather_object([(sorted(index[i] for i in s if i in index), c) for s, c in local_tx.items()]):
        for items, c in part:
            if items:
                db_counter[tuple(items)] += c
    db = list(db_counter.items())
    ws, r = comm.get_world_size(), comm.get_rank()
    mine = {i for i in range(len(names)) if i % ws == r}
    out: Dict[Tuple[int, ...], int] = {}
    _mine(db, (), min_sup, max_pattern_length, out, allowed_last=mine)
    patterns: Dict[Tuple[int, ...], int] = {}
    for part in comm.all_gather_object(out):
        patterns.update(part)
    return names, patterns, n, {index[it]: c for it, c in qualified}


def fp_growth_device(block, min_support_count: int, min_support_percent: float, max_pattern_length: int,
                     backend=None, budget=None, pair_max_items=None, stats=None):
    """``fp_growth`` of this rank's items column (a packed ``StringBlock``) on the block's device with no per-row
    Python: returns ``(item names by index, (items int32, lens int64, sups int64), N, item supports)`` -- the
    patterns as the columns of ``ops.fpm.mine``, ``(len, tuple)`` ascending -- or None when the rows cannot be
    decided from bytes (on any rank): the caller then takes the host path.

    A row is an empty transaction when it is NULL or every byte is ASCII whitespace (0x09-0x0d, 0x1c-0x20); it still
    counts in N.  A row with no ASCII non-whitespace byte but some byte >= 0x80 may be Unicode whitespace only, which
    Python's ``strip()`` knows and the bytes do not tell: such a row, and a hash collision in ``unique_ids``, give
    None.  Items are split by ``ops.strings.split_tokens`` (Java ``String.split``), encoded by ``unique_ids``,
    de-duplicated per row and counted in torch.  Only the distinct items and their counts come to the host (one
    ``all_gather_object``), where the rule of ``fp_growth`` orders the qualifying ones; a lookup table maps local ids
    to ranks.  Every rank keeps its transactions: each level all-reduces its candidate counts.

    Known difference: ``split_tokens`` drops trailing empty items (``"A,B,"`` holds A and B) as the reference's
    ``String.split`` does; the host path's Python ``split`` keeps them (A, B and the empty item).

    ``backend`` is an ``ops.fpm.Backend`` (default: the kernels on a GPU block, the torch twins on a CPU block);
    ``stats`` (a list) receives the encode stage's time and then one entry per level from ``ops.fpm.mine``."""
    import time
    import torch
    from ...ops import fpm as F
    from ...ops.strings import split_tokens, unique_ids
    dev = block.device
    t0 = time.perf_counter()
    if backend is None:
        backend = F.DEVICE if dev.type == "cuda" else F.TWIN
    n_local = len(block)
    d, off = block.data, block.offsets.to(torch.int64)
    nb = int(d.numel())
    ws = _ascii_ws(d)
    high = d >= 0x80

    def _per_row(mask):
        cum = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
        if nb:
            torch.cumsum(mask.to(torch.int64), 0, out=cum[1:])
        return cum[off[1:]] - cum[off[:-1]]

    n_high, n_solid = _per_row(high), _per_row(~ws & ~high)
    empty = (n_solid == 0) & (n_high == 0)
    if block.nulls is not None:
        empty |= block.nulls.to(dev)
    undecided = bool(((n_solid == 0) & (n_high > 0) & ~empty).any())
    names_local: List[str] = []
    counts_local: List[int] = []
    pair = None
    u = 0
    if not undecided:
        tok, doc = split_tokens(block, ord(","))
        live = ~empty[doc]
        tok, doc = tok.take(torch.nonzero(live).reshape(-1)), doc[live]
        enc = unique_ids(tok)
        if enc is None:
            undecided = True
        else:
            ids, rep = enc
            u = int(rep.numel())
            if u:
                pair = torch.unique(doc * u + ids)                  # distinct (row, item), by row then item id
                counts_local = torch.bincount(pair % u, minlength=u).cpu().tolist()
                names_local = tok.take(rep).to_list()
    vote = _vote_items(undecided, names_local, counts_local, n_local, min_support_count, min_support_percent)
    if vote is None:
        return None
    qualified, n, min_sup = vote
    names = [it for it, _ in qualified]
    m = len(names)
    sup_by_index = {i: c for i, (_, c) in enumerate(qualified)}
    crow = torch.zeros(n_local + 1, dtype=torch.int64, device=dev)
    item = torch.zeros(0, dtype=torch.int32, device=dev)
    if m and pair is not None and pair.numel():
        row, r = torch.div(pair, u, rounding_mode="floor"), _rank_lut(qualified, names_local, dev)[pair % u]
        ok = r >= 0
        key = torch.sort(row[ok] * m + r[ok]).values                # by row, then by rank: ascending within a row
        row = torch.div(key, m, rounding_mode="floor")
        torch.cumsum(torch.bincount(row, minlength=n_local), 0, out=crow[1:])
        item = (key - row * m).to(torch.int32)
    item_sup = torch.tensor([c for _, c in qualified], dtype=torch.int64, device=dev)
    if stats is not None:
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        stats.append({"stage": "encode", "seconds": time.perf_counter() - t0, "rows": n_local, "items": m,
                      "entries": int(item.numel())})
    cols = F.mine(crow, item, m, item_sup, min_sup, int(max_pattern_length), backend, budget=budget,
                  pair_max_items=pair_max_items, stats=stats)
    return names, cols, n, sup_by_index


def patterns_dict(cols) -> Dict[Tuple[int, ...], int]:
    """``{sorted index tuple: support}`` (what ``association_rules`` reads) from the pattern columns of
    ``fp_growth_device``, in their order."""
    items, lens, sups = (t.cpu().tolist() for t in cols)
    out: Dict[Tuple[int, ...], int] = {}
    p = 0
    for ln, s in zip(lens, sups):
        out[tuple(items[p:p + ln])] = s
        p += ln
    return out


def association_rules(patterns: Dict[Tuple[int, ...], int], n: int, min_confidence: float, min_lift: float,
                      max_consequent_length: int):
    """(antecedent, consequent, support count, lift, support, confidence) for every rule passing the filters."""
    rules = []
    if max_consequent_length <= 0:
        return rules
    for pat, sup_xy in patterns.items():
        if len(pat) < 2:
            continue
        k = len(pat)
        for size in range(1, min(max_consequent_length, k - 1) + 1):
            from itertools import combinations
            for cons in combinations(pat, size):
                ante = tuple(i for i in pat if i not in cons)
                sup_x = patterns.get(ante)
                sup_y = patterns.get(tuple(cons))
                if not sup_x or not sup_y:
                    continue
                conf = sup_xy / sup_x
                lift = sup_xy * n / (sup_x * sup_y)
                if lift >= min_lift and conf >= min_confidence:
                    rules.append((ante, tuple(cons), sup_xy, lift, sup_xy / n, conf))
    return rules


# ---------------------------------------------------------------------------------------------------
# PrefixSpan (itemset elements; sequence / itemset extensions)
# ---------------------------------------------------------------------------------------------------
def _project(db, item, extend_element: bool):
    """Project each (sequence, count, position) on ``item``.

    A position is (element index, item offset) of the last matched item.  Itemset extension (``_item``)
    looks for ``item`` later in the same element; sequence extension looks in later elements."""
    out = []
    for seq, c, pos in db:
        found = None
        if extend_element:
            # the element that holds the last matched item, or a later element containing the whole last
            # pattern element plus the item
            e, off = pos
            el = seq[e]
            for k in range(off + 1, len(el)):
                if el[k] == item:
                    found = (e, k)
                    break
        else:
            e = pos[0] + 1 if pos is not None else 0
            for ee in range(e, len(seq)):
                el = seq[ee]
                if item in el:
                    found = (ee, el.index(item))
                    break
        if found is not None:
            out.append((seq, c, found))
    return out


def _support(db) -> int:
    return sum(c for _, c, _ in db)


def _span(db, pattern, last_element, min_sup, max_len, out):
    """``pattern`` is a tuple of elements (sorted tuples); ``db`` the sequences projected on it."""
    n_items = sum(len(e) for e in pattern)
    if n_items >= max_len:
        return
    seq_ext = Counter()
    item_ext = Counter()
    for seq, c, pos in db:
        e, off = pos
        seen_s, seen_i = set(), set()
        for ee in range(e + 1, len(seq)):
            for it in seq[ee]:
                seen_s.add(it)
        for k in range(off + 1, len(seq[e])):
            seen_i.add(seq[e][k])
        # itemset extension also when a later element contains the whole last element plus the item
        last = set(last_element)
        for ee in range(e + 1, len(seq)):
            el = seq[ee]
            if last.issubset(el):
                mx = max(last)
                for it in el:
                    if it > mx:
                        seen_i.add(it)
        for it in seen_s:
            seq_ext[it] += c
        for it in seen_i:
            item_ext[it] += c
    for it, c in sorted(item_ext.items()):
        if c < min_sup:
            continue
        new_last = tuple(last_element) + (it,)
        pat = pattern[:-1] + (new_last,)
        proj = []
        for seq, cc, pos in db:
            e, off = pos
            found = None
            for k in range(off + 1, len(seq[e])):
                if seq[e][k] == it:
                    found = (e, k)
                    break
            if found is None:
                for ee in range(e + 1, len(seq)):
                    if set(new_last).issubset(seq[ee]):
                        found = (ee, seq[ee].index(it))
                        break
            if found is not None:
                proj.append((seq, cc, found))
        out[pat] = _support(proj)
        _span(proj, pat, new_last, min_sup, max_len, out)
    for it, c in sorted(seq_ext.items()):
        if c < min_sup:
            continue
        pat = pattern + ((it,),)
        proj = _project(db, it, False)
        out[pat] = _support(proj)
        _span(proj, pat, (it,), min_sup, max_len, out)


def prefix_span(sequences: Sequence[Sequence[Sequence[str]]], min_support_count: int, min_support_percent: float,
                max_pattern_length: int):
    """Returns (item names, index 1.., patterns {tuple of element tuples: support}, N)."""
    occ = Counter()
    local = Counter()
    for s in sequences:
        for el in s:
            for it in el:
                occ[it] += 1
        local[tuple(tuple(el) for el in s)] += 1
    counts = Counter()
    for c in comm.all_gather_object(dict(occ)):
        counts.update(c)
    n = sum(comm.all_gather_object(len(sequences)))
    min_sup = _min_support(n, min_support_count, min_support_percent)
    qualified = [(it, c) for it, c in counts.items() if c >= min_sup]
    qualified.sort(key=lambda t: (-t[1], t[0]))
    names = [None] + [it for it, _ in qualified]
    index = {it: i + 1 for i, (it, _) in enumerate(qualified)}
    db_counter = Counter()
    for part in comm.all_gather_object(list(local.items())):
        for s, c in part:
            enc = []
            for el in s:
                ids = sorted({index[i] for i in el if i in index})
                if ids:
                    enc.append(tuple(ids))
            if enc:
                db_counter[tuple(enc)] += c
    db0 = list(db_counter.items())
    ws, r = comm.get_world_size(), comm.get_rank()
    out = {}
    for it in range(1, len(names)):
        if (it - 1) % ws != r:
            continue
        proj = _project([(s, c, None) for s, c in db0], it, False)
        sup = _support(proj)
        if sup < min_sup:
            continue
        pat = ((it,),)
        out[pat] = sup
        _span(proj, pat, (it,), min_sup, max_pattern_length, out)
    patterns = {}
    for part in comm.all_gather_object(out):
        patterns.update(part)
    return names, patterns, n


def prefix_span_device(block, min_support_count: int, min_support_percent: float, max_pattern_length: int,
                       backend=None, budget=None, stats=None):
    """``prefix_span`` of this rank's sequence column (a packed ``StringBlock``) on the block's device with no per-row
    Python: returns ``(item names, index 1.., (codes int32, lens int64, sups int64), N)`` -- the patterns as the
    columns of ``ops.prefixspan.mine`` (step codes ``2 * item + s`` of 0-based items; ``ops.prefixspan.decode`` gives
    the dict of ``prefix_span``) -- or None when the column cannot be proved from its bytes, on any rank, to parse as
    the host path parses it: the caller then takes the host path.

    The host parse is the contract: a row that is NULL or strips to nothing is an empty sequence that still counts in
    N; any other row is ``s.split(";")``, every element ``.strip()``ped and ``.split(",")``.  Here a row is empty
    when it is NULL or every byte is ASCII whitespace (0x09-0x0d, 0x1c-0x20); elements are trimmed of those bytes and
    split on the comma.  None is returned for a column with an empty item after the trim (a doubled, leading or
    trailing delimiter in a non-empty row: Python's ``split`` keeps an empty-string item there), an element whose
    first or last character has the UTF-8 lead byte C2, E1, E2 or E3 (it could be Unicode whitespace that ``strip()``
    removes), a row of more than 64 elements (judged on the raw count), or a hash collision in ``unique_ids``.

    Items qualify by occurrences over all ranks and are ordered by ``(-count, name)`` as in ``prefix_span``; only the
    distinct items with their counts cross ranks (one ``all_gather_object``), then each level's integer counts.
    ``backend`` is an ``ops.prefixspan.Backend`` (default: the kernels on a GPU block, the torch twins on a CPU
    block); ``stats`` (a list) receives the encode stage's time and then one entry per level."""
    import time
    import torch
    from ...common.strings import StringBlock
    from ...ops import prefixspan as S
    from ...ops.strings import split_tokens, unique_ids
    dev = block.device
    t0 = time.perf_counter()
    if backend is None:
        backend = S.DEVICE if dev.type == "cuda" else S.TWIN
    n_local = len(block)
    d, off = block.data, block.offsets.to(torch.int64)
    nb = int(d.numel())

    def _trimmed(blk):
        """First and last byte positions of every string of ``blk`` that are not ASCII whitespace (last < first:
        there is none)."""
        k = len(blk)
        lens = blk.lengths()
        seg = torch.repeat_interleave(torch.arange(k, device=dev), lens, output_size=int(blk.data.numel()))
        solid = torch.nonzero(~_ascii_ws(blk.data)).reshape(-1)
        first = torch.full((k,), int(blk.data.numel()), dtype=torch.int64, device=dev)
        last = torch.full((k,), -1, dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, seg[solid], solid, reduce="amin")
        last.scatter_reduce_(0, seg[solid], solid, reduce="amax")
        return first, last

    cum = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    if nb:
        torch.cumsum((~_ascii_ws(d)).to(torch.int64), 0, out=cum[1:])
    empty = (cum[off[1:]] - cum[off[:-1]]) == 0
    if block.nulls is not None:
        empty |= block.nulls.to(dev)
    live_rows = ~empty
    names_local: List[str] = []
    counts_local: List[int] = []
    undecided = False
    ids = el_row = el_of_tok = None
    u = 0
    if bool(live_rows.any()):
        # a trailing ';' ends a row with an empty element, which split_tokens would drop
        undecided = bool((d[(off[1:] - 1)[live_rows]] == ord(";")).any())
        if not undecided:
            els, el_row = split_tokens(block, ord(";"))
            keep = live_rows[el_row]
            els, el_row = els.take(torch.nonzero(keep).reshape(-1)), el_row[keep]
            undecided = int(torch.bincount(el_row, minlength=1).max()) > 64
        if not undecided:
            ed = els.data
            first, last = _trimmed(els)
            undecided = bool((last < first).any())                          # an element of whitespace only
        if not undecided:
            comma = ed == ord(",")
            b0, b1 = ed[first], ed[last]
            risky = (b0 == 0xC2) | ((b0 >= 0xE1) & (b0 <= 0xE3))
            # the lead byte of the last character: one back for a 2-byte character, two back for a 3-byte one
            cont = (b1 >= 0x80) & (b1 < 0xC0)
            p1, p2 = ed[(last - 1).clamp(min=0)], ed[(last - 2).clamp(min=0)]
            risky |= cont & (last - 1 >= first) & (p1 == 0xC2)
            risky |= cont & (last - 2 >= first) & (p2 >= 0xE1) & (p2 <= 0xE3)
            undecided = bool(risky.any() or comma[first].any() or comma[last].any()
                             or (comma[1:] & comma[:-1]).any())
        if not undecided:
            ln = last - first + 1
            toff = torch.zeros(int(ln.numel()) + 1, dtype=torch.int64, device=dev)
            torch.cumsum(ln, 0, out=toff[1:])
            src = torch.repeat_interleave(first - toff[:-1], ln) + torch.arange(int(toff[-1]), device=dev)
            tok, el_of_tok = split_tokens(StringBlock(ed[src], toff), ord(","))
            enc = unique_ids(tok)
            if enc is None:
                undecided = True
            else:
                ids, rep = enc
                u = int(rep.numel())
                counts_local = torch.bincount(ids, minlength=u).cpu().tolist()     # occurrences, duplicates included
                names_local = tok.take(rep).to_list()
    vote = _vote_items(undecided, names_local, counts_local, n_local, min_support_count, min_support_percent)
    if vote is None:
        return None
    qualified, n, min_sup = vote
    names = [None] + [it for it, _ in qualified]
    m = len(qualified)
    w = 8
    crow = torch.zeros(n_local * w + 1, dtype=torch.int64, device=dev)
    item = torch.zeros(0, dtype=torch.int32, device=dev)
    item_sup = torch.zeros(m, dtype=torch.int64, device=dev)
    if m and u:
        r = _rank_lut(qualified, names_local, dev)[ids]
        ok = r >= 0
        # distinct (element, rank), by element then rank; elements left empty drop out and the rest close up
        n_el = int(el_row.numel())
        key = torch.unique(el_of_tok[ok] * m + r[ok])
        el = torch.div(key, m, rounding_mode="floor")
        r = key - el * m
        has = torch.zeros(n_el, dtype=torch.bool, device=dev)
        has[el] = True
        seq_len = torch.bincount(el_row[has], minlength=n_local)
        before = torch.cumsum(has.to(torch.int64), 0) - has.to(torch.int64)
        row_first = torch.cumsum(seq_len, 0) - seq_len
        j = before[el] - row_first[el_row[el]]                  # the element's place among its row's kept elements
        w = S.field_width(int(seq_len.max()))
        slot = el_row[el] * w + j
        crow = torch.zeros(n_local * w + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(slot, minlength=n_local * w), 0, out=crow[1:])
        item = r.to(torch.int32)
        item_sup = torch.bincount(torch.unique(el_row[el] * m + r) % m, minlength=m)
    if m:
        comm.all_reduce(item_sup, "sum")                        # level 1: distinct (sequence, item) pairs
    if stats is not None:
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        stats.append({"stage": "encode", "seconds": time.perf_counter() - t0, "rows": n_local, "items": m,
                      "entries": int(item.numel()), "w": w})
    cols = S.mine(crow, item, m, n_local, w, item_sup, min_sup, int(max_pattern_length), backend, budget=budget,
                  stats=stats)
    return names, cols, n


def sequence_rules(patterns, n: int, min_confidence: float):
    """(antecedent elements, consequent element, support count, support, confidence)."""
    out = []
    for pat, sup_xy in patterns.items():
        if len(pat) <= 1:
            continue
        ante, cons = pat[:-1], pat[-1]
        sup_x = patterns.get(ante)
        if not sup_x:
            continue
        conf = sup_xy / sup_x
        if conf >= min_confidence:
            out.append((ante, (cons,), sup_xy, sup_xy / n, conf))
    return out
