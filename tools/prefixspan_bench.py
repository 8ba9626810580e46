#!/usr/bin/env python3
"""Sequential-pattern mining on one GPU: the device path of ``PrefixSpanBatchOp`` (``ops/prefixspan.py``,
``alink_fpm_seq_counts`` in ``ops/csrc/fpm.hip``) by stage and level, its count kernel beside the itemset class kernel,
and the host path it leaves in place (``profiles/prefixspan.txt``).

    python tools/prefixspan_bench.py                            # every part below
    python tools/prefixspan_bench.py --rows 1000000 --percents 0.01 --host-rows 0 --cross ""

The table: ``--rows`` sequences of ``--elements`` elements of 1 to ``--items`` draws (with replacement) from a
``--vocab``-item Zipf(``--zipf``) vocabulary, written on the device as the operator's sequence column (4-digit names,
commas inside an element, semicolons between elements, one packed ``StringBlock``).

* per ``--percents`` value (``minSupportPercent``, ``--max-len``): ``prefix_span_device`` by stage -- encode, bitmap,
  each level with its candidates and kept patterns -- after one warm-up run at a tenth of the rows;
* the count kernel on the bitmap and the largest candidate batch of levels 2 and 3 of that run: milliseconds (device
  events, best of ``--reps``) and ps per (candidate, 64-bit word), next to ``alink_fpm_class_counts`` on the same
  bitmap with the same classes read as itemsets (the same loads but for the chain's share, no ``after``, a plain
  popcount), and the ratio of the two;
* ``--host-rows``: the host path (the operator's ``to_list`` / ``split`` / ``prefix_span`` / sort) against the device
  path on the first ``--host-rows`` rows at the first percent, in this process, equal patterns checked;
* ``--cross``: both paths at each of these row counts, for the crossover ``SPM_MIN_ROWS``.

One JSON line per part.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    """Best milliseconds of ``reps`` calls of ``fn`` (device events), after one warm-up call."""
    fn()
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t = a.elapsed_time(b)
        best = t if best is None else min(best, t)
    return best


def table(n, vocab, elements, items, zipf, seed, dev):
    """The sequence column of ``n`` rows as a packed block on ``dev``."""
    from alink_amd.common.strings import StringBlock
    g = torch.Generator(device=dev).manual_seed(seed)
    wgt = 1.0 / torch.arange(1, vocab + 1, device=dev, dtype=torch.float64) ** zipf
    cdf = torch.cumsum(wgt / wgt.sum(), 0)
    ids = torch.searchsorted(cdf, torch.rand((n, elements, items), device=dev, generator=g, dtype=torch.float64))
    ids = ids.clamp(max=vocab - 1)
    cnt = torch.randint(1, items + 1, (n, elements), device=dev, generator=g)
    cell = torch.empty((n, elements, items, 5), dtype=torch.uint8, device=dev)
    for k, p in enumerate((1000, 100, 10, 1)):
        cell[..., k] = (torch.div(ids, p, rounding_mode="floor") % 10 + 48).to(torch.uint8)
    pos = torch.arange(items, device=dev).reshape(1, 1, items)
    last = pos == (cnt.unsqueeze(-1) - 1)
    cell[..., 4] = torch.where(last, 59, 44).to(torch.uint8)     # ';' after an element's last item, ',' inside
    keep = (pos < cnt.unsqueeze(-1)).unsqueeze(-1).expand(n, elements, items, 5).clone()
    keep[:, elements - 1, :, 4] &= ~last[:, elements - 1]        # no separator after a row's last item
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(keep.reshape(n, -1).sum(1), 0, out=off[1:])
    return StringBlock(cell.reshape(-1)[keep.reshape(-1)], off)


def head(block, n):
    return block.row_range(0, n, 0, int(block.offsets[n]))


def device_run(block, percent, max_len, backend=None):
    from alink_amd.models.associationrule import mining as M
    stats = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = M.prefix_span_device(block, -1, percent, max_len, backend=backend, stats=stats)
    torch.cuda.synchronize()
    return res, stats, time.perf_counter() - t0


def host_run(block, percent, max_len):
    """What the operator's host path does with the column, up to the sorted pattern rows."""
    from alink_amd.models.associationrule import mining as M
    t0 = time.perf_counter()
    seqs = []
    for s in block.to_list():
        if s is None or not s.strip():
            seqs.append([])
            continue
        seqs.append([el.strip().split(",") for el in s.split(";")])
    names, pats, n = M.prefix_span(seqs, -1, percent, max_len)
    order = sorted(pats, key=lambda t: (sum(len(e) for e in t), t))
    prow = [(";".join(",".join(names[i] for i in el) for el in pat), int(pats[pat]), sum(len(e) for e in pat))
            for pat in order]
    return (names, pats), len(prow), time.perf_counter() - t0


def stage_report(stats, total):
    enc = stats[0]
    levels = [{k: s[k] for k in ("level", "candidates", "kept", "seconds")} for s in stats[1:]]
    bitmap = stats[-1]["bitmap_seconds"] if len(stats) > 1 else 0.0
    # the bitmap is built in the first level and kept (one row block), or rebuilt per block in every level; its
    # time is reported on its own.  With several blocks it also holds the wait for the block before it, whose
    # counts are still running when the next build is timed: then read a level as seconds + bitmap_s
    done = 0.0
    for lv, s in zip(levels, stats[1:]):
        lv["bitmap_s"] = s["bitmap_seconds"] - done
        lv["seconds"] -= lv["bitmap_s"]
        done = s["bitmap_seconds"]
    out = {"encode_s": enc["seconds"], "items": enc["items"], "entries": enc["entries"], "w": enc["w"],
           "bitmap_s": bitmap, "levels": levels, "total_s": total}
    if len(stats) > 1:
        out["W"], out["row_blocks"] = stats[1]["W"], stats[1]["row_blocks"]
    return out


def micro(cap, reps):
    """``seq_counts`` on what the run left in ``cap`` (its bitmap and its largest batch per parent length), and
    ``class_counts`` on the same bitmap with the same classes read as itemsets."""
    from alink_amd.ops import fpm as F, prefixspan as S
    B, n_seq, w = cap["B"], cap["n_seq"], cap["w"]
    W = int(B.shape[1])
    out = []
    for P, (prefix, ptr, ext) in sorted(cap["cls"].items()):
        ne = int(ext.numel())
        tiles = int(((ptr[1:] - ptr[:-1] + 15) // 16).sum())
        ms = timed(lambda: S.seq_counts(B, n_seq, w, prefix, ptr, ext), reps)
        items = ((prefix >> 1).contiguous(), ptr, (ext >> 1).contiguous())
        ms_c = timed(lambda: F.class_counts(B, *items), reps)
        out.append({"level": P + 1, "classes": int(prefix.shape[0]), "candidates": ne, "words": W, "w": w,
                    "seq_ms": ms, "seq_ps_per_candidate_word": ms * 1e9 / (ne * W), "class_ms": ms_c,
                    "class_ps_per_candidate_word": ms_c * 1e9 / (ne * W), "seq_over_class": ms / ms_c,
                    "loads_per_step": {"extensions": ne, "chain": tiles * P}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--elements", type=int, default=5)
    ap.add_argument("--items", type=int, default=3)
    ap.add_argument("--zipf", type=float, default=1.0)
    ap.add_argument("--max-len", type=int, default=10)
    ap.add_argument("--percents", default="0.01,0.001")
    ap.add_argument("--host-rows", type=int, default=20_000)
    ap.add_argument("--cross", default="100,300,1000,3000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--micro-candidates", type=int, default=4_000_000)
    a = ap.parse_args()
    from alink_amd.ops import _lib, fpm as F, prefixspan as S
    _lib.require()
    dev = torch.device("cuda:0")
    block = table(a.rows, a.vocab, a.elements, a.items, a.zipf, 1, dev)
    percents = [float(x) for x in a.percents.split(",") if x]
    device_run(head(block, max(a.rows // 10, 1)), percents[0], a.max_len)      # warm-up: allocator, kernels, hashes
    for pc in percents:
        cap = {"cls": {}}

        def seq(B, n_seq, w, prefix, ptr, ext, **kw):
            cap.update({"B": B, "n_seq": n_seq, "w": w})
            P, old = int(prefix.shape[1]), cap["cls"].get(int(prefix.shape[1]))
            if P <= 2 and ext.numel() <= a.micro_candidates and (old is None or ext.numel() > old[2].numel()):
                cap["cls"][P] = (prefix, ptr, ext)
            return S.seq_counts(B, n_seq, w, prefix, ptr, ext, **kw)

        calls = S.SPM_CALLS
        res, stats, total = device_run(block, pc, a.max_len, S.Backend(F.build_bitmap, seq))
        rep = stage_report(stats, total)
        lens = res[1][1]
        rep.update({"part": "device", "rows": a.rows, "min_support_percent": pc, "patterns": int(lens.numel()),
                    "longest": int(lens.max()) if lens.numel() else 0, "launches": S.SPM_CALLS - calls})
        print(json.dumps(rep), flush=True)
        if "B" in cap:
            for line in micro(cap, a.reps):
                line.update({"part": "kernel", "min_support_percent": pc})
                print(json.dumps(line), flush=True)
        del cap, res
    sizes = [int(x) for x in a.cross.split(",") if x] + ([a.host_rows] if a.host_rows > 0 else [])
    for n in sizes:
        sub = head(block, min(n, a.rows))
        device_run(sub, percents[0], a.max_len)
        res, stats, t_dev = device_run(sub, percents[0], a.max_len)
        (names, pats), n_pat, t_host = host_run(sub.to("cpu"), percents[0], a.max_len)
        same = names == res[0] and pats == S.decode(res[1])
        print(json.dumps({"part": "host_vs_device", "rows": len(sub), "min_support_percent": percents[0],
                          "patterns": n_pat, "host_s": t_host, "device_s": t_dev, "equal": bool(same)}), flush=True)


if __name__ == "__main__":
    main()
