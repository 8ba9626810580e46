#!/usr/bin/env python3
"""Frequent-itemset mining on one GPU: the device path of ``FpGrowthBatchOp`` (``ops/fpm.py``, ``ops/csrc/fpm.hip``)
by stage, its two count kernels by variant, and the host path it leaves in place (``profiles/fpgrowth.txt``).

    python tools/fpgrowth_bench.py                              # every part below
    python tools/fpgrowth_bench.py --rows 1000000 --percents 0.01 --host-rows 0 --cross ""

The table: ``--rows`` transactions of ``--items`` draws (with replacement, so about that many distinct items) from a
``--vocab``-item Zipf(``--zipf``) vocabulary, written on the device as the operator's items column (4-digit names
joined by commas, one packed ``StringBlock``).

* per ``--percents`` value (``minSupportPercent``, default ``maxPatternLength``): ``fp_growth_device`` by stage --
  encode, bitmap, each level with its candidates and kept itemsets -- after one warm-up run at a tenth of the rows;
* the two count kernels on the bitmap and the largest candidate batches of that run, by variant (chunk, splits,
  grid): milliseconds (device events, best of ``--reps``), ps per (candidate, 64-bit word), and the bytes
  each variant reads from the L2 side per second, beside 6.3 TB/s (HBM, streamed) and 8.6 TB/s (Infinity Cache,
  random rows) of the MI355X -- context, not a pass mark;
* ``--host-rows``: the host path (the operator's ``to_list`` / ``split`` / ``fp_growth`` / sort) against the device
  path on the first ``--host-rows`` rows of the table at the first percent, in this process, equal patterns checked;
* ``--cross``: both paths at each of these row counts, for the crossover ``FPM_MIN_ROWS``.

One JSON line per part.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BPS, MALL_BPS = 6.3e12, 8.6e12


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


def table(n, vocab, items, zipf, seed, dev):
    """The items column of ``n`` transactions as a packed block on ``dev``: ``items`` 4-digit names a row."""
    from alink_amd.common.strings import StringBlock
    g = torch.Generator(device=dev).manual_seed(seed)
    w = 1.0 / torch.arange(1, vocab + 1, device=dev, dtype=torch.float64) ** zipf
    cdf = torch.cumsum(w / w.sum(), 0)
    ids = torch.searchsorted(cdf, torch.rand((n, items), device=dev, generator=g, dtype=torch.float64))
    ids = ids.clamp(max=vocab - 1)
    cell = torch.empty((n, items, 5), dtype=torch.uint8, device=dev)
    for k, p in enumerate((1000, 100, 10, 1)):
        cell[:, :, k] = (torch.div(ids, p, rounding_mode="floor") % 10 + 48).to(torch.uint8)
    cell[:, :, 4] = 44
    width = 5 * items - 1
    data = cell.reshape(n, 5 * items)[:, :width].contiguous().reshape(-1)
    return StringBlock(data, torch.arange(n + 1, device=dev, dtype=torch.int64) * width)


def head(block, n):
    width = int(block.offsets[1])
    return block.row_range(0, n, 0, n * width)


def device_run(block, percent, backend=None):
    from alink_amd.models.associationrule import mining as M
    stats = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = M.fp_growth_device(block, -1, percent, 10, backend=backend, stats=stats)
    torch.cuda.synchronize()
    return res, stats, time.perf_counter() - t0


def host_run(block, percent):
    """What the operator's host path does with the column, up to the sorted pattern rows."""
    from alink_amd.models.associationrule import mining as M
    t0 = time.perf_counter()
    rows = block.to_list()
    tx = [s.split(",") if s is not None and s.strip() else [] for s in rows]
    names, pats, n, _ = M.fp_growth(tx, -1, percent, 10)
    order = sorted(pats, key=lambda t: (len(t), t))
    prow = [(",".join(names[i] for i in pat), int(pats[pat]), len(pat)) for pat in order]
    return (names, pats), len(prow), time.perf_counter() - t0


def stage_report(stats, total):
    enc = stats[0]
    levels = [{k: s[k] for k in ("level", "path", "candidates", "kept", "seconds")} for s in stats[1:]]
    bitmap = stats[-1]["bitmap_seconds"] if len(stats) > 1 else 0.0
    for lv in levels[:1]:
        lv["seconds"] -= bitmap              # the first level builds the bitmap; reported on its own
    return {"encode_s": enc["seconds"], "items": enc["items"], "entries": enc["entries"], "bitmap_s": bitmap,
            "levels": levels, "total_s": total}


def micro(cap, reps):
    """The count kernels on what the run left in ``cap``: its bitmap and its largest batch per prefix length."""
    from alink_amd.ops import fpm as F
    B = cap["B"]
    m, W = int(B.shape[0]), int(B.shape[1])
    out = []
    pairs = m * (m - 1) // 2
    if m >= 2:
        T = (m + 63) // 64
        staged = T * (T + 1) // 2 * 128 * W * 8                 # both slabs of every block on or above the diagonal
        for chunk, splits in ((32, 0), (16, 0), (32, 1), (32, 4), (32, 16), (32, 64)):
            ms = timed(lambda: F.pair_counts(B, chunk=chunk, splits=splits), reps)
            out.append({"kernel": "pair", "items": m, "words": W, "chunk": chunk, "splits": splits, "ms": ms,
                        "ps_per_pair_word": ms * 1e9 / (pairs * W), "l2_side_TBps": staged / ms / 1e9})
    for P, (prefix, ptr, ext) in sorted(cap["cls"].items()):
        nc, ne = int(prefix.shape[0]), int(ext.numel())
        tiles = int(((ptr[1:] - ptr[:-1] + 15) // 16).sum())
        read = (ne + tiles * P) * W * 8                         # every extension row once, the prefix rows per tile
        for chunk, grid in ((0, 0), (128, 0), (512, 0), (2048, 0), (8192, 0), (0, 512), (0, 4096)):
            ms = timed(lambda: F.class_counts(B, prefix, ptr, ext, chunk=chunk, grid=grid), reps)
            out.append({"kernel": "class", "prefix_len": P, "classes": nc, "candidates": ne, "words": W,
                        "chunk": chunk, "grid": grid, "ms": ms,
                        "ps_per_candidate_word": ms * 1e9 / (ne * W), "l2_side_TBps": read / ms / 1e9})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--items", type=int, default=10)
    ap.add_argument("--zipf", type=float, default=1.0)
    ap.add_argument("--percents", default="0.01,0.001")
    ap.add_argument("--host-rows", type=int, default=100_000)
    ap.add_argument("--cross", default="100,1000,10000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--micro-candidates", type=int, default=4_000_000)
    a = ap.parse_args()
    from alink_amd.models.associationrule import mining as M
    from alink_amd.ops import _lib, fpm as F
    _lib.require()
    dev = torch.device("cuda:0")
    block = table(a.rows, a.vocab, a.items, a.zipf, 1, dev)
    percents = [float(x) for x in a.percents.split(",") if x]
    device_run(head(block, max(a.rows // 10, 1)), percents[0])          # warm-up: allocator, kernels, hashes
    for pc in percents:
        cap = {"cls": {}}

        def pair(B, **kw):
            cap["B"] = B
            return F.pair_counts(B, **kw)

        def cls(B, prefix, ptr, ext, **kw):
            cap["B"] = B
            P, old = int(prefix.shape[1]), cap["cls"].get(int(prefix.shape[1]))
            if ext.numel() <= a.micro_candidates and (old is None or ext.numel() > old[2].numel()):
                cap["cls"][P] = (prefix, ptr, ext)
            return F.class_counts(B, prefix, ptr, ext, **kw)

        calls = F.FPM_CALLS
        res, stats, total = device_run(block, pc, F.Backend(F.build_bitmap, pair, cls))
        rep = stage_report(stats, total)
        rep.update({"part": "device", "rows": a.rows, "min_support_percent": pc, "patterns": int(res[1][1].numel()),
                    "longest": int(res[1][1].max()) if res[1][1].numel() else 0, "launches": F.FPM_CALLS - calls})
        print(json.dumps(rep), flush=True)
        if "B" in cap:
            for line in micro(cap, a.reps):
                line.update({"part": "kernel", "min_support_percent": pc})
                print(json.dumps(line), flush=True)
        del cap, res
    sizes = [int(x) for x in a.cross.split(",") if x] + ([a.host_rows] if a.host_rows > 0 else [])
    for n in sizes:
        sub = head(block, min(n, a.rows))
        device_run(sub, percents[0])
        res, stats, t_dev = device_run(sub, percents[0])
        (names, pats), n_pat, t_host = host_run(sub.to("cpu"), percents[0])
        same = names == res[0] and pats == M.patterns_dict(res[1])
        print(json.dumps({"part": "host_vs_device", "rows": len(sub), "min_support_percent": percents[0],
                          "patterns": n_pat, "host_s": t_host, "device_s": t_dev, "equal": bool(same)}), flush=True)


if __name__ == "__main__":
    main()
