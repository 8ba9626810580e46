"""Seeded transaction tables and a brute-force oracle for the frequent-itemset tests (test_fpgrowth_device.py,
test_fpgrowth_gpu.py).  The oracle shares no code with either path of the operator: Python sets,
``itertools.combinations`` over the frequent items, exact integer supports."""
import math
from itertools import combinations

import numpy as np

ITEM_SEP = ","


def split_row(s):
    """The operator's host rule for one cell of the items column."""
    return s.split(ITEM_SEP) if s is not None and s.strip() else []


def gen_rows(seed, n, vocab, max_len=5, zipf=1.2, shuffle_dups=True):
    """``n`` item strings over ``vocab`` with Zipf-like popularity; some rows repeat an item (set semantics)."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, len(vocab) + 1) ** zipf
    w /= w.sum()
    rows = []
    for _ in range(n):
        k = int(rng.integers(1, max_len + 1))
        it = [vocab[j] for j in rng.choice(len(vocab), size=k, p=w)]        # with replacement: duplicates happen
        if not shuffle_dups:
            it = sorted(set(it))
        rows.append(ITEM_SEP.join(it))
    return rows


def oracle(transactions, min_support_count, min_support_percent, max_len):
    """``(names, {index tuple: support}, N)`` by brute force: items ordered by support descending then name
    ascending, every combination of frequent items counted against every transaction set."""
    sets = [set(t) for t in transactions]
    n = len(sets)
    min_sup = int(min_support_count) if min_support_count is not None and min_support_count >= 0 \
        else int(math.floor(n * min_support_percent))
    sup = {}
    for s in sets:
        for it in s:
            sup[it] = sup.get(it, 0) + 1
    names = sorted((it for it, c in sup.items() if c >= min_sup), key=lambda it: (-sup[it], it))
    keep = max(min_sup, 1)
    pats = {}
    for L in range(1, min(max_len, len(names)) + 1):
        found = False
        for combo in combinations(range(len(names)), L):
            want = {names[i] for i in combo}
            c = sum(1 for s in sets if want <= s)
            if c >= keep:
                pats[combo] = c
                found = True
        if not found:
            break
    return names, pats, n


def random_bits(seed, n, m, density=0.3, empty_rows=0.1, zero_items=()):
    """bool [n, m]: transaction t holds item i; a share of the transactions holds nothing."""
    rng = np.random.default_rng(seed)
    D = rng.random((n, m)) < density
    D[rng.random(n) < empty_rows] = False
    for i in zero_items:
        D[:, i] = False
    return D


def csr_of(D):
    """``(crow int64 [n + 1], item int32 [nnz])`` of bool [n, m], items ascending within a row."""
    n = D.shape[0]
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(D.sum(1), out=crow[1:])
    return crow, np.nonzero(D)[1].astype(np.int32)


def row_stride(n):
    return max(2, ((n + 63) // 64 + 1) // 2 * 2)


def packed(D):
    """int64 [m, row_stride(n)]: bit t of row i = D[t, i], little-endian, zero padding (``numpy.packbits``)."""
    n, m = D.shape
    W = row_stride(n)
    full = np.zeros((m, W * 64), dtype=np.uint8)
    full[:, :n] = D.T
    return np.packbits(full, axis=1, bitorder="little").view(np.int64).reshape(m, W)


def pair_oracle(D):
    """int64 [m, m]: the transactions that hold both items for i < j, zero elsewhere."""
    X = D.astype(np.int64)
    return np.triu(X.T @ X, 1)


def random_classes(seed, m, P, n_classes, ext_sizes):
    """Classes with ``P`` prefix items each and the given numbers of extensions (cycled): ``(prefix int32
    [classes, P], cls_ptr int64 [classes + 1], ext int32 [candidates])``, the items of a candidate distinct."""
    rng = np.random.default_rng(seed)
    prefix = np.zeros((n_classes, P), dtype=np.int32)
    ptr = np.zeros(n_classes + 1, dtype=np.int64)
    ext = []
    for c in range(n_classes):
        k = min(int(ext_sizes[c % len(ext_sizes)]), m - P)
        perm = rng.permutation(m)
        prefix[c] = np.sort(perm[:P])
        ext.append(np.sort(perm[P:P + k]))
        ptr[c + 1] = ptr[c] + k
    return prefix, ptr, np.concatenate(ext).astype(np.int32)


def class_oracle(D, prefix, ptr, ext):
    out = np.zeros(len(ext), dtype=np.int64)
    for c in range(prefix.shape[0]):
        has = D[:, prefix[c]].all(1)
        for e in range(ptr[c], ptr[c + 1]):
            out[e] = int((has & D[:, ext[e]]).sum())
    return out
