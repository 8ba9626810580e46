"""Seeded sequence tables and a brute-force oracle for the sequential-pattern tests (test_prefixspan_device.py,
test_prefixspan_gpu.py).  The oracle knows no bitmap: a table is a bool array ``D[t, j, i]`` (element ``j`` of
sequence ``t`` holds item ``i``; a sequence's elements beyond its length hold nothing), and the support of a pattern
is counted by matching its elements, in order, against the earliest later element of each sequence that holds them
all.  ``packed_fields`` builds the field layout of ``ops/prefixspan.py`` with numpy."""
import numpy as np

ITEM_SEP, ELEMENT_SEP = ",", ";"


def row_stride(n):
    return max(2, ((n + 63) // 64 + 1) // 2 * 2)


def random_table(seed, n_seq, w, m, density=0.5, empty=0.1):
    """bool [n_seq, w, m]: lengths uniform in 0 .. w (a share of the sequences is empty), no empty element inside a
    sequence's length."""
    rng = np.random.default_rng(seed)
    D = rng.random((n_seq, w, m)) < density
    hole = ~D.any(2)
    D[hole, rng.integers(0, m, size=int(hole.sum()))] = True
    lens = rng.integers(0, w + 1, size=n_seq)
    lens[rng.random(n_seq) < empty] = 0
    D[np.arange(w)[None, :] >= lens[:, None]] = False
    return D


def packed_fields(D, w=None):
    """int64 [m, row_stride(n_seq * w)]: bit ``j`` of field ``t`` (``w`` bits, back to back, little-endian) of row
    ``i`` = ``D[t, j, i]``; zero padding."""
    n_seq, width, m = D.shape
    w = width if w is None else w
    assert w in (8, 16, 32, 64) and width <= w
    W = row_stride(n_seq * w)
    full = np.zeros((m, W * 64), dtype=np.uint8)
    slots = np.zeros((n_seq, w, m), dtype=np.uint8)
    slots[:, :width] = D
    full[:, :n_seq * w] = slots.reshape(n_seq * w, m).T
    return np.packbits(full, axis=1, bitorder="little").view(np.int64).reshape(m, W)


def slot_csr(D, w=None):
    """``(crow int64 [n_seq * w + 1], item int32)``: slot ``t * w + j`` holds the items of element ``j``."""
    n_seq, width, m = D.shape
    w = width if w is None else w
    slots = np.zeros((n_seq, w, m), dtype=bool)
    slots[:, :width] = D
    flat = slots.reshape(n_seq * w, m)
    crow = np.zeros(n_seq * w + 1, dtype=np.int64)
    np.cumsum(flat.sum(1), out=crow[1:])
    return crow, np.nonzero(flat)[1].astype(np.int32)


def elements_of(codes):
    """The elements (lists of 0-based items) of a row of step codes ``2 * item + s``."""
    pat = []
    for c in codes:
        c = int(c)
        if c & 1:
            pat.append([c >> 1])
        else:
            pat[-1].append(c >> 1)
    return pat


def support(D, codes):
    """Sequences of ``D`` that hold the pattern: its elements matched in order, each at the earliest element after
    the one before that holds all its items (the earliest match leaves the most room, so it decides)."""
    n_seq, w, _ = D.shape
    pos = np.full(n_seq, -1)
    alive = np.ones(n_seq, dtype=bool)
    j = np.arange(w)[None, :]
    for el in elements_of(codes):
        ok = D[:, :, el].all(2) & (j > pos[:, None])
        alive &= ok.any(1)
        pos = np.where(alive, ok.argmax(1), w)
    return int(alive.sum())


def seq_oracle(D, prefix, ptr, ext):
    out = np.zeros(len(ext), dtype=np.int64)
    for c in range(prefix.shape[0]):
        for e in range(ptr[c], ptr[c + 1]):
            out[e] = support(D, list(prefix[c]) + [ext[e]])
    return out


def random_seq_classes(seed, m, P, n_classes, ext_sizes):
    """Classes of ``P`` step codes (the first an S code, the others S or I at random, an I code's item above the one
    before it) and the given numbers of extension codes (cycled), ascending within a class: ``(prefix int32
    [classes, P], cls_ptr int64 [classes + 1], ext int32 [candidates])``."""
    rng = np.random.default_rng(seed)
    prefix = np.zeros((n_classes, P), dtype=np.int32)
    ptr = np.zeros(n_classes + 1, dtype=np.int64)
    ext = []
    for c in range(n_classes):
        it = int(rng.integers(0, m))
        prefix[c, 0] = 2 * it + 1
        for q in range(1, P):
            if it < m - 1 and rng.random() < 0.5:
                it = int(rng.integers(it + 1, m))
                prefix[c, q] = 2 * it
            else:
                it = int(rng.integers(0, m))
                prefix[c, q] = 2 * it + 1
        pool = [2 * b + 1 for b in range(m)] + [2 * b for b in range(it + 1, m)]
        k = int(ext_sizes[c % len(ext_sizes)])
        ext.append(np.sort(rng.choice(pool, size=k, replace=k > len(pool))))
        ptr[c + 1] = ptr[c] + k
    return prefix, ptr, np.concatenate(ext).astype(np.int32)


def edge_table(w):
    """Four sequences of three items around the edges of ``after`` and of the field count, and what they give.
    Sequence 0 has exactly ``w`` elements and item 0 only in the last one (the top bit of its field: nothing comes
    after it, and nothing may reach the next field); its neighbour 1 holds item 1 in element 0 and item 0 nowhere;
    sequence 2 holds item 0 in element 0 only and item 1 in element 1; sequence 3 holds both in element 0 only.
    Returns ``(D, prefix, ptr, ext, want)`` for the parent ``(S 0)`` with the extensions ``I 1`` and ``S 1``."""
    D = np.zeros((4, w, 3), dtype=bool)
    D[0, :, 2] = True
    D[0, w - 1, 0] = True
    D[1, 0, 1] = True
    D[2, 0, 0] = D[2, 1, 1] = True
    D[3, 0, 0] = D[3, 0, 1] = True
    prefix = np.array([[1]], dtype=np.int32)
    return D, prefix, np.array([0, 2], dtype=np.int64), np.array([2, 3], dtype=np.int32), np.array([1, 1])


def ones_table(w, n_seq):
    """Every item in every element, sequence ``t`` of ``t % (w + 1)`` elements: the support of an S-chain of ``k``
    items is the number of sequences with at least ``k`` elements.  Returns ``(D, lens)``."""
    lens = np.arange(n_seq) % (w + 1)
    D = np.ones((n_seq, w, 2), dtype=bool)
    D[np.arange(w)[None, :] >= lens[:, None]] = False
    return D, lens


def parse_row(s):
    """The operator's host rule for one cell of the sequence column."""
    if s is None or not s.strip():
        return []
    return [el.strip().split(ITEM_SEP) for el in s.split(ELEMENT_SEP)]


def gen_rows(seed, n, vocab, max_elements=5, max_items=3, zipf=1.0, blanks=True):
    """``n`` sequence strings over ``vocab`` with Zipf-like popularity: draws with replacement, so an element can
    repeat an item; some elements carry ASCII whitespace at their edges."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, len(vocab) + 1) ** zipf
    p /= p.sum()
    rows = []
    for _ in range(n):
        els = []
        for _ in range(int(rng.integers(1, max_elements + 1))):
            el = ITEM_SEP.join(vocab[j] for j in rng.choice(len(vocab), size=int(rng.integers(1, max_items + 1)), p=p))
            if blanks and rng.random() < 0.2:
                el = " " + el + "\t"
            els.append(el)
        rows.append(ELEMENT_SEP.join(els))
    return rows
