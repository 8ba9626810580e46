"""Exact fp64 oracle for the nearest-centroid kernels, with derived (not tuned) slack, and the input families that
exercise ties, padding, magnitude and long fp32 sums.  A plain module: ``tests/test_kmeans_oracle.py`` validates it
on the CPU paths, ``tests/test_kmeans_oracle_gpu.py`` holds the HIP kernels to it.

The operation.  Rows ``X`` are bf16, centroids ``C`` fp64.  The operand preparation rounds ``C`` to bf16 (``cb``);
every path then takes ``argmax_c s[r,c]`` with ``s[r,c] = x_r . cb_c - |cb_c|^2 / 2`` (== argmin of the squared
distance).  Here ``s`` is formed in fp64 from the exact bf16 values: a product of two bf16 numbers has 16
significant bits, so it is exact, and the 129-term fp64 sum is off by at most ``129 * 2^-53`` relative -- nothing
next to what follows.

What a correct kernel may get wrong, per row r (``e_r``):

* the fp32 sum.  The kernels start the MFMA accumulator at ``-|cb_c|^2/2`` and add the 128 exact products in fp32,
  in some order.  The standard bound for an n-term fp32 sum in any order is ``(n-1) u sum|t_i|`` (to first
  order) with ``u = 2^-24``; with the rounding of the init term itself, for 129 terms
  ``|s32 - s| <= 129 * 2^-24 * (sum_j |x_rj cb_cj| + |cb_c|^2/2)``.  Both the winner and the runner-up carry such
  an error, so ``e_r`` takes the maximum over c.
* the packed argmax.  The fused kernels overwrite the 7 low mantissa bits of the fp32 score with an index field:
  the compared value is the score truncated to 17 significant bits, off by less than ``2^-16 |s32|``.  Maximised
  over c: ``2^-16 * max_c |s[r,c]|``.
* the absolute floor.  Below the smallest fp32 normal, ``2^-126``, the matrix pipeline may flush and relative bounds
  mean nothing; ``e_r`` is at least that.

``e_r`` is the sum of the three.  If the kernel prefers a over the true best b, then
``s_b - e_r <= s32_b~ <= s32_a~ <= s_a + e_r``, so ``s_b - s_a <= 2 e_r``: the acceptable set of row r is
``{c < k : s_best - s[r,c] <= 2 e_r}``.  A row whose set is a singleton is *decided*: every correct kernel returns
that index.

Exact ties.  When every entry of a row and of the centroids is a small multiple of a power of two, each product and
``|cb_c|^2/2`` is a multiple of a quantum ``q``; if ``sum_j |x_rj cb_cj| + |cb_c|^2/2 < 2^24 q`` for every c,
every partial sum of the fp32 computation, in any order, is an integer multiple of q below ``2^24 q`` and therefore
exact.  The fp32 scores of such a row equal ``s`` bit for bit, and two centroids with equal ``s`` are a *bit-exact
tie*: the rule of the project (``argmax``, a strict ``<`` in the reference's closest-centre loop) gives the row to
the LOWEST tied index.  A row is reported as a tie row only when, in addition, nothing but the tied centroids is in
its acceptable set, so that the truncation cannot bring a third centroid into play.

Sums.  Given the kernel's own assignment ``a``, cluster c holds ``m_c`` rows; the kernels add them in fp32 in some
grouping (per wave, per workgroup) and then reduce the per-workgroup partials in fp64.  Any such scheme is a
summation tree of depth at most ``m_c`` over exactly representable terms, so per (cluster, dim)
``|sum32 - sum| <= m_c * 2^-24 * sum_{r in c} |x_rj|`` -- the worst-case sequential bound, which dominates every
shallower tree.  Counts are integers below 2^24 per workgroup and must be equal.  No additive term.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import torch

U = 2.0 ** -24          # fp32 unit roundoff
TRUNC = 2.0 ** -16      # 7 mantissa bits dropped from a 24-bit significand
FLOOR = 2.0 ** -126     # smallest fp32 normal
D = 128


class Oracle(NamedTuple):
    s: torch.Tensor          # [n, k] fp64 scores
    e: torch.Tensor          # [n] fp64 error bound e_r
    accept: torch.Tensor     # [n, k] bool acceptable sets
    decided: torch.Tensor    # [n] bool: singleton set
    tie: torch.Tensor        # [n] bool: bit-exact tie (see the module docstring)
    expected: torch.Tensor   # [n] int64: lowest index holding the best fp64 score (binding on decided | tie rows)

    @property
    def pinned(self) -> torch.Tensor:
        return self.decided | self.tie


def _low_exponent(v: torch.Tensor) -> torch.Tensor:
    """Exponent of the lowest set bit of every bf16-exact fp64 value (a large number for zeros)."""
    m, ex = torch.frexp(v)
    mi = (m.abs() * 256.0).to(torch.int64)              # 8 significant bits -> an integer in [128, 256)
    low = torch.log2((mi & -mi).clamp_min(1).double()).to(torch.int64)
    out = ex.to(torch.int64) - 8 + low
    return torch.where(v == 0, torch.full_like(out, 4096), out)


def oracle(X: torch.Tensor, C: torch.Tensor) -> Oracle:
    """The acceptable sets of every row of X (bf16 [n, d]) against the centroids C (fp64 [k, d]); CPU, fp64."""
    assert X.dtype == torch.bfloat16 and C.dtype == torch.float64
    Xd = X.detach().cpu().double()
    Cb = C.detach().cpu().to(torch.bfloat16).double()
    half = 0.5 * (Cb * Cb).sum(1)
    s = Xd @ Cb.T - half
    mag = Xd.abs() @ Cb.abs().T + half                   # sum_j |x_rj cb_cj| + |cb_c|^2/2
    e = 129.0 * U * mag.max(1).values + TRUNC * s.abs().max(1).values + FLOOR
    best = s.max(1, keepdim=True).values
    accept = (best - s) <= 2.0 * e[:, None]
    decided = accept.sum(1) == 1
    top = s == best
    expected = top.to(torch.int8).argmax(1)              # first maximal value: the lowest tied index
    # fp32-exact rows: quantum of the products and of |c|^2/2, all magnitudes below 2^24 quanta
    ex = _low_exponent(Xd).min(1).values
    ec = int(_low_exponent(Cb).min()) if Cb.numel() else 4096
    qexp = torch.minimum(ex + ec, torch.full_like(ex, 2 * ec - 1)).clamp(-2000, 2000)
    q = torch.ldexp(torch.ones_like(e), qexp.to(torch.int32))
    exact = (mag.max(1).values < 2.0 ** 24 * q) & (q >= FLOOR)
    tie = exact & (top.sum(1) >= 2) & (accept == top).all(1)
    return Oracle(s, e, accept, decided, tie, expected)


def check_assignment(o: Oracle, a: torch.Tensor, k: int, what: str = "") -> None:
    """``a`` [n]: every index in range and in its row's acceptable set; equal to the expected index on decided
    rows and on bit-exact tie rows (the lowest tied index)."""
    a = a.detach().cpu().to(torch.int64)
    n = o.s.shape[0]
    assert a.shape == (n,), what
    assert int(a.min()) >= 0 and int(a.max()) < k, f"{what}: index out of [0, {k})"
    inside = o.accept.gather(1, a[:, None])[:, 0]
    bad = (~inside).nonzero()[:, 0]
    assert bad.numel() == 0, (f"{what}: {bad.numel()} rows outside the acceptable set, first row {int(bad[0])}: "
                              f"got {int(a[bad[0]])}, best {int(o.expected[bad[0]])}")
    wrong = (o.pinned & (a != o.expected)).nonzero()[:, 0]
    assert wrong.numel() == 0, (f"{what}: {wrong.numel()} decided / tied rows differ, first row {int(wrong[0])}: "
                                f"got {int(a[wrong[0]])}, expected {int(o.expected[wrong[0]])} "
                                f"(tie row: {bool(o.tie[wrong[0]])})")


def check_sums(X: torch.Tensor, a: torch.Tensor, got: torch.Tensor, k: int, what: str = "") -> None:
    """``got`` [k, d+1] = [sum_x | count] against the fp64 sums of X by the assignment ``a``: counts equal, sums
    within ``m_c 2^-24 sum_{r in c} |x_rj|`` (module docstring), nothing added."""
    Xd = X.detach().cpu().double()
    a = a.detach().cpu().to(torch.int64)
    got = got.detach().cpu().double()
    n, d = Xd.shape
    ref = torch.zeros((k, d), dtype=torch.float64).index_add_(0, a, Xd)
    mag = torch.zeros((k, d), dtype=torch.float64).index_add_(0, a, Xd.abs())
    cnt = torch.bincount(a, minlength=k).double()
    assert torch.equal(got[:, d], cnt), f"{what}: counts differ from the assignment's"
    assert float(got[:, d].sum()) == n, what
    err = (got[:, :d] - ref).abs()
    tol = cnt[:, None] * U * mag
    over = err > tol
    assert not bool(over.any()), (f"{what}: {int(over.sum())} sums outside m_c 2^-24 sum|x|; worst err/tol "
                                  f"{float((err / tol.clamp_min(1e-300))[over].max()):.3g}")


def check_counts(o: Oracle, counts: torch.Tensor, k: int, what: str = "") -> None:
    """Counts-only paths: a count vector is right when it is reachable by an assignment inside the acceptable
    sets -- at least the pinned rows of c, at most the rows that accept c -- and sums to n."""
    counts = counts.detach().cpu().to(torch.int64)[:k]
    n = o.s.shape[0]
    assert int(counts.sum()) == n, f"{what}: counts sum to {int(counts.sum())}, not {n}"
    lo = torch.bincount(o.expected[o.pinned], minlength=k)
    hi = o.accept.sum(0)
    assert bool(((counts >= lo) & (counts <= hi)).all()), f"{what}: counts {counts.tolist()} outside [{lo.tolist()}, {hi.tolist()}]"


# ------------------------------------------------------------------------------------------------------------------
# input families (CPU tensors: X bf16 [n, 128], C fp64 [k, 128] with bf16-exact values unless stated)
# ------------------------------------------------------------------------------------------------------------------

def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(seed)


def _int_centroids(k: int, g: torch.Generator, lo: int = -2, hi: int = 2) -> torch.Tensor:
    """k distinct centroids of small non-zero integers (norms 128 .. 512: far apart)."""
    v = torch.randint(lo, hi, (k, D), generator=g).double()
    return torch.where(v >= 0, v + 1.0, v)                # {-2, -1, 1, 2}


def dup_groups(k: int):
    """Duplicate-centroid groups: (0, k-1), an adjacent pair inside one 16-block, a pair straddling a 16-block
    boundary and a triple; fewer where k has no room."""
    if k >= 100:
        return [(0, k - 1), (5, 6), (15, 16), (33, 50, 97)]
    if k >= 20:
        return [(0, k - 1), (5, 6), (15, 16), (2, 9, 17)]
    return [(0, k - 1)] if k >= 2 else []


@functools.lru_cache(maxsize=None)
def tie_family(k: int, origin: bool = False, seed: int = 0):
    """Exact ties of both signs.  The duplicated centroids have entries in {-1, 0, 1} (the smallest norms, so the
    zero rows tie on them too), the second and later copies with -0.0 where the first has +0.0.  Rows, for every
    centroid c: 2c (positive best score), c/4 (negative best score), -c (negative scores, the winner is another
    centroid), then rows of +0.0 and of -0.0.  ``origin``: the (0, k-1) pair sits exactly at the origin, so the
    zero rows' best score is +-0 and its packed form a denormal bit pattern."""
    g = _gen(1000 + 7 * k + seed)
    C = _int_centroids(k, g)
    for gi, grp in enumerate(dup_groups(k)):
        base = torch.randint(-1, 2, (D,), generator=g).double()
        base[: 8 + 4 * gi] = 0.0                          # distinct norms per group; the triple's is the smallest
        if origin and gi == 0:
            base = torch.zeros(D, dtype=torch.float64)
        for j, c in enumerate(grp):
            C[c] = torch.where(base == 0, torch.tensor(-0.0 if j else 0.0, dtype=torch.float64), base)
    rows = [2.0 * C, 0.25 * C, -C, torch.zeros(2, D, dtype=torch.float64), -torch.zeros(2, D, dtype=torch.float64)]
    X = torch.cat(rows).to(torch.bfloat16)
    assert torch.equal(X.double(), torch.cat(rows))       # representable
    return X, C


@functools.lru_cache(maxsize=None)
def padding_family(k: int, n: int, seed: int = 0):
    """The winner sits at index k-1, next to the padded slots.  Every centroid is b + noise with b = 4 * ones;
    centroid k-1 is b/2 + noise.  A third of the rows is c_{k-1} itself (positive best score), a third
    -2^12 * b (every real score hugely negative, k-1 the least: a -3e38 pad slot must still lose), a third small
    random integers."""
    g = _gen(2000 + 131 * k + n + seed)
    b = torch.full((D,), 4.0, dtype=torch.float64)
    C = b + torch.randint(-1, 2, (k, D), generator=g).double()
    C[k - 1] = 0.5 * b + torch.randint(-1, 2, (D,), generator=g).double()
    kind = torch.arange(n) % 3
    X = torch.randint(-3, 4, (n, D), generator=g).double()
    X[kind == 0] = C[k - 1]
    X[kind == 1] = -(2.0 ** 12) * b
    return X.to(torch.bfloat16), C


@functools.lru_cache(maxsize=None)
def blob_family(n: int, k: int, scale_exp: int, seed: int = 0):
    """Well-separated blobs (centres 4 * randn, unit noise, centroids = centres + 0.3 * randn) with every entry
    scaled by 2^scale_exp (exact in bf16): scores of about 2^(2 scale_exp + 11)."""
    g = _gen(3000 + n + 17 * k + seed)
    centers = torch.randn(k, D, generator=g) * 4
    lab = torch.randint(0, k, (n,), generator=g)
    X = (centers[lab] + torch.randn(n, D, generator=g)).to(torch.bfloat16)
    C = (centers + 0.3 * torch.randn(k, D, generator=g)).to(torch.bfloat16).double()
    sc = 2.0 ** scale_exp
    return (X.double() * sc).to(torch.bfloat16), C * sc


@functools.lru_cache(maxsize=None)
def offset_family(n: int, k: int, seed: int = 0):
    """Un-centred blobs: centres 64 + randn (mean 64, spread 1), rows = centre + noise of 1/4, everything on the
    bf16 grid (spacing 1/2 at 64).  |c|^2 is about 5e5 while the centres are 16 apart: the scores cancel to
    1 part in 4000 of their terms."""
    g = _gen(4000 + n + 17 * k + seed)
    centers = (64.0 + torch.randn(k, D, generator=g)).to(torch.bfloat16)
    lab = torch.randint(0, k, (n,), generator=g)
    X = (centers.float()[lab] + 0.25 * torch.randn(n, D, generator=g)).to(torch.bfloat16)
    return X, centers.double()


@functools.lru_cache(maxsize=None)
def one_cluster_family(n: int = 70001, k: int = 100, seed: int = 0):
    """One real cluster: every row is centroid 0 plus unit noise, scaled by 2^8; the other k-1 centroids lie
    far away.  One cluster's rows are then summed in fp32 by as few workgroups as the grid has."""
    g = _gen(5000 + n + k + seed)
    centers = torch.randn(k, D, generator=g) * 4
    X = ((centers[0] + torch.randn(n, D, generator=g)).to(torch.bfloat16).double() * 256.0).to(torch.bfloat16)
    return X, centers.to(torch.bfloat16).double() * 256.0


@functools.lru_cache(maxsize=None)
def cached_oracle(family: str, *args) -> Oracle:
    """The oracle of ``<family>_family(*args)``, computed once per process and shared by the tests."""
    X, C = globals()[family + "_family"](*args)
    return oracle(X, C)
