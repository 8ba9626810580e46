"""Stochastic Outlier Selection on the GPU (``csrc/sos.hip`` through ``ops/sos.py``) against the longdouble oracle of
``sos_helpers``: the search bit for bit on the rows that are not fragile, the products within their bound, the same
bits for every grid, run, range split and row alignment, bounded memory, and the operator on device columns."""
import numpy as np
import pytest
import torch

import sos_helpers as H
from alink_amd.models.outlier import sos as M
from alink_amd.ops import sos as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COMPARED = {}


def _x(c):
    return torch.from_numpy(c.X).to(DEV)


def _id(s):
    return f"seed{s[0]}-n{s[1]}-d{s[2]}"


@pytest.mark.parametrize("spec", H.CASES + H.SWEEP, ids=_id)
def test_search_and_products_match_oracle(spec):
    c = H.case(*spec)
    X = _x(c)
    assert S.sos_selected(X) or X.shape[1] > S.SOS_MAX_D
    before = S.SOS_CALLS
    beta, s, iters = S.search(X, c.perplexity)
    p = S.products(X, beta, s)
    assert S.SOS_CALLS == before + 2
    COMPARED[spec] = (H.check_search(c, beta, s, iters), X.shape[0])
    H.check_products(c, beta, s, p)


def test_sweep_compares_95_percent_of_rows():
    for spec in H.SWEEP:
        if spec not in COMPARED:        # when run alone
            c = H.case(*spec)
            COMPARED[spec] = (int((~c.fragile).sum()), len(c.fragile))
    done = sum(COMPARED[s][0] for s in H.SWEEP)
    total = sum(COMPARED[s][1] for s in H.SWEEP)
    print("rows compared", done, "of", total)
    assert done >= 0.95 * total


@pytest.mark.parametrize("spec", (H.CASES[0], H.CASES[1], H.CASES[8]), ids=_id)
def test_same_bits_for_every_grid_and_run(spec):
    c = H.case(*spec)
    X = _x(c)
    ref = S.search(X, c.perplexity)
    pref = S.products(X, ref[0], ref[1])
    for grid in (0, 1, 7, 7):
        got = S.search(X, c.perplexity, grid=grid)
        for a, b in zip(ref, got):
            assert torch.equal(a, b)
        assert torch.equal(pref, S.products(X, ref[0], ref[1], grid=grid))


def test_row_ranges_concatenate_bit_equal():
    c = H.case(*H.CASES[0])
    X = _x(c)
    n = X.shape[0]
    full = S.search(X, c.perplexity)
    pfull = S.products(X, full[0], full[1])
    cuts = (0, 1, 64, 65, n)
    parts = [S.search(X, c.perplexity, rows=(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    for i in range(3):
        assert torch.equal(full[i], torch.cat([p[i] for p in parts]))
    assert torch.equal(pfull, torch.cat([S.products(X, full[0], full[1], cols=(a, b))
                                         for a, b in zip(cuts[:-1], cuts[1:])]))
    empty = S.search(X, c.perplexity, rows=(5, 5))
    assert all(t.numel() == 0 for t in empty)


@pytest.mark.parametrize("spec", (H.CASES[0], H.CASES[1]), ids=_id)      # d = 5 and d = 33
def test_offset_rows_same_bits(spec):
    c = H.case(*spec)
    X = _x(c)
    flat = torch.empty(X.numel() + 2, dtype=torch.float64, device=DEV)
    base = 1 if flat.data_ptr() % 16 == 0 else 2
    Xo = flat[base:base + X.numel()].view(X.shape).copy_(X)
    assert Xo.data_ptr() % 16 == 8 and Xo.is_contiguous() and S.sos_selected(Xo)
    ref = S.search(X, c.perplexity)
    got = S.search(Xo, c.perplexity)
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    assert torch.equal(S.products(X, ref[0], ref[1]), S.products(Xo, ref[0], ref[1]))


def test_memory_stays_linear_in_n():
    """Scratch above the inputs: the image and the padded copy it is permuted from (n x 32 x 8 bytes each at d <= 32),
    the centred rows and the temporaries of centring (3 x n d x 8 = 0.75 of it at d = 8) and a dozen [n] vectors:
    under 3 such units, so 4 is allowed.  A [4096, n] block would be 32 units."""
    n, d = 4096, 8
    X = torch.randn((n, d), dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    S.scores(X, 30.0)                           # warm: the library and the allocator
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    p = S.scores(X, 30.0)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak bytes", peak, "units", peak / (n * 32 * 8))
    assert p is not None and p.shape == (n,)
    assert peak < 4 * n * 32 * 8


def test_operator_on_device_blocks(monkeypatch):
    c = H.case(*H.CASES[0])
    before = S.SOS_CALLS
    got = H.run_op(H.vector_table(c.X, DEV), c.perplexity, DEV)
    assert S.SOS_CALLS == before + 2
    H.check_scores(c, torch.from_numpy(got))
    # a CSR column 20 wide: the case's 5 columns spread over 20
    wide = np.zeros((c.X.shape[0], 20))
    wide[:, [0, 3, 7, 12, 19]] = c.X
    before = S.SOS_CALLS
    got = H.run_op(H.csr_table(wide, DEV), c.perplexity, DEV)
    assert S.SOS_CALLS == before + 2
    H.check_scores(c, torch.from_numpy(got))
    # ALINK_SOS_HIP=0: the former function, bit for bit
    monkeypatch.setenv("ALINK_SOS_HIP", "0")
    before = S.SOS_CALLS
    got = H.run_op(H.vector_table(c.X, DEV), c.perplexity, DEV)
    want = M.sos_scores(_x(c), c.perplexity).cpu().numpy()
    assert S.SOS_CALLS == before
    assert np.array_equal(got, want)
