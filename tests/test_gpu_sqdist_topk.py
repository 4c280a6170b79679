"""SSCDR's distance score under the fused mask + top-k: ``F_.fullsort_neg_sqdist_topk`` (cdr_fullsort_neg_sqdist_topk_f32) against
``torch.topk`` of the evaluation-masked matrix ``F_.fullsort_neg_sqdist`` writes for the same operands.  The two kernels run the same MFMA
chain over the same k pairs in the same order, take their norms from the same kernel and apply the same expression, so the values must be
BIT-equal; columns may differ only between exactly tied scores.  Shapes: the smallest that reach each path of the plan."""
import pytest
import torch

from helpers import DEV

pytestmark = pytest.mark.gpu
NEG_INF = -float('inf')


def _operands(U, D, N, seed):
    from recbole_cdr_amd import functional as F_
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    torch.manual_seed(seed)                                                      # (the tests' random histories)
    ue = F_.sqnorm_normalize(torch.randn(U, D, device=DEV, generator=g))
    tab = F_.sqnorm_normalize(torch.randn(N, D, device=DEV, generator=g))
    return ue, tab


def _csr(cols, U):
    indptr = torch.zeros(U + 1, dtype=torch.int64, device=DEV)
    indptr[1:] = torch.cumsum(torch.tensor([c.numel() for c in cols], device=DEV), 0)
    return indptr, torch.cat(cols)


def _masked(full, indptr, hist, exclude_first_col=True):
    masked = full.clone()
    if exclude_first_col:
        masked[:, 0] = NEG_INF
    if indptr is not None:
        masked[torch.repeat_interleave(torch.arange(full.shape[0], device=DEV), indptr[1:] - indptr[:-1]), hist] = NEG_INF
    return masked


def _assert_topk_of(masked, k, got_v, got_i):
    """values bit-equal to torch.topk's (NaN never ranks: torch.topk would put it first), columns gather them, no column twice, (-inf, -1)
    where the row has run out of unmasked columns"""
    want_v = torch.topk(torch.where(torch.isnan(masked), torch.full_like(masked, NEG_INF), masked), k, dim=1).values
    assert torch.equal(got_v, want_v), (got_v - want_v).abs().max()
    live = got_v > NEG_INF
    assert bool((got_i[~live] == -1).all()) and bool((got_i[live] >= 0).all())
    gathered = torch.gather(masked, 1, got_i.clamp(min=0))
    assert torch.equal(torch.where(live, gathered, want_v), want_v)              # only exact ties may swap
    uniq = torch.where(live, got_i, -1 - torch.arange(k, device=DEV).expand_as(got_i)).sort(1).values
    assert int((uniq[:, 1:] == uniq[:, :-1]).sum()) == 0


@pytest.mark.parametrize('U,D,N,k,one_slab', [
    (40, 128, 9000, 10, False),       # fused, MT = 1, one partial user block, slab tails of < 64 columns
    (70, 64, 70001, 20, False),       # > 2 tiles per stripe at 256 stripes: the in-register fast path and the queues, not only slow_scan
    (600, 128, 40000, 10, False),     # MT = 2, five user blocks, the last one partial
    (130, 32, 20000, 5, False),       # D = 32: the unfused passes (distance GEMM + topk_rows_kernel)
    (5, 64, 20011, 10, False),        # U <= 8: the unfused passes
    (33, 128, 64, 64, True),          # rows left with fewer than k unmasked columns: (-inf, -1)
])
def test_sqdist_topk_matches_topk_of_masked_distances(U, D, N, k, one_slab):
    from recbole_cdr_amd import functional as F_
    ue, tab = _operands(U, D, N, U + N)
    n0 = N if one_slab else N // 3
    slab0, slab1 = tab[:n0].contiguous(), (None if one_slab else tab[n0:].contiguous())
    full = F_.fullsort_neg_sqdist(ue, tab)
    best = torch.topk(full, min(7, N), dim=1).indices                            # each user's 7 best columns go into its history ...
    rnd = torch.randint(0, N, (U, 30), device=DEV)                               # ... with 30 random ones
    indptr, hist = _csr([torch.unique(torch.cat([best[u], rnd[u]])) for u in range(U)], U)
    got_v, got_i = F_.fullsort_neg_sqdist_topk(ue, slab0, slab1, k=k, hist_indptr=indptr, hist_cols=hist)
    _assert_topk_of(_masked(full, indptr, hist), k, got_v, got_i)
    if N - k < 40:
        assert bool((got_i == -1).any())                                         # the case exists for the padding
    # no history, PAD column kept: plain top-k of the matrix
    got_v2, got_i2 = F_.fullsort_neg_sqdist_topk(ue, slab0, slab1, k=k, exclude_first_col=False)
    _assert_topk_of(full, k, got_v2, got_i2)


@pytest.mark.parametrize('U,D,k,two_slabs', [(70, 64, 10, False), (520, 128, 10, True)])
def test_sqdist_topk_seeded_thresholds(U, D, k, two_slabs):
    """Past 16 x 65,536 columns a sample call seeds every stripe's threshold.  Exact ties at the sample's k-th value (item rows copied
    inside and outside the sample); the history masks each user's best SAMPLE columns, so the seed must be the k-th value of the MASKED
    sample."""
    from recbole_cdr_amd import functional as F_
    N = 16 * 65536 + 4097
    ue, tab = _operands(U, D, N, U + k)
    torch.manual_seed(U + k)
    src = torch.randint(1, 65536, (3000,), device=DEV)
    tab[torch.randint(65536, N, (3000,), device=DEV)] = tab[src]
    tab[torch.randint(1, 65536, (500,), device=DEV)] = tab[src[:500]]
    n0 = N if not two_slabs else 9 * 65536 + 13
    slab0, slab1 = tab[:n0].contiguous(), (tab[n0:].contiguous() if two_slabs else None)
    full = F_.fullsort_neg_sqdist(ue, tab)
    best_sample = torch.topk(full[:, :65536], 12, dim=1).indices
    best_all = torch.topk(full, 5, dim=1).indices
    indptr, hist = _csr([torch.unique(torch.cat([best_sample[u], best_all[u]])) for u in range(U)], U)
    got_v, got_i = F_.fullsort_neg_sqdist_topk(ue, slab0, slab1, k=k, hist_indptr=indptr, hist_cols=hist)
    full[:, 0] = NEG_INF                                                         # (in place: the matrix is 2 GB at 520 users)
    full[torch.repeat_interleave(torch.arange(U, device=DEV), indptr[1:] - indptr[:-1]), hist] = NEG_INF
    _assert_topk_of(full, k, got_v, got_i)


def test_sqdist_topk_never_ranks_a_nan_column():
    """Column 0 scores NaN for every user.  (``F_.sqnorm_normalize`` divides by max(|x|^2, 1), so a zero row stays zero -- that finite
    case is checked first; the NaN a plain x / |x|^2 would leave there is planted in the normalised table.)  No list and no threshold may
    take it: with the PAD mask the result is the masked reference; without it column 0 is still never returned and all values are finite."""
    from recbole_cdr_amd import functional as F_
    U, D, N, k = 70, 64, 9000, 10
    g = torch.Generator(device=DEV); g.manual_seed(3)
    torch.manual_seed(3)
    ue = F_.sqnorm_normalize(torch.randn(U, D, device=DEV, generator=g))
    raw = torch.randn(N, D, device=DEV, generator=g)
    raw[0] = 0.0
    tab = F_.sqnorm_normalize(raw)
    for plant_nan in (False, True):
        if plant_nan:
            tab[0] = float('nan')
        n0 = N // 3
        slab0, slab1 = tab[:n0].contiguous(), tab[n0:].contiguous()
        full = F_.fullsort_neg_sqdist(ue, tab)
        assert bool(torch.isnan(full[:, 0]).all()) == plant_nan and not bool(torch.isnan(full[:, 1:]).any())
        best = torch.topk(full[:, 1:], 7, dim=1).indices + 1
        indptr, hist = _csr([torch.unique(torch.cat([best[u], torch.randint(0, N, (30,), device=DEV)])) for u in range(U)], U)
        got_v, got_i = F_.fullsort_neg_sqdist_topk(ue, slab0, slab1, k=k, hist_indptr=indptr, hist_cols=hist)
        _assert_topk_of(_masked(full, indptr, hist), k, got_v, got_i)
        got_v2, got_i2 = F_.fullsort_neg_sqdist_topk(ue, slab0, slab1, k=k, hist_indptr=indptr, hist_cols=hist, exclude_first_col=False)
        assert bool(torch.isfinite(got_v2).all())
        if plant_nan:
            assert not bool((got_i2 == 0).any())
        _assert_topk_of(_masked(full, indptr, hist, exclude_first_col=False), k, got_v2, got_i2)


@pytest.mark.parametrize('U,D,N', [(70, 64, 9000), (130, 32, 5000)])
def test_col_sqnorm_argument_changes_no_bit(U, D, N):
    from recbole_cdr_amd import functional as F_
    ue, tab = _operands(U, D, N, 11)
    n0 = N // 3
    slab0, slab1 = tab[:n0].contiguous(), tab[n0:].contiguous()
    a_v, a_i = F_.fullsort_neg_sqdist_topk(ue, slab0, slab1, k=10)
    b_v, b_i = F_.fullsort_neg_sqdist_topk(ue, slab0, slab1, k=10, col_sqnorm=F_.row_sqnorm(tab))
    assert torch.equal(a_v, b_v) and torch.equal(a_i, b_i)


def test_row_sqnorm_is_the_distance_entry_s_column_norm():
    from recbole_cdr_amd import binding as B_, functional as F_
    U, D, N = 40, 64, 3001
    ue, tab = _operands(U, D, N, 5)
    scratch = torch.empty(U + N, device=DEV)
    out = torch.empty(U, N, device=DEV)
    B_.call('cdr_fullsort_neg_sqdist_f32', B_.stream(), B_.f32(ue), U, D, B_.f32(tab), N, B_.f32(scratch), B_.f32(out))
    assert torch.equal(F_.row_sqnorm(tab), scratch[U:]) and torch.equal(F_.row_sqnorm(ue), scratch[:U])
