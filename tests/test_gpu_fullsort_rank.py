"""Rank of the ground-truth positives over the masked catalogue: ``F_.fullsort_rank`` / ``F_.fullsort_neg_sqdist_rank`` / ``F_.rank_rows``
(cdr_fullsort_rank_f32, cdr_fullsort_neg_sqdist_rank_f32, cdr_rank_rows_f32) against torch arithmetic on the matrix the EXISTING
``F_.fullsort_scores`` / ``F_.fullsort_neg_sqdist`` write for the same operands.  The counts are integers over the same score bits:
compared with ``torch.equal``, ``pos_score`` bit for bit; no tolerance anywhere.  Shapes: ``test_gpu_sqdist_topk.py``'s, which reach every
path of the scoring plan (whole MFMA tiles, slab tails, the generic GEMM, the streaming GEMV)."""
import ctypes

import pytest
import torch

from helpers import DEV

pytestmark = pytest.mark.gpu
INF = float('inf')
SHAPES = [
    (40, 128, 9000, False),       # persistent MFMA kernel, one 32-row tile per wave, slab tails of < 64 columns
    (70, 64, 70001, False),
    (600, 128, 40000, False),     # two tiles per wave, five user blocks, the last one partial
    (130, 32, 20000, False),      # D = 32: the generic GEMM
    (5, 64, 20011, False),        # U <= 8: the streaming GEMV (dot products) / the distance GEMM
    (33, 128, 64, True),          # one tile, one slab
]


def _operands(U, D, N, seed, normalize=False):
    from recbole_cdr_amd import functional as F_
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    ue, tab = torch.randn(U, D, device=DEV, generator=g), torch.randn(N, D, device=DEV, generator=g)
    return (F_.sqnorm_normalize(ue), F_.sqnorm_normalize(tab)) if normalize else (ue, tab)


def _csr(cols, U):
    indptr = torch.zeros(U + 1, dtype=torch.int64, device=DEV)
    indptr[1:] = torch.cumsum(torch.tensor([c.numel() for c in cols], device=DEV), 0)
    return indptr, torch.cat(cols).to(device=DEV, dtype=torch.int64)


def _rows_of(indptr):
    return torch.repeat_interleave(torch.arange(indptr.numel() - 1, device=DEV), indptr[1:] - indptr[:-1])


def _history(full, seed):
    """each user's 7 best columns plus 30 random ones (test_gpu_sqdist_topk.py's)"""
    U, N = full.shape
    torch.manual_seed(seed)
    best = torch.topk(torch.nan_to_num(full, nan=-INF), min(7, N), dim=1).indices
    rnd = torch.randint(0, N, (U, 30), device=DEV)
    return _csr([torch.unique(torch.cat([best[u], rnd[u]])) for u in range(U)], U)


def _masked(full, hindptr, hist, exclude_first_col):
    """masked columns -> NaN (a NaN compares false against everything: it is counted nowhere, exactly like a NaN score)"""
    m = full.clone()
    if exclude_first_col:
        m[:, 0] = float('nan')
    if hindptr is not None:
        m[_rows_of(hindptr), hist] = float('nan')
    return m


def _positives(full, masked, n0, seed, extra=None):
    """per user a random 0..12 unmasked columns plus the planted ones: the best and the worst unmasked column, column N - 1, the first
    column of slab 1, a column inside each slab's tail; user 0 has 300 random ones; users 1, 2, 3 have none"""
    U, N = full.shape
    g = torch.Generator(); g.manual_seed(seed)
    ok = ~torch.isnan(masked)
    best = torch.where(ok, full, torch.full_like(full, -INF)).argmax(1).cpu()
    worst = torch.where(ok, full, torch.full_like(full, INF)).argmin(1).cpu()
    okc = ok.cpu()
    cols = []
    for u in range(U):
        if u in (1, 2, 3):
            cols.append(torch.empty(0, dtype=torch.int64))
            continue
        c = torch.randint(0, N, (300 if u == 0 else int(torch.randint(0, 13, (1,), generator=g)),), generator=g)
        c = c[okc[u, c]]
        planted = [int(best[u]), int(worst[u]), N - 1, n0 % N, max(n0 - 2, 0), max(N - 3, 0)] + ([] if extra is None else extra[u])
        cols.append(torch.unique(torch.cat([c, torch.tensor(planted, dtype=torch.int64)])))
    return _csr(cols, U)


def _want(full, masked, pindptr, pcols):
    """the contract, by torch on the materialised matrix"""
    U, N = full.shape
    col = torch.arange(N, device=DEV).unsqueeze(0)
    gt, eq, eqb = (torch.empty(pcols.numel(), dtype=torch.int32, device=DEV) for _ in range(3))
    ptr = pindptr.tolist()
    for u in range(U):
        p0, p1 = ptr[u], ptr[u + 1]
        if p0 == p1:
            continue
        c = pcols[p0:p1]
        t = masked[u, c].unsqueeze(1)
        row = masked[u].unsqueeze(0)
        same = row == t
        bad = torch.isnan(t.squeeze(1))
        for out, val in ((gt, (row > t).sum(1)), (eq, same.sum(1)), (eqb, (same & (col < c.unsqueeze(1))).sum(1))):
            out[p0:p1] = torch.where(bad, torch.full_like(val, -1), val).to(torch.int32)
    return full[_rows_of(pindptr), pcols], gt, eq, eqb, (~torch.isnan(masked)).sum(1).to(torch.int32)


def _assert_same(got, want):
    for name, g, w in zip(('pos_score', 'gt', 'eq', 'eq_before', 'n_unmasked'), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if name == 'pos_score':
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), name          # bit for bit (NaNs included)
        else:
            assert torch.equal(g, w), (name, int((g != w).sum()), g[g != w][:5], w[g != w][:5])


def _slabs(tab, one_slab):
    n0 = tab.shape[0] if one_slab else tab.shape[0] // 3
    return n0, tab[:n0].contiguous(), (None if one_slab else tab[n0:].contiguous())


@pytest.mark.parametrize('distance', [False, True])
@pytest.mark.parametrize('U,D,N,one_slab', SHAPES)
def test_rank_matches_counts_on_the_materialised_matrix(U, D, N, one_slab, distance):
    from recbole_cdr_amd import functional as F_
    ue, tab = _operands(U, D, N, U + N, normalize=distance)
    n0, slab0, slab1 = _slabs(tab, one_slab)
    full = F_.fullsort_neg_sqdist(ue, tab) if distance else F_.fullsort_scores(ue, slab0, slab1)
    rank = F_.fullsort_neg_sqdist_rank if distance else F_.fullsort_rank
    hindptr, hist = _history(full, U + N)
    for with_hist in (True, False):
        for excl in (True, False):
            hi, hc = (hindptr, hist) if with_hist else (None, None)
            masked = _masked(full, hi, hc, excl)
            pindptr, pcols = _positives(full, masked, n0, U + N + 1)
            got = rank(ue, slab0, slab1, pindptr, pcols, hi, hc, exclude_first_col=excl)
            want = _want(full, masked, pindptr, pcols)
            _assert_same(got, want)
            ok = want[1] >= 0
            assert bool((got[2][ok] >= 1).all()) and int(ok.sum()) > 0
            if not with_hist and not excl:
                assert bool(ok.all()) and bool((got[4] == N).all())
    if distance:      # passing the column norms changes no bit
        again = rank(ue, slab0, slab1, pindptr, pcols, None, None, exclude_first_col=False, col_sqnorm=F_.row_sqnorm(tab))
        _assert_same(again, got)
    again = rank(ue, slab0, slab1, pindptr, pcols, None, None, exclude_first_col=False)
    _assert_same(again, got)                                                               # run to run


def test_rank_counts_exact_ties():
    """entries from {-1, 0, 1}: integer scores, thousands of exact ties per user; the history (best columns + random ones) holds tied
    columns"""
    from recbole_cdr_amd import functional as F_
    U, D, N = 70, 64, 5000
    g = torch.Generator(device=DEV); g.manual_seed(7)
    ue = torch.randint(-1, 2, (U, D), device=DEV, generator=g).float()
    tab = torch.randint(-1, 2, (N, D), device=DEV, generator=g).float()
    n0, slab0, slab1 = _slabs(tab, False)
    full = F_.fullsort_scores(ue, slab0, slab1)
    assert torch.equal(full, full.round()) and int((full[0] == full[0, 1]).sum()) > 50
    hindptr, hist = _history(full, 7)
    masked = _masked(full, hindptr, hist, True)
    tied_hist = (full[_rows_of(hindptr), hist].unsqueeze(1) == full[_rows_of(hindptr)]).sum(1) > 1
    assert bool(tied_hist.any())
    pindptr, pcols = _positives(full, masked, n0, 8)
    got = F_.fullsort_rank(ue, slab0, slab1, pindptr, pcols, hindptr, hist)
    _assert_same(got, _want(full, masked, pindptr, pcols))
    assert int(got[2].max()) > 100 and int(got[3].max()) > 50                               # eq, eq_before really count ties


@pytest.mark.parametrize('distance', [False, True])
def test_rank_flags_masked_and_nan_positives(distance):
    """a masked positive and a positive whose item row holds a NaN get -1 three times; a NaN column elsewhere is counted nowhere and
    n_unmasked excludes it"""
    from recbole_cdr_amd import functional as F_
    U, D, N = 70, 64, 9000
    ue, tab = _operands(U, D, N, 3, normalize=distance)
    nan_pos, nan_other = 77, N // 3 + 5
    tab[nan_pos, 3] = float('nan')
    tab[nan_other, 0] = float('nan')
    n0, slab0, slab1 = _slabs(tab, False)
    full = F_.fullsort_neg_sqdist(ue, tab) if distance else F_.fullsort_scores(ue, slab0, slab1)
    assert bool(torch.isnan(full[:, nan_pos]).all()) and bool(torch.isnan(full[:, nan_other]).all())
    hindptr, hist = _history(full, 3)
    hist_of = [hist[hindptr[u]:hindptr[u + 1]] for u in range(U)]
    extra = [[nan_pos, int(hist_of[u][len(hist_of[u]) // 2])] for u in range(U)]             # the NaN column and a history column
    masked = _masked(full, hindptr, hist, True)
    pindptr, pcols = _positives(full, masked, n0, 4, extra=extra)
    rank = F_.fullsort_neg_sqdist_rank if distance else F_.fullsort_rank
    got = rank(ue, slab0, slab1, pindptr, pcols, hindptr, hist)
    _assert_same(got, _want(full, masked, pindptr, pcols))
    prow = _rows_of(pindptr)
    in_hist = torch.zeros(U, N, dtype=torch.bool, device=DEV)
    in_hist[_rows_of(hindptr), hist] = True
    flagged = (pcols == nan_pos) | in_hist[prow, pcols] | (pcols == 0)
    for x in got[1:4]:
        assert bool((x[flagged] == -1).all()) and bool((x[~flagged] >= 0).all())
    assert int(flagged.sum()) >= 2 * (U - 3)
    n_hist_or_pad = (in_hist | (torch.arange(N, device=DEV) == 0)).sum(1)
    nan_cols = torch.zeros(N, dtype=torch.bool, device=DEV); nan_cols[[nan_pos, nan_other]] = True
    assert torch.equal(got[4].long(), N - n_hist_or_pad - (nan_cols & ~in_hist).sum(1))


@pytest.mark.parametrize('U,N', [(1, 1), (1, 63), (3, 64), (1, 65), (9, 20000)])
def test_rank_rows_strided_rows_and_column_passes(U, N):
    """``rank_rows`` on rows that are ld > N apart, in one call and as two column passes with ``col_off`` / ``accumulate``"""
    from recbole_cdr_amd import functional as F_
    g = torch.Generator(device=DEV); g.manual_seed(N)
    torch.manual_seed(N)
    big = torch.round(torch.randn(U, N + 37, device=DEV, generator=g) * 8) / 8             # steps of 1/8: ties
    scores = big[:, :N]
    assert U == 1 or scores.stride(0) == N + 37
    full = scores.contiguous()
    if N > 100:
        full[:, 500] = float('nan'); big[:, 500] = float('nan')
    hindptr, hist = _csr([torch.unique(torch.randint(0, N, (min(5, N),), device=DEV)) for _ in range(U)], U)
    for excl in (False, True):
        masked = _masked(full, hindptr, hist, excl)
        cols = [torch.unique(torch.randint(0, N, (min(9, N),))) for _ in range(U)]
        if U > 2:
            cols[1] = torch.empty(0, dtype=torch.int64)
        pindptr, pcols = _csr(cols, U)
        want = _want(full, masked, pindptr, pcols)
        got = F_.rank_rows(scores, pindptr, pcols, hindptr, hist, exclude_first_col=excl)
        _assert_same(got, want)
        if N >= 2:
            cut = N // 2 if N < 100 else 8192 + 11
            first = F_.rank_rows(big[:, cut:N], pindptr, pcols, hindptr, hist, exclude_first_col=excl, pos_score=want[0], col_off=cut)
            both = F_.rank_rows(big[:, :cut], pindptr, pcols, hindptr, hist, exclude_first_col=excl, pos_score=want[0], col_off=0,
                                out=first[1:], accumulate=True)
            _assert_same(both, want)


@pytest.mark.parametrize('U,D,N', [(70, 64, 70001), (600, 128, 40000)])
def test_rank_agrees_with_the_fused_topk(U, D, N):
    """position 1 + gt + eq_before is the positive's place in ``F_.fullsort_topk``'s list (existing code), with its value; a positive
    further down is not in the list"""
    from recbole_cdr_amd import functional as F_
    k = 20
    ue, tab = _operands(U, D, N, 1000 + U)
    n0, slab0, slab1 = _slabs(tab, False)
    full = F_.fullsort_scores(ue, slab0, slab1)
    hindptr, hist = _history(full, 1000 + U)
    masked = _masked(full, hindptr, hist, True)
    top = torch.topk(torch.nan_to_num(masked, nan=-INF), k + 6, dim=1)
    assert bool((top.values[:, :k] > top.values[:, 1:k + 1]).all()), 'a tie among the k + 1 largest: change the seed'
    extra = [top.indices[u, [0, 4, k - 1, k, k + 5]].tolist() for u in range(U)]            # positions 1, 5, k, k + 1, k + 6
    pindptr, pcols = _positives(full, masked, n0, 5, extra=extra)
    score, gt, _eq, eqb, _n = F_.fullsort_rank(ue, slab0, slab1, pindptr, pcols, hindptr, hist)
    vals, idx = F_.fullsort_topk(ue, slab0, slab1, k=k, hist_indptr=hindptr, hist_cols=hist)
    prow = _rows_of(pindptr)
    live = gt >= 0
    pos = (1 + gt + eqb).long()
    inside = live & (pos <= k)
    assert int(inside.sum()) >= 3 * (U - 3) and int((live & ~inside).sum()) >= 2 * (U - 3)
    assert torch.equal(idx[prow[inside], pos[inside] - 1], pcols[inside])
    assert torch.equal(vals[prow[inside], pos[inside] - 1].view(torch.int32), score[inside].view(torch.int32))
    outside = ~inside
    assert not bool((idx[prow[outside]] == pcols[outside].unsqueeze(1)).any())


def test_rank_without_positives_and_refusals():
    from recbole_cdr_amd import binding as B_, functional as F_
    U, D, N = 40, 64, 3001
    ue, tab = _operands(U, D, N, 5)
    full = F_.fullsort_scores(ue, tab)
    hindptr, hist = _history(full, 5)
    none = torch.zeros(U + 1, dtype=torch.int64, device=DEV)
    score, gt, eq, eqb, nun = F_.fullsort_rank(ue, tab, None, none, torch.empty(0, dtype=torch.int64, device=DEV), hindptr, hist)
    assert score.numel() == gt.numel() == eq.numel() == eqb.numel() == 0
    assert torch.equal(nun, (~torch.isnan(_masked(full, hindptr, hist, True))).sum(1).to(torch.int32))
    need = ctypes.c_size_t(0)
    B_._check(B_.load().cdr_fullsort_rank_workspace_bytes(U, D, N, 0, 1, ctypes.byref(need)), 'workspace_bytes')
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    pindptr = none.clone(); pindptr[1:] = 1
    pcols = torch.tensor([5], device=DEV)
    f, i = torch.empty(4, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV)
    n_out = torch.full((U,), -7, dtype=torch.int32, device=DEV)

    def call(outs, nbytes):
        B_.call('cdr_fullsort_rank_f32', B_.stream(), B_.f32(ue), U, D, B_.f32(tab), N, None, 0, B_.i64(pindptr), B_.i64(pcols), None, None, 1,
                *outs, B_.raw(ws), nbytes)

    with pytest.raises(RuntimeError, match='invalid argument'):
        call((B_.f32(f), B_.raw(i), None, B_.raw(i), B_.raw(n_out)), need.value)
    with pytest.raises(RuntimeError, match='workspace'):
        call((B_.f32(f), B_.raw(i), B_.raw(i), B_.raw(i), B_.raw(n_out)), need.value - 1)
    torch.cuda.synchronize()
    assert bool((n_out == -7).all())                                                         # refused: nothing was launched
