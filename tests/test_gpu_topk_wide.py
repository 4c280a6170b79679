"""Mask + top-k lists beyond 64 entries (1 <= k <= 1,024): ``F_.fullsort_topk_wide`` / ``F_.fullsort_neg_sqdist_topk_wide`` /
``F_.topk_rows`` (cdr_fullsort_topk_wide_f32, cdr_fullsort_neg_sqdist_topk_wide_f32, cdr_topk_rows_f32), the models'
``full_sort_topk(k > 64)`` / ``full_sort_topk_wide`` and ``Trainer.evaluate`` with ``eval_route='topk'``.  The wanted result everywhere is
the stable descending sort of the masked matrix the EXISTING ``F_.fullsort_scores`` / ``F_.fullsort_neg_sqdist`` / ``full_sort_predict``
write for the same operands: masked and NaN entries -> -inf, entries equal to -inf dropped, (-inf, -1) behind them.  Values are compared
bit for bit and columns with ``torch.equal``: no tolerance anywhere (the trainer's metric dicts: the 1e-7 of the existing route pair)."""
import pytest
import torch

from helpers import DEV, base_config
from test_gpu_fullsort_rank import SHAPES, _csr, _history, _operands, _rows_of, _slabs

pytestmark = pytest.mark.gpu
INF = float('inf')
NAN = float('nan')


def _sorted_masked(full, hindptr=None, hist=None, exclude_first_col=True):
    """(values, columns) of every row of the masked matrix in the total order: score descending, then column ascending"""
    m = torch.nan_to_num(full.clone().float(), nan=-INF, posinf=INF, neginf=-INF)
    if exclude_first_col:
        m[:, 0] = -INF
    if hindptr is not None:
        m[_rows_of(hindptr), hist] = -INF
    return torch.sort(m, dim=1, descending=True, stable=True)


def _first_k(sv, si, k):
    U, N = sv.shape
    kk = min(k, N)
    vals = torch.full((U, k), -INF, device=DEV)
    idx = torch.full((U, k), -1, dtype=torch.int64, device=DEV)
    vals[:, :kk] = sv[:, :kk]
    idx[:, :kk] = torch.where(sv[:, :kk] == -INF, torch.full_like(si[:, :kk], -1), si[:, :kk])
    return vals, idx


def _want(full, k, hindptr=None, hist=None, exclude_first_col=True):
    return _first_k(*_sorted_masked(full, hindptr, hist, exclude_first_col), k)


def _assert_lists(got, want, what=''):
    (gv, gi), (wv, wi) = got, want
    assert gv.dtype == torch.float32 and gi.dtype == torch.int64 and gv.shape == wv.shape and gi.shape == wi.shape, what
    bad = gi != wi
    assert not bool(bad.any()), (what, int(bad.sum()), torch.nonzero(bad)[:4].tolist(), gi[bad][:4].tolist(), wi[bad][:4].tolist())
    assert torch.equal(gv.view(torch.int32), wv.view(torch.int32)), what                       # bit for bit
    pad = gi < 0
    assert bool((gv[pad] == -INF).all()) and bool((gi[pad] == -1).all()) and bool((gv[~pad] > -INF).all()), what


@pytest.mark.parametrize('distance', [False, True])
@pytest.mark.parametrize('U,D,N,one_slab', SHAPES)
def test_lists_match_the_sorted_masked_matrix(U, D, N, one_slab, distance):
    from recbole_cdr_amd import functional as F_
    ue, tab = _operands(U, D, N, U + N, normalize=distance)
    n0, slab0, slab1 = _slabs(tab, one_slab)
    full = F_.fullsort_neg_sqdist(ue, tab) if distance else F_.fullsort_scores(ue, slab0, slab1)
    wide = F_.fullsort_neg_sqdist_topk_wide if distance else F_.fullsort_topk_wide
    hindptr, hist = _history(full, U + N)
    ks = (65, 100, 1000) + ((1024,) if (U, N) == (70, 70001) else ())
    got = None
    for with_hist in (True, False):
        for excl in (True, False):
            hi, hc = (hindptr, hist) if with_hist else (None, None)
            sv, si = _sorted_masked(full, hi, hc, excl)
            for k in ks:
                got = wide(ue, slab0, slab1, k, hi, hc, exclude_first_col=excl)
                _assert_lists(got, _first_k(sv, si, k), (k, with_hist, excl))
    k = ks[-1]
    again = wide(ue, slab0, slab1, k, None, None, exclude_first_col=False)
    assert torch.equal(again[0].view(torch.int32), got[0].view(torch.int32)) and torch.equal(again[1], got[1])      # run to run
    if distance:      # passing the column norms changes no bit
        again = wide(ue, slab0, slab1, k, None, None, exclude_first_col=False, col_sqnorm=F_.row_sqnorm(tab))
        assert torch.equal(again[0].view(torch.int32), got[0].view(torch.int32)) and torch.equal(again[1], got[1])


def _tie_operands(U, D, N, seed):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    return (torch.randint(-1, 2, (U, D), device=DEV, generator=g).float(), torch.randint(-1, 2, (N, D), device=DEV, generator=g).float())


@pytest.mark.parametrize('N,k', [(20011, 300), (8191, 100), (8192, 100), (8193, 100)])
def test_exact_ties_resolve_to_the_smaller_column(N, k):
    """operands from {-1, 0, 1}: integer scores, thousands of exact ties per user, across block, stripe and slab boundaries"""
    from recbole_cdr_amd import functional as F_
    U, D = 9, 64
    ue, tab = _tie_operands(U, D, N, N)
    n0, slab0, slab1 = _slabs(tab, False)
    full = F_.fullsort_scores(ue, slab0, slab1)
    assert torch.equal(full, full.round()) and int((full[0] == full[0, 1]).sum()) > 50
    hindptr, hist = _history(full, N)
    want = _want(full, k, hindptr, hist)
    assert int((want[0][:, 1:] == want[0][:, :-1]).sum()) > U * k // 2                           # the lists are mostly ties
    _assert_lists(F_.fullsort_topk_wide(ue, slab0, slab1, k, hindptr, hist), want)
    _assert_lists(F_.topk_rows(full, k, hindptr, hist), want)


@pytest.mark.parametrize('k', [100, 1024])
@pytest.mark.parametrize('N', [1, 64, 65, 1025])
def test_short_rows_and_special_values(N, k):
    """fewer than k unmasked columns: the pads are exactly (-inf, -1); a user whose history leaves 3 columns; a NaN user row lists
    nothing; +inf is an ordinary score, -inf and NaN scores are never listed"""
    from recbole_cdr_amd import functional as F_
    U, D = 4, 64
    ue, tab = _operands(U, D, N, N + k)
    ue[2] = NAN
    if N >= 64:
        tab[7, 0], tab[11, 0], tab[13, 0], tab[17, 1] = INF, -INF, NAN, INF
    n0, slab0, slab1 = _slabs(tab, N < 64)
    full = F_.fullsort_scores(ue, slab0, slab1)
    keep = torch.tensor([c for c in (1, 7, N - 1) if c < N], device=DEV).unique()
    hist1 = torch.tensor([c for c in range(N) if c not in keep.tolist()], dtype=torch.int64, device=DEV)
    none = torch.empty(0, dtype=torch.int64, device=DEV)
    hindptr, hist = _csr([none, hist1, none, torch.tensor([0, N - 1], device=DEV).unique()], U)
    want = _want(full, k, hindptr, hist)
    got = F_.fullsort_topk_wide(ue, slab0, slab1, k, hindptr, hist)
    _assert_lists(got, want)
    assert bool((got[1][2] == -1).all()) and int((got[1][1] >= 0).sum()) <= 3
    if N >= 64:
        assert bool(torch.isnan(full[0, 13])) and bool(torch.isinf(full[0, 7])) and bool(torch.isinf(full[0, 11]))
        hi_col, lo_col = (7, 11) if float(full[0, 7]) > 0 else (11, 7)
        assert int(got[1][0, 0]) in (hi_col, 17) and float(got[0][0, 0]) == INF
        assert not bool(((got[1][0] == lo_col) | (got[1][0] == 13)).any())
    _assert_lists(F_.topk_rows(full, k, hindptr, hist), want)


@pytest.mark.parametrize('U,N', [(1, 1), (1, 63), (3, 64), (1, 65), (9, 20000)])
def test_topk_rows_strided_rows_and_column_passes(U, N):
    """``topk_rows`` on rows that are ld > N apart, in one call and as two column passes with ``col_off`` / ``accumulate`` in both orders"""
    from recbole_cdr_amd import functional as F_
    k = 100
    g = torch.Generator(device=DEV); g.manual_seed(U * N)
    wide = torch.randn(U, N + 5, device=DEV, generator=g)
    wide[:, N:] = 1e9                                                     # (past the rows: must never be listed)
    view = wide[:, :N]
    full = view.contiguous()
    hindptr, hist = _history(full, N)
    want = _want(full, k, hindptr, hist)
    _assert_lists(F_.topk_rows(full, k, hindptr, hist), want, 'contiguous')
    _assert_lists(F_.topk_rows(view, k, hindptr, hist), want, 'strided')
    assert torch.equal(view, full)                                        # only read
    if N > 1:
        h = N // 2
        blocks = [(view[:, :h], 0), (view[:, h:], h)]
        for order in (blocks, blocks[::-1]):
            out = F_.topk_rows(order[0][0], k, hindptr, hist, col_off=order[0][1])
            out = F_.topk_rows(order[1][0], k, hindptr, hist, col_off=order[1][1], out=out, accumulate=True)
            _assert_lists(out, want, 'two passes')


@pytest.mark.parametrize('U,D,N', [(70, 64, 70001), (600, 128, 40000)])
def test_agrees_with_the_fused_topk_up_to_64(U, D, N):
    from recbole_cdr_amd import functional as F_
    ue, tab = _operands(U, D, N, U + N)
    n0, slab0, slab1 = _slabs(tab, False)
    full = F_.fullsort_scores(ue, slab0, slab1)
    hindptr, hist = _history(full, U + N)
    top = _sorted_masked(full, hindptr, hist)[0][:, :65]
    assert bool((top[:, :-1] > top[:, 1:]).all()), 'a tie among the top 65: change the seed'
    for k in (10, 64):
        fv, fi = F_.fullsort_topk(ue, slab0, slab1, k, hindptr, hist)
        wv, wi = F_.fullsort_topk_wide(ue, slab0, slab1, k, hindptr, hist)
        assert torch.equal(fi, wi) and torch.equal(fv.view(torch.int32), wv.view(torch.int32)), k


def test_a_positive_at_rank_position_r_sits_at_entry_r_minus_1():
    """the tie rule is the rank route's: 1 + gt + eq_before, on data that is mostly ties"""
    from recbole_cdr_amd import functional as F_
    U, D, N, k = 9, 64, 20011, 300
    ue, tab = _tie_operands(U, D, N, 5)
    n0, slab0, slab1 = _slabs(tab, False)
    full = F_.fullsort_scores(ue, slab0, slab1)
    hindptr, hist = _history(full, 5)
    sv, si = _sorted_masked(full, hindptr, hist)
    g = torch.Generator(); g.manual_seed(6)
    cols = []
    for u in range(U):                       # 40 columns out of the user's first 400 in the order (many inside the list), 40 random ones
        pick = si[u, torch.randperm(400, generator=g)[:40].to(DEV)]
        cols.append(torch.unique(torch.cat([pick, torch.randint(0, N, (40,), generator=g).to(DEV)])))
    pindptr, pcols = _csr(cols, U)
    _score, gt, _eq, eqb, _nun = F_.fullsort_rank(ue, slab0, slab1, pindptr, pcols, hindptr, hist)
    _vals, idx = F_.fullsort_topk_wide(ue, slab0, slab1, k, hindptr, hist)
    r = 1 + gt.long() + eqb.long()
    inside = (gt >= 0) & (r <= k)
    assert int(inside.sum()) > 20 * U and int((eqb[inside] > 0).sum()) > U
    assert torch.equal(idx[_rows_of(pindptr)[inside], r[inside] - 1], pcols[inside])
    outside = (gt >= 0) & (r > k)
    assert not bool((idx[_rows_of(pindptr)[outside]] == pcols[outside].unsqueeze(1)).any())


# ---- models -----------------------------------------------------------------------------------------------------------------------------
def _model_case(name):
    """(model, interaction of 128 users, predict_fallback or None)"""
    from recbole_cdr_amd.data.interaction import Interaction
    from test_gpu_eval_metrics import _dataset, _emcdr, _ids, _trainer
    ids = _ids()
    torch.manual_seed(13)
    fallback = None
    src = False
    if name.startswith('EMCDR'):
        cfg, model, ids = _emcdr()
        model.set_phase(name.split('-')[1])
        src = model.phase == 'SOURCE'
    elif name == 'SSCDR':
        from recbole_cdr_amd.model.cross_domain_recommender.sscdr import SSCDR
        cfg = base_config(DEV, embedding_size=64, margin=0.3, mlp_hidden_size=[24], **{'lambda': 0.5})
        model = SSCDR(cfg, _dataset(ids)).to(DEV)
        model.set_phase('TARGET')
    elif name == 'CoNet':
        from recbole_cdr_amd.model.cross_domain_recommender.conet import CoNet
        cfg = base_config(DEV, embedding_size=32, reg_weight=0.01, mlp_hidden_size=[64, 32, 16, 8])
        model = CoNet(cfg, _dataset(ids)).to(DEV)
    else:
        from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
        native = name == 'DeepAPF-native'
        cfg = base_config(DEV, embedding_size=16, beta=0.5, eval_batch_size=1 << 16, **({'native_full_sort': True} if native else {}))
        model = DeepAPF(cfg, _dataset(ids)).to(DEV)
        model.set_phase('TARGET')
        assert hasattr(model, 'full_sort_topk') == native
        if not native:
            fallback = _trainer(cfg, model)._predict_all_pairs
    model.eval()
    users = torch.arange(1, 129, device=DEV)
    return model, Interaction({(model.SOURCE_USER_ID if src else model.TARGET_USER_ID): users}), fallback


@pytest.mark.parametrize('name', ['EMCDR-SOURCE', 'EMCDR-TARGET', 'EMCDR-OVERLAP', 'SSCDR', 'CoNet', 'DeepAPF-native', 'DeepAPF-predict'])
def test_models_list_100_items(name):
    """``full_sort_topk(interaction, 100, ...)`` -- ``full_sort_topk_wide(predict_fallback=...)`` for the model with ``predict`` only --
    equals the sorted masked ``full_sort_predict``; ``fullsort_topk_min_items`` plays no part above 64"""
    model, inter, fallback = _model_case(name)
    U, k = len(inter), 100
    with torch.no_grad():
        full = (fallback(inter, U) if fallback is not None else model.full_sort_predict(inter).view(U, -1)).float().clone()
    N = full.shape[1]
    assert N == (71 if name == 'EMCDR-SOURCE' else 1500)                                       # (SOURCE: two slabs, fewer than k columns)
    hindptr, hist = _history(full, 3)
    want = _want(full, k, hindptr, hist)
    if fallback is not None:
        got = model.full_sort_topk_wide(inter, k, hindptr, hist, predict_fallback=fallback)
        with pytest.raises(NotImplementedError):
            model.full_sort_topk_wide(inter, k, hindptr, hist)
    else:
        got = model.full_sort_topk(inter, k, hindptr, hist)
    _assert_lists(got, want, name)
    if fallback is None:
        for min_items in (0, 10 ** 9):
            model.__dict__['fullsort_topk_min_items'] = min_items
            _assert_lists(model.full_sort_topk(inter, k, hindptr, hist), want, (name, min_items))
        _assert_lists(model.full_sort_topk_wide(inter, k, hindptr, hist), want, name)


def test_default_route_chunks_the_users():
    """the base-class default takes the users in chunks of at most ``RANK_ROWS_MAX_SCORES`` scores: same lists"""
    model, inter, _ = _model_case('CoNet')
    full = model.full_sort_predict(inter).view(len(inter), -1).float().clone()
    hindptr, hist = _history(full, 4)
    model.RANK_ROWS_MAX_SCORES = 50 * full.shape[1]                                            # 128 users: chunks of 50, 50, 28
    _assert_lists(model.full_sort_topk_wide(inter, 100, hindptr, hist), _want(full, 100, hindptr, hist))


def test_trainer_topk_route_returns_the_rank_route_s_metrics():
    """``eval_route='topk'`` with topk = [10, 100, 500] against ``eval_route='rank'``: the hit matrices are identical by the tie rule; the
    bound is the one tests/test_eval_metrics_host.py holds this route pair to"""
    from test_gpu_eval_metrics import _batches, _emcdr, _trainer
    cfg, model, ids = _emcdr(topk=[10, 100, 500], metrics=['Recall', 'NDCG', 'MAP'])
    batches = _batches(model, ids)
    a = _trainer(dict(cfg, eval_route='topk'), model).evaluate(batches)
    b = _trainer(dict(cfg, eval_route='rank'), model).evaluate(batches)
    assert set(a) == set(b) == {f'{m}@{k}' for m in ('recall', 'ndcg', 'map') for k in (10, 100, 500)}
    for key in a:
        print(key, a[key], b[key])
        assert abs(a[key] - b[key]) <= 1e-7, (key, a[key], b[key])
    assert a['recall@500'] > a['recall@10'] > 0
    with pytest.raises(ValueError, match='1024'):
        _trainer(dict(cfg, eval_route='topk', topk=[10, 1025]), model).evaluate(batches)


def test_refusals():
    from recbole_cdr_amd import functional as F_
    from test_gpu_eval_metrics import _emcdr
    ue, tab = _operands(40, 64, 3000, 1)
    full = F_.fullsort_scores(ue, tab)
    hindptr, hist = _history(full, 1)
    for k in (0, 1025):
        with pytest.raises(RuntimeError, match='cdr_fullsort_topk_wide'):
            F_.fullsort_topk_wide(ue, tab, None, k)
        with pytest.raises(RuntimeError, match='cdr_fullsort_neg_sqdist_topk_wide'):
            F_.fullsort_neg_sqdist_topk_wide(ue, tab, None, k)
        with pytest.raises(RuntimeError, match='cdr_topk_rows'):
            F_.topk_rows(full, k)
    for pair in ((hindptr, None), (None, hist)):
        with pytest.raises(ValueError, match='hist'):
            F_.fullsort_topk_wide(ue, tab, None, 100, *pair)
        with pytest.raises(ValueError, match='hist'):
            F_.topk_rows(full, 100, *pair)
    model = _emcdr()[1]
    model.__dict__['_dist_cfg'] = True
    with pytest.raises(NotImplementedError, match='one GPU'):
        model.full_sort_topk_wide(None, 100)
    assert F_.WIDE_TOPK_MAX == 1024
