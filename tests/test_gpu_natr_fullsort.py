"""NATR's one-launch full sort (csrc/cdr_natr_fullsort.hip behind functional.natr_history_summary; reference natr.py:112-156) on the
device: the scores and the key-side summary against a float64 restatement with derived bounds (natr_fullsort_fp64), the fused mask + top-k
epilogue against torch.topk of the masked scores, the reference's golden vectors, the opt-in model methods and ``Trainer.evaluate`` on every
route, and the entries' refusals.

Worst error / bound on an MI355X, per case (Dt, Ds, L, U, N, k), overlap_items / overlap_users (the tests print them):
scores (test 1): (8, 16, 3, 5, 77, 5) 0.073 / 0.080; (12, 8, 5, 7, 100, 1) 0.068 / 0.058; (16, 8, 6, 33, 2049, 64) 0.096 / 0.100;
(64, 64, 50, 70, 4001, 10) 0.058 / 0.037; (128, 32, 9, 40, 4000, 50) 0.017 / 0.021; (64, 16, 4, 3, 300001, 10) 0.047 / 0.045.
summary (test 2): 0.031 / 0.026; 0.048 / 0.045; 0.088 / 0.133; 0.011 / 0.014; 0.014 / 0.028; 0.011 / 0.042.
Users left out of an index comparison (a tie among their top k + 1): 0 % in every case, with and without a history.
Model test, 60 users x 501 items: full_sort_predict 0.041 / 0.034, predict 0.027 / 0.027; no user's top-10 list differs between routes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from golden_util import Golden, cases
from helpers import DEV, FakeDataset, assert_close, base_config, load_params, to_dev
from natr_fullsort_fp64 import fullsort_depths, make_case, natr_pair_fp64, natr_summary_fp64

pytestmark = pytest.mark.gpu

NEG = -float('inf')

CASES = [(8, 16, 3, 5, 77, 5),               # tail tile
         (12, 8, 5, 7, 100, 1),              # the fixtures' widths; a width that is no multiple of 8; k = 1
         (16, 8, 6, 33, 2049, 64),           # k = 64; several user chunks
         (64, 64, 50, 70, 4001, 10),         # the defaults; the summary chunked
         (128, 32, 9, 40, 4000, 50),         # the widest instantiation
         (64, 16, 4, 3, 300001, 10)]         # more than one round of tiles per workgroup; the seeded thresholds
TOPK_ONLY = [(64, 8, 2, 33, 1, 10),          # every column masked, all padding
             (64, 16, 4, 160, 81921, 10)]    # the seeded path with three user groups, just over its threshold of 81,920 items; a partial last tile
MODES = [False, True]                        # key_is_item: overlap_items, overlap_users


def _summary_args(c):
    return (c['src'], c['hist'], c['mask_mat'], c['key_tab'], c['keys'], c['Wt'], c['bt'], c['wu'], c['bu'], c['wd'], c['bd'])


@functools.lru_cache(maxsize=None)
def _case(Dt, Ds, L, U, N, key_is_item):
    """The inputs, the device's key-side summary and the kernel's [U, N] scores of a case: computed once, shared by the tests, never
    modified."""
    from recbole_cdr_amd import functional as F_
    c = make_case(Dt, Ds, L, U, N, key_is_item, device=DEV)
    su = F_.natr_history_summary(*_summary_args(c))
    full = F_.natr_fullsort(key_is_item, su, c['key_tab'], c['other_tab'], c['uid'], N, c['wd'])
    torch.cuda.synchronize()
    return c, su, full


def _pair_args(c, su):
    return (c['key_is_item'], su, c['key_tab'], c['other_tab'], c['uid'], c['N'], c['wd'])


@pytest.mark.parametrize('key_is_item', MODES)
@pytest.mark.parametrize('Dt,Ds,L,U,N,k', CASES)
def test_natr_fullsort_scores_within_fp64_bounds(Dt, Ds, L, U, N, k, key_is_item):
    """Every element of ``natr_fullsort`` lies within its derived bound of the float64 restatement of the pair stage on the same fp32
    summary (the kernel's real accumulation depths); a rerun is bit-equal."""
    from recbole_cdr_amd import functional as F_
    c, su, full = _case(Dt, Ds, L, U, N, key_is_item)
    assert tuple(full.shape) == (U, N) and bool(torch.isfinite(full).all())
    ref = natr_pair_fp64(*_pair_args(c, su), depths=fullsort_depths(Dt))
    r = ref.ratio(full)
    worst = float(r.max())
    print(f'case Dt={Dt} Ds={Ds} L={L} U={U} N={N} key_is_item={key_is_item}: worst error / bound {worst:.3f}, '
          f'scores {float(full.min()):.4f}..{float(full.max()):.4f}')
    assert worst <= 1.0, (worst, int(r.argmax()) // N, int(r.argmax()) % N)
    again = F_.natr_fullsort(*_pair_args(c, su))
    assert torch.equal(again, full)


@pytest.mark.parametrize('key_is_item', MODES)
@pytest.mark.parametrize('Dt,Ds,L,U,N,k', CASES)
def test_natr_history_summary_chunked_is_bit_equal_and_within_bounds(Dt, Ds, L, U, N, k, key_is_item):
    """``natr_history_summary`` at ``chunk_rows = 7`` is bit-equal to one chunk, and lies within the summary stage's bounds; the planted
    keys (length 0, 1 and beyond L) are among the rows."""
    from recbole_cdr_amd import functional as F_
    c, su, _full = _case(Dt, Ds, L, U, N, key_is_item)
    keys = c['keys']
    if keys.numel() > 4096:                                                 # the 300,001 item keys: every 80th and the planted ones
        keys = torch.cat([keys[:3], keys[3::80]])
    args = list(_summary_args(c))
    args[4] = keys
    one = F_.natr_history_summary(*args, chunk_rows=keys.numel())
    seven = F_.natr_history_summary(*args, chunk_rows=7)
    assert tuple(one.shape) == (keys.numel(), Dt)
    assert torch.equal(one, seven)
    pos = keys if key_is_item else torch.arange(keys.numel(), device=DEV)
    assert torch.equal(one, su[pos])
    lens = c['lens'][keys]
    want_lens = [0] if keys.numel() < 3 else [0, 1, L + 2]
    assert [int(x) for x in lens[:len(want_lens)]] == want_lens
    ref = natr_summary_fp64(c['src'], c['hist'], c['mask_mat'], c['key_tab'], keys, c['Wt'], c['bt'], c['wu'], c['bu'])
    worst = float(ref.ratio(one).max())
    print(f'summary Dt={Dt} Ds={Ds} L={L} keys={keys.numel()} key_is_item={key_is_item}: worst error / bound {worst:.3f}')
    assert worst <= 1.0


def _padded_topk(masked, k):
    U, N = masked.shape
    kk = min(k, N)
    v, i = torch.topk(masked, kk, dim=1)
    if kk < k:
        v = torch.cat([v, v.new_full((U, k - kk), NEG)], 1)
        i = torch.cat([i, i.new_full((U, k - kk), -1)], 1)
    return v, torch.where(v == NEG, torch.full_like(i, -1), i)


def _untied_users(masked, k):
    """Users with no tie among their top k + 1 stored values (padding aside)."""
    top = torch.topk(masked, min(k + 1, masked.shape[1]), dim=1).values
    if top.shape[1] < 2:
        return torch.ones(masked.shape[0], dtype=torch.bool, device=masked.device)
    return ~((top[:, 1:] == top[:, :-1]) & (top[:, 1:] > NEG)).any(1)


def _check(masked, k, got_v, got_i, what=''):
    want_v, want_i = _padded_topk(masked, k)
    assert tuple(got_v.shape) == tuple(got_i.shape) == (masked.shape[0], k) and got_i.dtype == torch.int64
    assert torch.equal(got_v, want_v), (got_v - want_v).abs().nan_to_num(posinf=9.0).max()          # EVERY user, bit-equal
    real = got_v > NEG
    assert bool((got_i[~real] == -1).all()) and bool((got_i[real] >= 0).all())
    # the column of every entry holds that entry's value and is not masked; no duplicates among a user's columns
    picked = torch.gather(masked, 1, got_i.clamp(min=0))
    assert torch.equal(picked[real], want_v[real])
    s = torch.sort(torch.where(real, got_i, -1 - torch.arange(k, device=got_i.device).expand_as(got_i)), dim=1).values
    assert bool((s[:, 1:] != s[:, :-1]).all())
    # indices: every user with no tie among their top k + 1 values; at most 5 % of the users may be left out
    ok = _untied_users(masked, k)
    left_out = 1.0 - float(ok.float().mean())
    print(f'{what}: users left out of the index comparison (a tie among their top k+1): {100 * left_out:.1f} %')
    assert left_out <= 0.05
    assert torch.equal(got_i[ok], want_i[ok])


@pytest.mark.parametrize('key_is_item', MODES)
@pytest.mark.parametrize('Dt,Ds,L,U,N,k', CASES + TOPK_ONLY)
def test_natr_fullsort_topk_matches_topk_of_masked_scores(Dt, Ds, L, U, N, k, key_is_item):
    """Fused mask + top-k == torch.topk over the evaluation-masked output of ``natr_fullsort`` on the same operands: one scoring body, two
    epilogues, so the values are bit-equal for every user; indices are compared for every user without a tie among their top k + 1.  The
    history holds each user's 7 best columns and 30 random ones, so the mask decides the result; a second call runs without history and
    keeps the PAD column.  The last case is a one-item catalogue: the padding contract."""
    from recbole_cdr_amd import functional as F_
    c, su, full = _case(Dt, Ds, L, U, N, key_is_item)
    g = torch.Generator().manual_seed(U + N)
    best = torch.topk(full, min(7, N), dim=1).indices
    rnd = torch.randint(0, N, (U, 30), generator=g).to(DEV)
    cols = [torch.unique(torch.cat([best[u], rnd[u]])) for u in range(U)]           # ascending, deduplicated
    indptr = torch.zeros(U + 1, dtype=torch.int64, device=DEV)
    indptr[1:] = torch.cumsum(torch.tensor([x.numel() for x in cols], device=DEV), 0)
    hist = torch.cat(cols)
    masked = full.clone()
    masked[:, 0] = NEG
    for u in range(U):
        masked[u, cols[u]] = NEG
    tag = f'case Dt={Dt} U={U} N={N} k={k} key_is_item={key_is_item}'
    got_v, got_i = F_.natr_fullsort_topk(*_pair_args(c, su), k, hist_indptr=indptr, hist_cols=hist)
    _check(masked, k, got_v, got_i, tag + ' with history')
    got_v2, got_i2 = F_.natr_fullsort_topk(*_pair_args(c, su), k, exclude_first_col=False)
    _check(full, k, got_v2, got_i2, tag + ' without history')
    if N == 1:
        # PAD kept: one real entry, then padding; PAD masked: padding only
        assert bool((got_i2[:, 0] == 0).all()) and bool((got_i2[:, 1:] == -1).all()) and bool((got_v2[:, 1:] == NEG).all())
        v3, i3 = F_.natr_fullsort_topk(*_pair_args(c, su), k)
        assert bool((v3 == NEG).all()) and bool((i3 == -1).all())


# ---- model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cases('natr_'))
def test_natr_full_sort_predict_golden(name):
    """A flag-on model with the reference's golden parameters: the columns of ``full_sort_predict`` at the fixture's evaluation items equal
    the reference's ``predict`` output of phase 'TARGET' within the project's golden tolerance (test_gpu_models5.py's for ``predict``)."""
    from recbole_cdr_amd.data.interaction import Interaction
    from recbole_cdr_amd.model.cross_domain_recommender.natr import NATR
    g = Golden(name)
    ds = FakeDataset(g.idspace(), g['aux/s_pairs'], g['aux/t_pairs'])
    ds.device = DEV
    cfg = base_config(DEV, source_embedding_size=int(g.meta('Ds')), target_embedding_size=int(g.meta('Dt')),
                      reg_weight=float(g.meta('reg_weight')), max_inter_length=int(g.meta('max_inter_length')), native_full_sort=True)
    model = NATR(cfg, ds).to(DEV)
    load_params(model, g.group('param'))
    model.set_phase('TARGET')
    model.eval()
    ev = to_dev(g.group('evalin'), DEV)
    users, items = ev['target_user_id'], ev['target_item_id']
    N = model.target_num_items
    scores = model.full_sort_predict(Interaction({'target_user_id': users})).view(users.numel(), N)
    got = scores[torch.arange(users.numel(), device=DEV), items]
    assert_close(got, g['predict/TARGET'], what=f'{name}: full_sort_predict at the evaluation pairs')


EVAL_SEED = {'overlap_users': 21, 'overlap_items': 21}


def _eval_ids(mode):
    from oracle.common import IdSpace
    if mode == 'overlap_items':
        return IdSpace(OU=1, TOU=70, SOU=22, OI=18, TOI=483, SOI=16)            # test_gpu_eval_fallback.py's: 60 users x 501 items
    return IdSpace(OU=40, TOU=30, SOU=35, OI=1, TOI=500, SOI=70)                # the same sizes with the users overlapped


def _eval_model(mode, flag, device=DEV, **kw):
    """NATR of test_gpu_eval_fallback.py's set-up (Ds = 16, Dt = 24, L = 6), built from a fixed seed."""
    from recbole_cdr_amd.model.cross_domain_recommender.natr import NATR
    ids = _eval_ids(mode)
    torch.manual_seed(EVAL_SEED[mode])
    rng = np.random.RandomState(4)
    tu, ti = np.arange(1, ids.target_num_users), np.arange(1, ids.target_num_items)
    su = np.arange(ids.OU + ids.TOU, ids.total_num_users)
    si = np.concatenate([np.arange(1, ids.OI), np.arange(ids.OI + ids.TOI, ids.total_num_items)])
    s_pairs = np.unique(np.stack([rng.choice(su, 300), rng.choice(si, 300)], 1), axis=0)
    t_pairs = np.unique(np.stack([rng.choice(tu, 900), rng.choice(ti, 900)], 1), axis=0)
    ds = FakeDataset(ids, s_pairs, t_pairs)
    ds.device = device
    extra = {'native_full_sort': True} if flag else {}
    cfg = base_config(device, source_embedding_size=16, target_embedding_size=kw.get('Dt', 24), reg_weight=1e-3, max_inter_length=6,
                      topk=[5, 10], **extra)
    model = NATR(cfg, ds)
    assert model.mode == mode
    with torch.no_grad():                                                    # rows large enough for scores that differ beyond rounding
        for n, p in model.named_parameters():
            if n.endswith('_embedding.weight'):
                p.copy_(torch.randn(p.shape) * 0.4)
    model = model.to(device)
    model.set_phase('TARGET')
    model.eval()
    return ids, cfg, model


def _eval_sets(N, n_users=60):
    rng = np.random.RandomState(2)
    users = np.arange(1, n_users + 1)
    ev = np.unique(np.stack([np.repeat(users, 4), rng.randint(1, N, 4 * n_users)], 1), axis=0)
    hi = np.unique(np.stack([np.repeat(users, 12), rng.randint(1, N, 12 * n_users)], 1), axis=0)
    return users, ev, hi


def _model_reference(model, ut, N):
    """Both stages' reference on the model's operands: the pair stage on the float64 summary WITH its bound (``predict`` and the full sort
    each compute their own fp32 summary), and with the bound that also holds ``predict``'s operation order."""
    ki = model.mode == 'overlap_users'
    hist, src = (model.history_user_matrix, model.source_user_embedding.weight) if ki else \
        (model.history_item_matrix, model.source_item_embedding.weight)
    key_tab, other_tab = (model.target_item_embedding.weight, model.target_user_embedding.weight) if ki else \
        (model.target_user_embedding.weight, model.target_item_embedding.weight)
    keys = torch.arange(N, device=ut.device) if ki else ut
    su = natr_summary_fp64(src.detach(), hist, model.mask_mat, key_tab.detach(), keys, model.transfer_layer.weight.detach(),
                           model.transfer_layer.bias.detach(), model.unit_attention_layer.weight.detach(),
                           model.unit_attention_layer.bias.detach())
    return natr_pair_fp64(ki, su, key_tab.detach(), other_tab.detach(), ut, N, model.domain_attention_layer.weight.detach(),
                          depths=fullsort_depths(key_tab.shape[1]), cover_predict=True, bd=model.domain_attention_layer.bias.detach())


@pytest.mark.parametrize('mode', ['overlap_items', 'overlap_users'])
def test_natr_native_full_sort_model_and_trainer(mode, monkeypatch):
    """Flag on, 60 users x 501 items: ``full_sort_predict`` and ``predict`` over all pairs both lie inside one reference's bounds;
    ``Trainer.evaluate`` gives the same metrics on the fused route (forced with ``fullsort_topk_min_items = 0``), on scores + torch.topk
    and from a flag-off model with the same parameters -- a user whose top-k list the two roundings (``predict``'s form, the kernel's)
    order differently may differ between routes: those users are counted (at most 5 %) and each may move a mean metric by 1 / 60.  The item keys' summary
    (overlap_users) is built once per ``evaluate``, the user keys' once per batch; a parameter changed after ``unfreeze_eval()`` is seen."""
    from recbole_cdr_amd import functional as F_
    from recbole_cdr_amd.data.dataloader import FullSortEvalLoader
    from recbole_cdr_amd.data.interaction import Interaction
    from recbole_cdr_amd.trainer.trainer import Trainer
    ids, cfg, model = _eval_model(mode, True)
    _ids2, cfg_off, off = _eval_model(mode, False)
    off.load_state_dict(model.state_dict())
    assert not hasattr(off, 'full_sort_topk')
    with pytest.raises(NotImplementedError):
        off.full_sort_predict(Interaction({'target_user_id': torch.ones(1, dtype=torch.int64, device=DEV)}))
    N, k = ids.target_num_items, 10
    assert N == 501
    users, ev, hi = _eval_sets(N)
    ut = torch.as_tensor(users, device=DEV)
    pairs = Interaction({'target_user_id': ut.repeat_interleave(N), 'target_item_id': torch.arange(N, device=DEV).repeat(ut.numel())})
    want = model.predict(pairs).view(60, N).float()
    assert torch.equal(off.predict(pairs).view(60, N).float(), want)
    got = model.full_sort_predict(Interaction({'target_user_id': ut})).view(60, N)
    ref = _model_reference(model, ut, N)
    r_fs, r_pr = float(ref.ratio(got).max()), float(ref.ratio(want).max())
    print(f'{mode}: worst error / bound: full_sort_predict {r_fs:.3f}, predict {r_pr:.3f}; largest |difference| {float((got - want).abs().max()):.3e}')
    assert r_fs <= 1.0 and r_pr <= 1.0
    # users whose list the two roundings (``predict``'s form, the kernel's form) order differently: near-ties between the routes
    rows, colsn = torch.from_numpy(hi[:, 0] - 1).to(DEV), torch.from_numpy(hi[:, 1]).to(DEV)
    masked = want.clone()
    masked[:, 0] = NEG
    masked[rows, colsn] = NEG
    m_fs = got.clone()
    m_fs[:, 0] = NEG
    m_fs[rows, colsn] = NEG
    reordered = int((torch.topk(masked, k, dim=1).indices != torch.topk(m_fs, k, dim=1).indices).any(1).sum())
    print(f'{mode}: users whose top-{k} list differs between predict and full_sort_predict: {reordered} of 60')
    assert reordered <= 3                                                      # 5 % of the users
    slack = 1e-6 + reordered / 60.0
    order = torch.argsort(rows * N + colsn)
    indptr = torch.zeros(61, dtype=torch.int64, device=DEV)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=60), 0)
    model.fullsort_topk_min_items = 0
    v, i = model.full_sort_topk(Interaction({'target_user_id': ut}), k, hist_indptr=indptr, hist_cols=colsn[order].contiguous())
    _check(m_fs, k, v, i, f'{mode} model')
    # the trainer, three ways; the summary calls are counted
    calls = []
    real = F_.natr_history_summary
    monkeypatch.setattr(F_, 'natr_history_summary', lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])

    def evaluate(m, c, **kw):
        loader = FullSortEvalLoader('target_user_id', ev, hi, N, 4096, DEV, users_per_batch=25)
        del calls[:]
        return Trainer(dict(c, graph_step=False, **kw), m).evaluate(loader), len(calls)

    per_batch = 1 if mode == 'overlap_users' else 3                            # three batches of 25, 25 and 10 users
    res = [evaluate(model, cfg, eval_users_per_batch=0), evaluate(model, cfg, fused_topk=False), evaluate(off, cfg_off)]
    assert [n for _r, n in res] == [per_batch, per_batch, 0]
    assert '_eval_su' not in model.__dict__ and '_eval_frozen' not in model.__dict__
    res = [r for r, _n in res]
    assert len(res[0]) == 10
    for other in res[1:]:
        assert set(other) == set(res[0])
        for key in res[0]:
            assert np.isfinite(res[0][key]) and abs(res[0][key] - other[key]) <= slack, (key, res[0][key], other[key])
    # outside a bracket every call recomputes from the live parameters
    with torch.no_grad():
        model.transfer_layer.weight.mul_(1.5)
    got2 = model.full_sort_predict(Interaction({'target_user_id': ut})).view(60, N)
    assert not torch.equal(got2, got)
    ref2 = _model_reference(model, ut, N)
    assert float(ref2.ratio(got2).max()) <= 1.0


def test_natr_native_full_sort_outside_the_kernels_widths():
    """target_embedding_size = 6 (no multiple of 4): the opted-in methods still work, on chunked ``phase2_forward`` inside
    ``full_sort_predict``."""
    from recbole_cdr_amd.data.interaction import Interaction
    ids, _cfg, model = _eval_model('overlap_items', True, Dt=6)
    N = ids.target_num_items
    ut = torch.arange(1, 8, device=DEV)
    pairs = Interaction({'target_user_id': ut.repeat_interleave(N), 'target_item_id': torch.arange(N, device=DEV).repeat(ut.numel())})
    got = model.full_sort_predict(Interaction({'target_user_id': ut})).view(7, N)
    assert torch.equal(got, model.predict(pairs).view(7, N).float())
    model.fullsort_topk_min_items = 0
    v, i = model.full_sort_topk(Interaction({'target_user_id': ut}), 5)
    m = got.clone()
    m[:, 0] = NEG
    _check(m, 5, v, i, 'Dt = 6')


def test_natr_fullsort_refuses_bad_arguments_before_any_launch():
    """k = 0 / 65, Dt = 6 / 132 and a workspace one byte short come back non-zero with an error text; the outputs of a refused call are
    untouched (nothing was launched)."""
    from recbole_cdr_amd import binding as B_
    from recbole_cdr_amd import functional as F_
    c, su, _full = _case(8, 16, 3, 5, 77, False)
    for k in (0, 65):
        with pytest.raises(RuntimeError, match='cdr_natr_fullsort_topk'):
            F_.natr_fullsort_topk(*_pair_args(c, su), k)
    lib = B_.load()
    need = ctypes.c_size_t(0)
    assert lib.cdr_natr_fullsort_topk_workspace_bytes(5, 77, 10, ctypes.byref(need)) == 0 and need.value > 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    vals = torch.full((5, 10), 7.0, device=DEV)
    idx = torch.full((5, 10), 7, dtype=torch.int64, device=DEV)
    out = torch.full((5, 77), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    wide = torch.zeros(200, 132, device=DEV)
    wd = c['wd'].reshape(-1).contiguous()

    def head(Dt, tab=None):
        s, kt, ot = (su, c['key_tab'], c['other_tab']) if tab is None else (tab, tab, tab)
        return (B_.stream(), 0, p(s), Dt, p(kt), Dt, p(ot), Dt, p(c['uid']), 5, 77, Dt, p(wd))

    def topk(Dt, k, nbytes, tab=None):
        return lib.cdr_natr_fullsort_topk(*head(Dt, tab), k, None, None, 1, p(vals), p(idx), p(ws), nbytes)

    for k in (0, 65):
        assert topk(8, k, need.value) != 0 and b'k = ' in lib.cdr_last_error()
    for Dt in (6, 132):
        assert topk(Dt, 10, need.value, wide) != 0 and b'outside the kernel' in lib.cdr_last_error()
        assert lib.cdr_natr_fullsort(*head(Dt, wide), p(out), 77) != 0 and b'outside the kernel' in lib.cdr_last_error()
    assert topk(8, 10, need.value - 1) != 0 and b'workspace' in lib.cdr_last_error()
    torch.cuda.synchronize()
    assert bool((vals == 7.0).all()) and bool((idx == 7).all()) and bool((out == 7.0).all())
    assert topk(8, 10, need.value) == 0
    torch.cuda.synchronize()
    assert bool((vals < 1.0).all()) and bool((idx >= 1).all())
