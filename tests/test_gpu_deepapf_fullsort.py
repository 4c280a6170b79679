"""DeepAPF's one-launch full sort (csrc/cdr_deepapf_fullsort.hip; reference deepapf.py:111-161) on the device: the scores against a float64
restatement with derived bounds (deepapf_fullsort_fp64), the fused mask + top-k epilogue against torch.topk of the masked scores, the
reference's golden vectors, the opt-in model methods and ``Trainer.evaluate`` on every route, and the entries' refusals.

Worst error / bound of test 1 on an MI355X, per case (D, U, N, k, n_overlap), overlap_users / overlap_items (the test prints them):
(8, 5, 77, 5, 3) 0.433 / 0.375; (16, 33, 2049, 64, 20) 0.356 / 0.393; (64, 70, 20011, 10, 40) 0.143 / 0.130; (128, 40, 4000, 50, 25)
0.053 / 0.061; (12, 7, 100, 1, 4) 0.378 / 0.309; (64, 3, 300001, 10, 2) 0.143 / 0.140; (64, 40, 9001, 20, 9001) 0.067 / 0.059.  Users with
a tie among their top k + 1: 0 % in every case but (128, 40, 4000, 50, 25) overlap_items, 2.5 % (1 of 40)."""
import copy
import ctypes
import functools
import pickle

import numpy as np
import pytest
import torch

from deepapf_fullsort_fp64 import deepapf_fullsort_fp64, fullsort_depths, make_case
from golden_util import Golden, cases
from helpers import DEV, FakeDataset, assert_close, base_config, load_params, to_dev

pytestmark = pytest.mark.gpu

NEG = -float('inf')

CASES = [(8, 5, 77, 5, 3),                   # tail tile, one pass of 32 features a quarter full
         (16, 33, 2049, 64, 20),             # k = 64, several user chunks
         (64, 70, 20011, 10, 40),            # the default width, nine user chunks
         (128, 40, 4000, 50, 25),            # the widest instantiation (four passes), a large k
         (12, 7, 100, 1, 4),                 # a width that is no multiple of 8, k = 1
         (64, 3, 300001, 10, 2),             # more than one round of tiles per workgroup; the seeded thresholds
         (64, 40, 9001, 20, 9001)]           # nobody masked
TOPK_ONLY = [(64, 33, 1, 10, 0),             # a one-item catalogue: padding
             (64, 160, 81921, 10, 40000)]    # the seeded path with three user groups, just over its threshold of 81,920 items; a partial last tile
MODES = [False, True]                        # key_is_item: overlap_users, overlap_items


def _call_args(c):
    return (c['key_is_item'], c['share'], c['only'], c['other'], c['uid'], c['N'], c['n_overlap'], c['W1'], c['b1'], c['w2'], c['wp'])


@functools.lru_cache(maxsize=None)
def _case(D, U, N, n_overlap, key_is_item):
    """The inputs and the kernel's [U, N] scores of a case: computed once, shared by the tests, never modified."""
    from recbole_cdr_amd import functional as F_
    c = make_case(D, U, N, n_overlap, key_is_item, device=DEV)
    full = F_.deepapf_fullsort(*_call_args(c))
    torch.cuda.synchronize()
    return c, full


@pytest.mark.parametrize('key_is_item', MODES)
@pytest.mark.parametrize('D,U,N,k,n_overlap', CASES)
def test_deepapf_fullsort_scores_within_fp64_bounds(D, U, N, k, n_overlap, key_is_item):
    """Every element of ``deepapf_fullsort`` lies within its derived bound of the float64 restatement (the kernel's real accumulation
    depths; a ReLU unit within its bound of 0 counts as either branch); both sides of the strict mask occur; a rerun is bit-equal."""
    from recbole_cdr_amd import functional as F_
    c, full = _case(D, U, N, n_overlap, key_is_item)
    assert tuple(full.shape) == (U, N) and bool(torch.isfinite(full).all())
    keys = torch.arange(N, device=DEV) if key_is_item else c['uid']
    if n_overlap < N:
        assert bool((keys == n_overlap).any()) and bool((keys == n_overlap + 1).any())
    else:
        assert not bool((keys > n_overlap).any())
    ref, amb = deepapf_fullsort_fp64(*_call_args(c), depths=fullsort_depths(D))
    r = ref.ratio(full)
    worst = float(r.max())
    print(f'case D={D} U={U} N={N} n_overlap={n_overlap} key_is_item={key_is_item}: worst error / bound {worst:.3f}, '
          f'{amb} ambiguous ReLU units, scores {float(full.min()):.3f}..{float(full.max()):.3f}')
    assert worst <= 1.0, (worst, int(r.argmax()) // N, int(r.argmax()) % N)
    again = F_.deepapf_fullsort(*_call_args(c))
    assert torch.equal(again, full)


def _padded_topk(masked, k):
    U, N = masked.shape
    kk = min(k, N)
    v, i = torch.topk(masked, kk, dim=1)
    if kk < k:
        v = torch.cat([v, v.new_full((U, k - kk), NEG)], 1)
        i = torch.cat([i, i.new_full((U, k - kk), -1)], 1)
    return v, torch.where(v == NEG, torch.full_like(i, -1), i)


def _check(masked, k, got_v, got_i):
    want_v, _ = _padded_topk(masked, k)
    assert tuple(got_v.shape) == tuple(got_i.shape) == (masked.shape[0], k) and got_i.dtype == torch.int64
    assert torch.equal(got_v, want_v), (got_v - want_v).abs().nan_to_num(posinf=9.0).max()
    real = got_v > NEG
    assert bool((got_i[~real] == -1).all()) and bool((got_i[real] >= 0).all())
    # the column of every entry holds that entry's value (columns may differ from torch's only between exactly tied scores) and is not masked
    picked = torch.gather(masked, 1, got_i.clamp(min=0))
    assert torch.equal(picked[real], want_v[real])
    # no duplicates among a user's columns
    s = torch.sort(torch.where(real, got_i, -1 - torch.arange(k, device=got_i.device).expand_as(got_i)), dim=1).values
    assert bool((s[:, 1:] != s[:, :-1]).all())


@pytest.mark.parametrize('key_is_item', MODES)
@pytest.mark.parametrize('D,U,N,k,n_overlap', CASES + TOPK_ONLY)
def test_deepapf_fullsort_topk_matches_topk_of_masked_scores(D, U, N, k, n_overlap, key_is_item):
    """Fused mask + top-k == torch.topk over the evaluation-masked output of ``deepapf_fullsort`` on the same operands: one scoring body,
    two epilogues, so the values are bit-equal; columns may differ only between exactly tied scores.  The history holds each user's 7 best
    columns and 30 random ones, so the mask decides the result; a second call runs without history and keeps the PAD column.  The last
    two cases: a one-item catalogue (the padding contract), and seeded thresholds with several user groups."""
    from recbole_cdr_amd import functional as F_
    c, full = _case(D, U, N, n_overlap, key_is_item)
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
    # a condition, not a tolerance: the tie rule must have almost nothing to decide
    top = torch.topk(masked, min(k + 1, N), dim=1).values
    tied = ((top[:, 1:] == top[:, :-1]) & (top[:, 1:] > NEG)).any(1).float().mean().item() if top.shape[1] > 1 else 0.0
    print(f'case D={D} U={U} N={N} k={k} key_is_item={key_is_item}: users with a tie among their top k+1: {100 * tied:.1f} %')
    assert tied <= 0.05
    got_v, got_i = F_.deepapf_fullsort_topk(*_call_args(c), k, hist_indptr=indptr, hist_cols=hist)
    _check(masked, k, got_v, got_i)
    got_v2, got_i2 = F_.deepapf_fullsort_topk(*_call_args(c), k, exclude_first_col=False)
    _check(full, k, got_v2, got_i2)
    if N == 1:
        # PAD kept: one real entry, then padding; PAD masked: padding only
        assert bool((got_i2[:, 0] == 0).all()) and bool((got_i2[:, 1:] == -1).all()) and bool((got_v2[:, 1:] == NEG).all())
        v3, i3 = F_.deepapf_fullsort_topk(*_call_args(c), k)
        assert bool((v3 == NEG).all()) and bool((i3 == -1).all())


# ---- model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cases('deepapf_'))
def test_deepapf_full_sort_predict_golden(name):
    """A flag-on model with the reference's golden parameters: the columns of ``full_sort_predict`` at the fixture's evaluation items equal
    the reference's ``predict`` output within the project's golden tolerance (1e-5 relative) -- both overlap modes at D = 8."""
    from recbole_cdr_amd.data.interaction import Interaction
    from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
    g = Golden(name)
    ds = FakeDataset(g.idspace())
    ds.device = DEV
    model = DeepAPF(base_config(DEV, embedding_size=int(g.meta('D')), beta=0.5, native_full_sort=True), ds).to(DEV)
    load_params(model, g.group('param'))
    model.eval()
    ev = to_dev(g.group('evalin'), DEV)
    users, items = ev['target_user_id'], ev['target_item_id']
    N = model.target_num_items
    scores = model.full_sort_predict(Interaction({'target_user_id': users})).view(users.numel(), N)
    got = scores[torch.arange(users.numel(), device=DEV), items]
    assert_close(got, g['predict/BOTH'], what=f'{name}: full_sort_predict at the evaluation pairs')


EVAL_SEED = {'overlap_users': 22, 'overlap_items': 24}          # seeds at which every top-(k + 1) gap exceeds twice the bound


def _eval_ids(mode):
    from oracle.common import IdSpace
    if mode == 'overlap_users':
        return IdSpace(OU=40, TOU=30, SOU=35, OI=1, TOI=500, SOI=70)            # test_gpu_eval_fallback.py's: 60 users x 501 items
    return IdSpace(OU=1, TOU=70, SOU=22, OI=201, TOI=300, SOI=16)               # the same sizes with the items overlapped


def _eval_model(mode, flag, seed=None, device=DEV):
    """DeepAPF of test_gpu_eval_fallback.py's set-up (D = 16), built on the CPU from a fixed seed, its six tables overwritten by randn x 0.3."""
    from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
    ids = _eval_ids(mode)
    torch.manual_seed(EVAL_SEED[mode] if seed is None else seed)
    extra = {'native_full_sort': True} if flag else {}
    cfg = base_config(device, embedding_size=16, beta=0.5, topk=[5, 10], eval_batch_size=1000, **extra)
    model = DeepAPF(cfg, FakeDataset(ids))
    assert model.mode == mode
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith('_embedding.weight'):
                p.copy_(torch.randn(p.shape) * 0.3)
            elif n.endswith('.0.bias'):
                p.copy_(torch.randn(p.shape) * 0.1)
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


def _all_pairs(model, users, N, device=DEV):
    from recbole_cdr_amd.data.interaction import Interaction
    ut = torch.as_tensor(users, device=device)
    return ut, Interaction({'target_user_id': ut.repeat_interleave(N), 'target_item_id': torch.arange(N, device=device).repeat(ut.numel())})


def _model_reference(model, ut, N):
    """test 1's reference for the model's operands, with the bound that also holds ``predict``'s operation order."""
    ki, share, only, other, n_over, W1, b1, w2, wp = model._fullsort_operands()
    D = share.shape[1]
    ref, _ = deepapf_fullsort_fp64(ki, share.detach(), only.detach(), other.detach(), ut, N, n_over, W1.detach(), b1.detach(), w2.detach(),
                                   wp.detach(), depths=fullsort_depths(D), cover_predict=True)
    return ref


@pytest.mark.parametrize('mode', ['overlap_users', 'overlap_items'])
def test_deepapf_native_full_sort_model_and_trainer(mode):
    """Flag on, 60 users x 501 items: ``full_sort_predict`` and ``predict`` over all pairs both lie inside the fp64 reference's bounds; every
    user's adjacent gaps among ranks 1..k + 1 of the masked ``predict`` scores exceed twice the bound (so the order is decided), and
    ``full_sort_topk`` (fused launch forced) returns the item lists of mask + torch.topk of ``predict``; ``Trainer.evaluate`` gives the same
    metrics on the fused route, with ``fused_topk=False`` and from a flag-off model with the same parameters; a pickle round trip and a
    deepcopy of the flag-on model still evaluate.  Flag off: the reference's contract."""
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
    ut, pairs = _all_pairs(model, users, N)
    want = model.predict(pairs).view(60, N).float()
    assert torch.equal(off.predict(pairs).view(60, N).float(), want)
    got = model.full_sort_predict(Interaction({'target_user_id': ut})).view(60, N)
    ref = _model_reference(model, ut, N)
    r_fs, r_pr = float(ref.ratio(got).max()), float(ref.ratio(want).max())
    print(f'{mode}: worst error / bound: full_sort_predict {r_fs:.3f}, predict {r_pr:.3f}; largest |difference| {float((got - want).abs().max()):.3e}')
    assert r_fs <= 1.0 and r_pr <= 1.0
    assert bool(((got - want).abs().double() <= 2 * ref.e).all())
    # the order of every user's first k + 1 unmasked items is decided beyond the bound
    rows, colsn = torch.from_numpy(hi[:, 0] - 1).to(DEV), torch.from_numpy(hi[:, 1]).to(DEV)
    masked = want.clone()
    masked[:, 0] = NEG
    masked[rows, colsn] = NEG
    top_v, top_i = torch.topk(masked, k + 1, dim=1)
    gaps = (top_v[:, :-1] - top_v[:, 1:]).double()
    b = torch.gather(ref.e, 1, top_i)
    margin = gaps - 2 * torch.maximum(b[:, :-1], b[:, 1:])
    print(f'{mode}: smallest (gap - 2 bound) among ranks 1..{k + 1}: {float(margin.min()):.3e}')
    assert bool((margin > 0).all())
    order = torch.argsort(rows * N + colsn)
    indptr = torch.zeros(61, dtype=torch.int64, device=DEV)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=60), 0)
    model.fullsort_topk_min_items = 0
    v, i = model.full_sort_topk(Interaction({'target_user_id': ut}), k, hist_indptr=indptr, hist_cols=colsn[order].contiguous())
    assert torch.equal(i, top_i[:, :k])
    m_fs = got.clone()
    m_fs[:, 0] = NEG
    m_fs[rows, colsn] = NEG
    _check(m_fs, k, v, i)
    # the trainer, three ways
    def evaluate(m, c, **kw):
        loader = FullSortEvalLoader('target_user_id', ev, hi, N, 4096, DEV, users_per_batch=25)
        return Trainer(dict(c, graph_step=False, **kw), m).evaluate(loader)
    res = [evaluate(model, cfg), evaluate(model, cfg, fused_topk=False), evaluate(off, cfg_off)]
    assert len(res[0]) == 10
    for other in res[1:]:
        assert set(other) == set(res[0])
        for key in res[0]:
            assert np.isfinite(res[0][key]) and abs(res[0][key] - other[key]) <= 1e-6, (key, res[0][key], other[key])
    for clone in (pickle.loads(pickle.dumps(model)), copy.deepcopy(model)):
        assert hasattr(clone, 'full_sort_topk') and clone.fullsort_topk_min_items == 0
        again = evaluate(clone, cfg)
        for key in res[0]:
            assert abs(res[0][key] - again[key]) <= 1e-6, (key, res[0][key], again[key])


def test_deepapf_native_full_sort_outside_the_kernels_widths():
    """embedding_size = 6 (no multiple of 4): the opted-in methods still work, on chunked ``predict`` inside ``full_sort_predict``."""
    from oracle.common import IdSpace
    from recbole_cdr_amd.data.interaction import Interaction
    from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
    ids = IdSpace(OU=40, TOU=30, SOU=35, OI=1, TOI=500, SOI=70)
    torch.manual_seed(5)
    model = DeepAPF(base_config(DEV, embedding_size=6, beta=0.5, native_full_sort=True), FakeDataset(ids)).to(DEV)
    model.eval()
    N = ids.target_num_items
    ut, pairs = _all_pairs(model, np.arange(1, 8), N)
    got = model.full_sort_predict(Interaction({'target_user_id': ut})).view(7, N)
    assert torch.equal(got, model.predict(pairs).view(7, N).float())
    model.fullsort_topk_min_items = 0
    v, i = model.full_sort_topk(Interaction({'target_user_id': ut}), 5)
    m = got.clone()
    m[:, 0] = NEG
    _check(m, 5, v, i)


def test_deepapf_fullsort_refuses_bad_arguments_before_any_launch():
    """k = 0 / 65, D = 6 / 132 and a workspace one byte short come back non-zero with an error text; the outputs of a refused call are
    untouched (nothing was launched)."""
    from recbole_cdr_amd import binding as B_
    from recbole_cdr_amd import functional as F_
    c, _full = _case(8, 5, 77, 3, False)
    for k in (0, 65):
        with pytest.raises(RuntimeError, match='cdr_deepapf_fullsort_topk'):
            F_.deepapf_fullsort_topk(*_call_args(c), k)
    lib = B_.load()
    need = ctypes.c_size_t(0)
    assert lib.cdr_deepapf_fullsort_topk_workspace_bytes(5, 77, 10, ctypes.byref(need)) == 0 and need.value > 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    vals = torch.full((5, 10), 7.0, device=DEV)
    idx = torch.full((5, 10), 7, dtype=torch.int64, device=DEV)
    out = torch.full((5, 77), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    wide = torch.zeros(200, 132, device=DEV)

    def head(D, tab=None):
        s, o, t = (c['share'], c['only'], c['other']) if tab is None else (tab, tab, tab)
        return (B_.stream(), 0, p(s), D, p(o), D, p(t), D, p(c['uid']), 5, 77, D, 3, p(c['W1']), p(c['b1']), p(c['w2']), p(c['wp']))

    def topk(D, k, nbytes, tab=None):
        return lib.cdr_deepapf_fullsort_topk(*head(D, tab), k, None, None, 1, p(vals), p(idx), p(ws), nbytes)

    for k in (0, 65):
        assert topk(8, k, need.value) != 0 and b'k = ' in lib.cdr_last_error()
    for D in (6, 132):
        assert topk(D, 10, need.value, wide) != 0 and b'outside the kernel' in lib.cdr_last_error()
        assert lib.cdr_deepapf_fullsort(*head(D, wide), p(out), 77) != 0 and b'outside the kernel' in lib.cdr_last_error()
    assert topk(8, 10, need.value - 1) != 0 and b'workspace' in lib.cdr_last_error()
    torch.cuda.synchronize()
    assert bool((vals == 7.0).all()) and bool((idx == 7).all()) and bool((out == 7.0).all())
    assert topk(8, 10, need.value) == 0
    torch.cuda.synchronize()
    assert bool((vals < 1.0).all()) and bool((idx >= 1).all())
