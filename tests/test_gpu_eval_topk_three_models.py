"""SSCDR, CLFM and DCDCSR evaluate through ``full_sort_topk`` like the other seven models: for every phase / mode case their
``full_sort_predict`` distinguishes, the fused mask + top-k returns the bits of ``torch.topk`` over the masked ``full_sort_predict``
-- and so it does for the other contraction models, EMCDR (every phase, both overlap modes), CMF and BiTGCF, and for all six
``full_sort_rank`` returns the positives' bits of ``full_sort_predict`` and the counts of ``trainer.rank_counts_reference`` over it;
``Trainer.evaluate`` returns the same metrics on both routes; SSCDR's evaluation bracket normalises its item table once and leaves nothing
behind.  Small models: 501 target items, 70 users of width 64 (the fused kernel itself runs), a non-empty history."""
import pickle

import numpy as np
import pytest
import torch

from helpers import DEV, FakeDataset, base_config

pytestmark = pytest.mark.gpu
NEG_INF = -float('inf')
D, K, N_USERS = 64, 10, 70


def _ids(mode):
    from oracle.common import IdSpace
    if mode == 'overlap_users':
        return IdSpace(OU=40, TOU=45, SOU=35, OI=1, TOI=500, SOI=70)
    return IdSpace(OU=1, TOU=84, SOU=80, OI=30, TOI=471, SOI=60)


def _dataset(ids, seed=0):
    """Interactions inside each domain's own id ranges (SSCDR samples from the source lists, DCDCSR counts popularities)."""
    rng = np.random.RandomState(seed)
    src_u = np.array(list(range(1, ids.OU)) + list(range(ids.OU + ids.TOU, ids.total_num_users)))
    src_i = np.array(list(range(1, ids.OI)) + list(range(ids.OI + ids.TOI, ids.total_num_items)))
    s_pairs = np.unique(np.stack([rng.choice(src_u, 400), rng.choice(src_i, 400)], 1), axis=0).astype(np.int64)
    t_pairs = np.unique(np.stack([rng.randint(1, ids.target_num_users, 900), rng.randint(1, ids.target_num_items, 900)], 1), axis=0).astype(np.int64)
    ds = FakeDataset(ids, s_pairs, t_pairs)
    ds.device = DEV
    return ds


def _model(name, mode='overlap_users'):
    ids = _ids(mode)
    torch.manual_seed(31)
    if name == 'SSCDR':
        from recbole_cdr_amd.model.cross_domain_recommender.sscdr import SSCDR
        cfg = base_config(DEV, embedding_size=D, margin=0.3, mlp_hidden_size=[48], topk=[5, 10], **{'lambda': 0.5})
        model = SSCDR(cfg, _dataset(ids)).to(DEV)
        with torch.no_grad():                        # rows longer than 1: the normalisation divides (max(|x|^2, 1) is 1 after the initialisation)
            for n, p in model.named_parameters():
                if n.endswith('embedding.weight'):
                    p.mul_(4.0)
    elif name == 'CLFM':
        from recbole_cdr_amd.model.cross_domain_recommender.clfm import CLFM
        cfg = base_config(DEV, user_embedding_size=48, source_item_embedding_size=D, target_item_embedding_size=D, share_embedding_size=24,
                          alpha=0.3, reg_weight=0.01, topk=[5, 10])
        model = CLFM(cfg, FakeDataset(ids)).to(DEV)
    else:
        from recbole_cdr_amd.model.cross_domain_recommender.dcdcsr import DCDCSR
        cfg = base_config(DEV, latent_factor_model='BPR', embedding_size=D, mlp_hidden_size=[48], k=4, map_batch_size=32, topk=[5, 10])
        model = DCDCSR(cfg, _dataset(ids)).to(DEV)
    model.eval()
    return ids, cfg, model


def _interaction(model, ids, source=False):
    from recbole_cdr_amd.data.interaction import Interaction
    if source:
        pool = np.array(list(range(1, ids.OU)) + list(range(ids.OU + ids.TOU, ids.total_num_users)))
        return Interaction({model.SOURCE_USER_ID: torch.from_numpy(pool[:N_USERS]).to(DEV)})
    return Interaction({model.TARGET_USER_ID: torch.arange(1, N_USERS + 1, device=DEV)})


def _assert_topk_equals_masked_predict(model, interaction, seed=0):
    U = N_USERS
    scores = model.full_sort_predict(interaction).view(U, -1).clone()
    N = scores.shape[1]
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    best = torch.topk(scores, 3, dim=1).indices
    rnd = torch.randint(0, N, (U, 12), device=DEV, generator=g)
    cols = [torch.unique(torch.cat([best[u], rnd[u]])) for u in range(U)]
    indptr = torch.zeros(U + 1, dtype=torch.int64, device=DEV)
    indptr[1:] = torch.cumsum(torch.tensor([c.numel() for c in cols], device=DEV), 0)
    hist = torch.cat(cols)
    scores[:, 0] = NEG_INF
    scores[torch.repeat_interleave(torch.arange(U, device=DEV), indptr[1:] - indptr[:-1]), hist] = NEG_INF
    want_v = torch.topk(scores, K, dim=1).values
    got_v, got_i = model.full_sort_topk(interaction, K, hist_indptr=indptr, hist_cols=hist)
    assert got_v.shape == (U, K) and got_i.dtype == torch.int64
    assert torch.equal(got_v, want_v), (got_v - want_v).abs().max()
    assert torch.equal(torch.gather(scores, 1, got_i), want_v)
    _assert_rank_equals_counts_over_masked_predict(model, interaction, scores, best, got_i, indptr, hist, g)
    return N


def _assert_rank_equals_counts_over_masked_predict(model, interaction, masked, best, top, hist_indptr, hist_cols, g):
    """``full_sort_rank`` under the same history: ``pos_score`` is the bits of the positives' entries of ``full_sort_predict``, the counts
    are ``trainer.rank_counts_reference`` over the same matrix with the masked entries NaN.  Positives per user: the best and the k-th
    unmasked column, three random ones, and the best column of all -- which the history masks (-1 three times)."""
    from recbole_cdr_amd.trainer.trainer import rank_counts_reference
    U, N = masked.shape
    pos = torch.cat([top[:, :1], top[:, K - 1:], best[:, :1], torch.randint(0, N, (U, 3), device=DEV, generator=g)], 1)
    cols = [torch.unique(pos[u]) for u in range(U)]
    pindptr = torch.zeros(U + 1, dtype=torch.int64, device=DEV)
    pindptr[1:] = torch.cumsum(torch.tensor([c.numel() for c in cols], device=DEV), 0)
    pcols = torch.cat(cols)
    prow = torch.repeat_interleave(torch.arange(U, device=DEV), pindptr[1:] - pindptr[:-1])
    full = model.full_sort_predict(interaction).view(U, -1)
    nan = torch.where(masked == NEG_INF, torch.full_like(masked, float('nan')), masked)
    assert bool((nan[prow, pcols] != nan[prow, pcols]).any()) and bool((masked != NEG_INF)[:, 1:].any(1).all())
    score, gt, eq, eqb, nun = model.full_sort_rank(interaction, pindptr, pcols, hist_indptr=hist_indptr, hist_cols=hist_cols)
    assert torch.equal(score.view(torch.int32), full[prow, pcols].view(torch.int32))
    _, *want = rank_counts_reference(nan, prow, pcols)
    for name, a, b in zip(('gt', 'eq', 'eq_before', 'n_unmasked'), (gt, eq, eqb, nun), want):
        assert a.dtype == b.dtype == torch.int32 and torch.equal(a, b), (name, int((a != b).sum()))
    assert bool((gt[pcols == top[prow, 0]] == 0).all())                             # the best unmasked column has nothing above it


@pytest.mark.parametrize('mode', ['overlap_users', 'overlap_items'])
@pytest.mark.parametrize('phase', ['SOURCE', 'TARGET', 'BOTH'])
def test_sscdr_full_sort_topk_equals_topk_of_masked_predict(phase, mode):
    ids, _, model = _model('SSCDR', mode)
    model.set_phase(phase)
    inter = _interaction(model, ids, source=phase == 'SOURCE')
    want_n = ids.OI + ids.SOI if phase == 'SOURCE' else ids.target_num_items
    model.fullsort_topk_min_items = 0                                            # the fused entry
    assert _assert_topk_equals_masked_predict(model, inter) == want_n
    model.freeze_for_eval()                                                      # ... on the cached operand and its norms
    assert _assert_topk_equals_masked_predict(model, inter, seed=1) == want_n
    model.unfreeze_eval()
    del model.fullsort_topk_min_items                                            # the default threshold: full_sort_predict + masked_topk
    from recbole_cdr_amd import functional as F_
    assert want_n < F_.SQDIST_TOPK_MIN_ITEMS
    _assert_topk_equals_masked_predict(model, inter, seed=2)


def test_sscdr_full_sort_topk_few_users():
    """A remainder batch of at most eight users (where the dot-product entry streams a GEMV) still ranks the distance matrix's bits."""
    from recbole_cdr_amd.data.interaction import Interaction
    ids, _, model = _model('SSCDR', 'overlap_items')
    model.set_phase('BOTH')
    model.fullsort_topk_min_items = 0
    users = torch.arange(1, 6, device=DEV)
    inter = Interaction({model.TARGET_USER_ID: users})
    scores = model.full_sort_predict(inter).view(5, -1).clone()
    scores[:, 0] = NEG_INF
    got_v, got_i = model.full_sort_topk(inter, K)
    want_v = torch.topk(scores, K, dim=1).values
    assert got_v.shape == (5, K) and torch.equal(got_v, want_v) and torch.equal(torch.gather(scores, 1, got_i), want_v)


def test_clfm_full_sort_topk_equals_topk_of_masked_predict():
    ids, _, model = _model('CLFM')
    model.set_phase('BOTH')
    assert _assert_topk_equals_masked_predict(model, _interaction(model, ids)) == ids.target_num_items


@pytest.mark.parametrize('mode', ['overlap_users', 'overlap_items'])
def test_dcdcsr_full_sort_topk_equals_topk_of_masked_predict_in_its_three_table_cases(mode):
    ids, _, model = _model('DCDCSR', mode)
    model.set_phase('SOURCE')
    assert _assert_topk_equals_masked_predict(model, _interaction(model, ids, source=True)) == ids.OI + ids.SOI
    model.set_phase('TARGET')
    assert _assert_topk_equals_masked_predict(model, _interaction(model, ids)) == ids.target_num_items
    model.set_phase('TARGET')                                                    # the second visit builds affine_embedding
    assert model.affine_embedding is not None
    assert _assert_topk_equals_masked_predict(model, _interaction(model, ids)) == ids.target_num_items


@pytest.mark.parametrize('mode', ['overlap_users', 'overlap_items'])
@pytest.mark.parametrize('phase', ['SOURCE', 'TARGET', 'OVERLAP'])
def test_emcdr_full_sort_topk_equals_topk_of_masked_predict(phase, mode):
    """SOURCE and OVERLAP / overlap_items score two row ranges, OVERLAP a mapped operand; with one shared item (overlap_users) the first
    range of SOURCE is the PAD row alone."""
    import test_gpu_candidate_eval as cand
    model, _, n_cols, _, _, _ = cand._emcdr_case(phase, mode)
    ids = _ids(mode)
    assert _assert_topk_equals_masked_predict(model, _interaction(model, ids, source=phase == 'SOURCE')) == n_cols
    assert n_cols == (ids.OI + ids.SOI if phase == 'SOURCE' else ids.target_num_items)


def test_cmf_full_sort_topk_equals_topk_of_masked_predict():
    import test_gpu_candidate_eval as cand
    ids, model = cand._default_route_model('CMF', cmf_width=D)
    assert _assert_topk_equals_masked_predict(model, _interaction(model, ids)) == ids.target_num_items


def test_bitgcf_full_sort_topk_equals_topk_of_masked_predict():
    import test_gpu_candidate_eval as cand
    ids, model = cand._bitgcf_model(n_layers=1)                                  # rows of 2 x 32 floats
    assert model.get_restore_e()[0].shape[1] == D
    assert _assert_topk_equals_masked_predict(model, _interaction(model, ids)) == ids.target_num_items


@pytest.mark.parametrize('name', ['SSCDR', 'CLFM', 'DCDCSR'])
def test_evaluate_returns_the_same_metrics_on_both_routes(name):
    """60 users x 501 items, random data (no ties at the cut): the fused route in one 60-user batch, in batches of 26 / 26 / 8 users, and
    the materialised route."""
    from recbole_cdr_amd.data.dataloader import FullSortEvalLoader
    from recbole_cdr_amd.trainer.trainer import Trainer
    ids, cfg, model = _model(name)
    model.set_phase('TARGET')
    if name == 'SSCDR':
        model.fullsort_topk_min_items = 0
    N, n_users = ids.target_num_items, 60
    rng = np.random.RandomState(2)
    users = np.arange(1, n_users + 1)
    ev = np.unique(np.stack([np.repeat(users, 4), rng.randint(1, N, 4 * n_users)], 1), axis=0)
    hi = np.unique(np.stack([np.repeat(users, 12), rng.randint(1, N, 12 * n_users)], 1), axis=0)

    def evaluate(**kw):
        loader = FullSortEvalLoader('target_user_id', ev, hi, N, 4096, DEV, users_per_batch=26)
        return Trainer(dict(cfg, graph_step=False, **kw), model).evaluate(loader)
    res = [evaluate(), evaluate(eval_users_per_batch=0), evaluate(fused_topk=False)]
    assert set(res[0]) == {f'{m}@{k}' for m in ('recall', 'hit', 'precision', 'mrr', 'ndcg') for k in (5, 10)}
    assert all(np.isfinite(v) for v in res[0].values())
    assert res[0] == res[1] == res[2], res
    assert '_eval_items' not in model.__dict__ and '_eval_frozen' not in model.__dict__


def test_sscdr_evaluation_bracket_normalises_the_item_table_once(monkeypatch):
    from recbole_cdr_amd import functional as F_
    ids, _, model = _model('SSCDR', 'overlap_items')
    model.set_phase('BOTH')                                                      # two item ranges: the mapped overlap rows, the target-only rows
    model.fullsort_topk_min_items = 0
    inter = _interaction(model, ids)
    heights = {ids.OI, ids.target_num_items - ids.OI}
    assert N_USERS not in heights
    calls, real = [], F_.sqnorm_normalize

    def counting(x):
        if x.shape[0] in heights:
            calls.append(x.shape[0])
        return real(x)
    monkeypatch.setattr(F_, 'sqnorm_normalize', counting)
    outside = model.full_sort_predict(inter)
    model.full_sort_topk(inter, K)
    assert sorted(calls) == sorted(list(heights) * 2)                                  # outside a bracket every call normalises
    keys = set(model.state_dict())
    del calls[:]
    model.freeze_for_eval()
    a = model.full_sort_topk(inter, K)
    b = model.full_sort_topk(inter, K)
    inside = model.full_sort_predict(inter)
    assert sorted(calls) == sorted(heights)                                      # once for the three calls
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(inside, outside)
    assert model.__dict__['_eval_items']['sqnorm'] is not None
    assert set(model.state_dict()) == keys
    clone = pickle.loads(pickle.dumps(model))
    assert '_eval_items' not in clone.__dict__ and '_eval_frozen' not in clone.__dict__
    model.unfreeze_eval()
    assert '_eval_items' not in model.__dict__
    model.freeze_for_eval()
    model.full_sort_topk(inter, K)
    assert '_eval_items' in model.__dict__
    model.set_phase('TARGET')
    assert '_eval_items' not in model.__dict__
    model.full_sort_topk(inter, K)
    model.train()
    assert '_eval_items' not in model.__dict__ and '_eval_frozen' not in model.__dict__
