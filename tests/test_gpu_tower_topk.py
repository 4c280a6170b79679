"""The MLP-tower full-sort with the evaluation mask + top-k as its epilogue (cdr_conet_fullsort_topk) against the score-writing form of
the same kernel, and the models built on it: CoNet.full_sort_topk, DTCDR.full_sort_predict / full_sort_topk and ``Trainer.evaluate`` on
both routes.  Reference of the evaluation: recbole Trainer._full_sort_batch_eval (scores -> -inf at PAD and history -> torch.topk) over
conet.py:222-242 / dtcdr.py:112-126."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

from helpers import DEV, FakeDataset, base_config

pytestmark = pytest.mark.gpu

NEG = -float('inf')


def _tower(D, layers, U, N):
    """The inputs of test_conet_fullsort_kernel_vs_fp64_tower (which pins conet_fullsort to fp64): seed D + N, randn x 0.3, xavier weights."""
    from recbole_cdr_amd import functional as F_
    g = torch.Generator().manual_seed(D + N)
    dims = [2 * D] + layers
    Ws = [torch.randn(b, a, generator=g) * (2.0 / (a + b)) ** 0.5 for a, b in zip(dims[:-1], dims[1:])]
    bs = [torch.randn(b, generator=g) * 0.1 for b in dims[1:]]
    wo, bo = torch.randn(1, dims[-1], generator=g) * 0.5, torch.randn(1, generator=g) * 0.1
    users, items = torch.randn(U, D, generator=g) * 0.3, torch.randn(N, D, generator=g) * 0.3
    dv = lambda t: t.to(DEV)
    P = F_.gemm(dv(items), dv(Ws[0])[:, D:], trans_b=True)
    Q = F_.gemm(dv(users), dv(Ws[0])[:, :D], trans_b=True, bias=dv(bs[0]))
    return P, Q, [dv(w) for w in Ws[1:]], [dv(b) for b in bs[1:]], dv(wo), dv(bo)


def _padded_topk(masked, k):
    """torch.topk of a masked matrix in the kernel's contract: (-inf, -1) where fewer than k unmasked columns are left."""
    U, N = masked.shape
    kk = min(k, N)
    v, i = torch.topk(masked, kk, dim=1)
    if kk < k:
        v = torch.cat([v, v.new_full((U, k - kk), NEG)], 1)
        i = torch.cat([i, i.new_full((U, k - kk), -1)], 1)
    return v, torch.where(v == NEG, torch.full_like(i, -1), i)


def _check(masked, k, got_v, got_i):
    want_v, _ = _padded_topk(masked, k)
    assert tuple(got_v.shape) == tuple(got_i.shape) == (masked.shape[0], k)
    assert torch.equal(got_v, want_v), (got_v - want_v).abs().nan_to_num(posinf=9.0).max()
    real = got_v > NEG
    assert bool((got_i[~real] == -1).all()) and bool((got_i[real] >= 0).all())
    # the column of every entry holds that entry's value (columns may differ from torch's only between exactly tied scores) and is not masked
    picked = torch.gather(masked, 1, got_i.clamp(min=0))
    assert torch.equal(picked[real], want_v[real])
    # no duplicates among a user's columns
    s = torch.sort(torch.where(real, got_i, -1 - torch.arange(k, device=got_i.device).expand_as(got_i)), dim=1).values
    assert bool((s[:, 1:] != s[:, :-1]).all())


CASES = [(16, [64, 32, 16, 8], 5, 77, 10),           # tail tile
         (64, [64, 32, 16, 8], 70, 20011, 10),       # more than one 32-user chunk
         (64, [32, 16], 40, 9001, 20),               # DTCDR's instantiation, h1 <= 32
         (8, [12, 8, 4], 3, 41, 5),                  # widths that are not multiples of 8
         (32, [48, 24], 7, 100, 1),                  # k = 1
         (16, [20, 32, 32, 32], 33, 2049, 64),       # k larger than a tile, k = 64 (24 users per workgroup: two user groups), widest tail
         (128, [64, 32, 16, 8], 130, 4000, 50),      # several user groups at a large k, C3's D
         (64, [32, 16], 3, 300001, 10),              # more than one round of tiles per workgroup (the top-k grid is at most 512 x 128 items; the seeded path)
         (64, [64, 8], 33, 1, 10),                   # a one-item catalogue: padding
         (64, [32, 16], 160, 81921, 10)]             # the seeded path with two user groups, just over its threshold of 81,920 items; a partial last tile


@pytest.mark.parametrize('D,layers,U,N,k', CASES)
def test_tower_topk_matches_topk_of_masked_scores(D, layers, U, N, k):
    """Fused mask + top-k == torch.topk over the evaluation-masked output of ``conet_fullsort`` on the same operands: one tower, two
    epilogues, so the values are bit-equal; columns may differ only between exactly tied scores.  The history holds each user's 7 best
    columns and 30 random ones, so the mask decides the result; a second call runs without history and keeps the PAD column."""
    from recbole_cdr_amd import functional as F_
    P, Q, Ws, bs, wo, bo = _tower(D, layers, U, N)
    full = F_.conet_fullsort(P, Q, Ws, bs, wo, bo)
    g = torch.Generator().manual_seed(U + N)
    best = torch.topk(full, min(7, N), dim=1).indices
    rnd = torch.randint(0, N, (U, 30), generator=g).to(DEV)
    cols = [torch.unique(torch.cat([best[u], rnd[u]])) for u in range(U)]           # ascending, deduplicated
    indptr = torch.zeros(U + 1, dtype=torch.int64, device=DEV)
    indptr[1:] = torch.cumsum(torch.tensor([c.numel() for c in cols], device=DEV), 0)
    hist = torch.cat(cols)
    masked = full.clone()
    masked[:, 0] = NEG
    for u in range(U):
        masked[u, cols[u]] = NEG
    # the tie rule must have almost nothing to decide: at most 5 % of the users have two equal values among their top k + 1
    top = torch.topk(masked, min(k + 1, N), dim=1).values
    tied = ((top[:, 1:] == top[:, :-1]) & (top[:, 1:] > NEG)).any(1).float().mean().item() if top.shape[1] > 1 else 0.0
    print(f'case D={D} {layers} U={U} N={N} k={k}: users with a tie among their top k+1: {100 * tied:.1f} %, '
          f'scores {float(full.min()):.3f}..{float(full.max()):.3f}')
    assert tied <= 0.05
    got_v, got_i = F_.conet_fullsort_topk(P, Q, Ws, bs, wo, bo, k, hist_indptr=indptr, hist_cols=hist)
    _check(masked, k, got_v, got_i)
    got_v2, got_i2 = F_.conet_fullsort_topk(P, Q, Ws, bs, wo, bo, k, exclude_first_col=False)
    _check(full, k, got_v2, got_i2)
    if N == 1:
        # PAD kept: one real entry, then padding; PAD masked: padding only
        assert bool((got_i2[:, 0] == 0).all()) and bool((got_i2[:, 1:] == -1).all()) and bool((got_v2[:, 1:] == NEG).all())
        v3, i3 = F_.conet_fullsort_topk(P, Q, Ws, bs, wo, bo, k)
        assert bool((v3 == NEG).all()) and bool((i3 == -1).all())


def test_tower_topk_refuses_bad_arguments_before_any_launch():
    """k outside 1..64, a tower outside cdr_conet_fullsort_supported and a workspace that is too small come back as CDR_EINVAL with an
    error text; the outputs of a refused call are untouched (nothing was launched)."""
    from recbole_cdr_amd import binding as B_
    from recbole_cdr_amd import functional as F_
    P, Q, Ws, bs, wo, bo = _tower(16, [64, 32, 16, 8], 5, 77)
    for k in (0, 65):
        with pytest.raises(RuntimeError, match='cdr_conet_fullsort_topk'):
            F_.conet_fullsort_topk(P, Q, Ws, bs, wo, bo, k)
    wide = torch.zeros(40, 64, device=DEV)                                            # a tail layer of width 40 > 32
    with pytest.raises(RuntimeError, match='outside the kernel'):
        F_.conet_fullsort_topk(P, Q, [wide], [torch.zeros(40, device=DEV)], torch.zeros(1, 40, device=DEV), bo, 10)
    lib = B_.load()
    need = ctypes.c_size_t(0)
    assert lib.cdr_conet_fullsort_topk_workspace_bytes(5, 77, 10, ctypes.byref(need)) == 0 and need.value > 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    vals = torch.full((5, 10), 7.0, device=DEV)
    idx = torch.full((5, 10), 7, dtype=torch.int64, device=DEV)
    dims = (ctypes.c_int * 3)(32, 16, 8)
    Wp = (ctypes.c_void_p * 3)(*[w.data_ptr() for w in Ws])
    bp = (ctypes.c_void_p * 3)(*[b.data_ptr() for b in bs])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    args = lambda nbytes: (B_.stream(), p(P), P.stride(0), p(Q), Q.stride(0), 5, 77, 64, 3, dims, Wp, bp, p(wo), p(bo), 10, None, None, 1,
                           p(vals), p(idx), p(ws), nbytes)
    assert lib.cdr_conet_fullsort_topk(*args(need.value - 1)) != 0
    assert b'workspace' in lib.cdr_last_error()
    torch.cuda.synchronize()
    assert bool((vals == 7.0).all()) and bool((idx == 7).all())
    assert lib.cdr_conet_fullsort_topk(*args(need.value)) == 0
    torch.cuda.synchronize()
    assert bool((vals < 1.0).all()) and bool((idx >= 1).all())


# ---- models -----------------------------------------------------------------------------------------------------------------------
def _ids():
    from oracle.common import IdSpace
    return IdSpace(OU=120, TOU=100, SOU=90, OI=1, TOI=3000, SOI=400)


def _history(U, N, per_user, seed):
    g = torch.Generator().manual_seed(seed)
    cols = [torch.unique(torch.randint(1, N, (per_user,), generator=g)) for _ in range(U)]
    indptr = torch.zeros(U + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.tensor([c.numel() for c in cols]), 0)
    return indptr.to(DEV), torch.cat(cols).to(DEV)


def _masked(scores, indptr, cols):
    m = scores.clone()
    m[:, 0] = NEG
    rows = torch.repeat_interleave(torch.arange(m.shape[0], device=m.device), indptr[1:] - indptr[:-1])
    m[rows, cols] = NEG
    return m


def _dtcdr(hidden, seed=3):
    from recbole_cdr_amd.model.cross_domain_recommender.dtcdr import DTCDR
    from recbole_cdr_amd.data.interaction import Interaction
    ids = _ids()
    torch.manual_seed(seed)
    model = DTCDR(base_config(DEV, embedding_size=64, mlp_hidden_size=hidden, dropout_prob=0.2, base_model='NeuMF', alpha=0.3), FakeDataset(ids)).to(DEV)
    with torch.no_grad():                                    # biases away from their zero initialisation
        for p in model.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    model.eval()
    users = torch.tensor([1, 2, 50, 119, 120, 121, 200, 219, 7], device=DEV)
    return ids, model, users, Interaction({'target_user_id': users})


@pytest.mark.parametrize('hidden', [[32, 16], [24]])
def test_dtcdr_full_sort_predict_equals_predict_on_every_pair(hidden):
    """full_sort_predict(users)[u, i] == predict on the pair (u, i) (what the reference's evaluation calls) within 1e-5 relative, for all
    pairs of 9 users x 3,001 target items: the default tower on the full-sort kernel, a one-layer ``mlp_hidden_size`` (no tail layer) on
    the per-user route.  full_sort_topk == mask + torch.topk of full_sort_predict, values bit-equal."""
    from recbole_cdr_amd.data.interaction import Interaction
    ids, model, users, inter = _dtcdr(hidden)
    N = ids.target_num_items
    got = model.full_sort_predict(inter).view(users.numel(), -1)
    assert tuple(got.shape) == (9, N)
    pairs = Interaction({'target_user_id': users.repeat_interleave(N), 'target_item_id': torch.arange(N, device=DEV).repeat(users.numel())})
    want = model.predict(pairs).view(users.numel(), N)
    rel = ((got - want).abs() / want.abs()).max().item()
    print(f'DTCDR {hidden}: full_sort_predict vs predict, largest relative difference {rel:.3e}')
    assert rel <= 1e-5
    indptr, cols = _history(users.numel(), N, 40, 5)
    for min_items in (None, 0):                  # the default route at this catalogue size (unfused), then the fused launch forced
        if min_items is not None:
            model.fullsort_topk_min_items = min_items
        v, i = model.full_sort_topk(inter, 10, hist_indptr=indptr, hist_cols=cols)
        _check(_masked(got, indptr, cols), 10, v, i)


def test_dtcdr_eval_cache_lives_inside_the_bracket_only():
    """P is kept between freeze_for_eval() and unfreeze_eval() and nowhere else: a training step between two evaluations changes the
    scores, and a pickled model holds no cache."""
    ids, model, users, inter = _dtcdr([32, 16])
    from recbole_cdr_amd.data.interaction import Interaction
    model.freeze_for_eval()
    a = model.full_sort_predict(inter).clone()
    assert '_eval_P' in model.__dict__
    assert torch.equal(model.full_sort_predict(inter), a)
    blob = pickle.dumps(model)
    assert '_eval_P' not in pickle.loads(blob).__dict__ and '_eval_frozen' not in pickle.loads(blob).__dict__
    assert len(blob) < sum(p.numel() for p in model.parameters()) * 4 + (1 << 20)          # no table-sized extra tensor
    model.unfreeze_eval()
    assert '_eval_P' not in model.__dict__
    # one dense training step on a BOTH batch
    model.train()
    g = torch.Generator().manual_seed(1)
    B = 256
    batch = Interaction({'source_user_id': torch.randint(1, ids.OU, (B,), generator=g).to(DEV),
                         'source_item_id': torch.randint(ids.OI + ids.TOI, ids.total_num_items, (B,), generator=g).to(DEV),
                         'source_label': torch.randint(0, 2, (B,), generator=g).float().to(DEV),
                         'target_user_id': users.repeat(29)[:B].contiguous(),
                         'target_item_id': torch.randint(1, ids.target_num_items, (B,), generator=g).to(DEV),
                         'target_label': torch.randint(0, 2, (B,), generator=g).float().to(DEV)})
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    model.calculate_loss(batch).backward()
    opt.step()
    model.eval()
    model.freeze_for_eval()
    b = model.full_sort_predict(inter)
    model.unfreeze_eval()
    assert not torch.equal(a, b) and float((a - b).abs().max()) > 1e-4


@pytest.mark.parametrize('hidden,fused', [([64, 32, 16, 8], True), ([64, 32, 16, 8], False), ([80, 16], True)])
def test_conet_full_sort_topk_equals_masked_topk_of_full_sort_predict(hidden, fused):
    """CoNet.full_sort_topk == mask + torch.topk of full_sort_predict, inside and outside a freeze_for_eval() bracket: on the fused launch,
    with ``fullsort_fused = False`` and for a tower outside the kernel's range (first width 80) on the torch route."""
    from recbole_cdr_amd.model.cross_domain_recommender.conet import CoNet
    from recbole_cdr_amd.data.interaction import Interaction
    ids = _ids()
    torch.manual_seed(8)
    model = CoNet(base_config(DEV, embedding_size=32, reg_weight=0.01, mlp_hidden_size=hidden), FakeDataset(ids)).to(DEV)
    model.eval()
    model.fullsort_fused = fused
    model.fullsort_topk_min_items = 0            # the fused launch also for this small catalogue (the default keeps it for >= 250,000 items)
    users = torch.arange(1, 41, device=DEV)
    inter = Interaction({'target_user_id': users})
    N = ids.target_num_items
    indptr, cols = _history(40, N, 25, 9)
    for frozen in (False, True):
        if frozen:
            model.freeze_for_eval()
        scores = model.full_sort_predict(inter).view(40, N)
        v, i = model.full_sort_topk(inter, 20, hist_indptr=indptr, hist_cols=cols)
        _check(_masked(scores, indptr, cols), 20, v, i)
        if frozen:
            model.unfreeze_eval()


def _eval_loader(ids, n_users=60, seed=2):
    from recbole_cdr_amd.data.dataloader import FullSortEvalLoader
    rng = np.random.RandomState(seed)
    N = ids.target_num_items
    users = np.arange(1, n_users + 1)
    ev = np.stack([np.repeat(users, 4), rng.randint(1, N, 4 * n_users)], 1)
    hi = np.stack([np.repeat(users, 12), rng.randint(1, N, 12 * n_users)], 1)
    return FullSortEvalLoader('target_user_id', ev, hi, N, 4096, DEV, users_per_batch=25)


@pytest.mark.parametrize('name', ['CoNet', 'DTCDR'])
def test_trainer_evaluate_same_metrics_on_both_routes(name):
    """Trainer.evaluate over 60 users x 501 items with a history: the fused mask + top-k route and the score-matrix route give the same
    metric dictionary (bit-equal values; hits can differ only through the order of exactly tied scores, of which there are none here)."""
    from oracle.common import IdSpace
    from recbole_cdr_amd.trainer.trainer import Trainer
    from recbole_cdr_amd.model.cross_domain_recommender.conet import CoNet
    from recbole_cdr_amd.model.cross_domain_recommender.dtcdr import DTCDR
    ids = IdSpace(OU=40, TOU=30, SOU=35, OI=1, TOI=500, SOI=70)
    torch.manual_seed(12)
    if name == 'CoNet':
        cfg = base_config(DEV, embedding_size=16, reg_weight=0.01, mlp_hidden_size=[64, 32, 16, 8], topk=[5, 10])
        model = CoNet(cfg, FakeDataset(ids)).to(DEV)
    else:
        cfg = base_config(DEV, embedding_size=16, mlp_hidden_size=[32, 16], dropout_prob=0.1, base_model='NeuMF', alpha=0.3, topk=[5, 10])
        model = DTCDR(cfg, FakeDataset(ids)).to(DEV)
    res = []
    for fused in (True, False):
        model.fullsort_topk_min_items = 0        # (500 items: the models' default would take the unfused route inside full_sort_topk)
        trainer = Trainer(dict(cfg, fused_topk=fused, deferred_adam=False), model)
        res.append(trainer.evaluate(_eval_loader(ids)))
        assert '_eval_P' not in model.__dict__
    assert set(res[0]) == set(res[1]) and len(res[0]) == 10
    for k in res[0]:
        assert np.isfinite(res[0][k]) and res[0][k] == res[1][k], (k, res[0][k], res[1][k])
