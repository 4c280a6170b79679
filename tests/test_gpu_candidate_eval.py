"""Sampled-candidate evaluation on the GPU: ``functional.candidate_scores`` (cdr_candidate_scores_f32) against float64 with a
propagated rounding bound, ``functional.candidate_rank`` (cdr_candidate_rank_f32) against integer counts taken on the same score bits,
the models' native ``candidate_scores`` against the base-class route through the existing ``predict``, and ``Trainer.evaluate`` over a
``NegSampleEvalLoader`` against brute-force metrics on the reference's formulation (a row of -inf with the candidates' scores scattered
in).

Worst error / bound of ``candidate_scores`` on an MI355X: see DESIGN.md 4.4.6."""
import numpy as np
import pytest
import torch

from fp64_bounds import EV, U32, gam
from helpers import DEV, FakeDataset, base_config

pytestmark = pytest.mark.gpu
K_COLS = 8192                                    # kRankCols of csrc/cdr_rank.h: candidates per workgroup of the rank kernel
NAN = float('nan')


def _ragged(U, N, n0, seed, max_rand=150):
    """A ragged candidate CSR over U users and a catalogue of N columns split at n0: user 0 has 65 candidates including columns 0, n0 - 1,
    n0 and N - 1; then users with 0, 1, 63, 64, K_COLS and K_COLS + 1 candidates; the rest between 1 and ``max_rand``.  Positives: a
    subset of each user's candidates (0..6; the K_COLS user has 300, several walks of kRankBatch = 16)."""
    g = torch.Generator(); g.manual_seed(seed)
    counts = [65, 0, 1, 63, 64, K_COLS, K_COLS + 1][:U] + torch.randint(1, max_rand + 1, (max(U - 7, 0),), generator=g).tolist()
    cols, pos, indptr, pindptr = [], [], [0], [0]
    for u, n in enumerate(counts):
        n = min(n, N)
        c = torch.randperm(N, generator=g)[:n]
        if u == 0:
            plant = torch.tensor(sorted({0, max(n0 - 1, 0), min(n0, N - 1), N - 1}))
            c = torch.cat([plant, c[~torch.isin(c, plant)]])[:n]
        c = torch.sort(c).values
        npos = 300 if n == K_COLS else int(torch.randint(0, 7, (1,), generator=g))
        p = torch.sort(c[torch.randperm(n, generator=g)[:min(npos, n)]]).values
        cols.append(c); pos.append(p)
        indptr.append(indptr[-1] + n); pindptr.append(pindptr[-1] + p.numel())
    t = lambda x: torch.as_tensor(x, dtype=torch.int64, device=DEV)
    return t(indptr), torch.cat(cols).to(DEV), t(pindptr), torch.cat(pos).to(DEV)


def _operands(U, N, n0, D, seed):
    g = torch.Generator(); g.manual_seed(seed)
    ue = (torch.randn(U, D, generator=g) * 0.5).to(DEV)
    tab = (torch.randn(N, D, generator=g) * 0.5).to(DEV)
    return ue, tab


def _scores_fp64(ue, tab, indptr, cols, distance):
    """The kernel's operations restated on EV: products (differences and squares) rounded once each, a sum of D terms in any order."""
    rows = torch.repeat_interleave(torch.arange(ue.shape[0], device=DEV), indptr[1:] - indptr[:-1])
    out_v, out_e = [], []
    for s in range(0, cols.numel(), 1 << 15):                    # [chunk, D] float64 blocks
        u, i = EV(ue[rows[s:s + (1 << 15)]].double()), EV(tab[cols[s:s + (1 << 15)]].double())
        if distance:
            d = u - i
            r = -((d * d).sum(1))
        else:
            x = (u.v * i.v).sum(1)
            r = EV(x, gam(ue.shape[1] + 2) * (u.v * i.v).abs().sum(1) + U32 * x.abs())       # the project's dot-product bound
        out_v.append(r.v); out_e.append(r.e)
    return EV(torch.cat(out_v), torch.cat(out_e))


# ---- 4. candidate_scores against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [30, 64, 128, 256])
@pytest.mark.parametrize('U', [1, 70, 600])
def test_candidate_scores_against_fp64(D, U):
    from recbole_cdr_amd import functional as F_
    worst = 0.0
    for N, split in ((9000, True), (70001, True), (9000, False)):
        n0 = N // 3 if split else N
        ue, tab = _operands(U, N, n0, D, seed=D + U)
        indptr, cols, _, _ = _ragged(U, N, n0, seed=U + N)
        slab0, slab1 = (tab[:n0], tab[n0:]) if split else (tab, None)
        assert {0, N - 1} | ({n0 - 1, n0} if split else set()) <= set(cols[:int(indptr[1])].tolist())      # the planted columns
        for distance in (False, True):
            got = F_.candidate_scores(ue, slab0, slab1, indptr, cols, distance=distance)
            assert got.shape == cols.shape and got.dtype == torch.float32
            want = _scores_fp64(ue, tab, indptr, cols, distance)
            ratio = want.ratio(got)
            worst = max(worst, float(ratio.max()) if ratio.numel() else 0.0)
            assert bool((ratio <= 1.0).all()), (D, U, N, distance, float(ratio.max()))
            if split and not distance and U == 70:                  # the slab boundary: one buffer or two, the same bits
                assert torch.equal(got, F_.candidate_scores(ue, tab, None, indptr, cols))
                assert torch.equal(got, F_.candidate_scores(ue, None, tab, indptr, cols))
    print(f'candidate_scores D={D} U={U}: worst error / bound {worst:.3f}')


def test_candidate_scores_empty_lists():
    from recbole_cdr_amd import functional as F_
    ue, tab = _operands(3, 50, 50, 64, seed=1)
    z = torch.zeros(4, dtype=torch.int64, device=DEV)
    assert F_.candidate_scores(ue, tab, None, z, torch.zeros(0, dtype=torch.int64, device=DEV)).numel() == 0


# ---- 5. candidate_rank against integer counts on the same score bits ------------------------------------------------------------------
def _rank_brute(indptr, cols, scores, pindptr, pcols):
    """numpy, user by user: the contract of cdr_candidate_rank_f32 read literally"""
    indptr, cols, pindptr, pcols = (x.cpu().numpy() for x in (indptr, cols, pindptr, pcols))
    s = scores.cpu().numpy()
    P, U = pcols.size, indptr.size - 1
    t = np.full(P, np.nan, np.float32)
    gt, eq, eqb = (np.full(P, -1, np.int32) for _ in range(3))
    n = np.zeros(U, np.int32)
    for u in range(U):
        c, v = cols[indptr[u]:indptr[u + 1]], s[indptr[u]:indptr[u + 1]]
        ok = ~np.isnan(v)
        n[u] = ok.sum()
        for p in range(pindptr[u], pindptr[u + 1]):
            at = np.nonzero(c == pcols[p])[0]
            if at.size == 0 or np.isnan(v[at[0]]):
                continue
            t[p] = v[at[0]]
            gt[p] = (v[ok] > t[p]).sum()
            same = ok & (v == t[p])
            eq[p], eqb[p] = same.sum(), (same & (c < pcols[p])).sum()
    return t, gt, eq, eqb, n


def _assert_rank_equal(got, want):
    t, gt, eq, eqb, n = got
    wt, wgt, weq, weqb, wn = want
    t = t.cpu().numpy()
    assert t.dtype == np.float32 and np.array_equal(np.isnan(t), np.isnan(wt))
    assert np.array_equal(t[~np.isnan(wt)].view(np.int32), wt[~np.isnan(wt)].view(np.int32))          # pos_score bit for bit
    for a, b in ((gt, wgt), (eq, weq), (eqb, weqb), (n, wn)):
        assert a.dtype == torch.int32 and torch.equal(a.cpu(), torch.from_numpy(b))


@pytest.mark.parametrize('U,N', [(1, 9000), (70, 9000), (600, 9000), (70, 70001)])
def test_candidate_rank_against_counts_on_the_same_bits(U, N):
    from recbole_cdr_amd import functional as F_
    indptr, cols, pindptr, pcols = _ragged(U, N, N // 3, seed=U + N)
    ue, tab = _operands(U, N, N // 3, 64, seed=3)
    scores = F_.candidate_scores(ue, tab[:N // 3], tab[N // 3:], indptr, cols)
    got = F_.candidate_rank(indptr, cols, scores, pindptr, pcols)
    _assert_rank_equal(got, _rank_brute(indptr, cols, scores, pindptr, pcols))
    assert int(got[1].min()) >= 0 and int(got[2].min()) >= 1
    again = F_.candidate_rank(indptr, cols, scores, pindptr, pcols)                    # run to run: the same bits
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(got, again))
    if U <= 70 and N == 9000:                                                          # (the trainer's device: cpu restatement agrees)
        ref = F_.candidate_rank_reference(indptr, cols, scores, pindptr, pcols)
        assert all(torch.equal(a, b) for a, b in zip(got[1:], ref[1:]))


def test_candidate_rank_ties_nan_and_missing_positives():
    from recbole_cdr_amd import functional as F_
    U, N = 70, 9000
    indptr, cols, pindptr, pcols = _ragged(U, N, N // 3, seed=5)
    g = torch.Generator(); g.manual_seed(9)
    scores = torch.randint(0, 5, (cols.numel(),), generator=g).float().to(DEV)          # integer-valued: ties everywhere
    ip, pp = indptr.tolist(), pindptr.tolist()
    big = 5                                                                             # the user with K_COLS candidates and 300 positives
    assert ip[big + 1] - ip[big] == K_COLS and pp[big + 1] - pp[big] == 300
    # a NaN candidate that is no positive (user 0), a positive whose score is NaN (user `big`), a positive that is not in its user's range
    mine = set(pcols[pp[0]:pp[1]].tolist())
    scores[next(c for c in range(ip[0], ip[1]) if int(cols[c]) not in mine)] = NAN
    nan_pos = pp[big] + 17
    scores[ip[big] + int(torch.nonzero(cols[ip[big]:ip[big + 1]] == pcols[nan_pos])[0])] = NAN
    w = next(u for u in range(7, U) if pp[u + 1] > pp[u])                                # a user that has a positive
    missing = pp[w]
    hi = int(pcols[missing + 1]) if missing + 1 < pp[w + 1] else N
    taken = set(cols[ip[w]:ip[w + 1]].tolist())
    pcols = pcols.clone()
    pcols[missing] = next(c for c in range(hi) if c not in taken)                        # (the positives stay ascending)
    got = F_.candidate_rank(indptr, cols, scores, pindptr, pcols)
    want = _rank_brute(indptr, cols, scores, pindptr, pcols)
    _assert_rank_equal(got, want)
    t, gt, eq, eqb, n = got
    for p in (nan_pos, missing):
        assert (int(gt[p]), int(eq[p]), int(eqb[p])) == (-1, -1, -1) and bool(torch.isnan(t[p]))
    assert int((gt < 0).sum()) == 2
    assert int(n[0]) == 64 and int(n[big]) == K_COLS - 1 and int(n[1]) == 0                 # the NaN candidates are counted nowhere
    assert int(eq.max()) > 50 and int(eqb.max()) > 50


def test_candidate_rank_refusals():
    from recbole_cdr_amd import binding as B_
    indptr, cols, pindptr, pcols = _ragged(8, 9000, 3000, seed=2)
    scores = torch.rand(cols.numel(), device=DEV)
    P, C = pcols.numel(), cols.numel()
    sent = [torch.full((P,), 7.5, device=DEV)] + [torch.full((n,), -77, device=DEV, dtype=torch.int32) for n in (P, P, P, 8)]
    for hole in range(5):
        outs = [B_.raw(x) for x in sent]
        outs[hole] = None
        with pytest.raises(RuntimeError, match='invalid argument'):
            B_.call('cdr_candidate_rank_f32', B_.stream(), 8, B_.i64(indptr), B_.i64(cols), B_.f32(scores), C, B_.i64(pindptr), B_.i64(pcols), P,
                    *outs)
    with pytest.raises(RuntimeError, match='invalid argument'):
        B_.call('cdr_candidate_scores_f32', B_.stream(), B_.f32(scores), 8, 4, B_.f32(scores), 8, None, 0, B_.i64(cols), B_.i64(cols), C, 0, None)
    with pytest.raises(RuntimeError, match='invalid argument'):
        B_.call('cdr_candidate_scores_f32', B_.stream(), B_.f32(scores), 8, 4, B_.f32(scores), 8, None, 0, B_.i64(cols), B_.i64(cols), C, 2,
                B_.f32(scores))
    torch.cuda.synchronize()
    assert bool((sent[0] == 7.5).all()) and all(bool((x == -77).all()) for x in sent[1:])
    # nothing to do: no launch, CDR_OK, the outputs untouched
    for U_, C_, P_ in ((0, C, P), (8, 0, P), (8, C, 0)):
        B_.call('cdr_candidate_rank_f32', B_.stream(), U_, B_.i64(indptr), B_.i64(cols), B_.f32(scores), C_, B_.i64(pindptr), B_.i64(pcols), P_,
                *[B_.raw(x) for x in sent])
    torch.cuda.synchronize()
    assert bool((sent[0] == 7.5).all()) and all(bool((x == -77).all()) for x in sent[1:])


# ---- 6. the models: the native candidate_scores against the base-class route through the existing predict -------------------------------
def _ids(mode):
    from oracle.common import IdSpace
    if mode == 'overlap_users':
        return IdSpace(OU=40, TOU=45, SOU=35, OI=1, TOI=500, SOI=70)
    return IdSpace(OU=1, TOU=84, SOU=80, OI=30, TOI=471, SOI=60)


def _dataset(ids, seed=0):
    rng = np.random.RandomState(seed)
    src_u = np.array(list(range(1, ids.OU)) + list(range(ids.OU + ids.TOU, ids.total_num_users)))
    src_i = np.array(list(range(1, ids.OI)) + list(range(ids.OI + ids.TOI, ids.total_num_items)))
    s_pairs = np.unique(np.stack([rng.choice(src_u, 400), rng.choice(src_i, 400)], 1), axis=0).astype(np.int64)
    t_pairs = np.unique(np.stack([rng.randint(1, ids.target_num_users, 900), rng.randint(1, ids.target_num_items, 900)], 1), axis=0).astype(np.int64)
    ds = FakeDataset(ids, s_pairs, t_pairs)
    ds.device = DEV
    return ds


N_USERS = 48


def _users(model, ids, source=False):
    from recbole_cdr_amd.data.interaction import Interaction
    if source:
        pool = np.array(list(range(1, ids.OU)) + list(range(ids.OU + ids.TOU, ids.total_num_users)))
        return Interaction({model.SOURCE_USER_ID: torch.from_numpy(pool[:N_USERS]).to(DEV)})
    return Interaction({model.TARGET_USER_ID: torch.arange(1, N_USERS + 1, device=DEV)})           # overlapped and target-only users


def _ev_mlp(x, layers):
    """layers: [(W [out, in], b or None, tanh?)] -- the linear kernels' operations on EV: a contraction of `in` terms, the bias, tanhf"""
    for W, b, tanh in layers:
        x = x.matmul(EV(W.detach().double().t()), depth=W.shape[1])
        if b is not None:
            x = x + EV(b.detach().double().unsqueeze(0))
        if tanh:
            x = x.tanh()
    return x


def _ev_take(ev, idx):
    return EV(ev.v[idx], ev.e[idx])


def _ev_sqnorm_normalize(x):
    """x / max(sum x^2, 1) per row (sscdr.py:120-124)"""
    return x / (x * x).sum(1, keepdim=True).maximum(1.0)


def _ev_scores(u, items, indptr, cols, distance):
    rows = torch.repeat_interleave(torch.arange(u.v.shape[0], device=DEV), indptr[1:] - indptr[:-1])
    a, b = _ev_take(u, rows), _ev_take(items, cols)
    if distance:
        d = a - b
        return -((d * d).sum(1))
    return (a * b).sum(1)


def _emcdr_case(phase, mode):
    """-> (model, interaction, n_cols, first slab's rows, fp64 operands with their formation error (user_e [U, D], items [n_cols, D]))"""
    from recbole_cdr_amd import binding as B_
    from recbole_cdr_amd.model.cross_domain_recommender.emcdr import EMCDR
    from fp64_bounds import ev_cat, ev_where
    ids = _ids(mode)
    cfg = base_config(DEV, latent_factor_model='BPR', source_embedding_size=64, target_embedding_size=64, reg_weight=0.01,
                      mapping_function='linear' if mode == 'overlap_items' else 'mlp', mlp_hidden_size=[24])
    torch.manual_seed(17)
    model = EMCDR(cfg, _dataset(ids)).to(DEV)
    model.set_phase(phase)
    model.eval()
    assert model.mode == mode
    OI, TI = ids.OI, ids.target_num_items
    layers = [(W, b, act == B_.ACT_TANH) for W, b, act in model.mapping_layers()]
    tab = lambda name: getattr(model, name).weight.detach().double()
    inter = _users(model, ids, source=phase == 'SOURCE')
    if phase == 'SOURCE':
        W = tab('source_item_embedding')
        return model, inter, OI + ids.SOI, OI, EV(tab('source_user_embedding')[inter[model.SOURCE_USER_ID]]), EV(torch.cat([W[:OI], W[TI:]]))
    users = inter[model.TARGET_USER_ID]
    u = EV(tab('target_user_embedding')[users])
    items = EV(tab('target_item_embedding')[:TI])
    if phase == 'OVERLAP' and mode == 'overlap_users':
        u = ev_where((users < ids.OU).unsqueeze(1), _ev_mlp(EV(tab('source_user_embedding')[users]), layers), u)
    elif phase == 'OVERLAP':
        items = ev_cat([_ev_mlp(EV(tab('source_item_embedding')[:OI]), layers), _ev_take(items, slice(OI, TI))])
    return model, inter, TI, OI, u, items


def _native_vs_predict(model, inter, n_cols, n0, u, items, distance=False, predict_extra=0.0, seed=0):
    """Both routes within their fp64 bound of the exact scores of the exact operands, hence within the sum of the two of each other.
    ``predict_extra``: roundings the predict route adds on the score itself, in units of U32 |x|."""
    from recbole_cdr_amd.model.crossdomain_recommender import CrossDomainRecommender
    indptr, cols, _, _ = _ragged(N_USERS, n_cols, max(n0, 1), seed=seed, max_rand=80)
    assert type(model).candidate_scores is not CrossDomainRecommender.candidate_scores
    native = model.candidate_scores(inter, indptr, cols, 4096)
    base = CrossDomainRecommender.candidate_scores(model, inter, indptr, cols, 1000)                 # predict, in chunks of 1,000 pairs
    assert native.shape == base.shape == cols.shape and native.dtype == torch.float32
    want = _ev_scores(u, items, indptr, cols, distance)
    e_native, e_base = want.e, want.e + predict_extra * U32 * want.mag
    r_native = ((native.double() - want.v).abs() / e_native).max()
    r_base = ((base.double() - want.v).abs() / e_base).max()
    r_both = ((native.double() - base.double()).abs() / (e_native + e_base)).max()
    print(f'{type(model).__name__} {getattr(model, "phase", "")} {getattr(model, "mode", "")}: error / bound native {float(r_native):.3f} '
          f'predict {float(r_base):.3f} native - predict {float(r_both):.3f}')
    assert float(r_native) <= 1.0 and float(r_base) <= 1.0 and float(r_both) <= 1.0
    assert bool((native != 0).any())


@pytest.mark.parametrize('mode', ['overlap_users', 'overlap_items'])
@pytest.mark.parametrize('phase', ['SOURCE', 'TARGET', 'OVERLAP'])
def test_emcdr_native_candidate_scores_agree_with_predict(phase, mode):
    _native_vs_predict(*_emcdr_case(phase, mode))


def test_dcdcsr_native_candidate_scores_agree_with_predict():
    from recbole_cdr_amd.model.cross_domain_recommender.dcdcsr import DCDCSR
    ids = _ids('overlap_users')
    cfg = base_config(DEV, latent_factor_model='BPR', embedding_size=64, mlp_hidden_size=[48], k=4, map_batch_size=32)
    torch.manual_seed(19)
    model = DCDCSR(cfg, _dataset(ids)).to(DEV)
    model.set_phase('TARGET')
    model.eval()
    inter = _users(model, ids)
    u = EV(model.target_user_embedding.weight.detach().double()[inter[model.TARGET_USER_ID]])
    items = EV(model.target_item_embedding.weight.detach().double()[:ids.target_num_items])
    _native_vs_predict(model, inter, ids.target_num_items, ids.OI, u, items)


def _bitgcf_model(n_layers=2):
    """(the scored rows are (n_layers + 1) x 32 wide: the layers' outputs, concatenated)"""
    from recbole_cdr_amd.model.cross_domain_recommender.bitgcf import BiTGCF
    ids = _ids('overlap_users')
    cfg = base_config(DEV, embedding_size=32, n_layers=n_layers, reg_weight=1e-3, lambda_source=0.8, lambda_target=0.7, drop_rate=0.0,
                      connect_way='concat')
    torch.manual_seed(23)
    model = BiTGCF(cfg, _dataset(ids)).to(DEV)
    model.eval()
    return ids, model


def test_bitgcf_native_candidate_scores_agree_with_predict():
    ids, model = _bitgcf_model()
    inter = _users(model, ids)
    with torch.no_grad():
        _, _, tu, ti = model.forward()
        _, _, tu2, ti2 = model.forward()
    # both routes read the propagation's output: it is the same bits on every call, so it is the exact operand of both
    assert torch.equal(tu, tu2) and torch.equal(ti, ti2)
    u, items = EV(tu.double()[inter[model.TARGET_USER_ID]]), EV(ti.double()[:ids.target_num_items])
    _native_vs_predict(model, inter, ids.target_num_items, ids.OI, u, items)


@pytest.mark.parametrize('phase', ['TARGET', 'OVERLAP'])
def test_sscdr_native_candidate_scores_agree_with_predict(phase):
    from recbole_cdr_amd.model.cross_domain_recommender.sscdr import SSCDR
    from fp64_bounds import ev_where
    ids = _ids('overlap_users')
    cfg = base_config(DEV, embedding_size=64, margin=0.3, mlp_hidden_size=[48], **{'lambda': 0.5})
    torch.manual_seed(29)
    model = SSCDR(cfg, _dataset(ids)).to(DEV)
    with torch.no_grad():                            # rows longer than 1: the normalisation divides
        for n, p in model.named_parameters():
            if n.endswith('embedding.weight'):
                p.mul_(4.0)
    model.set_phase(phase)
    model.eval()
    inter = _users(model, ids)
    users = inter[model.TARGET_USER_ID]
    tab = lambda name: getattr(model, name).weight.detach().double()
    u = EV(tab('target_user_embedding')[users])
    if phase == 'OVERLAP':
        layers = [(m.weight, m.bias, True) for m in model.mapping_layer.mlp_layers if isinstance(m, torch.nn.Linear)]
        u = ev_where((users < ids.OU).unsqueeze(1), _ev_mlp(EV(tab('source_user_embedding')[users]), layers), u)
    u, items = _ev_sqnorm_normalize(u), _ev_sqnorm_normalize(EV(tab('target_item_embedding')[:ids.target_num_items]))
    # predict takes the square root of the sum and squares it again (the triplet kernel's distance): sqrtf within one ulp (2 U32), doubled
    # by the square, the product's own rounding, one more for the kernel's float sum handed over: 6 U32 |x|
    _native_vs_predict(model, inter, ids.target_num_items, ids.OI, u, items, distance=True, predict_extra=6.0)
    # inside the evaluation bracket the item operand is the cached normalised buffer: the same bits
    indptr, cols, _, _ = _ragged(N_USERS, ids.target_num_items, 1, seed=4, max_rand=80)
    outside = model.candidate_scores(inter, indptr, cols)
    model.freeze_for_eval()
    try:
        assert torch.equal(model.candidate_scores(inter, indptr, cols), outside) and model._eval_item_cache() is not None
    finally:
        model.unfreeze_eval()


def _default_route_model(name, cmf_width=16):
    ids = _ids('overlap_users')
    torch.manual_seed(37)
    if name == 'CLFM':
        from recbole_cdr_amd.model.cross_domain_recommender.clfm import CLFM
        model = CLFM(base_config(DEV, user_embedding_size=48, source_item_embedding_size=64, target_item_embedding_size=64,
                                 share_embedding_size=24, alpha=0.3, reg_weight=0.01), FakeDataset(ids)).to(DEV)
    elif name == 'CMF':
        from recbole_cdr_amd.model.cross_domain_recommender.cmf import CMF
        model = CMF(base_config(DEV, embedding_size=cmf_width, alpha=0.3, **{'lambda': 0.02, 'gamma': 0.05}), FakeDataset(ids)).to(DEV)
    elif name == 'CoNet':
        from recbole_cdr_amd.model.cross_domain_recommender.conet import CoNet
        model = CoNet(base_config(DEV, embedding_size=16, reg_weight=0.01, mlp_hidden_size=[64, 32, 16, 8]), FakeDataset(ids)).to(DEV)
    elif name == 'DTCDR':
        from recbole_cdr_amd.model.cross_domain_recommender.dtcdr import DTCDR
        model = DTCDR(base_config(DEV, embedding_size=16, mlp_hidden_size=[32, 16], dropout_prob=0.1, base_model='NeuMF', alpha=0.3),
                      FakeDataset(ids)).to(DEV)
    elif name == 'DeepAPF':
        from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
        model = DeepAPF(base_config(DEV, embedding_size=16, beta=0.5), FakeDataset(ids)).to(DEV)
        model.set_phase('TARGET')
    else:
        from oracle.common import IdSpace
        from recbole_cdr_amd.model.cross_domain_recommender.natr import NATR
        ids = IdSpace(OU=1, TOU=70, SOU=22, OI=18, TOI=483, SOI=16)
        rng = np.random.RandomState(4)
        tu, ti = np.arange(1, ids.target_num_users), np.arange(1, ids.target_num_items)
        su = np.arange(ids.OU + ids.TOU, ids.total_num_users)
        si = np.concatenate([np.arange(1, ids.OI), np.arange(ids.OI + ids.TOI, ids.total_num_items)])
        ds = FakeDataset(ids, np.unique(np.stack([rng.choice(su, 300), rng.choice(si, 300)], 1), axis=0),
                         np.unique(np.stack([rng.choice(tu, 900), rng.choice(ti, 900)], 1), axis=0))
        ds.device = DEV
        model = NATR(base_config(DEV, source_embedding_size=16, target_embedding_size=24, reg_weight=1e-3, max_inter_length=6), ds).to(DEV)
        model.set_phase('TARGET')
    model.eval()
    return ids, model


@pytest.mark.parametrize('name', ['CLFM', 'CMF', 'CoNet', 'DTCDR', 'DeepAPF', 'NATR'])
def test_default_route_models_score_candidates_through_predict(name):
    """These keep the base class's route -- CLFM and CMF because their ``predict`` applies a sigmoid, the others because their score is
    no contraction of two rows: [C] finite scores, the values of one ``predict`` call over the expanded pairs."""
    from recbole_cdr_amd.model.crossdomain_recommender import CrossDomainRecommender
    ids, model = _default_route_model(name)
    assert type(model).candidate_scores is CrossDomainRecommender.candidate_scores
    inter = _users(model, ids)
    indptr, cols, _, _ = _ragged(N_USERS, ids.target_num_items, max(ids.OI, 1), seed=6, max_rand=40)
    frozen = hasattr(model, 'freeze_for_eval')
    if frozen:
        model.freeze_for_eval()
    try:
        got = model.candidate_scores(inter, indptr, cols, 700)
        rows = torch.repeat_interleave(torch.arange(N_USERS, device=DEV), indptr[1:] - indptr[:-1])
        pairs = inter.index_select(rows)
        pairs.update({model.TARGET_ITEM_ID: cols})
        whole = model.predict(pairs).reshape(-1).float()
    finally:
        if frozen:
            model.unfreeze_eval()
    assert got.shape == cols.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert torch.allclose(got, whole, rtol=1e-5, atol=1e-6)                   # (the chunk size may change a tower's kernel, not its value)
    if name in ('CLFM', 'CMF'):
        assert float(got.min()) > 0.0 and float(got.max()) < 1.0               # probabilities: the sigmoid is part of what is ranked
    model.__dict__['_dist_cfg'] = True
    with pytest.raises(NotImplementedError, match='one GPU'):
        model.candidate_scores(inter, indptr, cols, 700)


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------
def _e2e_ids():
    from oracle.common import IdSpace
    return IdSpace(OU=200, TOU=150, SOU=35, OI=1, TOI=1499, SOI=70)


def _e2e_dataset(ids, seed=0):
    rng = np.random.RandomState(seed)
    src_u = np.array(list(range(1, ids.OU)) + list(range(ids.OU + ids.TOU, ids.total_num_users)))
    src_i = np.arange(ids.OI + ids.TOI, ids.total_num_items)
    tgt_u, tgt_i = np.arange(1, ids.OU + ids.TOU), np.arange(1, ids.OI + ids.TOI)
    s_pairs = np.unique(np.stack([rng.choice(src_u, 900), rng.choice(src_i, 900)], 1), axis=0).astype(np.int64)
    t_pairs = np.unique(np.stack([rng.choice(tgt_u, 900), rng.choice(tgt_i, 900)], 1), axis=0).astype(np.int64)
    return FakeDataset(ids, s_pairs, t_pairs)


def _e2e(mode, **kw):
    from recbole_cdr_amd.data.dataloader import eval_loader_for
    from recbole_cdr_amd.model.cross_domain_recommender.emcdr import EMCDR
    ids = _e2e_ids()
    ds = _e2e_dataset(ids)
    cfg = base_config(DEV, latent_factor_model='BPR', source_embedding_size=64, target_embedding_size=64, reg_weight=0.01,
                      mapping_function='linear', mlp_hidden_size=[24], eval_args={'mode': mode}, **kw)
    torch.manual_seed(11)
    model = EMCDR(cfg, ds).to(DEV)
    model.set_phase('TARGET')
    rng = np.random.RandomState(7)
    users = np.arange(1, ids.OU + ids.TOU)
    taken = set(map(tuple, ds.t_pairs.tolist()))
    ev = np.stack([np.repeat(users, 3), rng.randint(1, ids.target_num_items, 3 * users.size)], 1)
    ev = np.array([p for p in np.unique(ev, axis=0).tolist() if tuple(p) not in taken], dtype=np.int64)
    loader = eval_loader_for(cfg, 'target', ds, 'target_user_id', 'target_item_id', ev, ds.t_pairs, DEV, users_per_batch=128, resample=False)
    return ids, ds, cfg, model, ev, loader


def _brute_metrics(model, loader, n_items, topk, names):
    """fp64 formulas on a stable descending sort of the reference formulation, from the loader's own candidates and the model's
    candidate_scores bits"""
    kmax = max(topk)
    per = {f'{n}@{k}': [] for n in names for k in topk}
    num = den = 0.0
    model.eval()
    for inter, (indptr, cols), pu, pi in loader:
        scores = model.candidate_scores(inter, indptr, cols, 4096)
        U = len(inter)
        rows = torch.repeat_interleave(torch.arange(U, device=DEV), indptr[1:] - indptr[:-1])
        full = torch.full((U, n_items), -float('inf'), device=DEV, dtype=torch.float32)
        full[rows, cols] = scores
        order = torch.sort(full, dim=1, descending=True, stable=True).indices[:, :kmax].cpu().numpy()       # ties: the smaller column first
        full = full.double().cpu()
        pu, pi = pu.cpu(), pi.cpu()
        for u in range(U):
            pos = pi[pu == u].tolist()
            hit = np.array([c in pos for c in order[u]], dtype=np.float64)
            for k in topk:
                h = hit[:k]
                disc = 1.0 / np.log2(np.arange(2, k + 2))
                vals = {'recall': h.sum() / max(len(pos), 1), 'ndcg': (h * disc).sum() / disc[:max(min(len(pos), k), 1)].sum(),
                        'map': (np.cumsum(h) / np.arange(1, k + 1) * h).sum() / max(min(len(pos), k), 1)}
                for n in names:
                    per[f'{n}@{k}'].append(vals[n])
            cand = cols[int(indptr[u]):int(indptr[u + 1])].tolist()
            negs = [c for c in cand if c not in pos]
            if pos and negs:
                sp, sn = full[u, pos].unsqueeze(1), full[u, negs].unsqueeze(0)
                num += float((sp > sn).sum() + 0.5 * (sp == sn).sum()) / len(negs)
                den += len(pos)
    out = {key: float(np.mean(v)) for key, v in per.items()}
    out['gauc'] = num / den
    return out


@pytest.mark.parametrize('mode', ['uni20', 'pop20'])
def test_evaluate_over_a_sampled_loader_equals_brute_force(mode):
    """The trainer's values are fp32 means of <= 349 per-user values in [0, 1] formed with a handful of fp32 operations each: within 2e-6 of
    the fp64 formulas (the bound tests/test_gpu_eval_metrics.py uses for the same arithmetic); GAUC is computed in fp64: 1e-12."""
    from recbole_cdr_amd.data.dataloader import NegSampleEvalLoader
    from recbole_cdr_amd.trainer.trainer import Trainer
    ids, ds, cfg, model, ev, loader = _e2e(mode, metrics=['Recall', 'NDCG', 'MAP', 'GAUC'], topk=[5, 100])
    assert isinstance(loader, NegSampleEvalLoader) and loader.sample_by == 20
    assert loader.sampler.distribution == ('uniform' if mode == 'uni20' else 'popularity')
    tr = Trainer(cfg, model)
    assert tr.eval_mode == ('by', 20, loader.sampler.distribution)
    got = tr.evaluate(loader)
    assert loader.draws == 1 and loader.step == 128                                       # (the caller's cut came back)
    want = _brute_metrics(model, loader, ids.target_num_items, [5, 100], ('recall', 'ndcg', 'map'))
    assert loader.draws == 1                                                              # resample=False: the same candidates
    assert set(got) == set(want) == {'recall@5', 'recall@100', 'ndcg@5', 'ndcg@100', 'map@5', 'map@100', 'gauc'}
    print(mode, got)
    assert abs(got['gauc'] - want['gauc']) <= 1e-12, (got['gauc'], want['gauc'])
    for key in want:
        assert abs(got[key] - want[key]) <= 2e-6, (key, got[key], want[key])
    assert got['recall@100'] == 1.0 and 0.0 < got['recall@5'] < 1.0                       # every list is shorter than 100
    # the sampler's properties, on the loader's own draw
    gptr, gcols = loader._cand
    rows = torch.repeat_interleave(torch.arange(loader.users.size, device=DEV), gptr[1:] - gptr[:-1])
    users = torch.from_numpy(loader.users).to(DEV)[rows]
    N = ids.total_num_items
    key = users * N + gcols
    is_pos = torch.isin(key, torch.from_numpy(ev[:, 0] * N + ev[:, 1]).to(DEV))
    assert int(is_pos.sum()) == len(ev)                                                   # the positives are candidates
    neg, neg_key = gcols[~is_pos], key[~is_pos]
    assert int(neg.min()) >= 1 and int(neg.max()) < ids.target_num_items                  # never PAD, never outside the target range
    assert not bool(torch.isin(neg_key, torch.from_numpy(ds.t_pairs[:, 0] * N + ds.t_pairs[:, 1]).to(DEV)).any())      # never a used item
    n_pos = torch.bincount(loader._rank, minlength=loader.users.size)
    assert bool(((gptr[1:] - gptr[:-1]) <= n_pos * 21).all()) and bool(((gptr[1:] - gptr[:-1]) > n_pos * 15).all())


def test_full_mode_gives_the_full_sort_loader_and_source_is_always_full_sort():
    from recbole_cdr_amd.data.dataloader import FullSortEvalLoader, eval_loader_for
    ids = _e2e_ids()
    ds = _e2e_dataset(ids)
    ev = np.array([[1, 5], [2, 7]])
    for cfg in ({'device': DEV}, {'device': DEV, 'eval_args': {'mode': 'full'}}):
        assert type(eval_loader_for(cfg, 'target', ds, 'target_user_id', 'target_item_id', ev, ds.t_pairs, DEV)) is FullSortEvalLoader
    src = eval_loader_for({'device': DEV, 'eval_args': {'mode': 'uni20'}}, 'source', ds, 'source_user_id', 'source_item_id',
                          ds.s_pairs[:5], ds.s_pairs[5:], DEV)
    assert type(src) is FullSortEvalLoader and getattr(src, 'eval_mode', 'full') == 'full'


def test_valid_metric_over_a_sampled_loader_and_a_mixed_pair_of_loaders():
    """``valid_metric: 'ndcg@5'`` drives early stopping over a sampled valid loader for two epochs; a (source full-sort, target sampled)
    pair of valid loaders evaluates each its own way."""
    from recbole_cdr_amd.data.dataloader import eval_loader_for
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    from recbole_cdr_amd.utils import InputType
    from test_gpu_trainer_graph import _loaders
    ids, ds, cfg, model, ev, loader = _e2e('uni20', learning_rate=0.01, train_modes=['TARGET'], epoch_num=['2'], source_split=False,
                                           eval_step=1, epochs=2, metrics=['NDCG'], valid_metric='ndcg@5', topk=[5])
    dl = _loaders(ids, ds, ds.s_pairs, ds.t_pairs, InputType.PAIRWISE, 64, 1)
    seen = []
    trainer = CrossDomainTrainer(cfg, model)
    best, result = trainer.fit(dl, valid_data=loader, callback_fn=lambda epoch, score: seen.append(score))
    assert len(seen) == 2 and set(result) == {'ndcg@5'} and best == result['ndcg@5'] == max(seen) and 0.0 < best < 1.0
    assert loader.draws == 1
    # source full-sort + target sampled
    cfg2 = dict(cfg, train_modes=['SOURCE', 'TARGET'], epoch_num=['1', '1'], source_split=True, epochs=1)
    torch.manual_seed(11)
    model2 = type(model)(cfg2, ds).to(DEV)
    src = eval_loader_for(cfg2, 'source', ds, 'source_user_id', 'source_item_id', ds.s_pairs[::7], np.delete(ds.s_pairs, np.s_[::7], axis=0), DEV)
    seen2 = []
    trainer2 = CrossDomainTrainer(cfg2, model2)
    trainer2.fit(_loaders(ids, ds, ds.s_pairs, ds.t_pairs, InputType.PAIRWISE, 64, 1), valid_data=(src, loader),
                 callback_fn=lambda epoch, score: seen2.append(score))
    assert len(seen2) == 2 and all(0.0 <= s <= 1.0 for s in seen2)
