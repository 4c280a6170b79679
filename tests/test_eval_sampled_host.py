"""Host-side checks (no GPU) of sampled-candidate evaluation (eval_args mode uniN / popN): ``resolve_eval_mode``, the
``NegSampleEvalLoader`` on the CPU with a sampler that returns planted items, and a ``device: cpu`` trainer on a hand-made example against
the test's own fp64 formulas over the reference's formulation (a row of -inf over the catalogue with the candidates' scores scattered in)."""
import numpy as np
import pytest
import torch

NEG_INF = -float('inf')


# ---- 1. the setting ------------------------------------------------------------------------------------------------------------------
def test_resolve_eval_mode():
    from recbole_cdr_amd.trainer.trainer import Trainer, resolve_eval_mode
    assert resolve_eval_mode({}) == ('full', None, 'uniform')
    assert resolve_eval_mode({'eval_args': None}) == ('full', None, 'uniform')
    assert resolve_eval_mode({'eval_args': {'split': {'RS': [8, 1, 1]}}}) == ('full', None, 'uniform')
    assert resolve_eval_mode({'eval_args': {'mode': 'full'}}) == ('full', None, 'uniform')
    assert resolve_eval_mode({'eval_args': {'mode': 'uni100'}}) == ('by', 100, 'uniform')
    assert resolve_eval_mode({'eval_args': {'mode': 'pop7'}}) == ('by', 7, 'popularity')
    # recbole compares the mode's first three letters case-sensitively: 'Uni5' is not a mode
    for bad in ('Uni5', 'uni0', 'uni', 'top5', 'uni-3', 'uni1.5', 'pop', 'POP10', 'full5', 7):
        with pytest.raises(ValueError, match=r'the mode \[.*\] in eval_args is not supported\.'):
            resolve_eval_mode({'eval_args': {'mode': bad}})
    with pytest.raises(ValueError, match='labeled evaluation and the value metrics'):
        resolve_eval_mode({'eval_args': {'mode': 'labeled'}})
    model = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match='labeled'):
        Trainer({'device': 'cpu', 'eval_args': {'mode': 'labeled'}}, model)
    with pytest.raises(ValueError, match='not supported'):
        Trainer({'device': 'cpu', 'eval_args': {'mode': 'Uni5'}}, model)
    assert Trainer({'device': 'cpu', 'eval_args': {'mode': 'pop20'}}, model).eval_mode == ('by', 20, 'popularity')
    assert Trainer({'device': 'cpu'}, model).eval_mode == ('full', None, 'uniform')


# ---- 2. the loader -------------------------------------------------------------------------------------------------------------------
# users 3, 5, 9; sample_by = 3.  user 3 draws item 30 twice for one positive; item 30 is also drawn for user 5.
PLANTS = {(3, 10): [30, 31, 30], (3, 20): [32, 33, 34], (5, 11): [30, 40, 41], (9, 12): [50, 51, 52], (9, 13): [53, 54, 55],
          (9, 14): [56, 57, 58]}
EVAL_PAIRS = np.array([[9, 13], [3, 20], [5, 11], [3, 10], [9, 12], [9, 14], [3, 20]])           # unsorted, one pair twice
WANT = {3: ([10, 20, 30, 31, 32, 33, 34], [10, 20]), 5: ([11, 30, 40, 41], [11]), 9: (list(range(12, 15)) + list(range(50, 59)), [12, 13, 14])}


class PlantedSampler:
    """k-major [P * k]: negative j of positive p at j * P + p.  Every call after the first shifts the items by 100 per call."""

    def __init__(self):
        self.calls = 0

    def __call__(self, users, items, k):
        shift = 100 * self.calls
        self.calls += 1
        P = users.numel()
        out = torch.empty(P * k, dtype=torch.int64)
        for p, (u, i) in enumerate(zip(users.tolist(), items.tolist())):
            for j in range(k):
                out[j * P + p] = PLANTS[(u, i)][j] + shift
        return out


def _loader(**kw):
    from recbole_cdr_amd.data.dataloader import NegSampleEvalLoader
    kw.setdefault('eval_batch_size', 4096)
    return NegSampleEvalLoader('uid', 'iid', EVAL_PAIRS, PlantedSampler(), 3, device='cpu', **kw)


def _per_user(loader):
    out = {}
    for inter, (indptr, cols), pu, pi in loader:
        users = inter['uid'].tolist()
        assert indptr.numel() == len(users) + 1 and int(indptr[0]) == 0 and int(indptr[-1]) == cols.numel()
        for r, u in enumerate(users):
            assert u not in out
            out[u] = (cols[int(indptr[r]):int(indptr[r + 1])].tolist(), sorted(pi[pu == r].tolist()))
    return out


def test_loader_candidates_are_a_csr_of_distinct_ascending_items():
    loader = _loader()
    assert loader.eval_mode == 'sampled' and loader.users.tolist() == [3, 5, 9]
    got = _per_user(loader)
    assert got == WANT
    for u, (cands, pos) in got.items():
        assert cands == sorted(set(cands))                               # ascending and distinct per user
        assert set(pos) <= set(cands)                                    # the positives are among the candidates
        assert len(cands) <= len(pos) * (1 + 3)
    assert len(got[3][0]) < 2 * (1 + 3)                                  # the repeated draw collapsed to one column
    assert len(got[5][0]) == 1 * (1 + 3) and 30 in got[5][0] and 30 in got[3][0]      # one item, two users: kept for both


def test_loader_expand_round_trips():
    loader = _loader(users_per_batch=2, resample=False)
    for batch in loader:
        inter, (indptr, cols), pu, pi = batch
        pairs, row_idx, pu2, pi2 = loader.expand(batch)
        assert len(pairs) == cols.numel() == row_idx.numel()
        assert torch.equal(pairs['iid'], cols) and torch.equal(pairs['uid'], inter['uid'][row_idx])
        assert torch.equal(pu2, pu) and torch.equal(pi2, pi)
        back = torch.zeros(len(inter) + 1, dtype=torch.int64)
        back[1:] = torch.cumsum(torch.bincount(row_idx, minlength=len(inter)), 0)
        assert torch.equal(back, indptr)


def test_loader_batch_cut():
    from recbole_cdr_amd.data.dataloader import NegSampleEvalLoader
    step = NegSampleEvalLoader.recbole_step
    # pairs per user 8, 4, 12 -> descending 12, 8, 4
    assert step([8, 4, 12], 11) == 1                                     # at least one, even when the largest does not fit
    assert step([8, 4, 12], 19) == 1 and step([8, 4, 12], 20) == 2 and step([8, 4, 12], 23) == 2 and step([8, 4, 12], 24) == 3
    assert step([8, 4, 12], 1 << 20) == 3 and step([50], 10) == 1
    assert _loader(eval_batch_size=16).step == 1 and len(_loader(eval_batch_size=16)) == 3
    assert _loader(eval_batch_size=20).step == 2 and len(_loader(eval_batch_size=20)) == 2
    assert _loader(eval_batch_size=16, users_per_batch=3).step == 3
    # the cut changes no user's content
    loader = _loader(resample=False)
    for n in (1, 2, 3, 7):
        assert loader.rebatch(n) is loader and loader.step == n and len(loader) == -(-3 // n)
        assert _per_user(loader) == WANT
    assert loader.sampler.calls == 1


def test_loader_resample():
    keep = _loader(resample=False)
    assert _per_user(keep) == WANT and _per_user(keep) == WANT and keep.sampler.calls == 1 and keep.draws == 1
    again = _loader(resample=True)
    first, second = _per_user(again), _per_user(again)
    assert again.sampler.calls == 2 and first == WANT
    assert second[5] == ([11, 130, 140, 141], [11])                      # a new draw: the planted items of the second call


# ---- 3. a device: cpu trainer on a hand-made example -----------------------------------------------------------------------------------
N_ITEMS = 40
# user row -> (candidate columns, positives): about 12 candidates each; row 2 has no positive
EXAMPLE = [
    ([1, 3, 4, 7, 9, 12, 15, 20, 22, 30, 33, 39], [4, 22]),
    ([2, 3, 5, 8, 11, 13, 17, 19, 23, 29, 31], [2, 19, 31]),
    ([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], []),
    ([6, 10, 14, 18, 21, 24, 26, 27, 28, 34, 35, 36, 38], [38]),
]


class _Inter(dict):
    def to(self, dev):
        return self

    def __len__(self):
        return int(self['target_user_id'].numel())

    def index_select(self, idx):
        return _Inter({k: v[idx] for k, v in self.items()})

    def __getitem__(self, key):
        return dict.__getitem__(self, key) if isinstance(key, str) else _Inter({k: v[key] for k, v in self.items()})


class _Batches(list):
    eval_mode = 'sampled'


def _stub_model():
    from recbole_cdr_amd.model.crossdomain_recommender import CrossDomainRecommender

    class Stub(torch.nn.Module):
        TARGET_ITEM_ID = 'target_item_id'
        candidate_scores = CrossDomainRecommender.candidate_scores          # the default route: predict on the expanded pairs
        _candidate_guard = CrossDomainRecommender._candidate_guard

        def __init__(self):
            super().__init__()
            g = torch.Generator(); g.manual_seed(5)
            self.w = torch.nn.Parameter(torch.randn(4, 6, generator=g))
            self.items = torch.randn(N_ITEMS, 6, generator=g)
            self.predict_calls = 0

        def table(self):
            return torch.round((self.w @ self.items.t()).detach() * 2) / 2                          # steps of 0.5: exact ties

        def predict(self, inter):
            self.predict_calls += 1
            return self.table()[inter['target_user_id'], inter['target_item_id']]

    return Stub()


def _example_batches(cut):
    out = _Batches()
    for lo in range(0, len(EXAMPLE), cut):
        rows = EXAMPLE[lo:lo + cut]
        indptr = torch.tensor([0] + list(np.cumsum([len(c) for c, _ in rows])), dtype=torch.int64)
        cols = torch.tensor([c for cs, _ in rows for c in cs], dtype=torch.int64)
        pu = torch.tensor([r for r, (_, ps) in enumerate(rows) for _ in ps], dtype=torch.int64)
        pi = torch.tensor([p for _, ps in rows for p in ps], dtype=torch.int64)
        out.append((_Inter({'target_user_id': torch.arange(lo, lo + len(rows))}), (indptr, cols), pu, pi))
    return out


def _own_metrics(table, topk):
    """fp64 formulas on a stable descending sort of the reference formulation: a row of -inf over the catalogue, the candidates' scores
    scattered in, ties to the smaller column"""
    kmax = max(topk)
    per = {}
    num = den = 0.0
    for u, (cands, pos) in enumerate(EXAMPLE):
        row = torch.full((N_ITEMS,), NEG_INF, dtype=torch.float64)
        row[cands] = table[u, cands].double()
        order = torch.sort(row, descending=True, stable=True).indices.tolist()[:kmax]
        hit = np.array([c in pos for c in order], dtype=np.float64)
        for k in topk:
            h = hit[:k]
            disc = 1.0 / np.log2(np.arange(2, k + 2))
            vals = {'recall': h.sum() / max(len(pos), 1), 'hit': float(h.sum() > 0), 'precision': h.sum() / k,
                    'mrr': (1.0 / (1 + int(np.argmax(h)))) if h.any() else 0.0,
                    'ndcg': (h * disc).sum() / disc[:max(min(len(pos), k), 1)].sum(),
                    'map': (np.cumsum(h) / np.arange(1, k + 1) * h).sum() / max(min(len(pos), k), 1)}
            for n, v in vals.items():
                per.setdefault(f'{n}@{k}', []).append(v)
        negs = [c for c in cands if c not in pos]
        if pos and negs:
            sp, sn = row[pos].unsqueeze(1), row[negs].unsqueeze(0)
            num += float((sp > sn).sum() + 0.5 * (sp == sn).sum()) / len(negs)
            den += len(pos)
    out = {key: float(np.mean(v)) for key, v in per.items()}
    out['gauc'] = num / den
    return out


@pytest.mark.parametrize('cut', [4, 3, 1])
def test_cpu_trainer_on_a_hand_made_example(cut):
    from recbole_cdr_amd.trainer.trainer import Trainer
    names = ['Recall', 'NDCG', 'MRR', 'Hit', 'Precision', 'MAP', 'GAUC']
    model = _stub_model()
    table = model.table()
    # the example has what it is for: exact ties between a positive and other candidates, and every list shorter than kmax = 20
    tied = 0
    for u, (cands, pos) in enumerate(EXAMPLE):
        assert len(cands) < 20
        for p in pos:
            tied += int((table[u, cands] == table[u, p]).sum()) - 1
    assert tied >= 2
    tr = Trainer({'device': 'cpu', 'metrics': names, 'topk': [1, 3, 20], 'eval_batch_size': 7, 'eval_args': {'mode': 'uni11'}}, model)
    got = tr.evaluate(_example_batches(cut))
    want = _own_metrics(table, [1, 3, 20])
    assert set(got) == set(want) and len(got) == 6 * 3 + 1
    assert model.predict_calls == sum(-(-sum(len(c) for c, _ in EXAMPLE[lo:lo + cut]) // 7) for lo in range(0, 4, cut))     # chunks of 7 pairs
    assert abs(got['gauc'] - want['gauc']) < 1e-12, (got['gauc'], want['gauc'])
    for key in want:
        assert abs(got[key] - want[key]) < 1e-6, (key, got[key], want[key])
    assert got['recall@20'] == pytest.approx(0.75) and got['precision@20'] < got['precision@3']          # the -inf tail holds no hit


def test_cpu_trainer_refuses_a_positive_outside_its_candidates():
    from recbole_cdr_amd.trainer.trainer import Trainer
    batches = _example_batches(4)
    inter, cand, pu, pi = batches[0]
    batches[0] = (inter, cand, torch.cat([pu, torch.tensor([2])]), torch.cat([pi, torch.tensor([25])]))      # 25 is not a candidate of row 2
    with pytest.raises(ValueError, match='does not rank such a positive'):
        Trainer({'device': 'cpu', 'topk': [3]}, _stub_model()).evaluate(batches)


def test_candidate_rank_reference_counts():
    """the plain-torch restatement on a tiny list with a NaN candidate, a NaN positive and an absent positive"""
    from recbole_cdr_amd.functional import candidate_rank_reference
    nan = float('nan')
    indptr = torch.tensor([0, 5, 5, 8])
    cols = torch.tensor([2, 4, 6, 7, 9, 1, 3, 5])
    scores = torch.tensor([1.0, 2.0, 1.0, nan, 1.0, nan, 0.5, 0.5])
    pindptr = torch.tensor([0, 2, 2, 5])
    pcols = torch.tensor([6, 8, 1, 3, 5])
    t, gt, eq, eqb, n = candidate_rank_reference(indptr, cols, scores, pindptr, pcols)
    assert gt.tolist() == [1, -1, -1, 0, 0] and eq.tolist() == [3, -1, -1, 2, 2] and eqb.tolist() == [1, -1, -1, 0, 1]
    assert n.tolist() == [4, 0, 2] and n.dtype == gt.dtype == torch.int32
    assert t[0] == 1.0 and torch.isnan(t[1]) and torch.isnan(t[2]) and t[3] == 0.5
