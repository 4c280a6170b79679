"""Host-side checks (no GPU) of the evaluation settings: ``metrics_from_hits`` and the GAUC arithmetic on a hand-worked example, a
``device: cpu`` trainer with MAP and GAUC at a ``topk`` above 64, the refusals of ``config['metrics']`` / ``config['eval_route']``, and the
declarations of the rank entries (header, binding, ABI version)."""
import os
import re
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_ENTRIES = ('cdr_fullsort_rank_workspace_bytes', 'cdr_fullsort_rank_f32', 'cdr_fullsort_neg_sqdist_rank_workspace_bytes',
                'cdr_fullsort_neg_sqdist_rank_f32', 'cdr_rank_rows_f32')


def test_metrics_from_hits_and_gauc_on_a_hand_worked_example():
    """Three users, kmax = 4.
    user 0: 2 positives at list positions 1 and 3     user 1: 1 positive at position 2     user 2: 3 positives, one at position 4.
    map@k = (sum of precision@j over the hit positions j <= k) / min(n_pos, k), averaged over the users."""
    from recbole_cdr_amd.trainer.trainer import metrics_from_hits, gauc_from_counts
    hit = torch.tensor([[1., 0., 1., 0.], [0., 1., 0., 0.], [0., 0., 0., 1.]])
    n_pos = torch.tensor([2., 1., 3.])
    got = metrics_from_hits(hit, n_pos, [2, 4], ('recall', 'hit', 'precision', 'mrr', 'ndcg', 'map'))
    l2 = lambda x: float(np.log2(x))
    want = {
        'recall@2': (Fr(1, 2) + 1 + 0) / 3, 'recall@4': (1 + 1 + Fr(1, 3)) / 3,
        'hit@2': Fr(2, 3), 'hit@4': Fr(1),
        'precision@2': (Fr(1, 2) + Fr(1, 2) + 0) / 3, 'precision@4': (Fr(2, 4) + Fr(1, 4) + Fr(1, 4)) / 3,
        'mrr@2': (1 + Fr(1, 2) + 0) / 3, 'mrr@4': (1 + Fr(1, 2) + Fr(1, 4)) / 3,
        # user 0 @2: P@1 = 1 -> 1 / min(2, 2);  user 1 @2: P@2 = 1/2 -> (1/2) / 1;  user 2 @2: nothing
        'map@2': (Fr(1, 2) + Fr(1, 2) + 0) / 3,
        # user 0 @4: (P@1 + P@3) / 2 = (1 + 2/3) / 2;  user 1: (1/2) / 1;  user 2: P@4 / min(3, 4) = (1/4) / 3
        'map@4': (Fr(5, 6) + Fr(1, 2) + Fr(1, 12)) / 3,
    }
    for key, val in want.items():
        assert abs(got[key] - float(val)) < 1e-6, (key, got[key], float(val))
    ndcg2 = (1.0 / (1 + 1 / l2(3)) + (1 / l2(3)) / 1.0 + 0.0) / 3
    ndcg4 = ((1 + 1 / l2(4)) / (1 + 1 / l2(3)) + (1 / l2(3)) / 1.0 + (1 / l2(5)) / (1 + 1 / l2(3) + 1 / l2(4))) / 3
    assert abs(got['ndcg@2'] - ndcg2) < 1e-6 and abs(got['ndcg@4'] - ndcg4) < 1e-6
    assert set(got) == set(want) | {'ndcg@2', 'ndcg@4'}
    # the default names are what evaluate always returned
    assert set(metrics_from_hits(hit, n_pos, [2])) == {'recall@2', 'hit@2', 'precision@2', 'mrr@2', 'ndcg@2'}

    # GAUC.  user 0: 10 unmasked items, 2 positives: one alone at the top (gt = 0, eq = 1 -> rank 1), one tied with two negatives behind one
    #         better item (gt = 1, eq = 3 -> average rank 1 + (3 + 1) / 2 = 3).  pair = 11 * 2 - 3 - (1 + 3) = 15 of 8 * 2 -> 15/16.
    #         (pairwise: the top positive beats 8 negatives; the tied one loses to none (the better item is the other positive), ties with
    #          2 -> 6 + 2 / 2 = 7;  (8 + 7) / 16.)
    # user 1: 5 items, 1 positive at the bottom (gt = 4, eq = 1 -> rank 5): pair = 6 - 1 - 5 = 0 -> 0.
    # user 2: no positive -> dropped.   user 3: 3 items, all positives -> no negative -> dropped.
    gt = torch.tensor([0, 1, 4, 0, 1, 2])
    eq = torch.tensor([1, 3, 1, 1, 1, 1])
    rank = gt.double() + (eq.double() + 1) / 2
    assert rank.tolist() == [1.0, 3.0, 5.0, 1.0, 2.0, 3.0]
    prow = torch.tensor([0, 0, 1, 3, 3, 3])
    rank_sum = torch.zeros(4, dtype=torch.float64).index_add_(0, prow, rank)
    gauc = gauc_from_counts(torch.tensor([2, 1, 0, 3]), torch.tensor([10, 5, 7, 3]), rank_sum)
    assert abs(gauc - float((Fr(15, 16) * 2 + 0 * 1) / 3)) < 1e-15
    assert np.isnan(gauc_from_counts(torch.tensor([0]), torch.tensor([4]), torch.zeros(1, dtype=torch.float64)))


def _cpu_batches(n_users=40, n_items=150, seed=3):
    rng = np.random.RandomState(seed)
    batches = []
    for lo in range(0, n_users, 16):
        n = min(16, n_users - lo)
        hr = np.repeat(np.arange(n), 5); hc = rng.randint(1, n_items, hr.size)
        taken = set(zip(hr.tolist(), hc.tolist()))
        pu = np.repeat(np.arange(n), 4); pi = rng.randint(1, n_items, pu.size)
        pairs = np.unique(np.stack([pu, pi], 1), axis=0)
        pairs = np.array([p for p in pairs.tolist() if tuple(p) not in taken and p[0] != 2])        # row 2: a user without positives
        hist = (torch.from_numpy(hr), torch.from_numpy(hc)) if lo != 16 else None
        batches.append(({'lo': lo, 'n': n}, hist, torch.from_numpy(pairs[:, 0]), torch.from_numpy(pairs[:, 1])))
    return batches


def test_cpu_trainer_map_gauc_and_topk_above_64():
    """``device: cpu``, ``metrics: ['MAP', 'GAUC']``, ``topk: [3, 100]``: the keys are map@3, map@100 and gauc, and the values are those of
    a brute-force walk over the masked matrix (stable descending order for the lists, every (positive, negative) pair for GAUC).  Some scores
    are rounded so that ties occur."""
    from recbole_cdr_amd.trainer.trainer import Trainer
    n_items = 150

    class Inter(dict):
        def to(self, dev):
            return self

        def __len__(self):
            return self['n']

    class Stub(torch.nn.Module):
        target_num_items = n_items

        def __init__(self):
            super().__init__()
            g = torch.Generator(); g.manual_seed(0)
            self.w = torch.nn.Parameter(torch.randn(40, 8, generator=g))
            self.items = torch.randn(n_items, 8, generator=g)

        def scores(self, inter):
            return torch.round((self.w[inter['lo']:inter['lo'] + inter['n']] @ self.items.t()).detach() * 2) / 2      # steps of 0.5: ties

        def full_sort_predict(self, inter):
            return self.scores(inter).reshape(-1)

    batches = [(Inter(b[0]),) + b[1:] for b in _cpu_batches(n_items=n_items)]
    model = Stub()
    tr = Trainer({'device': 'cpu', 'metrics': ['MAP', 'GAUC'], 'topk': [3, 100], 'valid_metric': 'gauc'}, model)
    assert tr.metrics == ('map', 'gauc') and tr.eval_route == 'auto' and tr.valid_metric == 'gauc'
    got = tr.evaluate(batches)
    assert set(got) == {'map@3', 'map@100', 'gauc'}

    ap = {3: [], 100: []}
    num = den = 0.0
    for inter, hist, pu, pi in batches:
        s = model.scores(inter).double()
        s[:, 0] = -np.inf
        if hist is not None:
            s[hist] = -np.inf
        for u in range(inter['n']):
            pos = set(pi[pu == u].tolist())
            order = torch.sort(s[u], descending=True, stable=True).indices.tolist()            # ties: the smaller column first
            for k in ap:
                hits, acc = 0, 0.0
                for j, c in enumerate(order[:k]):
                    if c in pos:
                        hits += 1
                        acc += hits / (j + 1)
                ap[k].append(acc / max(min(len(pos), k), 1))
            negs = [c for c in range(n_items) if s[u, c] != -np.inf and c not in pos]
            if pos and negs:
                sp, sn = s[u, sorted(pos)].unsqueeze(1), s[u, negs].unsqueeze(0)
                num += float((sp > sn).sum() + 0.5 * (sp == sn).sum()) / len(negs)               # = auc_u * pos_len
                den += len(pos)
    assert abs(got['gauc'] - num / den) < 1e-12
    for k in ap:
        assert abs(got[f'map@{k}'] - float(np.mean(ap[k]))) < 1e-6

    # the rank route returns the default route's numbers where both can answer (no ties within the compared lists needed: both break them
    # towards the smaller column on this route pair -- torch.topk on the CPU is not specified to, so compare on a tie-free model)
    model.scores = lambda inter: (model.w[inter['lo']:inter['lo'] + inter['n']] @ model.items.t()).detach()
    a = Trainer({'device': 'cpu', 'topk': [5, 10]}, model).evaluate(batches)
    b = Trainer({'device': 'cpu', 'topk': [5, 10], 'eval_route': 'rank'}, model).evaluate(batches)
    assert set(a) == set(b) == {f'{m}@{k}' for m in ('recall', 'hit', 'precision', 'mrr', 'ndcg') for k in (5, 10)}
    for key in a:
        assert abs(a[key] - b[key]) < 1e-7, (key, a[key], b[key])


def test_metrics_and_route_refusals():
    from recbole_cdr_amd.trainer.trainer import Trainer, resolve_metrics
    model = torch.nn.Linear(2, 2)
    for bad, word in ((['AUC'], 'labeled'), (['LogLoss'], 'labeled'), (['ItemCoverage'], 'item counts'), (['GiniIndex'], 'item counts'),
                      (['nonsense'], 'supported')):
        with pytest.raises(ValueError, match=word):
            Trainer({'device': 'cpu', 'metrics': bad}, model)
    with pytest.raises(ValueError, match='gauc'):
        Trainer({'device': 'cpu', 'metrics': ['Recall', 'GAUC'], 'eval_route': 'topk'}, model)
    with pytest.raises(ValueError, match='eval_route'):
        Trainer({'device': 'cpu', 'eval_route': 'fastest'}, model)
    assert resolve_metrics({}) is None
    assert resolve_metrics({'metrics': 'NDCG'}) == ('ndcg',)
    assert resolve_metrics({'metrics': ['Recall', 'MRR', 'NDCG', 'Hit', 'Precision', 'MAP', 'GAUC']}) == \
        ('recall', 'mrr', 'ndcg', 'hit', 'precision', 'map', 'gauc')
    tr = Trainer({'device': 'cpu'}, model)
    assert tr.metrics is None and tr.eval_route == 'auto'


def test_rank_entries_are_declared_and_the_abi_version_stands():
    from recbole_cdr_amd import binding
    header = open(os.path.join(ROOT, 'include', 'cdr_hip.h')).read()
    for name in RANK_ENTRIES:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in binding._SIGNATURES and name in binding.exported_symbols()
    assert int(re.search(r'#define\s+CDR_ABI_VERSION\s+(\d+)', header).group(1)) == binding.ABI_VERSION == 64


def test_rank_entries_refuse_bad_arguments_without_a_device():
    """A NULL output, catalogues of 2^31 columns and a short workspace return CDR_EINVAL with an error text before anything is launched."""
    import ctypes
    from recbole_cdr_amd import binding
    lib = binding.load()
    need = ctypes.c_size_t(0)
    assert lib.cdr_fullsort_rank_workspace_bytes(0, 64, 100, 0, 5, ctypes.byref(need)) != 0
    assert lib.cdr_fullsort_rank_workspace_bytes(40, 64, 0, 0, 5, ctypes.byref(need)) != 0
    assert lib.cdr_fullsort_rank_workspace_bytes(40, 64, 100, 0, 5, None) != 0
    assert lib.cdr_fullsort_rank_workspace_bytes(1024, 128, 10_000_000, 0, 10_240, ctypes.byref(need)) == 0
    assert 0 < need.value <= (256 << 20) + 256                     # the staging of one column pass, whatever the catalogue
    assert lib.cdr_fullsort_rank_workspace_bytes(40, 64, 3000, 6000, 5, ctypes.byref(need)) == 0
    assert need.value == 40 * 6000 * 4
    sq = ctypes.c_size_t(0)
    assert lib.cdr_fullsort_neg_sqdist_rank_workspace_bytes(40, 64, 3000, 6000, 5, ctypes.byref(sq)) == 0
    assert sq.value == need.value + ((4 * (40 + 9000) + 255) & ~255)
    buf = (ctypes.c_float * 4096)()                                 # stands in for every array: a refused call reads none of them
    p = ctypes.cast(buf, ctypes.c_void_p)

    def rank(outs=(p, p, p, p, p), n0=3000, n1=6000, nbytes=None, pos=p):
        return lib.cdr_fullsort_rank_f32(None, p, 40, 64, p, n0, p, n1, pos, p, None, None, 1, *outs, p, need.value if nbytes is None else nbytes)

    for i in range(5):
        assert rank(outs=tuple(None if j == i else p for j in range(5))) != 0 and b'invalid argument' in lib.cdr_last_error()
    assert rank(pos=None) != 0
    assert rank(n0=1 << 30, n1=1 << 30) != 0 and b'invalid argument' in lib.cdr_last_error()
    assert rank(nbytes=need.value - 1) != 0 and b'workspace' in lib.cdr_last_error()
    assert lib.cdr_fullsort_neg_sqdist_rank_f32(None, p, 40, 64, p, 3000, p, 6000, None, p, p, None, None, 1, p, p, p, p, p, p, sq.value - 1) != 0
    assert b'workspace' in lib.cdr_last_error()
    assert lib.cdr_rank_rows_f32(None, p, 10, 4, 20, 0, p, p, None, None, 1, p, p, p, p, p, 0) != 0          # ld < N
    assert lib.cdr_rank_rows_f32(None, p, 20, 4, 20, 0, p, p, None, None, 1, p, None, p, p, p, 0) != 0        # a NULL output
    assert lib.cdr_rank_rows_f32(None, p, 20, 4, 20, (1 << 31) - 20, p, p, None, None, 1, p, p, p, p, p, 0) != 0
