"""Host-side checks (no GPU) of the non-accuracy metrics (itemcoverage, averagepopularity, shannonentropy, giniindex, tailpercentage):
a literal numpy / ``collections.Counter`` restatement of recbole 1.0.1's formulas on a hand-worked example, ``functional.ListStats`` on
``device: cpu`` against it, ``data.tail_items`` / ``data.train_item_counts``, a ``device: cpu`` ``Trainer.evaluate`` with all five, the
refusals, and the declaration of ``cdr_list_stats_accumulate`` (header, binding, ABI version, CDR_EINVAL without a device)."""
import math
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ('itemcoverage', 'averagepopularity', 'shannonentropy', 'giniindex', 'tailpercentage')


def restate_tail(cnt, ratio=0.1):
    """recbole TailPercentage.get_tail over the counter's items (count >= 1)"""
    ratio = 0.1 if ratio is None or ratio <= 0 else ratio
    seen = [(i, int(c)) for i, c in enumerate(cnt) if c >= 1]
    if ratio > 1:
        return {i for i, c in seen if c <= ratio}
    seen.sort(key=lambda ic: (ic[1], ic[0]))
    return {i for i, _ in seen[:max(int(len(seen) * ratio), 1)]}


def restate(L, cnt, topk, tail=()):
    """The five formulas, literally.  L: [U, kmax] item ids, -1 a pad; cnt: [N] training counts; tail: a set of item ids."""
    L, cnt = np.asarray(L), np.asarray(cnt)
    U, N = L.shape[0], len(cnt)
    out = {}
    for k in sorted(set(topk)):
        sub = L[:, :k]
        c = Counter(int(i) for i in sub.ravel() if i >= 0)
        T, R = U * k, len(c)
        out[f'itemcoverage@{k}'] = R / N
        out[f'averagepopularity@{k}'] = float(np.mean([sum(int(cnt[i]) for i in row if i >= 0) / k for row in sub]))
        out[f'tailpercentage@{k}'] = float(np.mean([sum(1 for i in row if i >= 0 and int(i) in tail) / k for row in sub]))
        out[f'shannonentropy@{k}'] = sum(-(v / T) * math.log(v / T) for v in c.values()) / R
        s = sorted(c.values())
        out[f'giniindex@{k}'] = sum((2 * (N - R + r) - N - 1) * s[r - 1] for r in range(1, R + 1)) / T / N
    return out


HAND_CNT = [0, 5, 3, 1, 1, 2, 0]                                     # N = 7: item 0 is PAD, item 6 was never interacted with
HAND_L = [[1, 2, 3, 4], [1, 3, 5, -1], [2, 1, 4, 6]]                 # 3 users, one pad


def _hand_values():
    """k = 2: lists [1,2] [1,3] [2,1]: c = {1: 3, 2: 2, 3: 1}, T = 6, R = 3.  popularity (5+3)/2, (5+1)/2, (3+5)/2.  The tail set at
    ratio 0.1 is max(int(5 * 0.1), 1) = 1 item of (count, id) order 3, 4, 5, 2, 1: {3}: one of user 1's two entries.
    gini: s = [1, 2, 3] at idx 5, 6, 7: (2 * 5 - 8) * 1 + (2 * 6 - 8) * 2 + (2 * 7 - 8) * 3 = 28, / 6 / 7.
    k = 4: c = {1: 3, 2: 2, 3: 2, 4: 2, 5: 1, 6: 1} (the pad counts nowhere), T = 12 all the same, R = 6.  popularity 10/4, 8/4, 9/4.
    tail: item 3 once in user 0's and once in user 1's list.  gini: s = [1, 1, 2, 2, 2, 3] at idx 2..7: -4 - 2 + 0 + 4 + 8 + 18 = 24."""
    ln = math.log
    return {
        'itemcoverage@2': 3 / 7, 'itemcoverage@4': 6 / 7,
        'averagepopularity@2': (4 + 3 + 4) / 3, 'averagepopularity@4': (2.5 + 2 + 2.25) / 3,
        'tailpercentage@2': (0 + 0.5 + 0) / 3, 'tailpercentage@4': (0.25 + 0.25 + 0) / 3,
        'shannonentropy@2': -(3 / 6 * ln(3 / 6) + 2 / 6 * ln(2 / 6) + 1 / 6 * ln(1 / 6)) / 3,
        'shannonentropy@4': -(3 / 12 * ln(3 / 12) + 3 * (2 / 12 * ln(2 / 12)) + 2 * (1 / 12 * ln(1 / 12))) / 6,
        'giniindex@2': 28 / 6 / 7, 'giniindex@4': 24 / 12 / 7,
    }


def _close(got, want, keys=None):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for key in (keys or want):
        if key.startswith('itemcoverage'):
            assert got[key] == want[key], (key, got[key], want[key])
        else:
            # float64 sums of at most 1e5 terms: 1e5 * 1.1e-16
            assert abs(got[key] - want[key]) <= 1e-10 * abs(want[key]), (key, got[key], want[key])


def test_the_restatement_and_list_stats_on_a_hand_worked_example():
    from recbole_cdr_amd import functional as F_
    from recbole_cdr_amd.data import tail_items
    want = _hand_values()
    assert restate_tail(HAND_CNT) == {3}
    mine = restate(HAND_L, HAND_CNT, [2, 4], tail={3})
    assert set(mine) == set(want)
    for key in want:
        assert abs(mine[key] - want[key]) <= 1e-15, (key, mine[key], want[key])
    cnt = torch.tensor(HAND_CNT)
    stats = F_.ListStats(cnt, [2, 4], tail_mask=tail_items(cnt, 0.1))
    stats.add(torch.tensor(HAND_L))
    got = stats.result(3, FIVE)
    assert all(type(v) is float for v in got.values())
    _close(got, want)
    assert stats.rec_count.tolist() == [[0, 3, 2, 1, 0, 0, 0], [0, 0, 0, 1, 2, 1, 1]]                # the buckets [0, 2) and [2, 4)
    assert stats.col_pop.tolist() == [13, 9, 4, 1] and stats.col_tail.tolist() == [0, 1, 1, 0] and int(stats.n_bad) == 0


def _random_lists(U=37, kmax=50, N=211, seed=5):
    rng = np.random.RandomState(seed)
    L = np.stack([rng.permutation(np.arange(1, N))[:kmax] for _ in range(U)]).astype(np.int64)
    L[5, 30:] = -1; L[6, 2:] = -1; L[20, 9:] = -1                     # short lists: pads behind the last entry
    L[:, :3] = L[:, :3] % 7 + 1                                       # a few items head most lists
    cnt = rng.randint(0, 6, N)                                        # ties in the counts, items with count 0
    cnt[0] = 0
    return L, cnt


def test_list_stats_cpu_against_the_restatement():
    """U = 37, topk = [10, 3, 10, 50] (unsorted, a duplicate), N = 211, pads, ties in the counts; two batches, the second with the pads
    marked by a value of -inf instead of an index of -1."""
    from recbole_cdr_amd import functional as F_
    from recbole_cdr_amd.data import tail_items
    L, cnt = _random_lists()
    topk = [10, 3, 10, 50]
    tail = restate_tail(cnt, 0.1)
    want = restate(L, cnt, topk, tail)
    assert set(want) == {f'{n}@{k}' for n in FIVE for k in (3, 10, 50)}
    c = torch.from_numpy(cnt)
    mask = tail_items(c, 0.1)
    assert set(torch.nonzero(mask).view(-1).tolist()) == tail
    stats = F_.ListStats(c, topk, tail_mask=mask)
    assert stats.rec_count.shape == (3, 211) and stats.pos_bucket.tolist() == [0] * 3 + [1] * 7 + [2] * 40
    t = torch.from_numpy(L)
    stats.add(t[:20])
    vals = torch.where(t[20:] < 0, torch.tensor(-float('inf')), torch.rand(17, 50))
    stats.add(t[20:].clamp(min=0) + (t[20:] < 0) * 17, vals)          # the index behind a -inf value is whatever torch.topk left there
    _close(stats.result(37, FIVE), want)
    # names select; without a tail mask tailpercentage is refused; an id >= N is counted, never indexed with, and refused at the end
    assert set(stats.result(37, ['GiniIndex'])) == {'giniindex@3', 'giniindex@10', 'giniindex@50'}
    plain = F_.ListStats(c, [3])
    plain.add(t[:, :3].contiguous())
    with pytest.raises(ValueError, match='tail_mask'):
        plain.result(37, ['tailpercentage'])
    assert plain.result(37, ['itemcoverage']) == {'itemcoverage@3': want['itemcoverage@3']}
    plain.add(torch.tensor([[3, 211, 500]]))
    assert int(plain.n_bad) == 2
    with pytest.raises(ValueError, match='211'):
        plain.result(38, ['itemcoverage'])
    for bad_topk in ([], [0], [1025]):
        with pytest.raises(ValueError, match='topk'):
            F_.ListStats(c, bad_topk)
    with pytest.raises(ValueError, match='integer'):
        F_.ListStats(c.float(), [3])


def test_tail_items_and_train_item_counts():
    from recbole_cdr_amd.data import tail_items, train_item_counts
    cnt = torch.tensor([0, 4, 1, 0, 2, 1, 7, 1, 2, 9, 3, 5, 6, 8, 1, 2, 3, 4, 5, 6, 7, 8, 9])        # 21 items seen, items 0 and 3 not
    for ratio in (0.1, 5, None, 0, -1, 0.5, 1, 1.5):
        got = tail_items(cnt, ratio)
        assert got.dtype == torch.bool and got.shape == cnt.shape
        assert set(torch.nonzero(got).view(-1).tolist()) == restate_tail(cnt.tolist(), ratio), ratio
        assert not bool(got[0]) and not bool(got[3])                  # count 0: in no tail set
    # ratio 0.1: int(21 * 0.1) = 2 items of the four with count 1 (ids 2, 5, 7, 14): the two smallest ids
    assert torch.nonzero(tail_items(cnt, 0.1)).view(-1).tolist() == [2, 5]
    assert torch.nonzero(tail_items(cnt, None)).view(-1).tolist() == [2, 5]
    # ratio 5 > 1: a count threshold
    assert torch.nonzero(tail_items(cnt, 5)).view(-1).tolist() == [i for i, c in enumerate(cnt.tolist()) if 1 <= c <= 5]
    assert torch.nonzero(tail_items(torch.tensor([0, 3, 3, 3]), 0.1)).view(-1).tolist() == [1]        # at least one item
    assert not bool(tail_items(torch.zeros(5, dtype=torch.int64), 0.1).any())
    pairs = np.array([[1, 2], [1, 2], [3, 4], [2, 0], [5, 6], [9, 2]])
    assert train_item_counts(pairs, 8).tolist() == [0, 0, 3, 0, 1, 0, 1, 0]                            # index 0 stays 0
    got = train_item_counts(torch.from_numpy(pairs), 7, 'cpu')
    assert got.dtype == torch.int64 and got.tolist() == [0, 0, 3, 0, 1, 0, 1]
    with pytest.raises(ValueError, match='outside'):
        train_item_counts(pairs, 6)


N_ITEMS = 150


class Inter(dict):
    def to(self, dev):
        return self

    def __len__(self):
        return self['n']


class Stub(torch.nn.Module):
    target_num_items = N_ITEMS

    def __init__(self):
        super().__init__()
        g = torch.Generator(); g.manual_seed(0)
        self.w = torch.nn.Parameter(torch.randn(40, 8, generator=g))
        self.items = torch.randn(N_ITEMS, 8, generator=g)

    def scores(self, inter):
        return (self.w[inter['lo']:inter['lo'] + inter['n']] @ self.items.t()).detach()        # continuous: no ties

    def full_sort_predict(self, inter):
        return self.scores(inter).reshape(-1)


def _cpu_batches(seed=3):
    """40 users in batches of 16, 5 history items and up to 4 positives each; row 3 of the first batch has all but 12 items in its history
    (a list of 20 ends in pads); the second batch has no history"""
    rng = np.random.RandomState(seed)
    batches = []
    for lo in range(0, 40, 16):
        n = min(16, 40 - lo)
        hr = np.repeat(np.arange(n), 5); hc = rng.randint(1, N_ITEMS, hr.size)
        if lo == 0:
            keep = rng.permutation(np.arange(1, N_ITEMS))[12:]
            hr, hc = np.concatenate([hr, np.full(keep.size, 3)]), np.concatenate([hc, keep])
        taken = set(zip(hr.tolist(), hc.tolist()))
        pu = np.repeat(np.arange(n), 4); pi = rng.randint(1, N_ITEMS, pu.size)
        pairs = np.unique(np.stack([pu, pi], 1), axis=0)
        pairs = np.array([p for p in pairs.tolist() if tuple(p) not in taken])
        hist = (torch.from_numpy(hr), torch.from_numpy(hc)) if lo != 16 else None
        batches.append((Inter({'lo': lo, 'n': n}), hist, torch.from_numpy(pairs[:, 0]), torch.from_numpy(pairs[:, 1])))
    return batches


def _stable_lists(model, batches, kmax):
    """the lists of the stable-sorted masked matrix, -1 where the entry is masked"""
    out = []
    for inter, hist, _, _ in batches:
        s = model.scores(inter).clone()
        s[:, 0] = -np.inf
        if hist is not None:
            s[hist] = -np.inf
        v, i = torch.sort(s, dim=1, descending=True, stable=True)
        out.append(torch.where(v[:, :kmax] == -np.inf, torch.tensor(-1), i[:, :kmax]))
    return torch.cat(out).numpy()


def test_cpu_trainer_with_all_five_and_recall():
    from recbole_cdr_amd.trainer.trainer import Trainer
    model, batches = Stub(), _cpu_batches()
    rng = np.random.RandomState(9)
    cnt = rng.randint(0, 9, N_ITEMS); cnt[0] = 0
    names = ['ItemCoverage', 'AveragePopularity', 'ShannonEntropy', 'GiniIndex', 'TailPercentage', 'Recall']
    cfg = {'device': 'cpu', 'metrics': names, 'topk': [3, 20], 'item_counts': cnt, 'tail_ratio': 0.2, 'valid_metric': 'ItemCoverage@20'}
    tr = Trainer(cfg, model)
    assert tr.list_metrics == FIVE and tr.valid_metric == 'itemcoverage@20'
    got = tr.evaluate(batches)
    assert set(got) == {f'{n}@{k}' for n in FIVE + ('recall',) for k in (3, 20)}
    L = _stable_lists(model, batches, 20)
    assert (L[3] == -1).sum() == 8 and (L >= 0).sum() == 40 * 20 - 8                 # the padded list is in
    want = restate(L, cnt, [3, 20], restate_tail(cnt, 0.2))
    _close({k: v for k, v in got.items() if not k.startswith('recall')}, want)
    plain = Trainer({'device': 'cpu', 'metrics': ['Recall'], 'topk': [3, 20]}, model).evaluate(batches)
    assert plain == {k: v for k, v in got.items() if k.startswith('recall')}
    # gauc rides along: the rank route answers recall and gauc, the lists feed the five
    both = Trainer(dict(cfg, metrics=names + ['GAUC']), model).evaluate(batches)
    assert set(both) == set(got) | {'gauc'}
    _close({k: v for k, v in both.items() if k.split('@')[0] in FIVE}, want)
    ranked = Trainer({'device': 'cpu', 'metrics': ['Recall', 'GAUC'], 'topk': [3, 20]}, model).evaluate(batches)
    assert {k: v for k, v in both.items() if k.split('@')[0] not in FIVE} == ranked

    # a loader's own item_counts wins over config['item_counts']; eval_loader_for's argument is that attribute
    class Loader(list):
        pass
    own = Loader(batches)
    own.item_counts = torch.from_numpy(cnt) * 2
    doubled = tr.evaluate(own)
    assert abs(doubled['averagepopularity@20'] - 2 * got['averagepopularity@20']) <= 1e-10 * doubled['averagepopularity@20']
    assert doubled['giniindex@3'] == got['giniindex@3']
    # counts shorter than the column space: refused with the vector's length, not indexed with
    own.item_counts = torch.from_numpy(cnt[:100])
    with pytest.raises(ValueError, match='100'):
        tr.evaluate(own)


def test_eval_loader_for_sets_the_loader_s_item_counts():
    import inspect
    from recbole_cdr_amd.data import dataloader
    assert inspect.signature(dataloader.eval_loader_for).parameters['item_counts'].default is None

    class DS:
        num_overlap_item, num_target_only_item, num_total_item = 1, 9, 15
    pairs = np.array([[1, 2], [2, 3]])
    cnt = torch.arange(10)
    a = dataloader.eval_loader_for({}, 'target', DS, 'uid', 'iid', pairs, pairs[:0], 'cpu', item_counts=cnt)
    assert a.item_counts is cnt
    assert not hasattr(dataloader.eval_loader_for({}, 'target', DS, 'uid', 'iid', pairs, pairs[:0], 'cpu'), 'item_counts')


def test_refusals():
    from recbole_cdr_amd.trainer.trainer import Trainer, resolve_metrics
    model = torch.nn.Linear(2, 2)
    cnt = np.arange(10)
    for name in FIVE:
        with pytest.raises(ValueError, match='item counts'):
            Trainer({'device': 'cpu', 'metrics': [name]}, model)
        with pytest.raises(ValueError, match=r"config\['item_counts'\]"):
            resolve_metrics({'metrics': [name], 'item_counts': None})
        assert resolve_metrics({'metrics': [name.upper(), 'recall'], 'item_counts': cnt}) == (name, 'recall')
    base = {'device': 'cpu', 'metrics': ['GiniIndex', 'Recall'], 'item_counts': cnt}
    with pytest.raises(ValueError, match="eval_route='rank' holds no list"):
        Trainer(dict(base, eval_route='rank'), model)
    with pytest.raises(ValueError, match='1024'):
        Trainer(dict(base, topk=[10, 1025]), model)
    for mode in ('uni100', 'pop5'):
        with pytest.raises(ValueError, match='sampled'):
            Trainer(dict(base, eval_args={'mode': mode}), model)
    with pytest.raises(ValueError, match='dist_group'):
        Trainer(dict(base, dist_group=True, optimizer_mode='rowwise'), model)
    with pytest.raises(ValueError, match='1-D integer'):
        Trainer(dict(base, item_counts=np.ones((3, 3), dtype=np.int64)), model)
    with pytest.raises(ValueError, match='1-D integer'):
        Trainer(dict(base, item_counts=np.ones(3)), model)
    ok = Trainer(dict(base, topk=[10, 1024], eval_route='topk', valid_metric='itemcoverage@10'), model)
    assert ok.list_metrics == ('giniindex',) and ok.valid_metric == 'itemcoverage@10' and ok.item_counts.dtype == torch.int64

    class Sampled(list):
        eval_mode = 'sampled'
    with pytest.raises(ValueError, match='sampled'):
        ok.evaluate(Sampled())
    # a config without the five and without item_counts is what it was
    tr = Trainer({'device': 'cpu'}, model)
    assert tr.list_metrics == () and tr.item_counts is None


def test_the_entry_is_declared_and_the_abi_version_stands():
    from recbole_cdr_amd import binding
    header = open(os.path.join(ROOT, 'include', 'cdr_hip.h')).read()
    name = 'cdr_list_stats_accumulate'
    assert re.search(r'\bint\s+' + name + r'\s*\(', header)
    assert name in binding._SIGNATURES and name in binding.exported_symbols() and len(binding._SIGNATURES[name]) == 14
    assert int(re.search(r'#define\s+CDR_ABI_VERSION\s+(\d+)', header).group(1)) == binding.ABI_VERSION == 64


def test_the_entry_refuses_bad_arguments_without_a_device():
    """A NULL required pointer, kmax / U / N / n_bucket / ld out of range and a tail without its column sums return CDR_EINVAL with an
    error text before anything is launched; U = 0 launches nothing."""
    import ctypes
    from recbole_cdr_amd import binding
    lib = binding.load()
    buf = (ctypes.c_int64 * 4096)()                                 # stands in for every array: a refused call reads none of them
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(idx=p, ld=100, U=8, kmax=100, bucket=p, n_bucket=3, N=1000, cnt=p, tail=p, rec=p, pop=p, ctail=p, bad=p):
        return lib.cdr_list_stats_accumulate(None, idx, ld, U, kmax, bucket, n_bucket, N, cnt, tail, rec, pop, ctail, bad)

    for kw in ({'idx': None}, {'bucket': None}, {'cnt': None}, {'rec': None}, {'pop': None}, {'bad': None}, {'tail': None}, {'ctail': None},
               {'kmax': 0}, {'kmax': 1025, 'ld': 1025}, {'ld': 99}, {'U': -1}, {'U': 1 << 30}, {'N': 0}, {'N': 1 << 31}, {'n_bucket': 0},
               {'n_bucket': 101}):
        assert call(**kw) == -1, kw                                   # CDR_EINVAL
        assert b'cdr_list_stats_accumulate: invalid argument' in lib.cdr_last_error(), kw
    assert call(U=0) == 0 and call(U=0, idx=None) == 0 and call(U=0, tail=None, ctail=None) == 0
