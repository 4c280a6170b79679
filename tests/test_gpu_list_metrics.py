"""``cdr_list_stats_accumulate`` (through ``functional.ListStats``) against ``torch.bincount`` / integer sums of the same lists, bit for
bit, and ``Trainer.evaluate`` with the five non-accuracy metrics on ``test_gpu_eval_metrics.py``'s tiny models against the host test's
literal restatement applied to the lists the model's own ``full_sort_topk`` / ``full_sort_topk_wide`` returns for the same batches."""
import pytest
import torch

from helpers import DEV
from test_gpu_eval_metrics import _batches, _dataset, _emcdr, _ids, _trainer
from test_list_metrics_host import FIVE, restate, restate_tail

pytestmark = pytest.mark.gpu

#          U, kmax,   ld,     N
SHAPES = [(1, 1, 1, 1), (3, 65, 80, 1000), (70, 1024, 1024, 70001), (2048, 10, 10, 5)]


def _lists(U, kmax, ld, N, seed=0, pads=True, bad=False):
    """idx [U, kmax] as a view of a [U, ld] buffer whose columns behind kmax hold values that must not be read (they would count as bad
    ids); ids uniform over [0, N) -- at N = 5 every user holds the same few ids -- with about a tenth pads and, with ``bad``, ids >= N"""
    g = torch.Generator(device=DEV); g.manual_seed(seed + U + N)
    full = torch.full((U, ld), 1 << 40, device=DEV, dtype=torch.int64)
    idx = full[:, :kmax]
    idx.copy_(torch.randint(0, N, (U, kmax), device=DEV, generator=g))
    if pads:
        idx[torch.rand(U, kmax, device=DEV, generator=g) < 0.1] = -1
    n_bad = 0
    if bad:
        where = torch.rand(U, kmax, device=DEV, generator=g) < 0.05
        where[0, 0] = True
        junk = torch.tensor([N, N + 5, 1 << 33, (1 << 63) - 1], device=DEV)
        idx[where] = junk[torch.randint(0, 4, (int(where.sum()),), device=DEV, generator=g)]
        n_bad = int(where.sum())
    return idx, n_bad


def _operands(N, seed=1):
    g = torch.Generator(device=DEV); g.manual_seed(seed + N)
    cnt = torch.randint(0, 1 << 40, (N,), device=DEV, generator=g)                  # sums past 2^32: the 64-bit adds are whole
    tail = torch.rand(N, device=DEV, generator=g) < 0.3
    return cnt, tail


def _topk_for(kmax, n_bucket):
    if n_bucket == 1 or kmax < 4:
        return [kmax]
    return [kmax, max(kmax // 7, 1), kmax // 2, kmax // 2, kmax - 1]                  # 4 distinct values, unsorted, one twice


def _reference(idx, ks, N, cnt, tail):
    """(rec_count [n_bucket, N] int32, col_pop [kmax], col_tail [kmax], n_bad) by bincount per bucket and integer column sums"""
    ok = (idx >= 0) & (idx < N)
    safe = idx.clamp(0, N - 1)
    rec, lo = [], 0
    for k in ks:
        sel = ok[:, lo:k]
        rec.append(torch.bincount(safe[:, lo:k][sel], minlength=N).to(torch.int32))
        lo = k
    pop = (cnt[safe] * ok).sum(0)
    tl = (tail[safe].long() * ok).sum(0) if tail is not None else None
    return torch.stack(rec), pop, tl, int((idx >= N).sum())


def _check(stats, ref):
    rec, pop, tl, n_bad = ref
    assert torch.equal(stats.rec_count, rec)
    assert torch.equal(stats.col_pop, pop)
    assert (stats.col_tail is None and tl is None) or torch.equal(stats.col_tail, tl)
    assert int(stats.n_bad) == n_bad


@pytest.mark.parametrize('n_bucket', [1, 4])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_buffers_equal_bincount_and_integer_sums(shape, n_bucket):
    from recbole_cdr_amd import functional as F_
    U, kmax, ld, N = shape
    cnt, tail = _operands(N)
    topk = _topk_for(kmax, n_bucket)
    for bad in (False, True):
        for use_tail in (True, False):
            idx, n_bad = _lists(U, kmax, ld, N, bad=bad)
            stats = F_.ListStats(cnt, topk, tail_mask=tail if use_tail else None)
            assert len(stats.ks) == (1 if kmax < 4 else n_bucket) and stats.kmax == kmax
            stats.add(idx)
            ref = _reference(idx, stats.ks, N, cnt, tail if use_tail else None)
            assert ref[3] == n_bad
            _check(stats, ref)
            if bad:
                with pytest.raises(ValueError, match=str(N)):
                    stats.result(U, ['itemcoverage'])
    # two calls over halves = one call over the whole = the same call again (integer atomics: no run-to-run difference)
    idx, _ = _lists(U, kmax, ld, N, seed=7, pads=U > 1)               # (one user with one entry: not a pad, the metrics divide by R)
    whole, again, halves = (F_.ListStats(cnt, topk, tail_mask=tail) for _ in range(3))
    whole.add(idx); again.add(idx)
    halves.add(idx[:U // 2]); halves.add(idx[U // 2:])
    for other in (again, halves):
        _check(other, (whole.rec_count, whole.col_pop, whole.col_tail, 0))
    _check(whole, _reference(idx, whole.ks, N, cnt, tail))
    # the metrics of these buffers are the restatement's
    got = whole.result(U, FIVE)
    want = restate(idx.cpu().numpy(), cnt.cpu().numpy(), topk, set(torch.nonzero(tail).view(-1).tolist())) if U * kmax <= 4096 else None
    if want is not None:
        assert set(got) == set(want)
        for key in want:
            assert abs(got[key] - want[key]) <= 1e-10 * abs(want[key]), (key, got[key], want[key])


def test_no_users_and_the_pad_rule_for_values():
    from recbole_cdr_amd import binding as B_, functional as F_
    cnt, tail = _operands(1000)
    stats = F_.ListStats(cnt, [3, 10], tail_mask=tail)
    stats.add(torch.zeros(0, 10, device=DEV, dtype=torch.int64))
    B_.call('cdr_list_stats_accumulate', B_.stream(), None, 10, 0, 10, B_.raw(stats.pos_bucket), 2, 1000, B_.i64(cnt), B_.raw(stats.tail),
            B_.raw(stats.rec_count), B_.i64(stats.col_pop), B_.i64(stats.col_tail), B_.i64(stats.n_bad))
    assert not bool(stats.rec_count.any()) and not bool(stats.col_pop.any()) and not bool(stats.col_tail.any()) and int(stats.n_bad) == 0
    # vals == -inf marks a pad whatever the index says (torch.topk of a masked matrix)
    idx, _ = _lists(9, 10, 10, 1000, pads=False)
    vals = torch.rand(9, 10, device=DEV)
    vals[:, 7:] = -float('inf')
    stats.add(idx, vals)
    padded = idx.clone(); padded[:, 7:] = -1
    _check(stats, _reference(padded, stats.ks, 1000, cnt, tail))


def _model_lists(tr, batches, kmax, wide):
    """the lists the model's own full_sort_topk / full_sort_topk_wide returns for the batches, inside the evaluation bracket"""
    model = tr.model
    model.eval()
    frozen = hasattr(model, 'freeze_for_eval')
    if frozen:
        model.freeze_for_eval()
    try:
        with torch.no_grad():
            out = [tr._topk_lists(inter, len(inter), hist, kmax, wide=wide) for inter, hist, _, _ in batches]
    finally:
        if frozen:
            model.unfreeze_eval()
    return torch.cat(out).cpu().numpy()


def _compare(got, want):
    """coverage exactly, the other four within 1e-10 relative (float64 sums of at most 1e5 terms)"""
    for key in want:
        print(key, got[key], want[key])
        if key.startswith('itemcoverage'):
            assert got[key] == want[key], (key, got[key], want[key])
        else:
            assert abs(got[key] - want[key]) <= 1e-10 * abs(want[key]), (key, got[key], want[key])


def _check_trainer(cfg, model, ids, topk, wide):
    from recbole_cdr_amd.data import train_item_counts
    N = ids.OI + ids.TOI
    cnt = train_item_counts(_dataset(ids).t_pairs, N, DEV)
    assert cnt.shape == (N,) and int(cnt[0]) == 0 and int(cnt.sum()) > 0
    batches = _batches(model, ids)
    names = ['ItemCoverage', 'AveragePopularity', 'ShannonEntropy', 'GiniIndex', 'TailPercentage', 'Recall', 'NDCG']
    tr = _trainer(dict(cfg, metrics=names, topk=topk, item_counts=cnt, tail_ratio=0.2), model)
    got = tr.evaluate(batches)
    assert set(got) == {f'{n}@{k}' for n in FIVE + ('recall', 'ndcg') for k in topk}
    L = _model_lists(tr, batches, max(topk), wide)
    assert (L[6] == -1).sum() == max(topk) - 3                         # row 6: three unmasked items, the rest of its list pads
    want = restate(L, cnt.cpu().numpy(), topk, restate_tail(cnt.cpu().numpy(), 0.2))
    _compare(got, want)
    plain = _trainer(dict(cfg, metrics=['Recall', 'NDCG'], topk=topk), model).evaluate(batches)
    assert plain == {k: v for k, v in got.items() if k.split('@')[0] in ('recall', 'ndcg')}
    return tr, batches, cnt, got


def test_trainer_emcdr_fused_lists():
    cfg, model, ids = _emcdr()
    _check_trainer(cfg, model, ids, [5, 10], wide=False)


def test_trainer_emcdr_wide_lists_under_auto_and_gauc_alongside():
    cfg, model, ids = _emcdr()
    tr, batches, cnt, got = _check_trainer(cfg, model, ids, [10, 100], wide=True)
    assert tr.eval_route == 'auto'
    both = _trainer(dict(cfg, metrics=['GAUC', 'ItemCoverage'], topk=[10, 100], item_counts=cnt), model).evaluate(batches)
    assert set(both) == {'gauc', 'itemcoverage@10', 'itemcoverage@100'}
    assert both['itemcoverage@10'] == got['itemcoverage@10'] and both['itemcoverage@100'] == got['itemcoverage@100']
    only = _trainer(dict(cfg, metrics=['GAUC'], topk=[10, 100]), model).evaluate(batches)
    assert both['gauc'] == only['gauc']


def test_trainer_predict_only_model(monkeypatch):
    """DeepAPF without ``native_full_sort`` defines ``predict`` only.  At topk = [10, 100] its lists come from ``full_sort_topk_wide`` (the
    chunked ``predict`` through the wide selection): checked like EMCDR's.  At k <= 64 the list route is the trainer's chunked ``predict`` +
    mask + ``torch.topk``, which breaks ties as it likes -- and this model's fp32 scores do tie at a list's last place (seen: one entry of
    1,745 differs from the wide route's list) -- so there the check is in two halves, each exact: the metrics are the restatement's on the
    lists the trainer counted, and those lists are a top-k of the masked matrix (their scores are ``torch.topk``'s values, place for place,
    and a place is a pad exactly where that value is -inf)."""
    from helpers import base_config
    from recbole_cdr_amd import functional as F_
    from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
    from test_gpu_eval_metrics import _masked_scores
    ids = _ids()
    torch.manual_seed(13)
    cfg = base_config(DEV, embedding_size=16, beta=0.5, eval_batch_size=1 << 16)
    model = DeepAPF(cfg, _dataset(ids)).to(DEV)
    assert not hasattr(model, 'full_sort_topk')
    _, batches, cnt, _ = _check_trainer(cfg, model, ids, [10, 100], wide=True)

    counted, add = [], F_.ListStats.add

    def spy(self, idx, vals=None):
        counted.append(idx.clone() if vals is None else torch.where(vals == -float('inf'), torch.full_like(idx, -1), idx))
        return add(self, idx, vals)

    monkeypatch.setattr(F_.ListStats, 'add', spy)
    names = ['ItemCoverage', 'AveragePopularity', 'ShannonEntropy', 'GiniIndex', 'TailPercentage']
    tr = _trainer(dict(cfg, metrics=names, topk=[5, 10], item_counts=cnt, tail_ratio=0.2), model)
    got = tr.evaluate(batches)
    assert len(counted) == len(batches)
    for L, b in zip(counted, batches):
        s = _masked_scores(tr, b)
        v = torch.topk(s, 10, dim=1).values
        assert torch.equal(L < 0, v == -float('inf'))
        assert torch.equal(torch.where(L < 0, v, s.gather(1, L.clamp(min=0))), v)
    L = torch.cat(counted).cpu().numpy()
    assert (L[6] == -1).sum() == 7
    _compare(got, restate(L, cnt.cpu().numpy(), [5, 10], restate_tail(cnt.cpu().numpy(), 0.2)))
