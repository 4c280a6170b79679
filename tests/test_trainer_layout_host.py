"""The trainer's layout after its split (CPU, no native call): ``trainer.trainer`` still exports every name it did, the fused steps and
the evaluation loaders no longer load it, the one CSR builder equals both constructions it replaced, ``Evaluation`` evaluates on its own,
and the model-side chunk walk tiles the users exactly once."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recbole_cdr_amd  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every public name of recbole_cdr_amd.trainer.trainer before the split (its module namespace, imports of whole modules left out)
EXPORTED = {
    'recbole_cdr_amd.optim': ('DenseAdam', 'DenseSGD', 'DenseAdagrad', 'DenseRMSprop', 'RowAwareAdam', 'LEARNERS', 'dense_optimizer',
                              'resolve_learner', '_DenseLearner', '_dense_adam_load', '_refuse'),
    'recbole_cdr_amd.eval_config': ('DEFAULT_METRICS', 'TOPK_METRICS', 'VALUE_METRICS', 'NON_ACCURACY_METRICS', 'FUSED_TOPK_MAX',
                                    'WIDE_TOPK_MAX', 'resolve_metrics', 'resolve_eval_mode', 'resolve_eval_route'),
    'recbole_cdr_amd.trainer.evaluation': ('DEFAULT_METRICS', 'TOPK_METRICS', 'VALUE_METRICS', 'NON_ACCURACY_METRICS', 'FUSED_TOPK_MAX',
                                           'WIDE_TOPK_MAX', 'resolve_metrics', 'resolve_eval_mode', 'resolve_eval_route',
                                           'metrics_from_hits', 'gauc_from_counts', 'rank_counts_reference'),
    'recbole_cdr_amd.trainer.trainer': ('early_stopping', 'Trainer', 'CrossDomainTrainer', 'DCDCSRTrainer'),
    'recbole_cdr_amd.utils': ('train_mode2state',),
}


def test_trainer_module_exports_what_it_did():
    import importlib
    from recbole_cdr_amd.trainer import trainer as T
    for home, names in EXPORTED.items():
        mod = importlib.import_module(home)
        for name in names:
            assert getattr(T, name) is getattr(mod, name), (home, name)
    assert issubclass(T.Trainer, T.Evaluation)
    import recbole_cdr_amd.trainer as pkg
    assert pkg.CrossDomainTrainer is T.CrossDomainTrainer and pkg.DCDCSRTrainer is T.DCDCSRTrainer


_CHILD = r'''
import sys
import recbole_cdr_amd.fused
assert 'recbole_cdr_amd.trainer.trainer' not in sys.modules, 'fused loads the trainer'
import numpy as np
from recbole_cdr_amd.data.dataloader import eval_loader_for, FullSortEvalLoader


class Dataset:
    num_overlap_item, num_target_only_item, num_total_item = 3, 4, 9


pairs = np.array([[1, 2], [1, 5], [2, 3]])
loader = eval_loader_for({'eval_args': {'mode': 'full'}}, 'target', Dataset(), 'uid', 'iid', pairs, np.array([[1, 4]]), 'cpu')
assert type(loader) is FullSortEvalLoader and len(list(loader)) == 1
assert 'recbole_cdr_amd.trainer.trainer' not in sys.modules, 'the evaluation loaders load the trainer'
print('layers ok')
'''


def test_fused_and_loaders_do_not_load_the_trainer():
    """In a fresh process: neither ``import recbole_cdr_amd.fused`` nor ``eval_loader_for`` of a plain full-sort mode imports
    ``trainer/trainer.py``."""
    done = subprocess.run([sys.executable, '-c', _CHILD], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and 'layers ok' in done.stdout, done.stderr[-2000:]


def _old_sorted_csr(rows, hc, n_user):
    """The construction ``_topk_lists`` held inline before the one builder (without its final None for an empty list)."""
    span = int(hc.max()) + 1 if hc.numel() else 1
    key = torch.sort(rows * span + hc).values
    cols = (key % span).contiguous()
    indptr = torch.zeros(n_user + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.bincount(key // span, minlength=n_user), 0)
    return indptr, cols


def _old_unique_csr(rows, cols, n_user):
    """``Trainer._csr`` before the one builder."""
    span = int(cols.max()) + 1 if cols.numel() else 1
    key = torch.unique(rows * span + cols)
    indptr = torch.zeros(n_user + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.bincount(key // span, minlength=n_user), 0)
    return indptr, (key % span).contiguous()


def _csr_cases():
    g = torch.Generator(); g.manual_seed(5)
    n_user = 9
    rows = torch.randint(0, n_user - 1, (60,), generator=g)               # the last user stays empty
    rows[rows == 3] = 4                                                   # ... and user 3 has no pairs
    cols = torch.randint(1, 12, (60,), generator=g)                       # 60 pairs over 7 x 11 cells: repeated pairs
    rows, cols = torch.cat([rows, rows[:10]]), torch.cat([cols, cols[:10]])
    assert torch.unique(rows * 100 + cols).numel() < rows.numel()
    return {'random': (rows, cols, n_user),
            'one user': (torch.full((20,), 2), torch.randint(0, 6, (20,), generator=g), 5),
            'empty': (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 4)}


@pytest.mark.parametrize('case', ['random', 'one user', 'empty'])
def test_one_csr_builder_equals_both_it_replaced(case):
    from recbole_cdr_amd.trainer.evaluation import Evaluation
    rows, cols, n_user = _csr_cases()[case]
    for distinct, old in ((False, _old_sorted_csr), (True, _old_unique_csr)):
        indptr, out = Evaluation._csr(rows, cols, n_user, distinct)
        want_indptr, want = old(rows, cols, n_user)
        assert indptr.dtype == torch.int64 and out.dtype == torch.int64
        assert torch.equal(indptr, want_indptr) and torch.equal(out, want)
        assert int(indptr[0]) == 0 and int(indptr[-1]) == out.numel() == (torch.unique(rows * 100 + cols).numel() if distinct else rows.numel())
        for u in range(n_user):
            seg = out[indptr[u]:indptr[u + 1]]
            mine = cols[rows == u].tolist()
            assert seg.tolist() == (sorted(set(mine)) if distinct else sorted(mine))     # the user's own columns, ascending
    # the history form: no history, or an empty one, is (None, None) on both flavours, as the routes always handed it to the model
    ev = Evaluation.__new__(Evaluation)
    ev.device = 'cpu'
    for distinct in (False, True):
        assert ev._history_csr(None, n_user, distinct) == (None, None)
        got = ev._history_csr((rows, cols), n_user, distinct)
        if rows.numel() == 0:
            assert got == (None, None)
        else:
            want = (_old_unique_csr if distinct else _old_sorted_csr)(rows, cols, n_user)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _stub_and_batches():
    """The stub model and batches of test_host_side.py::test_evaluate_topk_path_equals_full_matrix_path."""

    class Stub(torch.nn.Module):
        target_num_items = 57

        def __init__(self):
            super().__init__()
            g = torch.Generator(); g.manual_seed(0)
            self.w = torch.nn.Parameter(torch.randn(40, 8, generator=g))
            self.items = torch.randn(57, 8, generator=g)

        def full_sort_predict(self, inter):
            return (self.w[inter['uid']] @ self.items.t()).reshape(-1)

        def full_sort_topk(self, inter, k, hist_indptr=None, hist_cols=None):
            s = (self.w[inter['uid']] @ self.items.t()).detach().clone()
            s[:, 0] = -float('inf')
            if hist_indptr is not None:
                for u in range(s.shape[0]):
                    s[u, hist_cols[hist_indptr[u]:hist_indptr[u + 1]]] = -float('inf')
            return torch.topk(s, k, dim=1)

    class Inter(dict):
        def to(self, dev):
            return self

        def __len__(self):
            return self['uid'].numel()

    rng = np.random.RandomState(3)
    batches = []
    for lo in (0, 16, 32):
        uid = torch.arange(lo, min(lo + 16, 40))
        n = uid.numel()
        hr = np.repeat(np.arange(n), 5); hc = rng.randint(1, 57, hr.size)
        pu = np.repeat(np.arange(n), 3); pi = rng.randint(1, 57, pu.size)
        pairs = np.unique(np.stack([pu, pi], 1), axis=0)                      # (user, item) positives, deduplicated
        hist = (torch.from_numpy(hr), torch.from_numpy(hc)) if lo != 16 else None     # one batch without history
        batches.append((Inter(uid=uid), hist, torch.from_numpy(pairs[:, 0]), torch.from_numpy(pairs[:, 1])))
    return Stub(), batches


def _unmasked_positives(batches):
    """The same batches with the positives that fall into their user's history left out: the rank route refuses to rank those."""
    out = []
    for inter, hist, pu, pi in batches:
        if hist is not None:
            taken = set(zip(hist[0].tolist(), hist[1].tolist()))
            keep = torch.tensor([(u, i) not in taken for u, i in zip(pu.tolist(), pi.tolist())])
            pu, pi = pu[keep], pi[keep]
        out.append((inter, hist, pu, pi))
    return out


@pytest.mark.parametrize('fused_topk', [True, False])
@pytest.mark.parametrize('metrics', [None, ('map', 'gauc')])
def test_evaluation_alone_returns_the_trainers_dict(fused_topk, metrics):
    from recbole_cdr_amd.trainer.evaluation import Evaluation
    from recbole_cdr_amd.trainer.trainer import Trainer
    model, batches = _stub_and_batches()
    cfg = {'device': 'cpu', 'topk': [5, 10], 'valid_metric': 'Recall@10', 'fused_topk': fused_topk}
    if metrics is not None:                                # gauc: the rank route, on the CPU through rank_counts_reference
        cfg['metrics'] = list(metrics)
        batches = _unmasked_positives(batches)
    tr = Trainer.__new__(Trainer)
    tr.config, tr.model, tr.device, tr.topk, tr.fused_topk = cfg, model, 'cpu', [5, 10], fused_topk
    if metrics is not None:
        tr.metrics = metrics
    ev = Evaluation(cfg, model)
    assert not hasattr(ev, 'optimizer') and (ev.metrics, ev.topk, ev.fused_topk, ev.eval_route) == (metrics, [5, 10], fused_topk, 'auto')
    want, got = tr.evaluate(batches), ev.evaluate(batches)
    assert got == want                                     # the same arithmetic: equal floats
    keys = {f'{m}@{k}' for m in ('recall', 'hit', 'precision', 'mrr', 'ndcg') for k in (5, 10)} if metrics is None else \
        {'map@5', 'map@10', 'gauc'}
    assert set(got) == keys and all(v == v for v in got.values())
    assert got['recall@10' if metrics is None else 'map@10'] > 0
    if metrics is not None:
        with pytest.raises(ValueError, match='is masked'):                # (the stub's own positives: some are in the history)
            ev.evaluate(_stub_and_batches()[1])


class _Walked(torch.nn.Module):
    """Borrows the model-side chunk walk for a CPU stub of 13 items."""
    from recbole_cdr_amd.model.crossdomain_recommender import CrossDomainRecommender as _base
    RANK_ROWS_MAX_SCORES = _base.RANK_ROWS_MAX_SCORES
    _score_chunks = _base._score_chunks
    full_sort_predict = _base.full_sort_predict                         # (raises NotImplementedError)

    def __init__(self):
        super().__init__()
        g = torch.Generator(); g.manual_seed(1)
        self.table = torch.randn(20, 13, generator=g)
        self.calls = []

    def scores(self, inter, n_user=None):
        self.calls.append(len(inter))
        return self.table[inter['uid']].clone()


class _WithFullSort(_Walked):
    def full_sort_predict(self, inter):
        return self.scores(inter).reshape(-1)


@pytest.mark.parametrize('kind', ['full_sort_predict', 'predict_fallback'])
def test_chunk_walk_tiles_the_users_once(kind, monkeypatch):
    from recbole_cdr_amd.data.interaction import Interaction
    model = _WithFullSort() if kind == 'full_sort_predict' else _Walked()
    fallback = None if kind == 'full_sort_predict' else model.scores
    inter = Interaction({'uid': torch.tensor([3, 9, 0, 19, 4, 4, 11])})
    whole = list(model._score_chunks(inter, fallback))                  # the class's own limit: one block
    assert [(s, e) for s, e, _ in whole] == [(0, 7)] and model.calls == [7]
    monkeypatch.setattr(type(model), 'RANK_ROWS_MAX_SCORES', 2 * 13 + 5)           # 7 x 13 is too tall: chunks of 2 users
    model.calls.clear()
    blocks = list(model._score_chunks(inter, fallback))
    assert [(s, e) for s, e, _ in blocks] == [(0, 2), (2, 4), (4, 6), (6, 7)]
    assert model.calls == [7, 2, 2, 2, 1]                                # the first block was scored whole, then redone in chunks
    for s, e, scores in blocks:
        assert scores.shape == (e - s, 13) and torch.equal(scores, whole[0][2][s:e])
    # one user is never re-cut, however small the limit
    monkeypatch.setattr(type(model), 'RANK_ROWS_MAX_SCORES', 1)
    model.calls.clear()
    one = list(model._score_chunks(inter[2:3], fallback))
    assert [(s, e) for s, e, _ in one] == [(0, 1)] and model.calls == [1] and torch.equal(one[0][2], whole[0][2][2:3])
    if kind == 'predict_fallback':                                       # without a fallback the model's refusal comes through
        with pytest.raises(NotImplementedError):
            list(model._score_chunks(inter, None))
