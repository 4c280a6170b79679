"""The models whose row-wise step updates through the general segmented apply (fused._Step._apply -> cdr_rowwise_apply) under
config['learner'] = 'adagrad': SSCDR, CLFM, DTCDR (dropout 0), DeepAPF and DCDCSR -- and CMF, whose joint step on shared tables takes the
host-state entry cdr_point_step_fused_pair --, built at the sizes their own row-wise tests use.
One trainer step (DCDCSR: its whole four-phase schedule, whose loaders the trainer helper owns) with optimizer_mode='rowwise' against
the same model's optimizer_mode='dense' step from the same parameters and batch, both with learner='adagrad' and weight_decay = 0
(where the row-wise form IS the dense one): every parameter -- tables and the small dense ones -- and every sum of squared gradients
within the tolerance of those models' rowwise-vs-dense Adam tests (rtol 1e-4, atol lr * 5e-2 on parameters, 5e-5 on losses).
"""
import pytest
import torch

from helpers import DEV, assert_close

pytestmark = pytest.mark.gpu

LR = 0.01


class _OneBatch:
    """A training loader cut to the first batch of every epoch (host loaders only: no device producer)."""

    def __init__(self, inner):
        self.__dict__['_inner'] = inner

    def __iter__(self):
        first = True
        for batch in self._inner:                   # (the rest of the epoch is drawn and dropped: the loaders end their epoch, and both
            if first:                               # runs leave the samplers where the other does)
                first = False
                yield batch

    def __getattr__(self, name):
        if name == 'device_producer':
            raise AttributeError(name)
        return getattr(self._inner, name)

    def __setattr__(self, name, value):
        setattr(self._inner, name, value)


@pytest.fixture
def trainers(monkeypatch):
    """Every trainer built while the test runs, in order."""
    from recbole_cdr_amd.trainer.trainer import Trainer
    seen, orig = [], Trainer.__init__

    def init(self, config, model):
        orig(self, config, model)
        seen.append(self)
    monkeypatch.setattr(Trainer, '__init__', init)
    return seen


def _sums_dense(trainer):
    names = {id(p): k for k, p in trainer.model.named_parameters()}
    return {names[id(p)]: st['sum'] for p, st in trainer.optimizer.state.items()}


def _sums_rowwise(model):
    names = {id(p): k for k, p in model.named_parameters()}
    out = {f'{k}.weight': st.exp_avg_sq for k, st in model._fused['states'].items()}
    for step in model._fused['steps'].values():
        opt = getattr(step, 'w_opt', None) or getattr(step, 'map_opt', None)
        if opt is not None:
            assert type(opt).__name__ == 'DenseAdagrad', type(opt).__name__
            out.update({names[id(p)]: st['sum'] for p, st in opt.state.items()})
    return out


def _compare(tag, dense, rowwise, trainers, losses=True):
    (log_d, par_d, model_d), (log_r, par_r, model_r) = dense[:3], rowwise[:3]
    tr_d, tr_r = trainers[-2], trainers[-1]
    assert tr_d.optimizer_mode == 'dense' and tr_r.optimizer_mode == 'rowwise' and tr_d.learner == tr_r.learner == 'adagrad'
    assert type(tr_d.optimizer).__name__ == 'DenseAdagrad' and len(tr_r.optimizer.state) == 0
    assert all(st.exp_avg is None and st.exp_avg_sq is not None for st in model_r._fused['states'].values())
    if losses:
        assert_close(torch.tensor(log_r), torch.tensor(log_d), rtol=5e-5, what=f'{tag}: epoch losses')
    for k in par_d:
        assert_close(par_r[k], par_d[k], rtol=1e-4, atol=LR * 5e-2, what=f'{tag}: {k}')
    sd, sr = _sums_dense(tr_d), _sums_rowwise(model_r)
    moved = [k for k in sd if bool((sd[k] != 0).any())]
    assert moved and set(moved) <= set(sr), (tag, sorted(set(moved) - set(sr)))
    for k in moved:
        scale = float(sd[k].abs().max())
        assert_close(sr[k], sd[k], rtol=1e-4, atol=1e-4 * scale, what=f'{tag}: sum of {k}')
    tables = [k for k in moved if k.endswith('embedding.weight')]
    assert tables, tag
    print(f'\n{tag}: {len(par_d)} parameters, {len(moved)} sums ({len(tables)} tables) agree between the row-wise and the dense Adagrad step')


def _both_cfg(mode):
    return dict(learning_rate=LR, weight_decay=0.0, learner='adagrad', optimizer_mode=mode, train_modes=['BOTH'], epoch_num=['1'],
                source_split=False, eval_step=0, epochs=1, graph_step=False)


@pytest.mark.parametrize('name', ['cmf', 'clfm', 'dtcdr', 'deepapf'])
def test_both_phase_models_rowwise_adagrad_step_equals_dense(name, trainers):
    import importlib
    mod = importlib.import_module(f'test_gpu_{name}_rowwise')
    from test_gpu_cmf_rowwise import _host_loaders, _ids_small
    ids = mod._ids_users() if hasattr(mod, '_ids_users') else _ids_small()
    mk, reset = _host_loaders(ids)
    one = lambda: _OneBatch(mk())
    dense = mod._fit(_both_cfg('dense'), ids, one, reset, 12)
    rowwise = mod._fit(_both_cfg('rowwise'), ids, one, reset, 12)
    _compare(name.upper(), dense, rowwise, trainers)


def test_sscdr_rowwise_adagrad_steps_equal_dense(trainers):
    """One step of each of SSCDR's phases (SOURCE, TARGET, OVERLAP; the device sampler draws the same ids in both runs)."""
    import test_gpu_sscdr_rowwise as mod
    from oracle.common import IdSpace
    from test_gpu_exact_rowwise_adam import _small_loaders
    ids = IdSpace(OU=20, TOU=15, SOU=18, OI=1, TOI=30, SOI=34)
    mk, reset = _small_loaders(ids, 'BPR')
    one = lambda: _OneBatch(mk())
    cfg = lambda mode: dict(mod._config(LR, optimizer_mode=mode, learner='adagrad', weight_decay=0.0), epoch_num=['1', '1', '1'], eval_step=0, epochs=1)
    dense = mod._fit(cfg('dense'), ids, one, reset, 12)
    rowwise = mod._fit(cfg('rowwise'), ids, one, reset, 12)
    _compare('SSCDR', dense, rowwise, trainers)


def test_dcdcsr_rowwise_adagrad_schedule_equals_dense(trainers):
    """DCDCSRTrainer over SOURCE -> TARGET -> BOTH -> TARGET (the helper of test_gpu_dcdcsr_rowwise.py owns the loaders, so the whole
    schedule runs: every step class of the model -- BPR, map, frozen-side BPR -- is visited)."""
    import test_gpu_dcdcsr_rowwise as mod
    dense = mod._fit(dict(optimizer_mode='dense', learner='adagrad', weight_decay=0.0))
    rowwise = mod._fit(dict(optimizer_mode='rowwise', learner='adagrad', weight_decay=0.0))
    assert set(rowwise[2]._fused['steps']) >= {'map', 'frozen'}
    _compare('DCDCSR', dense, rowwise, trainers)
    assert_close(rowwise[2].benchmark_embedding, dense[2].benchmark_embedding, rtol=1e-4, atol=LR * 5e-2, what='benchmark table')
    assert_close(rowwise[2].affine_embedding, dense[2].affine_embedding, rtol=1e-4, atol=LR * 5e-2, what='affine table')
