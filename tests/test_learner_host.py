"""config['learner'] on the host side (no GPU): which optimizer the trainer builds, every refusal -- each raised before any optimizer
state exists --, the one-tensor RowwiseState of Adagrad, and the state_dict layout of the native dense optimizers, round-tripped through
torch.optim.Adagrad / RMSprop / SGD on CPU tensors."""
import copy
import os
import re
import warnings

import pytest
import torch

from helpers import base_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Model(torch.nn.Module):
    def __init__(self, fused=True):
        super().__init__()
        self.emb = torch.nn.Embedding(12, 4)
        self.lin = torch.nn.Linear(4, 3)
        if fused:
            self.fused_train_step = lambda *a, **k: None
            self.fused_sync = lambda: None


def _trainer(**kw):
    from recbole_cdr_amd.trainer.trainer import Trainer
    model = _Model()
    return Trainer(base_config('cpu', **kw), model), model


def test_learner_absent_or_adam_builds_todays_optimizer():
    from recbole_cdr_amd.trainer.trainer import DenseAdam, RowAwareAdam
    for kw in ({}, {'learner': 'adam'}, {'learner': 'Adam'}, {'learner': None}):
        tr, _ = _trainer(**kw)
        assert type(tr.optimizer) is DenseAdam and not isinstance(tr.optimizer, RowAwareAdam) and tr.learner == 'adam'
        assert tr._fused_kw() == {'opt': 'adam', 'lr': 1e-3, 'weight_decay': 0.0}


@pytest.mark.parametrize('name,cls', [('sgd', 'DenseSGD'), ('adagrad', 'DenseAdagrad'), ('rmsprop', 'DenseRMSprop'), ('AdaGrad', 'DenseAdagrad')])
def test_learner_selects_the_native_dense_optimizer_with_torch_defaults(name, cls):
    from recbole_cdr_amd.trainer import trainer as T
    tr, model = _trainer(learner=name, learning_rate=0.02, weight_decay=0.003)
    assert type(tr.optimizer) is getattr(T, cls) and tr.learner == name.lower()
    g = tr.optimizer.param_groups[0]
    assert g['lr'] == 0.02 and g['weight_decay'] == 0.003 and len(g['params']) == len(list(model.parameters()))
    want = {'sgd': torch.optim.SGD, 'adagrad': torch.optim.Adagrad, 'rmsprop': torch.optim.RMSprop}[name.lower()]
    ref = want([torch.nn.Parameter(torch.zeros(1))], lr=0.02, weight_decay=0.003).param_groups[0]
    assert {k: v for k, v in g.items() if k != 'params'} == {k: v for k, v in ref.items() if k != 'params'}
    assert len(tr.optimizer.state) == 0
    assert hasattr(tr.optimizer, 'loss_pair') and not hasattr(tr.optimizer, 'row_opt')        # deferred Adam is off for these


def test_deferred_adam_is_adams_alone():
    """A model that offers enable_deferred_adam is never asked for it under another learner."""
    from recbole_cdr_amd.trainer.trainer import Trainer, DenseAdagrad
    model = _Model()
    model.enable_deferred_adam = lambda **kw: (_ for _ in ()).throw(AssertionError('deferred Adam requested'))
    tr = Trainer(base_config('cpu', learner='adagrad'), model)
    assert type(tr.optimizer) is DenseAdagrad


def test_refusals_come_before_any_state():
    from recbole_cdr_amd.trainer.trainer import Trainer
    built = []
    model = _Model()
    orig = torch.optim.Optimizer.__init__

    def spy(self, *a, **k):
        built.append(type(self).__name__)
        return orig(self, *a, **k)
    torch.optim.Optimizer.__init__ = spy
    try:
        with pytest.raises(ValueError, match='sparse_adam'):
            Trainer(base_config('cpu', learner='sparse_adam'), model)
        with pytest.raises(ValueError, match='square_avg decays every step'):
            Trainer(base_config('cpu', learner='rmsprop', optimizer_mode='rowwise'), model)
        with pytest.raises(ValueError, match='dist_group'):
            Trainer(base_config('cpu', learner='adagrad', optimizer_mode='rowwise', dist_group=object()), model)
        with pytest.raises(ValueError, match="rowwise_adam='exact'"):
            Trainer(base_config('cpu', learner='adagrad', optimizer_mode='rowwise', rowwise_adam='exact'), model)
        assert built == [] and '_fused' not in model.__dict__
    finally:
        torch.optim.Optimizer.__init__ = orig
    # what is NOT refused: the sharded steps implement SGD, and rowwise_adam is not read in dense mode beyond its own check
    assert Trainer(base_config('cpu', learner='sgd', optimizer_mode='rowwise', dist_group=object()), model).learner == 'sgd'
    with pytest.raises(ValueError, match="applies to optimizer_mode='rowwise'"):
        Trainer(base_config('cpu', learner='sgd', rowwise_adam='exact'), model)
    with pytest.warns(UserWarning, match='unrecognized optimizer'):
        tr = Trainer(base_config('cpu', learner='lion'), model)
    assert tr.learner == 'adam' and type(tr.optimizer).__name__ == 'DenseAdam'
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        tr = Trainer(base_config('cpu', learner='adagrad', optimizer_mode='rowwise'), model)
    assert tr._fused_kw() == {'opt': 'adagrad', 'lr': 1e-3, 'weight_decay': 0.0, 'eps': 1e-10}


def test_fused_layers_refuse_unknown_and_unsupported_optimizers_before_any_state():
    from recbole_cdr_amd import fused
    from recbole_cdr_amd.model.rowwise import RowwiseTraining
    assert (fused.OPT_SGD, fused.OPT_ADAM, fused.OPT_ADAGRAD) == (0, 1, 2)
    assert RowwiseTraining._fused_args('adagrad', 'lazy', 0.1, (0.9, 0.999), 1e-10, 0.0)[1] == fused.OPT_ADAGRAD
    assert RowwiseTraining._fused_args('sgd', 'lazy', 0.1, (0.9, 0.999), 1e-8, 0.0)[1] == fused.OPT_SGD
    for bad in ('rmsprop', 'adgrad', 'SGD', None):
        with pytest.raises(ValueError, match='opt must be one of'):
            RowwiseTraining._fused_args(bad, 'lazy', 0.1, (0.9, 0.999), 1e-8, 0.0)
        with pytest.raises(ValueError, match='opt must be one of'):
            fused._Step(bad, 0.1, (0.9, 0.999), 1e-8, 0.0)
    with pytest.raises(ValueError, match="needs opt='adam'"):
        RowwiseTraining._fused_args('adagrad', 'exact', 0.1, (0.9, 0.999), 1e-10, 0.0)
    t = torch.zeros(6, 4)
    for cls, args in ((fused.KMajorBPRStep, (t, t, 4)), (fused.KMajorPointStep, (t, t, 4))):
        with pytest.raises(ValueError, match='no Adagrad form'):
            cls(*args, opt='adagrad')
    with pytest.raises(ValueError, match='needs opt=adam'):
        fused.RowwiseState(t, fused.OPT_ADAGRAD, exact=True)


def test_rowwise_state_for_adagrad_holds_exactly_one_table_sized_tensor():
    from recbole_cdr_amd import fused
    table = torch.randn(10, 8)
    st = fused.RowwiseState(table, fused.OPT_ADAGRAD)
    held = [v for v in st.__dict__.values() if torch.is_tensor(v) and v is not table]
    assert len(held) == 1 and held[0] is st.exp_avg_sq and held[0].shape == table.shape and not bool(held[0].any())
    assert st.exp_avg is None and st._step_dev is None and not st.exact and not hasattr(st, 'last') and not hasattr(st, 'hp')
    adam = fused.RowwiseState(table, fused.OPT_ADAM)
    assert sum(torch.is_tensor(v) and v is not table for v in adam.__dict__.values()) == 2
    assert fused.RowwiseState(table, fused.OPT_SGD).exp_avg_sq is None


@pytest.mark.parametrize('kind', ['sgd', 'adagrad', 'rmsprop'])
def test_state_dict_round_trips_through_torch(kind):
    from recbole_cdr_amd.trainer.trainer import dense_optimizer
    tcls = {'sgd': torch.optim.SGD, 'adagrad': torch.optim.Adagrad, 'rmsprop': torch.optim.RMSprop}[kind]
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
    topt = tcls(ps, lr=0.05, weight_decay=0.01)
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn_like(p)
        topt.step()
    sd = topt.state_dict()
    mine = dense_optimizer(kind, [torch.nn.Parameter(p.detach().clone()) for p in ps], 0.05, 0.01)
    mine.load_state_dict(copy.deepcopy(sd))                          # (load_state_dict keeps the tensors it is given) torch's checkpoint loads under the native class ...
    back = mine.state_dict()
    assert back['param_groups'] == sd['param_groups']
    assert sorted(back['state']) == sorted(sd['state'])
    for i, st in sd['state'].items():
        assert sorted(back['state'][i]) == sorted(st), (kind, sorted(back['state'][i]), sorted(st))
        for k, v in st.items():
            assert torch.equal(torch.as_tensor(back['state'][i][k]), torch.as_tensor(v)), (kind, i, k)
    want_keys = {'sgd': set(), 'adagrad': {'step', 'sum'}, 'rmsprop': {'step', 'square_avg'}}[kind]
    assert all(set(st) == want_keys for st in back['state'].values()) and (kind == 'sgd') == (len(back['state']) == 0)
    t2 = tcls([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=0.5)
    t2.load_state_dict(copy.deepcopy(back))                                         # ... and back, and torch goes on stepping from it
    for a, b in zip(t2.param_groups[0]['params'], ps):
        a.grad = torch.ones_like(a)
        b.grad = torch.ones_like(b)
    t2.step(); topt.step()
    for a, b in zip(t2.param_groups[0]['params'], ps):
        assert torch.equal(a, b)


@pytest.mark.parametrize('kind', ['adagrad', 'rmsprop'])
def test_checkpoint_written_before_every_parameter_had_a_gradient_steps_under_torch(kind):
    """torch.optim.Adagrad creates every parameter's state in __init__ and its step() reads it unchecked; the native classes create it at
    the first gradient.  A state_dict written in between (EMCDR after its SOURCE phase) carries a zero state for the rest, so torch's
    class goes on from it; an optimizer that never stepped (the unused dense one of rowwise mode) writes no state at all."""
    from recbole_cdr_amd.trainer.trainer import dense_optimizer
    tcls = {'adagrad': torch.optim.Adagrad, 'rmsprop': torch.optim.RMSprop}[kind]
    key = {'adagrad': 'sum', 'rmsprop': 'square_avg'}[kind]
    torch.manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(6))]
    mine = dense_optimizer(kind, ps, 0.05, 0.0)
    assert mine.state_dict()['state'] == {}
    mine.state[ps[0]] = {'step': torch.tensor(2.0), key: torch.full_like(ps[0], 0.25)}          # as two steps on ps[0] alone leave it
    sd = mine.state_dict()
    assert sorted(sd['state']) == [0, 1] and float(sd['state'][1]['step']) == 0.0
    assert sd['state'][1][key].shape == ps[1].shape and not bool(sd['state'][1][key].any())
    assert ps[1] not in mine.state                                                              # (writing the file creates nothing)
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    topt = tcls(qs, lr=0.5)
    topt.load_state_dict(copy.deepcopy(sd))
    ref = tcls([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=0.05)
    rq = ref.param_groups[0]['params']
    ref.state[rq[0]].update({'step': torch.tensor(2.0), key: torch.full_like(ps[0], 0.25)})
    for a, b in zip(qs, rq):
        a.grad = torch.ones_like(a); b.grad = torch.ones_like(b)
    topt.step(); ref.step()                                                                     # (KeyError: 'sum' without the zero state)
    for a, b in zip(qs, rq):
        assert torch.equal(a, b)
    back = dense_optimizer(kind, [torch.nn.Parameter(p.detach().clone()) for p in ps], 0.05, 0.0)
    back.load_state_dict(copy.deepcopy(sd))
    assert back.state_dict()['state'].keys() == sd['state'].keys()


def test_unsupported_torch_options_are_refused():
    from recbole_cdr_amd.trainer.trainer import DenseAdagrad, DenseRMSprop, DenseSGD
    p = [torch.nn.Parameter(torch.zeros(2))]
    for make in (lambda: DenseSGD(p, momentum=0.9), lambda: DenseSGD(p, nesterov=True), lambda: DenseAdagrad(p, lr_decay=0.1),
                 lambda: DenseAdagrad(p, initial_accumulator_value=0.1), lambda: DenseRMSprop(p, centered=True), lambda: DenseRMSprop(p, momentum=0.5)):
        with pytest.raises(ValueError, match='not supported'):
            make()


def test_header_codes_and_the_new_export():
    from recbole_cdr_amd import binding
    text = open(os.path.join(ROOT, 'include', 'cdr_hip.h')).read()
    for name, val in (('CDR_OPT_SGD', 0), ('CDR_OPT_ADAM', 1), ('CDR_OPT_ADAGRAD', 2), ('CDR_OPT_RMSPROP', 3), ('CDR_ABI_VERSION', 64)):
        assert re.search(rf'#define {name} {val}\b', text), name
    assert 'cdr_opt_multi_dev' in binding.exported_symbols() and len(binding._SIGNATURES['cdr_opt_multi_dev']) == 13
    assert 'cdr_point_step_fused_pair' in binding.exported_symbols() and len(binding._SIGNATURES['cdr_point_step_fused_pair']) == 36
    assert 'the row-wise entries below take CDR_OPT_SGD and CDR_OPT_ADAM only' not in text and 'exp_avg = NULL, exp_avg_sq = the table-sized sum' in text
    assert binding.ABI_VERSION == 64


def test_checkpoint_of_another_learner_is_refused(tmp_path):
    from recbole_cdr_amd.trainer.trainer import Trainer

    class M(_Model):
        def other_parameter(self):
            return None

        def load_other_parameter(self, p):
            pass
    path = str(tmp_path / 'ck.pth')
    Trainer(base_config('cpu', learner='adagrad'), M(fused=False)).save_checkpoint(path, epoch=0)
    assert torch.load(path, weights_only=False)['learner'] == 'adagrad'
    with pytest.raises(ValueError, match="learner='adagrad'"):
        Trainer(base_config('cpu', learner='adam'), M(fused=False)).resume_checkpoint(path)
    with pytest.raises(ValueError, match="learner='adagrad'"):
        Trainer(base_config('cpu', learner='sgd'), M(fused=False)).resume_checkpoint(path)
    tr = Trainer(base_config('cpu', learner='adagrad'), M(fused=False))
    tr.resume_checkpoint(path)
    assert tr.start_epoch == 1
