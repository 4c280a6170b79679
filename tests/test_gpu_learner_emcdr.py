"""EMCDR through CrossDomainTrainer.fit with config['learner'] = 'adagrad' (SOURCE, TARGET, OVERLAP on a tiny dataset), in both
optimizer modes: finite losses, evaluation runs, k-major batches train on the per-triple step, a checkpoint written between phases and
resumed continues bit-equal to the uninterrupted run, and a checkpoint of one learner does not resume under another."""
import math

import numpy as np
import pytest
import torch

from helpers import DEV, base_config
from test_gpu_trainer_graph import _dataset, _loaders

pytestmark = pytest.mark.gpu


def _cfg(mode, **kw):
    c = base_config(DEV, latent_factor_model='BPR', source_embedding_size=16, target_embedding_size=16, reg_weight=0.01,
                    mapping_function='non_linear', mlp_hidden_size=[24], learning_rate=0.05, weight_decay=0.0, learner='adagrad',
                    optimizer_mode=mode, train_modes=['SOURCE', 'TARGET', 'OVERLAP'], epoch_num=['2', '2', '2'], source_split=False,
                    eval_step=0, epochs=2, topk=[5])
    c.update(kw)
    return c


def _fit(cfg, k, seed=3, model=None, dl=None, resume=None):
    from recbole_cdr_amd.model.cross_domain_recommender.emcdr import EMCDR
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    from recbole_cdr_amd.utils import InputType
    ids, ds, s_pairs, t_pairs = _dataset(1)
    if model is None:
        torch.manual_seed(seed)
        model = EMCDR(cfg, ds).to(DEV)
    if dl is None:
        torch.manual_seed(77)
        dl = _loaders(ids, ds, s_pairs, t_pairs, InputType.PAIRWISE, 64, k, shuffle=True)
    trainer = CrossDomainTrainer(cfg, model)
    if resume is not None:
        trainer.resume_checkpoint(resume)
    log = []
    orig = trainer._train_epoch
    trainer._train_epoch = lambda data, e: (log.append(orig(data, e)) or log[-1])
    trainer.fit(dl)
    torch.cuda.synchronize()
    return trainer, model, dl, log, (ids, t_pairs)


def _evaluate(trainer, model, ids, t_pairs):
    from recbole_cdr_amd.data.interaction import Interaction
    users = torch.as_tensor(np.unique(t_pairs[:, 0])[:20], device=DEV)
    pos_i = torch.as_tensor([t_pairs[t_pairs[:, 0] == int(u)][0, 1] for u in users.cpu()], device=DEV)
    batch = (Interaction({model.TARGET_USER_ID: users}), None, torch.arange(users.numel(), device=DEV), pos_i)
    return trainer.evaluate([batch])


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('mode', ['dense', 'rowwise'])
def test_emcdr_fit_with_adagrad(mode, k):
    from recbole_cdr_amd.trainer.trainer import DenseAdagrad
    trainer, model, _, log, (ids, t_pairs) = _fit(_cfg(mode), k)
    assert len(log) == 6 and all(math.isfinite(v) and v > 0 for v in log), log
    assert type(trainer.optimizer) is DenseAdagrad
    res = _evaluate(trainer, model, ids, t_pairs)
    assert set(res) >= {'recall@5', 'ndcg@5'} and all(math.isfinite(v) for v in res.values())
    if mode == 'dense':
        sums = [st['sum'] for st in trainer.optimizer.state.values()]
        assert len(sums) == len(list(model.parameters())) and all(bool((s > 0).any()) for s in sums)
        assert trainer.graph_stats['replayed'] > 0                          # captured dense steps keep working under the new optimizer
        return
    steps, states = model._fused['steps'], model._fused['states']
    # k-major batches (k = 2) are routed to the per-triple step: the per-positive kernels implement SGD and Adam only
    assert ('bpr', 'source') in steps and ('bpr', 'target') in steps and not any(key[0] == 'bprk' for key in steps)
    assert all(st.exp_avg is None and st.exp_avg_sq is not None and bool((st.exp_avg_sq > 0).any()) for st in states.values())
    assert type(steps[('map', 'user')].map_opt) is DenseAdagrad and len(steps[('map', 'user')].map_opt.state) > 0
    assert len(trainer.optimizer.state) == 0 and trainer.graph_stats['replayed'] == 0


def test_rowwise_adagrad_checkpoint_resumes_bit_equal_and_refuses_another_learner(tmp_path):
    from recbole_cdr_amd.model.cross_domain_recommender.emcdr import EMCDR
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    # the uninterrupted run
    _, whole, _, log_w, _ = _fit(_cfg('rowwise'), 1)
    # the same run cut after the SOURCE phase: checkpoint, a NEW model and trainer, resume, the remaining phases on the same loaders
    first = _cfg('rowwise', train_modes=['SOURCE'], epoch_num=['2'])
    tr1, m1, dl, log_a, (ids, _) = _fit(first, 1)
    path = str(tmp_path / 'mid.pth')
    tr1.save_checkpoint(path, epoch=1)
    saved = torch.load(path, weights_only=False)
    assert saved['learner'] == 'adagrad' and saved['rowwise']['opt'] == 'adagrad'
    assert all(rec['exp_avg'] is None for rec in saved['rowwise']['tables'].values())
    rest = _cfg('rowwise', train_modes=['TARGET', 'OVERLAP'], epoch_num=['2', '2'])
    torch.manual_seed(99)                                                    # (another initialisation: everything comes from the file)
    m2 = EMCDR(rest, _dataset(1)[1]).to(DEV)
    _, m2, _, log_b, _ = _fit(rest, 1, model=m2, dl=dl, resume=path)
    assert log_a + log_b == log_w, (log_a, log_b, log_w)
    pw = dict(whole.named_parameters())
    for name, p in m2.named_parameters():
        assert torch.equal(p.view(torch.int32), pw[name].view(torch.int32)), f'{name}: the resumed run differs from the uninterrupted one'
    sw, s2 = whole.fused_optimizer_state(), m2.fused_optimizer_state()
    assert sorted(sw['tables']) == sorted(s2['tables'])
    for name, rec in sw['tables'].items():
        assert rec['step'] == s2['tables'][name]['step'], name
        assert torch.equal(rec['exp_avg_sq'], s2['tables'][name]['exp_avg_sq']), name
    # the same file under another learner
    for other in ('adam', 'sgd'):
        torch.manual_seed(1)
        m3 = EMCDR(_cfg('rowwise', learner=other), _dataset(1)[1]).to(DEV)
        before = {k: v.detach().clone() for k, v in m3.named_parameters()}
        with pytest.raises(ValueError, match="learner='adagrad'"):
            CrossDomainTrainer(_cfg('rowwise', learner=other), m3).resume_checkpoint(path)
        assert '_fused' not in m3.__dict__ and all(torch.equal(v, before[k]) for k, v in m3.named_parameters())
    with pytest.raises(ValueError, match="written under opt='adagrad'"):
        m3.load_fused_optimizer_state(saved['rowwise'], opt='adam')
    assert '_fused' not in m3.__dict__
