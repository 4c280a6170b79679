"""SSCDR on the O(batch) row-wise path (``optimizer_mode='rowwise'``): ``SSCDR.fused_train_step`` -- fused.FusedTripletStep on a domain's
tables, fused.SSCDRMapStep on the three tables of the OVERLAP phase -- pinned to the reference's own gradients (the golden fixtures,
sscdr.py:133-187), to the dense trainer under the exact row-wise Adam, and to itself across a checkpoint."""
import numpy as np
import pytest
import torch

from golden_util import Golden, cases
from helpers import DEV, FakeDataset, assert_close, base_config, load_params, to_dev

pytestmark = pytest.mark.gpu

TABLES = ('source_user_embedding', 'source_item_embedding', 'target_user_embedding', 'target_item_embedding')


@pytest.mark.parametrize('phase', ['SOURCE', 'TARGET', 'BOTH', 'OVERLAP'])
@pytest.mark.parametrize('name', cases('sscdr_'))
def test_fused_train_step_takes_the_references_sgd_step(name, phase):
    """One plain SGD step with lr = 1 from the fixture's parameters: the loss is the reference's, every parameter with a reference
    gradient lands on param - grad, every other parameter stays bit-equal.  OVERLAP draws its semi-supervised ids from numpy's
    global stream (seed 99, as the reference did)."""
    from recbole_cdr_amd.model.cross_domain_recommender.sscdr import SSCDR
    g = Golden(name)
    ids = g.idspace()
    indptr, indices = g['aux/hist_indptr'], g['aux/hist_indices']
    mode_users = ids.mode == 'overlap_users'
    own = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    pairs = np.stack([own, indices], 1) if mode_users else np.stack([indices, own], 1)
    ds = FakeDataset(ids, s_pairs=pairs.astype(np.int64), t_pairs=np.zeros((1, 2), dtype=np.int64))
    cfg = base_config(DEV, embedding_size=int(g.meta('D')), margin=float(g.meta('margin')),
                      mlp_hidden_size=[int(x) for x in g.meta('mlp_hidden_size')], **{'lambda': float(g.meta('lam'))})
    model = SSCDR(cfg, ds).to(DEV)
    params = g.group('param')
    load_params(model, params)
    inter = to_dev(g.group('in'), DEV)
    model.set_phase(phase)
    np.random.seed(99)
    loss = model.fused_train_step(inter, opt='sgd', lr=1.0)
    torch.cuda.synchronize()
    assert_close(loss, g[f'loss/{phase}'], what=f'{name}:{phase}:loss')
    grads = g.group(f'grad/{phase}')
    assert grads and (phase != 'OVERLAP' or any(k.startswith('mapping_layer') for k in grads))
    for k, p in model.named_parameters():
        if k in grads:
            assert float(grads[k].abs().max()) > 0
            assert_close(p, params[k] - grads[k], what=f'{name}:{phase}:{k}')
            assert not torch.equal(p.detach().cpu(), params[k]), k
        else:
            assert torch.equal(p.detach().cpu(), params[k]), f'{name}:{phase}:{k} moved without a reference gradient'
    touched = {k[:-len('.weight')] for k in grads if not k.startswith('mapping_layer')}
    assert set(model._fused['states']) == touched and all(st.step == 1 for st in model._fused['states'].values())


def _dataset(ids, seed=0):
    """Source interactions of the overlapped users (SSCDR samples its semi-supervised ids from them) and a few target pairs."""
    rng = np.random.RandomState(seed)
    src_u = np.array(list(range(1, ids.OU)) + list(range(ids.OU + ids.TOU, ids.total_num_users)))
    src_i = np.arange(ids.OI + ids.TOI, ids.total_num_items)
    s_pairs = np.unique(np.stack([rng.choice(src_u, 160), rng.choice(src_i, 160)], 1), axis=0).astype(np.int64)
    return FakeDataset(ids, s_pairs=s_pairs, t_pairs=np.zeros((1, 2), dtype=np.int64))


def _config(lr, **kw):
    return base_config(DEV, embedding_size=16, margin=0.3, mlp_hidden_size=[24], sscdr_device_sampler=True, seed=7, learning_rate=lr,
                       train_modes=['SOURCE', 'TARGET', 'OVERLAP'], epoch_num=['2', '1', '2'], source_split=False, eval_step=1, epochs=2,
                       graph_step=False, **{'lambda': 0.5}, **kw)


def _fit(cfg, ids, mk, reset, seed):
    from recbole_cdr_amd.model.cross_domain_recommender.sscdr import SSCDR
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    torch.manual_seed(seed)
    model = SSCDR(cfg, _dataset(ids)).to(DEV)
    reset()
    trainer = CrossDomainTrainer(cfg, model)
    log = []
    orig = trainer._train_epoch
    trainer._train_epoch = lambda data, e: (log.append(orig(data, e)) or log[-1])
    trainer.fit(mk())
    torch.cuda.synchronize()
    return log, {k: v.detach().clone() for k, v in model.named_parameters()}, model


def test_exact_rowwise_trainer_matches_the_dense_adam():
    """SSCDR over SOURCE -> TARGET -> OVERLAP with the device sampler: optimizer_mode='rowwise', rowwise_adam='exact' against
    optimizer_mode='dense' (DenseAdam over every table) on the same model, seed and batches -- epoch losses and every parameter within
    the tolerances of EMCDR's test of the same name; the lazy row-wise run is far outside them."""
    from oracle.common import IdSpace
    from test_gpu_exact_rowwise_adam import _small_loaders
    ids = IdSpace(OU=20, TOU=15, SOU=18, OI=1, TOI=30, SOI=34)
    lr = 0.01
    mk, reset = _small_loaders(ids, 'BPR')
    log_d, par_d, _ = _fit(_config(lr, optimizer_mode='dense'), ids, mk, reset, 12)
    log_e, par_e, model = _fit(_config(lr, optimizer_mode='rowwise', rowwise_adam='exact'), ids, mk, reset, 12)
    log_l, par_l, _ = _fit(_config(lr, optimizer_mode='rowwise'), ids, mk, reset, 12)
    assert len(log_e) == 5 and model.phase == 'OVERLAP'
    assert all(st.exact for st in model._fused['states'].values()) and set(model._fused['states']) == set(TABLES)
    assert set(model._fused['steps']) == {('triplet', 'source'), ('triplet', 'target'), ('map', 'user')}
    print('epoch losses dense', log_d, 'exact', log_e, 'lazy', log_l)
    assert_close(torch.tensor(log_e), torch.tensor(log_d), rtol=5e-5, what='epoch losses')
    for k in par_d:
        print(f'{k}: max |exact - dense| {float((par_e[k] - par_d[k]).abs().max()):.3e} (atol {lr * 5e-2:.1e})')
        assert_close(par_e[k], par_d[k], rtol=1e-4, atol=lr * 5e-2, what=k)
    worst = max(float((par_l[f'{k}.weight'] - par_d[f'{k}.weight']).abs().max()) for k in TABLES)
    assert worst > 20 * lr * 5e-2, worst


@pytest.mark.parametrize('adam', ['lazy', 'exact'])
def test_rowwise_checkpoint_resume_is_bit_exact(adam, tmp_path):
    """Two epochs row-wise (SOURCE, OVERLAP), save_checkpoint, resume_checkpoint into a fresh model and trainer, one more step of each
    kind: bit-equal to the uninterrupted run -- tables, mapping, row-wise moments and update counts, the mapping's Adam state and the ids
    the device sampler draws."""
    from oracle.common import IdSpace
    from recbole_cdr_amd.model.cross_domain_recommender.sscdr import SSCDR
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    from test_gpu_exact_rowwise_adam import _small_loaders
    ids = IdSpace(OU=20, TOU=15, SOU=18, OI=1, TOI=30, SOI=34)
    lr = 0.01
    extra = {'rowwise_adam': 'exact'} if adam == 'exact' else {}
    cfg = dict(_config(lr, optimizer_mode='rowwise', **extra), train_modes=['SOURCE', 'OVERLAP'], epoch_num=['1', '1'], eval_step=0, epochs=1)
    mk, reset = _small_loaders(ids, 'BPR')
    kw = {'lr': lr, 'adam': adam}

    def more(model):
        g = torch.Generator(); g.manual_seed(3)
        r = lambda lo, hi: torch.randint(lo, hi, (40,), generator=g).to(DEV)
        model.set_phase('OVERLAP')
        l1 = model.fused_train_step({'overlap': torch.randperm(ids.OU - 1, generator=g)[:12].add(1).reshape(12, 1).to(DEV)}, **kw)
        model.set_phase('SOURCE')
        l2 = model.fused_train_step({'source_user_id': r(1, ids.OU), 'source_item_id': r(ids.OI + ids.TOI, ids.total_num_items),
                                     'neg_source_item_id': r(ids.OI + ids.TOI, ids.total_num_items)}, **kw)
        model.fused_sync()
        torch.cuda.synchronize()
        return torch.stack([l1.reshape(()), l2.reshape(())])

    def fresh():
        torch.manual_seed(21)
        m = SSCDR(cfg, _dataset(ids)).to(DEV)
        return m, CrossDomainTrainer(cfg, m)

    m_a, t_a = fresh()
    reset()
    t_a.fit(mk())
    path = str(tmp_path / 'ckpt.pth')
    t_a.save_checkpoint(path, epoch=0)
    la = more(m_a)
    m_b, t_b = fresh()
    t_b.resume_checkpoint(path)
    assert m_b.phase == 'OVERLAP' and set(m_b._fused['states']) == {'source_user_embedding', 'source_item_embedding', 'target_user_embedding'}
    lb = more(m_b)
    assert torch.equal(la, lb), (la, lb)
    for (k, pa), (_, pb) in zip(m_a.named_parameters(), m_b.named_parameters()):
        assert torch.equal(pa, pb), k
    sa, sb = m_a.fused_optimizer_state(), m_b.fused_optimizer_state()
    assert sa['sampler_calls'] == sb['sampler_calls'] and sa['sampler_calls']['user'] > 1
    for name in sa['tables']:
        assert sa['tables'][name]['step'] == sb['tables'][name]['step'] > 0, name
        assert torch.equal(sa['tables'][name]['exp_avg'], sb['tables'][name]['exp_avg']), name
        assert torch.equal(sa['tables'][name]['exp_avg_sq'], sb['tables'][name]['exp_avg_sq']), name
    for pa, pb in zip(sa['mapping']['user']['state'].values(), sb['mapping']['user']['state'].values()):
        for q in pa:
            assert torch.equal(torch.as_tensor(pa[q]), torch.as_tensor(pb[q])), q


def test_fused_train_step_refuses_what_it_cannot_do_and_leaves_no_state():
    from oracle.common import IdSpace
    from recbole_cdr_amd.model.cross_domain_recommender.sscdr import SSCDR
    ids = IdSpace(OU=20, TOU=15, SOU=18, OI=1, TOI=30, SOI=34)
    g = torch.Generator(); g.manual_seed(1)
    r = lambda lo, hi: torch.randint(lo, hi, (40,), generator=g).to(DEV)
    b = {'source_user_id': r(1, ids.OU), 'source_item_id': r(ids.OI + ids.TOI, ids.total_num_items),
         'neg_source_item_id': r(ids.OI + ids.TOI, ids.total_num_items), 'overlap': torch.arange(1, 9).reshape(8, 1).to(DEV)}
    for extra, exc, msg in (({'dist_group': True}, NotImplementedError, 'dist_group'),
                            ({'embedding_size': 6, 'mlp_hidden_size': [8]}, ValueError, r'embedding_size % 4 == 0'),
                            ({'embedding_size': 260}, ValueError, r'embedding_size <= 256')):
        m = SSCDR(dict(_config(0.01), **extra), _dataset(ids)).to(DEV)
        before = {k: v.detach().clone() for k, v in m.named_parameters()}
        for phase in ('SOURCE', 'OVERLAP'):
            m.set_phase(phase)
            for adam in ('lazy', 'exact'):
                with pytest.raises(exc, match=msg):
                    m.fused_train_step(b, lr=0.01, adam=adam)
        assert '_fused' not in m.__dict__
        assert all(torch.equal(v, before[k]) for k, v in m.named_parameters())
    m = SSCDR(_config(0.01), _dataset(ids)).to(DEV)
    m.set_phase('SOURCE')
    with pytest.raises(ValueError, match="opt='adam'"):
        m.fused_train_step(b, opt='sgd', lr=0.01, adam='exact')
    assert '_fused' not in m.__dict__
