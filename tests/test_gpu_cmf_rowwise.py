"""CMF on the O(batch) row-wise path (``optimizer_mode='rowwise'``): fused.FusedPointPairStep / csrc/cdr_step.hip
cdr_point_step_fused_pair_dev trains BOTH domains' pointwise batches on the SHARED user and item tables (cmf.py:41-42, 81-99) with ONE
update per touched row from the sum of its source and target contributions -- the reference's single torch.optim.Adam step.

Checked against: the reference's golden gradients (one SGD step with lr = 1 moves every row by -grad), a float64 restatement of the summed
loss and ONE optimizer update at up to 1,048,576 + 524,288 rows (per-element bounds of fp64_bounds.py, as test_gpu_step_fp64.py), and the
dense trainer (optimizer_mode='dense') through CrossDomainTrainer with rowwise_adam='exact'."""
import numpy as np
import pytest
import torch

from fp64_bounds import U32, apply_fp64, gam, pair_grads_fp64, ulp32
from golden_util import Golden, cases
from helpers import DEV, FakeDataset, base_config, load_params, to_dev, assert_close
from test_gpu_step_fp64 import K_COEF, LOSS_RTOL, _check_table, _fmt, _live, _occ_sums, _snapshot, _zipf

pytestmark = pytest.mark.gpu


def _cmf(ids, D=16, alpha=0.3, lam=0.02, gamma=0.05, **kw):
    from recbole_cdr_amd.model.cross_domain_recommender.cmf import CMF
    cfg = base_config(DEV, embedding_size=D, alpha=alpha, **{'lambda': lam, 'gamma': gamma}, **kw)
    return CMF(cfg, FakeDataset(ids)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------- 1. golden pin

@pytest.mark.parametrize('name', cases('cmf_'))
def test_one_sgd_step_moves_every_row_by_the_reference_gradient(name):
    """lr = 1 SGD: row r moves by exactly -grad/BOTH[r] of the reference (B_s = 20 != B_t = 27, users and items in both domains);
    the returned total is loss/BOTH; rows outside the batch keep their bits."""
    g = Golden(name)
    model = _cmf(g.idspace(), D=int(g.meta('D')), alpha=float(g.meta('alpha')), lam=float(g.meta('lam')), gamma=float(g.meta('gamma')))
    load_params(model, g.group('param'))
    inter = to_dev(g.group('in'), DEV)
    assert inter['source_user_id'].numel() != inter['target_user_id'].numel()
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    loss = model.fused_train_step(inter, opt='sgd', lr=1.0)
    torch.cuda.synchronize()
    assert_close(loss, g['loss/BOTH'], what=f'{name}: loss')
    for k, p in model.named_parameters():
        ref = g[f'grad/BOTH/{k}']
        moved = (before[k].double() - p.detach().double()).cpu()
        want = torch.as_tensor(ref).double()
        # helpers.assert_close's per-row tolerance (1e-5 relative, row-scaled floor) plus one ulp of the stored fp32 row: w - g is rounded
        # to fp32 when it is written, which at |w| ~ 0.2 is of the order of the tolerance of a 3e-4 gradient row
        rowmax = want.abs().amax(1, keepdim=True)
        tol = 1e-5 * want.abs() + 1e-5 * torch.maximum(rowmax, 1e-2 * want.abs().max()) + ulp32(p.detach().double().cpu()) + 1e-12
        bad = (moved - want).abs() > tol
        assert not bool(bad.any()), f'{name}: {k}: {int(bad.sum())} elements off the reference gradient, e.g. {torch.nonzero(bad)[0].tolist()}'
        untouched = (torch.as_tensor(ref).to(DEV) == 0).all(1)
        assert torch.equal(p.detach()[untouched].view(torch.int32), before[k][untouched].view(torch.int32)), k
    st = model._fused['states']
    assert st['user_embedding'].step == st['item_embedding'].step == 1


# ---------------------------------------------------------------------------------------------------------------------- 2. fp64 bounds

def _pair_ids(shape, Bs, Bt, nu, ni, gen):
    """(su, si, tu, ti) of one step; ``shape``: 'zipf' (Zipf items plus one item hot in both domains), 'overlap' (every target user also
    a source user), 'once_each' (every row exactly once in each domain: the case two per-domain steps would update twice), 'far'
    (logits far enough out to saturate the fp32 sigmoid: BCE's -100 log clamp and its 1e-12 backward clamp)."""
    r = lambda n, hi: torch.randint(0, hi, (n,), device=DEV, generator=gen)
    if shape == 'once_each':
        assert Bs == Bt
        pu, pi = torch.randperm(nu, device=DEV, generator=gen)[:Bs], torch.randperm(ni, device=DEV, generator=gen)[:Bs]
        return pu, pi, pu[torch.randperm(Bs, device=DEV, generator=gen)], pi[torch.randperm(Bs, device=DEV, generator=gen)]
    su, si, tu, ti = r(Bs, nu), r(Bs, ni), r(Bt, nu), r(Bt, ni)
    if shape == 'zipf':
        si, ti = _zipf(Bs, ni, gen), _zipf(Bt, ni, gen)
        si[::97] = ni // 2 + 1
        ti[::89] = ni // 2 + 1                                  # one item hot in both domains
        su[0], tu[0], si[1], ti[1] = 0, nu - 1, 0, ni - 1
    elif shape == 'overlap':
        tu = su[r(Bt, Bs)]
    return su, si, tu, ti


def _far_rows(U, I):
    """Rows 0..63 of both tables with entries 1 (users) and +-2 (items): a pair of them scores +-2 D."""
    U[:64] = 1.0
    I[:64] = 2.0
    I[32:64] = -2.0


def _far_ids(Bs, Bt, nu, ni, gen):
    r = lambda n, lo, hi: torch.randint(lo, hi, (n,), device=DEV, generator=gen)
    su, si, tu, ti = r(Bs, 0, nu), r(Bs, 64, ni), r(Bt, 0, nu), r(Bt, 64, ni)
    k = Bs // 8
    su[:k], si[:k] = r(k, 0, 64), r(k, 0, 64)                # |x| = 2 D: both sigmoid clamps
    tu[:k], ti[:k] = r(k, 0, 64), r(k, 0, 64)
    return su, si, tu, ti


def _cases():
    return [
        (1 << 20, 1 << 19, 128, 'adam', 0.02, 0.05, 0.01, 'zipf'),
        (1 << 19, 1 << 20, 64, 'sgd', 0.02, 0.05, 0.0, 'overlap'),
        (131072, 131072, 128, 'adam', 0.0, 0.0, 0.01, 'once_each'),
        (65536, 65536, 16, 'sgd', 0.02, 0.05, 0.01, 'once_each'),
        (4096, 3000, 64, 'adam', 0.0, 0.0, 0.0, 'overlap'),
        (20000, 30000, 64, 'adam', 0.02, 0.05, 0.0, 'far'),
        (2048, 2048, 16, 'adam', 0.02, 0.05, 0.01, 'zipf'),
    ]


@pytest.mark.parametrize('Bs,Bt,D,opt,lam,gamma,wd,shape', _cases())
def test_pair_step_vs_fp64(Bs, Bt, D, opt, lam, gamma, wd, shape):
    """Three teacher-forced steps of FusedPointPairStep against the fp64 summed loss and ONE optimizer update per touched row: every
    touched element within its bound, every other row (and its neighbours) bit-identical, the total and the four unweighted parts
    within 1e-5, each table's update count advanced once per step."""
    from recbole_cdr_amd.fused import FusedPointPairStep
    alpha = 0.3
    nu, ni = max(Bs + Bt, 4096), max((Bs + Bt) // 2, 2048)
    gen = torch.Generator(device=DEV); gen.manual_seed(Bs + 3 * Bt + D)
    U = torch.empty(nu, D, device=DEV).normal_(0, 0.1, generator=gen)
    I = torch.empty(ni, D, device=DEV).normal_(0, 0.1, generator=gen)
    if shape == 'far':
        _far_rows(U, I)
    lr = 1e-3 if opt == 'adam' else 0.5
    fs = FusedPointPairStep(U, I, Bs, Bt, alpha, lam, gamma, opt=opt, lr=lr, weight_decay=wd)
    ust, ist = fs.ustate, fs.istate
    tag = f'FusedPointPairStep {Bs}+{Bt} D={D} {opt} reg={lam},{gamma} wd={wd} {shape}'
    worst = {}
    for t in range(1, 4):
        su, si, tu, ti = _far_ids(Bs, Bt, nu, ni, gen) if shape == 'far' else _pair_ids(shape, Bs, Bt, nu, ni, gen)
        ys = (torch.rand(Bs, device=DEV, generator=gen) < 0.5).float()
        yt = (torch.rand(Bt, device=DEV, generator=gen) < 0.5).float()
        bu, bi = _snapshot(ust, opt), _snapshot(ist, opt)
        loss, parts, upart, ipart = pair_grads_fp64(bu['w'], bi['w'], [(su, si, ys, lam, alpha), (tu, ti, yt, gamma, 1 - alpha)])
        wu, wi = apply_fp64(bu, upart, D, opt, lr, wd, t), apply_fp64(bi, ipart, D, opt, lr, wd, t)
        out = fs.step(su, si, ys, tu, ti, yt)
        torch.cuda.synchronize()
        got = out[:5].tolist()
        want = [loss, parts[0][0], parts[1][0], parts[0][1], parts[1][1]]
        for j, (a, b) in enumerate(zip(got, want)):
            assert abs(a - b) <= LOSS_RTOL * abs(b) + 1e-12, f'{tag} step {t}: out[{j}] {a!r} vs fp64 {b!r}'
        assert ust.step == ist.step == t and int(ust.step_dev) == int(ist.step_dev) == t, f'{tag}: update counts'
        for name, wt in (('U', _check_table(f'{tag} step {t} U', bu, _live(ust, opt), upart[0], wu)),
                         ('I', _check_table(f'{tag} step {t} I', bi, _live(ist, opt), ipart[0], wi))):
            for k, v in wt.items():
                worst[f'{name}.{k}'] = max(worst.get(f'{name}.{k}', 0.0), v)
        del bu, bi, wu, wi, upart, ipart
    print(f'\n{tag}: worst error / bound over 3 steps: {_fmt(worst)}')


def test_two_per_domain_steps_are_a_different_optimizer():
    """The yardstick the joint step replaces: on rows that occur once in each domain, two FusedPointStep calls (one per domain) leave the
    tables measurably away from the joint step's single Adam update (which test_pair_step_vs_fp64 pins to the fp64 reference)."""
    from recbole_cdr_amd.fused import FusedPointPairStep, FusedPointStep
    B, D, nu, ni = 4096, 32, 8192, 8192
    gen = torch.Generator(device=DEV); gen.manual_seed(7)
    U = torch.empty(nu, D, device=DEV).normal_(0, 0.1, generator=gen)
    I = torch.empty(ni, D, device=DEV).normal_(0, 0.1, generator=gen)
    su, si, tu, ti = _pair_ids('once_each', B, B, nu, ni, gen)
    ys = (torch.rand(B, device=DEV, generator=gen) < 0.5).float()
    yt = (torch.rand(B, device=DEV, generator=gen) < 0.5).float()
    U2, I2 = U.clone(), I.clone()
    FusedPointPairStep(U, I, B, B, 0.5, 0.0, 0.0, opt='adam', lr=1e-3).step(su, si, ys, tu, ti, yt)
    s = FusedPointStep(U2, I2, B, loss='bce', opt='adam', lr=1e-3)
    s.step(su, si, ys)
    s.step(tu, ti, yt)
    torch.cuda.synchronize()
    assert float((U - U2).abs().max()) > 5e-4 and s.ustate.step == 2


# ---------------------------------------------------------------------------------------------------------------------- 3. the trainer

def _ids_small():
    from oracle.common import IdSpace
    return IdSpace(OU=20, TOU=15, SOU=18, OI=6, TOI=30, SOI=34)


def _host_loaders(ids, seed=0):
    """Pointwise host loaders of the BOTH phase over fixed interactions (source 96 rows, target 80: the source column wraps
    independently); ``reset()`` rewinds the negative samplers, so every run sees the same batches."""
    from recbole_cdr_amd.data import CrossDomainDataloader, OverlapDataloader, DomainTrainLoader
    from recbole_cdr_amd.utils import InputType
    rng = np.random.RandomState(seed)
    src_u = np.array(list(range(1, ids.OU)) + list(range(ids.OU + ids.TOU, ids.total_num_users)))
    src_i = np.array(list(range(1, ids.OI)) + list(range(ids.OI + ids.TOI, ids.total_num_items)))
    tgt_u, tgt_i = np.arange(1, ids.OU + ids.TOU), np.arange(1, ids.OI + ids.TOI)
    s_inter = {'source_user_id': torch.from_numpy(rng.choice(src_u, 96)), 'source_item_id': torch.from_numpy(rng.choice(src_i, 96))}
    t_inter = {'target_user_id': torch.from_numpy(rng.choice(tgt_u, 80)), 'target_item_id': torch.from_numpy(rng.choice(tgt_i, 80))}
    neg = {}

    def reset():
        neg['s'], neg['t'] = np.random.RandomState(seed + 1), np.random.RandomState(seed + 2)
    reset()
    s_sampler = lambda u, i, k: torch.from_numpy(neg['s'].choice(src_i, u.numel() * k)).to(u.device)
    t_sampler = lambda u, i, k: torch.from_numpy(neg['t'].choice(tgt_i, u.numel() * k)).to(u.device)
    mk = lambda: CrossDomainDataloader(
        DomainTrainLoader(s_inter, 'source_user_id', 'source_item_id', 'source_label', 'neg_', 24, 1, InputType.POINTWISE, s_sampler),
        DomainTrainLoader(t_inter, 'target_user_id', 'target_item_id', 'target_label', 'neg_', 32, 1, InputType.POINTWISE, t_sampler),
        OverlapDataloader(ids.OU, 8))
    return mk, reset


def _full_cfg(**kw):
    return base_config(DEV, embedding_size=16, alpha=0.3, **{'lambda': 0.02, 'gamma': 0.05}, **kw)


def _fit(cfg, ids, mk, reset, seed):
    from recbole_cdr_amd.model.cross_domain_recommender.cmf import CMF
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    torch.manual_seed(seed)
    full = _full_cfg(**cfg)
    model = CMF(full, FakeDataset(ids)).to(DEV)
    reset()
    trainer = CrossDomainTrainer(full, model)
    log = []
    orig = trainer._train_epoch
    trainer._train_epoch = lambda data, e: (log.append(orig(data, e)) or log[-1])
    trainer.fit(mk())
    torch.cuda.synchronize()
    return log, {k: v.detach().clone() for k, v in model.named_parameters()}, model


def test_exact_rowwise_trainer_matches_the_dense_adam():
    """CrossDomainTrainer over three BOTH epochs: optimizer_mode='rowwise' with rowwise_adam='exact' against optimizer_mode='dense'
    (TwoDomainPointLoss + DenseAdam over both tables) on the same model, seed and batches -- epoch losses and every parameter within the
    tolerances of the EMCDR trainer test; the lazy row-wise run is far outside them."""
    ids = _ids_small()
    lr = 0.01
    mk, reset = _host_loaders(ids)
    base = dict(learning_rate=lr, weight_decay=1e-3, train_modes=['BOTH'], epoch_num=['3'], source_split=False, eval_step=0, epochs=3)
    log_d, par_d, _ = _fit(dict(base, optimizer_mode='dense'), ids, mk, reset, 12)
    log_e, par_e, model = _fit(dict(base, optimizer_mode='rowwise', rowwise_adam='exact'), ids, mk, reset, 12)
    log_l, par_l, _ = _fit(dict(base, optimizer_mode='rowwise'), ids, mk, reset, 12)
    assert len(log_e) == 3 and all(st.exact for st in model._fused['states'].values()) and len(model._fused['states']) == 2
    steps = model._fused['states']['user_embedding'].step
    assert steps == model._fused['states']['item_embedding'].step == 3 * 5          # 80 target positives, 16 (+ 16 negatives) per batch
    assert_close(torch.tensor(log_e), torch.tensor(log_d), rtol=5e-5, what='epoch losses')
    for k in par_d:
        assert_close(par_e[k], par_d[k], rtol=1e-4, atol=lr * 5e-2, what=k)
    worst = max(float((par_l[k] - par_d[k]).abs().max()) for k in par_d)
    assert worst > 20 * lr * 5e-2, worst


# ---------------------------------------------------------------------------------------------------------------------- 4. determinism, capture

def _dataset(seed, n_s, n_t, ids):
    rng = np.random.RandomState(seed)
    src_u = np.r_[1:ids.OU, ids.OU + ids.TOU:ids.total_num_users]
    src_i = np.r_[1:ids.OI, ids.OI + ids.TOI:ids.total_num_items]
    s_pairs = np.unique(np.stack([rng.choice(src_u, n_s), rng.choice(src_i, n_s)], 1), axis=0)
    t_pairs = np.unique(np.stack([rng.randint(1, ids.OU + ids.TOU, n_t), rng.randint(1, ids.OI + ids.TOI, n_t)], 1), axis=0)
    rng.shuffle(s_pairs); rng.shuffle(t_pairs)
    return FakeDataset(ids, s_pairs, t_pairs), s_pairs, t_pairs


def _device_loaders(ids, ds, s_pairs, t_pairs, batch_s, batch_t, seed=5):
    from recbole_cdr_amd.data import CrossDomainDataloader, OverlapDataloader, DomainTrainLoader
    from recbole_cdr_amd.sampler import DeviceNegSampler
    from recbole_cdr_amd.utils import InputType
    dt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    s_smp, t_smp = DeviceNegSampler(ds, 'source', s_pairs, DEV, seed=seed), DeviceNegSampler(ds, 'target', t_pairs, DEV, seed=seed + 1)
    gen = lambda j: torch.Generator(device=DEV).manual_seed(1000 * seed + j)
    return CrossDomainDataloader(
        DomainTrainLoader({'source_user_id': dt(s_pairs[:, 0]), 'source_item_id': dt(s_pairs[:, 1])}, 'source_user_id', 'source_item_id',
                          'source_label', 'neg_', batch_s, 1, InputType.POINTWISE, s_smp, shuffle=True, generator=gen(1)),
        DomainTrainLoader({'target_user_id': dt(t_pairs[:, 0]), 'target_item_id': dt(t_pairs[:, 1])}, 'target_user_id', 'target_item_id',
                          'target_label', 'neg_', batch_t, 1, InputType.POINTWISE, t_smp, shuffle=True, generator=gen(2)),
        OverlapDataloader(ids.OU, 64, device=DEV, shuffle=True, generator=gen(3)))


@pytest.mark.parametrize('adam', ['lazy', 'exact'])
def test_rowwise_fit_is_deterministic_and_survives_capture(adam):
    """Device loaders, small batches (1,024 + 2,048 source + target positives, each with one sampled negative): two captured runs (the
    step -- and in exact mode its catch-up -- replayed as hipGraphs) are bit-equal to each other and to graph_step=False: epoch losses,
    tables, moments, update counts."""
    from oracle.common import IdSpace
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    ids = IdSpace(OU=3000, TOU=500, SOU=400, OI=200, TOI=2500, SOI=2200)
    ds, s_pairs, t_pairs = _dataset(3, 40000, 60000, ids)
    extra_cfg = dict(learning_rate=0.01, train_modes=['BOTH'], epoch_num=['2'], source_split=False, eval_step=0, epochs=2,
                     optimizer_mode='rowwise', rowwise_adam=adam)
    outs = []
    for graph in (True, True, False):
        torch.manual_seed(3)
        from recbole_cdr_amd.model.cross_domain_recommender.cmf import CMF
        cfg = dict(base_config(DEV, embedding_size=32, alpha=0.4, **{'lambda': 0.01, 'gamma': 0.02}), **extra_cfg, graph_step=graph)
        model = CMF(cfg, ds).to(DEV)
        dl = _device_loaders(ids, ds, s_pairs, t_pairs, 1024, 2048)
        trainer = CrossDomainTrainer(cfg, model)
        log = []
        orig = trainer._train_epoch
        trainer._train_epoch = lambda data, e, o=orig, l=log: (l.append(o(data, e)) or l[-1])
        trainer.fit(dl)
        torch.cuda.synchronize()
        outs.append((log, {k: v.detach().clone() for k, v in model.named_parameters()}, model.fused_optimizer_state(),
                     dict(trainer.graph_stats)))
    g1, g2, eager = outs
    assert g1[3]['captures'] >= 1 and g1[3]['replayed'] > 0 and eager[3]['replayed'] == 0, (g1[3], eager[3])
    for other in (g2, eager):
        assert other[0] == g1[0], (other[0], g1[0])
        for k in g1[1]:
            assert torch.equal(g1[1][k], other[1][k]), k
        for name in g1[2]['tables']:
            a, b = g1[2]['tables'][name], other[2]['tables'][name]
            assert a['step'] == b['step'] > 0, name
            assert torch.equal(a['exp_avg'], b['exp_avg']) and torch.equal(a['exp_avg_sq'], b['exp_avg_sq']), name


# ---------------------------------------------------------------------------------------------------------------------- 5. checkpoint

def _batch(ids, n, Bs=40, Bt=56):
    g = torch.Generator(); g.manual_seed(100 + n)
    r = lambda k, lo, hi: torch.randint(lo, hi, (k,), generator=g).to(DEV)
    return {'source_user_id': r(Bs, 1, ids.OU), 'source_item_id': r(Bs, ids.OI + ids.TOI, ids.total_num_items),
            'source_label': (torch.rand(Bs, generator=g) < 0.5).float().to(DEV),
            'target_user_id': r(Bt, 1, ids.OU + ids.TOU), 'target_item_id': r(Bt, 1, ids.OI + ids.TOI),
            'target_label': (torch.rand(Bt, generator=g) < 0.5).float().to(DEV)}


def test_exact_checkpoint_resume_is_bit_exact(tmp_path):
    """save_checkpoint after three exact-mode steps (the tables flushed to their update counts) and resume_checkpoint into a fresh model
    and trainer: the final state equals the uninterrupted run bit for bit."""
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    ids = _ids_small()
    cfg = dict(learning_rate=0.01, optimizer_mode='rowwise', rowwise_adam='exact', train_modes=['BOTH'], epoch_num=['1'],
               source_split=False, eval_step=0, epochs=1)

    def fresh():
        from recbole_cdr_amd.model.cross_domain_recommender.cmf import CMF
        torch.manual_seed(21)
        m = CMF(_full_cfg(**cfg), FakeDataset(ids)).to(DEV)
        return m, CrossDomainTrainer(_full_cfg(**cfg), m)

    run = lambda m, ns: [m.fused_train_step(_batch(ids, n), lr=0.01, adam='exact') for n in ns]
    m_a, _ = fresh()
    run(m_a, range(6))
    m_a.fused_sync()
    m_b, t_b = fresh()
    run(m_b, range(3))
    path = str(tmp_path / 'ckpt.pth')
    t_b.save_checkpoint(path, epoch=0)
    m_c, t_c = fresh()
    t_c.resume_checkpoint(path)
    assert all(st.exact and int(st.last.min()) == st.step == 3 for st in m_c._fused['states'].values())
    run(m_c, range(3, 6))
    m_c.fused_sync()
    torch.cuda.synchronize()
    for (k, pa), (_, pc) in zip(m_a.named_parameters(), m_c.named_parameters()):
        assert torch.equal(pa, pc), k
    sa, sc = m_a.fused_optimizer_state(), m_c.fused_optimizer_state()
    for name in sa['tables']:
        assert sa['tables'][name]['step'] == sc['tables'][name]['step'] == 6, name
        assert torch.equal(sa['tables'][name]['exp_avg'], sc['tables'][name]['exp_avg']), name
        assert torch.equal(sa['tables'][name]['exp_avg_sq'], sc['tables'][name]['exp_avg_sq']), name


# ---------------------------------------------------------------------------------------------------------------------- 6. refusals

def test_refusals_come_before_any_launch():
    """A batch without both domains' fields (names the phase), adam='exact' with SGD, a second Adam mode on the same tables, and
    config['dist_group'] each raise ValueError -- and leave the tables, their states and update counts untouched."""
    ids = _ids_small()
    torch.manual_seed(4)
    m = _cmf(ids)
    b = _batch(ids, 0)
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    m.set_phase('SOURCE')
    src_only = {k: v for k, v in b.items() if k.startswith('source')}
    with pytest.raises(ValueError, match='SOURCE batch has no target_user_id'):
        m.fused_train_step(src_only, lr=0.01)
    m.set_phase('BOTH')
    with pytest.raises(ValueError, match="opt='adam'"):
        m.fused_train_step(b, opt='sgd', lr=0.01, adam='exact')
    assert not m.__dict__.get('_fused', {}).get('states')
    torch.cuda.synchronize()
    for k, v in m.named_parameters():
        assert torch.equal(v, before[k]), k
    m.fused_train_step(b, lr=0.01)
    torch.cuda.synchronize()
    moved = {k: v.detach().clone() for k, v in m.named_parameters()}
    with pytest.raises(ValueError, match='one row-wise Adam mode'):
        m.fused_train_step(b, lr=0.01, adam='exact')
    torch.cuda.synchronize()
    for k, v in m.named_parameters():
        assert torch.equal(v, moved[k]), k
    assert all(st.step == 1 for st in m._fused['states'].values())
    md = _cmf(ids, dist_group=True)
    with pytest.raises(ValueError, match='dist_group'):
        md.fused_train_step(b, lr=0.01)
    assert md.fused_graph_key(b) is None and not md.__dict__.get('_fused')
    assert m.fused_graph_key(b, adam='exact') == ('cmf', 40, 56, 'exact')
    big = {'source_user_id': torch.empty(65536), 'target_user_id': torch.empty(65536)}
    assert m.fused_graph_key(big) is None
