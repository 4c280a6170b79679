"""CLFM on the O(batch) row-wise path (``optimizer_mode='rowwise'``): csrc/cdr_clfm.hip's cdr_clfm_fwd_grad (the factor map, BCE and
the three fp32-MFMA gradient contractions of one domain) and fused.FusedCLFMStep (four tables row-wise, three small weights by the exact
dense Adam).

Checked against: the reference's golden gradients (one SGD step with lr = 1 moves every parameter by -grad), the float64 restatement of
clfm_fp64.py element by element over three teacher-forced steps (its bounds are derived there and shown to bite in
test_clfm_rowwise_host.py), the dense trainer through CrossDomainTrainer with rowwise_adam='exact', and a checkpoint round trip."""
import ctypes

import pytest
import torch

from clfm_fp64 import clfm_depths, clfm_domain_fp64, clfm_weight_parts
from fp64_bounds import LOSS_RTOL, apply_fp64, ulp32
from golden_util import Golden, cases
from helpers import DEV, FakeDataset, base_config, load_params, to_dev, assert_close
from test_gpu_cmf_rowwise import _batch, _host_loaders, _ids_small
from test_gpu_step_fp64 import _check_table, _fmt, _live, _snapshot, _zipf

pytestmark = pytest.mark.gpu

TABLES = ('source_user_embedding', 'source_item_embedding', 'target_user_embedding', 'target_item_embedding')


def _clfm(ids, Du=16, Di=16, share=8, alpha=0.3, reg=0.01, **kw):
    from recbole_cdr_amd.model.cross_domain_recommender.clfm import CLFM
    cfg = base_config(DEV, user_embedding_size=Du, source_item_embedding_size=Di, target_item_embedding_size=Di, share_embedding_size=share,
                      alpha=alpha, reg_weight=reg, **kw)
    return CLFM(cfg, FakeDataset(ids)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------- 1. golden pin

@pytest.mark.parametrize('name', cases('clfm_'))
def test_one_sgd_step_moves_every_parameter_by_the_reference_gradient(name):
    """lr = 1 SGD: every parameter -- the four tables and every linear weight -- moves by -grad/BOTH of the reference (Du = 12, Di = 16,
    B_s = 20 != B_t = 27); the returned total is loss/BOTH; rows whose reference gradient is all zero keep their bits."""
    g = Golden(name)
    model = _clfm(g.idspace(), Du=int(g.meta('user_embedding_size')), Di=int(g.meta('item_embedding_size')),
                  share=int(g.meta('share_embedding_size')), alpha=float(g.meta('alpha')), reg=float(g.meta('reg_weight')))
    load_params(model, g.group('param'))
    inter = to_dev(g.group('in'), DEV)
    assert inter['source_user_id'].numel() == 20 and inter['target_user_id'].numel() == 27
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    loss = model.fused_train_step(inter, opt='sgd', lr=1.0)
    torch.cuda.synchronize()
    assert tuple(loss.shape) == (1,)
    assert_close(loss, g['loss/BOTH'], what=f'{name}: loss')
    assert len(before) == (5 if int(g.meta('share_embedding_size')) == int(g.meta('item_embedding_size')) else 7)
    for k, p in model.named_parameters():
        ref = g[f'grad/BOTH/{k}']
        moved = (before[k].double() - p.detach().double()).cpu()
        want = torch.as_tensor(ref).double()
        # the tolerance of test_gpu_cmf_rowwise.py::test_one_sgd_step_moves_every_row_by_the_reference_gradient: helpers.assert_close's
        # per-row tolerance plus one ulp of the stored fp32 row (w - g is rounded to fp32 when it is written)
        rowmax = want.abs().amax(1, keepdim=True)
        tol = 1e-5 * want.abs() + 1e-5 * torch.maximum(rowmax, 1e-2 * want.abs().max()) + ulp32(p.detach().double().cpu()) + 1e-12
        bad = (moved - want).abs() > tol
        assert not bool(bad.any()), f'{name}: {k}: {int(bad.sum())} elements off the reference gradient, e.g. {torch.nonzero(bad)[0].tolist()}'
        untouched = (torch.as_tensor(ref).to(DEV) == 0).all(1)
        assert torch.equal(p.detach()[untouched].view(torch.int32), before[k][untouched].view(torch.int32)), k
    st = model._fused['states']
    assert sorted(st) == sorted(TABLES) and all(s.step == 1 for s in st.values())


# ---------------------------------------------------------------------------------------------------------------------- 2. fp64, element by element

def _ids(shape, B, nu, ni, gen):
    r = lambda n, lo, hi: torch.randint(lo, hi, (n,), device=DEV, generator=gen)
    if shape == 'once':                                       # every user exactly once
        return torch.randperm(nu, device=DEV, generator=gen)[:B], r(B, 0, ni)
    if shape == 'zipf':                                       # one item with more than 256 occurrences, ids 0 and rows - 1 of both tables
        uid, iid = r(B, 0, nu), _zipf(B, ni, gen)
        iid[::3] = ni // 2 + 1
        uid[0], uid[1], iid[1], iid[2] = 0, nu - 1, 0, ni - 1
        return uid, iid
    if shape == 'far':                                        # the first eighth pairs a planted user with a planted item
        uid, iid = r(B, 0, nu), r(B, 64, ni)
        k = B // 8
        uid[:k], iid[:k] = r(k, 0, 64), r(k, 0, 64)
        return uid, iid
    return r(B, 0, nu), r(B, 0, ni)


def _plant_far(U, I, W):
    """As test_gpu_cmf_rowwise._far_rows, through the factor map: users 0..63 are all ones, items 0..31 / 32..63 the multiples of
    f = W 1 that score +200 / -200 with them -- far past both of BCE's clamps (the fp32 sigmoid is exactly 1 / 0 there)."""
    U[:64] = 1.0
    f = W.sum(1)
    I[:32] = 200.0 * f / (f * f).sum()
    I[32:64] = -200.0 * f / (f * f).sum()


def _wsnap(step, p, opt, clone=True):
    c = (lambda t: t.clone()) if clone else (lambda t: t)
    d = {'w': c(p.data)}
    if opt == 'adam':
        st = step.w_opt.state.get(p) or {}
        d['m'] = c(st['exp_avg']) if st else torch.zeros_like(p.data)
        d['v'] = c(st['exp_avg_sq']) if st else torch.zeros_like(p.data)
    return d


def _step_cases():
    #  Du,  Di, share,    Bs,    Bt, ids,       opt,    wd,   reg
    return [
        (12, 16, 6, 1, 33, 'uniform', 'adam', 0.0, 0.01),            # sub-tile widths, one row, ragged tile
        (64, 96, 32, 2049, 1000, 'zipf', 'sgd', 0.01, 0.01),          # unequal widths, three item tiles, long duplicate segments at both Ds
        (128, 128, 0, 4096, 4096, 'uniform', 'adam', 0.01, 0.0),      # largest LDS tile, no shared part
        (64, 64, 64, 20000, 30000, 'once', 'adam', 0.0, 0.01),        # no only-part; more tiles than resident workgroups
        (64, 64, 32, 2000, 1500, 'far', 'sgd', 0.0, 0.01),            # both BCE clamps
    ]


@pytest.mark.parametrize('Du,Di,share,Bs,Bt,shape,opt,wd,reg', _step_cases())
def test_clfm_step_vs_fp64(Du, Di, share, Bs, Bt, shape, opt, wd, reg):
    """Three teacher-forced steps of FusedCLFMStep against clfm_fp64's restatement with the kernel's real accumulation depths: the
    kernel's own outputs (every element of GU, GI and dW of both domains, the seven scalars of each out8), every element of every touched
    table row and of the three weights after ONE optimizer update within its bound, every other table row bit-identical, each table's
    update count advanced once per step; the third step rerun from the same state is bit-equal."""
    from recbole_cdr_amd import binding as B_
    from recbole_cdr_amd.fused import FusedCLFMStep
    alpha = 0.3
    nu, ni = (32768, 4096) if shape == 'once' else (64, 48) if Bt < 64 else (4096, 2048)
    gen = torch.Generator(device=DEV); gen.manual_seed(Du + 3 * Di + Bs)
    tabs = [torch.empty(n, D, device=DEV).normal_(0, 0.1, generator=gen) for n, D in ((nu, Du), (ni, Di), (nu, Du), (ni, Di))]
    xav = lambda r: torch.nn.Parameter(torch.empty(r, Du, device=DEV).normal_(0, (2.0 / (r + Du)) ** 0.5, generator=gen)) if r else None
    weights = (xav(share), xav(Di - share), xav(Di - share))
    names = ('shared', 'source_only', 'target_only')
    lr = 1e-3 if opt == 'adam' else 0.5
    fs = FusedCLFMStep(*tabs, weights, Bs, Bt, alpha, reg, opt=opt, lr=lr, weight_decay=wd)
    tag = f'FusedCLFMStep Du={Du} Di={Di} share={share} {Bs}+{Bt} {shape} {opt} wd={wd} reg={reg}'
    need = ctypes.c_size_t(0)
    grids = []
    for n in (Bs, Bt):
        B_._check(B_.load().cdr_clfm_fwd_grad_workspace_bytes(n, Du, Di, ctypes.byref(need)), 'cdr_clfm_fwd_grad_workspace_bytes')
        grids.append(need.value // (4 * Du * Di))
    if shape == 'once':
        assert -(-Bt // 32) > grids[1] >= 256, 'more tiles than workgroups: every workgroup accumulates dW over several tiles'
    worst = {}
    stack = lambda d: torch.cat([w.data for w in (weights[0], weights[1 + d]) if w is not None])

    def run(t, ids, ys, check):
        (su, si), (tu, ti) = ids
        if shape == 'far':
            for d in (0, 1):
                _plant_far(tabs[2 * d], tabs[2 * d + 1], stack(d))
        before = [_snapshot(st, opt) for st in fs.states]
        wbefore = [None if w is None else _wsnap(fs, w, opt) for w in weights]
        W = [stack(0).clone(), stack(1).clone()]
        out = fs.step(su, si, ys[0], tu, ti, ys[1])
        torch.cuda.synchronize()
        if not check:
            return out
        refs = []
        for d, (uid, iid, w) in enumerate(((su, si, alpha), (tu, ti, 1 - alpha))):
            B = uid.numel()
            ref = clfm_domain_fp64(before[2 * d]['w'], before[2 * d + 1]['w'], W[d], uid, iid, ys[d], w, reg, clfm_depths(B, Du, Di, grids[d]))
            refs.append(ref)
            got = fs.out16[8 * d:8 * d + 8].tolist()
            for j, k in enumerate(('total', 'bce', 'emb', 'nu', 'ni', 'cu', 'ci')):
                assert abs(got[j] - ref[k]) <= LOSS_RTOL * abs(ref[k]) + 1e-30, f'{tag} step {t} domain {d}: out8[{j}] ({k}) {got[j]!r} vs fp64 {ref[k]!r}'
            assert got[7] == 0.0
            if shape == 'far':
                k = B // 8
                assert bool((ref['g'].v[:k] == 0).all()) and abs(ref['bce']) > 5.0, 'the planted pairs saturate: g = 0 and -100 log clamps'
            for k, buf in (('GU', fs.GU[d][:B]), ('GI', fs.GI[d][:B]), ('dW', fs.dW[d])):
                assert bool(torch.isfinite(buf).all()), f'{tag} step {t} domain {d}: non-finite {k}'
                r = ref[k].ratio(buf)
                worst[f'{k}{d}'] = max(worst.get(f'{k}{d}', 0.0), float(r.max()))
                assert float(r.max()) <= 1.0, (f'{tag} step {t} domain {d}: {k} error / bound = {float(r.max()):.3g} at element '
                                               f'{divmod(int(r.argmax()), r.shape[1])}')
        assert abs(float(out) - (refs[0]['total'] + refs[1]['total'])) <= LOSS_RTOL * abs(refs[0]['total'] + refs[1]['total'])
        assert tuple(out.shape) == (1,)
        for j, (st, part, D) in enumerate(zip(fs.states, (refs[0]['upart'], refs[0]['ipart'], refs[1]['upart'], refs[1]['ipart']), (Du, Di, Du, Di))):
            assert st.step == t, f'{tag}: update count of {TABLES[j]}'
            wt = _check_table(f'{tag} step {t} {TABLES[j]}', before[j], _live(st, opt), part[0], apply_fp64(before[j], part, D, opt, lr, wd, t))
            for k, v in wt.items():
                worst[f'{TABLES[j][:8]}.{k}'] = max(worst.get(f'{TABLES[j][:8]}.{k}', 0.0), v)
        wparts = clfm_weight_parts(refs[0], refs[1], share)
        assert set(wparts) == {n for n, w in zip(names, weights) if w is not None}
        for n, w, wb in zip(names, weights, wbefore):
            if w is None:
                continue
            wt = _check_table(f'{tag} step {t} {n}', wb, _wsnap(fs, w, opt, clone=False), wparts[n][0], apply_fp64(wb, wparts[n], 0, opt, lr, wd, t))
            for k, v in wt.items():
                worst[f'{n}.{k}'] = max(worst.get(f'{n}.{k}', 0.0), v)
        return out

    rows_out = lambda: [fs.GU[0][:Bs], fs.GI[0][:Bs], fs.GU[1][:Bt], fs.GI[1][:Bt]]

    def draw():
        ids = (_ids(shape, Bs, nu, ni, gen), _ids(shape, Bt, nu, ni, gen))
        return ids, [(torch.rand(n, device=DEV, generator=gen) < 0.5).float() for n in (Bs, Bt)]

    for t in (1, 2):
        run(t, *draw(), check=True)
    # the third step twice from the same state: no float atomics anywhere, so every bit agrees
    saved = [_snapshot(st, opt) for st in fs.states]
    wsaved = [None if w is None else _wsnap(fs, w, opt) for w in weights]
    wsteps = None if fs.w_opt is None else [fs.w_opt.state[p]['step'].clone() for p in fs.params]
    ids, ys = draw()
    out_a = run(3, ids, ys, check=True).clone()
    first = ([{k: v.clone() for k, v in _live(st, opt).items()} for st in fs.states], [None if w is None else _wsnap(fs, w, opt) for w in weights],
             fs.out16.clone(), [x.clone() for x in rows_out()], fs.dW.clone())
    for st, sv in zip(fs.states, saved):
        for k, v in _live(st, opt).items():
            v.copy_(sv[k])
        st.step = 2
    for w, sv in zip(weights, wsaved):
        if w is not None:
            for k, v in _wsnap(fs, w, opt, clone=False).items():
                v.copy_(sv[k])
    if wsteps is not None:
        for p, s in zip(fs.params, wsteps):
            fs.w_opt.state[p]['step'].copy_(s)
    out_b = run(3, ids, ys, check=False)
    assert torch.equal(out_a, out_b) and all(st.step == 3 for st in fs.states)
    assert torch.equal(first[2].view(torch.int32), fs.out16.view(torch.int32)) and torch.equal(first[4].view(torch.int32), fs.dW.view(torch.int32))
    for a, b in zip(first[3], rows_out()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{tag}: rerun of step 3 differs in a gradient row'
    for j, st in enumerate(fs.states):
        for k, v in _live(st, opt).items():
            assert torch.equal(first[0][j][k].view(torch.int32), v.view(torch.int32)), f'{tag}: rerun of step 3 differs in {TABLES[j]}.{k}'
    for n, w, a in zip(names, weights, first[1]):
        if w is not None:
            for k, v in _wsnap(fs, w, opt, clone=False).items():
                assert torch.equal(a[k].view(torch.int32), v.view(torch.int32)), f'{tag}: rerun of step 3 differs in {n}.{k}'
    print(f'\n{tag}: worst error / bound over 3 steps: {_fmt(worst)}')


# ---------------------------------------------------------------------------------------------------------------------- 3. the trainer

def _full_cfg(**kw):
    return base_config(DEV, user_embedding_size=16, source_item_embedding_size=16, target_item_embedding_size=16, share_embedding_size=8,
                       alpha=0.3, reg_weight=0.01, **kw)


def _fit(cfg, ids, mk, reset, seed):
    from recbole_cdr_amd.model.cross_domain_recommender.clfm import CLFM
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    torch.manual_seed(seed)
    full = _full_cfg(**cfg)
    model = CLFM(full, FakeDataset(ids)).to(DEV)
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
    (DenseAdam over the four tables and the three linears) on the same model, seed and batches -- epoch losses and every parameter
    within the tolerances of test_gpu_cmf_rowwise.py::test_exact_rowwise_trainer_matches_the_dense_adam; the lazy run is outside them."""
    ids = _ids_small()
    lr = 0.01
    mk, reset = _host_loaders(ids)
    base = dict(learning_rate=lr, weight_decay=1e-3, train_modes=['BOTH'], epoch_num=['3'], source_split=False, eval_step=0, epochs=3)
    log_d, par_d, _ = _fit(dict(base, optimizer_mode='dense'), ids, mk, reset, 12)
    log_e, par_e, model = _fit(dict(base, optimizer_mode='rowwise', rowwise_adam='exact'), ids, mk, reset, 12)
    log_l, par_l, _ = _fit(dict(base, optimizer_mode='rowwise'), ids, mk, reset, 12)
    assert len(log_e) == 3 and all(st.exact for st in model._fused['states'].values()) and sorted(model._fused['states']) == sorted(TABLES)
    assert all(st.step == 3 * 5 for st in model._fused['states'].values())          # 80 target positives, 16 (+ 16 negatives) per batch
    assert len(par_d) == 7
    assert_close(torch.tensor(log_e), torch.tensor(log_d), rtol=5e-5, what='epoch losses')
    for k in par_d:
        assert_close(par_e[k], par_d[k], rtol=1e-4, atol=lr * 5e-2, what=k)
    worst = max(float((par_l[k] - par_d[k]).abs().max()) for k in par_d)
    assert worst > 20 * lr * 5e-2, worst


# ---------------------------------------------------------------------------------------------------------------------- 4. checkpoint

def test_exact_checkpoint_resume_is_bit_exact(tmp_path):
    """save_checkpoint after three exact-mode steps (the tables flushed to their update counts) and resume_checkpoint into a fresh model
    and trainer: the final state equals the uninterrupted run bit for bit -- tables, their moments and counts, the three weights and the
    weights' Adam moments and step counts."""
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    ids = _ids_small()
    cfg = dict(learning_rate=0.01, optimizer_mode='rowwise', rowwise_adam='exact', train_modes=['BOTH'], epoch_num=['1'],
               source_split=False, eval_step=0, epochs=1)

    def fresh():
        from recbole_cdr_amd.model.cross_domain_recommender.clfm import CLFM
        torch.manual_seed(21)
        m = CLFM(_full_cfg(**cfg), FakeDataset(ids)).to(DEV)
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
    assert sorted(m_c._fused['states']) == sorted(TABLES)
    assert all(st.exact and int(st.last.min()) == st.step == 3 for st in m_c._fused['states'].values())
    run(m_c, range(3, 6))
    m_c.fused_sync()
    torch.cuda.synchronize()
    for (k, pa), (_, pc) in zip(m_a.named_parameters(), m_c.named_parameters()):
        assert torch.equal(pa, pc), k
    sa, sc = m_a.fused_optimizer_state(), m_c.fused_optimizer_state()
    for name in TABLES:
        assert sa['tables'][name]['step'] == sc['tables'][name]['step'] == 6, name
        assert torch.equal(sa['tables'][name]['exp_avg'], sc['tables'][name]['exp_avg']), name
        assert torch.equal(sa['tables'][name]['exp_avg_sq'], sc['tables'][name]['exp_avg_sq']), name
    wa, wc = sa['weights']['state'], sc['weights']['state']
    assert sorted(wa) == sorted(wc) == [0, 1, 2]
    for j in wa:
        assert int(wa[j]['step']) == int(wc[j]['step']) == 6, j
        assert torch.equal(wa[j]['exp_avg'], wc[j]['exp_avg']) and torch.equal(wa[j]['exp_avg_sq'], wc[j]['exp_avg_sq']), j
        assert float(wa[j]['exp_avg'].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------- 5. refusals

def test_refusals_come_before_any_launch():
    """A batch without both domains' fields (names the phase), adam='exact' with SGD, a second Adam mode on the same tables,
    config['dist_group'] and widths the kernel rejects each raise what fused_train_step documents -- and leave the tables, their states
    and update counts and the weights untouched; the native entry refuses Du = 6, Di = 132 and B = 0 with CDR_EINVAL."""
    from recbole_cdr_amd import binding as B_
    ids = _ids_small()
    torch.manual_seed(4)
    m = _clfm(ids)
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
    assert all(not torch.equal(moved[k], before[k]) for k in moved)
    with pytest.raises(ValueError, match='one row-wise Adam mode'):
        m.fused_train_step(b, lr=0.01, adam='exact')
    torch.cuda.synchronize()
    for k, v in m.named_parameters():
        assert torch.equal(v, moved[k]), k
    assert all(st.step == 1 for st in m._fused['states'].values())
    assert all(int(st['step']) == 1 for st in m._fused['steps']['clfm'].w_opt.state.values())
    md = _clfm(ids, dist_group=True)
    with pytest.raises(NotImplementedError, match='dist_group'):
        md.fused_train_step(b, lr=0.01)
    assert not md.__dict__.get('_fused') and not hasattr(md, 'fused_graph_key')
    mw = _clfm(ids, Du=6, share=6)
    with pytest.raises(ValueError, match='user_embedding_size = 6'):
        mw.fused_train_step(b, lr=0.01)
    assert not mw.__dict__.get('_fused')
    # the native entry itself
    lib = B_.load()
    buf = torch.zeros(4096, device=DEV)
    idx = torch.zeros(8, device=DEV, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for Du, Di, n in ((6, 16, 8), (12, 132, 8), (12, 16, 0)):
        rc = lib.cdr_clfm_fwd_grad(B_.ctx(DEV), B_.stream(), p(buf), p(buf), Du, Di, p(buf), p(idx), p(idx), p(buf), n, 0.3, 0.01, p(buf), p(buf),
                                   p(buf), p(buf), p(buf), buf.numel() * 4)
        assert rc == -1 and b'cdr_clfm_fwd_grad' in lib.cdr_last_error(), (Du, Di, n, rc)
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0
