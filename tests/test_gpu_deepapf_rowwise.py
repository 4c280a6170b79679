"""DeepAPF on the O(batch) row-wise path (``optimizer_mode='rowwise'``): csrc/cdr_deepapf.hip's cdr_deepapf_fwd_grad (the two-candidate
attention of one domain forward and backward on the fp32 MFMA, three compact gradient rows per occurrence and every parameter gradient)
and fused.FusedDeepAPFStep (five tables row-wise, each advanced once per step, the share table from both batches; the four parameters by
the exact dense Adam).

Checked against: the reference's golden gradients in both overlap modes (one SGD step with lr = 1 moves every parameter by -grad), the
float64 restatement of deepapf_fp64.py element by element over three teacher-forced steps (its bounds are derived there and shown to bite
in test_deepapf_rowwise_host.py) with the third step rerun from the same state, the dense trainer through CrossDomainTrainer with
rowwise_adam='exact', and a checkpoint round trip."""
import ctypes

import pytest
import torch

from deepapf_fp64 import (ROLES, deepapf_depths, deepapf_domain_fp64, deepapf_grid, deepapf_packed, deepapf_table_parts,
                          deepapf_weight_parts, n_params)
from fp64_bounds import LOSS_RTOL, apply_fp64
from golden_util import Golden, cases
from helpers import DEV, FakeDataset, base_config, load_params, to_dev, assert_close
from test_gpu_cmf_rowwise import _batch, _host_loaders
from test_gpu_dtcdr_rowwise import _assert_moved, _wsnap
from test_gpu_step_fp64 import _check_table, _fmt, _live, _snapshot, _zipf

pytestmark = pytest.mark.gpu

USER_TABLES = ('share_user_embedding', 'source_user_embedding', 'source_item_embedding', 'target_user_embedding', 'target_item_embedding')
ITEM_TABLES = ('share_item_embedding', 'source_item_embedding', 'source_user_embedding', 'target_item_embedding', 'target_user_embedding')


def _ids_users():
    from oracle.common import IdSpace
    return IdSpace(OU=20, TOU=15, SOU=18, OI=1, TOI=30, SOI=34)


def _deepapf(ids, D=16, **kw):
    from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
    ds = FakeDataset(ids)
    ds.device = DEV
    return DeepAPF(base_config(DEV, embedding_size=D, beta=0.5, **kw), ds).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------- 1. golden pin

@pytest.mark.parametrize('name', cases('deepapf_'))
def test_one_sgd_step_moves_every_parameter_by_the_reference_gradient(name):
    """lr = 1 SGD in both overlap modes (D = 8, B_s = 20 != B_t = 27): the nine parameters with a reference gradient -- five tables, the
    mode's attention MLP, the predict layer -- move by -grad/BOTH; the four without one (the other MLP, the other side's share table) and
    every table row the batch does not name keep their bits; the returned total is loss/BOTH; every live table's update count is 1."""
    g = Golden(name)
    model = _deepapf(g.idspace(), D=int(g.meta('D')))
    load_params(model, g.group('param'))
    model.train()
    inter = to_dev(g.group('in'), DEV)
    assert inter['source_user_id'].numel() == 20 and inter['target_user_id'].numel() == 27
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    loss = model.fused_train_step(inter, opt='sgd', lr=1.0)
    torch.cuda.synchronize()
    assert tuple(loss.shape) == (1,) and len(before) == 13
    assert_close(loss, g['loss/BOTH'], what=f'{name}: loss')
    want = g.group('grad/BOTH', as_torch=False)
    assert len(want) == 9
    live = USER_TABLES if name.endswith('users') else ITEM_TABLES
    assert {k for k in want if k.endswith('embedding.weight')} == {f'{t}.weight' for t in live}
    for k, p in model.named_parameters():
        if k not in want:
            assert torch.equal(p.detach().view(torch.int32), before[k].view(torch.int32)), f'{k} has no reference gradient and moved'
            continue
        _assert_moved(k, before[k], p.detach(), want[k], name)
        if k.endswith('embedding.weight'):
            untouched = (torch.as_tensor(want[k]).to(DEV) == 0).all(1)
            assert torch.equal(p.detach()[untouched].view(torch.int32), before[k][untouched].view(torch.int32)), k
    st = model._fused['states']
    assert sorted(st) == sorted(live) and all(s.step == 1 for s in st.values())


# ---------------------------------------------------------------------------------------------------------------------- 2. fp64, element by element

def _params(D, gen):
    ps = [torch.empty(D, D, device=DEV).normal_(0, (1.0 / D) ** 0.5, generator=gen), torch.empty(D, device=DEV).normal_(0, 0.1, generator=gen),
          torch.empty(1, D, device=DEV).normal_(0, 0.5, generator=gen), torch.empty(1, D, device=DEV).normal_(0, 0.5, generator=gen)]
    return tuple(torch.nn.Parameter(p) for p in ps)


def _full_state(fs, opt):
    tabs = [{k: v.clone() for k, v in _live(st, opt).items()} for st in fs.states]
    ws = [q.data.clone() for q in fs.params]
    adam = [{k: v.clone() for k, v in fs.w_opt.state[q].items()} for q in fs.params] if fs.w_opt is not None else None
    return tabs, ws, adam, [st.step for st in fs.states]


def _restore(fs, opt, saved):
    tabs, ws, adam, steps = saved
    for st, sv, n in zip(fs.states, tabs, steps):
        for k, v in _live(st, opt).items():
            v.copy_(sv[k])
        st.step = n
    for q, w in zip(fs.params, ws):
        q.data.copy_(w)
    if adam is not None:
        for q, sv in zip(fs.params, adam):
            for k, v in fs.w_opt.state[q].items():
                v.copy_(sv[k])


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _step_cases():
    #   D,   Bs,    Bt,    opt,    wd,   ids,       mask
    return [
        (12, 1, 33, 'adam', 0.0, 'uniform', 'half'),          # a sub-tile width that is no multiple of 8, one row, a ragged tile
        (4, 64, 64, 'sgd', 0.0, 'uniform', 'half'),           # the narrowest rows, full tiles
        (96, 2049, 1000, 'sgd', 0.01, 'zipf', 'half'),        # three column tiles (9 dW1 tiles), long duplicate segments
        (128, 4096, 4096, 'adam', 0.01, 'uniform', 'half'),   # the largest LDS footprint, non-temporal row traffic
        (64, 20000, 30000, 'adam', 0.0, 'unique', 'half'),    # more tiles than resident workgroups: dW1 carried across a workgroup's tiles
        (64, 2000, 1500, 'adam', 0.0, 'planted', 'half'),     # rows that drive p to exactly 0 and 1: both BCE clamps
        (16, 40, 33, 'adam', 0.0, 'uniform', 'all'),          # every key masked
        (16, 40, 33, 'sgd', 0.0, 'uniform', 'none'),          # no key masked
        (16, 40, 33, 'adam', 0.01, 'edge', 'half'),           # keys n_overlap - 1, n_overlap, n_overlap + 1 in both batches
    ]


@pytest.mark.parametrize('case,D,Bs,Bt,opt,wd,idkind,mask', [(i,) + c for i, c in enumerate(_step_cases())])
def test_deepapf_step_vs_fp64(case, D, Bs, Bt, opt, wd, idkind, mask):
    """Three teacher-forced steps of FusedDeepAPFStep against deepapf_fp64's restatement with the kernel's real accumulation depths: the
    kernel's own outputs (every element of GS, GO and GT of both domains -- a masked occurrence's GS row +0.0 bit for bit --, of both
    packed parameter gradients and of each out8), every element of every touched row of the five tables and of the four parameters after
    ONE optimizer update within its bound, every other table row bit-identical, each table's update count advanced exactly once per
    step; the third step rerun from the same state is bit-equal.  The overlap mode alternates with the case number: it decides which id
    space (the larger or the smaller) is the key's."""
    from recbole_cdr_amd.fused import FusedDeepAPFStep
    users = case % 2 == 0
    big = Bs >= 1000
    nk, no = ((4096, 2048) if users else (2048, 4096)) if big else ((24, 20) if users else (20, 24))
    if idkind == 'unique':
        nk = 40000
    n_over = {'half': nk // 2, 'all': -1, 'none': nk}[mask]
    gen = torch.Generator(device=DEV); gen.manual_seed(100 * D + Bs + case)
    tabs = [torch.empty(n, D, device=DEV).normal_(0, 0.5, generator=gen) for n in (nk, nk, no, nk, no)]
    params = _params(D, gen)
    lr = 1e-3 if opt == 'adam' else 0.5
    fs = FusedDeepAPFStep(*tabs, params, n_over, Bs, Bt, opt=opt, lr=lr, weight_decay=wd)
    tag = f'FusedDeepAPFStep {"users" if users else "items"} D={D} {Bs}+{Bt} {opt} wd={wd} {idkind} mask={mask}'
    grids = [deepapf_grid(n, D) for n in (Bs, Bt)]
    assert fs.n_params == n_params(D) and [fs.grid(Bs), fs.grid(Bt)] == grids
    assert fs.fws.numel() == max(grids) * 4 * n_params(D)
    if idkind == 'unique':
        assert Bs > 32 * grids[0] and Bt > 32 * grids[1], 'more tiles than workgroups: a workgroup walks several tiles and carries dW1 across them'
    worst = {}
    r = lambda n, hi: torch.randint(0, hi, (n,), device=DEV, generator=gen)

    for t in (1, 2, 3):
        if idkind == 'unique':
            ks, kt = torch.randperm(nk, device=DEV, generator=gen)[:Bs], torch.randperm(nk, device=DEV, generator=gen)[:Bt]
        elif idkind == 'zipf':
            ks, kt = _zipf(Bs, nk, gen), _zipf(Bt, nk, gen)
            ks[:300] = 5; ks[300], ks[301] = 0, nk - 1; kt[0], kt[1], kt[2] = 0, nk - 1, 5
        else:
            ks, kt = r(Bs, nk), r(Bt, nk)
        os_, ot = r(Bs, no), r(Bt, no)
        if idkind == 'zipf':
            os_[0], os_[1] = 0, no - 1
        if idkind == 'edge':
            for k in (ks, kt):
                k[:3] = torch.tensor([n_over - 1, n_over, n_over + 1], device=DEV)
        ys = [(torch.rand(n, device=DEV, generator=gen) < 0.5).float() for n in (Bs, Bt)]
        if idkind == 'planted':
            # key row 3 (not masked) and key row nk - 1 (masked) against other rows 1 (p = 1) and 2 (p = 0): z = +-100 sum|wp|
            sg = torch.sign(params[3].data.reshape(-1))
            for tb in (tabs[0], tabs[1], tabs[3]):
                tb[3] = 10.0 * sg; tb[nk - 1] = 10.0 * sg
            for tb in (tabs[2], tabs[4]):
                tb[1] = 10.0; tb[2] = -10.0
            for k, o, y in ((ks, os_, ys[0]), (kt, ot, ys[1])):
                k[:4] = torch.tensor([3, 3, nk - 1, nk - 1], device=DEV)
                o[:4] = torch.tensor([1, 2, 1, 2], device=DEV)
                y[:4] = torch.tensor([0.0, 1.0, 1.0, 0.0], device=DEV)
            assert 100.0 * float(params[3].data.abs().sum()) > 1000.0
        before = [_snapshot(st, opt) for st in fs.states]
        wbefore = [_wsnap(fs, q, opt) for q in params]
        p_before = [q.data.clone() for q in params]
        saved = _full_state(fs, opt) if t == 3 else None
        out = fs.step(ks, os_, ys[0], kt, ot, ys[1])
        torch.cuda.synchronize()
        refs = []
        for d, (key, oid, row0) in enumerate(((ks, os_, 0), (kt, ot, Bs))):
            B = key.numel()
            ref = deepapf_domain_fp64(before[0]['w'], before[1 + 2 * d]['w'], before[2 + 2 * d]['w'], p_before, key, oid, ys[d], n_over, 1.0,
                                      deepapf_depths(B, D, grids[d]))
            refs.append(ref)
            got = fs.out16[8 * d:8 * d + 8].tolist()
            for j, k in enumerate(('total', 'bce')):
                assert abs(got[j] - ref[k]) <= LOSS_RTOL * abs(ref[k]) + 1e-30, f'{tag} step {t} domain {d}: out8[{j}] ({k}) {got[j]!r} vs fp64 {ref[k]!r}'
            assert got[2:] == [0.0] * 6
            for name, buf in (('GS', fs.GS[row0:row0 + B]), ('GO', fs.GO[d][:B]), ('GT', fs.GT[d][:B])):
                assert bool(torch.isfinite(buf).all()), f'{tag} step {t} domain {d}: non-finite rows in {name}'
                ratio = ref[name].ratio(buf)
                worst[name] = max(worst.get(name, 0.0), float(ratio.max()))
                assert float(ratio.max()) <= 1.0, (f'{tag} step {t} domain {d}: {name}: error / bound = {float(ratio.max()):.3g} at '
                                                   f'element {divmod(int(ratio.argmax()), D)}')
            masked = key > n_over
            assert bool((ref['masked'] == masked).all()) and int(masked.sum()) == {'all': B, 'none': 0}.get(mask, int(masked.sum()))
            gs = fs.GS[row0:row0 + B]
            assert bool((gs.view(torch.int32)[masked] == 0).all()), f'{tag} step {t} domain {d}: a masked occurrence\'s GS row is not +0.0'
            if idkind == 'edge':
                assert masked[:3].tolist() == [False, False, True] and bool((gs[1] != 0).any()), 'key == n_overlap keeps its share row'
            if idkind == 'planted':
                # p is exactly 1 or 0 there, in fp32 and in fp64: the -100 clamp of the loss and the 1e-12 clamp of the backward (g = 0)
                assert bool((ref['g'].v[:4] == 0).all()) and ref['bce'] > 100.0 * 2 / B
                assert bool((fs.GT[d][:4] == 0).all()) and bool((fs.GO[d][:4] == 0).all()), 'the planted rows saturate: both clamps are taken'
            ratio = deepapf_packed(ref).ratio(fs.dP[d])
            worst[f'dP{d}'] = max(worst.get(f'dP{d}', 0.0), float(ratio.max()))
            assert bool(torch.isfinite(fs.dP[d]).all()) and float(ratio.max()) <= 1.0, \
                f'{tag} step {t} domain {d}: packed parameter gradient: error / bound = {float(ratio.max()):.3g} at element {int(ratio.argmax())}'
        total = refs[0]['total'] + refs[1]['total']
        assert tuple(out.shape) == (1,) and abs(float(out) - total) <= LOSS_RTOL * abs(total)
        parts = deepapf_table_parts(refs[0], refs[1], ks, os_, kt, ot)
        for j, (st, role) in enumerate(zip(fs.states, ROLES)):
            assert st.step == t, f'{tag}: update count of {role} after step {t}: {st.step}'
            wt = _check_table(f'{tag} step {t} {role}', before[j], _live(st, opt), parts[role][0], apply_fp64(before[j], parts[role], D, opt, lr, wd, t))
            for k, v in wt.items():
                worst[f'{role}.{k}'] = max(worst.get(f'{role}.{k}', 0.0), v)
        for j, (q, wb, part) in enumerate(zip(params, wbefore, deepapf_weight_parts(refs[0], refs[1]))):
            wt = _check_table(f'{tag} step {t} parameter {j}', wb, _wsnap(fs, q, opt, clone=False), part[0], apply_fp64(wb, part, 0, opt, lr, wd, t))
            for k, v in wt.items():
                worst[f'param.{k}'] = max(worst.get(f'param.{k}', 0.0), v)
        if t == 3:                                           # the same step from the same state: bit-equal
            first = _full_state(fs, opt) + (fs.GS.clone(), [g.clone() for g in fs.GO + fs.GT], fs.dP.clone(), fs.out16.clone(), out.clone())
            _restore(fs, opt, saved)
            out_b = fs.step(ks, os_, ys[0], kt, ot, ys[1])
            torch.cuda.synchronize()
            second = _full_state(fs, opt)
            n = Bs + Bt
            assert _bits(first[8], out_b) and second[3] == [3] * 5
            for role, a, b in zip(ROLES, first[0], second[0]):
                assert all(_bits(a[k], b[k]) for k in a), f'{tag}: the rerun differs in {role}'
            assert all(_bits(a, b) for a, b in zip(first[1], second[1])), f'{tag}: the rerun differs in a parameter'
            if opt == 'adam':
                assert all(torch.equal(a[k], b[k]) for a, b in zip(first[2], second[2]) for k in a), f'{tag}: the rerun differs in the Adam state'
            assert _bits(first[4][:n], fs.GS[:n]) and _bits(first[6], fs.dP) and _bits(first[7], fs.out16)
            for (a, b), m in zip(zip(first[5], fs.GO + fs.GT), (Bs, Bt, Bs, Bt)):
                assert _bits(a[:m], b[:m]), f'{tag}: the rerun differs in a gradient-row buffer'
    if idkind in ('edge', 'zipf', 'planted'):
        assert bool(torch.isin(ks, kt).any()), 'a key named by both domains: ONE update of its share row from the sum (the share table advanced once per step)'
    if idkind == 'zipf':
        assert int(torch.bincount(ks).max()) > 256
    print(f'\n{tag}: worst error / bound over 3 steps: {_fmt(worst)} | overall {max(worst.values()):.3g}')


# ---------------------------------------------------------------------------------------------------------------------- 3. the trainer

def _fit(cfg, ids, mk, reset, seed):
    from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    torch.manual_seed(seed)
    full = base_config(DEV, embedding_size=16, beta=0.5, **cfg)
    model = DeepAPF(full, FakeDataset(ids)).to(DEV)
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
    (DenseAdam over every parameter with a gradient) on the same model, seed and batches -- epoch losses and every parameter within the
    tolerances of test_gpu_cmf_rowwise.py::test_exact_rowwise_trainer_matches_the_dense_adam (as the CLFM and DTCDR tests); the
    parameters without a gradient do not move in either; the lazy run is outside those tolerances."""
    ids = _ids_users()
    lr = 0.01
    mk, reset = _host_loaders(ids)
    base = dict(learning_rate=lr, weight_decay=1e-3, train_modes=['BOTH'], epoch_num=['3'], source_split=False, eval_step=0, epochs=3)
    log_d, par_d, _ = _fit(dict(base, optimizer_mode='dense'), ids, mk, reset, 12)
    log_e, par_e, model = _fit(dict(base, optimizer_mode='rowwise', rowwise_adam='exact'), ids, mk, reset, 12)
    log_l, par_l, _ = _fit(dict(base, optimizer_mode='rowwise'), ids, mk, reset, 12)
    assert len(log_e) == 3 and all(st.exact for st in model._fused['states'].values()) and sorted(model._fused['states']) == sorted(USER_TABLES)
    assert all(st.step == 3 * 5 for st in model._fused['states'].values())          # 80 target positives, 16 (+ 16 negatives) per batch
    assert len(par_d) == 13
    assert_close(torch.tensor(log_e), torch.tensor(log_d), rtol=5e-5, what='epoch losses')
    for k in par_d:
        assert_close(par_e[k], par_d[k], rtol=1e-4, atol=lr * 5e-2, what=k)
    worst = max(float((par_l[k] - par_d[k]).abs().max()) for k in par_d)
    assert worst > lr * 5e-2, worst


# ---------------------------------------------------------------------------------------------------------------------- 4. checkpoint

def test_exact_checkpoint_resume_is_bit_exact(tmp_path):
    """save_checkpoint after three exact-mode steps (the tables flushed to their update counts) and resume_checkpoint into a fresh model
    and trainer, two more steps: the final state equals the uninterrupted run bit for bit -- tables, their moments and counts, the four
    parameters with their Adam moments and step counts."""
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    ids = _ids_users()
    cfg = dict(learning_rate=0.01, optimizer_mode='rowwise', rowwise_adam='exact', train_modes=['BOTH'], epoch_num=['1'],
               source_split=False, eval_step=0, epochs=1)

    def fresh():
        from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
        torch.manual_seed(21)
        full = base_config(DEV, embedding_size=16, beta=0.5, **cfg)
        m = DeepAPF(full, FakeDataset(ids)).to(DEV)
        m.train()
        return m, CrossDomainTrainer(full, m)

    def run(m, ns):
        for n in ns:
            m.fused_train_step(_batch(ids, n), lr=0.01, adam='exact')

    m_a, _ = fresh()
    run(m_a, range(5))
    m_a.fused_sync()
    m_b, t_b = fresh()
    run(m_b, range(3))
    path = str(tmp_path / 'ckpt.pth')
    t_b.save_checkpoint(path, epoch=0)
    m_c, t_c = fresh()
    t_c.resume_checkpoint(path)
    assert sorted(m_c._fused['states']) == sorted(USER_TABLES)
    assert all(st.exact and int(st.last.min()) == st.step == 3 for st in m_c._fused['states'].values())
    run(m_c, range(3, 5))
    m_c.fused_sync()
    torch.cuda.synchronize()
    for (k, pa), (_, pc) in zip(m_a.named_parameters(), m_c.named_parameters()):
        assert torch.equal(pa, pc), k
    sa, sc = m_a.fused_optimizer_state(), m_c.fused_optimizer_state()
    for name in USER_TABLES:
        assert sa['tables'][name]['step'] == sc['tables'][name]['step'] == 5, name
        assert torch.equal(sa['tables'][name]['exp_avg'], sc['tables'][name]['exp_avg']), name
        assert torch.equal(sa['tables'][name]['exp_avg_sq'], sc['tables'][name]['exp_avg_sq']), name
    wa, wc = sa['weights']['state'], sc['weights']['state']
    assert sorted(wa) == sorted(wc) == list(range(4))
    for j in wa:
        assert int(wa[j]['step']) == int(wc[j]['step']) == 5, j
        assert torch.equal(wa[j]['exp_avg'], wc[j]['exp_avg']) and torch.equal(wa[j]['exp_avg_sq'], wc[j]['exp_avg_sq']), j
        assert float(wa[j]['exp_avg'].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------- 5. refusals

def test_refusals_come_before_any_launch():
    """A batch without both domains' fields (names the phase), adam='exact' with SGD, empty and unequal-length batches, a second Adam
    mode on a model already trained with the other, config['dist_group'] and widths the kernel rejects each raise what fused_train_step
    documents -- and leave the tables, their states and update counts and the parameters untouched; the native entry refuses D = 6,
    D = 132, D = 0, D = 2 and B = 0 with CDR_EINVAL."""
    from recbole_cdr_amd import binding as B_
    ids = _ids_users()
    torch.manual_seed(4)
    m = _deepapf(ids)
    b = _batch(ids, 0)
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    m.set_phase('SOURCE')
    src_only = {k: v for k, v in b.items() if k.startswith('source')}
    with pytest.raises(ValueError, match='SOURCE batch has no target_user_id'):
        m.fused_train_step(src_only, lr=0.01)
    m.set_phase('BOTH')
    with pytest.raises(ValueError, match="opt='adam'"):
        m.fused_train_step(b, opt='sgd', lr=0.01, adam='exact')
    with pytest.raises(ValueError, match='at least one row per domain'):
        m.fused_train_step(dict(b, target_user_id=b['target_user_id'][:0], target_item_id=b['target_item_id'][:0], target_label=b['target_label'][:0]))
    with pytest.raises(ValueError, match='ids and labels of equal length'):
        m.fused_train_step(dict(b, source_label=b['source_label'][:3]))
    assert '_fused' not in m.__dict__
    torch.cuda.synchronize()
    for k, v in m.named_parameters():
        assert torch.equal(v, before[k]), k
    m.fused_train_step(b, lr=0.01)
    torch.cuda.synchronize()
    moved = {k: v.detach().clone() for k, v in m.named_parameters()}
    live = {f'{t}.weight' for t in USER_TABLES} | {'user_mlp.0.weight', 'user_mlp.0.bias', 'user_mlp.2.weight', 'predict_layer.weight'}
    assert {k for k in moved if not torch.equal(moved[k], before[k])} == live
    with pytest.raises(ValueError, match='one row-wise Adam mode'):
        m.fused_train_step(b, lr=0.01, adam='exact')
    torch.cuda.synchronize()
    for k, v in m.named_parameters():
        assert torch.equal(v, moved[k]), k
    assert all(st.step == 1 for st in m._fused['states'].values())
    assert all(int(st['step']) == 1 for st in m._fused['steps']['deepapf'].w_opt.state.values())
    md = _deepapf(ids, dist_group=True)
    with pytest.raises(NotImplementedError, match='dist_group'):
        md.fused_train_step(b, lr=0.01)
    assert '_fused' not in md.__dict__ and not hasattr(md, 'fused_graph_key')
    for D in (6, 132):
        mw = _deepapf(ids, D=D)
        with pytest.raises(ValueError, match=f'embedding_size = {D}.*optimizer_mode=dense'):
            mw.fused_train_step(b, lr=0.01)
        assert '_fused' not in mw.__dict__
    # the native entry itself
    lib = B_.load()
    buf = torch.zeros(1 << 16, device=DEV)
    idx = torch.zeros(8, device=DEV, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for D, n in ((6, 8), (132, 8), (0, 8), (2, 8), (8, 0)):
        rc = lib.cdr_deepapf_fwd_grad(B_.ctx(DEV), B_.stream(), p(buf), p(buf), p(buf), D, p(buf), p(idx), p(idx), p(buf), n, 2, 1.0, 0, p(buf),
                                      p(buf), p(buf), p(buf), p(buf), p(buf), buf.numel() * 4)
        assert rc == -1 and b'cdr_deepapf_fwd_grad' in lib.cdr_last_error(), (D, n, rc)
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0
