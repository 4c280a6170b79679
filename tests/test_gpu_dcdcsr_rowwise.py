"""DCDCSR on the O(batch) row-wise path (``optimizer_mode='rowwise'``): csrc/cdr_dcdcsr.hip's cdr_dcdcsr_map_fwd_grad (the max-min
normalisation, the tanh MLP, the MSE and the whole backward with the even tie split on the fp32 MFMA, one gradient row per occurrence and
every parameter gradient), fused.FusedDCDCSRMapStep (the unit table row-wise, the MLP by the exact dense Adam) and
fused.FusedFrozenSideBPRStep (the second TARGET visit: the affine table read only).

Checked against: the reference's golden gradients of all four stages in both overlap modes (one SGD step with lr = 1 moves every parameter
by -grad), the float64 restatement of dcdcsr_fp64.py element by element over three teacher-forced steps (its bounds are derived there and
shown to bite in test_dcdcsr_rowwise_host.py) with the third step rerun from the same state, fp64_bounds.bpr_grads_fp64 for the
frozen-side step, the dense trainer through DCDCSRTrainer with rowwise_adam='exact', a checkpoint round trip, the refusals, and the
step's peak memory."""
import ctypes

import numpy as np
import pytest
import torch

from dcdcsr_fp64 import (dcdcsr_depths, dcdcsr_grid, dcdcsr_map_fp64, dcdcsr_packed, dcdcsr_table_part, dcdcsr_weight_parts, n_params)
from fp64_bounds import LOSS_RTOL, apply_fp64, bpr_grads_fp64
from golden_util import Golden, cases
from helpers import DEV, FakeDataset, base_config, load_params, to_dev, assert_close
from test_gpu_dtcdr_rowwise import _assert_moved, _wsnap
from test_gpu_models5 import _loaders
from test_gpu_step_fp64 import _check_table, _fmt, _live, _snapshot

pytestmark = pytest.mark.gpu


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------- 1. golden pin

@pytest.mark.parametrize('name', cases('dcdcsr_'))
def test_one_sgd_step_per_stage_moves_every_parameter_by_the_reference_gradient(name):
    """lr = 1 SGD in both overlap modes (D = 8, hidden [12], map_batch_size 9), the stages SOURCE, TARGET, BOTH and TARGET2 in order with
    ``set_phase``, the golden parameters reloaded after each stage's step (and the row-wise state dropped, so that a stage's states are
    the tables it updated): every parameter in grad/<stage> moves by -grad, the returned loss is loss/<stage>; every parameter without a
    reference gradient in that stage, every row the batch does not name and the affine table keep their bits; only the tables with a
    gradient have a state, with update count 1."""
    from recbole_cdr_amd.model.cross_domain_recommender.dcdcsr import DCDCSR
    g = Golden(name)
    ds = FakeDataset(g.idspace(), g['aux/s_pairs'], g['aux/t_pairs'])
    ds.device = DEV
    cfg = base_config(DEV, latent_factor_model='BPR', embedding_size=int(g.meta('D')), mlp_hidden_size=[int(x) for x in g.meta('mlp_hidden_size')],
                      k=int(g.meta('k')), map_batch_size=int(g.meta('map_batch_size')))
    model = DCDCSR(cfg, ds).to(DEV)
    inter = to_dev(g.group('in'), DEV)
    assert int(g.meta('D')) == 8 and int(g.meta('map_batch_size')) == 9
    unit = 'user' if name.endswith('users') else 'item'
    other = 'item' if unit == 'user' else 'user'
    tables_of = {'SOURCE': {'source_user_embedding', 'source_item_embedding'}, 'TARGET': {'target_user_embedding', 'target_item_embedding'},
                 'BOTH': {f'target_{unit}_embedding'}, 'TARGET2': {f'target_{other}_embedding'}}
    for phase, tag in (('SOURCE', 'SOURCE'), ('TARGET', 'TARGET'), ('BOTH', 'BOTH'), ('TARGET', 'TARGET2')):
        load_params(model, g.group('param'))
        model.set_phase(phase)
        if phase == 'BOTH':
            assert_close(model.benchmark_embedding, g['fwd/benchmark_embedding'], what='benchmark')
            np.random.seed(77)
        affine = None
        if tag == 'TARGET2':
            assert_close(model.affine_embedding, g['fwd/affine_embedding'], what='affine')
            affine = model.affine_embedding.clone()
        before = {k: v.detach().clone() for k, v in model.named_parameters()}
        loss = model.fused_train_step(inter, opt='sgd', lr=1.0)
        torch.cuda.synchronize()
        assert_close(loss.reshape(()), g[f'loss/{tag}'], what=f'{name}: {tag}: loss')
        want = g.group(f'grad/{tag}', as_torch=False)
        mlp = {k for k in before if k.startswith('mapping_mlp_layers')}
        assert len(mlp) == 4 and set(want) == {f'{t}.weight' for t in tables_of[tag]} | (mlp if tag == 'BOTH' else set()), (tag, sorted(want))
        for k, p in model.named_parameters():
            if k not in want:
                assert _bits(p.detach(), before[k]), f'{tag}: {k} has no reference gradient and moved'
                continue
            _assert_moved(k, before[k], p.detach(), want[k], f'{name}: {tag}')
            if k.endswith('embedding.weight'):
                untouched = (torch.as_tensor(want[k]).to(DEV) == 0).all(1)
                assert bool(untouched.any()) and _bits(p.detach()[untouched], before[k][untouched]), (tag, k)
        if affine is not None:
            assert _bits(model.affine_embedding, affine), 'the affine table is read only'
        st = model._fused['states']
        assert set(st) == tables_of[tag] and all(s.step == 1 for s in st.values()), (tag, {k: s.step for k, s in st.items()})
        del model.__dict__['_fused']


# ---------------------------------------------------------------------------------------------------------------------- 2. fp64, element by element

def _layers(dims, gen):
    out = []
    for l in range(len(dims) - 1):
        W = torch.empty(dims[l + 1], dims[l], device=DEV).normal_(0, (1.0 / dims[l]) ** 0.5, generator=gen)
        b = torch.empty(dims[l + 1], device=DEV).normal_(0, 0.1, generator=gen)
        out.append((torch.nn.Parameter(W), torch.nn.Parameter(b)))
    return out


def _plant_ties(T):
    """Row 3: two tied maxima; row 5: two tied minima (an update breaks a tie: planted again before every step)."""
    D = T.shape[1]
    T[3, D - 1] = T[3, 1] = T[3].max() + 0.25
    T[5, 0] = T[5, D - 2] = T[5].min() - 0.25


def _full_state(fs, opt):
    tab = {k: v.clone() for k, v in _live(fs.state, opt).items()}
    ws = [q.data.clone() for q in fs.params]
    adam = [{k: v.clone() for k, v in fs.w_opt.state[q].items()} for q in fs.params] if fs.w_opt is not None else None
    return tab, ws, adam, fs.state.step


def _restore(fs, opt, saved):
    tab, ws, adam, step = saved
    for k, v in _live(fs.state, opt).items():
        v.copy_(tab[k])
    fs.state.step = step
    for q, w in zip(fs.params, ws):
        q.data.copy_(w)
    if adam is not None:
        for q, sv in zip(fs.params, adam):
            for k, v in fs.w_opt.state[q].items():
                v.copy_(sv[k])


def _map_cases():
    #   n,      dims,              ids,        opt,    wd
    return [
        (1, (4, 4), 'repeat', 'adam', 0.0),                   # one occurrence, the narrowest rows, one layer
        (9, (8, 12, 8), 'repeat', 'sgd', 0.01),               # the fixtures' shape
        (33, (8, 12, 8), 'equal', 'adam', 0.0),               # ONE id 33 times: a segment one beyond the apply's 32-occurrence cut
        (33, (64, 128, 64), 'distinct', 'adam', 0.01),        # the default shape (weights in LDS, 16 dW tiles), a tile and one row
        (70, (64, 128, 64), 'repeat', 'sgd', 0.0),            # three tiles, the last ragged
        (70, (128, 128, 128), 'repeat', 'adam', 0.0),         # the widest rows: the weight operand through L2, 32 dW tiles
        (9, (128, 128, 128), 'distinct', 'sgd', 0.01),
        (70, (8, 12, 16, 8), 'repeat', 'adam', 0.01),         # three layers, widths that are no multiples of 8 or 32
        (33, (8, 12, 16, 8), 'distinct', 'sgd', 0.0),
        ('grid', (8, 12, 8), 'repeat', 'adam', 0.0),          # n = 32 grid + 1: a workgroup walks two tiles and carries dW across them
    ]


@pytest.mark.parametrize('case,n,dims,idkind,opt,wd', [(i,) + c for i, c in enumerate(_map_cases())])
def test_dcdcsr_map_step_vs_fp64(case, n, dims, idkind, opt, wd):
    """Three teacher-forced steps of FusedDCDCSRMapStep against dcdcsr_fp64's restatement with the kernel's real accumulation depths: the
    kernel's own outputs (every element of G, of the packed parameter gradient and of out8), every element of every touched row of the
    table and of every MLP parameter after ONE optimizer update within its bound, every other table row bit-identical, the update count
    advanced once per step; the third step rerun from the same state is bit-equal.  Rows with two tied maxima and two tied minima are in
    every batch."""
    from recbole_cdr_amd.fused import FusedDCDCSRMapStep
    dims = list(dims)
    D = dims[0]
    if n == 'grid':
        n = 32 * dcdcsr_grid(1 << 20, dims) + 1
    rows = 4096 if n > 1000 else 96
    gen = torch.Generator(device=DEV); gen.manual_seed(1000 * case + D + n)
    T = torch.empty(rows, D, device=DEV).normal_(0, 0.5, generator=gen)
    bench = torch.empty(rows, D, device=DEV).normal_(0, 0.5, generator=gen)
    layers = _layers(dims, gen)
    params = [q for pair in layers for q in pair]
    lr = 1e-3 if opt == 'adam' else 0.5
    fs = FusedDCDCSRMapStep(T, bench, layers, n, opt=opt, lr=lr, weight_decay=wd)
    tag = f'FusedDCDCSRMapStep n={n} dims={dims} {idkind} {opt} wd={wd}'
    grid = dcdcsr_grid(n, dims)
    assert fs.n_params == n_params(dims) and fs.grid(n) == grid and fs.fws.numel() == grid * 4 * n_params(dims)
    if n > 1000:
        assert n == 32 * grid + 1, 'one more tile than workgroups'
    worst = {}
    for t in (1, 2, 3):
        _plant_ties(T)
        if idkind == 'equal':
            idx = torch.full((n,), 3, device=DEV, dtype=torch.int64)
        elif idkind == 'distinct':
            idx = torch.randperm(rows, device=DEV, generator=gen)[:n]
            for j, r in enumerate((3, 5)):
                if j < n and not bool((idx == r).any()):
                    idx[j] = r
            assert idx.unique().numel() == n
        else:
            idx = torch.randint(0, rows, (n,), device=DEV, generator=gen)
            idx[0] = 3
            if n > 1:
                idx[n - 1] = 5
            if n >= 9:
                idx[4] = idx[2]; idx[7] = 3                  # repeats, the tied-maximum row among them
        before = _snapshot(fs.state, opt)
        wbefore = [_wsnap(fs, q, opt) for q in params]
        p_before = [q.data.clone() for q in params]
        saved = _full_state(fs, opt) if t == 3 else None
        out = fs.step(idx)
        torch.cuda.synchronize()
        ref = dcdcsr_map_fp64(before['w'], bench, p_before, idx, dcdcsr_depths(n, dims, grid))
        nmax, nmin = ref['ties']
        assert int(nmax.max()) == 2 and (n == 1 or idkind == 'equal' or int(nmin.max()) == 2), 'the planted ties are in the batch'
        got = fs.out8.tolist()
        assert abs(got[0] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-30, f'{tag} step {t}: out8[0] {got[0]!r} vs fp64 {ref["loss"]!r}'
        assert got[1:] == [0.0] * 7 and out.dim() == 0 and float(out) == got[0]
        G = fs.G[:n]
        assert bool(torch.isfinite(G).all()), f'{tag} step {t}: non-finite rows in G'
        ratio = ref['G'].ratio(G)
        worst['G'] = max(worst.get('G', 0.0), float(ratio.max()))
        assert float(ratio.max()) <= 1.0, f'{tag} step {t}: G: error / bound = {float(ratio.max()):.3g} at element {divmod(int(ratio.argmax()), D)}'
        ratio = dcdcsr_packed(ref).ratio(fs.dP)
        worst['dP'] = max(worst.get('dP', 0.0), float(ratio.max()))
        assert bool(torch.isfinite(fs.dP).all()) and float(ratio.max()) <= 1.0, \
            f'{tag} step {t}: packed parameter gradient: error / bound = {float(ratio.max()):.3g} at element {int(ratio.argmax())}'
        assert fs.state.step == t, f'{tag}: update count after step {t}: {fs.state.step}'
        part = dcdcsr_table_part(ref, idx)
        wt = _check_table(f'{tag} step {t} table', before, _live(fs.state, opt), part[0], apply_fp64(before, part, D, opt, lr, wd, t))
        for k, v in wt.items():
            worst[f'table.{k}'] = max(worst.get(f'table.{k}', 0.0), v)
        for j, (q, wb, wpart) in enumerate(zip(params, wbefore, dcdcsr_weight_parts(ref))):
            wt = _check_table(f'{tag} step {t} parameter {j}', wb, _wsnap(fs, q, opt, clone=False), wpart[0], apply_fp64(wb, wpart, 0, opt, lr, wd, t))
            for k, v in wt.items():
                worst[f'param.{k}'] = max(worst.get(f'param.{k}', 0.0), v)
        if t == 3:                                           # the same step from the same state: bit-equal
            first = _full_state(fs, opt) + (fs.G[:n].clone(), fs.dP.clone(), fs.out8.clone())
            _restore(fs, opt, saved)
            fs.step(idx)
            torch.cuda.synchronize()
            second = _full_state(fs, opt)
            assert second[3] == 3 and all(_bits(first[0][k], second[0][k]) for k in first[0]), f'{tag}: the rerun differs in the table'
            assert all(_bits(a, b) for a, b in zip(first[1], second[1])), f'{tag}: the rerun differs in a parameter'
            if opt == 'adam':
                assert all(torch.equal(a[k], b[k]) for a, b in zip(first[2], second[2]) for k in a), f'{tag}: the rerun differs in the Adam state'
            assert _bits(first[4], fs.G[:n]) and _bits(first[5], fs.dP) and _bits(first[6], fs.out8)
    print(f'\n{tag}: worst error / bound over 3 steps: {_fmt(worst)} | overall {max(worst.values()):.3g}')


# ---------------------------------------------------------------------------------------------------------------------- 3. the frozen-side step

@pytest.mark.parametrize('frozen', ['user', 'item'])
@pytest.mark.parametrize('B,D', [(1, 8), (33, 64), (70, 8), (70, 64)])
def test_frozen_side_step_vs_fp64(frozen, B, D):
    """Three steps of FusedFrozenSideBPRStep against fp64_bounds.bpr_grads_fp64 (reg 0) and apply_fp64: the loss, every touched row of the
    trained table within its bound, every other row bit-identical; the frozen operand keeps its bits and has no state.  The frozen operand
    has fewer rows than the table it stands in for (10 against 36, as the users fixture's target_num_users against total_num_users); ids
    repeat."""
    from recbole_cdr_amd.fused import FusedFrozenSideBPRStep
    gen = torch.Generator(device=DEV); gen.manual_seed(10 * B + D + (frozen == 'user'))
    n_frozen, n_full, n_other = 10, 36, 30
    affine = torch.empty(n_frozen, D, device=DEV).normal_(0, 0.3, generator=gen)
    trained = torch.empty(n_other, D, device=DEV).normal_(0, 0.3, generator=gen)
    full = torch.empty(n_full, D, device=DEV).normal_(0, 0.3, generator=gen)        # the table the affine operand stands in for: untouched
    U, I = (affine, trained) if frozen == 'user' else (trained, affine)
    for opt, wd in (('adam', 0.01), ('sgd', 0.0)):
        lr = 1e-3 if opt == 'adam' else 0.5
        fs = FusedFrozenSideBPRStep(U, I, frozen, B, opt=opt, lr=lr, weight_decay=wd)
        assert fs._states() == (fs.state,) and fs.state.table is trained
        a0, f0 = affine.clone(), full.clone()
        tag = f'FusedFrozenSideBPRStep frozen={frozen} B={B} D={D} {opt}'
        worst = {}
        for t in (1, 2, 3):
            r = lambda hi: torch.randint(0, hi, (B,), device=DEV, generator=gen)
            uid, pid, nid = r(U.shape[0]), r(I.shape[0]), r(I.shape[0])
            if B > 8:
                uid[3] = uid[1]; pid[5] = pid[2]; nid[6] = pid[2]; nid[7] = nid[0]
            before = _snapshot(fs.state, opt)
            loss, upart, ipart = bpr_grads_fp64(U, I, uid, pid, nid, 0.0)
            part = ipart if frozen == 'user' else upart
            want = apply_fp64(before, part, D, opt, lr, wd, t)
            out = fs.step(uid, pid, nid)
            torch.cuda.synchronize()
            assert abs(float(out[0]) - loss) <= LOSS_RTOL * abs(loss), f'{tag} step {t}: loss {float(out[0])!r} vs fp64 {loss!r}'
            assert fs.state.step == t
            for k, v in _check_table(f'{tag} step {t}', before, _live(fs.state, opt), part[0], want).items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert _bits(affine, a0) and _bits(full, f0), f'{tag}: the frozen operand moved'
        print(f'\n{tag}: worst error / bound over 3 steps: {_fmt(worst)}')


# ---------------------------------------------------------------------------------------------------------------------- 4. the trainer

MODES, EPOCHS = ['SOURCE', 'TARGET', 'BOTH', 'TARGET'], [2, 1, 2, 1]


def _ids_users():
    from oracle.common import IdSpace
    return IdSpace(OU=20, TOU=15, SOU=18, OI=1, TOI=30, SOI=34)


def _fit(cfg, record=None):
    """DCDCSRTrainer.fit with the sizes of test_gpu_models5.py::test_dcdcsr_trainer_phase_loop_matches_oracle_training.  ``record``: a dict
    that receives, per table, the rows the run's steps name."""
    from recbole_cdr_amd.model.cross_domain_recommender.dcdcsr import DCDCSR
    from recbole_cdr_amd.trainer import DCDCSRTrainer
    from recbole_cdr_amd.utils import InputType
    ids = _ids_users()
    torch.manual_seed(13)
    mk, reset, s_pairs, t_pairs = _loaders(ids, InputType.PAIRWISE, 1, seed=4)
    full = base_config(DEV, latent_factor_model='BPR', embedding_size=16, mlp_hidden_size=[24], k=4, map_batch_size=32, learning_rate=0.01,
                       train_modes=MODES, epoch_num=[str(e) for e in EPOCHS], source_split=False, eval_step=1, epochs=2, **cfg)
    ds = FakeDataset(ids, s_pairs, t_pairs)
    ds.device = DEV
    model = DCDCSR(full, ds).to(DEV)
    init = {k: v.detach().clone() for k, v in model.named_parameters()}
    trainer = DCDCSRTrainer(full, model)
    log, orig = [], trainer._train_epoch
    trainer._train_epoch = lambda data, e: (log.append(orig(data, e)) or log[-1])
    if record is not None:
        step = model.fused_train_step

        def recording(interaction, **kw):
            count, unit = model.phase2count[model.phase], model._unit()
            named = lambda table, ids_: record.setdefault(table, set()).update(int(i) for i in ids_.reshape(-1).tolist())
            if model.phase == 'BOTH':
                state = np.random.get_state()                # the draw the step is about to make
                named(f'target_{unit}_embedding', torch.from_numpy(np.random.randint(0, ids.target_num_users, 32)))
                np.random.set_state(state)
            else:
                d = model.phase.lower()
                u, p, n = interaction[f'{d}_user_id'], interaction[f'{d}_item_id'], interaction[f'neg_{d}_item_id']
                if count == 1 or unit != 'user':
                    named(f'{d}_user_embedding', u)
                if count == 1 or unit != 'item':
                    named(f'{d}_item_embedding', torch.cat([p.reshape(-1), n.reshape(-1)]))
            return step(interaction, **kw)
        model.fused_train_step = recording
    np.random.seed(5)
    trainer.fit(mk())
    torch.cuda.synchronize()
    assert model.phase == 'OVERLAP' and len(log) == sum(EPOCHS)
    return log, {k: v.detach().clone() for k, v in model.named_parameters()}, model, init


def test_exact_rowwise_trainer_matches_the_dense_adam():
    """DCDCSRTrainer over SOURCE -> TARGET -> BOTH -> TARGET: optimizer_mode='rowwise' with rowwise_adam='exact' against
    optimizer_mode='dense' on the same model, seed, loaders and numpy stream -- per-epoch losses and every parameter within the tolerances
    of test_gpu_cmf_rowwise.py::test_exact_rowwise_trainer_matches_the_dense_adam, and the benchmark and affine tables within them too:
    ``set_phase`` read SYNCED tables (in exact mode the rows lag behind their update counts until ``fused_sync``).  A lazy run finishes
    with finite losses and leaves every row it never names bit-unchanged."""
    lr = 0.01
    log_d, par_d, m_d, _ = _fit(dict(optimizer_mode='dense'))
    log_e, par_e, m_e, _ = _fit(dict(optimizer_mode='rowwise', rowwise_adam='exact'))
    st = m_e._fused['states']
    assert sorted(st) == ['source_item_embedding', 'source_user_embedding', 'target_item_embedding', 'target_user_embedding']
    assert all(s.exact for s in st.values())
    # one state per table across the phases: the target tables were stepped by the first TARGET visit and by BOTH (users) or TARGET2 (items)
    assert set(m_e._fused['steps']) >= {'map', 'frozen'}
    n_both = int(next(iter(m_e._fused['steps']['map'].w_opt.state.values()))['step'])
    n_target = st['target_item_embedding'].step // 2                       # the two TARGET visits run one epoch each over the same loader
    assert n_both > 0 and n_target > 0 and st['target_item_embedding'].step == 2 * n_target
    assert st['target_user_embedding'].step == n_target + n_both and st['source_user_embedding'].step == st['source_item_embedding'].step > 0
    assert_close(torch.tensor(log_e), torch.tensor(log_d), rtol=5e-5, what='epoch losses')
    for k in par_d:
        assert_close(par_e[k], par_d[k], rtol=1e-4, atol=lr * 5e-2, what=k)
    assert_close(m_e.benchmark_embedding, m_d.benchmark_embedding, rtol=1e-4, atol=lr * 5e-2, what='benchmark table')
    assert_close(m_e.affine_embedding, m_d.affine_embedding, rtol=1e-4, atol=lr * 5e-2, what='affine table')
    named = {}
    log_l, par_l, m_l, init = _fit(dict(optimizer_mode='rowwise'), record=named)
    assert all(np.isfinite(v) for v in log_l) and not any(s.exact for s in m_l._fused['states'].values())
    assert sorted(named) == sorted(st)
    for table, rows in named.items():
        k = f'{table}.weight'
        never = torch.ones(par_l[k].shape[0], dtype=torch.bool, device=DEV)
        never[torch.tensor(sorted(rows), device=DEV)] = False
        assert bool(never.any()) and _bits(par_l[k][never], init[k][never]), f'{table}: a row the lazy run never names moved'
        assert not _bits(par_l[k][~never], init[k][~never])


# ---------------------------------------------------------------------------------------------------------------------- 5. checkpoint

def test_exact_checkpoint_resume_is_bit_exact(tmp_path):
    """save_checkpoint after three exact-mode BOTH steps (the table flushed to its update count) and resume_checkpoint into a fresh model
    and trainer, two more steps: the final state equals the uninterrupted run bit for bit -- tables, the unit table's moments and count,
    the MLP's parameters with their Adam moments and step counts.  (A checkpoint holds no benchmark table and no visit counts, in
    either optimizer mode; the test hands both to the resumed model, as a caller that resumes inside a BOTH phase has to.)"""
    from recbole_cdr_amd.model.cross_domain_recommender.dcdcsr import DCDCSR
    from recbole_cdr_amd.trainer import DCDCSRTrainer
    from recbole_cdr_amd.utils import InputType
    ids = _ids_users()
    _, _, s_pairs, t_pairs = _loaders(ids, InputType.PAIRWISE, 1, seed=4)
    cfg = base_config(DEV, latent_factor_model='BPR', embedding_size=16, mlp_hidden_size=[24], k=4, map_batch_size=32, learning_rate=0.01,
                      optimizer_mode='rowwise', rowwise_adam='exact', train_modes=MODES, epoch_num=['1'] * 4, source_split=False, eval_step=0,
                      epochs=1)

    def fresh(phases=('SOURCE', 'TARGET', 'BOTH')):
        torch.manual_seed(21)
        ds = FakeDataset(ids, s_pairs, t_pairs)
        ds.device = DEV
        m = DCDCSR(cfg, ds).to(DEV)
        m.train()
        for ph in phases:
            m.set_phase(ph)
        return m, DCDCSRTrainer(cfg, m)

    def run(m, ns):
        for n in ns:
            np.random.seed(100 + n)
            m.fused_train_step({}, lr=0.01, adam='exact')

    m_a, _ = fresh()
    run(m_a, range(5))
    m_a.fused_sync()
    m_b, t_b = fresh()
    run(m_b, range(3))
    path = str(tmp_path / 'ckpt.pth')
    t_b.save_checkpoint(path, epoch=0)
    m_c, t_c = fresh(phases=())
    t_c.resume_checkpoint(path)
    assert m_c.phase == 'BOTH'
    m_c.phase2count = dict(m_b.phase2count)
    m_c.benchmark_embedding = m_b.benchmark_embedding.clone()
    assert _bits(m_a.benchmark_embedding, m_b.benchmark_embedding)
    st = m_c._fused['states']
    assert sorted(st) == ['target_user_embedding'] and st['target_user_embedding'].exact
    assert int(st['target_user_embedding'].last.min()) == st['target_user_embedding'].step == 3
    run(m_c, range(3, 5))
    m_c.fused_sync()
    torch.cuda.synchronize()
    for (k, pa), (_, pc) in zip(m_a.named_parameters(), m_c.named_parameters()):
        assert torch.equal(pa, pc), k
    sa, sc = m_a.fused_optimizer_state(), m_c.fused_optimizer_state()
    ta, tc = sa['tables']['target_user_embedding'], sc['tables']['target_user_embedding']
    assert ta['step'] == tc['step'] == 5
    assert torch.equal(ta['exp_avg'], tc['exp_avg']) and torch.equal(ta['exp_avg_sq'], tc['exp_avg_sq'])
    wa, wc = sa['weights']['state'], sc['weights']['state']
    assert sorted(wa) == sorted(wc) == list(range(4))
    for j in wa:
        assert int(wa[j]['step']) == int(wc[j]['step']) == 5, j
        assert torch.equal(wa[j]['exp_avg'], wc[j]['exp_avg']) and torch.equal(wa[j]['exp_avg_sq'], wc[j]['exp_avg_sq']), j
        assert float(wa[j]['exp_avg'].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------- 6. refusals

def _dcdcsr(ids, D=16, hidden=(24,), **kw):
    from recbole_cdr_amd.model.cross_domain_recommender.dcdcsr import DCDCSR
    from recbole_cdr_amd.utils import InputType
    _, _, s_pairs, t_pairs = _loaders(ids, InputType.PAIRWISE, 1, seed=4)
    ds = FakeDataset(ids, s_pairs, t_pairs)
    ds.device = DEV
    torch.manual_seed(4)
    return DCDCSR(base_config(DEV, latent_factor_model='BPR', embedding_size=D, mlp_hidden_size=list(hidden), k=4, map_batch_size=32, **kw),
                  ds).to(DEV)


def _triples(ids, n=24, seed=0):
    g = torch.Generator(); g.manual_seed(seed)
    r = lambda lo, hi: torch.randint(lo, hi, (n,), generator=g).to(DEV)
    return {'source_user_id': r(1, ids.OU), 'source_item_id': r(ids.OI + ids.TOI, ids.total_num_items),
            'neg_source_item_id': r(ids.OI + ids.TOI, ids.total_num_items), 'target_user_id': r(1, ids.OU + ids.TOU),
            'target_item_id': r(1, ids.OI + ids.TOI), 'neg_target_item_id': r(1, ids.OI + ids.TOI)}


def test_refusals_come_before_any_launch():
    """adam other than 'lazy' / 'exact', adam='exact' with SGD, a batch without the phase's fields, empty and unequal-length id lists, a
    (phase, visit) pair without a loss, a second Adam mode on a model already trained with the other, config['dist_group'], an
    embedding_size the BPR step does not take and MLP widths the kernel rejects each raise what fused_train_step documents -- and leave the
    tables, their states and update counts and the parameters untouched; the native entry refuses its bad shapes with CDR_EINVAL."""
    from recbole_cdr_amd import binding as B_
    ids = _ids_users()
    m = _dcdcsr(ids)
    b = _triples(ids)
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    m.set_phase('SOURCE')
    with pytest.raises(ValueError, match='adam must be'):
        m.fused_train_step(b, lr=0.01, adam='dense')
    with pytest.raises(ValueError, match="opt='adam'"):
        m.fused_train_step(b, opt='sgd', lr=0.01, adam='exact')
    with pytest.raises(ValueError, match='the batch has no source_user_id'):
        m.fused_train_step({k: v for k, v in b.items() if 'target' in k}, lr=0.01)
    with pytest.raises(ValueError, match='at least one triple'):
        m.fused_train_step({k: v[:0] for k, v in b.items()}, lr=0.01)
    with pytest.raises(ValueError, match='id lists of equal length'):
        m.fused_train_step(dict(b, neg_source_item_id=b['neg_source_item_id'][:3]), lr=0.01)
    assert '_fused' not in m.__dict__
    torch.cuda.synchronize()
    for k, v in m.named_parameters():
        assert torch.equal(v, before[k]), k
    m.fused_train_step(b, lr=0.01)
    torch.cuda.synchronize()
    moved = {k: v.detach().clone() for k, v in m.named_parameters()}
    assert {k for k in moved if not torch.equal(moved[k], before[k])} == {'source_user_embedding.weight', 'source_item_embedding.weight'}
    with pytest.raises(ValueError, match='one row-wise Adam mode'):
        m.fused_train_step(b, lr=0.01, adam='exact')
    m.set_phase('SOURCE')
    with pytest.raises(ValueError, match="visit 2 of phase 'SOURCE'"):
        m.fused_train_step(b, lr=0.01)
    torch.cuda.synchronize()
    for k, v in m.named_parameters():
        assert torch.equal(v, moved[k]), k
    assert sorted(m._fused['states']) == ['source_item_embedding', 'source_user_embedding'] and all(s.step == 1 for s in m._fused['states'].values())
    md = _dcdcsr(ids, dist_group=True)
    md.set_phase('SOURCE')
    with pytest.raises(NotImplementedError, match='dist_group'):
        md.fused_train_step(b, lr=0.01)
    assert '_fused' not in md.__dict__ and not hasattr(md, 'fused_graph_key')
    for hidden in ((6,), (132,), (8, 8, 8)):
        mw = _dcdcsr(ids, hidden=hidden)
        mw.set_phase('SOURCE')
        with pytest.raises(ValueError, match='mapping MLP widths.*optimizer_mode=dense$'):
            mw.fused_train_step(b, lr=0.01)
        assert '_fused' not in mw.__dict__
    me = _dcdcsr(ids, D=6, hidden=(8,))
    me.set_phase('SOURCE')
    with pytest.raises(ValueError, match='got 6; use optimizer_mode=dense'):
        me.fused_train_step(b, lr=0.01)
    assert '_fused' not in me.__dict__
    # the native entry itself
    lib = B_.load()
    buf = torch.zeros(1 << 16, device=DEV)
    idx = torch.zeros(8, device=DEV, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for dims, n in (((8, 6, 8), 8), ((8, 132, 8), 8), ((8, 0, 8), 8), ((8,), 8), ((8, 8, 8, 8, 8), 8), ((8, 12, 12), 8), ((8, 12, 8), 0)):
        rc = lib.cdr_dcdcsr_map_fwd_grad(B_.ctx(DEV), B_.stream(), p(buf), p(buf), p(idx), n, len(dims) - 1, (ctypes.c_int * len(dims))(*dims),
                                         p(buf), p(buf), p(buf), p(buf), p(buf), buf.numel() * 4)
        assert rc == -1 and b'cdr_dcdcsr_map_fwd_grad' in lib.cdr_last_error(), (dims, n, rc)
    for bench, idl in ((None, p(idx)), (p(buf), None)):
        rc = lib.cdr_dcdcsr_map_fwd_grad(B_.ctx(DEV), B_.stream(), p(buf), bench, idl, 8, 2, (ctypes.c_int * 3)(8, 12, 8), p(buf), p(buf), p(buf),
                                         p(buf), p(buf), buf.numel() * 4)
        assert rc == -1 and b'cdr_dcdcsr_map_fwd_grad' in lib.cdr_last_error()
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------- 7. O(batch) memory

def test_the_map_step_allocates_o_batch_memory():
    """A 262,144-row unit table at D = 64 (64 MB), map_batch_size 1,024: after one warm step (the moments exist) one more step's peak
    allocation stays < 16 MB above the current one -- a quarter of one table, where a dense gradient alone would be 64 MB.  The bound is
    derived, not measured: the step's own buffers are G = 256 KB, the 32 workgroups' partials of 16,576 parameters (2,121,728 B), the
    packed gradient, the sort's keys and workspace -- 2.4 MB together, and allocated when the step object is built; a step itself
    allocates the packed parameters (66 KB) and nothing that grows with the table."""
    from recbole_cdr_amd.fused import FusedDCDCSRMapStep
    rows, D, n = 262144, 64, 1024
    gen = torch.Generator(device=DEV); gen.manual_seed(7)
    T = torch.empty(rows, D, device=DEV).normal_(0, 0.5, generator=gen)
    bench = torch.empty(rows, D, device=DEV).normal_(0, 0.5, generator=gen)
    fs = FusedDCDCSRMapStep(T, bench, _layers([64, 128, 64], gen), n, lr=1e-3)
    own = sum(t.numel() * t.element_size() for t in (fs.G, fs.keys, fs.perm, fs.ws, fs.fws, fs.dP))
    assert fs.G.numel() * 4 == 256 << 10 and fs.fws.numel() == 32 * 4 * n_params([64, 128, 64]) == 2121728
    assert own < 4 << 20, own                                 # (none of it is table-sized: the table is 64 MB)
    draw = lambda: torch.randint(0, rows, (n,), device=DEV, generator=gen)
    fs.step(draw())
    torch.cuda.synchronize()
    assert fs.state.exp_avg.shape == T.shape and float(fs.state.exp_avg.abs().max()) > 0
    idx = draw()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = fs.step(idx)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert np.isfinite(float(loss)) and fs.state.step == 2
    assert peak < 16 << 20, f'one map step allocated {peak} bytes at its peak: O(batch) is < 16 MB here, a dense gradient 64 MB'
