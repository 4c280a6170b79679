"""DTCDR on the O(batch) row-wise path (``optimizer_mode='rowwise'``): csrc/cdr_dtcdr.hip's cdr_dtcdr_fwd_grad (the NeuMF tower of one
domain forward and backward on the fp32 MFMA, the max routing and every parameter gradient) and fused.FusedDTCDRStep (four tables row-wise,
each advanced once per step from both batches; the twelve tower parameters by the exact dense Adam).

Checked against: the reference's golden gradients (one SGD step with lr = 1 moves every parameter by -grad), the float64 restatement of
dtcdr_fp64.py element by element over three teacher-forced steps (its bounds are derived there and shown to bite in
test_dtcdr_rowwise_host.py), the oracle under the product's own dropout masks, a rerun from the same state, the dense trainer through
CrossDomainTrainer with rowwise_adam='exact', and a checkpoint round trip."""
import ctypes

import pytest
import torch

from dtcdr_fp64 import (TABLES, dtcdr_depths, dtcdr_domain_fp64, dtcdr_grid, dtcdr_packed, dtcdr_table_parts, dtcdr_weight_parts,
                        n_params)
from fp64_bounds import LOSS_RTOL, apply_fp64, ulp32
from golden_util import Golden, cases
from helpers import DEV, FakeDataset, base_config, load_params, to_dev, assert_close
from test_gpu_cmf_rowwise import _batch, _host_loaders, _ids_small
from test_gpu_step_fp64 import _check_table, _fmt, _live, _snapshot

pytestmark = pytest.mark.gpu

EMB = tuple(f'{t}_embedding' for t in TABLES)


def _dtcdr(ids, D=16, hidden=(32, 16), p=0.0, alpha=0.3, **kw):
    from recbole_cdr_amd.model.cross_domain_recommender.dtcdr import DTCDR
    cfg = base_config(DEV, embedding_size=D, mlp_hidden_size=list(hidden), dropout_prob=p, base_model='NeuMF', alpha=alpha, **kw)
    return DTCDR(cfg, FakeDataset(ids)).to(DEV)


def _assert_moved(name, before, after, want, what):
    """before - after == want at the tolerance test_dtcdr_golden holds the gradient to (helpers.assert_close with the row floor of
    _check_grads; the predict layers' bias, one cancelling sum, at 1e-5 of its 3e-2 terms) plus one ulp of the stored fp32 value (w - g is
    rounded to fp32 when it is written)."""
    want = torch.as_tensor(want).double().cpu()
    moved = (before.double() - after.double()).cpu().reshape(want.shape)
    stored = ulp32(after.double().cpu()).reshape(want.shape)
    big = float(want.abs().max())
    if want.dim() == 2 and want.shape[1] > 1:
        floor = 1e-5 * torch.maximum(want.abs().amax(1, keepdim=True), torch.tensor(1e-2 * big, dtype=torch.float64))
    elif name.endswith('predict_layer.bias'):
        floor = torch.tensor(1e-5 * 3e-2, dtype=torch.float64)
    else:
        floor = torch.tensor(1e-6 * big, dtype=torch.float64)
    bad = (moved - want).abs() > 1e-5 * want.abs() + floor + stored + 1e-12
    assert not bool(bad.any()), (f'{what}: {name}: {int(bad.sum())} elements off the reference gradient, e.g. {torch.nonzero(bad)[0].tolist()}: '
                                 f'moved {float(moved[bad][0])!r} want {float(want[bad][0])!r}')


# ---------------------------------------------------------------------------------------------------------------------- 1. golden pin

@pytest.mark.parametrize('name', cases('dtcdr_'))
def test_one_sgd_step_moves_every_parameter_by_the_reference_gradient(name):
    """lr = 1 SGD: all 16 parameters -- the four tables and the twelve tower parameters -- move by -grad/BOTH of the reference (D = 8,
    hidden [12, 6], B_s = 20 != B_t = 27, exact ties of torch.maximum included); the returned total is loss/BOTH; table rows whose
    reference gradient is all zero keep their bits."""
    g = Golden(name)
    D, hidden = int(g.meta('D')), [int(x) for x in g.meta('mlp_hidden_size')]
    model = _dtcdr(g.idspace(), D=D, hidden=hidden, alpha=float(g.meta('alpha')))
    load_params(model, g.group('param'))
    model.train()
    inter = to_dev(g.group('in'), DEV)
    assert inter['source_user_id'].numel() == 20 and inter['target_user_id'].numel() == 27 and (D, hidden) == (8, [12, 6])
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    loss = model.fused_train_step(inter, opt='sgd', lr=1.0)
    torch.cuda.synchronize()
    assert tuple(loss.shape) == (1,) and len(before) == 16
    assert_close(loss, g['loss/BOTH'], what=f'{name}: loss')
    want = g.group('grad/BOTH', as_torch=False)
    ties = 0
    for k, p in model.named_parameters():
        ref = want[k]
        _assert_moved(k, before[k], p.detach(), ref, name)
        if k.endswith('embedding.weight'):
            untouched = (torch.as_tensor(ref).to(DEV) == 0).all(1)
            assert torch.equal(p.detach()[untouched].view(torch.int32), before[k][untouched].view(torch.int32)), k
    for kind in ('user', 'item'):
        s, t = before[f'source_{kind}_embedding.weight'], before[f'target_{kind}_embedding.weight']
        ids = torch.cat([inter[f'source_{kind}_id'], inter[f'target_{kind}_id']])
        ties += int((s[ids] == t[ids]).sum())
    assert ties > 0, 'the fixture exercises the 1/2 : 1/2 split'
    st = model._fused['states']
    assert sorted(st) == sorted(EMB) and all(s.step == 1 for s in st.values())


# ---------------------------------------------------------------------------------------------------------------------- 2. fp64, element by element

def _plant(tabs):
    """Exact ties and all-loser rows, as test_dtcdr_rowwise_host._case plants them, in both id spaces."""
    for S, T in ((tabs[0], tabs[2]), (tabs[1], tabs[3])):
        D = S.shape[1]
        T[0:6] = S[0:6]
        T[6:12, ::2] = S[6:12, ::2]
        T[12:15] = S[12:15] - 1.0
        T[15:18] = S[15:18] + 1.0
        if D >= 8:
            T[18:20, :D // 2] = S[18:20, :D // 2]


def _export_masks(seed, salt0, B, widths, p):
    """The product's masks of one domain, exported with cdr_dropout_dev on ones (0 or 1 / (1 - p)), one [B, width] tensor per layer."""
    from recbole_cdr_amd import binding as B_
    out = []
    for n, w in enumerate(widths):
        ones = torch.ones(B, w, device=DEV)
        m = torch.empty_like(ones)
        B_.call('cdr_dropout_dev', B_.stream(), B_.f32(ones), ones.numel(), p, B_.i64(seed), salt0 + n, B_.f32(m))
        out.append(m)
    return out


def _tower(D, hidden, gen):
    w = [2 * D] + list(hidden)
    ps = []
    for i, o in zip(w[:-1], w[1:]):
        ps += [torch.empty(o, i, device=DEV).normal_(0, (2.0 / (i + o)) ** 0.5, generator=gen), torch.empty(o, device=DEV).normal_(0, 0.1, generator=gen)]
    ps += [torch.empty(1, w[-1], device=DEV).normal_(0, 0.5, generator=gen), torch.empty(1, device=DEV).normal_(0, 0.1, generator=gen)]
    return tuple(torch.nn.Parameter(p) for p in ps)


def _wsnap(step, p, opt, clone=True):
    """A tower parameter (and its Adam moments) as two-dimensional [rows, columns] tensors (a bias is [n, 1])."""
    two = lambda t: t.reshape(t.shape[0], -1)
    c = (lambda t: two(t).clone()) if clone else two
    d = {'w': c(p.data)}
    if opt == 'adam':
        st = step.w_opt.state.get(p) or {}
        d['m'] = c(st['exp_avg']) if st else torch.zeros_like(two(p.data))
        d['v'] = c(st['exp_avg_sq']) if st else torch.zeros_like(two(p.data))
    return d


def _step_cases():
    #   D, hidden,        Bs,    Bt, opt,    wd,    p
    return [
        (4, [5, 3, 1], 1, 1, 'adam', 0.0, 0.0),               # the narrowest tower, one row per domain
        (8, [12, 6], 31, 33, 'sgd', 0.01, 0.0),               # the fixtures' widths (no multiples of 4), ragged tiles
        (64, [32, 16], 64, 32, 'adam', 0.01, 0.2),            # the default shape, full tiles, dropout in front of both layers
        (128, [64], 31, 33, 'sgd', 0.0, 0.0),                 # the widest rows (non-temporal row traffic), 16 dW_0 tiles, one layer
        (128, [64, 64, 64], 64, 32, 'adam', 0.0, 0.1),        # the largest LDS plan
        (8, [12, 6], 40000, 33, 'adam', 0.0, 0.0),            # more tiles than workgroups: dW carried across a workgroup's tiles
    ]


@pytest.mark.parametrize('D,hidden,Bs,Bt,opt,wd,p', _step_cases())
def test_dtcdr_step_vs_fp64(D, hidden, Bs, Bt, opt, wd, p):
    """Three teacher-forced steps of FusedDTCDRStep against dtcdr_fp64's restatement with the kernel's real accumulation depths: the
    kernel's own outputs (every element of the four gradient-row buffers -- a loser's element +0.0 bit for bit --, of both packed tower
    gradients and of each out8), every element of every touched table row and of the twelve tower parameters after ONE optimizer update
    within its bound, every other table row bit-identical, each table's update count advanced exactly once per step.  Ids come from a
    range small enough that rows repeat inside a batch and across the two batches; exact ties and all-loser rows are planted."""
    from recbole_cdr_amd.fused import FusedDTCDRStep
    alpha = 0.3
    nu, ni = (24, 20) if Bs < 1000 else (4096, 2048)
    gen = torch.Generator(device=DEV); gen.manual_seed(D + 7 * len(hidden) + Bs)
    tabs = [torch.empty(n, D, device=DEV).normal_(0, 0.5, generator=gen) for n in (nu, ni, nu, ni)]
    towers = (_tower(D, hidden, gen), _tower(D, hidden, gen))
    lr = 1e-3 if opt == 'adam' else 0.5
    fs = FusedDTCDRStep(*tabs, towers, Bs, Bt, alpha, dropout_prob=p, opt=opt, lr=lr, weight_decay=wd)
    tag = f'FusedDTCDRStep D={D} hidden={hidden} {Bs}+{Bt} {opt} wd={wd} p={p}'
    grids = [dtcdr_grid(n, D, hidden) for n in (Bs, Bt)]
    assert fs.n_params == n_params(D, hidden) and [fs.grid(Bs), fs.grid(Bt)] == grids
    if Bs > 1000:
        assert Bs > 32 * grids[0], 'more tiles than workgroups: at least one workgroup walks two tiles and carries dW across them'
    widths = [2 * D] + hidden[:-1]
    seed = torch.zeros(1, device=DEV, dtype=torch.int64)
    worst = {}
    r = lambda n, hi: torch.randint(0, hi, (n,), device=DEV, generator=gen)

    for t in (1, 2, 3):
        _plant(tabs)
        su, si, tu, ti = r(Bs, nu), r(Bs, ni), r(Bt, nu), r(Bt, ni)
        if Bs >= 4:
            su[:4] = torch.tensor([0, 7, 13, 16], device=DEV); tu[:4] = su[:4]          # tied, half-tied and all-loser rows, in both batches
            si[:4] = torch.tensor([1, 8, 14, 17], device=DEV); ti[:4] = si[:4]
        else:
            su[0], tu[0], si[0], ti[0] = 13, 13, 8, 8
        ys = [(torch.rand(n, device=DEV, generator=gen) < 0.5).float() for n in (Bs, Bt)]
        seed.fill_(1000 + t)
        before = [_snapshot(st, opt) for st in fs.states]
        wbefore = [[_wsnap(fs, q, opt) for q in tw] for tw in towers]
        tw_before = [[q.data.clone() for q in tw] for tw in towers]
        out = fs.step(su, si, ys[0], tu, ti, ys[1], seed=seed if p > 0 else None)
        torch.cuda.synchronize()
        refs = []
        for d, (uid, iid, w, salt0, row0) in enumerate(((su, si, alpha, 0, 0), (tu, ti, 1 - alpha, 64, Bs))):
            B = uid.numel()
            masks = _export_masks(seed, salt0, B, widths, p) if p > 0 else None
            ref = dtcdr_domain_fp64([b['w'] for b in before], tw_before[d], uid, iid, ys[d], w, masks, dtcdr_depths(B, D, hidden, grids[d]))
            refs.append(ref)
            got = fs.out16[8 * d:8 * d + 8].tolist()
            for j, k in enumerate(('total', 'bce')):
                assert abs(got[j] - ref[k]) <= LOSS_RTOL * abs(ref[k]) + 1e-30, f'{tag} step {t} domain {d}: out8[{j}] ({k}) {got[j]!r} vs fp64 {ref[k]!r}'
            assert got[2:] == [0.0] * 6
            for j, name in enumerate(TABLES):
                buf = fs.G[j][row0:row0 + B]
                assert bool(torch.isfinite(buf).all()), f'{tag} step {t} domain {d}: non-finite rows for {name}'
                ratio = ref['G'][name].ratio(buf)
                worst[f'G.{name}'] = max(worst.get(f'G.{name}', 0.0), float(ratio.max()))
                assert float(ratio.max()) <= 1.0, (f'{tag} step {t} domain {d}: rows for {name}: error / bound = {float(ratio.max()):.3g} at '
                                                   f'element {divmod(int(ratio.argmax()), D)}')
                half = ref['share'][:, :D] if name.endswith('user') else ref['share'][:, D:]
                loser = (half == 0) if name.startswith('source') else (half == 1)
                assert bool((buf.view(torch.int32)[loser] == 0).all()), f'{tag} step {t} domain {d}: a loser\'s element of {name} is not +0.0'
            ratio = dtcdr_packed(ref).ratio(fs.dP[d])
            worst[f'dP{d}'] = max(worst.get(f'dP{d}', 0.0), float(ratio.max()))
            assert bool(torch.isfinite(fs.dP[d]).all()) and float(ratio.max()) <= 1.0, \
                f'{tag} step {t} domain {d}: packed tower gradient: error / bound = {float(ratio.max()):.3g} at element {int(ratio.argmax())}'
        total = refs[0]['total'] + refs[1]['total']
        assert tuple(out.shape) == (1,) and abs(float(out) - total) <= LOSS_RTOL * abs(total)
        # planted rows are in the batch as planted: the routing is exercised on ties and on all-loser rows
        if Bs >= 4:
            sh = refs[0]['share']
            assert bool((sh[0] == 0.5).all()) and bool((sh[2] == 1).all()) and bool((sh[3] == 0).all()) and 0 < int((sh[1] == 0.5).sum()) < 2 * D
        parts = dtcdr_table_parts(refs[0], refs[1], su, si, tu, ti)
        for j, (st, name) in enumerate(zip(fs.states, TABLES)):
            assert st.step == t, f'{tag}: update count of {name} after step {t}: {st.step}'
            wt = _check_table(f'{tag} step {t} {name}', before[j], _live(st, opt), parts[name][0], apply_fp64(before[j], parts[name], D, opt, lr, wd, t))
            for k, v in wt.items():
                worst[f'{name}.{k}'] = max(worst.get(f'{name}.{k}', 0.0), v)
        for d, ref in enumerate(refs):
            for j, (q, wb, part) in enumerate(zip(towers[d], wbefore[d], dtcdr_weight_parts(ref))):
                wt = _check_table(f'{tag} step {t} tower {d} parameter {j}', wb, _wsnap(fs, q, opt, clone=False), part[0],
                                  apply_fp64(wb, part, 0, opt, lr, wd, t))
                for k, v in wt.items():
                    worst[f'tower{d}.{k}'] = max(worst.get(f'tower{d}.{k}', 0.0), v)
    assert int(torch.bincount(torch.cat([su, tu])).max()) >= 2
    print(f'\n{tag}: worst error / bound over 3 steps: {_fmt(worst)} | overall {max(worst.values()):.3g}')


# ---------------------------------------------------------------------------------------------------------------------- 3. dropout

def test_dropout_step_matches_the_oracle_under_the_same_masks():
    """p = 0.4, D = 16, hidden [32, 16], B = 96: the product's counter-based masks are exported with cdr_dropout_dev on ones (same device
    seed, salt and element order, as test_dtcdr_training_dropout_value_parity_with_the_same_mask does) and handed to the oracle; under
    the same seed the fused step's loss and an lr = 1 SGD displacement of every parameter equal the oracle's masked loss and gradients."""
    import numpy as np
    from oracle import dtcdr as o_dt
    from oracle.common import IdSpace
    ids = IdSpace(12, 10, 14, 1, 20, 24)
    D, hidden, p, B = 16, [32, 16], 0.4, 96
    torch.manual_seed(3)
    model = _dtcdr(ids, D=D, hidden=hidden, p=p)
    model.train()
    rng = np.random.RandomState(5)
    inter = {'source_user_id': torch.from_numpy(rng.randint(1, ids.total_num_users, B)), 'source_item_id': torch.from_numpy(rng.randint(1, ids.total_num_items, B)),
             'source_label': torch.from_numpy((rng.rand(B) < 0.5).astype(np.float32)),
             'target_user_id': torch.from_numpy(rng.randint(1, ids.OU + ids.TOU, B)), 'target_item_id': torch.from_numpy(rng.randint(1, ids.OI + ids.TOI, B)),
             'target_label': torch.from_numpy((rng.rand(B) < 0.5).astype(np.float32))}
    torch.manual_seed(91)          # the seed the model will draw (DTCDR._drop_seed: one draw from torch's CPU generator per step)
    seed_val = int(torch.empty((), dtype=torch.int64).random_(0, 2 ** 62).item())
    seed = torch.full((1,), seed_val, device=DEV, dtype=torch.int64)
    masks = {}
    for dom, salt0 in (('source', 0), ('target', 64)):
        for n, m in enumerate(_export_masks(seed, salt0, B, [2 * D] + hidden[:-1], p)):
            assert abs(float((m != 0).float().mean()) - (1 - p)) < 0.08
            masks[(dom, n)] = m.cpu()
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
    want = o_dt.calculate_loss(params, ids, inter, 0.3, masks)
    want.backward()
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    torch.manual_seed(91)
    loss = model.fused_train_step(to_dev(inter, DEV), opt='sgd', lr=1.0)
    torch.cuda.synchronize()
    assert int(model._drop_state) == seed_val
    assert_close(loss, want, what='loss')
    assert len(before) == 16
    for k, v in model.named_parameters():
        _assert_moved(k, before[k], v.detach(), params[k].grad, 'dropout step')


# ---------------------------------------------------------------------------------------------------------------------- 4. determinism

def test_a_step_rerun_from_the_same_state_is_bit_equal():
    """No float atomics anywhere: the same step from the same state (tables, moments, tower parameters and their Adam state, the same
    dropout seed) twice gives bit-equal tables, moments, weights, gradient rows and loss.  Two tiles per workgroup on the source side."""
    from recbole_cdr_amd.fused import FusedDTCDRStep
    D, hidden, Bs, Bt, nu, ni = 8, [12, 6], 40000, 3000, 4096, 2048
    gen = torch.Generator(device=DEV); gen.manual_seed(77)
    tabs = [torch.empty(n, D, device=DEV).normal_(0, 0.5, generator=gen) for n in (nu, ni, nu, ni)]
    _plant(tabs)
    towers = (_tower(D, hidden, gen), _tower(D, hidden, gen))
    fs = FusedDTCDRStep(*tabs, towers, Bs, Bt, 0.3, dropout_prob=0.1, opt='adam', lr=1e-3, weight_decay=0.01)
    r = lambda n, hi: torch.randint(0, hi, (n,), device=DEV, generator=gen)
    seed = torch.full((1,), 12345, device=DEV, dtype=torch.int64)
    batches = [(r(Bs, nu), r(Bs, ni), (torch.rand(Bs, device=DEV, generator=gen) < 0.5).float(), r(Bt, nu), r(Bt, ni),
                (torch.rand(Bt, device=DEV, generator=gen) < 0.5).float()) for _ in range(2)]
    fs.step(*batches[0], seed=seed)                      # (moments and Adam state exist)
    state = lambda: ([{k: v.clone() for k, v in _live(st, 'adam').items()} for st in fs.states],
                     [[{k: v.clone() for k, v in _wsnap(fs, q, 'adam').items()} for q in tw] for tw in towers],
                     [fs.w_opt.state[q]['step'].clone() for q in fs.params])
    saved = state()
    out_a = fs.step(*batches[1], seed=seed).clone()
    first = state() + ([g.clone() for g in fs.G], fs.dP.clone(), fs.out16.clone())
    for st, sv in zip(fs.states, saved[0]):
        for k, v in _live(st, 'adam').items():
            v.copy_(sv[k])
        st.step = 1
    for tw, svs in zip(towers, saved[1]):
        for q, sv in zip(tw, svs):
            for k, v in _wsnap(fs, q, 'adam', clone=False).items():
                v.copy_(sv[k])
    for q, s in zip(fs.params, saved[2]):
        fs.w_opt.state[q]['step'].copy_(s)
    out_b = fs.step(*batches[1], seed=seed)
    torch.cuda.synchronize()
    second = state() + (list(fs.G), fs.dP, fs.out16)
    bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bits(out_a, out_b) and all(st.step == 2 for st in fs.states)
    for j, (a, b) in enumerate(zip(first[0], second[0])):
        assert all(bits(a[k], b[k]) for k in a), f'rerun differs in {TABLES[j]}'
    for a_tw, b_tw in zip(first[1], second[1]):
        assert all(bits(a[k], b[k]) for a, b in zip(a_tw, b_tw) for k in a), 'rerun differs in a tower parameter or its moments'
    assert all(torch.equal(a, b) for a, b in zip(first[2], second[2]))
    n = Bs + Bt
    assert all(bits(a[:n], b[:n]) for a, b in zip(first[3], second[3])) and bits(first[4], second[4]) and bits(first[5], second[5])
    assert float(out_a) > 0 and all(float((a['w'] - s['w']).abs().max()) > 0 for a, s in zip(first[0], saved[0]))


# ---------------------------------------------------------------------------------------------------------------------- 5. the trainer

def _full_cfg(**kw):
    full = dict(embedding_size=16, mlp_hidden_size=[32, 16], dropout_prob=0.0, base_model='NeuMF', alpha=0.3)
    full.update(kw)
    return base_config(DEV, **full)


def _fit(cfg, ids, mk, reset, seed):
    from recbole_cdr_amd.model.cross_domain_recommender.dtcdr import DTCDR
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    torch.manual_seed(seed)
    full = _full_cfg(**cfg)
    model = DTCDR(full, FakeDataset(ids)).to(DEV)
    reset()
    trainer = CrossDomainTrainer(full, model)
    log = []
    orig = trainer._train_epoch
    trainer._train_epoch = lambda data, e: (log.append(orig(data, e)) or log[-1])
    trainer.fit(mk())
    torch.cuda.synchronize()
    return log, {k: v.detach().clone() for k, v in model.named_parameters()}, model


def test_exact_rowwise_trainer_matches_the_dense_adam():
    """CrossDomainTrainer over three BOTH epochs with dropout_prob = 0: optimizer_mode='rowwise' with rowwise_adam='exact' against
    optimizer_mode='dense' (DenseAdam over the four tables and the towers) on the same model, seed and batches -- epoch losses and every
    parameter within the tolerances of test_gpu_cmf_rowwise.py::test_exact_rowwise_trainer_matches_the_dense_adam; the lazy run is
    outside them."""
    ids = _ids_small()
    lr = 0.01
    mk, reset = _host_loaders(ids)
    base = dict(learning_rate=lr, weight_decay=1e-3, train_modes=['BOTH'], epoch_num=['3'], source_split=False, eval_step=0, epochs=3)
    log_d, par_d, _ = _fit(dict(base, optimizer_mode='dense'), ids, mk, reset, 12)
    log_e, par_e, model = _fit(dict(base, optimizer_mode='rowwise', rowwise_adam='exact'), ids, mk, reset, 12)
    log_l, par_l, _ = _fit(dict(base, optimizer_mode='rowwise'), ids, mk, reset, 12)
    assert len(log_e) == 3 and all(st.exact for st in model._fused['states'].values()) and sorted(model._fused['states']) == sorted(EMB)
    assert all(st.step == 3 * 5 for st in model._fused['states'].values())          # 80 target positives, 16 (+ 16 negatives) per batch
    assert len(par_d) == 16
    assert_close(torch.tensor(log_e), torch.tensor(log_d), rtol=5e-5, what='epoch losses')
    for k in par_d:
        assert_close(par_e[k], par_d[k], rtol=1e-4, atol=lr * 5e-2, what=k)
    worst = max(float((par_l[k] - par_d[k]).abs().max()) for k in par_d)
    assert worst > 20 * lr * 5e-2, worst


# ---------------------------------------------------------------------------------------------------------------------- 6. checkpoint

def test_exact_checkpoint_resume_is_bit_exact(tmp_path):
    """save_checkpoint after three exact-mode steps with dropout_prob = 0.1 (the tables flushed to their update counts) and
    resume_checkpoint into a fresh model and trainer, three more steps: the final state equals the uninterrupted run bit for bit -- tables,
    their moments and counts, the twelve tower parameters with their Adam moments and step counts, and the dropout seeds drawn."""
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    ids = _ids_small()
    cfg = dict(learning_rate=0.01, optimizer_mode='rowwise', rowwise_adam='exact', train_modes=['BOTH'], epoch_num=['1'],
               source_split=False, eval_step=0, epochs=1, dropout_prob=0.1)

    def fresh():
        from recbole_cdr_amd.model.cross_domain_recommender.dtcdr import DTCDR
        torch.manual_seed(21)
        m = DTCDR(_full_cfg(**cfg), FakeDataset(ids)).to(DEV)
        m.train()
        return m, CrossDomainTrainer(_full_cfg(**cfg), m)

    def run(m, ns):
        seeds = []
        for n in ns:
            m.fused_train_step(_batch(ids, n), lr=0.01, adam='exact')
            seeds.append(int(m._drop_state))
        return seeds

    m_a, _ = fresh()
    seeds_a = run(m_a, range(6))
    m_a.fused_sync()
    m_b, t_b = fresh()
    run(m_b, range(3))
    path = str(tmp_path / 'ckpt.pth')
    t_b.save_checkpoint(path, epoch=0)
    torch.manual_seed(999)                                   # (the resumed process has another generator state until the checkpoint is read)
    m_c, t_c = fresh()
    torch.manual_seed(555)
    t_c.resume_checkpoint(path)
    assert sorted(m_c._fused['states']) == sorted(EMB)
    assert all(st.exact and int(st.last.min()) == st.step == 3 for st in m_c._fused['states'].values())
    seeds_c = run(m_c, range(3, 6))
    m_c.fused_sync()
    torch.cuda.synchronize()
    assert seeds_c == seeds_a[3:] and len(set(seeds_a)) == 6, 'the resumed run draws the masks of the uninterrupted one'
    for (k, pa), (_, pc) in zip(m_a.named_parameters(), m_c.named_parameters()):
        assert torch.equal(pa, pc), k
    sa, sc = m_a.fused_optimizer_state(), m_c.fused_optimizer_state()
    for name in EMB:
        assert sa['tables'][name]['step'] == sc['tables'][name]['step'] == 6, name
        assert torch.equal(sa['tables'][name]['exp_avg'], sc['tables'][name]['exp_avg']), name
        assert torch.equal(sa['tables'][name]['exp_avg_sq'], sc['tables'][name]['exp_avg_sq']), name
    wa, wc = sa['weights']['state'], sc['weights']['state']
    assert sorted(wa) == sorted(wc) == list(range(12))
    for j in wa:
        assert int(wa[j]['step']) == int(wc[j]['step']) == 6, j
        assert torch.equal(wa[j]['exp_avg'], wc[j]['exp_avg']) and torch.equal(wa[j]['exp_avg_sq'], wc[j]['exp_avg_sq']), j
        assert float(wa[j]['exp_avg'].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------- 7. refusals

def test_refusals_come_before_any_launch():
    """A batch without both domains' fields (names the phase), adam='exact' with SGD, a second Adam mode on the same tables,
    config['dist_group'] and widths the kernel rejects each raise what fused_train_step documents -- and leave the tables, their states
    and update counts and the towers untouched; the native entry refuses D = 6, D = 132, hidden widths 0 and 65, 0 and 4 layers and
    B = 0 with CDR_EINVAL."""
    from recbole_cdr_amd import binding as B_
    ids = _ids_small()
    torch.manual_seed(4)
    m = _dtcdr(ids)
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
    assert all(int(st['step']) == 1 for st in m._fused['steps']['dtcdr'].w_opt.state.values())
    md = _dtcdr(ids, dist_group=True)
    with pytest.raises(NotImplementedError, match='dist_group'):
        md.fused_train_step(b, lr=0.01)
    assert not md.__dict__.get('_fused') and not hasattr(md, 'fused_graph_key')
    for kw, what in ((dict(D=6), 'embedding_size = 6'), (dict(D=132), 'embedding_size = 132'), (dict(hidden=(12, 65)), r'\[12, 65\]'),
                     (dict(hidden=(8, 8, 8, 8)), r'\[8, 8, 8, 8\]')):
        mw = _dtcdr(ids, **kw)
        with pytest.raises(ValueError, match=what):
            mw.fused_train_step(b, lr=0.01)
        assert not mw.__dict__.get('_fused')
    # the native entry itself
    lib = B_.load()
    buf = torch.zeros(1 << 16, device=DEV)
    idx = torch.zeros(8, device=DEV, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for D, hidden, n in ((6, [12, 6], 8), (132, [12, 6], 8), (8, [0, 6], 8), (8, [12, 65], 8), (8, [], 8), (8, [8, 8, 8, 8], 8), (8, [12, 6], 0)):
        h = (ctypes.c_int * max(len(hidden), 1))(*hidden)
        rc = lib.cdr_dtcdr_fwd_grad(B_.ctx(DEV), B_.stream(), p(buf), p(buf), p(buf), p(buf), D, len(hidden), h, p(buf), p(idx), p(idx), p(buf), n,
                                    0.3, 0.0, None, 0, 0, p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), buf.numel() * 4)
        assert rc == -1 and b'cdr_dtcdr_fwd_grad' in lib.cdr_last_error(), (D, hidden, n, rc)
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0
