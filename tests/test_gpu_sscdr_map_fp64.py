"""SSCDR's OVERLAP phase on the device against float64: functional.sqnorm_normalize (forward, saved length, backward), the one-launch map
loss functional.SSCDRMapLoss (cdr_sscdr_map_loss + cdr_scale2_unless_one), the dense route through functional.GatherMapRows
(cdr_gather_rows_multi and its three backward routes) and fused.SSCDRMapStep -- at widths that are no multiple of the 64 lanes of a row's
wave (4, 7, 8, 20, 100), above them (128, 256, 260), past the grid (8,197 rows: 2,048 blocks x 4 waves hold 8,192), on both sides of
L = sum x^2 = 1 and of the hinge, and with ids that repeat inside pos ++ neg.

The method is test_gpu_triplet_step.py's (sscdr_map_fp64.py states it and holds the reference): the reference is the loss in plain torch
in float64 with torch.autograd's gradients; triples within 1e-5 of a threshold (the hinge h = d1 - d2 + margin = 0, L = 1 of any of their
three rows) may take the other branch in fp32, are left out of the VALUE comparison (finite they must be) and may be at most 0.1 % of n; the
bound is the reference's own error: E_ref = max |ref32 - ref64| over the compared elements of a block, from the same restatement in
float32, the device within 4 E_ref, and 4 E_ref <= 1e-3 max |ref64| so that the bound resolves the block (over fewer than 32 compared
numbers -- the blocks at n = 1 and 3 -- E_ref is floored at half an fp32 ulp of max |ref64|: sscdr_map_fp64.check_block).  Zeros are held to
their bits: a closed hinge leaves both triplet blocks +0.0 and GT = -G3[:n] bit for bit, lamda = 0 leaves them +0.0 everywhere, a table row
named by no id has a +0.0 gradient and rows outside a step's batch keep w, m and v.  test_sscdr_map_fp64_host.py shows on the CPU that the
comparison rejects twelve single mutations of the kernel's formulas, and that every case here meets its conditions.

Both references of the dense route and of the step run on the CPU, from copies of the device's state: their sums (index_add_ per distinct
row, the bias gradients) then have a fixed order and E_ref does not move from run to run.

fused.SSCDRMapStep: three steps per case, each judged from the device's own state before it (teacher forcing).  SGD runs with lr = n / 16
(an update of the order of the row); the mapping is put back to its initial values after each SGD step (at that lr its plain-SGD update
would saturate the tanh and empty one side of L = 1; every update is checked before it is put back).  Adam starts from nonzero moments
and a different update count per table and per parameter; w, m, v against fp64_bounds.apply_fp64 at rtol 2e-5, atol lr x 1e-2
(test_gpu_step_widths.py gives the reasoning).  The mapping's gradients and updates are checked in the steps without a near-threshold
triple (the first of every case is one), under the same 4 E_ref.  One reference differs: at n = 4,099 the float32 reference adds the
12,297 per-row terms of a bias gradient in the device's own order (sscdr_map_fp64.wgrad_bias_sum, bias_sum_of); against torch's sum the
first layer's bias gradient at D = 8 stood at 5.2 and 5.8 E_ref (3.7e-7 of its largest element), in the device's order at 1.00.

Measured on an MI355X, worst max |device - ref64| / E_ref per part:
  * sqnorm_normalize: y 1.48, saved length 1.83, gx 1.06 (all at 40 x 260);
  * SSCDRMapLoss over its 54 cases: G3[:n] 1.00, G3[n:2n] 1.58 (n = 3), G3[2n:] 1.47 (n = 8,197, D = 8, go = 2.5), GT 1.28.  Before the
    kernel stored +0.0 the first case with a closed hinge failed the bit test: -cu x 0 left -0.0 in the triplet blocks;
  * the dense route, every route: table gradients 1.10, mapping gradients 1.39;
  * SSCDRMapStep with SGD: table rows 1.59 (n = 100) and 1.15 (n = 4,099), weight gradients 1.89 and 1.12, bias gradients 2.67 and 2.80,
    updated mapping values 2.30 and 1.71; with Adam max |device - fp64| <= 1.6e-7 on w, 8.3e-9 on m, 1.8e-11 on v against atol 1e-5."""
import pytest
import torch

import sscdr_map_fp64 as R
from fp64_bounds import LOSS_RTOL, apply_fp64
from helpers import DEV, assert_close

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------- A. normalize

@pytest.mark.parametrize('rows_,D', [(1, 4), (5, 7), (33, 20), (257, 64), (100, 100), (64, 256), (40, 260), (8197, 8)])
def test_sqnorm_normalize_vs_fp64(rows_, D):
    """y, the saved length and gx against float64; planted where there is room: a one-hot row (L == 1.0f exactly: not > 1, so y = x and
    gx = gy bit for bit), a zero row, a row of 10.0.  Rows with |L - 1| < 1e-5 are only checked for finiteness."""
    from recbole_cdr_amd import functional as F_
    gen = torch.Generator().manual_seed(31 * D + rows_)
    x = R.rows(rows_, D, gen)
    planted = rows_ >= 5
    if planted:
        x[1] = 0.0; x[1, D // 2] = 1.0
        x[2] = 0.0
        x[3] = 10.0
    gy = torch.randn(rows_, D, generator=gen)
    x, gy = x.to(DEV), gy.to(DEV)
    xd = x.clone().requires_grad_(True)
    y = F_.sqnorm_normalize(xd)
    ln = y.grad_fn.saved_tensors[1]
    y.backward(gy)
    torch.cuda.synchronize()
    out = {}
    for dtype in (torch.float64, torch.float32):
        xr = x.to(dtype).requires_grad_(True)
        yr, Lr = R.normalize(xr)
        out[dtype] = (yr.detach(), Lr, torch.autograd.grad(yr, xr, gy.to(dtype))[0])
    (y64, L64, g64), (y32, L32, g32) = out[torch.float64], out[torch.float32]
    keep = (L64 - 1).abs() >= R.NEAR
    if planted:
        assert float(ln[1]) == 1.0 and not bool(keep[1])
        assert torch.equal(_bits(y[1]), _bits(x[1])) and torch.equal(_bits(xd.grad[1]), _bits(gy[1])), 'the one-hot row: y = x, gx = gy'
        assert not bool(_bits(y[2]).any()) and float(ln[2]) == 0.0 and torch.equal(_bits(xd.grad[2]), _bits(gy[2])), 'the zero row'
        assert float(ln[3]) == 100.0 * D
    if rows_ >= 33:
        above = float((L64 > 1).double().mean())
        assert 0.2 <= above <= 0.8, above
    assert int((~keep).sum()) <= (1 if planted else 0) + R.CAP * rows_
    tag = f'sqnorm_normalize {rows_}x{D}'
    worst = {'y': R.check_block(f'{tag} y', y.detach(), y64, y32, keep), 'len': R.check_block(f'{tag} len', ln, L64, L32, keep),
             'gx': R.check_block(f'{tag} gx', xd.grad, g64, g32, keep)}
    print(f'{tag}: worst device / E_ref ' + ' '.join(f'{k}={v:.3f}' for k, v in worst.items()))


# ---------------------------------------------------------------------------------------------------------------------- B. the loss kernel

def _device_map_loss(M3, T, margin, lamda, go):
    from recbole_cdr_amd import functional as F_
    m3, tt = M3.clone().requires_grad_(True), T.clone().requires_grad_(True)
    total, parts = F_.SSCDRMapLoss.apply(m3, tt, margin, lamda)
    (total if go == 1.0 else total * go).backward(retain_graph=True)
    return total, parts, m3, tt


@pytest.mark.parametrize('lamda,go', [(R.LAMDA, 1.0), (R.LAMDA, 2.5), (0.0, 1.0)])
@pytest.mark.parametrize('margin', R.MARGINS)
@pytest.mark.parametrize('n,D', R.LOSS_SHAPES)
def test_sscdr_map_loss_vs_fp64(n, D, margin, lamda, go):
    """functional.SSCDRMapLoss on the kernel alone: sscdr_map_fp64.check_map_loss on the device's loss parts and four gradient blocks; a
    second call on the same inputs is bit-identical; a second backward through one node raises."""
    M3, T = (x.to(DEV) for x in R.loss_case(n, D))
    tag = f'SSCDRMapLoss n={n} D={D} margin={margin} lamda={lamda} go={go}'
    total, parts, m3, tt = _device_map_loss(M3, T, margin, lamda, go)
    torch.cuda.synchronize()
    got = {'total': total.detach(), 'parts': parts, 'G3': m3.grad, 'GT': tt.grad}
    worst = {}
    R.check_map_loss(tag, got, M3, T, margin, lamda, go, worst)
    print(f'{tag}: worst device / E_ref ' + ' '.join(f'{k}={v:.3f}' for k, v in worst.items()))
    with pytest.raises(RuntimeError, match='second time'):
        total.backward()
    total2, parts2, m3b, ttb = _device_map_loss(M3, T, margin, lamda, go)
    torch.cuda.synchronize()
    assert torch.equal(_bits(parts2), _bits(parts)) and torch.equal(_bits(m3b.grad), _bits(m3.grad)) and torch.equal(_bits(ttb.grad), _bits(tt.grad))


# ---------------------------------------------------------------------------------------------------------------------- C. the dense route

def _mapping(layers):
    from recbole_cdr_amd.model.cross_domain_recommender.sscdr import MLPLayers
    (W1, b1), (W2, b2) = layers
    m = MLPLayers([W1.shape[1], W1.shape[0], W2.shape[0]]).to(DEV)
    with torch.no_grad():
        for lin, (W, b) in zip((m.mlp_layers[1], m.mlp_layers[4]), layers):
            lin.weight.copy_(W); lin.bias.copy_(b)
    return m


def _dense_run(case, mapping):
    from recbole_cdr_amd import functional as F_
    tabs = [case[k].to(DEV).requires_grad_(True) for k in ('SA', 'TA', 'SB')]
    idx, pos, neg = (x.to(DEV) for x in case['batches'][0])
    for p in mapping.parameters():
        p.grad = None
    X3, Tt = F_.GatherMapRows.apply(tabs[0], tabs[1], tabs[2], idx, pos, neg, None)
    total, parts = F_.SSCDRMapLoss.apply(mapping(X3), Tt, case['margin'], case['lamda'])
    total.backward()
    torch.cuda.synchronize()
    return [parts.clone()] + [t.grad.clone() for t in tabs] + [p.grad.clone() for p in mapping.parameters()]


@pytest.mark.parametrize('D,route', [(8, 'atomic')] + [(D, r) for D in (20, 64) for r in ('atomic', 'ordered', 'sorted')])
def test_dense_route_vs_fp64(D, route):
    """GatherMapRows -> MLPLayers -> SSCDRMapLoss with table-sized gradients, as SSCDR.calculate_map_loss runs it: the atomic backward
    (cdr_scatter_add_rows_multi), set_deterministic(True) on cdr_ordered_bwd, and set_deterministic(True) with the ordered launch off (id
    sort + cdr_scatter_rows_sorted); D = 8 runs the atomic route only.  The three table gradients and the four parameter gradients against
    float64, each tensor under the 4 E_ref rule (both references on the CPU: a fixed order of their sums); rows named by no id are +0.0 bit
    for bit; the two deterministic routes repeat bit for bit."""
    from recbole_cdr_amd import functional as F_
    case = R.step_case(D, 'dense')
    mapping = _mapping(case['layers'])
    was = (F_._DETERMINISTIC[0], F_._ORDERED[0], F_._ORDERED_MAX[0])
    try:
        F_.set_deterministic(route != 'atomic')
        F_.set_ordered_backward(route != 'sorted')
        if route == 'ordered':
            assert F_.ordered_fits(D, 2 * case['n'])
        first = _dense_run(case, mapping)
        again = _dense_run(case, mapping) if route != 'atomic' else None
    finally:
        F_.set_deterministic(was[0])
        F_.set_ordered_backward(was[1], was[2])
    args = (case['SA'], case['TA'], case['SB'], case['layers'], *case['batches'][0], case['margin'], case['lamda'])
    r64, r32 = R.map_step(*args, torch.float64), R.map_step(*args, torch.float32)
    tag = f'dense route D={D} {route}'
    R.populations(tag, r64['h'], r64['L'], case['margin'], need_hinges=False)
    assert not bool(R.excluded(tag, r64['h'], r64['L']).any())
    for k, name in enumerate(('total', 'loss_s', 'loss_u')):
        g, w = float(first[0][k]), float(r64[name])
        assert abs(g - w) <= LOSS_RTOL * abs(w), f'{tag}: {name} {g!r} vs fp64 {w!r}'
    worst = {}
    for k, name in enumerate(('SA', 'TA', 'SB')):
        grad = first[1 + k].cpu()
        rows_, G64 = r64[name]
        named = torch.zeros(grad.shape[0], dtype=torch.bool)
        named[rows_] = True
        assert int((~named).sum()) >= 3 and not bool(_bits(grad[~named]).any()), f'{tag} {name}: a row named by no id is not +0.0'
        worst[name] = R.check_block(f'{tag} {name}', grad[rows_], G64, r32[name][1])
    for k, (g64, g32) in enumerate(zip(r64['params'], r32['params'])):
        worst[f'p{k}'] = R.check_block(f'{tag} p{k}', first[4 + k], g64, g32)
    print(f'{tag}: worst device / E_ref ' + ' '.join(f'{k}={v:.3f}' for k, v in worst.items()))
    if again is not None:
        for k, (a, b) in enumerate(zip(first, again)):
            assert torch.equal(_bits(a), _bits(b)), f'{tag}: rerun differs in result {k}'


# ---------------------------------------------------------------------------------------------------------------------- D. the step

def _cpu(d):
    return {k: v.cpu() if torch.is_tensor(v) else v for k, v in d.items()}


def _snapshot(st, opt):
    d = {'w': st.table.clone()}
    if opt == 'adam':
        d['m'], d['v'] = st.exp_avg.clone(), st.exp_avg_sq.clone()
    return d


def _param_state(fs, p):
    st = fs.map_opt.state[p]
    return {'w': p.detach().reshape(1, -1).clone(), 'm': st['exp_avg'].reshape(1, -1).clone(), 'v': st['exp_avg_sq'].reshape(1, -1).clone(),
            'step': int(st['step'])}


def _untouched_equal(tag, before, st, rows_):
    touched = torch.zeros(before['w'].shape[0], dtype=torch.bool, device=DEV)
    touched[rows_] = True
    live = {'w': st.table, 'm': st.exp_avg, 'v': st.exp_avg_sq}
    for name, t0 in before.items():
        bad = (_bits(t0) != _bits(live[name])).any(1) & ~touched
        assert not bool(bad.any()), f'{tag}.{name}: {int(bad.sum())} rows outside the batch written, e.g. row {int(torch.nonzero(bad)[0])}'


def _build_step(case, opt):
    from recbole_cdr_amd.fused import SSCDRMapStep
    n = case['n']
    tabs = [case[k].to(DEV) for k in ('SA', 'TA', 'SB')]
    mapping = _mapping(case['layers'])
    params = list(mapping.parameters())
    lr = R.sgd_lr(n) if opt == 'sgd' else R.ADAM_LR
    fs = SSCDRMapStep(*tabs, mapping, params, case['margin'], case['lamda'], opt=opt, lr=lr)
    states = (fs.sa_state, fs.ta_state, fs.sb_state)
    for st, c in zip(states, R.TABLE_STEPS):
        st.step = c
    if opt == 'adam':
        idx, pos, neg = case['batches'][0]
        ref = R.map_step(case['SA'], case['TA'], case['SB'], case['layers'], idx, pos, neg, case['margin'], case['lamda'], torch.float64)
        mom = R.step_moments(case, ref)
        for st, name in zip(states, ('SA', 'TA', 'SB')):
            st.exp_avg.copy_(mom[name][0]); st.exp_avg_sq.copy_(mom[name][1])
        for k, (p, (m, v)) in enumerate(zip(params, mom['params'])):
            s = fs.map_opt.state[p]
            s['step'] = torch.full((1,), R.PARAM_STEP0 + 97 * k, device=DEV, dtype=torch.int64)
            s['exp_avg'], s['exp_avg_sq'] = m.to(DEV), v.to(DEV)
    return fs, mapping, params, lr


def _run_step_case(D, opt, shape, check):
    """Three steps from the case's fixed inputs; ``check``: compare each with the restatements.  Returns what a rerun must repeat bit for bit."""
    case = R.step_case(D, shape)
    n = case['n']
    fs, mapping, params, lr = _build_step(case, opt)
    initial = [p.detach().clone() for p in params]
    states = {'SA': fs.sa_state, 'TA': fs.ta_state, 'SB': fs.sb_state}
    tag0 = f'SSCDRMapStep D={D} {opt} n={n}'
    outs, worst = [], {}
    for t, batch in enumerate(case['batches'], 1):
        idx, pos, neg = (x.to(DEV) for x in batch)
        if not check:
            outs.append(fs.step(idx, pos, neg).clone())
        else:
            tag = f'{tag0} step {t}'
            before = {k: _snapshot(st, opt) for k, st in states.items()}
            counts = {k: st.step for k, st in states.items()}
            pbefore = [_param_state(fs, p) if opt == 'adam' else {'w': p.detach().reshape(1, -1).clone()} for p in params]
            # both references on the CPU, from copies of the device's state: their sums (index_add_, the bias gradients) have a fixed order
            bcpu = {k: _cpu(b) for k, b in before.items()}
            pbefore = [_cpu(b) for b in pbefore]
            layers = [(params[0].detach().cpu(), params[1].detach().cpu()), (params[2].detach().cpu(), params[3].detach().cpu())]
            args = (bcpu['SA']['w'], bcpu['TA']['w'], bcpu['SB']['w'], layers, *batch, case['margin'], case['lamda'])
            r64 = R.map_step(*args, torch.float64)
            r32 = R.map_step(*args, torch.float32, bias_sum=R.bias_sum_of(n))
            R.populations(tag, r64['h'], r64['L'], case['margin'], need_hinges=False)
            mapped = float((r64['L'][1:] > 1).double().mean())
            assert 0.2 <= mapped <= 0.8, f'{tag}: {mapped:.3f} of the mapped rows have L > 1'
            ex = R.excluded(tag, r64['h'], r64['L'])
            n_excl = int(ex.sum())
            assert t > 1 or n_excl == 0, f'{tag}: the first step must hold no near-threshold triple'
            skip = R.skip_rows(case, batch, ex)
            loss = fs.step(idx, pos, neg).clone()
            torch.cuda.synchronize()
            outs.append(loss)
            got, want = float(loss), float(r64['total'])
            print(f'{tag}: loss {got:.8f} fp64 {want:.8f}; excluded triples {n_excl}')
            assert abs(got - want) <= LOSS_RTOL * abs(want), f'{tag}: loss {got!r} vs fp64 {want!r}'
            for name, st in states.items():
                rows_, G64 = r64[name]
                rows_d = rows_.to(DEV)
                assert st.step == counts[name] + 1, f'{tag} {name}: update count {st.step} after {counts[name]}'
                _untouched_equal(f'{tag} {name}', before[name], st, rows_d)
                assert bool(torch.isfinite(st.table[rows_d]).all()), f'{tag} {name}: non-finite rows'
                keep = ~skip[name][rows_]
                assert name != 'SA' or bool(keep.all())
                if opt == 'sgd':
                    w0 = bcpu[name]['w'][rows_]
                    ref64 = w0.double() - lr * G64
                    ref32 = w0 - torch.tensor(lr, dtype=torch.float32) * r32[name][1]
                    worst[name] = max(worst.get(name, 0.0), R.check_block(f'{tag} {name}', st.table[rows_d], ref64, ref32, keep))
                    upd, e_ref = float((lr * G64)[keep].abs().max()), float((ref32.double() - ref64)[keep].abs().max())
                    assert 4 * e_ref <= 1e-3 * upd, f'{tag} {name}: 4 E_ref {4 * e_ref:.3e} does not resolve the update {upd:.3e}'
                else:
                    zero = torch.zeros_like(G64)
                    want_s = apply_fp64(bcpu[name], (rows_, G64, zero, zero, torch.ones(rows_.numel(), dtype=torch.int64)), D, 'adam', lr, 0.0,
                                        counts[name] + 1)
                    for q, live in (('w', st.table), ('m', st.exp_avg), ('v', st.exp_avg_sq)):
                        now = live[rows_d].cpu()
                        assert bool(torch.isfinite(now).all()), f'{tag} {name}.{q}: non-finite rows'
                        d = float((now.double() - want_s[q][0])[keep].abs().max())
                        print(f'{tag} {name}.{q}: max |device - fp64| {d:.3e} (atol {lr * 1e-2:.1e})')
                        assert_close(now[keep], want_s[q][0][keep], rtol=2e-5, atol=lr * 1e-2, what=f'{tag} {name}.{q}')
            if n_excl == 0:
                for k, (p, g64, g32) in enumerate(zip(params, r64['params'], r32['params'])):
                    worst[f'p{k}.grad'] = max(worst.get(f'p{k}.grad', 0.0), R.check_block(f'{tag} p{k}.grad', p.grad, g64, g32))
                    if opt == 'sgd':
                        w0 = pbefore[k]['w'].view(p.shape)
                        ref64 = w0.double() - lr * g64
                        ref32 = w0 - torch.tensor(lr, dtype=torch.float32) * g32
                        worst[f'p{k}'] = max(worst.get(f'p{k}', 0.0), R.check_block(f'{tag} p{k}', p.detach(), ref64, ref32))
                    else:
                        rows_ = torch.zeros(1, dtype=torch.int64)
                        G = g64.reshape(1, -1)
                        want_p = apply_fp64(pbefore[k], (rows_, G, torch.zeros_like(G), torch.zeros_like(G), torch.ones_like(rows_)), D, 'adam',
                                            lr, 0.0, pbefore[k]['step'] + 1)
                        now = _param_state(fs, p)
                        assert now['step'] == pbefore[k]['step'] + 1, f'{tag} p{k}: update count'
                        for q in ('w', 'm', 'v'):
                            assert_close(now[q], want_p[q][0], rtol=2e-5, atol=lr * 1e-2, what=f'{tag} p{k}.{q}')
        if opt == 'sgd':
            with torch.no_grad():
                for p, p0 in zip(params, initial):
                    p.copy_(p0)
    if check and worst:
        print(f'{tag0}: worst device / E_ref ' + ' '.join(f'{k}={v:.3f}' for k, v in worst.items()))
    state = [fs.SA, fs.TA, fs.SB] + [p.detach() for p in params]
    if opt == 'adam':
        state += [x for st in states.values() for x in (st.exp_avg, st.exp_avg_sq)]
        state += [fs.map_opt.state[p][q] for p in params for q in ('exp_avg', 'exp_avg_sq')]
    return outs + [s.clone() for s in state]


@pytest.mark.parametrize('shape', list(R.STEP_SHAPES))
@pytest.mark.parametrize('opt', ['sgd', 'adam'])
@pytest.mark.parametrize('D', R.STEP_DIMS)
def test_sscdr_map_step_vs_fp64(D, opt, shape):
    first = _run_step_case(D, opt, shape, check=True)
    again = _run_step_case(D, opt, shape, check=False)
    torch.cuda.synchronize()
    assert len(first) == len(again)
    for k, (a, b) in enumerate(zip(first, again)):
        assert torch.equal(_bits(a), _bits(b)), f'rerun differs in result {k}'


@pytest.mark.parametrize('opt', ['sgd', 'adam'])
def test_sscdr_map_step_empty_batch_is_a_no_op(opt):
    """An empty batch leaves tables, moments, update counts and the mapping bit-identical and returns 0."""
    case = R.step_case(8, 'batch100')
    fs, mapping, params, lr = _build_step(case, opt)
    states = (fs.sa_state, fs.ta_state, fs.sb_state)
    before = [_snapshot(st, opt) for st in states]
    pbefore = [p.detach().clone() for p in params]
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    loss = fs.step(empty, empty, empty)
    torch.cuda.synchronize()
    assert float(loss) == 0.0
    live = lambda st: {'w': st.table, 'm': st.exp_avg, 'v': st.exp_avg_sq}
    for st, b, c in zip(states, before, R.TABLE_STEPS):
        assert st.step == c
        for q, t0 in b.items():
            assert torch.equal(_bits(t0), _bits(live(st)[q])), q
    for p, p0 in zip(params, pbefore):
        assert torch.equal(_bits(p.detach()), _bits(p0))
