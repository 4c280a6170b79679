"""FusedBPRStep / FusedPointStep with opt='adagrad' against float64, by the scheme of test_gpu_step_fp64.py: teacher forcing from the
device's own state, three steps that reuse rows, per-element bounds (adagrad_bounds.py derives them), rows outside the batch -- each
touched row's neighbours in particular -- and their sums compared bit for bit.  Then the product-level statement that the O(batch) step
IS torch.optim.Adagrad over the whole tables at weight_decay = 0, and the entries that keep refusing CDR_OPT_ADAGRAD.

Shapes: the smallest that reach every id path of csrc/cdr_step.hip -- 2,048 (small batch), 16,447 / 16,448 (id-counter threshold, both
pinned paths), 65,536 'hot' (one item 20,000 times: long segments, the count path's global list) with weight_decay, 131,073 (past the
counters) -- on tables of 200,000 rows; D = 8 and 256 once each; the general segmented apply once (fuse_singles=False)."""
import ctypes

import pytest
import torch

from adagrad_bounds import ADAGRAD_EPS, apply_adagrad_fp64
from fp64_bounds import LOSS_RTOL, bpr_grads_fp64, point_grads_fp64
from helpers import DEV
from test_gpu_step_fp64 import _bpr_ids, _check_table, _fmt, _mark_edges, _zipf

pytestmark = pytest.mark.gpu

ROWS = 200_000


def _snap(st):
    assert st.exp_avg is None, 'Adagrad keeps ONE state tensor'
    return {'w': st.table.clone(), 'v': st.exp_avg_sq.clone()}


def _live(st):
    return {'w': st.table, 'v': st.exp_avg_sq}


def _tables(D, gen, nu=ROWS, ni=ROWS):
    return (torch.empty(nu, D, device=DEV).normal_(0, 0.1, generator=gen), torch.empty(ni, D, device=DEV).normal_(0, 0.1, generator=gen))


def _run(fs, grads, steps, lr, wd, tag):
    """``steps``: the step's argument tuples; ``grads(bu_w, bi_w, *args)`` -> (loss, user part, item part) in float64."""
    ust, ist, D = fs.ustate, fs.istate, fs.D
    worst = {}
    for t, args in enumerate(steps, start=1):
        bu, bi = _snap(ust), _snap(ist)
        loss, upart, ipart = grads(bu['w'], bi['w'], *args)
        wu = apply_adagrad_fp64(bu, upart, D, lr, wd)
        wi = apply_adagrad_fp64(bi, ipart, D, lr, wd)
        out = fs.step(*args)
        torch.cuda.synchronize()
        got = float(out[0])
        assert abs(got - loss) <= LOSS_RTOL * abs(loss), f'{tag} step {t}: loss {got!r} vs fp64 {loss!r}'
        assert ust.step == t and ist.step == t
        for name, wt in (('U', _check_table(f'{tag} step {t} U', bu, _live(ust), upart[0], wu)),
                         ('I', _check_table(f'{tag} step {t} I', bi, _live(ist), ipart[0], wi))):
            for k, v in wt.items():
                worst[f'{name}.{k}'] = max(worst.get(f'{name}.{k}', 0.0), v)
        del bu, bi, wu, wi, upart, ipart
    print(f'\n{tag}: worst error / bound over {len(steps)} steps: {_fmt(worst)}')
    return worst


BPR_CASES = [(2048, 64, 'auto', 0.01, 0.0, 'uniform', True), (2048, 128, 'auto', 0.01, 0.0, 'uniform', True),
             (16447, 128, 'count', 0.01, 0.0, 'uniform', True), (16447, 128, 'sort', 0.01, 0.0, 'uniform', True),
             (16448, 128, 'count', 0.01, 0.0, 'uniform', True), (16448, 128, 'sort', 0.01, 0.0, 'uniform', True),
             (65536, 128, 'auto', 0.01, 0.01, 'hot', True), (131073, 64, 'auto', 0.01, 0.0, 'uniform', True),
             (2048, 8, 'auto', 0.01, 0.0, 'uniform', True), (2048, 256, 'auto', 0.01, 0.0, 'uniform', True),
             (16448, 64, 'auto', 0.01, 0.01, 'zipf', False)]


@pytest.mark.parametrize('B,D,path,reg,wd,shape,fuse', BPR_CASES)
def test_fused_bpr_step_adagrad_vs_fp64(B, D, path, reg, wd, shape, fuse):
    from recbole_cdr_amd.fused import FusedBPRStep
    gen = torch.Generator(device=DEV); gen.manual_seed(B + D)
    U, I = _tables(D, gen)
    lr = 1e-2
    fs = FusedBPRStep(U, I, B, opt='adagrad', lr=lr, eps=ADAGRAD_EPS, reg_weight=reg, weight_decay=wd, id_path=path, fuse_singles=fuse)
    assert fs.fuse_singles == fuse
    # ids over a window of the batch's order inside the 200,000-row tables, so that rows recur across the three steps (the window's
    # edges and rows 0 / ROWS - 1 are in every batch: _mark_edges)
    win_u, win_i = min(ROWS, max(2 * B, 4096)), min(ROWS, max(B, 2048))
    steps = []
    for _ in range(3):
        u, p, n = _bpr_ids(shape, B, win_u, win_i, gen)
        u[6], p[7], n[8] = ROWS - 1, ROWS - 1, ROWS - 1
        steps.append((u, p, n))
    _run(fs, lambda Uw, Iw, u, p, n: bpr_grads_fp64(Uw, Iw, u, p, n, reg), steps, lr, wd,
         f'FusedBPRStep adagrad B={B} D={D} {path} reg={reg} wd={wd} {shape} fuse_singles={fuse}')


@pytest.mark.parametrize('kind,B,fuse', [('mse', 2048, True), ('bce', 16448, True), ('mse', 16448, False)])
def test_fused_point_step_adagrad_vs_fp64(kind, B, fuse):
    from recbole_cdr_amd.fused import FusedPointStep
    D, reg, lr = 128, 0.01, 1e-2
    wd = 0.01 if kind == 'bce' else 0.0
    gen = torch.Generator(device=DEV); gen.manual_seed(B + (kind == 'bce'))
    U, I = _tables(D, gen)
    fs = FusedPointStep(U, I, B, loss=kind, opt='adagrad', lr=lr, eps=ADAGRAD_EPS, reg_weight=reg, weight_decay=wd, fuse_singles=fuse)
    win_u, win_i = min(ROWS, max(2 * B, 4096)), min(ROWS, max(B // 2, 1024))
    steps = []
    for t in range(1, 4):
        u = torch.randint(0, win_u, (B,), device=DEV, generator=gen)
        i = _zipf(B, win_i, gen) if t == 2 else torch.randint(0, win_i, (B,), device=DEV, generator=gen)
        _mark_edges(u, i, None, win_u, win_i, gen)
        u[6], i[7] = ROWS - 1, ROWS - 1
        steps.append((u, i, (torch.rand(B, device=DEV, generator=gen) < 0.5).float()))
    _run(fs, lambda Uw, Iw, u, i, y: point_grads_fp64(Uw, Iw, u, i, y, reg, kind), steps, lr, wd,
         f'FusedPointStep adagrad {kind} B={B} D={D} wd={wd} fuse_singles={fuse}')


@pytest.mark.parametrize('Bs,Bt,D,lam,gamma,wd,shape', [(4096, 3000, 64, 0.02, 0.05, 0.0, 'overlap'), (20000, 30000, 128, 0.02, 0.05, 0.01, 'zipf')])
def test_fused_point_pair_step_adagrad_vs_fp64(Bs, Bt, D, lam, gamma, wd, shape):
    """CMF's joint step on shared tables through cdr_point_step_fused_pair (the host-state entry): ONE Adagrad update per touched row from
    the sum of both domains' contributions, by the scheme of test_gpu_cmf_rowwise.py::test_pair_step_vs_fp64."""
    from fp64_bounds import pair_grads_fp64
    from recbole_cdr_amd.fused import FusedPointPairStep
    from test_gpu_cmf_rowwise import _pair_ids
    alpha, lr = 0.3, 1e-2
    nu, ni = max(Bs + Bt, 4096), max((Bs + Bt) // 2, 2048)
    gen = torch.Generator(device=DEV); gen.manual_seed(Bs + 3 * Bt + D)
    U, I = _tables(D, gen, nu, ni)
    fs = FusedPointPairStep(U, I, Bs, Bt, alpha, lam, gamma, opt='adagrad', lr=lr, eps=ADAGRAD_EPS, weight_decay=wd)
    ust, ist = fs.ustate, fs.istate
    tag = f'FusedPointPairStep adagrad {Bs}+{Bt} D={D} reg={lam},{gamma} wd={wd} {shape}'
    worst = {}
    for t in range(1, 4):
        su, si, tu, ti = _pair_ids(shape, Bs, Bt, nu, ni, gen)
        ys = (torch.rand(Bs, device=DEV, generator=gen) < 0.5).float()
        yt = (torch.rand(Bt, device=DEV, generator=gen) < 0.5).float()
        bu, bi = _snap(ust), _snap(ist)
        loss, parts, upart, ipart = pair_grads_fp64(bu['w'], bi['w'], [(su, si, ys, lam, alpha), (tu, ti, yt, gamma, 1 - alpha)])
        wu, wi = apply_adagrad_fp64(bu, upart, D, lr, wd), apply_adagrad_fp64(bi, ipart, D, lr, wd)
        out = fs.step(su, si, ys, tu, ti, yt)
        torch.cuda.synchronize()
        for j, (a, b) in enumerate(zip(out[:5].tolist(), [loss, parts[0][0], parts[1][0], parts[0][1], parts[1][1]])):
            assert abs(a - b) <= LOSS_RTOL * abs(b) + 1e-12, f'{tag} step {t}: out[{j}] {a!r} vs fp64 {b!r}'
        assert ust.step == ist.step == t
        for name, wt in (('U', _check_table(f'{tag} step {t} U', bu, _live(ust), upart[0], wu)),
                         ('I', _check_table(f'{tag} step {t} I', bi, _live(ist), ipart[0], wi))):
            for k, v in wt.items():
                worst[f'{name}.{k}'] = max(worst.get(f'{name}.{k}', 0.0), v)
    print(f'\n{tag}: worst error / bound over 3 steps: {_fmt(worst)}')


@pytest.mark.parametrize('S,k,D,reg,wd', [(4096, 2, 64, 0.01, 0.0), (6000, 3, 128, 0.01, 0.01)])
def test_rowwise_apply_rows_and_scaled_adagrad_vs_fp64(S, k, D, reg, wd):
    """cdr_rowwise_apply_rows and cdr_rowwise_apply_scaled with opt = CDR_OPT_ADAGRAD through the C ABI (no Python step takes them under
    Adagrad: their one caller, KMajorBPRStep, refuses it).  A KMajorBPRStep built for SGD lends its buffers, its forward
    (cdr_bpr_fwd_grad_kmajor: one user gradient row per positive, {user row, coefficient} records for the items) and its two-table sort;
    the two applies are then called by hand with exp_avg = NULL and the sums in exp_avg_sq, items first (they rebuild their gradient rows
    from the PRE-step user rows).  Reference: the B = S k tiled triples in float64 with the bounds of adagrad_bounds.py; two
    teacher-forced steps (the second on nonzero sums).  Short segments everywhere, one item with 700 occurrences and one user with 300
    positives (long segments: cut into pieces and finished by long_finish2_kernel), weight_decay 0 and 0.01, untouched rows and their
    sums bit-equal."""
    from recbole_cdr_amd import binding as B_
    from recbole_cdr_amd.fused import KMajorBPRStep, OPT_ADAGRAD
    lr, nu, ni = 1e-2, 20000, 10000
    gen = torch.Generator(device=DEV); gen.manual_seed(S + k + D)
    U, I = _tables(D, gen, nu, ni)
    VU, VI = torch.zeros_like(U), torch.zeros_like(I)
    fs = KMajorBPRStep(U, I, S, k=k, opt='sgd', lr=lr, reg_weight=reg, weight_decay=wd, fuse_singles=False)
    assert not fs.small and not fs.fuse_singles and fs.ustate.exp_avg_sq is None
    B = S * k
    hp = (lr, 0.9, 0.999, ADAGRAD_EPS, wd)
    worst = {}
    tag = f'cdr_rowwise_apply_rows/_scaled adagrad S={S} k={k} D={D} wd={wd}'
    for t in range(1, 3):
        u = torch.randint(0, nu, (S,), device=DEV, generator=gen)
        p = torch.randint(0, ni, (S,), device=DEV, generator=gen)
        n = torch.randint(0, ni, (B,), device=DEV, generator=gen)
        u[0], u[1], p[2], p[3], n[4], n[5] = 0, nu - 1, 0, ni - 1, 0, ni - 1
        n[torch.randperm(B, device=DEV, generator=gen)[:700]] = ni // 3          # a long item segment (> 32 occurrences, three pieces of 256)
        u[torch.randperm(S, device=DEV, generator=gen)[:300]] = nu // 3          # a long user segment
        n[S + 9] = p[9]                                                          # p == n in the second negative round
        bu, bi = {'w': U.clone(), 'v': VU.clone()}, {'w': I.clone(), 'v': VI.clone()}
        loss, upart, ipart = bpr_grads_fp64(bu['w'], bi['w'], u.repeat(k), p.repeat(k), n, reg)
        wu, wi = apply_adagrad_fp64(bu, upart, D, lr, wd), apply_adagrad_fp64(bi, ipart, D, lr, wd)
        ctxh, s = B_.ctx(U.device), B_.stream()
        B_.call('cdr_bpr_fwd_grad_kmajor', ctxh, s, B_.f32(U), B_.f32(I), D, B_.i64(u), B_.i64(p), B_.i64(n), S, k, float(fs.gamma), float(reg),
                B_.f32(fs.out6), B_.f32(fs.GU), B_.raw(fs.rec), None, None)
        base = fs._sort(u, p, n, S, ctxh)
        off = 4 * base * D                                                       # the item keys carry the table bit: pointers moved back
        B_.call('cdr_rowwise_apply_scaled', ctxh, s, OPT_ADAGRAD, ctypes.c_void_p(I.data_ptr() - off), None, ctypes.c_void_p(VI.data_ptr() - off), D,
                B_.raw(fs.keys[S:2 * S + B]), B_.raw(fs.perm[S:2 * S + B]), S + B, B_.raw(fs.rec), B_.f32(U), S, B_.f32(fs.out6[5:6]), *hp, 0, None, 0)
        B_.call('cdr_rowwise_apply_rows', ctxh, s, OPT_ADAGRAD, B_.f32(U), None, B_.f32(VU), D, B_.raw(fs.keys[:S]), B_.raw(fs.perm[:S]), S,
                B_.f32(fs.GU), S, B_.f32(fs.out6[4:5]), *hp, 0, None, 0)
        torch.cuda.synchronize()
        got = float(fs.out6[0])
        assert abs(got - loss) <= LOSS_RTOL * abs(loss), f'{tag} step {t}: loss {got!r} vs fp64 {loss!r}'
        for name, wt in (('U', _check_table(f'{tag} step {t} U', bu, {'w': U, 'v': VU}, upart[0], wu)),
                         ('I', _check_table(f'{tag} step {t} I', bi, {'w': I, 'v': VI}, ipart[0], wi))):
            for kk, v in wt.items():
                worst[f'{name}.{kk}'] = max(worst.get(f'{name}.{kk}', 0.0), v)
    print(f'\n{tag}: worst error / bound over 2 steps: {_fmt(worst)}')
    # the moment pointer is refused where Adagrad has none, and the sum is required
    lib = B_.load()
    pp = lambda x: ctypes.c_void_p(x.data_ptr())
    keep = U.clone()
    for m, v in ((pp(VU), pp(VU)), (None, None)):
        rc = lib.cdr_rowwise_apply_rows(ctxh, s, OPT_ADAGRAD, pp(U), m, v, D, pp(fs.keys), pp(fs.perm), S, pp(fs.GU), S, None, *hp, 0, None, 0)
        assert rc != 0 and b'opt' in lib.cdr_last_error()
    torch.cuda.synchronize()
    assert torch.equal(U, keep)


# ---------------------------------------------------------------------------------------------------------------------- lazy == dense

def _dense_step_fp64(U, I, SU, SI, u, p, n, reg, lr, gamma=1e-10):
    """One step of fp64 autograd (BPRLoss + reg EmbLoss, as emcdr.py's domain loss) + torch.optim.Adagrad over the WHOLE tables, from
    the given fp64 state; returns the new (U, I, sum_U, sum_I)."""
    Up, Ip = U.clone().requires_grad_(True), I.clone().requires_grad_(True)
    opt = torch.optim.Adagrad([Up, Ip], lr=lr, foreach=False)
    for q, s in ((Up, SU), (Ip, SI)):
        opt.state[q]['step'] = torch.tensor(0.0)
        opt.state[q]['sum'] = s.clone()
    ue, pe, ne = Up[u], Ip[p], Ip[n]
    x = (ue * pe).sum(1) - (ue * ne).sum(1)
    loss = -torch.log(gamma + torch.sigmoid(x)).mean() + reg * (ue.norm() + pe.norm()) / u.numel()
    loss.backward()
    opt.step()
    return Up.detach(), Ip.detach(), opt.state[Up]['sum'], opt.state[Ip]['sum']


def test_rowwise_adagrad_is_the_dense_adagrad_over_whole_tables():
    """20 steps of FusedBPRStep(opt='adagrad'), weight_decay = 0, 5,000 x 64 tables, B = 2,048 with Zipf positives, against fp64 autograd +
    torch.optim.Adagrad over the WHOLE tables.  What is checked:
      * rows no batch ever names are bit-equal to their initial values after all 20 steps, with a zero sum -- exactly what the dense sweep
        leaves them (s + 0 = s, w - lr 0 / (sqrt(s) + eps) = w);
      * EVERY step, from the device's own state, equals one dense fp64 step over the whole tables within the per-element bound b_t of
        adagrad_bounds.py on the batch's rows, and leaves every other row as the dense step does: bit for bit.
    The 20-step free-running fp64 run R from the initial state is carried along and compared at the end under
    acc = b_T + |F(dev_{T-1}) - F(R_{T-1})|  (F: the dense fp64 step).  That is the triangle inequality on the last step: once the per-step
    checks hold it cannot fail, and it bounds nothing on its own -- it is there as a consistency check of the two references and to print
    how far the two runs ended apart.  No a-priori bound on the free-running difference exists to assert: at a row's first touch the update
    lr g / (|g| + eps) is a step function of the gradient, so an element with |g| of the order of its fp32 error may legitimately come out
    with either sign and the two runs then differ by 2 lr there."""
    from recbole_cdr_amd.fused import FusedBPRStep
    rows, D, B, reg, lr, T = 5000, 64, 2048, 0.01, 1e-2, 20
    gen = torch.Generator(device=DEV); gen.manual_seed(20)
    U, I = _tables(D, gen, rows, rows)
    U0, I0 = U.clone(), I.clone()
    fs = FusedBPRStep(U, I, B, opt='adagrad', lr=lr, eps=ADAGRAD_EPS, reg_weight=reg, weight_decay=0.0)
    R = (U0.double(), I0.double(), torch.zeros(rows, D, device=DEV, dtype=torch.float64), torch.zeros(rows, D, device=DEV, dtype=torch.float64))
    acc = [torch.zeros(rows, D, device=DEV, dtype=torch.float64) for _ in range(4)]
    seen_u = torch.zeros(rows, dtype=torch.bool, device=DEV)
    seen_i = torch.zeros(rows, dtype=torch.bool, device=DEV)
    worst = 0.0
    lr32 = float(torch.tensor(lr, dtype=torch.float32))
    for t in range(1, T + 1):
        u = torch.randint(0, rows // 2, (B,), device=DEV, generator=gen)                 # (users of the upper half are never named)
        p = _zipf(B, rows, gen)
        n = torch.randint(0, rows // 2, (B,), device=DEV, generator=gen)
        seen_u[u] = True; seen_i[p] = True; seen_i[n] = True
        dev = (U.double(), I.double(), fs.ustate.exp_avg_sq.double(), fs.istate.exp_avg_sq.double())
        bu, bi = _snap(fs.ustate), _snap(fs.istate)
        _loss, upart, ipart = bpr_grads_fp64(bu['w'], bi['w'], u, p, n, reg)
        local = [torch.zeros(rows, D, device=DEV, dtype=torch.float64) for _ in range(4)]
        for (part, snap, iw, iv) in ((upart, bu, 0, 2), (ipart, bi, 1, 3)):
            want = apply_adagrad_fp64(snap, part, D, lr, 0.0)
            local[iw][part[0]] = want['w'][1]; local[iv][part[0]] = want['v'][1]
        Fdev = _dense_step_fp64(*dev, u, p, n, reg, lr32)
        FR = _dense_step_fp64(*R, u, p, n, reg, lr32)
        fs.step(u, p, n)
        torch.cuda.synchronize()
        now = (U.double(), I.double(), fs.ustate.exp_avg_sq.double(), fs.istate.exp_avg_sq.double())
        for k in range(4):
            r = ((now[k] - Fdev[k]).abs() / local[k].clamp(min=1e-300))[local[k] > 0]
            worst = max(worst, float(r.max()))
            assert float(r.max()) <= 1.0, f'step {t}, tensor {k}: error / bound {float(r.max()):.3g} against the dense fp64 step'
            same = local[k] == 0                                                # rows outside the batch: the dense step leaves them too
            assert torch.equal(now[k][same], dev[k][same]) and torch.equal(Fdev[k][same], dev[k][same])
            acc[k] = local[k] + (Fdev[k] - FR[k]).abs()
        R = FR
    final = (U.double(), I.double(), fs.ustate.exp_avg_sq.double(), fs.istate.exp_avg_sq.double())
    for k in range(4):
        over = (final[k] - R[k]).abs() > acc[k]
        assert not bool(over.any()), f'tensor {k}: the two fp64 references disagree on {int(over.sum())} elements (a bug of this test)'
    apart = max(float((final[k] - R[k]).abs().max()) for k in (0, 1))
    # never-touched rows: bit-equal to the initial tables, zero sums
    assert bool((~seen_u).any()) and bool((~seen_i).any())
    assert torch.equal(U[~seen_u].view(torch.int32), U0[~seen_u].view(torch.int32))
    assert torch.equal(I[~seen_i].view(torch.int32), I0[~seen_i].view(torch.int32))
    assert not bool(fs.ustate.exp_avg_sq[~seen_u].view(torch.int32).any()) and not bool(fs.istate.exp_avg_sq[~seen_i].view(torch.int32).any())
    assert fs.ustate.exp_avg is None and fs.istate.exp_avg is None
    print(f'\nrow-wise Adagrad vs dense fp64 Adagrad, {T} steps: worst per-step error / bound {worst:.3g}; free-running fp64 run ends '
          f'{apart:.3g} away at most (lr = {lr}); {int((~seen_u).sum())} user and {int((~seen_i).sum())} item rows never touched, bit-equal')


# ---------------------------------------------------------------------------------------------------------------------- refusals

def test_entries_without_an_adagrad_form_refuse_it_and_write_nothing():
    """cdr_bpr_step_fused_kmajor and cdr_map_step_unique with opt = CDR_OPT_ADAGRAD (2): the argument error, and every buffer handed over
    stays as it was."""
    from recbole_cdr_amd import binding as B_
    lib = B_.load()
    S, k, D = 64, 2, 16
    gen = torch.Generator(device=DEV); gen.manual_seed(6)
    U, I = _tables(D, gen, 512, 512)
    VU, VI = torch.zeros_like(U), torch.zeros_like(I)
    uid = torch.randint(0, 512, (S,), device=DEV, generator=gen)
    pid = torch.randint(0, 512, (S,), device=DEV, generator=gen)
    nid = torch.randint(0, 512, (S * k,), device=DEV, generator=gen)
    fb, hw = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.cdr_bpr_step_fused_kmajor_sizes(S, k, ctypes.byref(fb), ctypes.byref(hw)) == 0
    n_all = 2 * S + S * k
    bufs = {'out': torch.zeros(12, device=DEV), 'GU': torch.zeros(S, D, device=DEV), 'GI': torch.zeros(S + S * k, D, device=DEV),
            'keys': torch.zeros(n_all, device=DEV, dtype=torch.int32), 'perm': torch.zeros(n_all, device=DEV, dtype=torch.int32),
            'flags': torch.zeros(int(fb.value), device=DEV, dtype=torch.uint8), 'heads': torch.zeros(int(hw.value), device=DEV, dtype=torch.int32)}
    need = ctypes.c_size_t(0)
    assert lib.cdr_sort_workspace_bytes(n_all, 1024, ctypes.byref(need)) == 0
    ws = torch.zeros(int(need.value), device=DEV, dtype=torch.uint8)
    keep = {name: t.clone() for name, t in dict(bufs, U=U, I=I, VU=VU, VI=VI, ws=ws).items()}
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ctxh, s = B_.ctx(torch.device(DEV)), B_.stream()
    rc = lib.cdr_bpr_step_fused_kmajor(ctxh, s, 2, p(U), None, p(VU), 512, p(I), None, p(VI), 512, D, p(uid), p(pid), p(nid), S, k, 1e-10, 0.01,
                                       1e-2, 0.9, 0.999, 1e-10, 0.0, 1, 1, p(bufs['out']), p(bufs['GU']), p(bufs['GI']), p(bufs['keys']),
                                       p(bufs['perm']), p(bufs['flags']), p(bufs['heads']), p(ws), ws.numel())
    assert rc != 0 and b'opt' in lib.cdr_last_error(), 'cdr_bpr_step_fused_kmajor accepted CDR_OPT_ADAGRAD'
    # cdr_map_step_unique: one linear layer D -> D without bias
    W = torch.eye(D, device=DEV).contiguous()
    idx = torch.arange(1, 33, device=DEV, dtype=torch.int64)
    loss1 = torch.zeros(1, device=DEV)
    dims = (ctypes.c_int * 2)(D, D)
    plan = ctypes.c_size_t(0)
    assert lib.cdr_map_step_plan(1, dims, (ctypes.c_int * 1)(0), 32, ctypes.byref(plan)) == 0
    uws = torch.zeros(max(int(plan.value), 16), device=DEV, dtype=torch.uint8)
    one = lambda x: (ctypes.c_void_p * 1)(x)
    W0 = W.clone()
    rc = lib.cdr_map_step_unique(ctxh, s, 2, p(U), None, p(VU), p(I), None, p(VI), p(idx), 32, 1, dims, (ctypes.c_int * 1)(0), one(W.data_ptr()),
                                 one(None), one(None), one(None), one(None), one(None), one(None), one(None), None, None,
                                 1e-2, 0.9, 0.999, 1e-10, 0.0, p(loss1), p(uws), uws.numel())
    assert rc != 0 and b'opt' in lib.cdr_last_error(), 'cdr_map_step_unique accepted CDR_OPT_ADAGRAD'
    torch.cuda.synchronize()
    for name, t in dict(bufs, U=U, I=I, VU=VU, VI=VI, ws=ws).items():
        assert torch.equal(t, keep[name]), f'{name} was written by a refused call'
    assert torch.equal(W, W0) and float(loss1) == 0.0 and not bool(uws.any())
