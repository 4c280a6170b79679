"""fused.FusedTripletStep (SSCDR's domain step: cdr_triplet_fwd_grad -> one sort -> two segmented applies) against a float64 restatement
in plain torch -- gather, the squared-norm "normalize" (sscdr.py:120-124), F.triplet_margin_loss, torch.autograd.grad summed per distinct
row -- at every lane width (D = 8 .. 256: 2 .. 64 lanes per row, D = 24 with dead lanes inside a lane group) for both optimizers.

Two shapes, three steps each, every step judged from the device's own state before it (teacher forcing):
  * B = 2,048 triples over 512 users x 256 items: every row recurs;
  * B = 4,099 (odd) over 8,192 x 4,096: most rows occur once, several blocks.
Every batch: item 7 in 300 positives (past 256 occurrences: the piece kernels of the segmented apply), n == p in four triples, ids 0 and
rows - 1 in both tables.  Tables are randn * 0.6 / sqrt(D) with a random half of the rows multiplied by 4: about half of the gathered
rows are on each side of L = sum x^2 = 1, and the margin of 0.2 leaves both hinge branches populated -- asserted on the reference.

Near a threshold (|h| < 1e-5 for the hinge h = d1 - d2 + margin, |L - 1| < 1e-5 for a row) fp32 and fp64 may take different branches: the
rows of such triples and such rows are left out of the VALUE comparison (they must be finite; whether they moved cannot be told from a
zero gradient), and they may be at most 0.1 % of B.

Loss: within fp64_bounds.LOSS_RTOL of the fp64 value; out3[1] = the fp64 count of open hinges, give or take the excluded triples.
SGD rows: lr = B / 16 (an update of the row's own magnitude).  The bound is the REFERENCE's: the same restatement in float32 gives
E_ref = max |ref32 - ref64| over the compared elements, and the device must stay within 4 E_ref (another, fixed summation order over up to
~300 occurrences); 4 E_ref <= 1e-3 max |lr G64| is asserted too, so that the check resolves the update.
Adam rows: w, m, v against fp64_bounds.apply_fp64 at rtol 2e-5, atol lr * 1e-2 (test_gpu_step_widths.py gives the reasoning).
Rows outside the batch stay bit-identical in w, m and v; a second run from the same initial state repeats the first bit for bit.

Measured on an MI355X: the worst ratio max |device - ref64| / E_ref over the 12 SGD cases x 3 steps x 2 tables is 1.050 (D = 24, B = 2,048,
step 1, item table: 6.77e-07 against E_ref 6.45e-07 with max |lr G64| = 2.2); most cases sit at 1.000 because device and float32
restatement both end on the half ulp of the table's largest weights (1.19e-07 at |w| in [2, 4)).  4 E_ref stayed below 9e-6 of
max |lr G64| everywhere.  Adam: max |device - fp64| <= 1.6e-06 on w against atol 1e-05."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from fp64_bounds import LOSS_RTOL, apply_fp64
from helpers import DEV, assert_close

pytestmark = pytest.mark.gpu

MARGIN, EPS, STEPS, ADAM_LR = 0.2, 1e-6, 3, 1e-3
SHAPES = {'recurring': (2048, 512, 256), 'sparse': (4099, 8192, 4096)}
NEAR = 1e-5


def _tables(nu, ni, D, gen):
    out = []
    for rows in (nu, ni):
        t = torch.randn(rows, D, device=DEV, generator=gen) * (0.6 / D ** 0.5)
        t[torch.randperm(rows, device=DEV, generator=gen)[:rows // 2]] *= 4.0
        out.append(t)
    return out


def _batch(B, nu, ni, gen):
    u = torch.randint(0, nu, (B,), device=DEV, generator=gen)
    p = torch.randint(0, ni, (B,), device=DEV, generator=gen)
    n = torch.randint(0, ni, (B,), device=DEV, generator=gen)
    p[:300] = 7
    n[5:9] = p[5:9]
    u[400], u[401], p[402], p[403], n[404], n[405] = 0, nu - 1, 0, ni - 1, 0, ni - 1
    return u, p, n


def _restate(Uw, Iw, u, p, n, dtype):
    """The step's loss and per-distinct-row gradients in ``dtype`` from the fp32 tables: (loss, user rows, G_u, item rows, G_i, h [B],
    L of the gathered rows [3, B])."""
    B = u.numel()
    ru, inv_u = torch.unique(u, return_inverse=True)
    ri, inv_i = torch.unique(torch.cat([p, n]), return_inverse=True)
    Ur = Uw[ru].to(dtype).requires_grad_(True)
    Ir = Iw[ri].to(dtype).requires_grad_(True)

    def normalize(x):
        L = (x * x).sum(1, keepdim=True)
        return x / torch.where(L > 1, L, torch.ones_like(L)), L.detach().squeeze(1)

    (yu, Lu), (yp, Lp), (yn, Ln) = normalize(Ur[inv_u]), normalize(Ir[inv_i[:B]]), normalize(Ir[inv_i[B:]])
    loss = F.triplet_margin_loss(yu, yp, yn, margin=MARGIN, p=2, eps=EPS)
    Gu, Gi = torch.autograd.grad(loss, (Ur, Ir))
    with torch.no_grad():
        h = F.pairwise_distance(yu, yp, eps=EPS) - F.pairwise_distance(yu, yn, eps=EPS) + MARGIN
    return loss.detach(), ru, Gu, ri, Gi, h, torch.stack([Lu, Lp, Ln])


def _snapshot(st, opt):
    d = {'w': st.table.clone()}
    if opt == 'adam':
        d['m'], d['v'] = st.exp_avg.clone(), st.exp_avg_sq.clone()
    return d


def _untouched_equal(tag, before, st, rows):
    touched = torch.zeros(before['w'].shape[0], dtype=torch.bool, device=DEV)
    touched[rows] = True
    live = {'w': st.table, 'm': st.exp_avg, 'v': st.exp_avg_sq}
    for name, t0 in before.items():
        changed = (t0.view(torch.int32) != live[name].view(torch.int32)).any(1)
        bad = changed & ~touched                       # (every row outside the batch: the two neighbours of each touched row among them)
        assert not bool(bad.any()), f'{tag}.{name}: {int(bad.sum())} rows outside the batch written, e.g. row {int(torch.nonzero(bad)[0])}'


def _run(D, opt, shape, check):
    """Three steps from a fixed seed; ``check``: compare each with the restatements.  Returns what a rerun must repeat bit for bit."""
    from recbole_cdr_amd.fused import FusedTripletStep
    B, nu, ni = SHAPES[shape]
    gen = torch.Generator(device=DEV); gen.manual_seed(1000 * D + B)
    U, I = _tables(nu, ni, D, gen)
    lr = B / 16 if opt == 'sgd' else ADAM_LR
    fs = FusedTripletStep(U, I, B, margin=MARGIN, opt=opt, lr=lr)
    tag0 = f'FusedTripletStep D={D} {opt} B={B}'
    outs, worst = [], 0.0
    for t in range(1, STEPS + 1):
        u, p, n = _batch(B, nu, ni, gen)
        if not check:
            outs.append(fs.step(u, p, n).clone())
            continue
        tag = f'{tag0} step {t}'
        bu, bi = _snapshot(fs.ustate, opt), _snapshot(fs.istate, opt)
        loss64, ru, Gu64, ri, Gi64, h, L = _restate(bu['w'], bi['w'], u, p, n, torch.float64)
        # both branches of the hinge and of the normalisation are exercised
        n_open = int((h > 0).sum())
        assert n_open >= 8 and B - n_open >= 8, f'{tag}: {n_open} of {B} hinges open'
        above = float((L > 1).double().mean())
        assert 0.2 <= above <= 0.8, f'{tag}: {above:.3f} of the gathered rows have L > 1'
        # near-threshold triples and rows: out of the value comparison
        near_row = (L - 1).abs() < NEAR                                   # [3, B]
        near_t = ((h.abs() < NEAR) | near_row.any(0))
        n_excl = int(near_t.sum())
        assert n_excl <= 0.001 * B, f'{tag}: {n_excl} near-threshold triples of {B}'
        skip_u = torch.zeros(nu, dtype=torch.bool, device=DEV); skip_i = torch.zeros(ni, dtype=torch.bool, device=DEV)
        skip_u[u[near_t]] = True; skip_i[p[near_t]] = True; skip_i[n[near_t]] = True
        out = fs.step(u, p, n).clone()
        torch.cuda.synchronize()
        outs.append(out)
        got = float(out[0])
        print(f'{tag}: loss {got:.8f} fp64 {float(loss64):.8f}; open hinges {int(out[1])} fp64 {n_open}; excluded triples {n_excl}')
        assert abs(got - float(loss64)) <= LOSS_RTOL * abs(float(loss64)), f'{tag}: loss {got!r} vs fp64 {float(loss64)!r}'
        assert abs(int(out[1]) - n_open) <= n_excl and float(out[2]) == 0.0, f'{tag}: open hinges {int(out[1])} vs fp64 {n_open}'
        assert fs.ustate.step == t and fs.istate.step == t
        if opt == 'sgd':
            _, _, Gu32, _, Gi32, _, _ = _restate(bu['w'], bi['w'], u, p, n, torch.float32)
        for name, st, before, rows, G64, G32, skip in (('U', fs.ustate, bu, ru, Gu64, Gu32 if opt == 'sgd' else None, skip_u),
                                                       ('I', fs.istate, bi, ri, Gi64, Gi32 if opt == 'sgd' else None, skip_i)):
            _untouched_equal(f'{tag} {name}', before, st, rows)
            assert bool(torch.isfinite(st.table[rows]).all()), f'{tag} {name}: non-finite rows'
            keep = ~skip[rows]
            if opt == 'sgd':
                w0 = before['w'][rows]
                ref64 = w0.double() - lr * G64
                ref32 = (w0 - torch.tensor(lr, dtype=torch.float32, device=DEV) * G32).double()
                e_ref = float((ref32 - ref64)[keep].abs().max())
                e_dev = float((st.table[rows].double() - ref64)[keep].abs().max())
                upd = float((lr * G64)[keep].abs().max())
                worst = max(worst, e_dev / e_ref)
                print(f'{tag} {name}: max |device - ref64| {e_dev:.3e}  E_ref = max |ref32 - ref64| {e_ref:.3e}  ratio {e_dev / e_ref:.3f}  '
                      f'max |lr G64| {upd:.3e}')
                assert 4 * e_ref <= 1e-3 * upd, f'{tag} {name}: 4 E_ref {4 * e_ref:.3e} does not resolve the update {upd:.3e}'
                assert e_dev <= 4 * e_ref, f'{tag} {name}: max |device - ref64| {e_dev:.3e} > 4 E_ref {4 * e_ref:.3e}'
            else:
                zero = torch.zeros_like(G64)
                want = apply_fp64(before, (rows, G64, zero, zero, torch.ones(rows.numel(), dtype=torch.int64, device=DEV)), D, 'adam',
                                  lr, 0.0, t)
                for q, live in (('w', st.table), ('m', st.exp_avg), ('v', st.exp_avg_sq)):
                    assert bool(torch.isfinite(live[rows]).all()), f'{tag} {name}.{q}: non-finite rows'
                    d = float((live[rows].double() - want[q][0])[keep].abs().max())
                    print(f'{tag} {name}.{q}: max |device - fp64| {d:.3e} (atol {lr * 1e-2:.1e})')
                    assert_close(live[rows][keep], want[q][0][keep], rtol=2e-5, atol=lr * 1e-2, what=f'{tag} {name}.{q}')
    if check and opt == 'sgd':
        print(f'{tag0}: worst device / E_ref {worst:.3f}')
    state = [fs.U, fs.I] + ([fs.ustate.exp_avg, fs.ustate.exp_avg_sq, fs.istate.exp_avg, fs.istate.exp_avg_sq] if opt == 'adam' else [])
    return outs + [s.clone() for s in state]


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('opt', ['sgd', 'adam'])
@pytest.mark.parametrize('D', [8, 16, 24, 64, 128, 256])
def test_triplet_step_vs_fp64(D, opt, shape):
    first = _run(D, opt, shape, check=True)
    again = _run(D, opt, shape, check=False)
    torch.cuda.synchronize()
    assert len(first) == len(again)
    for k, (a, b) in enumerate(zip(first, again)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'rerun differs in result {k}'


@pytest.mark.parametrize('D', [6, 260])
def test_triplet_fwd_grad_refuses_the_width_and_launches_nothing(D):
    from recbole_cdr_amd import binding as B_
    B = 64
    U = torch.randn(32, D, device=DEV); I = torch.randn(32, D, device=DEV)
    ids = torch.randint(0, 32, (B,), device=DEV)
    out3 = torch.full((3,), -7.0, device=DEV)
    GU = torch.full((B, D), -7.0, device=DEV); GI = torch.full((2 * B, D), -7.0, device=DEV)
    rc = B_.load().cdr_triplet_fwd_grad(B_.ctx(DEV), B_.stream(), ctypes.c_void_p(U.data_ptr()), ctypes.c_void_p(I.data_ptr()), D,
                                        ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(ids.data_ptr()), B,
                                        MARGIN, EPS, ctypes.c_void_p(out3.data_ptr()), ctypes.c_void_p(GU.data_ptr()),
                                        ctypes.c_void_p(GI.data_ptr()))
    torch.cuda.synchronize()
    assert rc != 0 and b'invalid argument' in B_.load().cdr_last_error()
    assert bool((out3 == -7.0).all()) and bool((GU == -7.0).all()) and bool((GI == -7.0).all())
    with pytest.raises(ValueError, match='multiple of 4'):
        from recbole_cdr_amd.fused import FusedTripletStep
        FusedTripletStep(U, I, B)
