"""Self-tests of the bound helpers in fp64_bounds.py (no GPU): the gradient-free Adam recurrence that test_gpu_conet_fp64.py carries
through a row's postponed updates must hold an fp32 replay of the kernels' arithmetic (cdr_adam_math.h) and must NOT hold one whose bias
corrections are those of the neighbouring update."""
import pytest
import torch

from fp64_bounds import adam_idle_fp64, adam_replay_fp64


def _hp(t, lr, b1, b2):
    """cdr_adam_hp: step size and 1 / sqrt(bias correction 2) of update t, rounded once from fp64 to fp32."""
    return (torch.tensor(lr / (1.0 - b1 ** t), dtype=torch.float32), torch.tensor(1.0 / (1.0 - b2 ** t) ** 0.5, dtype=torch.float32))


def _replay_f32(w, m, v, t_from, n, lr, wd, b1, b2, eps, shift=0):
    """cdr_adam_elem with g = 0 in fp32, every operation rounded on its own; ``shift`` = -1 takes the bias corrections of update t - 1."""
    lr32, wd32, b132, b232, eps32 = (torch.tensor(x, dtype=torch.float32) for x in (lr, wd, b1, b2, eps))
    one = torch.tensor(1.0, dtype=torch.float32)
    for t in range(t_from + 1, t_from + n + 1):
        ss, bc2 = _hp(t + shift, float(lr32), float(b132), float(b232))
        g = wd32 * w if wd else torch.zeros_like(w)
        m = m + (g - m) * (one - b132)
        v = b232 * v + ((one - b232) * g) * g
        w = w - ss * (m * (one / (v.sqrt() * bc2 + eps32)))
    return w, m, v


def _rows(seed, n=4096, D=64):
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(n, D, generator=gen) * 0.5
    m = torch.randn(n, D, generator=gen) * 1e-3
    v = m * m * (0.25 + torch.rand(n, D, generator=gen)) + 1e-12
    return w, m, v


@pytest.mark.parametrize('wd,betas,eps', [(0.0, (0.9, 0.999), 1e-8), (1e-2, (0.9, 0.999), 1e-8), (1e-2, (0.8, 0.99), 1e-6)],
                         ids=['default', 'wd', 'betas'])
@pytest.mark.parametrize('t_from,n', [(1000, 1), (1000, 6), (0, 12), (3, 40)])
def test_idle_adam_bound_holds_fp32_and_sees_shifted_bias_correction(wd, betas, eps, t_from, n):
    lr = 1e-3
    b1, b2 = betas
    w, m, v = _rows(t_from + n)
    z = torch.zeros_like(w, dtype=torch.float64)
    ref, err = adam_replay_fp64({'w': w.double(), 'm': m.double(), 'v': v.double()}, {'w': z, 'm': z, 'v': z}, t_from, n, lr, wd, b1, b2, eps)
    got = _replay_f32(w, m, v, t_from, n, lr, wd, b1, b2, eps)
    for k, x in zip('wmv', got):
        r = float(((x.double() - ref[k]).abs() / err[k].clamp(min=1e-300)).max())
        assert r <= 1.0, (k, r)
    if t_from == 0 or (t_from >= 1000 and b2 != 0.999):
        return                  # (update 0 has no predecessor; b2 = 0.99 has forgotten its bias correction long before update 1,000)
    # bias corrections one update off: near update 1,000 (b2 = 0.999) that moves the update term by ~3e-4 of itself, in the first
    # updates by far more -- outside the bound, which is a few ulps of the term
    bad = _replay_f32(w, m, v, t_from, n, lr, wd, b1, b2, eps, shift=-1)[0]
    r = (bad.double() - ref['w']).abs() / err['w']
    assert float(r.max()) > 20, float(r.max())
    assert float((r > 1).double().mean()) > 0.5, float((r > 1).double().mean())


def test_idle_adam_bound_fixed_point_and_weight_decay():
    """wd = 0 and zero moments: the recurrence is the identity (the replay's fixed-point shortcut may skip it); with wd != 0 it moves."""
    w = torch.randn(64, 16, dtype=torch.float64)
    z = torch.zeros_like(w)
    st, er = adam_idle_fp64({'w': w, 'm': z, 'v': z}, {'w': z, 'm': z, 'v': z}, 1001, 1e-3)
    assert torch.equal(st['w'], w) and torch.equal(st['m'], z) and torch.equal(st['v'], z)
    st, er = adam_idle_fp64({'w': w, 'm': z, 'v': z}, {'w': z, 'm': z, 'v': z}, 1001, 1e-3, wd=1e-2)
    assert float(((st['w'] - w).abs() > 8 * er['w']).double().mean()) > 0.99


# ---------------------------------------------------------------------------------------------------------------------- dense-loss checker
# test_gpu_dense_loss_fp64.py's reference and checker without a GPU: plain torch fp32 autograd on the CPU (index_select + sum + torch's
# loss functions, gamma and the clamps as the oracle has them) must pass check_dense_result with every element checked, and three
# mutations of it -- the last interaction counted twice (what a wrong tail clamp does), one interaction dropped, positive and negative
# item swapped (pointwise: one label flipped) -- must each be rejected, at the C1 / C2 batch and past the forward's grid cap.

def _f32_dense(kind, tabs, doms, go, weights=None):
    """The drop-in losses in fp32 autograd.  ``doms``: [(ids..., reg, w)] -- one entry, or two for the pair; ``weights[d]``: a
    per-interaction factor on domain d's main loss (1 everywhere = the loss itself).  Returns check_dense_result's ``got``."""
    import torch.nn.functional as tf
    from fp64_bounds import GAMMA
    params = [t.detach().clone().requires_grad_(True) for t in tabs]
    U, I = params
    total, scalars = 0.0, {}
    for d, (*ids, reg, w) in enumerate(doms):
        u = U.index_select(0, ids[0])
        p = I.index_select(0, ids[1])
        B = ids[0].numel()
        if kind == 'bpr':
            n = I.index_select(0, ids[2])
            per = -torch.log(GAMMA + torch.sigmoid((u * p).sum(1) - (u * n).sum(1)))
        elif kind == 'mse':
            per = tf.mse_loss((u * p).sum(1), ids[2], reduction='none')
        else:
            per = tf.binary_cross_entropy(torch.sigmoid((u * p).sum(1)), ids[2], reduction='none')
        main = (per if weights is None or weights[d] is None else per * weights[d]).sum() / B
        nu, ni = (u * u).sum().sqrt(), (p * p).sum().sqrt()      # (torch's sum is pairwise; its fp32 CPU norm() is not: 3e-4 off at 8M terms)
        loss = main + reg * (nu + ni) / B
        total = total + w * loss
        sfx = str(d) if len(doms) > 1 else ''
        scalars.update({'main' + sfx: float(main.detach()), 'norm_u' + sfx: float(nu.detach()), 'norm_i' + sfx: float(ni.detach())})
        if len(doms) > 1:
            scalars['total' + sfx] = float(loss.detach())
    scalars['loss'] = float(total.detach())
    total.backward(torch.tensor(go, dtype=torch.float32))
    return {'scalars': scalars, 'coefs': [None] * len(doms), 'grads': [t.grad for t in params]}


def _dense_case(kind, B):
    """Inputs as test_gpu_dense_loss_fp64.py builds them on table (a), the fp64 reference, and the fp32 runner."""
    import test_gpu_dense_loss_fp64 as T
    from fp64_bounds import bpr_grads_fp64, f32, pair_grads_fp64, point_grads_fp64
    D, reg, go = 64, 0.01, f32(T.GO)
    gen = torch.Generator().manual_seed(B + len(kind))
    nu, ni = T.TABLES['a']
    U, I = T._tables('a', D, gen)
    detail = {}
    if kind == 'pair':
        Bt = B // 2 + 3
        su, si, ys, tu, ti, yt = T._pair_ids('hot', B, Bt, nu, ni, gen)
        w = (f32(0.3), f32(1.0 - 0.3))
        doms = [(su, si, ys, f32(0.02), w[0]), (tu, ti, yt, f32(0.0), w[1])]
        dl = []
        loss, _, upart, ipart = pair_grads_fp64(U, I, doms, go=go, detail=dl)
        ref = {'scalars': {'loss': loss}, 'coefs': [(d['g'], d['delta']) for d in dl], 'parts': [upart, ipart]}
        for j, d in enumerate(dl):
            ref['scalars'].update({f'total{j}': d['main'] + doms[j][3] * (d['nu'] + d['ni']) / (B, Bt)[j], f'main{j}': d['main'],
                                   f'norm_u{j}': d['nu'], f'norm_i{j}': d['ni']})
        return (U, I), doms, ref, D, go
    if kind == 'bpr':
        u, p, n = T._bpr_ids(B, nu, ni, gen, True)
        loss, *parts = bpr_grads_fp64(U, I, u, p, n, f32(reg), go=go, detail=detail)
        doms = [(u, p, n, f32(reg), 1.0)]
    else:
        u, i, y = T._point_ids(B, nu, ni, gen, True)
        loss, *parts = point_grads_fp64(U, I, u, i, y, f32(reg), kind, go=go, detail=detail)
        doms = [(u, i, y, f32(reg), 1.0)]
    ref = {'scalars': {'loss': loss, 'main': detail['main'], 'norm_u': detail['nu'], 'norm_i': detail['ni']},
           'coefs': [(detail['g'], detail['delta'])], 'parts': parts}
    return (U, I), doms, ref, D, go


def _past_cap(kind):
    import test_gpu_dense_loss_fp64 as T
    B = T.edges('bpr' if kind == 'bpr' else 'point', 64)[3] + 1
    assert T.is_ragged_tail('bpr' if kind == 'bpr' else 'point', 64, B)
    return B


@pytest.mark.parametrize('size', ['c1c2', 'past_cap'])
@pytest.mark.parametrize('kind', ['bpr', 'mse', 'bce', 'pair'])
def test_dense_checker_holds_fp32_autograd_and_rejects_three_mutations(kind, size):
    from fp64_bounds import check_dense_result
    B = 2048 if size == 'c1c2' else _past_cap(kind)
    tabs, doms, ref, D, go = _dense_case(kind, B)
    kk = 'bce' if kind == 'pair' else kind
    worst = check_dense_result(f'{kind} B={B} fp32 autograd', _f32_dense(kk, tabs, doms, go), ref, D)
    assert all(v <= 1.0 for v in worst.values()) and sum(k.startswith('grad') for k in worst) == 2
    for part, t in zip(ref['parts'], tabs):                     # every row of both tables is checked: batch rows + exact-zero rows
        assert part[1].shape == (part[0].numel(), D) and part[0].numel() <= t.shape[0]
    print(f'\n{kind} B={B}: fp32 autograd worst error / bound: ' + ' '.join(f'{k}={v:.3g}' for k, v in worst.items()))
    j = 1000                                                    # an interaction on ordinary rows (not the hot ones: 3 mod 8 / 3 mod 7)
    none = [None] * len(doms)
    twice = torch.ones(B); twice[-1] = 2.0
    dropped = torch.ones(B); dropped[j] = 0.0
    swapped = [tuple(x.clone() if torch.is_tensor(x) else x for x in d) for d in doms]
    if kind == 'bpr':
        swapped[0][1][j], swapped[0][2][j] = doms[0][2][j], doms[0][1][j]
        assert int(doms[0][1][j]) != int(doms[0][2][j])
    else:
        swapped[0][2][j] = 1.0 - doms[0][2][j]
    for name, got in (('last interaction counted twice', _f32_dense(kk, tabs, doms, go, [twice] + none[1:])),
                      ('one interaction dropped', _f32_dense(kk, tabs, doms, go, [dropped] + none[1:])),
                      ('positive and negative swapped / label flipped', _f32_dense(kk, tabs, swapped, go))):
        # past the cap one interaction moves the mean loss by less than LOSS_RTOL: there the per-element gradient bound alone must see it
        with pytest.raises(AssertionError, match='gradient [01]: error / bound' if size == 'past_cap' else 'error / bound|vs fp64'):
            check_dense_result(f'{kind} B={B} {name}', got, ref, D)
        print(f'{kind} B={B}: rejected: {name}')


def test_dense_case_table_covers_every_launch_regime_without_a_gpu():
    """The coverage assertion of test_gpu_dense_loss_fp64.py is pure arithmetic: it holds (and fails on a changed table) here too."""
    import test_gpu_dense_loss_fp64 as T
    T.test_case_table_covers_every_launch_regime()


def test_gemm_case_table_covers_every_regime_without_a_gpu():
    """test_gpu_gemm_fp64.py's regime and route coverage and its ambiguity cap are arithmetic on seeded inputs: checked here on the CPU."""
    import test_gpu_gemm_fp64 as T
    T.test_case_table_covers_every_regime()


def test_rowmodels_case_table_covers_every_regime_without_a_gpu():
    """test_gpu_rowmodels_fp64.py's case table: every NATR register count, the grid-stride sizes, and the ambiguity cap on the CPU."""
    import test_gpu_rowmodels_fp64 as T
    T.test_case_table_covers_every_regime()


def test_dim_case_table_covers_every_regime_without_a_gpu():
    """test_gpu_dim_fp64.py's case tables: every lanes-per-row instantiation, both grid-stride capacities and the big sort, from the constants."""
    import test_dim_loopback_host as T
    T.test_case_table_covers_every_regime()


def test_running_bounds_hold_for_fp32_on_the_cpu_and_reject_small_mutations():
    """fp64_bounds.EV without a GPU: torch's own fp32 results lie inside the bounds the two fp64 test files build (a product with a tanh
    epilogue; the oracle's max-min normalisation with tied extremes through autograd), and results that are subtly wrong do not."""
    import test_gpu_gemm_fp64 as G
    import test_gpu_rowmodels_fp64 as R
    from fp64_bounds import EV
    from oracle.dcdcsr import maxmin_normalize
    gen = torch.Generator().manual_seed(5)
    A, Bm, bias = torch.randn(70, 131, generator=gen), torch.randn(131, 45, generator=gen) * 0.3, torch.randn(45, generator=gen)
    ref = (EV(A.double()).matmul(EV(Bm.double()), 131, extra=G.K_MFMA) + EV(bias.double())).tanh()
    got = torch.tanh(A @ Bm + bias)
    assert float(ref.ratio(got).max()) <= 1.0
    assert float(ref.ratio(torch.tanh(A @ Bm + bias).t().contiguous().t() * (1 + 2e-6)).max()) > 1.0          # 17 ulps off
    A2 = A.clone(); A2[3, 130] = 0.0                                                                              # the last k of one row dropped
    assert float(ref.ratio(torch.tanh(A2 @ Bm + bias)).max()) > 1.0
    x, gy = R._maxmin_inputs(41, 65)
    mm, nmax, nmin = R.maxmin_fp64(x, gy)
    xg = x.clone().requires_grad_(True)
    y, mean_, max_ = maxmin_normalize(xg)
    y.backward(gy)
    assert float(mm['y'].ratio(y.detach()).max()) <= 1.0 and float(mm['gx'].ratio(xg.grad).max()) <= 1.0
    assert float(mm['stats'].ratio(torch.cat([mean_, max_], 1).detach()).max()) <= 1.0
    tied = int(torch.nonzero(nmax > 1)[0])                              # all of a tie's share to its first column instead of an even split
    bad = xg.grad.clone()
    cols = torch.nonzero(x[tied] == x[tied].max()).reshape(-1)
    share = gy[tied, cols[1]] / (x[tied].max() - (x[tied].max() + x[tied].min()) / 2) - bad[tied, cols[1]]
    bad[tied, cols[0]] -= share
    bad[tied, cols[1]] += share
    assert float(mm['gx'].ratio(bad).max()) > 1.0
