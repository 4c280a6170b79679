"""float64 restatement of CLFM's row-wise domain step (csrc/cdr_clfm.hip, fused.FusedCLFMStep) on fp64_bounds.EV pairs, shared by
test_gpu_clfm_rowwise.py (the kernel and the step on the device) and test_clfm_rowwise_host.py (an fp32 torch-autograd result and three
mutations of it on the CPU: the yardstick is shown to bite before it is trusted on the GPU).

For one domain of B rows:  u = U[uid]  i = I[iid]  F = u W^T  x = <F, i>  p = sigmoid(x)  g = w (p - y) / B
    GU[b] = g_b (i W)_b     GI[b] = g_b F_b     dW = (g (.) i)^T u     c_u = w reg / (B ||u||_F),  c_i = w reg / (B ||i||_F)
Bounds (derived, never tuned; u = 2^-24):
  * F, T = i W and dW are EV.matmul with the REAL accumulation depth of the kernel (``clfm_depths``: the MFMA chain runs over the width
    rounded up to 8; dW's chain is 32 rows per tile times the tiles a workgroup walks, plus the partials added in workgroup order) or,
    for a result whose summation order is not known (torch on the CPU), the any-order depth n - 1;
  * x: the per-lane chain over the lane's chunks of the row plus the three butterfly steps;  p: EV.sigmoid;
  * g: (p - y) carries p's bound; the coefficient's own roundings -- p - y, 1 - p, pq, the division by max(pq, 1e-12), 1 / B, w / B and
    the two products -- are the K_COEF = 8 ulps of fp64_bounds.  torch's fp32 backward clamp is kept as pair_grads_fp64 keeps it:
    the factor pq / 1e-12 where the fp32 pq is below 1e-12 (0 where the fp32 sigmoid saturates);
  * a gradient row g_b F_b / g_b T_b: one more product (EV.__mul__);  the row update sums the occurrences' EV errors into the part's E
    and goes through fp64_bounds.apply_fp64 as every other row-wise step;  the EmbLoss term c X[r] has the relative bound
    gamma_{D + K_REG + 1} of pair_grads_fp64 (one product more than the single-domain steps: the domain weight)."""
import torch

from fp64_bounds import EV, K_COEF, K_REG, U32, _occ_sums, check_dense_grad, check_scalar, f32, gam


def clfm_depths(B, Du, Di, grid):
    """Accumulation depths of csrc/cdr_clfm.hip for a launch of ``grid`` workgroups."""
    k8 = lambda d: -(-d // 8) * 8
    tiles = -(-B // 32)
    return dict(F=k8(Du), T=k8(Di), x=4 * -(-(Di // 4) // 8) + 3, dW=32 * -(-tiles // grid) + grid)


def clfm_domain_fp64(U, I, W, uid, iid, y, w, reg, depths=None):
    """One domain.  Returns a dict: the scalars of out8 ('total', 'bce', 'emb', 'nu', 'ni', 'cu', 'ci'), the per-occurrence gradient
    rows 'GU' [B, Du] / 'GI' [B, Di] and the weight gradient 'dW' [Di, Du] as EV pairs, the coefficient 'g' (EV), and the two parts
    'upart' / 'ipart' = (rows, G, A, E, occ) of fp64_bounds.apply_fp64 with the EmbLoss term included."""
    B, Du, Di = uid.numel(), U.shape[1], I.shape[1]
    d = depths or dict(F=Du - 1, T=Di - 1, x=Di - 1, dW=B - 1)
    w, reg = f32(w), f32(reg)
    ru, inv_u = torch.unique(uid, return_inverse=True)
    ri, inv_i = torch.unique(iid, return_inverse=True)
    u, i, Wv = EV(U[ru].double()[inv_u]), EV(I[ri].double()[inv_i]), EV(W.double())
    yv = y.double()
    F = u.matmul(EV(Wv.v.t().contiguous()), d['F'])
    x = (F * i).sum(1, depth=d['x'])
    p = x.sigmoid()
    s, q = torch.sigmoid(x.v), torch.sigmoid(-x.v)
    bce = float(-(yv * torch.log(s).clamp(min=-100) + (1 - yv) * torch.log(q).clamp(min=-100)).mean())
    p32 = torch.sigmoid(x.v.float())
    pq32 = ((1 - p32) * p32).double()
    low = pq32 < 1e-12
    clamp = torch.where(low, pq32 / 1e-12, torch.ones_like(pq32))
    scale = w / B
    gv = (s - yv) * clamp * scale
    rel_pq = torch.where(low & (clamp > 0), p.e / torch.minimum(s, q).clamp(min=1e-300), torch.zeros_like(p.e))
    g = EV._rnd(gv, p.e * clamp * scale + gv.abs() * rel_pq, k=K_COEF)
    g1 = g.unsqueeze(1)
    T = i.matmul(Wv, d['T'])
    GU, GI = g1 * T, g1 * F
    gi = i * g1
    dW = EV(gi.v.t().contiguous(), gi.e.t().contiguous()).matmul(u, d['dW'])
    nu, ni = float(u.v.norm()), float(i.v.norm())
    emb = (nu + ni) / B
    cu = w * reg / (B * nu) if reg and nu > 0 else 0.0
    ci = w * reg / (B * ni) if reg and ni > 0 else 0.0
    out = dict(total=w * (bce + reg * emb), bce=bce, emb=emb, nu=nu, ni=ni, cu=cu, ci=ci, GU=GU, GI=GI, dW=dW, g=g)
    for name, rows, inv, Gr, c, X, D in (('upart', ru, inv_u, GU, cu, u, Du), ('ipart', ri, inv_i, GI, ci, i, Di)):
        gc = gam(D + K_REG + 1)
        out[name] = (rows, *_occ_sums(rows.numel(), inv, Gr.v + c * X.v, Gr.v.abs() + abs(c) * X.v.abs(), Gr.e + gc * abs(c) * X.v.abs()))
    return out


def clfm_weight_parts(ref_s, ref_t, share):
    """{'shared' / 'source_only' / 'target_only': part} of the three linears from the two domains' dW: the shared weight's gradient is
    the sum of both domains' first ``share`` rows (two terms), the only-parts are the remaining rows of their own domain."""
    parts = {}
    ds, dt = ref_s['dW'], ref_t['dW']
    Di = ds.v.shape[0]
    rows = lambda n: torch.arange(n, device=ds.v.device)
    occ = lambda n, k: torch.full((n,), k, device=ds.v.device, dtype=torch.int64)
    if share > 0:
        parts['shared'] = (rows(share), ds.v[:share] + dt.v[:share], ds.v[:share].abs() + dt.v[:share].abs(), ds.e[:share] + dt.e[:share],
                           occ(share, 2))
    if share < Di:
        n = Di - share
        parts['source_only'] = (rows(n), ds.v[share:], ds.v[share:].abs(), ds.e[share:], occ(n, 1))
        parts['target_only'] = (rows(n), dt.v[share:], dt.v[share:].abs(), dt.e[share:], occ(n, 1))
    return parts


def check_clfm_result(tag, got, ref_s, ref_t, share):
    """An fp32 result of the whole BOTH-phase loss and its gradients against the two domains' references.  ``got``: {'loss': float,
    'tables': [dense gradients of the source user, source item, target user, target item table], 'weights': {'shared' / 'source_only'
    / 'target_only': gradient}}.  Every element of every gradient is compared (check_dense_grad: the batch's rows within their bounds,
    every other row +0.0).  Returns {quantity: worst error / bound}."""
    worst = {'loss': check_scalar(f'{tag}: loss', got['loss'], ref_s['total'] + ref_t['total'])}
    for name, grad, part in zip(('source_user', 'source_item', 'target_user', 'target_item'), got['tables'],
                                (ref_s['upart'], ref_s['ipart'], ref_t['upart'], ref_t['ipart'])):
        worst[name] = check_dense_grad(f'{tag}: gradient {name}', grad, part, grad.shape[1])
    wparts = clfm_weight_parts(ref_s, ref_t, share)
    assert set(wparts) == set(got['weights']), (sorted(wparts), sorted(got['weights']))
    for name, part in wparts.items():
        worst[name] = check_dense_grad(f'{tag}: gradient {name}', got['weights'][name], part, got['weights'][name].shape[1])
    return worst
