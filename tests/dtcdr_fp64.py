"""float64 restatement of DTCDR's row-wise domain step (csrc/cdr_dtcdr.hip, fused.FusedDTCDRStep) on fp64_bounds.EV pairs, shared by
test_gpu_dtcdr_rowwise.py (the kernel and the step on the device) and test_dtcdr_rowwise_host.py (an fp32 torch-autograd result of the
oracle and three mutations of it on the CPU: the yardstick is shown to bite before it is trusted on the GPU).

For one domain of B rows (L hidden layers, m_l the dropout mask of layer l already scaled by 1 / (1 - p), or 1):
    x = [max(Us[u], Ut[u]) | max(Is[i], It[i])]   h_0 = x   a_l = W_l (m_l h_l) + b_l   h_{l+1} = relu(a_l)   z = w_out . h_L + b_out
    p = sigmoid(z)   g = w (p - y) / B   gz_{L-1} = g w_out [a_{L-1} > 0]   gz_{l-1} = m_l (gz_l W_l) [a_{l-1} > 0]   gx = m_0 (gz_0 W_0)
    dW_l = gz_l^T (m_l h_l)   db_l = sum_b gz_l   dw_out = sum_b g h_L   db_out = sum_b g
    gx is routed element by element: to the source table where its value is larger, to the target table where it is smaller, 1/2 : 1/2
    on an exact tie (the comparison is on the exact fp32 table values: the routing is exact and carries no bound).
Bounds (derived, never tuned; u = 2^-24):
  * every contraction is EV.matmul with the REAL accumulation depth of the kernel (``dtcdr_depths``: an MFMA chain runs over the width
    rounded up to 8; a dW / db chain is 32 rows per tile times the tiles a workgroup walks, plus the partials added in workgroup order)
    or, for a result whose summation order is not known (torch on the CPU), the any-order depth n - 1; the bias add is matmul's second
    ``extra`` rounding;
  * a mask product m h is one rounding (1 / (1 - p) is no power of two);
  * a unit is EV.relu in the forward and EV.step in the backward: a unit whose pre-activation is within its bound of 0
    (``ambiguous()``) contributes the either-branch error |gradient| there, nothing elsewhere; ``ambiguous`` counts them;
  * z: the per-lane chain over the lane's eight columns, the three butterfly steps and the bias;  p: EV.sigmoid;
  * g: as clfm_fp64 -- (p - y) carries p's bound, the coefficient's own roundings are K_COEF ulps, torch's fp32 backward clamp kept;
  * a table's update sums the occurrences' rows of BOTH domains (each table receives rows from both batches) into one part and goes
    through fp64_bounds.apply_fp64 as every other row-wise step."""
import ctypes

import torch

from fp64_bounds import EV, K_COEF, _occ_sums, check_dense_grad, check_scalar, ev_cat, f32

TABLES = ('source_user', 'source_item', 'target_user', 'target_item')


def n_params(D, hidden):
    w = [2 * D] + list(hidden)
    return sum(o * i + o for i, o in zip(w[:-1], w[1:])) + w[-1] + 1


def dtcdr_grid(B, D, hidden):
    """Workgroups of cdr_dtcdr_fwd_grad for a batch of B rows: its workspace is one packed parameter vector per workgroup."""
    from recbole_cdr_amd import binding
    need = ctypes.c_size_t(0)
    rc = binding.load().cdr_dtcdr_fwd_grad_workspace_bytes(B, D, len(hidden), (ctypes.c_int * len(hidden))(*hidden), ctypes.byref(need))
    assert rc == 0, (B, D, hidden, rc)
    assert need.value % (4 * n_params(D, hidden)) == 0
    return need.value // (4 * n_params(D, hidden))


def dtcdr_depths(B, D, hidden, grid):
    """Accumulation depths of csrc/cdr_dtcdr.hip for a launch of ``grid`` workgroups."""
    k8 = lambda d: -(-d // 8) * 8
    w = [2 * D] + list(hidden)
    tiles = -(-B // 32)
    chain = 32 * -(-tiles // grid) + grid
    return dict(fwd=[k8(n) for n in w[:-1]], bwd=[k8(n) for n in w[1:]], z=8 + 3 + 1, dW=chain, db=chain)


def _masked(h, m):
    return h if m is None else EV._rnd(h.v * m, h.e * m)


def dtcdr_domain_fp64(tabs, tower, uid, iid, y, w, masks=None, depths=None):
    """One domain.  ``tabs`` = (Us, Is, Ut, It) fp32; ``tower`` = [W_0, b_0, ..., w_out, b_out] fp32; ``masks``: None or one [B, width_l]
    tensor per hidden layer (0 or 1 / (1 - p)).  Returns a dict: 'total', 'bce' (floats), 'g' and 'gx' (EV), 'G' {table: EV [B, D]: the
    occurrence's gradient row for that table}, 'dP' [(EV, shape) per tower parameter, in tower order], 'ambiguous' (units whose ReLU branch
    the bounds cannot tell), 'share' [B, 2 D] (the source tables' share of every element of gx: 1, 1/2 or 0)."""
    Us, Is, Ut, It = tabs
    B, D = uid.numel(), Us.shape[1]
    L = len(tower) // 2 - 1
    widths = [2 * D] + [tower[2 * l].shape[0] for l in range(L)]
    d = depths or dict(fwd=[n - 1 for n in widths[:-1]], bwd=[n - 1 for n in widths[1:]], z=widths[-1], dW=B - 1, db=B - 1)
    w = f32(w)
    au, bu, ai, bi = Us[uid].double(), Ut[uid].double(), Is[iid].double(), It[iid].double()
    x = torch.cat([torch.maximum(au, bu), torch.maximum(ai, bi)], 1)
    share = lambda a, b: (a > b).double() + 0.5 * (a == b).double()
    cs = torch.cat([share(au, bu), share(ai, bi)], 1)                  # the source tables' share of every element; the target's is 1 - cs
    ms = [None if masks is None else masks[l].double() for l in range(L)]
    h, dh, steps, amb = EV(x), [], [], 0
    for l in range(L):
        h = _masked(h, ms[l])
        dh.append(h)
        pre = h.matmul(EV(tower[2 * l].double().t().contiguous()), d['fwd'][l])
        pre = EV(pre.v + tower[2 * l + 1].double(), pre.e)
        steps.append(pre.step())
        amb += int(pre.ambiguous().sum())
        h = pre.relu()
    wout, bout = tower[2 * L].double().reshape(-1), tower[2 * L + 1].double().reshape(())
    z = (h * wout).sum(1, depth=d['z']) + bout
    yv = y.double()
    p = z.sigmoid()
    s, q = torch.sigmoid(z.v), torch.sigmoid(-z.v)
    bce = float(-(yv * torch.log(s).clamp(min=-100) + (1 - yv) * torch.log(q).clamp(min=-100)).mean())
    p32 = torch.sigmoid(z.v.float())
    pq32 = ((1 - p32) * p32).double()
    low = pq32 < 1e-12
    clamp = torch.where(low, pq32 / 1e-12, torch.ones_like(pq32))
    scale = w / B
    gv = (s - yv) * clamp * scale
    rel_pq = torch.where(low & (clamp > 0), p.e / torch.minimum(s, q).clamp(min=1e-300), torch.zeros_like(p.e))
    g = EV._rnd(gv, p.e * clamp * scale + gv.abs() * rel_pq, k=K_COEF)
    g1 = g.unsqueeze(1)
    dwout = (g1 * h).sum(0, depth=d['db'])
    dbout = g.sum(0, depth=d['db'])
    gz = (g1 * wout) * steps[L - 1]
    dW, db = [None] * L, [None] * L
    for l in reversed(range(L)):
        dW[l] = EV(gz.v.t().contiguous(), gz.e.t().contiguous()).matmul(dh[l], d['dW'])
        db[l] = gz.sum(0, depth=d['db'])
        gh = _masked(gz.matmul(EV(tower[2 * l].double()), d['bwd'][l], extra=1), ms[l])
        gz = gh * steps[l - 1] if l > 0 else gh
    gx = gz
    gs, gt = gx.exact_scale(cs), gx.exact_scale(1 - cs)
    G = {'source_user': gs[:, :D], 'target_user': gt[:, :D], 'source_item': gs[:, D:], 'target_item': gt[:, D:]}
    dP = [x_ for l in range(L) for x_ in ((dW[l], tuple(tower[2 * l].shape)), (db[l], tuple(tower[2 * l + 1].shape)))]
    dP += [(dwout, tuple(tower[2 * L].shape)), (dbout, tuple(tower[2 * L + 1].shape))]
    return dict(total=w * bce, bce=bce, g=g, gx=gx, G=G, dP=dP, ambiguous=amb, share=cs)


def dtcdr_packed(ref):
    """The tower's gradient as one EV vector in the packed layout of cdr_dtcdr_fwd_grad's ``dparams``."""
    return ev_cat([EV(ev.v.reshape(-1), ev.e.reshape(-1)) for ev, _ in ref['dP']])


def dtcdr_table_parts(ref_s, ref_t, su, si, tu, ti):
    """{table: part} of fp64_bounds.apply_fp64 / check_dense_grad: every table receives the rows of BOTH batches (source occurrences
    first), a row named by both gets the sum."""
    parts = {}
    for kind, ids in (('user', torch.cat([su, tu])), ('item', torch.cat([si, ti]))):
        rows, inv = torch.unique(ids, return_inverse=True)
        for dom in ('source', 'target'):
            name = f'{dom}_{kind}'
            G = ev_cat([ref_s['G'][name], ref_t['G'][name]])
            parts[name] = (rows, *_occ_sums(rows.numel(), inv, G.v, G.v.abs(), G.e))
    return parts


def dtcdr_weight_parts(ref):
    """One part per tower parameter, in tower order, as two-dimensional [rows, columns] gradients (a bias is [n, 1])."""
    out = []
    for ev, shape in ref['dP']:
        shape2 = shape if len(shape) == 2 else (shape[0], 1)
        v, e = ev.v.reshape(shape2), ev.e.reshape(shape2)
        n = shape2[0]
        out.append((torch.arange(n, device=v.device), v, v.abs(), e, torch.ones(n, device=v.device, dtype=torch.int64)))
    return out


def check_dtcdr_result(tag, got, ref_s, ref_t, su, si, tu, ti):
    """An fp32 result of the whole BOTH-phase loss and its gradients against the two domains' references.  ``got``: {'loss': float,
    'tables': {table: dense gradient}, 'towers': ([gradients of the source tower, tower order], [the same of the target])}.  Every element
    of every gradient is compared (check_dense_grad: the batch's rows within their bounds, every other row +0.0).  Returns
    {quantity: worst error / bound}."""
    worst = {'loss': check_scalar(f'{tag}: loss', got['loss'], ref_s['total'] + ref_t['total'])}
    parts = dtcdr_table_parts(ref_s, ref_t, su, si, tu, ti)
    assert set(got['tables']) == set(TABLES)
    for name in TABLES:
        grad = got['tables'][name]
        worst[name] = check_dense_grad(f'{tag}: gradient {name}', grad, parts[name], grad.shape[1])
    for dom, ref, grads in (('source', ref_s, got['towers'][0]), ('target', ref_t, got['towers'][1])):
        wparts = dtcdr_weight_parts(ref)
        assert len(wparts) == len(grads), (len(wparts), len(grads))
        for j, (part, gr) in enumerate(zip(wparts, grads)):
            gr2 = gr.reshape(part[1].shape)
            worst[f'{dom}.{j}'] = check_dense_grad(f'{tag}: gradient {dom} tower parameter {j}', gr2, part, gr2.shape[1])
    return worst
