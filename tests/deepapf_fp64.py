"""float64 restatement of DeepAPF's row-wise domain step (csrc/cdr_deepapf.hip, fused.FusedDeepAPFStep) on fp64_bounds.EV pairs, shared by
test_gpu_deepapf_rowwise.py (the kernel and the step on the device) and test_deepapf_rowwise_host.py (an fp32 torch-autograd result of
the oracle and three mutations of it on the CPU: the yardstick is shown to bite before it is trusted on the GPU).

For one domain of B rows (key names the overlapped side, oid the other side):
    s = share[key]  o = only[key]  t = other[oid]   xs = s t   xo = o t   pre = W1 x + b1   h = relu(pre)   a = w2 . h
    a_s = -1e31 where key > n_overlap (strictly)   (al_s, al_o) = softmax(a_s, a_o)   e = al_s s + al_o o   z = wp . (e t)   p = sigmoid(z)
    g = w (p - y) / B   ge = g wp t   d_s = <ge, s>   d_o = <ge, o>   dot = al_s d_s + al_o d_o   ga_s = al_s (d_s - dot)   ga_o likewise
    gh = ga w2 [pre > 0]   gx = gh W1   GS = al_s ge + gx_s t   GO = al_o ge + gx_o t   GT = g wp e + gx_s s + gx_o o
    dW1 = gh^T x   db1 = sum gh   dw2 = sum ga h   (each over the 2 B candidates)   dwp = sum_b g e t
Bounds (derived, never tuned; u = 2^-24):
  * the two row contractions (x W1^T and gh W1) are EV.matmul with the REAL accumulation depth of the kernel (``deepapf_depths``: an
    MFMA chain runs over the width rounded up to 8); the bias add is matmul's second ``extra`` rounding;
  * a row dot (a, z, d_s, d_o) is the per-lane chain over the lane's columns (four per 32 columns of width) and the three butterfly steps;
  * dW1, db1 and dw2 run over the 64-row operand of a tile (32 share and 32 only candidates): 64 rows per tile times the tiles a workgroup
    walks, plus the partials added in workgroup order; dwp over the tile's 32 rows: 32 rows per tile times the tiles, plus the grid.  (Both
    are upper bounds of the kernel's chains: db1 and dw2 split the 64 rows over 2..8 threads, dwp adds its tiles per lane first.)
  * for a result whose summation order is not known (torch on the CPU) every depth is the any-order n - 1;
  * a unit is EV.relu in the forward and EV.step in the backward: a unit whose pre-activation is within its bound of 0
    (``ambiguous()``) contributes the either-branch error |ga w2| there, nothing elsewhere; ``ambiguous`` counts them;
  * the masked score -1e31 is exact; its difference to the maximum carries a huge bound into EV.exp, which clamps it: the result is 0
    either way.  A masked occurrence's share row is taken as zeros, as the kernel does (it does not read the row): al_s = 0 makes every
    use of it vanish;
  * g: as clfm_fp64 / dtcdr_fp64 -- (p - y) carries p's bound, the coefficient's own roundings are K_COEF ulps, torch's fp32 backward
    clamp kept;
  * a table's update sums the occurrences' rows into one part (the share table: of BOTH domains) and goes through
    fp64_bounds.apply_fp64 as every other row-wise step."""
import ctypes

import torch

from fp64_bounds import EV, K_COEF, _occ_sums, check_dense_grad, check_scalar, ev_cat, ev_where, f32

ROLES = ('share', 'source_only', 'source_other', 'target_only', 'target_other')
PARAMS = ('W1', 'b1', 'w2', 'wp')


def n_params(D):
    return D * D + 3 * D


def deepapf_grid(B, D):
    """Workgroups of cdr_deepapf_fwd_grad for a batch of B rows: its workspace is one packed parameter vector per workgroup."""
    from recbole_cdr_amd import binding
    need = ctypes.c_size_t(0)
    rc = binding.load().cdr_deepapf_fwd_grad_workspace_bytes(B, D, ctypes.byref(need))
    assert rc == 0, (B, D, rc)
    assert need.value % (4 * n_params(D)) == 0
    return need.value // (4 * n_params(D))


def deepapf_depths(B, D, grid):
    """Accumulation depths of csrc/cdr_deepapf.hip for a launch of ``grid`` workgroups."""
    k8 = -(-D // 8) * 8
    per_wg = -(-(-(-B // 32)) // grid)                       # tiles a workgroup walks
    return dict(fwd=k8, bwd=k8, row=4 * -(-D // 32) + 3, cand=64 * per_wg + grid, rows=32 * per_wg + grid)


def deepapf_domain_fp64(share, only, other, params, key, oid, y, n_overlap, w=1.0, depths=None):
    """One domain.  ``share`` / ``only`` / ``other``: fp32 tables; ``params`` = (W1 [D, D], b1 [D], w2 [1, D] or [D], wp [1, D] or [D]) fp32.
    Returns a dict: 'total', 'bce' (floats), 'g', 'al_s' (EV [B]), 'masked' (bool [B]), 'GS' / 'GO' / 'GT' (EV [B, D]: the occurrence's
    gradient rows), 'dP' [(EV, shape) for W1, b1, w2, wp], 'ambiguous' (units whose ReLU branch the bounds cannot tell)."""
    B, D = key.numel(), share.shape[1]
    d = depths or dict(fwd=D - 1, bwd=D - 1, row=D - 1, cand=2 * B - 1, rows=B - 1)
    w = f32(w)
    W1, b1 = params[0].double(), params[1].double()
    w2, wp = params[2].double().reshape(-1), params[3].double().reshape(-1)
    masked = key > n_overlap
    S = share[key].double() * (~masked).double().unsqueeze(1)
    O, T = only[key].double(), other[oid].double()
    Se, Oe, Te = EV(S), EV(O), EV(T)
    X = ev_cat([Se * Te, Oe * Te])                           # [2 B, D]: the share candidates, then the only candidates
    pre = X.matmul(EV(W1.t().contiguous()), d['fwd'])
    pre = EV(pre.v + b1, pre.e)
    step = pre.step()
    amb = int(pre.ambiguous().sum())
    H = pre.relu()
    A = (H * w2).sum(1, depth=d['row'])
    big = torch.tensor(-1e31, dtype=torch.float32).double().to(share.device)
    a_s = ev_where(masked, EV(big.expand(B).clone()), A[:B])
    a_o = A[B:]
    m = a_s.maximum(a_o)
    es, eo = (a_s - m).exp(), (a_o - m).exp()
    al_s, al_o = es / (es + eo), eo / (es + eo)
    al1, ao1 = al_s.unsqueeze(1), al_o.unsqueeze(1)
    E = al1 * Se + ao1 * Oe
    z = ((E * Te) * wp).sum(1, depth=d['row'])
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
    ge = (g1 * wp) * Te
    d_s, d_o = (ge * Se).sum(1, depth=d['row']), (ge * Oe).sum(1, depth=d['row'])
    dot = al_s * d_s + al_o * d_o
    ga = ev_cat([al_s * (d_s - dot), al_o * (d_o - dot)])    # [2 B]
    ga1 = ga.unsqueeze(1)
    gh = (ga1 * w2) * step
    gx = gh.matmul(EV(W1), d['bwd'], extra=1)
    GS = al1 * ge + gx[:B] * Te
    GO = ao1 * ge + gx[B:] * Te
    GT = (g1 * wp) * E + gx[:B] * Se + gx[B:] * Oe
    dW1 = EV(gh.v.t().contiguous(), gh.e.t().contiguous()).matmul(X, d['cand'])
    db1 = gh.sum(0, depth=d['cand'])
    dw2 = (ga1 * H).sum(0, depth=d['cand'])
    dwp = ((g1 * E) * Te).sum(0, depth=d['rows'])
    dP = [(dW1, (D, D)), (db1, (D,)), (dw2, tuple(params[2].shape)), (dwp, tuple(params[3].shape))]
    return dict(total=w * bce, bce=bce, g=g, al_s=al_s, masked=masked, GS=GS, GO=GO, GT=GT, dP=dP, ambiguous=amb)


def deepapf_packed(ref):
    """The parameter gradient of one domain as one EV vector in the packed layout of cdr_deepapf_fwd_grad's ``dparams``."""
    return ev_cat([EV(ev.v.reshape(-1), ev.e.reshape(-1)) for ev, _ in ref['dP']])


def deepapf_table_parts(ref_s, ref_t, ks, os_, kt, ot):
    """{role: part} of fp64_bounds.apply_fp64 / check_dense_grad: the share table receives the rows of BOTH batches (source occurrences
    first; a row named by both gets the sum), every other table its own domain's."""
    parts = {}
    for role, ids, G in (('share', torch.cat([ks, kt]), ev_cat([ref_s['GS'], ref_t['GS']])), ('source_only', ks, ref_s['GO']),
                         ('source_other', os_, ref_s['GT']), ('target_only', kt, ref_t['GO']), ('target_other', ot, ref_t['GT'])):
        rows, inv = torch.unique(ids, return_inverse=True)
        parts[role] = (rows, *_occ_sums(rows.numel(), inv, G.v, G.v.abs(), G.e))
    return parts


def deepapf_weight_parts(ref_s, ref_t):
    """One part per parameter (W1, b1, w2, wp) of the SUMMED gradient dP_source + dP_target (one more fp32 addition), as two-dimensional
    [rows, columns] gradients (b1 is [D, 1])."""
    out = []
    for (a, shape), (b, _) in zip(ref_s['dP'], ref_t['dP']):
        ev = a + b
        shape2 = shape if len(shape) == 2 else (shape[0], 1)
        v, e = ev.v.reshape(shape2), ev.e.reshape(shape2)
        n = shape2[0]
        out.append((torch.arange(n, device=v.device), v, v.abs(), e, torch.ones(n, device=v.device, dtype=torch.int64)))
    return out


def check_deepapf_result(tag, got, ref_s, ref_t, ks, os_, kt, ot):
    """An fp32 result of the whole BOTH-phase loss and its gradients against the two domains' references.  ``got``: {'loss': float,
    'tables': {role: dense gradient}, 'params': [gradients of W1, b1, w2, wp]}.  Every element of every gradient is compared
    (check_dense_grad: the batch's rows within their bounds, every other row +0.0).  Returns {quantity: worst error / bound}."""
    worst = {'loss': check_scalar(f'{tag}: loss', got['loss'], ref_s['total'] + ref_t['total'])}
    parts = deepapf_table_parts(ref_s, ref_t, ks, os_, kt, ot)
    assert set(got['tables']) == set(ROLES)
    for role in ROLES:
        grad = got['tables'][role]
        worst[role] = check_dense_grad(f'{tag}: gradient {role}', grad, parts[role], grad.shape[1])
    wparts = deepapf_weight_parts(ref_s, ref_t)
    assert len(wparts) == len(got['params']) == len(PARAMS)
    for name, part, gr in zip(PARAMS, wparts, got['params']):
        gr2 = gr.reshape(part[1].shape)
        worst[name] = check_dense_grad(f'{tag}: gradient {name}', gr2, part, gr2.shape[1])
    return worst
