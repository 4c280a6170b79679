"""First-order fp32 error bounds and float64 references shared by the fp64 reference tests (test_gpu_step_fp64.py,
test_gpu_cmf_rowwise.py, test_gpu_dense_loss_fp64.py, test_gpu_bitgcf_fp64.py, ...).

u = 2^-24 is the unit roundoff of fp32 and gamma_k = k u / (1 - k u) the bound of a k-term fp32 sum or product chain (Higham).
apply_fp64 is one optimizer update in float64 from the device state before it, with the per-element bound described in
test_gpu_step_fp64.py's docstring."""
import torch

U32 = 2.0 ** -24            # unit roundoff of fp32
K_SUM = 8                   # the "small constant" of k = D + occurrences + K_SUM (product, subtraction p - n, reg / wd terms)
K_ADAM = 12                 # ulps of the Adam update term (see test_gpu_step_fp64.py's docstring)
K_COEF = 8                  # ulps of the per-occurrence loss coefficient beyond its score error
K_REG = 4                   # ulps of the EmbLoss coefficient reg / (B ||X||) beyond its D-term row sums (fp64 sum, sqrt, two fp32 ops)
LOSS_RTOL = 1e-5
GAMMA = 1e-10               # BPRLoss gamma (recbole): -log(gamma + sigmoid(pos - neg))


def gam(k):
    return k * U32 / (1.0 - k * U32)


def f32(x):
    """A hyper-parameter as the kernel receives it (a float launch argument)."""
    return float(torch.tensor(x, dtype=torch.float32))


def ulp32(x):
    """One ulp of the fp32 value nearest to x (fp64 tensor), elementwise."""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float('inf'))) - a).double()


def _grad_bound(D, G, A, E, occ):
    k = (D + occ + K_SUM).double().unsqueeze(1)
    gk = k * U32 / (1.0 - k * U32)
    return gk * A + (1.0 + gk) * E


def apply_fp64(state, part, D, opt, lr, wd, t, b1=0.9, b2=0.999, eps=1e-8):
    """The optimizer on the part's rows in float64 from the device state BEFORE the step; returns {name: (ref, bound)} for the
    rows' weights (and moments)."""
    rows, G, A, E, occ = part
    lr, wd, b1, b2, eps = f32(lr), f32(wd), f32(b1), f32(b2), f32(eps)
    w = state['w'][rows].double()
    if wd:
        G = G + wd * w
        A = A + wd * w.abs()
    eg = _grad_bound(D, G, A, E, occ)
    if opt == 'sgd':
        wn = w - lr * G
        return {'w': (wn, lr * eg + 2 * U32 * lr * G.abs() + ulp32(wn))}
    m0, v0 = state['m'][rows].double(), state['v'][rows].double()
    m = m0 + (G - m0) * (1 - b1)
    v = b2 * v0 + (1 - b2) * G * G
    em = (1 - b1) * eg + 3 * U32 * (m0.abs() + G.abs() + m.abs()) + ulp32(m)
    ev = (1 - b2) * (2 * G.abs() * eg + eg * eg) + 4 * U32 * (b2 * v0 + (1 - b2) * G * G) + ulp32(v)
    step_size = lr / (1 - b1 ** t)
    c2 = 1.0 / (1 - b2 ** t) ** 0.5
    den = v.sqrt() * c2 + eps
    T = step_size * m / den
    den_lo = (v - ev).clamp(min=0).sqrt() * c2 + eps
    den_hi = (v + ev).sqrt() * c2 + eps
    hi = step_size * torch.maximum((m + em) / den_lo, (m + em) / den_hi)
    lo = step_size * torch.minimum((m - em) / den_lo, (m - em) / den_hi)
    eT = torch.maximum(hi - T, T - lo) + K_ADAM * U32 * torch.maximum(hi.abs(), lo.abs())
    wn = w - T
    return {'w': (wn, eT + ulp32(wn)), 'm': (m, em), 'v': (v, ev)}


def adam_idle_fp64(state, err, t, lr, wd=0.0, b1=0.9, b2=0.999, eps=1e-8):
    """One gradient-free update (number t) of torch.optim.Adam in float64 -- what a row without a gradient goes through in the dense
    sweep and in the deferred form's replay -- from a REFERENCE state that already carries first-order bounds.  ``state`` / ``err``:
    {'w', 'm', 'v'} float64 tensors and their bounds.  The per-update terms are those of apply_fp64 with G = 0 (G = wd w when wd != 0),
    the input bounds propagated: e_m <- b1 e_m + ..., e_v <- b2 e_v + ..., e_w <- e_w + (the update term's bound) + ulp."""
    lr, wd, b1, b2, eps = f32(lr), f32(wd), f32(b1), f32(b2), f32(eps)
    w, m0, v0 = state['w'], state['m'], state['v']
    ew, em0, ev0 = err['w'], err['m'], err['v']
    if wd:
        G = wd * w
        eg = wd * ew + U32 * G.abs()
    else:
        G = torch.zeros_like(w)
        eg = torch.zeros_like(w)
    m = b1 * m0 + (1 - b1) * G
    v = b2 * v0 + (1 - b2) * G * G
    em = b1 * em0 + (1 - b1) * eg + 3 * U32 * (m0.abs() + G.abs() + m.abs()) + ulp32(m)
    ev = b2 * ev0 + (1 - b2) * (2 * G.abs() * eg + eg * eg) + 4 * U32 * v + ulp32(v)
    step_size = lr / (1 - b1 ** t)
    c2 = 1.0 / (1 - b2 ** t) ** 0.5
    T = step_size * m / (v.sqrt() * c2 + eps)
    den_lo = (v - ev).clamp(min=0).sqrt() * c2 + eps
    den_hi = (v + ev).sqrt() * c2 + eps
    hi = step_size * torch.maximum((m + em) / den_lo, (m + em) / den_hi)
    lo = step_size * torch.minimum((m - em) / den_lo, (m - em) / den_hi)
    eT = torch.maximum(hi - T, T - lo) + K_ADAM * U32 * torch.maximum(hi.abs(), lo.abs())
    wn = w - T
    return {'w': wn, 'm': m, 'v': v}, {'w': ew + eT + ulp32(wn), 'm': em, 'v': ev}


def adam_replay_fp64(state, err, t_from, n, lr, wd=0.0, b1=0.9, b2=0.999, eps=1e-8):
    """adam_idle_fp64 over updates t_from + 1 .. t_from + n, each with its own bias corrections."""
    for t in range(t_from + 1, t_from + n + 1):
        state, err = adam_idle_fp64(state, err, t, lr, wd, b1, b2, eps)
    return state, err


# ---------------------------------------------------------------------------------------------------------------------- fp64 losses
# Loss and summed per-row gradients of the three batch losses in float64 (test_gpu_step_fp64.py's docstring derives the bounds).
# A part = (rows, G, A, E, occ): unique row ids, summed gradient, sum|term|, summed coefficient-error terms, occurrences.
#
# What the dense drop-in path (functional.BPRGatherLoss / PointGatherLoss / TwoDomainPointLoss) adds to the row-wise steps:
#   * ``go``: the upstream gradient (a float as the backward kernel reads it).  It multiplies every gradient term and no loss value.  The
#     kernels form go * gcoef[t] (pair: (go * w_d) * gcoef[t]) and go * reg / (B ||X||): one (pair: two) more fp32 roundings on the
#     coefficient and one more on the reg coefficient.  The coefficient's own roundings are 1/B, the products and the division of
#     csrc/cdr_gather_loss.hip's g = ... lines -- at most 6 (BPR), 5 (BCE: pq cancels exactly, both factors are the same fp32 value),
#     3 (MSE) -- so K_COEF = 8 holds them with the upstream factor; the reg coefficient's count K_REG grows by one per extra product.
#   * separate EmbLoss tables (PointGatherLoss reg_user_w / reg_item_w): the norms and the reg terms come from the reg tables' rows
#     and land in the reg tables' gradients (two more parts).
#   * ``detail``: a dict that receives main loss, the two norms, the per-occurrence coefficients g (WITHOUT go) and their bound.

def _occ_sums(n_rows, inv, terms, absum, cerr):
    G = torch.zeros(n_rows, terms.shape[1], device=terms.device, dtype=torch.float64)
    A, E = torch.zeros_like(G), torch.zeros_like(G)
    G.index_add_(0, inv, terms); A.index_add_(0, inv, absum); E.index_add_(0, inv, cerr)
    return G, A, E, torch.bincount(inv, minlength=n_rows)


def bpr_grads_fp64(U, I, uid, pid, nid, reg, go=None, detail=None, k_reg_extra=0, k_score=None):
    """Loss and summed row gradients of  BPRLoss(u.p, u.n) + reg * EmbLoss(u, p)  (recbole; emcdr.py domain_loss) in float64.
    Returns (loss, user part, item part).  ``k_reg_extra``: further fp32 roundings of the EmbLoss coefficient beyond K_REG (the row-sharded
    step's per-rank norm sums and their all-reduce, test_gpu_shard_fp64.py); ``detail`` then also receives the coefficients and their
    relative bound.  ``k_score``: the k of the score's gamma_k (default D + 2: two D-term dot products and their difference on one GPU;
    the dimension layout passes its own, smaller count, test_gpu_dim_fp64.py)."""
    B, D = uid.numel(), U.shape[1]
    k_score = D + 2 if k_score is None else k_score
    ru, inv_u = torch.unique(uid, return_inverse=True)
    ri, inv_i = torch.unique(torch.cat([pid, nid]), return_inverse=True)
    Ur, Ir = U[ru].double(), I[ri].double()
    u, p, n = Ur[inv_u], Ir[inv_i[:B]], Ir[inv_i[B:]]
    ua, pa, na = u.abs(), p.abs(), n.abs()
    x = (u * p).sum(1) - (u * n).sum(1)
    ex = gam(k_score) * ((ua * pa).sum(1) + (ua * na).sum(1)) + U32 * x.abs()
    s, q = torch.sigmoid(x), torch.sigmoid(-x)
    h = GAMMA + s
    g = -(s * q) / h / B
    dgdx = -(s * q * (q - s) * h - (s * q) ** 2) / (h * h) / B
    dgds = -((1 - 2 * s) * h - s * q) / (h * h) / B
    delta = dgdx.abs() * ex + K_COEF * U32 * (dgds.abs() * s + g.abs())
    nu, ni = u.norm(), p.norm()
    main = -torch.log(GAMMA + s).mean()
    loss = main + reg * (nu + ni) / B
    if detail is not None:
        detail.update(main=float(main), nu=float(nu), ni=float(ni), g=g, delta=delta)
    k_reg = K_REG + k_reg_extra
    if go is not None:
        g, delta, k_reg = go * g, abs(go) * delta, k_reg + 1
    cu = (1.0 if go is None else go) * reg / (B * nu) if reg else 0.0
    ci = (1.0 if go is None else go) * reg / (B * ni) if reg else 0.0
    gc = gam(D + k_reg)
    if detail is not None:
        detail.update(cu=float(cu), ci=float(ci), gc=gc)
    g1, delta = g.unsqueeze(1), delta.unsqueeze(1)
    ut = (g1 * (p - n) + cu * u, g1.abs() * (pa + na) + abs(cu) * ua, delta * (p - n).abs() + gc * abs(cu) * ua)
    del x, s, q, h, dgdx, dgds
    it = (torch.cat([g1 * u + ci * p, -g1 * u]), torch.cat([g1.abs() * ua + abs(ci) * pa, g1.abs() * ua]),
          torch.cat([delta * ua + gc * abs(ci) * pa, delta * ua]))
    del u, p, n, ua, pa, na
    return float(loss), (ru, *_occ_sums(ru.numel(), inv_u, *ut)), (ri, *_occ_sums(ri.numel(), inv_i, *it))


def point_grads_fp64(U, I, uid, iid, label, reg, kind, go=None, RU=None, RI=None, detail=None, k_reg_extra=0, k_score=None):
    """Loss and summed row gradients of  MSE(u.i, y)  or  BCE(sigmoid(u.i), y)  + reg * EmbLoss(u, i)  in float64.  With ``RU`` / ``RI``
    the EmbLoss rows come from those tables (same ids) and two more parts, the reg tables' gradients, are returned.  ``k_reg_extra`` /
    ``k_score``: as bpr_grads_fp64's (the score here is one D-term dot product; default D + 2)."""
    B, D = uid.numel(), U.shape[1]
    k_score = D + 2 if k_score is None else k_score
    ru, inv_u = torch.unique(uid, return_inverse=True)
    ri, inv_i = torch.unique(iid, return_inverse=True)
    u, i = U[ru].double()[inv_u], I[ri].double()[inv_i]
    ua, ia = u.abs(), i.abs()
    y = label.double()
    x = (u * i).sum(1)
    ex = gam(k_score) * (ua * ia).sum(1) + U32 * x.abs()
    if kind == 'mse':
        d = x - y
        main = (d * d).mean()
        g = 2 * d / B
        delta = 2 * (ex + U32 * d.abs()) / B + K_COEF * U32 * g.abs()
    else:
        s, q = torch.sigmoid(x), torch.sigmoid(-x)
        main = -(y * torch.log(s).clamp(min=-100) + (1 - y) * torch.log(q).clamp(min=-100)).mean()
        g = (s - y) / B
        delta = s * q * ex / B + K_COEF * U32 * (g.abs() + s / B)
    sep = RU is not None
    ur, ir = (RU[ru].double()[inv_u], RI[ri].double()[inv_i]) if sep else (u, i)
    nu, ni = ur.norm(), ir.norm()
    loss = main + reg * (nu + ni) / B
    if detail is not None:
        detail.update(main=float(main), nu=float(nu), ni=float(ni), g=g, delta=delta)
    k_reg = K_REG + k_reg_extra
    if go is not None:
        g, delta, k_reg = go * g, abs(go) * delta, k_reg + 1
    cu = (1.0 if go is None else go) * reg / (B * nu) if reg else 0.0
    ci = (1.0 if go is None else go) * reg / (B * ni) if reg else 0.0
    gc = gam(D + k_reg)
    if detail is not None:
        detail.update(cu=float(cu), ci=float(ci), gc=gc)
    g1, d1 = g.unsqueeze(1), delta.unsqueeze(1)
    if sep:
        ut, it = (g1 * i, g1.abs() * ia, d1 * ia), (g1 * u, g1.abs() * ua, d1 * ua)
        rut, rit = (cu * ur, abs(cu) * ur.abs(), gc * abs(cu) * ur.abs()), (ci * ir, abs(ci) * ir.abs(), gc * abs(ci) * ir.abs())
        return (float(loss), (ru, *_occ_sums(ru.numel(), inv_u, *ut)), (ri, *_occ_sums(ri.numel(), inv_i, *it)),
                (ru, *_occ_sums(ru.numel(), inv_u, *rut)), (ri, *_occ_sums(ri.numel(), inv_i, *rit)))
    ut = (g1 * i + cu * u, g1.abs() * ia + abs(cu) * ua, d1 * ia + gc * abs(cu) * ua)
    it = (g1 * u + ci * i, g1.abs() * ua + abs(ci) * ia, d1 * ua + gc * abs(ci) * ia)
    return float(loss), (ru, *_occ_sums(ru.numel(), inv_u, *ut)), (ri, *_occ_sums(ri.numel(), inv_i, *it))


def pair_grads_fp64(U, I, doms, go=None, detail=None):
    """The summed loss  sum_d w_d (BCE(sigmoid(u.i), y) + reg_d EmbLoss(u, i))  over the domains ``doms`` = [(uid, iid, y, reg, w)] and its
    per-row gradients in float64 (one part per table: rows, summed gradient, sum|term|, summed coefficient errors, occurrences).  The BCE
    derivative keeps torch's fp32 clamp: (p - y) pq / max(pq, 1e-12) with pq from the fp32 sigmoid (0 where it saturates).  ``detail``: a
    list that receives one dict per domain (main, nu, ni, the coefficients g without w and go, their bound)."""
    D = U.shape[1]
    ru, inv_u = torch.unique(torch.cat([d[0] for d in doms]), return_inverse=True)
    ri, inv_i = torch.unique(torch.cat([d[1] for d in doms]), return_inverse=True)
    Ur, Ir = U[ru].double(), I[ri].double()
    ut, it, parts, loss, off = [[], [], []], [[], [], []], [], 0.0, 0
    f = 1.0 if go is None else go
    k_reg = K_REG if go is None else K_REG + 2
    for uid, iid, label, reg, w in doms:
        B = uid.numel()
        u, i = Ur[inv_u[off:off + B]], Ir[inv_i[off:off + B]]
        off += B
        ua, ia = u.abs(), i.abs()
        y = label.double()
        x = (u * i).sum(1)
        ex = gam(D + 2) * (ua * ia).sum(1) + U32 * x.abs()
        s, q = torch.sigmoid(x), torch.sigmoid(-x)
        p32 = torch.sigmoid(x.float())
        pq = ((1 - p32) * p32).double()
        clamp = torch.where(pq < 1e-12, pq / 1e-12, torch.ones_like(pq))
        main = -(y * torch.log(s).clamp(min=-100) + (1 - y) * torch.log(q).clamp(min=-100)).mean()
        if detail is not None:
            detail.append(dict(g=(s - y) * clamp / B, delta=s * q * ex / B + K_COEF * U32 * ((s - y).abs() / B + s / B)))
        g = f * w * (s - y) * clamp / B
        delta = abs(f) * w * (s * q * ex / B + K_COEF * U32 * ((s - y).abs() / B + s / B))
        nu, ni = u.norm(), i.norm()
        emb = (nu + ni) / B
        loss += w * (float(main) + reg * float(emb))
        parts.append((float(main), float(emb)))
        if detail is not None:
            detail[-1].update(main=float(main), nu=float(nu), ni=float(ni))
        cu = f * w * reg / (B * nu) if reg else 0.0
        ci = f * w * reg / (B * ni) if reg else 0.0
        gc = gam(D + k_reg)
        g1, d1 = g.unsqueeze(1), delta.unsqueeze(1)
        for acc, t in ((ut, (g1 * i + cu * u, g1.abs() * ia + abs(cu) * ua, d1 * ia + gc * abs(cu) * ua)),
                       (it, (g1 * u + ci * i, g1.abs() * ua + abs(ci) * ia, d1 * ua + gc * abs(ci) * ia))):
            for j in range(3):
                acc[j].append(t[j])
    upart = (ru, *_occ_sums(ru.numel(), inv_u, *[torch.cat(a) for a in ut]))
    ipart = (ri, *_occ_sums(ri.numel(), inv_i, *[torch.cat(a) for a in it]))
    return loss, parts, upart, ipart


# ---------------------------------------------------------------------------------------------------------------------- dense checker
# What test_gpu_dense_loss_fp64.py holds the drop-in losses to, and what test_fp64_bounds.py feeds an fp32 autograd result (and three
# mutations of it) through without a GPU.  No sampling: every scalar, every coefficient, every element of every row of every gradient.

def check_scalar(tag, got, want):
    assert abs(got - want) <= LOSS_RTOL * abs(want), f'{tag}: {got!r} vs fp64 {want!r} (rel {abs(got - want) / max(abs(want), 1e-300):.3g})'
    return abs(got - want) / (LOSS_RTOL * abs(want)) if want else 0.0


def check_dense_grad(tag, grad, part, D):
    """A dense [rows, D] gradient against a part: the batch's rows within _grad_bound element by element, EVERY other row +0.0 bit for
    bit.  Returns the worst error / bound."""
    rows, G, A, E, occ = part
    assert grad.dim() == 2 and grad.shape[1] == D == G.shape[1] and grad.dtype == torch.float32, (tag, tuple(grad.shape), grad.dtype)
    n = grad.shape[0]
    touched = torch.zeros(n, dtype=torch.bool, device=grad.device)
    touched[rows] = True
    assert int(touched.sum()) == rows.numel() and bool((occ > 0).all()), f'{tag}: the reference rows are not the distinct batch rows'
    dirty = (grad.contiguous().view(torch.int32) != 0).any(1) & ~touched
    assert not bool(dirty.any()), (f'{tag}: {int(dirty.sum())} of {n - rows.numel()} rows outside the batch are not +0.0, '
                                   f'e.g. row {int(torch.nonzero(dirty)[0])}: {grad[int(torch.nonzero(dirty)[0])][:4].tolist()}')
    got = grad[rows].double()
    assert bool(torch.isfinite(got).all()), f'{tag}: non-finite values'
    bound = _grad_bound(D, G, A, E, occ)
    err = (got - G).abs()
    r = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    worst = float(r.max())
    if worst > 1.0:
        j = int(r.argmax())
        row, col = j // D, j % D
        raise AssertionError(f'{tag}: error / bound = {worst:.3g} at table row {int(rows[row])} col {col} ({int(occ[row])} occurrences): '
                             f'got {float(got[row, col])!r} want {float(G[row, col])!r} bound {float(bound[row, col]):.3g}')
    return worst


def check_dense_result(tag, got, ref, D):
    """got: {'scalars': {name: float}, 'coefs': [tensor or None], 'grads': [dense gradient]}; ref: {'scalars': {name: float64 value},
    'coefs': [(g, delta)], 'parts': [part]} -- the same names, the same order.  Returns {quantity: worst error / bound}."""
    assert set(got['scalars']) == set(ref['scalars']) and len(got['grads']) == len(ref['parts']) and len(got['coefs']) == len(ref['coefs'])
    worst = {}
    for k, v in ref['scalars'].items():
        worst[k] = check_scalar(f'{tag}: {k}', got['scalars'][k], v)
    for j, (c, (g, delta)) in enumerate(zip(got['coefs'], ref['coefs'])):
        if c is None:
            continue
        assert c.shape == g.shape, (tag, c.shape, g.shape)
        err = (c.double() - g).abs()
        r = torch.where(err > 0, err / delta.clamp(min=1e-300), torch.zeros_like(err))
        worst[f'coef{j}'] = float(r.max())
        assert worst[f'coef{j}'] <= 1.0, (f'{tag}: coefficient of occurrence {int(r.argmax())} of batch {j}: got {float(c[int(r.argmax())])!r} '
                                          f'want {float(g[int(r.argmax())])!r}, error / bound = {worst[f"coef{j}"]:.3g}')
    for j, (gr, part) in enumerate(zip(got['grads'], ref['parts'])):
        worst[f'grad{j}'] = check_dense_grad(f'{tag}: gradient {j}', gr, part, D)
    return worst


# ---------------------------------------------------------------------------------------------------------------------- running bounds
# test_gpu_gemm_fp64.py and test_gpu_rowmodels_fp64.py restate a kernel operation by operation on EV pairs: ``v`` is the float64 value
# of the quantity, ``e`` a bound of |what the fp32 kernel holds - v| carried along by the standard model fl(a op b) = (a op b)(1 + d),
# |d| <= u (Higham, Accuracy and Stability, ch. 3: the running error analysis), with the input errors propagated through each
# operation's derivative.  Every rule charges its OWN rounding on top (an fma that saves one only makes the bound loose), a sum of n
# terms in ANY order gamma_{n-1} of the sum of magnitudes (the caller passes the real depth of a reduction whose order is known), and
# every rounding TINY = 2^-126 for a result that leaves the normal range (a flushed or denormal intermediate).
TINY = 2.0 ** -126
K_EXP = 2                   # ulps of expf (ocml documents 1)
K_TANH_EV = 4               # ulps of tanhf, as test_gpu_map_step_fp64.K_TANH
K_SIG_EV = 4                # expf, add and division of 1 / (1 + expf(-z)), as test_gpu_conet_fp64.K_SIG


class EV:
    __slots__ = ('v', 'e')

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def lift(x, like=None):
        if isinstance(x, EV):
            return x
        if not isinstance(x, torch.Tensor):
            x = torch.tensor(float(x), dtype=torch.float64, device=like.v.device if like is not None else None)
        return EV(x.double())

    @staticmethod
    def _rnd(v, e, k=1):
        """k roundings of a result whose exact-arithmetic value is v and whose propagated error is e."""
        return EV(v, e + k * U32 * (v.abs() + e) + TINY)

    @property
    def mag(self):
        return self.v.abs() + self.e

    def __neg__(self):
        return EV(-self.v, self.e)

    def __add__(self, o):
        o = EV.lift(o, self)
        return EV._rnd(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = EV.lift(o, self)
        return EV._rnd(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return EV.lift(o, self) - self

    def __mul__(self, o):
        o = EV.lift(o, self)
        return EV._rnd(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = EV.lift(o, self)
        q = self.v / o.v
        lo = (o.v.abs() - o.e).clamp(min=1e-300)
        return EV._rnd(q, (self.e + q.abs() * o.e) / lo)

    def __getitem__(self, idx):
        return EV(self.v[idx], self.e[idx])

    def unsqueeze(self, d):
        return EV(self.v.unsqueeze(d), self.e.unsqueeze(d))

    def exact_scale(self, c):
        """Multiplication by a power of two (or by an exact 0 / 1 mask): no rounding."""
        return EV(self.v * c, self.e * abs(c) if not isinstance(c, torch.Tensor) else self.e * c.abs())

    def sum(self, dim, depth=None, keepdim=False):
        """A sum of n terms; ``depth`` = the longest chain of additions a term goes through (default n - 1: any order)."""
        n = self.v.shape[dim]
        k = max(n - 1, 0) if depth is None else depth
        m = self.mag.sum(dim, keepdim=keepdim)
        return EV(self.v.sum(dim, keepdim=keepdim), self.e.sum(dim, keepdim=keepdim) + gam(k) * m + TINY)

    def amax(self, dim, keepdim=False):
        """max of computed values (fmaxf is exact): |max x^ - max x| <= the largest e among the entries that CAN be the computed maximum
        (v + e reaches the largest v - e)."""
        cand = (self.v + self.e) >= (self.v - self.e).amax(dim, keepdim=True)
        return EV(self.v.amax(dim, keepdim=keepdim), (self.e * cand).amax(dim, keepdim=keepdim))

    def maximum(self, o):
        o = EV.lift(o, self)
        return EV(torch.maximum(self.v, o.v), torch.maximum(self.e, o.e))

    def relu(self):
        """1-Lipschitz: the error passes where the unit can be alive, none where it is dead beyond its bound."""
        return EV(self.v.clamp(min=0), self.e * (self.v > -self.e))

    def step(self):
        """[x > 0] as the kernel evaluates it on ITS value: exact unless |x| <= e, where either branch may be taken (error 1)."""
        return EV((self.v > 0).double(), (self.v.abs() <= self.e).double() * (self.e > 0))

    def ambiguous(self):
        return (self.v.abs() <= self.e) & (self.e > 0)

    def exp(self):
        v = torch.exp(self.v)
        e = self.e.clamp(max=700.0)             # (a masked score of -1e31 carries a huge bound into an exponential that is 0 either way)
        return EV(v, v * torch.expm1(e) + K_EXP * U32 * v * torch.exp(e) + TINY)

    def tanh(self):
        a = torch.tanh(self.v)
        return EV(a, self.e.clamp(max=2.0) * (1 - a * a + 2 * self.e).clamp(max=1.0) + K_TANH_EV * ulp32(a) + TINY)

    def sigmoid(self):
        p = torch.sigmoid(self.v)
        return EV(p, (p * (1 - p) + self.e).clamp(max=0.25) * self.e + K_SIG_EV * U32 * p + TINY)

    def matmul(self, o, depth, extra=2):
        """self [M, K] @ o [K, N] accumulated along a chain of ``depth`` additions; ``extra`` roundings for the products and the
        epilogue's first operation."""
        o = EV.lift(o, self)
        v = self.v @ o.v
        m = self.mag @ o.mag
        e = self.e @ o.v.abs() + self.v.abs() @ o.e + self.e @ o.e
        return EV(v, e + gam(depth + extra) * m + TINY)

    def ratio(self, got):
        """error / bound of an fp32 result, elementwise (0 where the result is exact)."""
        err = (got.double() - self.v).abs()
        return torch.where(err > 0, err / self.e.clamp(min=1e-300), torch.zeros_like(err))


def ev_cat(parts, dim=0):
    return EV(torch.cat([p.v for p in parts], dim), torch.cat([p.e for p in parts], dim))


def ev_where(cond, a, b):
    a, b = EV.lift(a), EV.lift(b)
    return EV(torch.where(cond, a.v, b.v), torch.where(cond, a.e, b.e))


def colsum_depth(rows):
    """cdr_colsum (csrc/cdr_rows.hip:166-198, 618-632): slabs of 64 rows (at most 128 slabs, then longer ones); inside a slab a wave adds
    every fourth row into four accumulators (rows / 16 additions), three more to join them, three for the four waves; one thread then adds
    the slabs in order."""
    per = 64
    slabs = -(-rows // per)
    if slabs > 128:
        per = -(-rows // 128)
        slabs = -(-rows // per)
    return -(-per // 16) + 3 + 3 + slabs
