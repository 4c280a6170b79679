"""float64 restatement of DeepAPF's full-sort scoring kernel (csrc/cdr_deepapf_fullsort.hip; reference deepapf.py:111-161) on
fp64_bounds.EV pairs, shared by test_gpu_deepapf_fullsort.py (the kernel, the model and the trainer on the device) and
test_deepapf_fullsort_host.py (an fp32 CPU result and three mutations of it: the yardstick is shown to bite before it is trusted).

For user u and item i (key = the overlapped side's id; S / O = the key side's share / target-only row, T = the other side's row):
    x_c = c T   pre_c = W1 x_c + b1   a_c = w2 . relu(pre_c)   (c = S, O)     masked = key > n_overlap (strictly)
    m = max(a_S, a_O)   e_c = exp(a_c - m)   al_c = e_c / (e_S + e_O)
    z_c = sum_f (wp_f user_f) item_f   (the user-side row is multiplied by wp while it is staged, the item-side row sits in registers)
    z = al_S z_S + al_O z_O,  or z_O where masked (al_S = 0 and al_O = 1 exactly: the kernel skips or discards the share candidate)
    p = 1 / (1 + exp(-z))
Bounds (derived, never tuned; u = 2^-24):
  * x_c: one product.  pre_c: EV.matmul with the kernel's real accumulation depth -- the MFMA chain adds the D products of a row into
    one accumulator (zero padding adds exact zeros) -- plus matmul's two ``extra`` roundings for the products and the bias add;
  * a_c and z_c: a lane's chain over its at most min(D, 16 ceil(D / 32)) features and one exchange with the other wave half
    (``fullsort_depths``); the products of a_c are charged by EV's multiplication, an fma that saves a rounding only loosens the bound;
  * a unit whose pre-activation lies within its bound of 0 may take either branch: EV.relu passes the bound wherever the unit can be alive;
  * softmax: subtraction, EV.exp (K_EXP ulps), sum, division; the final combination two products and a sum; EV.sigmoid (K_SIG_EV ulps);
  * for a result whose summation order is not known (torch on the CPU) every depth is the any-order n - 1 (``depths=None``);
  * ``cover_predict``: ``predict`` (cdr_apf_prod, the fp32-MFMA contraction, cdr_apf_combine) forms z as wp . ((al_S S + al_O O) T) and runs
    its row sums over up to D terms; with this flag every row depth is D and z's bound is the larger of the two forms', so ONE reference
    holds the kernel and ``predict`` alike (the values of the two forms are the same number)."""
import torch

from fp64_bounds import EV, ev_where


def fullsort_depths(D):
    """Accumulation depths of csrc/cdr_deepapf_fullsort.hip at width D."""
    nb = -(-D // 32)
    return dict(fwd=D, row=min(D, 16 * nb) + 1)


def _att(X, W1t, b1, w2, d):
    pre = X.matmul(W1t, d['fwd'])
    pre = EV(pre.v + b1, pre.e)
    amb = int(pre.ambiguous().sum())
    return (pre.relu() * w2).sum(1, depth=d['row']), amb


def deepapf_fullsort_fp64(key_is_item, share, only, other, uid, N, n_overlap, W1, b1, w2, wp, depths=None, cover_predict=False,
                          budget=1 << 25):
    """EV [U, N] of the scores (``v`` the float64 value, ``e`` the bound of an fp32 result) and the number of ReLU units whose branch the
    bounds cannot tell.  Tables and parameters fp32 on one device; evaluated in user chunks of at most ``budget`` [pairs x D] elements."""
    D = share.shape[1]
    d = dict(depths) if depths is not None else dict(fwd=D - 1, row=D - 1)
    if cover_predict:
        d = dict(fwd=max(d['fwd'], D), row=max(d['row'], D))
    W1t = EV(W1.double().t().contiguous())
    b1d, w2d, wpd = b1.double().reshape(-1), w2.double().reshape(-1), wp.double().reshape(-1)
    uid = uid.reshape(-1)
    U = uid.numel()
    per = max(1, budget // (N * D))
    vs, es, amb = [], [], 0
    for s0 in range(0, U, per):
        ids = uid[s0:s0 + per]
        u = ids.numel()
        if key_is_item:
            masked = (torch.arange(N, device=share.device) > n_overlap).view(1, N).expand(u, N)
            S = share[:N].double().view(1, N, D).expand(u, N, D)
            O = only[:N].double().view(1, N, D).expand(u, N, D)
            T = other[ids].double().view(u, 1, D).expand(u, N, D)
        else:
            masked = (ids > n_overlap).view(u, 1).expand(u, N)
            S = share[ids].double().view(u, 1, D).expand(u, N, D)
            O = only[ids].double().view(u, 1, D).expand(u, N, D)
            T = other[:N].double().view(1, N, D).expand(u, N, D)
        masked = masked.reshape(-1)
        S = S.reshape(u * N, D) * (~masked).double().unsqueeze(1)            # a masked key's share row is not read: zeros
        O, T = O.reshape(u * N, D), T.reshape(u * N, D)
        Se, Oe, Te = EV(S), EV(O), EV(T)
        a_s, n1 = _att(Se * Te, W1t, b1d, w2d, d)
        a_o, n2 = _att(Oe * Te, W1t, b1d, w2d, d)
        amb += n1 + n2
        m = a_s.maximum(a_o)
        ex_s, ex_o = (a_s - m).exp(), (a_o - m).exp()
        den = ex_s + ex_o
        al_s, al_o = ex_s / den, ex_o / den
        wpe = EV(wpd.view(1, D).expand(u * N, D))
        if key_is_item:                                                      # the user-side row carries wp
            z_s, z_o = ((wpe * Te) * Se).sum(1, depth=d['row']), ((wpe * Te) * Oe).sum(1, depth=d['row'])
        else:
            z_s, z_o = ((wpe * Se) * Te).sum(1, depth=d['row']), ((wpe * Oe) * Te).sum(1, depth=d['row'])
        z = ev_where(masked, z_o, al_s * z_s + al_o * z_o)
        if cover_predict:
            al_s0 = ev_where(masked, EV(torch.zeros_like(al_s.v)), al_s)
            al_o0 = ev_where(masked, EV(torch.ones_like(al_o.v)), al_o)
            E = al_s0.unsqueeze(1) * Se + al_o0.unsqueeze(1) * Oe
            z2 = ((E * Te) * wpd).sum(1, depth=d['row'])
            z = EV(z.v, torch.maximum(z.e, z2.e + (z2.v - z.v).abs()))
        p = z.sigmoid()
        vs.append(p.v.view(u, N))
        es.append(p.e.view(u, N))
    return EV(torch.cat(vs), torch.cat(es)), amb


def fullsort_fp32(key_is_item, share, only, other, uid, N, n_overlap, W1, b1, w2, wp, strict=True, drop_b1=False, swap=False):
    """The same scores in fp32 torch (any device), the kernel's operation sequence; the three switches are the mutations the host test
    feeds the yardstick: a non-strict mask (key >= n_overlap), a dropped b1, swapped softmax weights."""
    uid = uid.reshape(-1)
    u, D = uid.numel(), share.shape[1]
    if key_is_item:
        key = torch.arange(N, device=share.device).view(1, N).expand(u, N)
        S, O, T = share[:N].view(1, N, D), only[:N].view(1, N, D), other[uid].view(u, 1, D)
        z_s, z_o = (((wp.view(-1) * T) * S).sum(-1), ((wp.view(-1) * T) * O).sum(-1))
    else:
        key = uid.view(u, 1).expand(u, N)
        S, O, T = share[uid].view(u, 1, D), only[uid].view(u, 1, D), other[:N].view(1, N, D)
        z_s, z_o = (((wp.view(-1) * S) * T).sum(-1), ((wp.view(-1) * O) * T).sum(-1))
    masked = key >= n_overlap if not strict else key > n_overlap
    bias = torch.zeros_like(b1) if drop_b1 else b1
    a_s = torch.relu((S * T) @ W1.t() + bias) @ w2.view(-1)
    a_o = torch.relu((O * T) @ W1.t() + bias) @ w2.view(-1)
    m = torch.maximum(a_s, a_o)
    e_s, e_o = torch.exp(a_s - m), torch.exp(a_o - m)
    al_s, al_o = e_s / (e_s + e_o), e_o / (e_s + e_o)
    if swap:
        al_s, al_o = al_o, al_s
    z = torch.where(masked, z_o.expand(u, N), al_s * z_s + al_o * z_o)
    return 1.0 / (1.0 + torch.exp(-z))


def make_case(D, U, N, n_overlap, key_is_item, device='cpu', n_user_rows=None):
    """The issue's input recipe: tables randn x 0.3, W1 = randn x sqrt(2 / 2D), b1 = randn x 0.1, w2 and wp = randn x 0.5, generator seeded
    with D + N + (1 in item mode).  Key ids n_overlap and n_overlap + 1 both occur (where the id range allows): overlap_items has items
    0..N-1; overlap_users evaluates the user ids n_overlap - U // 2 + 1 ... (clamped to >= 1) in a shuffled order."""
    g = torch.Generator().manual_seed(D + N + (1 if key_is_item else 0))
    n_users = n_user_rows or (max(n_overlap, 1) + U + 2)
    n_items = N + 3
    rows_s, rows_o, rows_t = (n_items, n_items, n_users) if key_is_item else (n_users, n_users, n_items)
    share = torch.randn(rows_s, D, generator=g) * 0.3
    only = torch.randn(rows_o, D, generator=g) * 0.3
    other = torch.randn(rows_t, D, generator=g) * 0.3
    W1 = torch.randn(D, D, generator=g) * (2.0 / (2 * D)) ** 0.5
    b1 = torch.randn(D, generator=g) * 0.1
    w2, wp = torch.randn(1, D, generator=g) * 0.5, torch.randn(1, D, generator=g) * 0.5
    if key_is_item:
        uid = torch.randperm(n_users - 1, generator=g)[:U] + 1
    else:
        lo = max(1, min(n_overlap - U // 2 + 1, n_users - U))
        if n_overlap >= N:                                                   # the "nobody masked" case: every evaluated id <= n_overlap
            lo = max(1, n_overlap - U + 1)
        uid = (torch.arange(U) + lo)[torch.randperm(U, generator=g)]
    dv = lambda t: t.to(device)
    return dict(key_is_item=key_is_item, share=dv(share), only=dv(only), other=dv(other), uid=dv(uid), N=N, n_overlap=n_overlap,
                W1=dv(W1), b1=dv(b1), w2=dv(w2), wp=dv(wp))
