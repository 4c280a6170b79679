"""float64 restatement of NATR's full-sort scoring (csrc/cdr_natr_fullsort.hip and functional.natr_history_summary; reference natr.py:112-156)
on fp64_bounds.EV pairs, shared by test_gpu_natr_fullsort.py (the kernels, the model and the trainer on the device) and
test_natr_fullsort_host.py (the algebra against the oracle, an fp32 CPU result and three mutations of it: the yardstick is shown to bite
before it is trusted).

Pair stage, for key row a = su (an fp32 INPUT here), p = the key's own target row, q = the other side's row, w = the gate's weight:
    D_ = a - p    M = |a| - |p|    wh = w / 2
    g  = sum_f (wh_f D__f) q_f + sum_f (wh_f M_f) |q_f|        pq = sum_f p_f q_f        dq = sum_f D__f q_f
    score = sigmoid(pq + sigmoid(g) dq)
Bounds (derived, never tuned; u = 2^-24):
  * D_ and M: one subtraction each (|x| is exact); wh = w / 2 exact; wh D_ and wh M one product each;
  * pq, dq, g: the MFMA chain adds the products of a row into one accumulator, two per instruction, padding adds exact zeros: a term goes
    through at most DP = 32 ceil(Dt / 32) additions in pq and dq and 2 DP in g (``fullsort_depths``); one more rounding is charged for the
    products (the MFMA fuses them: that only loosens the bound);
  * EV.sigmoid (K_SIG_EV ulps) of g, one product and one sum (the kernel's fma saves a rounding), EV.sigmoid of the logit;
  * for a result whose summation order is not known (torch on the CPU) every depth is the any-order n - 1 (``depths=None``).
Summary stage (functional.natr_history_summary = gather_rows, linear, cdr_natr_att_fwd; csrc/cdr_rowmodels.hip natr_fwd_kernel):
    he = src[hist[key]] Wt^T + bt   x_l = wu . relu(pk (.) he_l) + bu + (mask_l ? 0 : -10000)   att = softmax_l(x)   su = sum_l att_l he_l
  * he: EV.matmul, a chain of at most Ds additions and one more rounding for the products, then the bias by EV's addition;
  * x_l: one product, EV.relu (the bound passes wherever the unit can be alive), one product with wu, a lane's chain over ceil(Dt / 64)
    features and six exchange steps, then the two additions; the max is exact on the computed values; subtraction, EV.exp, the
    denominator's chain of L additions, one division; su: one product and a chain of L additions."""
import torch

from fp64_bounds import EV, ev_cat

NEG_BIAS = -10000.0


def fullsort_depths(Dt):
    """Accumulation depths of csrc/cdr_natr_fullsort.hip at width Dt."""
    dp = 32 * (-(-Dt // 32))
    return dict(dot=dp, gate=2 * dp)


def _abs(x):
    return EV(x.v.abs(), x.e)


def natr_pair_fp64(key_is_item, su, key_tab, other_tab, uid, N, w, depths=None, cover_predict=False, bd=None):
    """EV [U, N] of the scores (``v`` the float64 value, ``e`` the bound of an fp32 result).  ``su`` [keys, Dt] fp32: by position for user
    keys, by item id for item keys.  Tensors fp32 on one device.  ``cover_predict`` (with the gate's bias ``bd``): the bound also holds
    ``predict``'s operation order (cdr_natr_att_fwd: b_s, b_p, e^b_s / (e^b_s + e^b_p), the blended row's dot), so ONE reference holds
    the kernel and ``predict`` alike."""
    Dt = key_tab.shape[1]
    d = dict(depths) if depths is not None else dict(dot=Dt - 1, gate=2 * Dt - 1)
    uid = uid.reshape(-1)
    a = su if isinstance(su, EV) else EV(su.double())          # (an EV: the float64 summary with its bound, for a result computed from either)
    if key_is_item:
        a, p, q = a[:N], key_tab[:N].double(), other_tab[uid].double()
    else:
        p, q = key_tab[uid].double(), other_tab[:N].double()
    p, q = EV(p), EV(q)
    wh = EV(w.double().reshape(1, -1) * 0.5)
    Dd, M = a - p, _abs(a) - _abs(p)
    qt = EV(q.v.t().contiguous())
    pq = p.matmul(qt, d['dot'], extra=1)
    dq = Dd.matmul(qt, d['dot'], extra=1)
    t1, t2 = wh * Dd, wh * M
    g = ev_cat([t1, t2], 1).matmul(EV(torch.cat([qt.v, qt.v.abs()], 0)), d['gate'], extra=1)
    z = pq + g.sigmoid() * dq
    s = z.sigmoid()
    if cover_predict:
        # the direct form as natr_fwd_kernel evaluates it (a lane's chain over ceil(Dt / 64) features and six exchange steps per row sum):
        # the same number, another operation sequence; the bound becomes the larger of the two forms' (small cases only: [keys, others, Dt])
        lane = -(-Dt // 64) + 6
        aE, pE, qE, wE = a.unsqueeze(1), p.unsqueeze(1), q.unsqueeze(0), w.double().reshape(1, 1, -1)
        b0 = float(bd.double().reshape(-1)[0])
        b_s = ((aE * qE).relu() * wE).sum(2, depth=lane) + b0
        b_p = ((pE * qE).relu() * wE).sum(2, depth=lane) + b0
        e_s, e_p = b_s.exp(), b_p.exp()
        beta = e_s / (e_s + e_p)
        zu = beta.unsqueeze(2) * aE + (1.0 - beta).unsqueeze(2) * pE
        s2 = (zu * qE).sum(2, depth=lane).sigmoid()
        s = EV(s.v, torch.maximum(s.e, s2.e + (s2.v - s.v).abs()))
    return EV(s.v.t().contiguous(), s.e.t().contiguous()) if key_is_item else s


def natr_summary_fp64(src, hist, mask_mat, key_tab, keys, Wt, bt, wu, bu, budget=1 << 24):
    """EV [K, Dt] of su for the keys ``keys``, in key chunks of at most ``budget`` [keys x L x max(Ds, Dt)] elements."""
    keys = keys.reshape(-1)
    L, Dt, Ds = hist.shape[1], Wt.shape[0], Wt.shape[1]
    per = max(1, budget // (L * max(Ds, Dt)))
    Wtt = EV(Wt.double().t().contiguous())
    btd, wud, bud = bt.double().reshape(1, 1, -1), wu.double().reshape(1, 1, -1), float(bu.double().reshape(-1)[0])
    lane = -(-Dt // 64) + 6
    vs, es = [], []
    for s0 in range(0, keys.numel(), per):
        ids = keys[s0:s0 + per]
        n = ids.numel()
        he = EV(src[hist[ids]].double().reshape(n * L, Ds)).matmul(Wtt, Ds, extra=1)
        he = EV(he.v.view(n, L, Dt), he.e.view(n, L, Dt)) + btd
        pk = EV(key_tab[ids].double().unsqueeze(1))
        x = ((pk * he).relu() * wud).sum(2, depth=lane)
        x = (x + bud) + torch.where(mask_mat[ids] != 0, 0.0, NEG_BIAS).double()
        ex = (x - x.amax(1, keepdim=True)).exp()
        att = ex / ex.sum(1, depth=L, keepdim=True)
        su = (att.unsqueeze(2) * he).sum(1, depth=L)
        vs.append(su.v)
        es.append(su.e)
    return EV(torch.cat(vs), torch.cat(es))


def natr_fullsort_fp64(c, depths=None, su=None):
    """Both stages for a ``make_case`` dict: the pair stage on ``su`` (fp32; the float64 summary rounded to fp32 if not given)."""
    if su is None:
        su = natr_summary_fp64(c['src'], c['hist'], c['mask_mat'], c['key_tab'], c['keys'], c['Wt'], c['bt'], c['wu'], c['bu']).v.float()
    return natr_pair_fp64(c['key_is_item'], su, c['key_tab'], c['other_tab'], c['uid'], c['N'], c['wd'], depths=depths)


def pair_fp32(key_is_item, su, key_tab, other_tab, uid, N, w, bd=None, drop_absq=False, swap=False, one_sided_bd=False):
    """The pair stage in fp32 torch (any device), the kernel's formula; the three switches are the mutations the host test feeds the
    yardstick: the |q| term dropped, beta and 1 - beta swapped, b_d kept in one logit only."""
    uid = uid.reshape(-1)
    if key_is_item:
        a, p, q = su[:N], key_tab[:N], other_tab[uid]
    else:
        a, p, q = su, key_tab[uid], other_tab[:N]
    wh = 0.5 * w.reshape(1, -1)
    Dd, M = a - p, a.abs() - p.abs()
    g = (wh * Dd) @ q.t()
    if not drop_absq:
        g = g + (wh * M) @ q.abs().t()
    if one_sided_bd:
        g = g + bd.reshape(())
    sg = 1.0 / (1.0 + torch.exp(-g))
    if swap:
        sg = 1.0 - sg
    z = p @ q.t() + sg * (Dd @ q.t())
    s = 1.0 / (1.0 + torch.exp(-z))
    return s.t().contiguous() if key_is_item else s


def make_case(Dt, Ds, L, U, N, key_is_item, device='cpu'):
    """Tables, parameters and a history for one case, generator seeded with Dt + Ds + N + (1 in item mode).  Scales: target rows
    randn x s with s^2 sqrt(Dt) = 0.8, so p . q has a standard deviation of 0.8; the transfer layer is scaled so that transferred rows
    have about the same size; final logits stay inside about +-8 and fp32 sigmoids do not saturate into ties.  The history matrix
    [keys, L] holds source ids (0 = padding) with lengths drawn from 0 .. L + 3 and three planted keys: length 0 (all padding: uniform
    attention over pad rows), length 1, and a length beyond L (mask all ones, natr.py:80-81).  Keys: the evaluated users (user keys) or
    all items 0 .. N - 1 (item keys)."""
    g = torch.Generator().manual_seed(Dt + Ds + N + (1 if key_is_item else 0))
    s = (0.8 / Dt ** 0.5) ** 0.5
    n_users, n_items, n_src = U + 3, N + 3, 37
    user_tab = torch.randn(n_users, Dt, generator=g) * s
    item_tab = torch.randn(n_items, Dt, generator=g) * s
    src = torch.randn(n_src, Ds, generator=g) * 0.5
    Wt = torch.randn(Dt, Ds, generator=g) * (s / (0.5 * Ds ** 0.5))
    bt = torch.randn(Dt, generator=g) * 0.05
    wu, wd = torch.randn(1, Dt, generator=g), torch.randn(1, Dt, generator=g)
    bu, bd = torch.tensor([0.1]), torch.tensor([0.5])
    uid = torch.randperm(n_users - 1, generator=g)[:U] + 1
    n_keys = n_items if key_is_item else n_users
    lens = torch.randint(0, L + 4, (n_keys,), generator=g)
    planted = [0, 1, 2] if key_is_item else [int(x) for x in uid[:3]]
    for row, ln in zip(planted, (0, 1, L + 2)):
        if row < n_keys:
            lens[row] = ln
    hist = torch.randint(1, n_src, (n_keys, L), generator=g)
    mask_mat = (torch.arange(L) < lens.unsqueeze(1)).float()
    hist = hist * (mask_mat != 0)
    keys = torch.arange(N) if key_is_item else uid
    key_tab, other_tab = (item_tab, user_tab) if key_is_item else (user_tab, item_tab)
    dv = lambda t: t.to(device)
    return dict(key_is_item=key_is_item, src=dv(src), hist=dv(hist), mask_mat=dv(mask_mat), lens=dv(lens), key_tab=dv(key_tab),
                other_tab=dv(other_tab), keys=dv(keys), uid=dv(uid), N=N, Wt=dv(Wt), bt=dv(bt), wu=dv(wu), bu=dv(bu), wd=dv(wd), bd=dv(bd))
