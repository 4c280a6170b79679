"""First-order fp32 error bounds shared by the fp64 reference tests (test_gpu_step_fp64.py, test_gpu_bitgcf_fp64.py).

u = 2^-24 is the unit roundoff of fp32 and gamma_k = k u / (1 - k u) the bound of a k-term fp32 sum or product chain (Higham).
apply_fp64 is one optimizer update in float64 from the device state before it, with the per-element bound described in
test_gpu_step_fp64.py's docstring."""
import torch

U32 = 2.0 ** -24            # unit roundoff of fp32
K_SUM = 8                   # the "small constant" of k = D + occurrences + K_SUM (product, subtraction p - n, reg / wd terms)
K_ADAM = 12                 # ulps of the Adam update term (see test_gpu_step_fp64.py's docstring)


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
