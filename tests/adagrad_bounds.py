"""float64 references and per-element fp32 error bounds of the Adagrad update (torch.optim.Adagrad: lr_decay = 0, eps = 1e-10), derived
the way test_gpu_step_fp64.py's docstring derives Adam's, on the parts fp64_bounds.bpr_grads_fp64 / point_grads_fp64 return.

With u = 2^-24, the summed row gradient G and its bound e_g = fp64_bounds._grad_bound (weight decay folded in as a further term):
  * sum      s = s0 + G G:   e_s = 2 |G| e_g + e_g^2  (the gradient error through the square)  + 2 u (s0 + G G)  (the product's and the
    addition's roundings)  + ulp(s);
  * weights  w = w0 - T,  T = lr G / (sqrt(s) + eps):  T is evaluated at the corners of the intervals [G - e_g, G + e_g] x
    [max(s - e_s, 0), s + e_s] -- NOT linearised: at a row's first touch s = G^2, the quotient G / (|G| + eps) is a step function of G at
    the scale of eps and an element with |G| of the order of e_g may come out with either sign.  Two facts close the interval there:
    s >= G G holds for the fp64 values and, because fp32 addition of a non-negative s0 is monotone, for the device's values too, so both
    update terms are at most lr (1 + 4 u) in magnitude; hence |T_dev - T| <= 2 lr (1 + 4 u) whatever the corners say (LR_CAP).
    On top: K_ADAGRAD u of the term (IEEE sqrtf, the addition of eps, the division and the product with lr: four roundings of at most
    u each, 4 u to first order; 6 leaves room for their second-order products and for the sqrt's error carried through the quotient),
    and ulp(w) for the final subtraction."""
import torch

from fp64_bounds import U32, _grad_bound, f32, ulp32

K_ADAGRAD = 6               # ulps (units of u) of the Adagrad update term beyond its input intervals: see the docstring
ADAGRAD_EPS = 1e-10         # torch.optim.Adagrad's default


def adagrad_term_bound(G, eg, s, es, lr, eps):
    """(T, e_T): the update term in float64 and its bound over the input intervals."""
    T = lr * G / (s.sqrt() + eps)
    den_lo = (s - es).clamp(min=0).sqrt() + eps
    den_hi = (s + es).sqrt() + eps
    cands = [lr * (G + sg * eg) / d for sg in (-1.0, 1.0) for d in (den_lo, den_hi)]
    hi = torch.stack(cands).max(0).values
    lo = torch.stack(cands).min(0).values
    spread = torch.maximum(hi - T, T - lo)
    cap = torch.full_like(T, 2.0 * lr * (1.0 + 4 * U32))                    # LR_CAP: both terms are at most lr (1 + 4 u) in magnitude
    mag = torch.maximum(hi.abs(), lo.abs()).clamp(max=lr * (1.0 + 4 * U32))
    return T, torch.minimum(spread, cap) + K_ADAGRAD * U32 * mag


def apply_adagrad_fp64(state, part, D, lr, wd, eps=ADAGRAD_EPS):
    """One row-wise Adagrad update in float64 of the part's rows from the device state BEFORE the step ({'w': table, 'v': sum});
    returns {name: (ref, bound)} for the rows' weights 'w' and sums 'v'."""
    rows, G, A, E, occ = part
    lr, wd, eps = f32(lr), f32(wd), f32(eps)
    w = state['w'][rows].double()
    if wd:
        G = G + wd * w
        A = A + wd * w.abs()
    eg = _grad_bound(D, G, A, E, occ)
    s0 = state['v'][rows].double()
    s = s0 + G * G
    es = 2 * G.abs() * eg + eg * eg + 2 * U32 * (s0 + G * G) + ulp32(s)
    T, eT = adagrad_term_bound(G, eg, s, es, lr, eps)
    wn = w - T
    return {'w': (wn, eT + ulp32(wn)), 'v': (s, es)}
