"""float64 restatement of DCDCSR's row-wise map step (csrc/cdr_dcdcsr.hip, fused.FusedDCDCSRMapStep) on fp64_bounds.EV pairs, shared by
test_gpu_dcdcsr_rowwise.py (the kernel and the step on the device) and test_dcdcsr_rowwise_host.py (an fp32 torch-autograd result of
the oracle and three mutations of it on the CPU: the yardstick is shown to bite before it is trusted on the GPU).

For n sampled ids (repeats allowed):
    x = table[idx]   mx = max x   mn = min x   mean = (mx + mn) / 2   h = mx - mean   e = (x - mean) / h   (the same for bench -> b)
    a_0 = e   a_l = tanh(a_{l-1} W_l^T + b_l), l = 1..L   m = a_L   mse = sum (m - b)^2 / (n D)   g = 2 (m - b) / (n D)
    gpre_L = g (1 - m^2)   dW_l = gpre_l^T a_{l-1}   db_l = sum gpre_l   gpre_{l-1} = (gpre_l W_l) (1 - a_{l-1}^2)   gy = gpre_1 W_1
    G_i = gy / h - [x == mx] (Sg + Sy) / (2 h n_max) - [x == mn] (Sg - Sy) / (2 h n_min),  Sg = sum gy, Sy = sum gy e
Bounds (derived, never tuned; u = 2^-24):
  * max, min and the tie counts are exact: comparisons of inputs (as maxmin_fp64 of test_gpu_rowmodels_fp64.py); (mx + mn) / 2 is one
    rounding and an exact halving;
  * the two row contractions per layer (a W^T and gpre W) are EV.matmul with the REAL accumulation depth of the kernel (``dcdcsr_depths``:
    an MFMA chain runs over the width rounded up to 8); the bias add is matmul's second ``extra`` rounding; tanh is EV.tanh;
  * g: the fp32 coefficient 2 / (n D) (one rounding) times the difference: two roundings;
  * a row sum (Sg, Sy) is the per-lane chain over the lane's columns (four per 32 columns of width) and the three butterfly steps;
  * dW_l and db_l run over the 32 rows of a tile times the tiles a workgroup walks, plus the partials added in workgroup order (an upper
    bound of db's chain, which adds each tile's column sum to a running sum);
  * for a result whose summation order is not known (torch on the CPU) every depth is the any-order n - 1;
  * the table's update sums the occurrences' rows of a repeated id into one part and goes through fp64_bounds.apply_fp64 as every other
    row-wise step."""
import ctypes

import torch

from fp64_bounds import EV, _occ_sums, check_dense_grad, check_scalar, ev_cat, ev_where


def layer_dims(params):
    """[d_0, ..., d_L] of the packed (W1, b1, ..., WL, bL)."""
    return [int(params[0].shape[1])] + [int(params[2 * l].shape[0]) for l in range(len(params) // 2)]


def n_params(dims):
    return sum(dims[l + 1] * dims[l] + dims[l + 1] for l in range(len(dims) - 1))


def dcdcsr_grid(n, dims):
    """Workgroups of cdr_dcdcsr_map_fwd_grad for n ids: its workspace is one packed parameter vector per workgroup."""
    from recbole_cdr_amd import binding
    need = ctypes.c_size_t(0)
    rc = binding.load().cdr_dcdcsr_map_fwd_grad_workspace_bytes(n, len(dims) - 1, (ctypes.c_int * len(dims))(*dims), ctypes.byref(need))
    assert rc == 0, (n, dims, rc)
    assert need.value % (4 * n_params(dims)) == 0
    return need.value // (4 * n_params(dims))


def dcdcsr_depths(n, dims, grid):
    """Accumulation depths of csrc/cdr_dcdcsr.hip for a launch of ``grid`` workgroups."""
    k8 = lambda d: -(-d // 8) * 8
    per_wg = -(-(-(-n // 32)) // grid)                       # tiles a workgroup walks
    L = len(dims) - 1
    return dict(fwd=[k8(dims[l]) for l in range(L)], bwd=[k8(dims[l + 1]) for l in range(L)], row=4 * -(-dims[0] // 32) + 3,
                rows=32 * per_wg + grid)


def maxmin_ev(x):
    """x fp32 [n, D] -> (X, y, h, ismax, ismin): the normalised rows as EV, max / min / ties exact."""
    xd = x.double()
    X = EV(xd)
    mx, mn = EV(xd.amax(1, keepdim=True)), EV(xd.amin(1, keepdim=True))
    mean = (mx + mn).exact_scale(0.5)
    h = mx - mean
    return X, (X - mean) / h, h, xd == mx.v, xd == mn.v


def dcdcsr_map_fp64(table, bench, params, idx, depths=None):
    """``table`` / ``bench``: fp32 [rows, D]; ``params`` = [W1, b1, ..., WL, bL] fp32; ``idx`` int64 [n].  Returns a dict: 'loss' (float),
    'G' (EV [n, D]: one gradient row per occurrence), 'dP' [(EV, shape)] in the packed order, 'm' (EV [n, D])."""
    n, D = idx.numel(), table.shape[1]
    dims = layer_dims(params)
    L = len(dims) - 1
    assert dims[0] == dims[-1] == D
    d = depths or dict(fwd=[dims[l] - 1 for l in range(L)], bwd=[dims[l + 1] - 1 for l in range(L)], row=D - 1, rows=n - 1)
    X, e, h, ismax, ismin = maxmin_ev(table[idx])
    _, b, _, _, _ = maxmin_ev(bench[idx])
    acts = [e]
    for l in range(L):
        W, bias = params[2 * l].double(), params[2 * l + 1].double()
        pre = acts[-1].matmul(EV(W.t().contiguous()), d['fwd'][l])
        acts.append(EV(pre.v + bias, pre.e).tanh())
    m = acts[-1]
    diff = m - b
    loss = float((diff.v * diff.v).sum() / (n * D))
    scale = 2.0 / (n * D)
    g = EV._rnd(diff.v * scale, diff.e * scale, k=2)
    gpre = g * (1.0 - m * m)
    dP = [None] * (2 * L)
    gy = None
    for l in range(L, 0, -1):
        a_prev = acts[l - 1]
        dW = EV(gpre.v.t().contiguous(), gpre.e.t().contiguous()).matmul(a_prev, d['rows'])
        dP[2 * l - 2] = (dW, (dims[l], dims[l - 1]))
        dP[2 * l - 1] = (gpre.sum(0, depth=d['rows']), (dims[l],))
        gx = gpre.matmul(EV(params[2 * l - 2].double()), d['bwd'][l - 1], extra=1)
        if l > 1:
            gpre = gx * (1.0 - a_prev * a_prev)
        else:
            gy = gx
    Sg = gy.sum(1, depth=d['row'], keepdim=True)
    Sy = (gy * e).sum(1, depth=d['row'], keepdim=True)
    nmax, nmin = EV(ismax.double().sum(1, keepdim=True)), EV(ismin.double().sum(1, keepdim=True))
    cmax = (Sg + Sy) / (h.exact_scale(2.0) * nmax)
    cmin = (Sg - Sy) / (h.exact_scale(2.0) * nmin)
    G = gy / h
    G = ev_where(ismax, G - cmax, G)
    G = ev_where(ismin, G - cmin, G)
    return dict(loss=loss, G=G, dP=dP, m=m, ties=(ismax.sum(1), ismin.sum(1)))


def dcdcsr_packed(ref):
    """The parameter gradient as one EV vector in the packed layout of cdr_dcdcsr_map_fwd_grad's ``dparams``."""
    return ev_cat([EV(ev.v.reshape(-1), ev.e.reshape(-1)) for ev, _ in ref['dP']])


def dcdcsr_table_part(ref, idx):
    """The part of fp64_bounds.apply_fp64 / check_dense_grad: a row named several times gets the sum of its occurrences' rows."""
    rows, inv = torch.unique(idx, return_inverse=True)
    return (rows, *_occ_sums(rows.numel(), inv, ref['G'].v, ref['G'].v.abs(), ref['G'].e))


def dcdcsr_weight_parts(ref):
    """One part per parameter, as two-dimensional [rows, columns] gradients (a bias is [d, 1])."""
    out = []
    for ev, shape in ref['dP']:
        shape2 = shape if len(shape) == 2 else (shape[0], 1)
        v, e = ev.v.reshape(shape2), ev.e.reshape(shape2)
        k = shape2[0]
        out.append((torch.arange(k, device=v.device), v, v.abs(), e, torch.ones(k, device=v.device, dtype=torch.int64)))
    return out


def check_dcdcsr_result(tag, got, ref, idx):
    """An fp32 result of the map loss and its gradients against the reference.  ``got``: {'loss': float, 'table': dense gradient of the
    unit table, 'params': [gradients of W1, b1, ...]}.  Every element is compared (check_dense_grad: the sampled rows within their
    bounds, every other row +0.0).  Returns {quantity: worst error / bound}."""
    worst = {'loss': check_scalar(f'{tag}: loss', got['loss'], ref['loss'])}
    worst['table'] = check_dense_grad(f'{tag}: gradient table', got['table'], dcdcsr_table_part(ref, idx), got['table'].shape[1])
    wparts = dcdcsr_weight_parts(ref)
    assert len(wparts) == len(got['params'])
    for j, (part, gr) in enumerate(zip(wparts, got['params'])):
        name = f'{"W" if j % 2 == 0 else "b"}{j // 2 + 1}'
        gr2 = gr.reshape(part[1].shape)
        worst[name] = check_dense_grad(f'{tag}: gradient {name}', gr2, part, gr2.shape[1])
    return worst
