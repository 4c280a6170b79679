"""CoNet's C3 training step (csrc/cdr_conet.hip through functional.ConetFusedLoss, and the per-layer cdr_gemm route) and the deferred
row-wise Adam over its four tables (lazyadam.DeferredRowAdam, csrc/cdr_lazyadam.hip) against a float64 restatement in plain torch of the
reference's CoNet.calculate_loss and torch.optim.Adam, at the C3 benchmark's id space (156,096 users x 133,736 items, D = 128,
[64,32,16,8]), held to PER-ELEMENT first-order error bounds carried through the reference itself.

The reference (oracle/conet.py documents the definition): every row runs both towers, per layer s' = relu(Ws s + bs + [m] H t) and
t' = relu(Wt t + bt + [m] H s) with m = user < OU (overlap_users) or item < OI (overlap_items), PAD id 0 counting as overlapped; the
source output sigmoid(wo h + bo) on the first n_source rows, the target output on the rest; loss = the two BCE means + the UN-weighted
sum of ||H_l||_F.  The backward is written by hand.  Every case is teacher-forced: the reference starts from the device's own fp32
state read just before the step (tables, tower weights, moments, counts), so errors never pile up across steps.

Bounds (u = 2^-24, gamma_k = k u / (1 - k u); fp64_bounds: U32, gam, ulp32, apply_fp64 and its K_SUM / K_ADAM, adam_idle_fp64; the
constants below are named once and used as written):
  * layer z: gamma_{2 din + 2} (|W||x| + |b| + [m]|H||x'|) + e_x |W| + [m] e_x' |H|  (W exact: the device's own state);
    ReLU a: e_z where z > -e_z, 0 below; a unit with |z| <= e_z is AMBIGUOUS (counted and reported, never dropped);
  * output unit zo = h wo + bo: gamma_{dL + 1} (|h||wo| + |bo|) + e_h |wo|;  p = 1 / (1 + expf(-zo)): p (1 - p) e_zo + K_SIG u p;
  * the kernel's dL/dzo = ((go / n) (p - y) / max((1 - p) p, 1e-12)) (1 - p) p = (go / n)(p - y) up to its roundings:
    (go / n) e_p + K_GZ u |dzo|;  output gradient rows g = dzo wo: e_dzo |wo| + u |g|;
  * ReLU backward: e_g where z > e_z, 0 below -e_z, |g| + e_g at an ambiguous unit (both branches);
  * data backward: gamma_{2 dout + 1} (|g||W| + [m]|g'||H|) + e_g |W| + [m] e_g' |H|;
  * weight and bias gradients (sums over all R rows): gamma_{depth} A + (1 + gamma_{depth}) E with the depth of the reduction the launch
    geometry implies (_wgrad_depth: split_plan's chunks of kc rows, four per workgroup, then the finish's ngroup partials; _ou_depth:
    the output units' per-workgroup row walk, then ou_part's two-level sum; _gemm_depth: cdr_gemm's split-K) -- NOT gamma_R; the
    Frobenius term go H / ||H||_F rides in A;
  * table-row gradients: the per-occurrence rows' bounds (contraction depth of layer 0 inside) summed, plus gamma_{occ + K_SUM};
  * one optimizer step: apply_fp64; postponed updates: adam_idle_fp64 carried through the gradient-free updates last + 1 .. t.
Losses and last_loss_parts are held to LOSS_RTOL relative of the fp64 value.  Each case prints its worst error / bound per quantity."""
import gc

import numpy as np
import pytest
import torch

from fp64_bounds import K_SUM, U32, adam_idle_fp64, apply_fp64, gam
from helpers import DEV, FakeDataset, base_config

pytestmark = pytest.mark.gpu

K_SIG = 4                   # expf (within 2 ulp), the add and the division of p = 1 / (1 + expf(-z))
K_GZ = 8                    # roundings of dL/dzo: go / n, p - y, (1 - p) p, the division, the two products (and the go scale)
K_WG = 8                    # roundings of a weight gradient beyond its sum: the four waves' adds, the go scale, the Frobenius add
LOSS_RTOL = 1e-5
NUM_CU = 256                # CDR_NUM_CU (csrc/cdr_common.h)
ROWS = 32                   # kRows of csrc/cdr_conet.hip
C3 = dict(OU=5983, TOU=20986, SOU=129127, OI=1, TOI=18563, SOI=115172)
C3_ITEMS = dict(OU=1, TOU=20986, SOU=129127, OI=4001, TOI=18563, SOI=115172)
HIDDEN = [64, 32, 16, 8]
TABLE_STEP = 1000


def _cdiv(a, b):
    return -(-a // b)


def _ntiles(dims):
    """fill_tiles: (layer, pair of 64-row m tiles, 32-column n tile) jobs of conet_wgrad_kernel."""
    return sum(_cdiv(dims[l + 1], 64) * _cdiv(dims[l], 32) for l in range(len(dims) - 1))


def _wgrad_depth(R, ntiles):
    """Reduction depth of a layer's weight / bias gradient on the fused route: split_plan cuts the R rows into nsplit chunks of kc rows
    (one wave's MFMA chain each, +1 for the product); a workgroup adds its four waves' chunks; conet_wgrad_finish_kernel adds the
    ngroup = ceil(nsplit / 4) partials in order (groups of 8, then the rest)."""
    ns = 4 * max(NUM_CU // ntiles, 1)
    ns = max(1, min(ns, _cdiv(R, 64)))
    kc = (_cdiv(R, ns) + 7) & ~7
    nsplit = _cdiv(R, kc)
    return kc + 1 + 4 + _cdiv(nsplit, 4) + K_WG


def _ou_depth(R, dL):
    """Reduction depth of an output unit's gradient: each of rows_grid(R) workgroups walks its 32-row blocks in order into ou_acc; the
    finish adds the block partials b = ch, ch + nch, ... in nch strided sums and those in order."""
    nrb = _cdiv(R, ROWS)
    grid = max(1, min(nrb, 2048))
    nch = 256 // (2 * (dL + 1))
    return ROWS * _cdiv(nrb, grid) + _cdiv(grid, nch) + nch + K_WG


def _gemm_depth(R):
    """The per-layer route's weight gradients: cdr_gemm_f32 with K = R rows splits K into 256-row chunks added atomically (K >= 1024);
    its column sums (biases) and the output unit's linear backward are held to gamma_R."""
    return (256 + _cdiv(R, 256) if R >= 1024 else R) + K_WG


# ---------------------------------------------------------------------------------------------------------------------- fp64 reference

def conet_fp64(model, inter, go=1.0):
    """calculate_loss and every gradient in float64 from the model's fp32 state.  Returns a dict: 'loss', 'parts' (bce_s, bce_t, reg,
    ||H_l||...), 'params' [(G, A, E, kind)] in the order of model._fused_params() (kind: 'w' layer weight / bias, 'ou' output unit),
    'tables' [(rows, G, A, E, occ)] per table (A, E: sums over the occurrences of |row| and of the row's bound), 'amb' ambiguous units."""
    su, si, tu, ti = [t.detach().double() for t in model.table_parameters()]
    us, is_, ut, it = (inter[k].reshape(-1) for k in ('source_user_id', 'source_item_id', 'target_user_id', 'target_item_id'))
    y = torch.cat([inter['source_label'].reshape(-1), inter['target_label'].reshape(-1)]).double()
    ns, R = us.numel(), us.numel() + ut.numel()
    user, item = torch.cat([us, ut]), torch.cat([is_, it])
    m = ((user < model.overlapped_num_users) if model.mode == 'overlap_users' else (item < model.overlapped_num_items)).double()[:, None]
    ps = [p.detach().double() for p in model._fused_params()]
    L = len(model.crossparas)
    xs, xt = torch.cat([su[user], si[item]], 1), torch.cat([tu[user], ti[item]], 1)
    exs, ext = torch.zeros_like(xs), torch.zeros_like(xt)
    saved, amb = [], 0
    for l in range(L):
        Ws, bs, Wt, bt, H = ps[5 * l:5 * l + 5]
        Wsa, Wta, Ha = Ws.abs(), Wt.abs(), H.abs()
        g_ = gam(2 * Ws.shape[1] + 2)
        zs = xs @ Ws.T + bs + m * (xt @ H.T)
        ezs = g_ * (xs.abs() @ Wsa.T + bs.abs() + m * (xt.abs() @ Ha.T)) + exs @ Wsa.T + m * (ext @ Ha.T)
        zt = xt @ Wt.T + bt + m * (xs @ H.T)
        ezt = g_ * (xt.abs() @ Wta.T + bt.abs() + m * (xs.abs() @ Ha.T)) + ext @ Wta.T + m * (exs @ Ha.T)
        amb += int((zs.abs() <= ezs).sum()) + int((zt.abs() <= ezt).sum())
        saved.append((xs, exs, xt, ext, zs, ezs, zt, ezt))
        xs, exs = zs.clamp(min=0), ezs * (zs > -ezs)
        xt, ext = zt.clamp(min=0), ezt * (zt > -ezt)
    wo_s, bo_s, wo_t, bo_t = ps[5 * L:]
    src = torch.arange(R, device=xs.device) < ns
    h = torch.where(src[:, None], xs, xt)
    eh = torch.where(src[:, None], exs, ext)
    wo = torch.where(src[:, None], wo_s.reshape(1, -1), wo_t.reshape(1, -1))
    bo = torch.where(src, bo_s, bo_t)
    zo = (h * wo).sum(1) + bo
    ezo = gam(h.shape[1] + 1) * ((h.abs() * wo.abs()).sum(1) + bo.abs()) + (eh * wo.abs()).sum(1)
    p = torch.sigmoid(zo)
    ep = p * (1 - p) * ezo + K_SIG * U32 * p
    bce = -(y * torch.log(p) + (1 - y) * torch.log1p(-p))
    norms = [float(torch.linalg.vector_norm(ps[5 * l + 4])) for l in range(L)]
    parts = [float(bce[:ns].mean()), float(bce[ns:].mean()), sum(norms)] + norms
    nd = torch.where(src, float(ns), float(R - ns)).double()
    dz = go / nd * (p - y)
    edz = go / nd * ep + K_GZ * U32 * dz.abs()
    pg = [None] * len(ps)
    for o, (wo_, bo_, sel) in enumerate(((wo_s, bo_s, src), (wo_t, bo_t, ~src))):
        d, e, hh = dz[sel], edz[sel], h[sel]
        pg[5 * L + 2 * o] = ((d[:, None] * hh).sum(0).reshape(wo_.shape), (d.abs()[:, None] * hh.abs()).sum(0).reshape(wo_.shape),
                             (e[:, None] * hh.abs() + d.abs()[:, None] * eh[sel]).sum(0).reshape(wo_.shape), 'ou')
        pg[5 * L + 2 * o + 1] = (d.sum().reshape(1), d.abs().sum().reshape(1), e.sum().reshape(1), 'ou')
    gsv = torch.where(src[:, None], dz[:, None] * wo_s.reshape(1, -1), torch.zeros_like(h))
    gtv = torch.where(~src[:, None], dz[:, None] * wo_t.reshape(1, -1), torch.zeros_like(h))
    egs = torch.where(src[:, None], edz[:, None] * wo_s.abs().reshape(1, -1), torch.zeros_like(h)) + U32 * gsv.abs()
    egt = torch.where(~src[:, None], edz[:, None] * wo_t.abs().reshape(1, -1), torch.zeros_like(h)) + U32 * gtv.abs()
    del h, eh, wo
    for l in range(L - 1, -1, -1):
        Ws, bs, Wt, bt, H = ps[5 * l:5 * l + 5]
        xs, exs, xt, ext, zs, ezs, zt, ezt = saved[l]

        def relu_bwd(g, eg, z, ez):
            a = z.abs() <= ez
            return g * (z > 0), torch.where(a, g.abs() + eg, eg * (z > 0))
        gzs, egzs = relu_bwd(gsv, egs, zs, ezs)
        gzt, egzt = relu_bwd(gtv, egt, zt, ezt)
        fro = (go / norms[l]) * H
        pg[5 * l] = (gzs.T @ xs, gzs.abs().T @ xs.abs(), egzs.T @ xs.abs() + gzs.abs().T @ exs, 'w')
        pg[5 * l + 1] = (gzs.sum(0), gzs.abs().sum(0), egzs.sum(0), 'w')
        pg[5 * l + 2] = (gzt.T @ xt, gzt.abs().T @ xt.abs(), egzt.T @ xt.abs() + gzt.abs().T @ ext, 'w')
        pg[5 * l + 3] = (gzt.sum(0), gzt.abs().sum(0), egzt.sum(0), 'w')
        mgs, mgt, megs, megt = m * gzs, m * gzt, m * egzs, m * egzt
        pg[5 * l + 4] = (mgs.T @ xt + mgt.T @ xs + fro, mgs.abs().T @ xt.abs() + mgt.abs().T @ xs.abs() + fro.abs(),
                         megs.T @ xt.abs() + mgs.abs().T @ ext + megt.T @ xs.abs() + mgt.abs().T @ exs, 'w')
        Wsa, Wta, Ha = Ws.abs(), Wt.abs(), H.abs()
        g_ = gam(2 * Ws.shape[0] + 1)
        gsv = gzs @ Ws + mgt @ H
        egs = g_ * (gzs.abs() @ Wsa + mgt.abs() @ Ha) + egzs @ Wsa + megt @ Ha
        gtv = gzt @ Wt + mgs @ H
        egt = g_ * (gzt.abs() @ Wta + mgs.abs() @ Ha) + egzt @ Wta + megs @ Ha
    D = su.shape[1]
    tables = []
    for k, (g, eg, ids) in enumerate(((gsv[:, :D], egs[:, :D], user), (gsv[:, D:], egs[:, D:], item), (gtv[:, :D], egt[:, :D], user),
                                      (gtv[:, D:], egt[:, D:], item))):
        rows, inv = torch.unique(ids, return_inverse=True)
        G = torch.zeros(rows.numel(), D, device=g.device, dtype=torch.float64)
        A, E = torch.zeros_like(G), torch.zeros_like(G)
        G.index_add_(0, inv, g); A.index_add_(0, inv, g.abs()); E.index_add_(0, inv, eg)
        tables.append((rows, G, A, E, torch.bincount(inv, minlength=rows.numel())))
    loss = parts[0] + parts[1] + parts[2]
    return {'loss': loss, 'parts': parts, 'params': pg, 'tables': tables, 'amb': amb, 'R': R}


def _param_bound(G, A, E, depth):
    g_ = gam(depth)
    return g_ * A + (1 + g_) * E


def _table_bound(A, E, occ):
    g_ = gam(occ.double() + K_SUM).unsqueeze(1)
    return g_ * A + (1 + g_) * E


def _depths(model, R, fused):
    dims = model._dims
    if fused:
        wd, ou = _wgrad_depth(R, _ntiles(dims)), _ou_depth(R, dims[-1])
    else:
        wd, ou = _gemm_depth(R), R + K_WG
    out = []
    for l in range(len(dims) - 1):
        b = wd if fused else R + K_WG
        out += [wd, b, wd, b, wd + 1]
    return out + [ou] * 4


# ---------------------------------------------------------------------------------------------------------------------- checks

def _ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    return torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))


def _check(tag, got, ref, bound, worst, name):
    got = got.double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f'{tag} {name}: non-finite values'
    r = _ratio(got, ref, bound)
    w = float(r.max()) if r.numel() else 0.0
    worst[name] = max(worst.get(name, 0.0), w)
    if w > 1.0:
        j = int(r.reshape(-1).argmax())
        g_, f_, b_ = (float(x.reshape(-1)[j]) for x in (got, ref, bound))
        raise AssertionError(f'{tag} {name}: error / bound = {w:.3g} at flat index {j} (shape {tuple(r.shape)}): got {g_!r} want {f_!r} '
                             f'bound {b_:.3g}')


def _fmt(worst):
    return ' '.join(f'{k}={v:.3g}' for k, v in worst.items())


# ---------------------------------------------------------------------------------------------------------------------- models and batches

_CACHE = {}


@pytest.fixture(scope='module', autouse=True)
def _release_device_memory():
    """C3-sized tables, their fp64 restatements and the optimizers' moments take a few GB through torch's caching allocator: all of it
    goes back to the device when the module ends."""
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f'\nconet fp64 module: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB')
    _CACHE.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _ids(ids):
    from oracle.common import IdSpace
    return IdSpace(**ids)


def _model(ids=C3, D=128, hidden=HIDDEN, fused=True, seed=3):
    """CoNet with tables ~ N(0, 0.5^2) (pre-activations of order one) and biases ~ N(0, 0.1^2) (xavier leaves them at zero)."""
    from recbole_cdr_amd.model.cross_domain_recommender.conet import CoNet
    torch.manual_seed(seed)
    cfg = base_config(DEV, embedding_size=D, reg_weight=0.01, mlp_hidden_size=list(hidden), conet_fused=fused)
    model = CoNet(cfg, FakeDataset(_ids(ids))).to(DEV)
    assert model.fused_towers == fused
    gen = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if 'embedding' in n:
                p.normal_(0, 0.5, generator=gen)
            elif n.endswith('bias'):
                p.normal_(0, 0.1, generator=gen)
    return model


def _pools(ids, exclude_u=None, exclude_i=None):
    I = _ids(ids)
    U, It = I.total_num_users, I.total_num_items
    pools = {'su': np.r_[np.arange(0, I.OU), np.arange(I.OU + I.TOU, U)], 'si': np.r_[np.arange(0, I.OI), np.arange(I.OI + I.TOI, It)],
             'tu': np.arange(0, I.OU + I.TOU), 'ti': np.arange(0, I.OI + I.TOI)}
    for k in pools:
        ex = exclude_u if k.endswith('u') else exclude_i
        if ex is not None:
            pools[k] = np.setdiff1d(pools[k], ex)
    return pools


def _inter(su, si, sy, tu, ti, ty):
    t = lambda x, dt=torch.int64: torch.from_numpy(np.asarray(x)).to(dt).to(DEV)
    return {'source_user_id': t(su), 'source_item_id': t(si), 'source_label': t(sy, torch.float32),
            'target_user_id': t(tu), 'target_item_id': t(ti), 'target_label': t(ty, torch.float32)}


def _pointwise(rs, pools, S=819, k=4, pad=True):
    """SyntheticCrossDomainDataset.pointwise_batch's layout in both domains: S users repeated 1 + k times, positives then k-major
    negatives, labels [1] * S + [0] * S k; with ``pad``, PAD id 0 (overlapped by convention) as a user and an item of a few rows."""
    out = []
    for d in ('s', 't'):
        u = np.tile(rs.choice(pools[d + 'u'], S), 1 + k)
        i = rs.choice(pools[d + 'i'], S * (1 + k))
        if pad:
            u[3] = u[3 + S] = 0
            i[5] = 0
        out += [u, i, np.r_[np.ones(S), np.zeros(S * k)]]
    return _inter(*out)


def _random_rows(rs, pools, n_s, n_t):
    out = []
    for d, n in (('s', n_s), ('t', n_t)):
        out += [rs.choice(pools[d + 'u'], n), rs.choice(pools[d + 'i'], n), (rs.rand(n) < 0.3).astype(np.float32)]
    return _inter(*out)


# ---------------------------------------------------------------------------------------------------------------------- 2. loss and gradients

def _grad_case(tag, model, inter, fused=True, go=1.0):
    """One differentiated forward without a row optimizer (dense table gradients from the sorted scatter) against conet_fp64."""
    model.zero_grad(set_to_none=True)
    ref = conet_fp64(model, inter, go)
    loss = model.calculate_loss(inter)
    (loss * go if go != 1.0 else loss).backward()
    torch.cuda.synchronize()
    worst = {}
    got = float(loss.detach())
    assert abs(got - ref['loss']) <= LOSS_RTOL * abs(ref['loss']), (tag, got, ref['loss'])
    worst['loss'] = abs(got - ref['loss']) / (LOSS_RTOL * abs(ref['loss']))
    if fused:
        parts = model.last_loss_parts.double().cpu()
        want = ref['parts']
        for j, w in enumerate(want):
            assert abs(float(parts[1 + j]) - w) <= LOSS_RTOL * abs(w), (tag, 'loss part', j, float(parts[1 + j]), w)
            worst['parts'] = max(worst.get('parts', 0.0), abs(float(parts[1 + j]) - w) / (LOSS_RTOL * abs(w)))
    depths = _depths(model, ref['R'], fused)
    names = ['Ws', 'bs', 'Wt', 'bt', 'H']
    for j, (p, (G, A, E, kind), dep) in enumerate(zip(model._fused_params(), ref['params'], depths)):
        name = names[j % 5] if kind == 'w' else 'out'
        _check(tag, p.grad, G, _param_bound(G, A, E, dep), worst, name)
    for k, (p, (rows, G, A, E, occ)) in enumerate(zip(model.table_parameters(), ref['tables'])):
        g = p.grad
        _check(tag, g[rows], G, _table_bound(A, E, occ), worst, 'table')
        mask = torch.ones(g.shape[0], dtype=torch.bool, device=g.device)
        mask[rows] = False
        assert not bool(g[mask].any()), (tag, 'gradient outside the batch rows', k)
    print(f'\n{tag}: R={ref["R"]} ambiguous ReLU units={ref["amb"]} worst error/bound: {_fmt(worst)}')
    return worst


def _c3_batch(ids=C3, seed=7):
    return _pointwise(np.random.RandomState(seed), _pools(ids))


@pytest.mark.parametrize('env', [{}, {'CDR_CONET_FB_WAVES': '4'}, {'CDR_CONET_TWO_LAUNCH': '1'}, {'CDR_CONET_NO_DMA_TABLE': '1'}],
                         ids=['fb8', 'fb4', 'two_launch', 'no_dma_table'])
def test_c3_step_gradients_vs_fp64(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if 'c3' not in _CACHE:
        _CACHE.clear()
        _CACHE['c3'] = _model()
    _grad_case('c3 ' + (' '.join(env) or 'default'), _CACHE['c3'], _c3_batch())


def test_c3_gemm_route_vs_fp64():
    model = _model(fused=False)
    _grad_case('c3 conet_fused=False', model, _c3_batch(), fused=False)


def test_c3_upstream_gradient_other_than_one_vs_fp64():
    if 'c3' not in _CACHE:
        _CACHE.clear()
        _CACHE['c3'] = _model()
    _grad_case('c3 (2.5 * loss).backward()', _CACHE['c3'], _c3_batch(seed=8), go=2.5)


@pytest.mark.parametrize('n_s,n_t', [(1, 1), (3, 8187), (35000, 35001), (16380, 16380)], ids=['1+1', '3+8187', '70001', '4xC3'])
def test_c3_ragged_and_large_batches_vs_fp64(n_s, n_t):
    if 'c3' not in _CACHE:
        _CACHE.clear()
        _CACHE['c3'] = _model()
    rs = np.random.RandomState(n_s + n_t)
    if n_s == 16380:
        # (no row optimizer here: the deferred Adam's radix-sort route for id lists over 16,384 entries is reached by
        # test_c3_one_optimizer_step_every_row_vs_fp64[RowAwareAdam-default], whose batch has the same 32,760 rows)
        inter = _pointwise(rs, _pools(C3), S=3276)
    else:
        inter = _random_rows(rs, _pools(C3), n_s, n_t)
    _grad_case(f'c3 rows {n_s}+{n_t}', _CACHE['c3'], inter)


def test_c3_overlap_items_mode_vs_fp64():
    model = _model(ids=C3_ITEMS)
    assert model.mode == 'overlap_items'
    _grad_case('c3 overlap_items', model, _c3_batch(ids=C3_ITEMS, seed=9))


@pytest.mark.parametrize('D,hidden', [(64, [64, 32, 16, 8]), (40, [12, 8, 4]), (128, [32, 32, 16, 8]), (128, [64, 16, 8])],
                         ids=['D64', 'D40-12-8-4', 'D128-32-32-16-8', 'D128-64-16-8'])
def test_c3_layer_shapes_vs_fp64(D, hidden):
    _CACHE.clear()
    model = _model(D=D, hidden=hidden)
    _grad_case(f'c3 D={D} {hidden}', model, _c3_batch(seed=D + len(hidden)))


def test_c3_hot_user_long_duplicate_segments_vs_fp64():
    """One overlapped user in 1,000 rows of each domain: 2,000 occurrences in one sorted segment of each user table."""
    if 'c3' not in _CACHE:
        _CACHE.clear()
        _CACHE['c3'] = _model()
    inter = _c3_batch(seed=10)
    rs = np.random.RandomState(10)
    for d in ('source', 'target'):
        u = inter[f'{d}_user_id']
        u[torch.from_numpy(rs.choice(u.numel(), 1000, replace=False)).to(DEV)] = 4242
    _grad_case('c3 hot user', _CACHE['c3'], inter)


# ---------------------------------------------------------------------------------------------------------------------- 3. one optimizer step

OPTS = {'default': (1e-3, (0.9, 0.999), 1e-8, 0.0), 'wd': (1e-3, (0.9, 0.999), 1e-8, 1e-2), 'betas': (1e-3, (0.8, 0.99), 1e-6, 1e-2)}


def _adam_checkpoint(model, lr, betas, eps, wd, gen, quiet_rows=None):
    """A torch.optim.Adam checkpoint of every parameter: the tables at update TABLE_STEP, each tower parameter at a count of its own, all
    with nonzero moments -- except ``quiet_rows`` of every table, whose moments are zero."""
    adam = torch.optim.Adam(model.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=wd)
    tabs = {id(t) for t in model.table_parameters()}
    for j, p in enumerate(model.parameters()):
        st = adam.state[p]
        st['step'] = torch.tensor(float(TABLE_STEP if id(p) in tabs else 5 + 37 * j))
        st['exp_avg'] = torch.randn(p.shape, device=DEV, generator=gen) * 1e-2
        st['exp_avg_sq'] = st['exp_avg'] ** 2 * (0.25 + torch.rand(p.shape, device=DEV, generator=gen)) + 1e-8
        if id(p) in tabs and quiet_rows is not None:
            st['exp_avg'][quiet_rows] = 0
            st['exp_avg_sq'][quiet_rows] = 0
    return adam.state_dict()


def _full_part(rows_all, part, D):
    rows, G, A, E, occ = part
    Gf = torch.zeros(rows_all, D, device=DEV, dtype=torch.float64)
    Af, Ef = torch.zeros_like(Gf), torch.zeros_like(Gf)
    of = torch.zeros(rows_all, device=DEV, dtype=torch.int64)
    Gf[rows], Af[rows], Ef[rows], of[rows] = G, A, E, occ
    return torch.arange(rows_all, device=DEV), Gf, Af, Ef, of


@pytest.mark.parametrize('opt', list(OPTS))
@pytest.mark.parametrize('deferred', [True, False], ids=['RowAwareAdam', 'DenseAdam'])
def test_c3_one_optimizer_step_every_row_vs_fp64(deferred, opt):
    from recbole_cdr_amd.trainer.trainer import DenseAdam, RowAwareAdam
    lr, betas, eps, wd = OPTS[opt]
    _CACHE.clear()
    model = _model(seed=21)
    # RowAwareAdam-default takes 4 x C3 rows: id lists of 32,760 entries, the deferred Adam's radix-sort route (the only test that reaches it)
    inter = _pointwise(np.random.RandomState(22), _pools(C3), S=3276 if (deferred and opt == 'default') else 819)
    users = torch.unique(torch.cat([inter['source_user_id'], inter['target_user_id']]))
    gen = torch.Generator(device=DEV).manual_seed(23)
    U = model.source_user_embedding.weight.shape[0]
    outside = torch.ones(U, dtype=torch.bool, device=DEV)
    outside[users] = False
    quiet = torch.nonzero(outside).reshape(-1)[torch.randperm(int(outside.sum()), device=DEV, generator=gen)[:64]]
    items = model.source_item_embedding.weight.shape[0]
    quiet = quiet[quiet < min(U, items)]
    items_in = torch.unique(torch.cat([inter['source_item_id'], inter['target_item_id']]))
    quiet = quiet[~torch.isin(quiet, items_in)]
    sd = _adam_checkpoint(model, lr, betas, eps, wd, gen, quiet)
    optim = RowAwareAdam(model, lr=lr, betas=betas, eps=eps, weight_decay=wd) if deferred else DenseAdam(model.parameters(), lr=lr, betas=betas,
                                                                                                           eps=eps, weight_decay=wd)
    optim.load_state_dict(sd)
    tabs = model.table_parameters()
    if deferred:
        ro = model.row_opt
        mv = lambda k: (ro.exp_avg[k], ro.exp_avg_sq[k])
    else:
        mv = lambda k: (optim.state[tabs[k]]['exp_avg'], optim.state[tabs[k]]['exp_avg_sq'])
    before = [{'w': t.detach().clone(), 'm': mv(k)[0].clone(), 'v': mv(k)[1].clone()} for k, t in enumerate(tabs)]
    fps = model._fused_params()
    pbefore = [{'w': p.detach().clone().reshape(-1, p.shape[-1]), 'm': optim.state[p]['exp_avg'].clone().reshape(-1, p.shape[-1]),
                'v': optim.state[p]['exp_avg_sq'].clone().reshape(-1, p.shape[-1]), 't': int(optim.state[p]['step'])} for p in fps]
    ref = conet_fp64(model, inter)
    optim.zero_grad(set_to_none=True)
    loss = model.calculate_loss(inter)
    loss.backward()
    optim.step()
    if deferred:
        assert int(ro.counters[0]) == TABLE_STEP + 1 and ro.step_count == TABLE_STEP + 1
        for k, (rows, *_rest) in enumerate(ref['tables']):
            assert bool((ro.last[k][rows] == TABLE_STEP + 1).all()), k
        model.sync_tables()
        for k in range(4):
            assert bool((ro.last[k] == TABLE_STEP + 1).all()), k
    else:
        for t in tabs:
            assert int(optim.state[t]['step']) == TABLE_STEP + 1
    torch.cuda.synchronize()
    tag = f'one step {"RowAwareAdam" if deferred else "DenseAdam"} {opt} R={ref["R"]}'
    assert abs(float(loss.detach()) - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
    worst = {}
    D = model.latent_dim
    for k, t in enumerate(tabs):
        part = _full_part(t.shape[0], ref['tables'][k], D)
        want = apply_fp64(before[k], part, 0, 'adam', lr, wd, TABLE_STEP + 1, betas[0], betas[1], eps)
        m, v = mv(k)
        for name, got in (('w', t.detach()), ('m', m), ('v', v)):
            _check(tag, got, want[name][0], want[name][1], worst, 'table_' + name)
        for name, got in (('w', t.detach()), ('m', m), ('v', v)):
            same = torch.equal(got[quiet], before[k][name][quiet])
            assert same == (wd == 0.0), (tag, k, name, 'zero-moment rows outside the batch: fixed under wd = 0, moving otherwise')
    depths = _depths(model, ref['R'], True)
    for p, st, (G, A, E, _), dep in zip(fps, pbefore, ref['params'], depths):
        shp = st['w'].shape
        part = (torch.arange(shp[0], device=DEV), G.reshape(shp), A.reshape(shp), E.reshape(shp), torch.zeros(shp[0], device=DEV, dtype=torch.int64))
        want = apply_fp64(st, part, dep, 'adam', lr, wd, st['t'] + 1, betas[0], betas[1], eps)
        for name, got in (('w', p.detach()), ('m', optim.state[p]['exp_avg']), ('v', optim.state[p]['exp_avg_sq'])):
            _check(tag, got.reshape(shp), want[name][0], want[name][1], worst, 'tower_' + name)
        assert int(optim.state[p]['step']) == st['t'] + 1
    print(f'\n{tag}: ambiguous ReLU units={ref["amb"]} worst error/bound: {_fmt(worst)}')


# ---------------------------------------------------------------------------------------------------------------------- 4. postponed updates

VARIANTS = {                # (environment, DeferredRowAdam capacity or None, start from update 0, optimizer settings)
    'window': ({}, None, False, OPTS['default']),
    'window16': ({'CDR_LZ_SWEEP': '16'}, None, False, OPTS['default']),     # wraps three times between flushes: the lag bound is live
    'no_window': ({'CDR_LZ_SWEEP': '0'}, None, False, OPTS['default']),
    'sorted_prepare': ({'CDR_LZ_CLAIM': '0'}, None, False, OPTS['wd']),
    'ring64': ({}, 64, False, OPTS['betas']),
    'from_zero': ({}, None, True, OPTS['default']),
}
# (from update 0 with weight decay, every row without a gradient is driven by wd w alone and marches to 0 at ~lr per update; near 0 the
# update term's sensitivity to w is ~lr (1 - b1) / |w| and a first-order bound carried through hundreds of updates diverges.  The
# checkpointed variants keep weight decay, their moments being far from that regime.)


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_c3_postponed_updates_vs_fp64_chain(monkeypatch, variant):
    """300 eager C3 steps through RowAwareAdam.  A test-side fp64 mirror of every table row is carried through the gradient-free
    recurrence of every update (adam_idle_fp64) and reset to the device's own (w, m, v) of the batch's rows right after each step.
    Before every step the rows prepare_batch has just brought up are held to it; every 50 steps and at the end a flush() brings up
    every row -- the witness rows that never see a batch among them -- and all of them are held to it.
    A replay is exact whoever runs it, so the moving window shows only in last[]: after every step the window's chunk of each table must
    have been brought up, and no row may be more than the period + 1 updates behind.  At period 256 the 50-step flushes keep every row far
    inside that bound; 'window16' (period 16, three wraps between flushes) is where the lag bound itself is what holds."""
    from recbole_cdr_amd.lazyadam import DeferredRowAdam
    from recbole_cdr_amd.trainer.trainer import RowAwareAdam
    env, capacity, from_zero, (lr, betas, eps, wd) = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _CACHE.clear()
    steps = 300
    model = _model(seed=31)
    optim = RowAwareAdam(model, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    if capacity is not None:
        optim.row_opt = model.row_opt = DeferredRowAdam(model.table_parameters(), [0, 1, 0, 1], lr=lr, betas=betas, eps=eps,
                                                          weight_decay=wd, capacity=capacity)
    if not from_zero:
        optim.load_state_dict(_adam_checkpoint(model, lr, betas, eps, wd, torch.Generator(device=DEV).manual_seed(32)))
    ro = model.row_opt
    tabs = model.table_parameters()
    I = _ids(C3)
    rs = np.random.RandomState(33)
    wu = np.unique(np.r_[0, I.total_num_users - 1, I.OU - 1, I.OU, rs.choice(I.total_num_users, 300)])
    wi = np.unique(np.r_[0, I.total_num_items - 1, I.OI + I.TOI - 1, rs.choice(I.total_num_items, 300)])
    pools = _pools(C3, wu, wi)
    period = ro._sweep_period()
    window = period > 0 and env.get('CDR_LZ_CLAIM') != '0'       # (the sorted prepare has no window)
    worst_lag = 0
    ref = [{'w': t.detach().double(), 'm': ro.exp_avg[k].double(), 'v': ro.exp_avg_sq[k].double()} for k, t in enumerate(tabs)]
    err = [{n: torch.zeros_like(x) for n, x in r.items()} for r in ref]
    n = ro.step_count
    worst = {}
    tag = f'postponed {variant}'

    def check_rows(k, rows, what):
        for name, got in (('w', tabs[k].detach()), ('m', ro.exp_avg[k]), ('v', ro.exp_avg_sq[k])):
            sel = slice(None) if rows is None else rows
            _check(f'{tag} update {n}', got[sel], ref[k][name][sel], err[k][name][sel], worst, f'{what}_{name}')

    for s in range(steps):
        inter = _pointwise(rs, pools, pad=False)
        lists = [torch.unique(torch.cat([inter['source_user_id'], inter['target_user_id']])),
                 torch.unique(torch.cat([inter['source_item_id'], inter['target_item_id']]))]
        model.prepare_batch(inter)
        for k in range(4):
            check_rows(k, lists[ro.table_list[k]], 'replayed')
        optim.zero_grad(set_to_none=True)
        model.calculate_loss(inter).backward()
        optim.step()
        n += 1
        assert ro.step_count == n
        for k in range(4):
            ref[k], err[k] = adam_idle_fp64(ref[k], err[k], n, lr, wd, betas[0], betas[1], eps)
            rows = lists[ro.table_list[k]]
            assert bool((ro.last[k][rows] == n).all()), (tag, k)
            for name, got in (('w', tabs[k].detach()), ('m', ro.exp_avg[k]), ('v', ro.exp_avg_sq[k])):
                ref[k][name][rows] = got[rows].double()
                err[k][name][rows] = 0
            if window:
                # the window of update n (lz_prepare2_kernel: chunk (n - 1) % period of ceil(rows / period) rows) was brought to n - 1
                chunk = _cdiv(tabs[k].shape[0], period)
                c0 = ((n - 1) % period) * chunk
                assert bool((ro.last[k][c0:c0 + chunk] >= n - 1).all()), (tag, k, 'window chunk', (n - 1) % period)
                lag = int((n - ro.last[k]).max())
                worst_lag = max(worst_lag, lag)
                assert lag <= period + 1, (tag, k, lag, period)
        if (s + 1) % 50 == 0 or s + 1 == steps:
            ro.flush()
            for k in range(4):
                assert bool((ro.last[k] == n).all()), (tag, k)
                check_rows(k, None, 'flushed')
    if variant == 'window16':
        # between two flushes (50 updates) rows fall behind until the window reaches them: the lag bound above is what held them
        assert period - 1 <= worst_lag <= period + 1 < 50 // 2, (tag, worst_lag, period)
    print(f'\n{tag}: {steps} steps to update {n}, window period {period if window else 0}, worst lag {worst_lag}, ring {ro.capacity}: '
          f'worst error/bound: {_fmt(worst)}')
