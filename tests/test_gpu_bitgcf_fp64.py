"""BiTGCF (model/cross_domain_recommender/bitgcf.py, csrc/cdr_graph.hip) against a float64 restatement of the reference's forward and
calculate_loss (recbole_cdr bitgcf.py:92-250) in plain torch, at the C4 benchmark's graph sizes, held to PER-ELEMENT error bounds
carried through the reference itself instead of a blanket atol.

Inputs are the kernel's own: the model's CSR values (fp32, proven bit-equal to the reference's normalised adjacency) and degree
counts promoted to fp64, the device's fp32 tables, and under dropout the device's own masks (cdr_dropout_dev on ones, same seed,
salt 2 l + k).  Forward and backward are written out by hand so that every quantity x carries a first-order bound e_x of
|fp32 kernel - fp64 reference|.  u = 2^-24, gamma_k = k u / (1 - k u); every constant below is named once:
  * SpMM row r of A X (A >= 0):  gamma_{len_r} (A|X|)_r + (A e_X)_r.  Rows longer than LONG_ROW use the running-sum bound of the
    kernel's sequential sum in CSR order instead, (1 + gamma_{len_r}) u sum_k (|s_k| + |a_k x_k|) with s_k the fp64 partial sums --
    gamma_{len} of a 20,000-term row is too loose to see one missing term;
  * graph layer new = E + (side + E side): e_E |1 + side| + e_side |1 + E| + gamma_{K_LAYER} (|E| + |side| + |E side|);
    dropout m new (m exact): m e + u |m new|;
  * transfer on the overlapped rows, So = c_ss s + c_st t (c = (lam + d / (d_s + d_t + 1e-7)) / 2): the coefficients times the
    input bounds + gamma_{K_MIX} of the same sum of absolute terms;
  * normalise y = x / ||x||: e_||x|| = gamma_{D + K_NORM} ||x|| + ||e_x||_2, e_y = (e_x + |y| e_||x||) / ||x|| + u |y|;
    mean of nb blocks: sum e / nb + gamma_{nb} sum |b| / nb;
  * score of a batch row over W = (L + 1) D (concat) or D: gamma_W sum|a b| + sum(|a| e_b + e_a |b|); BCE coefficient
    c = (sigmoid(x) - y) / B: s (1 - s) e_x / B + K_COEF u (|c| + s / B);
  * backward: the same rules in reverse -- normalise (K_NORM_BWD roundings), the transfer's transpose, the mask, g (.) (1 + E) with
    gamma_2, the SpMM rule on it, the epilogue g (.) (1 + side) + A tmp with gamma_{K_LAYER}; every scatter of repeated batch ids
    (the stack gradient, the EmbLoss rows) with gamma_{occ + K_SUM} of the summed |terms| (fp64_bounds.K_SUM); the EmbLoss
    coefficient reg / (B ||X||) relative gamma_{D + K_EMB}.
The losses are held to LOSS_RTOL relative.  Where the reference's magnitude is exactly zero (rows beyond L hops of the batch, the
dropped elements) the bound is zero, so a stray write fails.  Each case prints its worst error / bound per quantity."""
import gc

import numpy as np
import pytest
import torch

from fp64_bounds import K_SUM, U32, apply_fp64, f32, gam
from helpers import DEV, FakeDataset, base_config, collect_ranks, load_params

pytestmark = pytest.mark.gpu

LONG_ROW = 1024             # rows longer than this get the running-sum SpMM bound
K_LAYER = 3                 # roundings of the graph-layer epilogues (fwd E + (side + E side), bwd g (1 + side) + acc)
K_MIX = 8                   # roundings of the transfer: a s, b t, their sum, (a + b) + 1e-7, the division, lam s, (1 - lam) t, two sums
K_NORM = 2                  # the sqrt and the rounding of the squared norm's last add beyond gamma_D
K_NORM_BWD = 4              # x / den, * proj, the subtraction, / den
K_COEF = 8                  # ulps of the BCE coefficient beyond its score error (expf, 1 - s, the division, 1 / B)
K_EMB = 4                   # EmbLoss: fp32 row sums of D squares, then fp64, a sqrt and two fp32 ops (as in test_gpu_step_fp64)
LOSS_RTOL = 1e-5
LAM_S, LAM_T, REG = 0.8, 0.8, 0.001
C4 = dict(OU=15435, TOU=6607, SOU=2651, OI=1, TOI=25802, SOI=33067)


def _ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    return torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))


def _check(tag, got, ref, bound, worst, name):
    got = got.double()
    assert got.shape == ref.shape, (tag, name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f'{tag} {name}: non-finite values'
    r = _ratio(got, ref, bound)
    w = float(r.max())
    worst[name] = max(worst.get(name, 0.0), w)
    if w > 1.0:
        j = int(r.reshape(-1).argmax())
        row, col = divmod(j, r.shape[1]) if r.dim() == 2 else (j, 0)
        g_, f_, b_ = (x.reshape(r.shape[0], -1)[row, col] for x in (got, ref, bound))
        raise AssertionError(f'{tag} {name}: error / bound = {w:.3g} at row {row} col {col}: got {float(g_)!r} want {float(f_)!r} '
                             f'bound {float(b_):.3g}')


def _fmt(worst):
    return ' '.join(f'{k}={v:.3g}' for k, v in worst.items())


# ---------------------------------------------------------------------------------------------------------------------- graphs

_CACHE = {}


@pytest.fixture(scope='module', autouse=True)
def _release_device_memory():
    """The graphs and their fp64 adjacencies are cached across this module's cases, and the offset-switch cases take ~30 GB through
    torch's caching allocator: afterwards all of it goes back to the device, so that later modules' free-HBM checks see what they
    saw without this module."""
    yield
    _CACHE.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _g1():
    if 'G1' not in _CACHE:
        from recbole_cdr_amd.data.synthetic import SyntheticCrossDomainDataset
        _CACHE['G1'] = SyntheticCrossDomainDataset(**C4, n_source_inter=809248, n_target_inter=2040000, seed=2022)
    return _CACHE['G1']


def _zipf_np(rng, n, rows, a=1.1):
    r = rng.rand(n)
    return np.clip((((float(rows) ** (1 - a) - 1) * r + 1) ** (1 / (1 - a))).astype(np.int64), 1, rows) - 1


def _g2():
    """The C4 id space with power-law degrees: a target item with 20,000 users, a target user with 5,000 items, many rows of one
    non-zero, overlapped users with no source pair, no target pair, and neither."""
    if 'G2' not in _CACHE:
        from oracle.common import IdSpace
        ids = IdSpace(**C4)
        rng = np.random.RandomState(7)
        nu, ni = ids.total_num_users, ids.total_num_items
        src_u = np.r_[1:ids.OU, ids.OU + ids.TOU:nu]; src_i = np.r_[1:ids.OI, ids.OI + ids.TOI:ni]
        tgt_u = np.r_[1:ids.OU + ids.TOU]; tgt_i = np.r_[1:ids.OI + ids.TOI]
        no_s, no_t, no_both = np.arange(100, 140), np.arange(200, 240), np.arange(300, 320)
        hub_i, hub_u = 777, ids.OU + 17                               # a target-only item, a target-only user

        def draw(us, its, n):
            pu, pi = rng.permutation(us), rng.permutation(its)
            return np.stack([pu[_zipf_np(rng, n, len(us))], pi[_zipf_np(rng, n, len(its))]], 1)
        s = draw(src_u, src_i, 809248)
        t = draw(tgt_u, tgt_i, 2040000)
        hub_fans = rng.choice(np.setdiff1d(tgt_u, np.r_[no_t, no_both]), 20000, replace=False)
        t = np.concatenate([t, np.stack([hub_fans, np.full(20000, hub_i)], 1),
                            np.stack([np.full(5000, hub_u), rng.choice(tgt_i, 5000, replace=False)], 1)])
        s = s[~np.isin(s[:, 0], np.r_[no_s, no_both])]
        t = t[~np.isin(t[:, 0], np.r_[no_t, no_both])]
        # the overlapped users with one empty domain get a few pairs in the other, so that batches reach them
        s = np.concatenate([s, np.stack([np.repeat(no_t, 3), rng.choice(src_i, 3 * len(no_t))], 1)])
        t = np.concatenate([t, np.stack([np.repeat(no_s, 3), rng.choice(tgt_i, 3 * len(no_s))], 1)])
        s, t = np.unique(s, axis=0), np.unique(t, axis=0)
        ds = FakeDataset(ids, s_pairs=s.astype(np.int64), t_pairs=t.astype(np.int64))
        ds.special = dict(no_s=no_s, no_t=no_t, no_both=no_both, hub_i=hub_i, hub_u=hub_u)
        _CACHE['G2'] = ds
    return _CACHE['G2']


def _g3():
    """An item-overlap id space (OI = 2,800) of more than 163,840 rows: the flagged backward reads its row bitmap from global memory."""
    if 'G3' not in _CACHE:
        from recbole_cdr_amd.data.synthetic import SyntheticCrossDomainDataset
        _CACHE['G3'] = SyntheticCrossDomainDataset(OU=20000, TOU=30000, SOU=30000, OI=2800, TOI=40000, SOI=45000,
                                                   n_source_inter=500000, n_target_inter=500000, seed=3)
    return _CACHE['G3']


def _pairs(ds, dom):
    return ds.s_pairs if dom == 'source' else ds.t_pairs


def _batch(ds, seed, S=2048):
    """2 x 4,096 rows in recbole's POINTWISE layout (S positives, S negatives), as bench.py --workload c4 draws them; on G2 the hubs
    and the overlapped users with an empty domain are forced in."""
    rng = np.random.RandomState(seed)
    out = {}
    sp = getattr(ds, 'special', None)
    n_items = ds.num_total_item if hasattr(ds, 'num_total_item') else ds.ids.total_num_items
    for dom in ('source', 'target'):
        pairs = _pairs(ds, dom)
        sel = pairs[rng.randint(0, len(pairs), S)].copy()
        if sp is not None:
            pick = lambda m, k: pairs[m][rng.permutation(int(m.sum()))[:k]]
            if dom == 'target':
                forced = np.concatenate([pick(np.isin(pairs[:, 0], sp['no_s']), 120), pick(pairs[:, 1] == sp['hub_i'], 200),
                                         pick(pairs[:, 0] == sp['hub_u'], 200)])
            else:
                forced = pick(np.isin(pairs[:, 0], sp['no_t']), 120)
            sel[:len(forced)] = forced
        items_all = np.unique(pairs[:, 1])
        u = np.tile(sel[:, 0], 2)
        i = np.concatenate([sel[:, 1], rng.choice(items_all, S)])
        y = np.concatenate([np.ones(S), np.zeros(S)]).astype(np.float32)
        assert int(i.max()) < n_items
        out[f'{dom}_user_id'] = torch.from_numpy(u).to(DEV)
        out[f'{dom}_item_id'] = torch.from_numpy(i).to(DEV)
        out[f'{dom}_label'] = torch.from_numpy(y).to(DEV)
    return out


def _model(ds, D=64, L=2, drop=0.3, cw='concat', sparse=True, fused=True):
    from recbole_cdr_amd.model.cross_domain_recommender.bitgcf import BiTGCF
    cfg = base_config(DEV, embedding_size=D, n_layers=L, reg_weight=REG, lambda_source=LAM_S, lambda_target=LAM_T, drop_rate=drop,
                      connect_way=cw, bitgcf_sparse_last_layer=sparse, bitgcf_fused_loss=fused)
    torch.manual_seed(2022)
    return BiTGCF(cfg, ds).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------- fp64 reference

class Adj:
    """One domain's normalised adjacency (the model's CSR) in fp64, with what the SpMM bound needs."""

    def __init__(self, g, chunk=1 << 20):
        ip = g.indptr.to(DEV)
        self.n = int(g.n_rows)
        self.col, self.val = g.indices.to(DEV), g.values.to(DEV).double()
        self.len = (ip[1:] - ip[:-1])
        self.row = torch.repeat_interleave(torch.arange(self.n, device=DEV), self.len)
        self.gl = (self.len.double() * U32 / (1.0 - self.len.double() * U32)).unsqueeze(1)      # gamma_{len_r}
        self.chunk = chunk
        self.lrows = torch.nonzero(self.len > LONG_ROW).flatten()
        if self.lrows.numel():
            lmask = (self.len > LONG_ROW)[self.row]
            self.lidx = torch.nonzero(lmask).flatten()                      # the long rows' non-zeros, CSR order
            ll = self.len[self.lrows]
            self.lseg = torch.repeat_interleave(torch.arange(self.lrows.numel(), device=DEV), ll)
            self.lstart = torch.cumsum(ll, 0) - ll

    def mm(self, X):
        out = torch.zeros(self.n, X.shape[1], device=DEV, dtype=torch.float64)
        for a in range(0, self.col.numel(), self.chunk):
            b = min(a + self.chunk, self.col.numel())
            out.index_add_(0, self.row[a:b], self.val[a:b, None] * X[self.col[a:b]])
        return out

    def spmm(self, X, eX, on_the_fly=None):
        """(A X, bound): X, eX fp64 [n, D]."""
        D = X.shape[1]
        Y = self.mm(torch.cat([X, X.abs(), eX], 1))
        AX, bound = Y[:, :D], self.gl * Y[:, D:2 * D] + Y[:, 2 * D:]
        if self.lrows.numel():
            P = self.val[self.lidx, None] * X[self.col[self.lidx]]
            C = P.cumsum(0)
            base = torch.where((self.lstart > 0).unsqueeze(1), C[(self.lstart - 1).clamp(min=0)], torch.zeros_like(C[:1]))
            part = C - base[self.lseg]
            run = torch.zeros(self.lrows.numel(), D, device=DEV, dtype=torch.float64)
            run.index_add_(0, self.lseg, part.abs() + P.abs())
            bound[self.lrows] = (1.0 + self.gl[self.lrows]) * U32 * run + Y[self.lrows, 2 * D:]
        return AX, bound


def _adj(model, key):
    """The two domains' Adj of graph ``key`` (every model of one dataset builds the same CSR)."""
    if ('adj', key) not in _CACHE:
        _CACHE[('adj', key)] = (Adj(model.source_graph), Adj(model.target_graph))
    return _CACHE[('adj', key)]


def _overlap_coefs(model, n, nu):
    """Per row: (c_ss, c_st, c_ts, c_tt, rounding factor) of the transfer, So = c_ss s + c_st t, To = c_ts s + c_tt t."""
    deg = model.degrees
    ds = torch.cat([deg['su'], deg['si']]).double()
    dt = torch.cat([deg['tu'], deg['ti']]).double()
    r = torch.arange(n, device=DEV)
    ov = (r < int(model.overlapped_num_users)) | ((r >= nu) & (r < nu + int(model.overlapped_num_items)))
    den = ds + dt + 1e-7
    ws, wt = ds / den, dt / den
    ls, lt = f32(LAM_S), f32(LAM_T)
    one, zero = torch.ones_like(ws), torch.zeros_like(ws)
    c_ss = torch.where(ov, (ls + ws) / 2, one); c_st = torch.where(ov, (1 - ls + wt) / 2, zero)
    c_ts = torch.where(ov, (1 - lt + ws) / 2, zero); c_tt = torch.where(ov, (lt + wt) / 2, one)
    k = torch.where(ov, torch.full_like(ws, gam(K_MIX)), zero)
    return [c.unsqueeze(1) for c in (c_ss, c_st, c_ts, c_tt, k)]


def propagate_fp64(model, adj, masks=None):
    """The reference's forward (bitgcf.py:174-205) in fp64 from the model's tables: (stacks {d: (value, bound)}, saved per layer)."""
    nu = model.total_num_users
    L = int(model.n_layers)
    E = {'s': torch.cat([model.source_user_embedding.weight, model.source_item_embedding.weight]).detach().double(),
         't': torch.cat([model.target_user_embedding.weight, model.target_item_embedding.weight]).detach().double()}
    n, D = E['s'].shape
    eE = {d: torch.zeros_like(E[d]) for d in 'st'}
    A = dict(zip('st', adj))
    c_ss, c_st, c_ts, c_tt, kmix = _overlap_coefs(model, n, nu)
    blocks = {d: [(E[d], torch.zeros_like(E[d]))] for d in 'st'}
    saved = []
    for l in range(L):
        lay = {}
        dr = {}
        for k, d in enumerate('st'):
            side, e_side = A[d].spmm(E[d], eE[d])
            Es = E[d] * side
            new = E[d] + (side + Es)
            e_new = eE[d] * (1 + side).abs() + e_side * (1 + E[d]).abs() + gam(K_LAYER) * (E[d].abs() + side.abs() + Es.abs())
            m = masks[(l, d)] if masks is not None else None
            if m is not None:
                new, e_new = m * new, m * e_new + U32 * (m * new).abs()
            dr[d] = (new, e_new)
            lay[d] = dict(E=E[d], eE=eE[d], side=side, e_side=e_side, m=m)
        (s, es), (t, et) = dr['s'], dr['t']
        xs = c_ss * s + c_st * t
        xt = c_ts * s + c_tt * t
        exs = c_ss * es + c_st * et + kmix * (c_ss * s.abs() + c_st * t.abs())
        ext = c_ts * es + c_tt * et + kmix * (c_ts * s.abs() + c_tt * t.abs())
        for d, x, ex in (('s', xs, exs), ('t', xt, ext)):
            nrm = x.norm(dim=1, keepdim=True)
            den = nrm.clamp(min=1e-12)
            e_nrm = gam(D + K_NORM) * nrm + ex.norm(dim=1, keepdim=True)
            y = x / den
            ey = (ex + y.abs() * e_nrm) / den + U32 * y.abs()
            blocks[d].append((y, ey))
            lay[d].update(x=x, ex=ex, nrm=den, e_nrm=e_nrm)
            E[d], eE[d] = x, ex
        saved.append(lay)
    nb = L + 1
    out = {}
    for d in 'st':
        if model.connect_way == 'concat':
            out[d] = (torch.cat([b[0] for b in blocks[d]], 1), torch.cat([b[1] for b in blocks[d]], 1))
        else:
            v = sum(b[0] for b in blocks[d]) / nb
            out[d] = (v, sum(b[1] for b in blocks[d]) / nb + gam(nb) * sum(b[0].abs() for b in blocks[d]) / nb)
    return out, saved, (c_ss, c_st, c_ts, c_tt, kmix)


def _scatter(n, W, rows, terms, absum, cerr):
    G = torch.zeros(n, W, device=DEV, dtype=torch.float64)
    A_, E_ = torch.zeros_like(G), torch.zeros_like(G)
    G.index_add_(0, rows, terms); A_.index_add_(0, rows, absum); E_.index_add_(0, rows, cerr)
    occ = torch.bincount(rows, minlength=n).double().unsqueeze(1)
    gk = (occ + K_SUM) * U32 / (1.0 - (occ + K_SUM) * U32)
    return G, gk * A_ + (1.0 + gk) * E_


def loss_fp64(model, inter, out, nu):
    """Both losses (bitgcf.py:207-240) and the stack gradients {d: (g, bound)} of  loss_s + loss_t."""
    losses, gstack, emb = [], {}, {}
    for d, pre in (('s', 'source'), ('t', 'target')):
        X, eX = out[d]
        n, W = X.shape
        u, i = inter[f'{pre}_user_id'].long(), inter[f'{pre}_item_id'].long() + nu
        y = inter[f'{pre}_label'].double()
        B = u.numel()
        a, b, ea, eb = X[u], X[i], eX[u], eX[i]
        x = (a * b).sum(1)
        ex = gam(W) * (a * b).abs().sum(1) + (a.abs() * eb + ea * b.abs()).sum(1)
        s = torch.sigmoid(x)
        bce = -(y * torch.log(s).clamp(min=-100) + (1 - y) * torch.log1p(-s).clamp(min=-100)).mean()
        c = ((s - y) / B).unsqueeze(1)
        ec = (s * (1 - s) * ex / B + K_COEF * U32 * ((s - y).abs() / B + s / B)).unsqueeze(1)
        rows = torch.cat([u, i])
        gstack[d] = _scatter(n, W, rows, torch.cat([c * b, c * a]), torch.cat([c.abs() * b.abs(), c.abs() * a.abs()]),
                             torch.cat([ec * b.abs() + c.abs() * eb, ec * a.abs() + c.abs() * ea]))
        wu = getattr(model, f'{pre}_user_embedding').weight.detach().double()
        wi = getattr(model, f'{pre}_item_embedding').weight.detach().double()
        Ub, Ib = wu[u], wi[i - nu]
        nu_, ni_ = Ub.norm(), Ib.norm()
        losses.append(float(bce + REG * (nu_ + ni_) / B))
        emb[d] = (torch.cat([u, i]), torch.cat([REG / (B * nu_) * Ub, REG / (B * ni_) * Ib]))
    return losses, gstack, emb


def backward_fp64(model, adj, saved, coefs, gstack, emb):
    """The four table gradients {name: (g, bound)} of loss_s + loss_t from the stack gradients, by hand."""
    L, D = int(model.n_layers), model.latent_dim
    nb = L + 1
    nu = model.total_num_users
    A = dict(zip('st', adj))
    c_ss, c_st, c_ts, c_tt, kmix = coefs
    gblk = {}
    for d in 'st':
        G, eG = gstack[d]
        if model.connect_way == 'concat':
            gblk[d] = [(G[:, b * D:(b + 1) * D], eG[:, b * D:(b + 1) * D]) for b in range(nb)]
        else:
            gblk[d] = [(G / nb, eG / nb + U32 * (G / nb).abs())] * nb
    gprev = {d: None for d in 'st'}
    for l in reversed(range(L)):
        lay = saved[l]
        ga = {}
        for d in 'st':
            s_ = lay[d]
            gy, egy = gblk[d][l + 1]
            den, e_nrm, x, ex = s_['nrm'], s_['e_nrm'], s_['x'], s_['ex']
            y = x / den
            p = (y * gy).sum(1, keepdim=True)
            ey = (ex + y.abs() * e_nrm) / den
            ep = (ey * gy.abs()).sum(1, keepdim=True) + (y.abs() * egy).sum(1, keepdim=True) + gam(D) * (y.abs() * gy.abs()).sum(1, keepdim=True)
            v = (gy - y * p) / den
            ev = (egy + ey * p.abs() + y.abs() * ep) / den + v.abs() * e_nrm / den + gam(K_NORM_BWD) * (gy.abs() + y.abs() * p.abs()) / den
            if gprev[d] is not None:
                g0, e0 = gprev[d]
                v, ev = g0 + v, e0 + ev + U32 * (g0 + v).abs()
            ga[d] = (v, ev)
        (a, ea), (b, eb) = ga['s'], ga['t']
        gn = {'s': (c_ss * a + c_ts * b, c_ss * ea + c_ts * eb + kmix * (c_ss * a.abs() + c_ts * b.abs())),
              't': (c_st * a + c_tt * b, c_st * ea + c_tt * eb + kmix * (c_st * a.abs() + c_tt * b.abs()))}
        for d in 'st':
            g, eg = gn[d]
            m = lay[d]['m']
            if m is not None:
                g, eg = m * g, m * eg + U32 * (m * g).abs()
            E, eE, side, e_side = lay[d]['E'], lay[d]['eE'], lay[d]['side'], lay[d]['e_side']
            tmp = g * (1 + E)
            etmp = eg * (1 + E).abs() + g.abs() * eE + gam(2) * tmp.abs()
            At, eAt = A[d].spmm(tmp, etmp)
            own = g * (1 + side)
            gE = own + At
            egE = eg * (1 + side).abs() + g.abs() * e_side + eAt + gam(K_LAYER) * (own.abs() + At.abs())
            gprev[d] = (gE, egE)
    res = {}
    for d, pre in (('s', 'source'), ('t', 'target')):
        g0, e0 = gblk[d][0]
        if gprev[d] is not None:
            g0, e0 = gprev[d][0] + g0, gprev[d][1] + e0
        rows, terms = emb[d]
        G = torch.zeros_like(g0)
        Aabs = torch.zeros_like(g0)
        G.index_add_(0, rows, terms); Aabs.index_add_(0, rows, terms.abs())
        occ = torch.bincount(rows, minlength=g0.shape[0]).double().unsqueeze(1)
        gk = (occ + K_SUM) * U32 / (1.0 - (occ + K_SUM) * U32)
        g = g0 + G
        e = e0 + gk * (g0.abs() + Aabs) + gam(D + K_EMB) * Aabs
        res[f'{pre}_user_embedding.weight'] = (g[:nu], e[:nu])
        res[f'{pre}_item_embedding.weight'] = (g[nu:], e[nu:])
    return res


def _masks(model, seed_val, p):
    """The device's own dropout masks of every (layer, domain): cdr_dropout_dev on ones, same seed, salt 2 l + k."""
    from recbole_cdr_amd import binding as B_
    n, D = model.total_num_users + model.total_num_items, model.latent_dim
    seed = torch.full((1,), seed_val, device=DEV, dtype=torch.int64)
    ones = torch.ones(n, D, device=DEV)
    out = {}
    for l in range(int(model.n_layers)):
        for k, d in enumerate('st'):
            m = torch.empty_like(ones)
            B_.call('cdr_dropout_dev', B_.stream(), B_.f32(ones), ones.numel(), p, B_.i64(seed), 2 * l + k, B_.f32(m))
            out[(l, d)] = m.double()
    return out


class _Spy:
    def __init__(self):
        from recbole_cdr_amd import binding as B_
        self.B_, self.real, self.seen = B_, B_.call, []

    def __enter__(self):
        def spy(name, *a):
            self.seen.append(name)
            return self.real(name, *a)
        self.B_.call = spy
        return self.seen

    def __exit__(self, *exc):
        self.B_.call = self.real


# ---------------------------------------------------------------------------------------------------------------------- one training step

def _run_case(tag, ds, gkey, bseed=2022, want_calls=(), not_calls=(), **kw):
    """calculate_loss + backward on the model, against the fp64 reference: both losses, the batch rows of both propagated stacks,
    the four table gradients.  Returns (model, worst, table gradients)."""
    from recbole_cdr_amd.utils import total_loss
    model = _model(ds, **kw)
    model.train()
    inter = _batch(ds, bseed)
    nu = model.total_num_users
    adj = _adj(model, gkey)
    p = float(model.drop_rate)
    torch.manual_seed(77)
    seed_val = int(torch.empty((), dtype=torch.int64).random_(0, 2 ** 62).item())
    masks = _masks(model, seed_val, p) if p else None
    # the propagated stacks the loss reads: the same launches (and the same dropout seed) as inside calculate_loss
    hint = (inter['source_user_id'], inter['source_item_id'], inter['target_user_id'], inter['target_item_id']) if model.sparse_last_layer else None
    torch.manual_seed(77)
    with torch.no_grad():
        S, T, _, _ = model._propagate(hint)
    torch.manual_seed(77)
    with _Spy() as seen:
        losses = model.calculate_loss(inter)
        total_loss(losses).sum().backward()
    torch.cuda.synchronize()
    if p:
        assert int(model._drop_state.item()) == seed_val
    for c in want_calls:
        assert c in seen, f'{tag}: {c} did not run ({sorted(set(seen))})'
    for c in not_calls:
        assert c not in seen, f'{tag}: {c} ran'
    out, saved, coefs = propagate_fp64(model, adj, masks)
    ref_losses, gstack, emb = loss_fp64(model, inter, out, nu)
    for got, want in zip(losses, ref_losses):
        got = float(got.detach())
        assert abs(got - want) <= LOSS_RTOL * abs(want), f'{tag}: loss {got!r} vs fp64 {want!r}'
    worst = {}
    rows = torch.unique(torch.cat([inter['source_user_id'], inter['target_user_id'], inter['source_item_id'] + nu, inter['target_item_id'] + nu]))
    for d, X in (('s', S), ('t', T)):
        _check(tag, X[rows], out[d][0][rows], out[d][1][rows], worst, f'stack_{d}')
    del S, T
    want = backward_fp64(model, adj, saved, coefs, gstack, emb)
    for k, v in model.named_parameters():
        _check(tag, v.grad, *want[k], worst, k.split('_embedding')[0])
    print(f'\n{tag}: losses {[float(x.detach()) for x in losses]} worst error / bound: {_fmt(worst)}')
    return model, worst, want


SPARSE_FUSED = ('cdr_row_flags', 'cdr_point_fwd_pair_ex', 'cdr_point_bwd_dense_pair')


@pytest.mark.parametrize('variant', ['c4', 'drop0', 'full_last_layer', 'unfused', 'mean', 'L3', 'D128', 'D40'])
def test_bitgcf_g1_vs_fp64(variant):
    """G1: exactly the graph bench.py --workload c4 builds; C4 defaults and one change each."""
    kw, want, no = {}, SPARSE_FUSED, ()
    if variant == 'drop0':
        kw = dict(drop=0.0)
    elif variant == 'full_last_layer':
        kw, want, no = dict(sparse=False), ('cdr_graph_layer_fwd', 'cdr_graph_layer_bwd'), ('cdr_row_flags', 'cdr_point_fwd_pair_ex')
    elif variant == 'unfused':
        kw, want, no = dict(fused=False), ('cdr_row_flags',), ('cdr_point_fwd_pair_ex',)
    elif variant == 'mean':
        kw = dict(cw='mean')
    elif variant == 'L3':
        kw = dict(L=3)
    elif variant == 'D128':
        kw = dict(D=128)
    elif variant == 'D40':
        kw = dict(D=40)
    _run_case(f'G1 {variant}', _g1(), 'G1', want_calls=want, not_calls=no, **kw)


def test_bitgcf_g1_deterministic_vs_fp64():
    """G1, C4 defaults under set_deterministic(True): the ordered scatters, within the same bounds and bit-equal across two runs."""
    from recbole_cdr_amd import functional as F_
    try:
        F_.set_deterministic(True)
        m1, _, _ = _run_case('G1 deterministic', _g1(), 'G1', want_calls=('cdr_row_flags', 'cdr_point_fwd_pair_ex', 'cdr_ordered_bwd'),
                             not_calls=('cdr_point_bwd_dense_pair',))
        g1 = {k: v.grad.clone() for k, v in m1.named_parameters()}
        del m1
        m2, _, _ = _run_case('G1 deterministic (again)', _g1(), 'G1')
        for k, v in m2.named_parameters():
            assert torch.equal(v.grad.view(torch.int32), g1[k].view(torch.int32)), f'{k}: not bit-equal across runs'
    finally:
        F_.set_deterministic(False)


@pytest.mark.parametrize('variant', ['c4', 'D128'])
def test_bitgcf_g2_power_law_vs_fp64(variant):
    """G2: the C4 id space with power-law degrees, a 20,000-user item, a 5,000-item user, rows of one non-zero, overlapped users
    with an empty domain (batches include them and the hubs)."""
    ds = _g2()
    sp = ds.special
    m = _model(ds)
    a_s, a_t = _adj(m, 'G2')
    nu = m.total_num_users
    assert int(a_t.len[nu + sp['hub_i']]) >= 20000 and int(a_t.len[sp['hub_u']]) >= 5000
    assert int((a_s.len == 1).sum()) > 100 and int((a_t.len == 1).sum()) > 100
    deg = m.degrees
    assert float(deg['su'][sp['no_s']].max()) == 0 and float(deg['tu'][sp['no_s']].min()) > 0
    assert float(deg['tu'][sp['no_t']].max()) == 0 and float(deg['su'][sp['no_t']].min()) > 0
    assert float(deg['su'][sp['no_both']].max()) == 0 and float(deg['tu'][sp['no_both']].max()) == 0
    assert int(sp['no_both'].max()) < m.overlapped_num_users
    del m
    _run_case(f'G2 {variant}', ds, 'G2', want_calls=SPARSE_FUSED, **(dict(D=128) if variant == 'D128' else {}))


@pytest.mark.parametrize('L', [2, 1])
def test_bitgcf_g3_global_bitmap_vs_fp64(L):
    """G3: more than 163,840 rows (the flagged backward's bitmap does not fit its 20 KB of LDS) and item overlap (OI = 2,800)."""
    ds = _g3()
    n = ds.num_total_user + ds.num_total_item
    assert n > 163840 and (n + 31) // 32 * 4 > 20 * 1024
    _run_case(f'G3 L={L}', ds, 'G3', want_calls=SPARSE_FUSED, L=L)


# ---------------------------------------------------------------------------------------------------------------------- evaluation

@pytest.mark.parametrize('graph', ['G1', 'G2'])
def test_bitgcf_evaluation_vs_fp64(graph):
    """forward() on every row, predict and full_sort_predict for 64 target users (eval: no dropout, every row of the last layer)."""
    ds = _g1() if graph == 'G1' else _g2()
    model = _model(ds)
    model.eval()
    nu, nti = model.total_num_users, model.target_num_items
    adj = _adj(model, graph)
    out, _, _ = propagate_fp64(model, adj, None)
    worst = {}
    with torch.no_grad():
        got = model.forward()
    for (name, X), (d, sl) in zip(zip(('su', 'si', 'tu', 'ti'), got), (('s', slice(0, nu)), ('s', slice(nu, None)), ('t', slice(0, nu)),
                                                                        ('t', slice(nu, None)))):
        _check(graph, X, out[d][0][sl], out[d][1][sl], worst, name)
    rng = np.random.RandomState(5)
    users = torch.from_numpy(rng.choice(np.unique(ds.t_pairs[:, 0]), 64, replace=False)).to(DEV)
    if graph == 'G2':
        users[:3] = torch.tensor([int(ds.special['hub_u']), int(ds.special['no_s'][0]), int(ds.special['no_both'][0])])
    items = torch.from_numpy(rng.randint(0, nti, 64)).to(DEV)
    Tu, eTu = out['t'][0][:nu], out['t'][1][:nu]
    Ti, eTi = out['t'][0][nu:nu + nti], out['t'][1][nu:nu + nti]
    W = Tu.shape[1]
    a, ea, b, eb = Tu[users], eTu[users], Ti[items], eTi[items]
    sc = (a * b).sum(1)
    esc = gam(W) * (a * b).abs().sum(1) + (a.abs() * eb + ea * b.abs()).sum(1)
    with torch.no_grad():
        pr = model.predict({model.TARGET_USER_ID: users, model.TARGET_ITEM_ID: items})
    _check(graph, pr.reshape(-1, 1), sc.unsqueeze(1), esc.unsqueeze(1), worst, 'predict')
    full_ref = a @ Ti.t()
    efull = gam(W) * (a.abs() @ Ti.abs().t()) + a.abs() @ eTi.t() + ea @ Ti.abs().t()
    with torch.no_grad():
        full = model.full_sort_predict({model.TARGET_USER_ID: users}).view(64, -1)
    _check(graph, full, full_ref, efull, worst, 'full_sort')
    print(f'\n{graph} evaluation: worst error / bound: {_fmt(worst)}')


# ---------------------------------------------------------------------------------------------------------------------- Adam

def test_bitgcf_g1_dense_adam_step_vs_fp64():
    """G1, C4 defaults: two DenseAdam steps (the optimizer C4 trains with), each from the device's own state and gradient, against
    fp64 Adam (fp64_bounds.apply_fp64: the gradient is the step's exact input, so its bound is zero)."""
    from recbole_cdr_amd.trainer.trainer import DenseAdam
    model, _, _ = _run_case('G1 adam', _g1(), 'G1')
    lr = 1e-3
    opt = DenseAdam(model.parameters(), lr=lr)
    worst = {}
    for t in (1, 2):
        before = {}
        for k, p in model.named_parameters():
            st = opt.state[p]
            before[k] = dict(w=p.detach().clone(), m=st['exp_avg'].clone() if st else torch.zeros_like(p),
                             v=st['exp_avg_sq'].clone() if st else torch.zeros_like(p), g=p.grad.detach().double())
        opt.step()
        torch.cuda.synchronize()
        for k, p in model.named_parameters():
            b = before[k]
            rows = torch.arange(p.shape[0], device=DEV)
            z = torch.zeros_like(b['g'])
            want = apply_fp64(b, (rows, b['g'], z, z, torch.zeros(p.shape[0], device=DEV, dtype=torch.int64)), p.shape[1], 'adam', lr, 0.0, t)
            st = opt.state[p]
            assert int(st['step'].item()) == t
            for name, got in (('w', p.detach()), ('m', st['exp_avg']), ('v', st['exp_avg_sq'])):
                _check(f'G1 adam step {t}', got, *want[name], worst, f'{k.split("_embedding")[0]}.{name}')
    print(f'\nG1 DenseAdam: worst error / bound over 2 steps: {_fmt(worst)}')


# ---------------------------------------------------------------------------------------------------------------------- row-sharded form

def _shard_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import recbole_cdr_amd  # noqa: F401
        from recbole_cdr_amd.bitgcf_shard import NativeGraphOps, ShardedBiTGCF
        torch.cuda.set_device(0)
        ds = _g1()
        params = _shard_params(ds)
        m = ShardedBiTGCF(ds.num_total_user, ds.num_total_item, ds.num_overlap_user, ds.num_overlap_item, ds.s_pairs, ds.t_pairs, 64, 2,
                          LAM_S, LAM_T, 'concat', REG, NativeGraphOps(DEV), init=params)
        losses = [float(x) for x in m.loss_and_grads(_batch(ds, 2022))]
        p = m.part
        grads = {}
        for k, v in m.params.items():
            users = '_user_' in k
            blk, total = (p.bu, p.nu) if users else (p.bi, p.ni)
            lo = rank * blk
            cnt = max(0, min(blk, total - lo))
            grads[k] = (np.arange(lo, lo + cnt), v.grad[:cnt].detach().cpu().numpy())
        prop = [t.cpu().numpy() for t in m.propagated_tables()]
        q.put((rank, losses, grads, prop))
    finally:
        dist.destroy_process_group()


def _shard_params(ds):
    g = torch.Generator().manual_seed(9)
    return {k: torch.randn(ds.num_total_user if '_user_' in k else ds.num_total_item, 64, generator=g) * 0.1
            for k in ('source_user_embedding.weight', 'source_item_embedding.weight', 'target_user_embedding.weight',
                      'target_item_embedding.weight')}


def test_bitgcf_row_sharded_g1_vs_fp64():
    """ShardedBiTGCF + NativeGraphOps on G1, world 2 over gloo on one GPU, drop_rate 0: each rank's losses, its table-gradient rows
    (global row ids) and the propagated tables against the same reference."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = collect_ranks(q, procs)
    ds = _g1()
    model = _model(ds, drop=0.0, sparse=False)
    load_params(model, _shard_params(ds))
    nu = model.total_num_users
    adj = _adj(model, 'G1')
    out, saved, coefs = propagate_fp64(model, adj, None)
    inter = _batch(ds, 2022)
    ref_losses, gstack, emb = loss_fp64(model, inter, out, nu)
    want = backward_fp64(model, adj, saved, coefs, gstack, emb)
    worst = {}
    for r, losses, grads, prop in res:
        for got, w in zip(losses, ref_losses):
            assert abs(got - w) <= LOSS_RTOL * abs(w), f'rank {r}: loss {got!r} vs fp64 {w!r}'
        for k, (rows, g) in grads.items():
            rows = torch.from_numpy(rows).to(DEV)
            _check(f'rank {r}', torch.from_numpy(g).to(DEV), want[k][0][rows], want[k][1][rows], worst, k.split('_embedding')[0])
        for X, (d, sl) in zip(prop, (('s', slice(0, nu)), ('s', slice(nu, None)), ('t', slice(0, nu)), ('t', slice(nu, None)))):
            _check(f'rank {r}', torch.from_numpy(X).to(DEV), out[d][0][sl], out[d][1][sl], worst, f'prop_{d}')
    print(f'\nG1 row-sharded world 2: worst error / bound: {_fmt(worst)}')


# ---------------------------------------------------------------------------------------------------------------------- 32-bit offsets

@pytest.mark.parametrize('flags', [False, True])
@pytest.mark.parametrize('side', ['below', 'above'])
def test_graph_layer_offset_switch_vs_fp64(side, flags):
    """cdr_graph_layer_fwd / _bwd at D = 64 on a random square graph of 4 non-zeros per row (and 8 rows of 5,000 reaching the
    highest indices) with n 64 = 2^30 -+ 64: the two sides of the kernels' 32-bit element-offset switch.  20,000 random rows, the
    last 1,000 and the long rows against fp64 of those rows; with flags, rows outside them must stay unwritten (forward) and the
    backward sees a gradient only on the flagged rows."""
    import ctypes
    from recbole_cdr_amd import binding as B_
    D = 64
    n = (1 << 24) - 1 if side == 'below' else (1 << 24) + 1
    free_b, _ = torch.cuda.mem_get_info()
    if free_b < 48e9:
        pytest.skip('needs ~40 GB of free HBM (six [2^24, 64] fp32 buffers and a 67 M non-zero graph)')
    gen = torch.Generator(device=DEV); gen.manual_seed(n)
    long_rows = torch.tensor([0, 1, n // 3, n // 2, n - 1001, n - 3, n - 2, n - 1], device=DEV)
    lens = torch.full((n,), 4, device=DEV, dtype=torch.int64)
    lens[long_rows] = 5000
    indptr = torch.zeros(n + 1, device=DEV, dtype=torch.int64)
    indptr[1:] = torch.cumsum(lens, 0)
    nnz = int(indptr[-1])
    cols = torch.randint(0, n, (nnz,), device=DEV, generator=gen)
    for r in long_rows.tolist():
        cols[int(indptr[r]):int(indptr[r + 1])] = n - 5000 + torch.arange(5000, device=DEV)      # the highest indices, ascending
    cols[indptr[n - 1000:n]] = n - 1                                                               # the last rows reach row n - 1
    vals = torch.rand(nnz, device=DEV, generator=gen) * 0.5 + 0.01
    E = torch.randn(n, D, device=DEV, generator=gen) * 0.1
    sample = torch.unique(torch.cat([torch.randint(0, n, (20000,), device=DEV, generator=gen), torch.arange(n - 1000, n, device=DEV), long_rows]))
    fl = None
    if flags:
        flagged = torch.unique(torch.cat([torch.randint(0, n, (1 << 20,), device=DEV, generator=gen), torch.arange(n - 500, n, device=DEV),
                                          long_rows[::2]]))
        need = ctypes.c_size_t(0)
        B_._check(B_.load().cdr_row_flags_layout(n, ctypes.byref(need)), 'cdr_row_flags_layout')
        fl = torch.empty(int(need.value), device=DEV, dtype=torch.uint8)
        ids = [flagged]
        B_._alive.extend(ids)
        B_.call('cdr_row_flags', B_.stream(), 1, (ctypes.c_void_p * 1)(flagged.data_ptr()), (ctypes.c_int64 * 1)(flagged.numel()),
                (ctypes.c_int64 * 1)(0), n, B_.raw(fl), fl.numel())
        fmask = torch.zeros(n, dtype=torch.bool, device=DEV)
        fmask[flagged] = True
    side_o = torch.full((n, D), float('nan'), device=DEV)
    new_o = torch.full((n, D), float('nan'), device=DEV)
    B_.call('cdr_graph_layer_fwd', B_.stream(), B_.i64(indptr), B_.i64(cols), B_.f32(vals), n, B_.f32(E), D, B_.f32(side_o), B_.f32(new_o),
            B_.raw(fl) if flags else None)
    torch.cuda.synchronize()
    # fp64 of the sampled rows only
    sl = lens[sample]
    srow = torch.repeat_interleave(torch.arange(sample.numel(), device=DEV), sl)
    pos = torch.repeat_interleave(indptr[sample], sl) + (torch.arange(int(sl.sum()), device=DEV) - torch.repeat_interleave(torch.cumsum(sl, 0) - sl, sl))
    sc, sv = cols[pos], vals[pos].double()

    def rows_spmm(X, eX):
        P = sv[:, None] * X[sc].double()
        out = torch.zeros(sample.numel(), D, device=DEV, dtype=torch.float64)
        A_ = torch.zeros_like(out)
        out.index_add_(0, srow, P); A_.index_add_(0, srow, P.abs())
        bnd = (sl.double() * U32 / (1 - sl.double() * U32)).unsqueeze(1) * A_
        if eX is not None:
            eA = torch.zeros_like(out); eA.index_add_(0, srow, sv[:, None] * eX[sc]); bnd = bnd + eA
        lng = torch.nonzero(sl > LONG_ROW).flatten()
        for j in lng.tolist():                                       # the running-sum bound of the few long rows
            seg = srow == j
            Pj = P[seg]
            bnd[j] = (1 + gam(int(sl[j]))) * U32 * (Pj.cumsum(0).abs().sum(0) + Pj.abs().sum(0)) + (0 if eX is None else eA[j])
        return out, bnd

    worst = {}
    Ed = E[sample].double()
    sd, esd = rows_spmm(E, None)
    nw = Ed + (sd + Ed * sd)
    enw = esd * (1 + Ed).abs() + gam(K_LAYER) * (Ed.abs() + sd.abs() + (Ed * sd).abs())
    chk = fmask[sample] if flags else torch.ones(sample.numel(), dtype=torch.bool, device=DEV)
    tag = f'offsets n={n} flags={flags}'
    _check(tag, side_o[sample][chk], sd[chk], esd[chk], worst, 'side')
    _check(tag, new_o[sample][chk], nw[chk], enw[chk], worst, 'new')
    if flags:
        assert bool(torch.isnan(new_o[sample][~chk]).all()) and bool(torch.isnan(side_o[sample][~chk]).all()), f'{tag}: unflagged rows written'
    del new_o
    gnew = torch.randn(n, D, device=DEV, generator=gen) * 0.01
    if flags:
        gnew[~fmask] = 0.0
    tmp = torch.empty(n, D, device=DEV)
    gE = torch.full((n, D), float('nan'), device=DEV)
    B_.call('cdr_graph_layer_bwd', B_.stream(), B_.i64(indptr), B_.i64(cols), B_.f32(vals), n, B_.f32(E), B_.f32(side_o), B_.f32(gnew), D,
            B_.f32(tmp), B_.f32(gE), B_.raw(fl) if flags else None)
    torch.cuda.synchronize()
    del tmp
    # the kernel's own side rows are its input: fp64 from them (side_o of unflagged rows is never read: their gnew is zero)
    sdev = torch.nan_to_num(side_o, nan=0.0)
    del side_o
    g = gnew
    # tmp = g (1 + E) on the sampled rows' columns only
    P = sv[:, None] * (g[sc].double() * (1 + E[sc].double()))
    etmp_abs = gam(2) * P.abs()
    At = torch.zeros(sample.numel(), D, device=DEV, dtype=torch.float64)
    Aa = torch.zeros_like(At); eAt = torch.zeros_like(At)
    At.index_add_(0, srow, P); Aa.index_add_(0, srow, P.abs()); eAt.index_add_(0, srow, etmp_abs)
    bnd = (sl.double() * U32 / (1 - sl.double() * U32)).unsqueeze(1) * Aa + eAt
    for j in torch.nonzero(sl > LONG_ROW).flatten().tolist():
        Pj = P[srow == j]
        bnd[j] = (1 + gam(int(sl[j]))) * U32 * (Pj.cumsum(0).abs().sum(0) + Pj.abs().sum(0)) + eAt[j]
    gs = g[sample].double()
    own = gs * (1 + sdev[sample].double())
    want = own + At
    ewant = bnd + gam(K_LAYER) * (own.abs() + At.abs())
    _check(tag, gE[sample], want, ewant, worst, 'gE')
    print(f'\n{tag}: worst error / bound: {_fmt(worst)}')
