"""The five extra models' row kernels (csrc/cdr_rowmodels.hip) and the two loss kernels they share with CoNet (cdr_bce_prob_*,
cdr_frobenius_*: csrc/cdr_elem.hip), driven through their autograd.Functions with a random upstream gradient, against a float64
restatement of the reference formulas:
  NatrAttention    oracle/natr.py:25-43 (phase2_forward)         MaxMinNormalize   oracle/dcdcsr.py:30-34 (maxmin_normalize)
  ApfProduct / ApfCombine   oracle/deepapf.py:18-36 (forward)     GatherMaxConcat   oracle/dtcdr.py:23-25 (neumf_forward)
  BCEProbLoss      torch.nn.BCELoss (log clamped at -100; backward (p - y) / max((1 - p) p, 1e-12))       FrobeniusNorm   torch.norm

Every restatement runs on fp64_bounds.EV pairs: the float64 value and a per-element first-order bound of the fp32 kernel's error, built
operation by operation in the order the kernel computes (one rounding per fp32 operation, gamma_{n-1} per n-term sum in any order,
K_EXP / K_SIG ulps for expf / the sigmoid, cdr_colsum's real depth for the parameter gradients' sums over the batch).  The backward
restatements start from the forward's EV outputs -- the kernels read their own fp32 att / su / beta / p back -- so the forward's error
rides along.  Nothing is skipped: a sign the kernel takes from a COMPUTED quantity (su . qi in NATR's gate) that is smaller than its own
bound makes that step ambiguous (error 1 on the step, both branches inside the bound); such rows are counted and capped at 0.5 % per
case by ``test_case_table_covers_every_regime``, which runs every restatement on the CPU (test_fp64_bounds.py).  Signs and comparisons of
INPUT values (pu . He, max / min ties, torch.maximum) are exact in fp32 and never ambiguous.

wave_grid caps at 2,048 workgroups x 4 waves: from row 8,193 on a wave takes a second row and reuses its LDS score array; the
elementwise kernels loop from 2,048 x 256 elements on.  Each family has a case past its cap."""
import itertools

import pytest
import torch

from fp64_bounds import EV, U32, colsum_depth, ev_cat, ev_where, gam
from helpers import DEV

pytestmark = pytest.mark.gpu

AMB_CAP = 0.005
WAVE_ROWS = 2048 * 4                 # wave_grid's cap (cdr_rowmodels.hip:15-21): rows past it start the grid-stride loop
ELEM_CAP = 2048 * 256                # grid_cap x kBlock elements
MAX_DIM, MAX_HIST = 256, 256         # CDR_ROWMODEL_MAX_DIM, CDR_NATR_MAX_HIST (include/cdr_hip.h)
K_LOG = 2                            # ulps of logf (ocml documents 1)
SENTINEL = -7.25e22

_worst = {}


def _record(family, ratios):
    w = max(ratios.values())
    _worst[family] = max(_worst.get(family, 0.0), w)
    print(f'\n[{family}] error / bound: ' + ' '.join(f'{k}={v:.3f}' for k, v in ratios.items()) + f' (family so far {_worst[family]:.3f})')
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (family, bad)


def _ratio(ref, got):
    assert got.shape == ref.v.shape, (tuple(got.shape), tuple(ref.v.shape))
    assert bool(torch.isfinite(got).all())
    return float(ref.ratio(got).max())


def _t(x):
    return EV(x.double())


# ---------------------------------------------------------------------------------------------------------------------- NATR

def _natr_cases():
    """(B, L, D).  J = ceil(D / 64) registers per lane: every J with a full and a ragged last register, every L edge, the widest J at
    the longest histories, and one batch past wave_grid's cap (every wave takes a second row)."""
    wide = [(1, 1), (63, 2), (64, 50), (65, 255), (65, 2), (100, 256), (128, 50), (129, 1), (129, 256), (192, 255), (193, 50),
            (193, 256), (256, 256), (256, 2), (1, 256)]
    return [(37, L, D) for D, L in wide] + [(WAVE_ROWS + 1 + 6, 3, 8)]


# With 37 rows the 0.5 % cap allows no ambiguous row at all, and a row has up to 256 chances of a |su . qi| below its bound.  So the inputs
# keep su . qi away from 0 by construction: |qi| >= 0.3, and every history column of a row is centred on c = +-[0.5, 0.9] with a spread of
# 0.25 (both signs of pu . He still occur down a column and across columns; su, an average of the column, stays near c).  A fully padded
# row's scores are all (score - 10000): the fp32 add leaves them u 10^4 = 6e-4 from their float64 values, in the reference as in the
# kernel, and att / su inherit that -- those rows get strictly one-signed columns with |He| >= 0.3.  The table test holds the cap on the float64 reference alone.


def _natr_inputs(B, L, D):
    gen = torch.Generator().manual_seed(B * 5 + L * 3 + D)
    r = lambda *s, k=1.0: torch.randn(*s, generator=gen) * k
    mag = lambda *s: torch.rand(*s, generator=gen) * 0.6 + 0.3
    sgn = lambda *s: (torch.rand(*s, generator=gen) < 0.5).float() * 2 - 1
    pu, qi = r(B, D, k=0.6), sgn(B, D) * mag(B, D)
    He = sgn(B, 1, D) * (torch.rand(B, 1, D, generator=gen) * 0.4 + 0.5) + r(B, L, D, k=0.25)
    lens = torch.randint(0, L + 1, (B,), generator=gen)
    lens[0], lens[1], lens[2] = 0, 1, L                         # a fully padded row, one real entry, a full row
    mask = (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)).float()
    pad = lens == 0
    He[pad] = (sgn(B, 1, D) * mag(B, L, D))[pad]
    s = 1.0 / D ** 0.5
    wu, bu, wd, bd = r(1, D, k=s), r(1, k=0.1), r(1, D, k=s), r(1, k=0.1)
    gp = r(B, k=0.8) + 0.3
    return He, pu, qi, mask, wu, bu, wd, bd, gp


def natr_fp64(He, pu, qi, mask, wu, bu, wd, bd, gp):
    """natr_fwd_kernel / natr_bwd_kernel (cdr_rowmodels.hip:212-378) on EV pairs.  Returns ({name: EV}, ambiguous rows, |logit| max)."""
    B, L, D = He.shape
    H, P, Q = _t(He), _t(pu), _t(qi)
    WU, WD, BU, BD = _t(wu.reshape(-1)), _t(wd.reshape(-1)), _t(bu.reshape(())), _t(bd.reshape(()))
    P1 = P.unsqueeze(1)
    x = P1 * H                                                   # pu . He: one rounding, the sign exact
    r_in = EV((x.v > 0).double())
    t = x.relu()
    sc = (WU * t).sum(2) + BU
    sc = sc + EV((mask == 0).double() * -10000.0)  # the fp32 add of -10000 costs u 10^4: charged by the add's own rounding
    # softmax is invariant under a shift common to the row: the float64 side may subtract the kernel's OWN maximum (which lies within
    # its bound of this one), so the maximum's error never enters att -- only the subtraction's rounding does
    mx = EV(sc.v.amax(1, keepdim=True))
    ex = (sc - mx).exp()
    att = ex / ex.sum(1, keepdim=True)
    su = (att.unsqueeze(2) * H).sum(1)
    xs, xp = su * Q, P * Q
    bs = (WD * xs.relu()).sum(1) + BD
    bp = (WD * xp.relu()).sum(1) + BD
    es, ep = bs.exp(), bp.exp()
    beta = es / (es + ep)
    b1, nb1 = beta.unsqueeze(1), (1.0 - beta).unsqueeze(1)
    zu = b1 * su + nb1 * P
    p = (zu * Q).sum(1).sigmoid()
    # backward
    gz = (_t(gp) * p * (1.0 - p)).unsqueeze(1)
    g_zu = gz * Q
    g_qi = gz * zu
    g_beta = (g_zu * (su - P)).sum(1)
    g_su = b1 * g_zu
    g_pu = nb1 * g_zu
    g_bs = (g_beta * beta * (1.0 - beta)).unsqueeze(1)
    g_bp = -g_bs
    rs = xs.step()                                               # computed su . qi: the one ambiguous sign
    rp = EV((xp.v > 0).double())                                 # pu . qi: inputs
    gwd_rows = g_bs * xs.relu() + g_bp * xp.relu()
    g_su = g_su + g_bs * WD * rs * Q
    g_qi = g_qi + (g_bs * WD * rs * su + g_bp * WD * rp * P)
    g_pu = g_pu + g_bp * WD * rp * Q
    gatt = (g_su.unsqueeze(1) * H).sum(2)
    dot = (att * gatt).sum(1, keepdim=True)
    g_sc = att * (gatt - dot)
    g_bu = g_sc.sum(1)
    gs2 = g_sc.unsqueeze(2)
    gwu_rows = (gs2 * t).sum(1)
    g_pu = g_pu + (gs2 * WU * r_in * H).sum(1)
    gH = att.unsqueeze(2) * g_su.unsqueeze(1) + gs2 * WU * r_in * P1
    d = colsum_depth(B)
    out = dict(p=p, gHe=gH, gpu=g_pu, gqi=g_qi, gwu=gwu_rows.sum(0, depth=d).unsqueeze(0), gbu=g_bu.sum(0, depth=d).unsqueeze(0),
               gwd=gwd_rows.sum(0, depth=d).unsqueeze(0))
    return out, xs.ambiguous().any(1), float(torch.maximum(bs.v.abs().max(), bp.v.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------- DeepAPF

def _apf_cases():
    """(B, D) of ApfCombine: every D path of its lane loop (below, at and past one wave; several rounds) and a batch past wave_grid's cap."""
    return [(41, 1), (41, 64), (41, 65), (41, 200), (WAVE_ROWS + 1 + 4, 5)]


def _apf_inputs(B, D):
    gen = torch.Generator().manual_seed(B * 3 + D)
    r = lambda *s, k=1.0: torch.randn(*s, generator=gen) * k
    a, s, o, t, wp = r(2 * B, 1, k=1.5), r(B, D, k=0.7), r(B, D, k=0.7), r(B, D, k=0.7), r(1, D, k=1.0 / D ** 0.5)
    n_overlap = 20
    ids = torch.randint(1, 41, (B,), generator=gen)               # both sides of n_overlap ...
    ids[0], ids[1], ids[2] = n_overlap, n_overlap + 1, n_overlap - 1   # ... and the edge: id == n_overlap keeps its share row
    gp = r(B, k=0.8) + 0.3
    return a, s, o, t, wp, ids, n_overlap, gp


def apf_combine_fp64(a, s, o, t, wp, ids, n_overlap, gp):
    """apf_combine_kernel / apf_combine_bwd_kernel (cdr_rowmodels.hip:94-150)."""
    B, D = s.shape
    masked = ids > n_overlap
    A = _t(a.reshape(-1))
    big = torch.tensor(-1e31, dtype=torch.float32).double().to(a.device)
    a_s = ev_where(masked, EV(big.expand(B).clone()), A[:B])
    a_o = A[B:]
    m = a_s.maximum(a_o)
    es, eo = (a_s - m).exp(), (a_o - m).exp()
    al_s, al_o = es / (es + eo), eo / (es + eo)
    S, O, T, W = _t(s), _t(o), _t(t), _t(wp.reshape(-1))
    p = (W * ((al_s.unsqueeze(1) * S + al_o.unsqueeze(1) * O) * T)).sum(1).sigmoid()
    # backward: al_o = 1 - al_s from the stored alpha_s
    al1, ao1 = al_s.unsqueeze(1), (1.0 - al_s).unsqueeze(1)
    gz = (_t(gp) * p * (1.0 - p)).unsqueeze(1)
    ev = al1 * S + ao1 * O
    ge = gz * W * T
    gwp_rows, gt, gs, go = gz * ev * T, gz * W * ev, al1 * ge, ao1 * ge
    d_s, d_o = (ge * S).sum(1), (ge * O).sum(1)
    dot = al_s * d_s + (1.0 - al_s) * d_o
    ga = ev_cat([al_s * (d_s - dot), (1.0 - al_s) * (d_o - dot)]).unsqueeze(1)
    return dict(p=p, ga=ga, gs=gs, go=go, gt=gt, gwp=gwp_rows.sum(0, depth=colsum_depth(B)).unsqueeze(0)), masked, al_s


# ---------------------------------------------------------------------------------------------------------------------- DCDCSR

def _maxmin_cases():
    return [(41, 2), (41, 63), (41, 64), (41, 65), (41, 100), (41, 300), (WAVE_ROWS + 1 + 5, 2), (WAVE_ROWS + 1 + 5, 7)]


def _maxmin_inputs(n, D):
    gen = torch.Generator().manual_seed(n + D * 11)
    x = torch.randn(n, D, generator=gen)
    gy = torch.randn(n, D, generator=gen) * 0.8 + 0.2
    if D > 2:                                                    # exact ties, made by copying fp32 values
        rows = torch.arange(n)
        imax, imin = x.argmax(1), x.argmin(1)
        for k, (src, every) in enumerate(((imax, 3), (imin, 4), (imax, 5))):      # rows 0 mod 3: tied maxima; 0 mod 4: tied minima; 0 mod 5: three-way
            sel = rows[rows % every == 0]
            free = torch.tensor([[c for c in range(D) if c != int(imax[i]) and c != int(imin[i])][k % (D - 2)] for i in sel])
            x[sel, free] = x[sel, src[sel]]
    return x, gy


def maxmin_fp64(x, gy):
    """maxmin_fwd_kernel / maxmin_bwd_kernel (cdr_rowmodels.hip:152-198).  max / min / the tie counts are exact (input comparisons)."""
    X, G = _t(x), _t(gy)
    mx, mn = X.amax(1, keepdim=True), EV(x.double().amin(1, keepdim=True))
    ismax, ismin = (X.v == mx.v).double(), (X.v == mn.v).double()
    mean = (mx + mn).exact_scale(0.5)
    h = mx - mean
    y = (X - mean) / h
    Gs, Ss = G.sum(1, keepdim=True), (G * y).sum(1, keepdim=True)
    cmax = (Gs + Ss) / (h.exact_scale(2.0) * EV(ismax.sum(1, keepdim=True)))
    cmin = (Gs - Ss) / (h.exact_scale(2.0) * EV(ismin.sum(1, keepdim=True)))
    g = G / h
    g = ev_where(ismax.bool(), g - cmax, g)
    g = ev_where(ismin.bool(), g - cmin, g)
    return dict(y=y, stats=ev_cat([mean, mx], 1), gx=g), ismax.sum(1), ismin.sum(1)


# ---------------------------------------------------------------------------------------------------------------------- DTCDR

def _gmax_cases():
    """(n, D, table rows): a small odd case and one with n D past the elementwise grid cap, D odd (the second half's pointer is then
    only 4-byte aligned), ids duplicated many times."""
    return [(50, 7, 20), (8200, 65, 500)]


def _gmax_inputs(n, D, rows):
    gen = torch.Generator().manual_seed(n + D)
    tabs = [torch.randn(rows, D, generator=gen) for _ in range(4)]
    tie = torch.rand(rows, D, generator=gen) < 0.25
    tabs[1][tie] = tabs[0][tie]                                   # exact ties: the gradient splits 0.5 / 0.5
    tabs[3][~tie] = tabs[2][~tie]
    uid, iid = torch.randint(0, rows, (n,), generator=gen), torch.randint(0, rows, (n,), generator=gen)
    g = torch.randn(n, 2 * D, generator=gen)
    return tabs, uid, iid, g


def gmax_bwd_fp64(A, Bt, ids, g):
    """gather_max2_bwd_kernel (cdr_rowmodels.hip:50-67): per occurrence g (or g / 2, exact) added atomically: depth = occurrences."""
    a, b = A[ids].double(), Bt[ids].double()
    wa = (a > b).double() + 0.5 * (a == b).double()
    occ = torch.bincount(ids, minlength=A.shape[0]).double().unsqueeze(1)
    out = []
    for w in (wa, 1.0 - wa):
        G = torch.zeros_like(A, dtype=torch.float64).index_add_(0, ids, w * g.double())
        Ab = torch.zeros_like(G).index_add_(0, ids, (w * g.double()).abs())
        out.append(EV(G, occ * U32 / (1 - occ * U32) * Ab))
    return out


# ---------------------------------------------------------------------------------------------------------------------- losses

def _bce_inputs(n):
    gen = torch.Generator().manual_seed(n)
    p = torch.rand(n, generator=gen).clamp(1e-4, 1 - 1e-4)
    y = (torch.rand(n, generator=gen) < 0.4).float()
    edge = torch.tensor([0.0, 0.0, 1.0, 1.0, 2.0 ** -130, 2.0 ** -130, 1 - 2.0 ** -24, 1 - 2.0 ** -24, 2.0 ** -149, 1e-30])
    p[:edge.numel()] = edge
    y[:edge.numel()] = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 1.0])
    return p, y


def _logc(x):
    """max(logf(x), -100) of a computed x >= 0: K_LOG ulps of the logarithm + the argument's error through 1 / x; the clamp is
    1-Lipschitz and the reference's own rule (torch.nn.BCELoss)."""
    v = torch.log(x.v).clamp(min=-100.0)
    e = torch.where(v > -100.0, x.e / (x.v - x.e).clamp(min=1e-300) + K_LOG * U32 * v.abs(), torch.zeros_like(v))
    return EV(v, e)


def bce_fp64(p, y, go):
    """bce_partial_kernel + scalar_finish_kernel, bce_bwd_kernel (cdr_elem.hip:66-97): fp32 terms, fp64 partials (n 2^-53: nothing beside
    the terms' own bounds), one rounding of the mean to fp32."""
    n = p.numel()
    P, Y = _t(p), _t(y)
    term = (Y - 1.0) * _logc(1.0 - P) - Y * _logc(P)
    loss = EV(term.v.mean(), term.e.mean() + (U32 + n * 2.0 ** -53) * term.v.abs().mean())
    g0 = _t(go) / EV(torch.tensor(float(n), dtype=torch.float64, device=p.device))
    den = ((1.0 - P) * P).maximum(EV(torch.tensor(1e-12, dtype=torch.float32).double().to(p.device)))
    return loss, g0 * (P - Y) / den


def frob_fp64(w, go):
    """sqsum_partial_kernel + finish, frobenius_bwd_kernel (cdr_elem.hip:99-117): fp32 squares (u each) summed in fp64, sqrt in fp64
    (halves the relative error), one rounding to fp32: (u / 2 + u + n 2^-53) ||w||."""
    W = _t(w.reshape(-1))
    n = W.v.numel()
    v = W.v.square().sum().sqrt()
    norm = EV(v, (1.5 * U32 + n * 2.0 ** -53) * v)
    return norm, (_t(go) / norm) * W


# ---------------------------------------------------------------------------------------------------------------------- the table test

def test_case_table_covers_every_regime():
    nat = _natr_cases()
    J = lambda D: -(-D // 64)
    assert {(J(D), D % 64 == 0) for _b, _l, D in nat if _b == 37} == {(j, f) for j in (1, 2, 3, 4) for f in (True, False)}
    assert {D for _b, _l, D in nat} >= {1, 63, 64, 65, 100, 128, 129, 192, 193, 256} and {L for _b, L, _d in nat} >= {1, 2, 50, 255, 256}
    assert {J(D) for _b, L, D in nat if L >= MAX_HIST - 1} == {1, 2, 3, 4} and any(L == MAX_HIST and D == MAX_DIM for _b, L, D in nat)
    assert any(B > WAVE_ROWS for B, _l, _d in nat)
    for B, L, D in nat:
        inp = _natr_inputs(B, L, D)
        mask = inp[3]
        assert bool((mask.sum(1) == 0).any()) and bool((mask.sum(1) == L).any()) and (L == 1 or bool((mask.sum(1) == 1).any()))
        _ref, amb, logit = natr_fp64(*inp)
        assert logit < 20.0, (B, L, D, logit)                       # exp(b_s) is unstabilised in the reference and the kernel alike
        assert int(amb.sum()) <= AMB_CAP * B, (B, L, D, int(amb.sum()))
        assert all(bool(torch.isfinite(v.v).all() and torch.isfinite(v.e).all()) for v in _ref.values())
    apf = _apf_cases()
    assert {D for _b, D in apf} >= {1, 64, 65, 200} and any(B > WAVE_ROWS for B, _d in apf)
    for B, D in apf:
        *inp, gp = _apf_inputs(B, D)
        ids, n_ov = inp[5], inp[6]
        assert bool((ids > n_ov).any()) and bool((ids < n_ov).any()) and bool((ids == n_ov).any())
        ref, masked, al_s = apf_combine_fp64(*inp, gp)
        assert bool((al_s.v[masked] == 0).all()) and bool((ref['ga'].v[:B][masked] == 0).all())
    mm = _maxmin_cases()
    assert {D for _n, D in mm} >= {2, 63, 64, 65, 100, 300} and any(n > WAVE_ROWS for n, _d in mm)
    for n, D in mm:
        x, gy = _maxmin_inputs(n, D)
        _ref, nmax, nmin = maxmin_fp64(x, gy)
        if D > 2:
            assert bool((nmax > 1).any()) and bool((nmin > 1).any()) and bool(((nmax == 1) & (nmin == 1)).any())
        else:
            assert bool(((nmax == 1) & (nmin == 1)).all())
        assert bool(torch.isfinite(_ref['gx'].e).all())
    assert any(n * D > ELEM_CAP for n, D, _r in _gmax_cases()) and any(D % 4 for _n, D, _r in _gmax_cases())
    for n, D, rows in _gmax_cases():
        tabs, uid, iid, g = _gmax_inputs(n, D, rows)
        assert bool((tabs[0][uid] == tabs[1][uid]).any()) and bool((tabs[2][iid] == tabs[3][iid]).any())
        assert int(torch.bincount(uid).max()) > 1
    assert _prod_shape()[0] * _prod_shape()[1] > ELEM_CAP and _frob_n() > 2048 * 1024
    p, y = _bce_inputs(_bce_n())
    assert float(p.min()) == 0.0 and float(p.max()) == 1.0 and bool(((p > 0) & (p < 2.0 ** -126)).any()) and bool((p == 1 - 2.0 ** -24).any())


def _prod_shape():
    return 2100, 251                 # past 2,048 x 256 elements: apf_prod's grid-stride loop, a ragged last pass


def _frob_n():
    return 2048 * 1024 + 77          # partial_grid (cdr_elem.hip:446-452): 1,024 elements per workgroup, 2,048 workgroups


def _bce_n():
    return 5000


# ---------------------------------------------------------------------------------------------------------------------- GPU side

def _dev(*ts):
    return [t.to(DEV) for t in ts]


@pytest.mark.parametrize('B,L,D', _natr_cases())
def test_natr_attention_vs_fp64(B, L, D):
    from recbole_cdr_amd import functional as F_
    He, pu, qi, mask, wu, bu, wd, bd, gp = _dev(*_natr_inputs(B, L, D))
    leaves = [t.requires_grad_(True) for t in (He, pu, qi, wu, bu, wd, bd)]
    He, pu, qi, wu, bu, wd, bd = leaves
    p = F_.NatrAttention.apply(He, pu, qi, mask, wu, bu, wd, bd)
    p.backward(gp)
    torch.cuda.synchronize()
    ref, amb, _logit = natr_fp64(He.detach(), pu.detach(), qi.detach(), mask, wu.detach(), bu.detach(), wd.detach(), bd.detach(), gp)
    assert int(amb.sum()) <= AMB_CAP * B
    got = dict(p=p.detach(), gHe=He.grad, gpu=pu.grad, gqi=qi.grad, gwu=wu.grad, gbu=bu.grad, gwd=wd.grad)
    _record(f'NATR J={-(-D // 64)}' + (' grid-stride' if B > WAVE_ROWS else ''), {k: _ratio(ref[k], got[k]) for k in ref})
    # beta is invariant under a shift of both gate logits: the kernel forms g_bs + (-g_bs), exactly 0 in every row
    assert bool((bd.grad == 0).all())


@pytest.mark.parametrize('B,D', _apf_cases())
def test_apf_combine_vs_fp64(B, D):
    from recbole_cdr_amd import functional as F_
    a, s, o, t, wp, ids, n_ov, gp = _apf_inputs(B, D)
    a, s, o, t, wp, ids, gp = _dev(a, s, o, t, wp, ids, gp)
    leaves = [x.requires_grad_(True) for x in (a, s, o, t, wp)]
    p = F_.ApfCombine.apply(*leaves, ids, n_ov)
    p.backward(gp)
    torch.cuda.synchronize()
    ref, masked, _al = apf_combine_fp64(*[x.detach() for x in leaves], ids, n_ov, gp)
    got = dict(p=p.detach(), ga=a.grad, gs=s.grad, go=o.grad, gt=t.grad, gwp=wp.grad)
    _record('ApfCombine' + (' grid-stride' if B > WAVE_ROWS else ''), {k: _ratio(ref[k], got[k]) for k in ref})
    # masked rows: softmax weight of the share branch exactly 0, and exactly no gradient into its score or its row
    assert bool(masked.any()) and bool((a.grad[:B, 0][masked] == 0).all()) and bool((s.grad[masked] == 0).all())
    al = torch.empty(B, device=DEV)
    pp = torch.empty(B, device=DEV)
    from recbole_cdr_amd import binding as B_
    B_.call('cdr_apf_combine', B_.stream(), B_.f32(a.detach().reshape(-1)), B_.f32(s.detach()), B_.f32(o.detach()), B_.f32(t.detach()),
            B_.f32(wp.detach().reshape(-1)), B_.i64(ids), int(n_ov), B, D, B_.f32(pp), B_.f32(al))
    assert bool((al[masked] == 0).all()) and bool((al[~masked] > 0).all()) and torch.equal(pp, p.detach())


def test_apf_product_past_the_grid_cap_vs_fp64():
    from recbole_cdr_amd import functional as F_
    B, D = _prod_shape()
    gen = torch.Generator().manual_seed(B + D)
    s, o, t = (torch.randn(B, D, generator=gen).to(DEV).requires_grad_(True) for _ in range(3))
    gX = torch.randn(2 * B, D, generator=gen).to(DEV)
    X = F_.ApfProduct.apply(s, o, t)
    X.backward(gX)
    torch.cuda.synchronize()
    S, O, T, G0, G1 = _t(s.detach()), _t(o.detach()), _t(t.detach()), _t(gX[:B]), _t(gX[B:])
    ref = dict(X=ev_cat([S * T, O * T]), gs=G0 * T, go=G1 * T, gt=G0 * S + G1 * O)
    got = dict(X=X.detach(), gs=s.grad, go=o.grad, gt=t.grad)
    _record('ApfProduct', {k: _ratio(ref[k], got[k]) for k in ref})


@pytest.mark.parametrize('n,D', _maxmin_cases())
def test_maxmin_normalize_vs_fp64(n, D):
    from recbole_cdr_amd import functional as F_
    x, gy = _dev(*_maxmin_inputs(n, D))
    x.requires_grad_(True)
    y, stats = F_.MaxMinNormalize.apply(x)
    y.backward(gy)
    torch.cuda.synchronize()
    ref, _nmax, _nmin = maxmin_fp64(x.detach(), gy)
    _record('MaxMinNormalize' + (' grid-stride' if n > WAVE_ROWS else ''),
            dict(y=_ratio(ref['y'], y.detach()), stats=_ratio(ref['stats'], stats), gx=_ratio(ref['gx'], x.grad)))
    assert torch.equal(stats[:, 1], x.detach().amax(1))                       # the max is an input value
    if D == 2:                                                                # (a, b) -> (+1, -1) or (-1, +1), never the same sign
        xd = x.detach()
        assert bool((torch.sign(y.detach()[:, 0]) == torch.sign(xd[:, 0] - xd[:, 1])).all()) and bool((y.detach().prod(1) < 0).all())


@pytest.mark.parametrize('n,D,rows', _gmax_cases())
def test_gather_max_concat_vs_fp64(n, D, rows):
    from recbole_cdr_amd import functional as F_
    tabs, uid, iid, g = _gmax_inputs(n, D, rows)
    tabs, (uid, iid, g) = _dev(*tabs), _dev(uid, iid, g)
    want = torch.cat([torch.maximum(tabs[0][uid], tabs[1][uid]), torch.maximum(tabs[2][iid], tabs[3][iid])], 1)
    refs = gmax_bwd_fp64(tabs[0], tabs[1], uid, g[:, :D]) + gmax_bwd_fp64(tabs[2], tabs[3], iid, g[:, D:])
    subsets = [m for m in itertools.product((False, True), repeat=4) if any(m)] if n <= 100 else [(True, True, True, True), (True, False, False, True)]
    worst = {}
    for need in subsets:                                                      # every subset: gA or gB (or a whole call) left out
        leaves = [t.detach().clone().requires_grad_(f) for t, f in zip(tabs, need)]
        out = F_.GatherMaxConcat.apply(*leaves, uid, iid)
        assert torch.equal(out, want)                                         # a selection of input values: bit-exact, both ldo = 2D halves
        out.backward(g)
        for k, (leaf, f) in enumerate(zip(leaves, need)):
            assert (leaf.grad is not None) == f
            if f:
                worst[f'g{k}'] = max(worst.get(f'g{k}', 0.0), _ratio(refs[k], leaf.grad))
    torch.cuda.synchronize()
    _record('GatherMaxConcat', worst)


def test_bce_prob_loss_edges_vs_fp64():
    from recbole_cdr_amd import functional as F_
    p, y = _dev(*_bce_inputs(_bce_n()))
    go = torch.tensor(0.7, device=DEV)
    p.requires_grad_(True)
    loss = F_.BCEProbLoss.apply(p, y)
    (loss * go).backward()
    torch.cuda.synchronize()
    lref, gref = bce_fp64(p.detach(), y, go)
    _record('BCEProbLoss', dict(loss=_ratio(lref, loss.detach()), gp=_ratio(gref, p.grad)))
    want = torch.nn.functional.binary_cross_entropy(p.detach().double(), y.double())
    assert abs(float(lref.v) - float(want)) <= 1e-12 * float(want)            # the restatement is torch's own rule in float64
    assert float(lref.e) <= 16 * U32 * float(lref.v)                          # fp64 partials: a few ulps, whatever n


def test_frobenius_norm_past_the_grid_cap_vs_fp64():
    from recbole_cdr_amd import functional as F_
    n = _frob_n()
    gen = torch.Generator().manual_seed(n)
    w = (torch.randn(n, generator=gen) * 0.3).to(DEV).requires_grad_(True)
    go = torch.tensor(-1.3, device=DEV)
    norm = F_.FrobeniusNorm.apply(w)
    (norm * go).backward()
    torch.cuda.synchronize()
    nref, gref = frob_fp64(w.detach(), go)
    _record('FrobeniusNorm', dict(norm=_ratio(nref, norm.detach()), gw=_ratio(gref, w.grad)))


@pytest.mark.parametrize('L,D', [(3, MAX_DIM + 1), (MAX_HIST + 1, 8), (0, 8)])
def test_natr_refuses_sizes_past_its_limits(L, D):
    """D = 257, L = 257 and L = 0 are errors (cdr_rowmodels.hip:471, 486), and nothing is written."""
    from recbole_cdr_amd import binding as B_
    B = 5
    f = lambda *s: torch.full(s, SENTINEL, device=DEV)
    He, pu, qi, mask = torch.randn(B, max(L, 1), D, device=DEV), torch.randn(B, D, device=DEV), torch.randn(B, D, device=DEV), torch.ones(B, max(L, 1), device=DEV)
    wu, bu, wd, bd = torch.randn(D, device=DEV), torch.randn(1, device=DEV), torch.randn(D, device=DEV), torch.randn(1, device=DEV)
    att, su, beta, p = f(B, max(L, 1)), f(B, D), f(B), f(B)
    outs = [att, su, beta, p]
    with pytest.raises(RuntimeError, match='cdr_natr_att_fwd'):
        B_.call('cdr_natr_att_fwd', B_.stream(), B_.f32(He), B_.f32(pu), B_.f32(qi), B_.f32(mask), B_.f32(wu), B_.f32(bu), B_.f32(wd), B_.f32(bd),
                B, L, D, B_.f32(att), B_.f32(su), B_.f32(beta), B_.f32(p))
    gHe, gpu, gqi, rwu, rwd, rb = f(B, max(L, 1), D), f(B, D), f(B, D), f(B, D), f(B, D), f(B, 2)
    outs += [gHe, gpu, gqi, rwu, rwd, rb]
    with pytest.raises(RuntimeError, match='cdr_natr_att_bwd'):
        B_.call('cdr_natr_att_bwd', B_.stream(), B_.f32(He), B_.f32(pu), B_.f32(qi), B_.f32(mask), B_.f32(wu), B_.f32(bu), B_.f32(wd), B_.f32(bd),
                B, L, D, B_.f32(att), B_.f32(su), B_.f32(beta), B_.f32(p), B_.f32(torch.ones(B, device=DEV)),
                B_.f32(gHe), B_.f32(gpu), B_.f32(gqi), B_.f32(rwu), B_.f32(rwd), B_.f32(rb))
    torch.cuda.synchronize()
    sent = torch.tensor(SENTINEL).view(torch.int32).item()
    assert all(bool((o.view(torch.int32) == sent).all()) for o in outs)
