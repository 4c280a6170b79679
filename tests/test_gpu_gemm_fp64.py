"""The general fp32 contraction (cdr_gemm_f32_ex, csrc/cdr_gemm.hip: functional.gemm) in every regime its host code selects, the three
ways cdr_fullsort_scores_f32 reaches it, cdr_fullsort_neg_sqdist_f32's epilogue, and every route of functional.LinearAct, against a
float64 product of the same fp32 operands under PER-ELEMENT first-order bounds.

``gemm_regime`` restates launch<> (csrc/cdr_gemm.hip:176-213) and ``linear_routes`` LinearAct.forward / backward (functional.py:631-720);
``test_case_table_covers_every_regime`` (run without a GPU from test_fp64_bounds.py) asserts that the tables below hold every regime and
route and that no LinearAct case can pass through its ambiguous ReLU units.

Bounds (u = 2^-24, gamma_k = k u / (1 - k u); fp64_bounds.EV carries value and bound through the epilogue operation by operation):
  * accumulator: gamma_{depth + K_MFMA} (|op(A)| |op(B)|)[m, n]; depth = K for one chain, 256 + ceil(K / 256) when K is split into
    256-wide chunks whose partial products meet in atomic adds (any order: bound only, no bit-reproducibility);
  * epilogue: one rounding per operation of cdr_gemm.hip:159-171 -- rowscale product, the add of C (accumulate 2: before the
    activation, 1: behind it), the bias add, tanhf K_TANH ulps, 1 / (1 + expf(-v)) K_SIG ulps of p; ReLU is 1-Lipschitz (a forward
    ReLU is never ambiguous);
  * EPI_SQDIST: -(((-2 acc) + rown[m]) + coln[n]) with rown / coln = gamma_D sums of the fp32 rows' squares: every term's bound is
    on the scale of that term, so the bound of the (cancelling) result is absolute on the scale of the three;
  * LinearAct: y as above; gz = gy act'(y) from the kernel's own y (its bound rides along; a ReLU unit with |z| <= e_z is AMBIGUOUS:
    either branch, error 1 on the step); dx = gz W depth dout; dW / db by the route's real reduction depth (``wgrad_depth``).
Every C buffer has ldc > N and sentinel columns that must come back bit-unchanged."""
import pytest
import torch

from fp64_bounds import EV, U32, colsum_depth, gam
from helpers import DEV

pytestmark = pytest.mark.gpu

NONE, TANH, RELU, SIG = 0, 1, 2, 3              # binding.ACT_*
K_MFMA = 2      # the product's rounding + one for v_mfma_f32_32x32x2_f32 adding its two products in an order we do not assume
BK = 32
SENTINEL = -7.25e22
AMB_CAP = 0.005


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------- launch<> restated

def gemm_regime(M, N, K, lda, ldb, a_off, b_off, bias, act, accumulate, sq=False):
    """csrc/cdr_gemm.hip:180-196.  a_off / b_off: the operand's offset in floats from a 16-byte aligned address."""
    vecA = lda % 4 == 0 and a_off % 4 == 0                                                       # :181
    vecB = ldb % 4 == 0 and b_off % 4 == 0                                                       # :182
    small_m = M <= 64 or _cdiv(M, 128) * _cdiv(N, 128) < 192                                     # :184
    tiles = (_cdiv(M, 32) if small_m else _cdiv(M, 128)) * _cdiv(N, 128)                         # :185
    split = (not sq) and tiles < 64 and K >= 1024 and not bias and act == NONE and accumulate != 2   # :189
    k_chunk = 256 if split else K                                                                # :190
    return dict(tile=32 if small_m else 128, small_m=small_m, tiles=tiles, splits=_cdiv(K, k_chunk), k_chunk=k_chunk, vecA=vecA, vecB=vecB)


def gemm_depth(K, reg):
    return 256 + reg['splits'] if reg['splits'] > 1 else K


def _g(id, ta, tb, M, N, K, pa=0, pb=0, oa=0, ob=0, bias=False, act=NONE, acc=0, rs=False):
    """pa / pb: extra floats per operand row (lda = width + pa); oa / ob: one-float offsets into a larger buffer."""
    return dict(id=id, ta=ta, tb=tb, M=M, N=N, K=K, pa=pa, pb=pb, oa=oa, ob=ob, bias=bias, act=act, acc=acc, rs=rs)


def _lds(c):
    wa = c['M'] if c['ta'] else c['K']
    wb = c['K'] if c['tb'] else c['N']
    return wa + c['pa'], wb + c['pb']


def _regime(c):
    lda, ldb = _lds(c)
    return gemm_regime(c['M'], c['N'], c['K'], lda, ldb, c['oa'], c['ob'], c['bias'], c['act'], c['acc'])


FORMS = {'NT': (False, True), 'NN': (False, False), 'TN': (True, False), 'TT': (True, True)}


def _gemm_cases():
    cs = []
    for name, (ta, tb) in FORMS.items():
        # <32,128>: ragged in M (33 = 32 + 1), N (130 = 128 + 2), K (37 = 32 + 5); every operand a column slice (lda, ldb > width)
        # pads chosen so that every leading dimension is a multiple of 4: the float4 paths, with a ragged last float4 per row
        cs.append(_g(f't32-{name}', ta, tb, 33, 130, 37, pa=3, pb=3 if tb else 2))
        # <128,128>: the smallest grids that reach 192 tiles; K = 44 ends inside the second BK step, M and N ragged against 128
        cs.append(_g(f't128-{name}', ta, tb, 129, 12161, 44, pa=3 if ta else 4, pb=4 if tb else 3))
    cs += [
        _g('t128-NT-65', False, True, 65, 24449, 20),                                # one row past M <= 64
        _g('t128-NN-square', False, False, 1537, 1800, 64, bias=True, act=RELU),     # 13 x 15 tiles, a full last K step
        # scalar-load fall-backs: a leading dimension that is no multiple of 4, a pointer that is only 4-byte aligned
        _g('vecA0-ld', False, True, 40, 140, 36, pa=1),
        _g('vecB0-ld', False, True, 40, 140, 36, pb=2),
        _g('vecA0-ptr', False, True, 40, 140, 36, oa=1),
        _g('vecB0-ptr', False, False, 40, 140, 36, ob=1),
        _g('vec0-TN-ld', True, False, 37, 131, 33, pa=2, pb=2),
        _g('vec0-t128-ptr', True, False, 132, 12200, 33, oa=1, ob=1, pa=4, pb=4),
        # each activation with bias; the CoNet cross unit's second call (accumulate 2 + rowscale + bias + ReLU)
        _g('act-none-bias', False, True, 70, 129, 31, bias=True),
        _g('act-tanh-bias', False, True, 70, 129, 31, bias=True, act=TANH),
        _g('act-relu-bias', False, True, 70, 129, 31, bias=True, act=RELU),
        _g('act-sig-bias', False, True, 70, 129, 31, bias=True, act=SIG),
        _g('cross-unit', False, True, 70, 64, 128, bias=True, act=RELU, acc=2, rs=True),
        _g('cross-unit-t128', False, True, 129, 12161, 16, bias=True, act=RELU, acc=2, rs=True),
        _g('post-add', False, False, 45, 200, 50, acc=1, rs=True),
        # split K (K >= 1024, tiles < 64): a K that ends inside a 256-row chunk, accumulate 0 (the pitched memset) and 1, rowscale
        _g('split-TN-0', True, False, 100, 70, 1024 + 37, pa=4, pb=2, rs=True),
        _g('split-TN-1', True, False, 100, 70, 1024 + 37, acc=1, rs=True),
        _g('split-NT-0', False, True, 33, 128, 2100, pa=4),
        _g('split-NN-1', False, False, 128, 33, 1500, acc=1, ob=1),
        _g('split-TT-0', True, True, 64, 129, 1061, rs=True),
        _g('nosplit-acc2', False, True, 40, 64, 1100, acc=2, bias=True, act=RELU, rs=True),     # K >= 1024 yet one chain (:189)
    ]
    return cs


def _sq_cases():
    """(U, N, D): cdr_fullsort_neg_sqdist_f32 at both tiles, ragged everywhere."""
    return [(33, 301, 37), (65, 24449, 16), (129, 12161, 50)]


def _fullsort_cases():
    """(id, U, N, D, user offset, item offset): the three ways cdr_fullsort_scores_f32 reaches launch<> (:1070-1090, :1028-1031)."""
    return [('unaligned-users', 9, 300, 20, 1, 0), ('unaligned-items-t128', 65, 24449, 64, 0, 1),
            ('odd-D-many-users-t128', 129, 12161, 32, 0, 0), ('odd-D-many-users-t32', 70, 1000, 36, 0, 0),
            ('persistent-tail', 129, 64 * 5 + 37, 64, 0, 0)]


def fullsort_route(U, N, D, uo, io):
    """Which kernel scores a slab (gemv_ok :280, score_persistent_ok :1006) and, for the generic one, (M, N) of its launch<> call."""
    aligned = uo % 4 == 0 and io % 4 == 0
    if U <= 8 and D % 4 == 0 and 16 <= D <= 256 and aligned:
        return 'gemv', None
    if U > 32 and D in (64, 128) and N >= 64 and aligned:
        return ('persistent+tail', (U, N % 64)) if N % 64 else ('persistent', None)
    return 'generic', (U, N)


# ---------------------------------------------------------------------------------------------------------------------- LinearAct restated

def wgrad_split(rows):
    """csrc/cdr_linear.hip:232-237."""
    n = min(_cdiv(rows, 512), 64)
    chunk = (_cdiv(rows, n) + 1) & ~1
    return chunk, _cdiv(rows, chunk)


def linear_routes(rows, dout, din, aligned, act, bias):
    """(forward, dx, dW / db) of functional.LinearAct for a contiguous x (``aligned``: 16-byte aligned) and contiguous weights."""
    fits = _cdiv(dout, 32) * _cdiv(din, 32) <= 1024                                              # _wgrad_tiles_fit :620
    fwd = 'linear_small' if rows <= 16384 and din % 4 == 0 and aligned else 'gemm'               # _small_linear :625
    if rows <= 16384:                                                                            # :656
        dx = 'linear_small' if dout % 4 == 0 else 'act_bwd+gemm'                                 # :660-672
        dw = 'wgrad_small' if fits else 'act_bwd+gemm_tn+colsum'                                 # :674-692
    else:
        dx = 'act_bwd+gemm'                                                                      # :696-703
        dw = 'wgrad_chunked' if rows <= (1 << 18) and fits else 'gemm_tn_splitk+colsum'          # :704-719
    return fwd, dx, dw


def wgrad_depth(rows, dout, din, route):
    """(dW depth, db depth): the longest chain of additions a term of the sum over ``rows`` goes through.
      wgrad_small / wgrad_chunked (cdr_linear.hip:41-43, 67-73, 97-99, 143-145): a wave's MFMA chain over its ``per`` rows of the
        workgroup's chunk, the eight waves in order, then the nz chunks in order; db the same with half the rows per lane + one shuffle;
      gemm_tn (cdr_gemm.hip:189-191): K = rows in one chain, or 256-row chunks + one atomic per chunk from K = 1024 on;
      colsum: fp64_bounds.colsum_depth."""
    if route in ('wgrad_small', 'wgrad_chunked'):
        chunk, nz = wgrad_split(rows)
        per = (_cdiv(min(chunk, rows), 8) + 1) & ~1
        d = per + 8 + nz + K_MFMA
        return d, d
    M, N = dout, din
    reg = gemm_regime(M, N, rows, dout, din, 0, 0, False, NONE, 0)
    return gemm_depth(rows, reg) + K_MFMA, colsum_depth(rows)


def _linear_cases():
    """(id, rows, dout, din, x offset, act, bias): the smallest shapes that select each route."""
    return [('small', 300, 64, 32, 0, TANH, True),
            ('dout%4', 130, 30, 32, 0, TANH, True),                       # dx = cdr_act_bwd + gemm(gz, W)
            ('din%4', 130, 32, 30, 0, RELU, True),                        # forward on the general contraction
            ('x-offset', 77, 16, 24, 1, SIG, True),                       # x a one-float-offset view: forward gemm with scalar loads
            ('tiles>1024', 64, 1056, 1024, 0, TANH, True),                # 33 x 32 = 1,056 tiles: cdr_act_bwd + TN gemm + cdr_colsum
            ('rows=16385', 16385, 8, 12, 0, SIG, True),                   # chunked dW, dx on the general contraction
            ('rows=2^18', 1 << 18, 12, 8, 0, RELU, True),                 # the chunked route's last row count (64 chunks)
            ('rows=2^18+1', (1 << 18) + 1, 8, 8, 0, TANH, True),          # TN gemm with split-K atomics, cdr_colsum db
            ('no-bias-none', 500, 20, 36, 0, NONE, False)]


def _linear_inputs(case):
    _id, rows, dout, din, xo, act, bias = case
    gen = torch.Generator().manual_seed(rows * 31 + dout * 7 + din)
    xbuf = torch.randn(rows * din + xo, generator=gen)
    W = torch.randn(dout, din, generator=gen) * (1.0 / din ** 0.5)
    b = torch.randn(dout, generator=gen) * 0.3 if bias else None
    gy = torch.randn(rows, dout, generator=gen) * 0.7 + 0.1
    return xbuf, W, b, gy


def linear_fp64(case, x, W, b, gy, y_dev=None):
    """y, dx, dW, db as EV pairs, and the rows with an ambiguous ReLU unit.  x, W, b, gy: fp32 tensors (any device)."""
    _id, rows, dout, din, xo, act, bias = case
    fwd, dxr, dwr = linear_routes(rows, dout, din, xo % 4 == 0, act, bias)
    X, Wd, G = EV(x.double()), EV(W.double()), EV(gy.double())
    z = X.matmul(EV(W.double().t().contiguous()), din, extra=K_MFMA)
    if b is not None:
        z = z + EV(b.double())
    y = {NONE: lambda t: t, TANH: EV.tanh, RELU: EV.relu, SIG: EV.sigmoid}[act](z)
    amb = torch.zeros(rows, dtype=torch.bool, device=x.device)
    if act == NONE:
        gz = G
    elif act == TANH:
        gz = G * (1.0 - y * y)
    elif act == SIG:
        gz = G * (y * (1.0 - y))
    else:
        gz = G * z.step()
        amb = z.ambiguous().any(1)
    dx = gz.matmul(Wd, dout, extra=K_MFMA)
    ddw, ddb = wgrad_depth(rows, dout, din, {'wgrad_small': 'wgrad_small', 'wgrad_chunked': 'wgrad_chunked'}.get(dwr, 'gemm_tn'))
    gzt = EV(gz.v.t().contiguous(), gz.e.t().contiguous())
    dW = gzt.matmul(X, ddw, extra=0)
    db = gz.sum(0, depth=ddb) if b is not None else None
    return y, dx, dW, db, amb


# ---------------------------------------------------------------------------------------------------------------------- the table test

def test_case_table_covers_every_regime():
    cs = _gemm_cases()
    regs = {c['id']: _regime(c) for c in cs}
    form = lambda c: next(k for k, v in FORMS.items() if v == (c['ta'], c['tb']))
    assert {(regs[c['id']]['tile'], form(c)) for c in cs} >= {(t, f) for t in (32, 128) for f in FORMS}
    vec = {(regs[c['id']]['tile'], form(c)) for c in cs if regs[c['id']]['vecA'] and regs[c['id']]['vecB']}
    assert vec >= {(t, f) for t in (32, 128) for f in FORMS}, vec                      # ... each also on the float4 loads
    sq = {gemm_regime(U, N, D, D, D, 0, 0, False, NONE, 0, sq=True)['tile'] for U, N, D in _sq_cases()}
    assert sq == {32, 128}
    split = [c for c in cs if regs[c['id']]['splits'] > 1]
    assert {c['acc'] for c in split} == {0, 1} and all(regs[c['id']]['small_m'] for c in split)
    # the 128-row tile needs >= 192 tiles, split K < 64: unreachable there, so both accumulate values at small_m is all there is
    assert all(gemm_regime(M, N, 4096, M, N, 0, 0, False, NONE, 0)['splits'] == 1 for M, N in ((129, 12161), (65, 24449), (1537, 1800)))
    assert any(c['rs'] for c in split) and {form(c) for c in split} == set(FORMS)
    assert any(_lds(c)[0] > (c['M'] if c['ta'] else c['K']) and c['acc'] == 0 for c in split)          # and ldc > N: every case
    assert any((c['K'] % 256) not in (0,) and c['K'] > 1024 and (c['K'] % BK) for c in split)          # K ends inside a chunk and a BK step
    assert any(c['acc'] == 2 and c['rs'] and c['bias'] and c['act'] == RELU for c in cs)
    assert any(c['acc'] == 2 and c['K'] >= 1024 and regs[c['id']]['splits'] == 1 for c in cs)
    assert {c['act'] for c in cs if c['bias']} == {NONE, TANH, RELU, SIG}
    for op, ld, off in (('vecA', 'pa', 'oa'), ('vecB', 'pb', 'ob')):
        zero, i = [c for c in cs if not regs[c['id']][op]], int(op == 'vecB')
        assert any(_lds(c)[i] % 4 and not c[off] for c in zero) and any(c[off] and _lds(c)[i] % 4 == 0 for c in zero), op
    assert any(not regs[c['id']]['vecA'] and regs[c['id']]['tile'] == 128 for c in cs)
    assert any(c['pa'] and c['pb'] for c in cs)
    assert any(c['M'] % 32 and c['N'] % 128 and c['K'] % BK for c in cs if regs[c['id']]['tile'] == 32)
    assert any(c['M'] % 128 and c['N'] % 128 and c['K'] % BK for c in cs if regs[c['id']]['tile'] == 128)
    assert regs['t128-NT-65']['tile'] == 128 and gemm_regime(64, 24449, 20, 20, 20, 0, 0, False, NONE, 0)['tile'] == 32
    assert gemm_regime(129, 12160, 44, 44, 44, 0, 0, False, NONE, 0)['tile'] == 32                     # 95 x 2 = 190 tiles: one short
    # the three ways the full-sort entry reaches launch<>, and the tile each selects
    seen = {}
    for id, U, N, D, uo, io in _fullsort_cases():
        route, mn = fullsort_route(U, N, D, uo, io)
        assert mn is not None, id
        seen.setdefault((route, (uo or io) != 0), set()).add(gemm_regime(mn[0], mn[1], D, D, D, uo, io, False, NONE, 0)['tile'])
    assert seen[('generic', True)] == {32, 128} and seen[('generic', False)] == {32, 128} and seen[('persistent+tail', False)] == {32}
    # LinearAct: every route, and no case that could pass through its ambiguous units
    routes = [linear_routes(rows, dout, din, xo % 4 == 0, act, bias) for _id, rows, dout, din, xo, act, bias in _linear_cases()]
    assert {r[0] for r in routes} == {'linear_small', 'gemm'} and {r[1] for r in routes} == {'linear_small', 'act_bwd+gemm'}
    assert {r[2] for r in routes} == {'wgrad_small', 'act_bwd+gemm_tn+colsum', 'wgrad_chunked', 'gemm_tn_splitk+colsum'}
    assert linear_routes(130, 30, 32, True, TANH, True) == ('linear_small', 'act_bwd+gemm', 'wgrad_small')
    assert linear_routes(77, 16, 24, False, SIG, True)[0] == 'gemm' and linear_routes(130, 32, 30, True, RELU, True)[0] == 'gemm'
    assert linear_routes(16384, 8, 12, True, SIG, True)[2] == 'wgrad_small' and wgrad_split(1 << 18) == (4096, 64)
    assert gemm_regime(8, 8, (1 << 18) + 1, 8, 8, 0, 0, False, NONE, 0)['splits'] == 1025
    for case in _linear_cases():
        xbuf, W, b, gy = _linear_inputs(case)
        _id, rows, dout, din, xo, act, bias = case
        *_r, amb = linear_fp64(case, xbuf[xo:].view(rows, din), W, b, gy)
        assert int(amb.sum()) <= AMB_CAP * rows, (_id, int(amb.sum()), rows)


# ---------------------------------------------------------------------------------------------------------------------- GPU side

def _operand(shape, pad, off, gen, scale=1.0):
    """A [r, c] fp32 operand on the device with leading dimension c + pad, ``off`` floats into a buffer of its own."""
    r, c = shape
    ld = c + pad
    buf = torch.full((r * ld + off + 4,), float('nan'))
    full = buf[off:off + r * ld].view(r, ld)
    full[:, :c] = torch.randn(r, c, generator=gen) * scale + 0.05
    dbuf = buf.to(DEV)
    view = dbuf[off:off + r * ld].view(r, ld)[:, :c]
    assert dbuf.data_ptr() % 16 == 0 and (view.data_ptr() % 16 == 0) == (off % 4 == 0)
    return view


def _c_buffer(M, N, gen, init):
    """[M, N + 5] filled with the sentinel; the logical C is its first N columns (ldc = N + 5)."""
    buf = torch.full((M, N + 5), SENTINEL)
    if init:
        buf[:, :N] = torch.randn(M, N, generator=gen) * 0.5
    return buf.to(DEV)


def _sentinels_intact(buf, N):
    return bool((buf[:, N:].contiguous().view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32).item()).all())


def _epilogue(c, acc, C0, bias, rs, reg, absprod):
    if reg['splits'] > 1:
        # cdr_gemm.hip:163-164: every chunk's partial (scaled by rowscale: one more rounding each) is added atomically to C (zeroed or
        # as given): a chain of 256 + splits additions plus the given C's, in any order, over the terms' magnitudes
        k = 256 + reg['splits'] + K_MFMA + int(c['rs']) + int(c['acc'] == 1)
        scale = rs.double().abs().unsqueeze(1) if c['rs'] else 1.0
        v = acc.v * (rs.double().unsqueeze(1) if c['rs'] else 1.0) + (C0.double() if c['acc'] == 1 else 0.0)
        return EV(v, gam(k) * (absprod * scale + (C0.double().abs() if c['acc'] == 1 else 0.0)))
    v = acc * EV(rs.double().unsqueeze(1)) if c['rs'] else acc
    fn = {NONE: lambda t: t, TANH: EV.tanh, RELU: EV.relu, SIG: EV.sigmoid}[c['act']]
    if c['acc'] == 2:
        v = EV(C0.double()) + v
        return fn(v + EV(bias.double())) if c['bias'] else fn(v)
    v = fn(v + EV(bias.double())) if c['bias'] else fn(v)
    return v + EV(C0.double()) if c['acc'] == 1 else v


_worst = {}


def _record(family, r):
    _worst[family] = max(_worst.get(family, 0.0), r)
    print(f'\n[{family}] worst error / bound = {r:.3f} (family so far {_worst[family]:.3f})')


@pytest.mark.parametrize('c', _gemm_cases(), ids=lambda c: c['id'])
def test_gemm_regimes_vs_fp64(c):
    from recbole_cdr_amd import functional as F_
    gen = torch.Generator().manual_seed(c['M'] * 7 + c['N'] * 3 + c['K'] + 2 * c['ta'] + c['tb'])
    M, N, K = c['M'], c['N'], c['K']
    A = _operand((K, M) if c['ta'] else (M, K), c['pa'], c['oa'], gen)
    Bm = _operand((N, K) if c['tb'] else (K, N), c['pb'], c['ob'], gen, scale=0.5)
    bias = (torch.randn(N, generator=gen) * 0.5).to(DEV) if c['bias'] else None
    rs = (torch.rand(M, generator=gen) + 0.25).to(DEV) if c['rs'] else None
    if c['rs'] and c['acc'] == 2:
        rs[::3] = 0.0                                           # the cross unit's mask: 0 / 1 rows
        rs[1::3] = 1.0
    cbuf = _c_buffer(M, N, gen, c['acc'] != 0)
    C0 = cbuf[:, :N].clone()
    reg = _regime(c)
    assert (A.stride(0), Bm.stride(0)) == _lds(c) and cbuf.stride(0) == N + 5
    F_.gemm(A, Bm, trans_a=c['ta'], trans_b=c['tb'], bias=bias, act=c['act'], out=cbuf[:, :N], accumulate=c['acc'], rowscale=rs)
    torch.cuda.synchronize()
    assert _sentinels_intact(cbuf, N), f'{c["id"]}: columns past N of the C buffer were written'
    opA = EV((A.t() if c['ta'] else A).double().contiguous())
    opB = EV((Bm.t() if c['tb'] else Bm).double().contiguous())
    acc = opA.matmul(opB, gemm_depth(K, reg), extra=K_MFMA)
    ref = _epilogue(c, acc, C0, bias, rs, reg, opA.v.abs() @ opB.v.abs())
    got = cbuf[:, :N]
    assert bool(torch.isfinite(got).all())
    r = ref.ratio(got)
    worst = float(r.max())
    _record(f'gemm tile {reg["tile"]}' + (' split-K' if reg['splits'] > 1 else ''), worst)
    j = int(r.argmax())
    assert worst <= 1.0, (f'{c["id"]} {reg}: error / bound = {worst:.3g} at ({j // N}, {j % N}): got {float(got[j // N, j % N])!r} '
                          f'want {float(ref.v[j // N, j % N])!r}')


def _unit_rows(n, D, gen):
    """Rows as sqnorm_normalize leaves them: squared norm <= 1 (some well inside)."""
    x = torch.randn(n, D, generator=gen)
    x = x / x.norm(dim=1, keepdim=True) * torch.rand(n, 1, generator=gen).clamp(min=0.05).sqrt()
    return x


@pytest.mark.parametrize('U,N,D', _sq_cases())
def test_neg_sqdist_epilogue_vs_fp64(U, N, D):
    """cdr_fullsort_neg_sqdist_f32 (SSCDR's evaluation, sscdr.py:253-259): -(|u|^2 - 2 u.v + |v|^2), which cancels for near rows."""
    from recbole_cdr_amd import binding as B_
    gen = torch.Generator().manual_seed(U + N + D)
    ue, it = _unit_rows(U, D, gen), _unit_rows(N, D, gen)
    it[: min(U, N)] = ue[: min(U, N)] * (1 - 2.0 ** -12)                      # near-coincident pairs: the result is ~1e-7 of its terms
    ue, it = ue.to(DEV), it.to(DEV)
    buf = torch.full((U * N + 16,), SENTINEL, device=DEV)
    out = buf[8:8 + U * N].view(U, N)
    scratch = torch.full((U + N + 8,), SENTINEL, device=DEV)
    B_.call('cdr_fullsort_neg_sqdist_f32', B_.stream(), B_.f32(ue), U, D, B_.f32(it), N, B_.f32(scratch), B_.f32(out))
    torch.cuda.synchronize()
    sent = torch.tensor(SENTINEL).view(torch.int32).item()
    assert bool((buf[:8].view(torch.int32) == sent).all()) and bool((buf[8 + U * N:].view(torch.int32) == sent).all())
    assert bool((scratch[U + N:].view(torch.int32) == sent).all())
    reg = gemm_regime(U, N, D, D, D, 0, 0, False, NONE, 0, sq=True)
    eu, ei = EV(ue.double()), EV(it.double())
    rown, coln = (eu * eu).sum(1), (ei * ei).sum(1)
    acc = eu.matmul(EV(it.double().t().contiguous()), D, extra=K_MFMA)
    ref = -((acc.exact_scale(-2.0) + rown.unsqueeze(1)) + coln.unsqueeze(0))
    r = ref.ratio(out)
    worst = float(r.max())
    _record(f'neg_sqdist tile {reg["tile"]}', worst)
    assert worst <= 1.0, (U, N, D, reg, worst)
    # absolute on the scale of the three terms: a bound of a few ulps of the (tiny) result would be wrong here
    assert bool((ref.e >= U32 * (rown.v.unsqueeze(1) + coln.v.unsqueeze(0))).all())


@pytest.mark.parametrize('id,U,N,D,uo,io', _fullsort_cases(), ids=[c[0] for c in _fullsort_cases()])
def test_fullsort_routes_into_gemm_vs_fp64(id, U, N, D, uo, io):
    from recbole_cdr_amd import functional as F_
    gen = torch.Generator().manual_seed(U * 3 + N + D)
    ue = _operand((U, D), 0, uo, gen)
    it = _operand((N, D), 0, io, gen, scale=0.5)
    assert ue.is_contiguous() and it.is_contiguous()
    buf = torch.full((U * N + 16,), SENTINEL, device=DEV)
    out = buf[8:8 + U * N].view(U, N)
    F_.fullsort_scores(ue, it, out=out)
    torch.cuda.synchronize()
    sent = torch.tensor(SENTINEL).view(torch.int32).item()
    assert bool((buf[:8].view(torch.int32) == sent).all()) and bool((buf[8 + U * N:].view(torch.int32) == sent).all())
    ref = EV(ue.double()).matmul(EV(it.double().t().contiguous()), D, extra=K_MFMA)
    r = ref.ratio(out)
    worst = float(r.max())
    _record('fullsort -> gemm', worst)
    assert worst <= 1.0, (id, fullsort_route(U, N, D, uo, io), worst)


@pytest.mark.parametrize('case', _linear_cases(), ids=[c[0] for c in _linear_cases()])
def test_linear_act_routes_vs_fp64(case):
    from recbole_cdr_amd import functional as F_
    _id, rows, dout, din, xo, act, bias = case
    routes = linear_routes(rows, dout, din, xo % 4 == 0, act, bias)
    xbuf, W, b, gy = _linear_inputs(case)
    xdev = xbuf.to(DEV)
    gyd = gy.to(DEV)
    outs = []
    for _ in range(2):
        x = xdev[xo:].view(rows, din).detach().requires_grad_(True)
        assert (x.data_ptr() % 16 == 0) == (xo % 4 == 0)
        Wd = W.to(DEV).requires_grad_(True)
        bd = b.to(DEV).requires_grad_(True) if bias else None
        y = F_.linear(x, Wd, bd, act)
        y.backward(gyd)
        outs.append((y.detach(), x.grad, Wd.grad, None if bd is None else bd.grad))
    torch.cuda.synchronize()
    yr, dxr, dWr, dbr, amb = linear_fp64(case, xdev[xo:].view(rows, din), W.to(DEV), None if b is None else b.to(DEV), gyd)
    assert int(amb.sum()) <= AMB_CAP * rows
    keep = ~amb
    worst = {}
    for name, got, ref, rowwise in (('y', outs[0][0], yr, True), ('dx', outs[0][1], dxr, True), ('dW', outs[0][2], dWr, False),
                                    ('db', outs[0][3], dbr, False)):
        if ref is None:
            assert got is None
            continue
        assert got.shape == ref.v.shape and bool(torch.isfinite(got).all()), name
        r = ref.ratio(got)
        if rowwise:
            r = r[keep]
        worst[name] = float(r.max())
    _record(f'LinearAct {routes[2]}', max(worst.values()))
    print(f'{_id} {routes}: ambiguous rows {int(amb.sum())}, error / bound {worst}')
    assert max(worst.values()) <= 1.0, (_id, routes, worst)
    fixed = ['y', 'dx'] + ([] if routes[2] == 'gemm_tn_splitk+colsum' else ['dW']) + ['db']
    for name, a, b2 in zip(('y', 'dx', 'dW', 'db'), outs[0], outs[1]):
        if name in fixed and a is not None:
            assert torch.equal(a, b2), f'{_id}: {name} differs between two runs on a fixed-order route'
