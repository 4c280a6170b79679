"""The dense drop-in loss kernels (csrc/cdr_gather_loss.hip: cdr_bpr_fwd, cdr_point_fwd, cdr_point_fwd_pair and their dense backward
cdr_bpr_bwd_dense, cdr_point_bwd_dense(_pair); csrc/cdr_ordered.hip cdr_ordered_bwd under set_deterministic) against a float64
restatement in plain torch, at the batch sizes of the C1 / C2 benchmark legs and on both sides of every point where the host code
changes the launch:

  * forward units (units_for, cdr_gather_loss.hip:501-507): a lane group takes 1 interaction while B <= 128 * (256 / lpr), then
    2..4 (BPR) or 2..8 (pointwise) -- the grid stays at 128 workgroups up to 4x / 8x that size;
  * finishing pass: inside the forward launch while grid <= kSignInMaxBlocks = 512 (cdr_common.h:208; the pair kernel: 2 * grid <= 512),
    a launch of its own above;
  * grid cap: grid_for (cdr_common.h:262-268) stops at 2,048 workgroups, the kernels grid-stride beyond: only there do the
    tc = t < B ? t : B - 1 clamp and the t < B guards of the unrolled loop meet a ragged tail;
  * backward form: lane groups for D < 64, a wave per interaction from D = 64 and for D % 4 != 0; its own grid cap past 8,192;
  * gradient zero-fill: cdr_scrub clears the dense gradient buffer as a side job of the forward launch (BPR, pair), strided over
    whatever grid the forward has; a plain fill on the scalar path.

``fwd_launch`` below restates units_for / grid_for; ``test_case_table_covers_every_launch_regime`` asserts that the case table holds
every regime for each forward kernel, so a later change of those constants fails instead of un-testing a branch.

Every case checks: the total, the main loss and the two Frobenius norms (out4[0..3]) to LOSS_RTOL = 1e-5 of the fp64 value; every
per-occurrence coefficient gcoef[t] within delta_t; EVERY element of EVERY row of each dense gradient -- the batch's rows within the
first-order bound fp64_bounds._grad_bound (it does not depend on the order of the adds: the atomic and the ordered route are held to
the same figure), all other rows +0.0 bit for bit.  Just before the forward a NaN-filled tensor of the gradient buffer's size is
allocated and freed, so the caching allocator most likely hands that memory to the gradient buffer: a zero-fill that stops short shows.
The upstream gradient is 1.7.  Constants of the bounds: fp64_bounds.py (K_COEF, K_REG, K_SUM, K_ADAM) and test_gpu_step_fp64.py's
docstring; the dense path's additions (upstream factor, pair weights, separate reg tables) are counted in fp64_bounds.py.

Step level: CMF (C1: D = 64, alpha 0.5, 2 x 2,048 rows) and EMCDR (C2: BPR and MF, D = 64, reg 0.01, B = 2,048, SOURCE and TARGET) on
the benchmark's id space, three eager steps calculate_loss -> backward -> trainer.DenseAdam.step, each judged from the device's own
fp32 parameters and moments before it (teacher forcing) over ALL rows of each table (G = 0 on rows outside the batch: the idle decay
of m and v, and at update 1 the bit-exact preservation of untouched rows); parameters without a gradient keep their bits."""
import pytest
import torch

from fp64_bounds import (GAMMA, apply_fp64, bpr_grads_fp64, check_dense_result, check_scalar, f32, pair_grads_fp64, point_grads_fp64)
from helpers import DEV, FakeDataset, base_config
from test_gpu_step_fp64 import _check_table, _fmt

pytestmark = pytest.mark.gpu

GO = 1.7                                     # upstream gradient handed to backward()

# ---------------------------------------------------------------------------------------------------------------------- launch geometry
K_BLOCK = 256                                # cdr_gather_loss.hip:13
UNROLL = {'bpr': 4, 'point': 8}              # kUnroll, kUnrollPoint (cdr_gather_loss.hip:14-15)
K_SMALL_GRID = 128                           # cdr_gather_loss.hip:501
K_SIGN_IN_MAX = 512                          # cdr_common.h:208
K_GRID_CAP = 2048                            # grid_for: CDR_NUM_CU * 8 (cdr_common.h:264)
REGIMES = ('grid<128', 'grid=128,1 unit', 'grid=128,max units', '128<grid<=finish-in-kernel', 'separate finish launch', 'capped+tail')


def lpr_for(D):
    """cdr_lpr_for (cdr_common.h:244-248)."""
    q, l = (D + 3) // 4, 1
    while l < q and l < 64:
        l <<= 1
    return l


def fwd_launch(kind, D, B):
    """(interactions per lane group per trip u, grid, whether grid_for capped it, groups per block, unroll) of the forward launch
    (cdr_bpr_fwd / cdr_point_fwd(_pair): cdr_gather_loss.hip:523-534, 585-603, 647-650; units_for :502-507; grid_for cdr_common.h:262)."""
    unroll = UNROLL['bpr' if kind == 'bpr' else 'point']
    if D % 4:
        per, u, units, unroll = K_BLOCK // 64, 1, B, 1          # scalar kernels: one wave per interaction, no unroll
    else:
        per = K_BLOCK // lpr_for(D)
        u = min(max(-(-B // (K_SMALL_GRID * per)), 1), unroll)
        units = -(-B // u)
    raw = max(-(-units // per), 1)
    return u, min(raw, K_GRID_CAP), raw > K_GRID_CAP, per, unroll


def regime(kind, D, B, sign_in_max=K_SIGN_IN_MAX):
    u, grid, capped, per, unroll = fwd_launch(kind, D, B)
    if capped:
        return REGIMES[5]
    if grid < K_SMALL_GRID:
        return REGIMES[0]
    if grid == K_SMALL_GRID:
        return REGIMES[1] if u == 1 else (REGIMES[2] if u == unroll else 'grid=128,some units')
    return REGIMES[3] if grid <= sign_in_max else REGIMES[4]


def edges(kind, D):
    """The last B of: 1 unit at grid 128; max units at grid 128; the in-kernel finish (grid 512); the uncapped grid (2,048)."""
    _, _, _, per, unroll = fwd_launch(kind, D, 1)
    return K_SMALL_GRID * per, K_SMALL_GRID * per * unroll, K_SIGN_IN_MAX * per * unroll, K_GRID_CAP * per * unroll


def is_ragged_tail(kind, D, B):
    """B at least one past the cap and not a multiple of groups-per-block x unroll."""
    _, _, capped, per, unroll = fwd_launch(kind, D, B)
    return capped and B >= edges(kind, D)[3] + 1 and B % (per * unroll) != 0


# ---------------------------------------------------------------------------------------------------------------------- the case table
TABLES = {'a': (6984, 3945),                 # the C1 / C2 id space of bench.py (ml-1m -> ml-100k union)
          'b': (300000, 200000)}             # most rows once; gradient buffers far larger than one pass of a 128-block grid


def _kernel_cases():
    """(kind, D, B, table, reg, separate reg tables, deterministic)"""
    out = []
    for D in (64, 128):
        for kind in ('bpr', 'mse', 'bce'):
            e1, emax, e512, ecap = edges(kind, D)
            Bs = [e1 // 2 + 7, e1, e1 + 1, emax, emax + 1, e512, e512 + 1, ecap, ecap + 1]
            for j, B in enumerate(Bs):
                if D == 64:
                    out.append((kind, D, B, 'a', 0.01 if j % 2 == 0 else 0.0, False, False))
                    if B in (e1, emax, e512 + 1, ecap + 1):
                        out.append((kind, D, B, 'b', 0.01, False, False))
                elif kind == 'bpr' or (kind == 'mse') == (j % 2 == 0):
                    out.append((kind, D, B, 'b', 0.01 if j % 2 else 0.0, False, False))
                    if B in (e1, ecap + 1):
                        out.append((kind, D, B, 'a', 0.01, False, False))
    # narrow (lane-group backward), chunked (D4 > LPR) and odd (scalar kernels, two-launch finish, plain-fill zeroing) widths: one small
    # and one past-the-cap B each
    for D in (32, 260, 50):
        for kind in ('bpr', 'mse', 'bce'):
            out.append((kind, D, 777, 'a', 0.01, False, False))
            out.append((kind, D, edges(kind, D)[3] + 3 * fwd_launch(kind, D, 1)[3] + 1, 'b' if D != 260 else 'a', 0.01, False, False))
    # separate EmbLoss tables (reg_user_w / reg_item_w: the kernel's SAME = false form)
    out += [('mse', 64, 2048, 'a', 0.01, True, False), ('bce', 64, edges('bce', 64)[2] + 1, 'b', 0.02, True, False),
            ('bce', 128, 3000, 'a', 0.01, True, False)]
    # set_deterministic(True): the C1 / C2 shapes and medium cases on cdr_ordered_bwd; 8,193 triples take the sorted route
    out += [('bpr', 64, 2048, 'a', 0.01, False, True), ('bpr', 64, 4096, 'a', 0.01, False, True), ('bpr', 64, 8193, 'a', 0.01, False, True),
            ('mse', 64, 2048, 'a', 0.01, False, True), ('bce', 64, 2048, 'a', 0.0, False, True), ('bce', 128, 8192, 'b', 0.01, False, True),
            ('mse', 64, 2048, 'a', 0.01, True, True)]
    return out


def _pair_cases():
    """(B_s, B_t, D, table, reg_s, reg_t, alpha, shape, deterministic); the pair kernel finishes in-kernel while 2 * grid <= 512."""
    return [(1000, 777, 64, 'a', 0.02, 0.05, 0.3, 'hot', False),
            (2048, 2048, 64, 'a', 0.0, 0.0, 0.5, 'hot', False),              # C1 as bench.py configures it
            (2048, 2048, 64, 'a', 0.0, 0.0, 0.5, 'hot', True),
            (1500, 3000, 64, 'a', 0.02, 0.0, 0.3, 'hot', True),              # reg on one domain only
            (16384, 9000, 64, 'a', 0.0, 0.05, 0.7, 'hot', False),
            (32768, 20000, 64, 'a', 0.02, 0.05, 0.3, 'hot', False),          # grid 256: the last in-kernel finish
            (20000, 32769, 64, 'b', 0.02, 0.0, 0.3, 'hot', False),           # grid 257: separate finish
            (262145, 100003, 64, 'a', 0.02, 0.05, 0.7, 'hot', False),        # capped, ragged tail in the source batch
            (8193, 5000, 128, 'b', 0.0, 0.05, 0.3, 'hot', False),
            (3000, 2000, 32, 'a', 0.02, 0.05, 0.3, 'hot', False),
            (700, 900, 260, 'a', 0.02, 0.05, 0.3, 'hot', False),
            (500, 800, 50, 'a', 0.02, 0.05, 0.3, 'hot', False),              # D % 4 != 0: two cdr_point_fwd launches and cdr_scalar_mix
            (20000, 30000, 64, 'b', 0.02, 0.05, 0.3, 'far', False)]          # BCE saturation


def test_case_table_covers_every_launch_regime():
    """Each forward kernel (BPR, pointwise, pair) meets every launch regime at the benchmark widths, with a ragged tail past the cap; the
    edges at D = 64 are the ones the kernels' constants give today (BPR 2,048 / 8,192 / 32,768 / 131,072; pointwise 2,048 / 16,384 /
    65,536 / 262,144), so a change of those constants fails here first."""
    assert edges('bpr', 64) == (2048, 8192, 32768, 131072) and edges('mse', 64) == (2048, 16384, 65536, 262144)
    assert edges('bpr', 128) == (1024, 4096, 16384, 65536) and edges('mse', 128) == (1024, 8192, 32768, 131072)
    assert [regime('bpr', 64, B) for B in (2048, 2049, 8192, 8193, 32768, 32769, 131072, 131073)] == \
        [REGIMES[1], REGIMES[0], REGIMES[2], REGIMES[3], REGIMES[3], REGIMES[4], REGIMES[4], REGIMES[5]]
    cases = _kernel_cases()
    for D in (64, 128):
        for kernel, kinds in (('bpr', ('bpr',)), ('point', ('mse', 'bce'))):
            seen = {regime(k, D, B) for k, d, B, *_ in cases if d == D and k in kinds}
            assert seen >= set(REGIMES), (kernel, D, set(REGIMES) - seen)
            assert any(is_ragged_tail(k, D, B) for k, d, B, *_ in cases if d == D and k in kinds), (kernel, D)
    for kind in ('mse', 'bce'):                                  # both loss kinds of the pointwise kernel, at the C1 / C2 width
        assert {regime(k, 64, B) for k, d, B, *_ in cases if d == 64 and k == kind} >= set(REGIMES), kind
    for D in (32, 260, 50):
        for kinds in (('bpr',), ('mse', 'bce')):
            mine = [(k, B) for k, d, B, *_ in cases if d == D and k in kinds]
            assert any(is_ragged_tail(k, D, B) for k, B in mine) and any(not fwd_launch(k, D, B)[2] for k, B in mine), (D, kinds)
    assert lpr_for(260) == 64 and 260 // 4 > 64 and lpr_for(32) == 8
    pairs = _pair_cases()
    seen = {regime('point', D, max(Bs, Bt), K_SIGN_IN_MAX // 2) for Bs, Bt, D, *_ in pairs if D == 64}
    assert seen >= set(REGIMES), set(REGIMES) - seen
    assert any(is_ragged_tail('point', D, max(Bs, Bt)) for Bs, Bt, D, *_ in pairs)
    assert fwd_launch('point', 64, 32768)[1] == 256 and fwd_launch('point', 64, 32769)[1] == 257          # both sides of 2 * grid <= 512
    assert any(Bs != Bt for Bs, Bt, *_ in pairs) and any(a != 0.5 for *_, a, _s, _d in pairs)
    assert any((rs == 0.0) != (rt == 0.0) for _bs, _bt, _D, _t, rs, rt, *_ in pairs)
    assert any(det for *_, det in cases) and any(det for *_, det in pairs)


# ---------------------------------------------------------------------------------------------------------------------- inputs
def _tables(table, D, gen, n=2):
    nu, ni = TABLES[table]
    return [torch.empty(nu if j % 2 == 0 else ni, D, device=gen.device).normal_(0, 0.1, generator=gen) for j in range(n)]


def _draw(B, rows, gen, hot_every=0):
    """Ids over [0, rows - 3): the last three rows are kept for the batch's last interaction; with ``hot_every`` one row (rows // 3)
    takes every hot_every-th place."""
    x = torch.randint(0, rows - 3, (B,), device=gen.device, generator=gen)
    if hot_every:
        x[3::hot_every] = rows // 3
    return x


def _bpr_ids(B, nu, ni, gen, hot):
    """A hot user and a hot item (an eighth of the batch each) on request; ids 0 and rows - 1; ~1 % of the triples with p == n; the
    last triple's three rows occur nowhere else."""
    u, p, n = _draw(B, nu, gen, 8 if hot else 0), _draw(B, ni, gen, 7 if hot else 0), _draw(B, ni, gen)
    same = torch.randint(0, B - 1, (max(1, B // 100),), device=gen.device, generator=gen)
    n[same] = p[same]
    u[0], u[1], p[2], n[4], p[5] = 0, nu - 1, 0, 0, ni - 1
    u[-1], p[-1], n[-1] = nu - 2, ni - 2, ni - 3
    items = torch.cat([p, n])
    assert int((u == nu - 2).sum()) == 1 and int((items == ni - 2).sum()) == 1 and int((items == ni - 3).sum()) == 1
    return u, p, n


def _point_ids(B, nu, ni, gen, hot):
    u, i = _draw(B, nu, gen, 8 if hot else 0), _draw(B, ni, gen, 7 if hot else 0)
    u[0], u[1], i[2], i[5] = 0, nu - 1, 0, ni - 1
    u[-1], i[-1] = nu - 2, ni - 2
    assert int((u == nu - 2).sum()) == 1 and int((i == ni - 2).sum()) == 1
    y = (torch.rand(B, device=gen.device, generator=gen) < 0.5).float()
    return u, i, y


def _far_rows(U, I):
    """Rows 0..63 of both tables with entries 1 (users) and +-2 (items): a pair of them scores +-2 D, far enough out for the fp32
    sigmoid to return exactly 1 or 0 -- BCE's -100 log clamp and the 1e-12 clamp of its backward."""
    U[:64] = 1.0
    I[:64] = 2.0
    I[32:64] = -2.0


def _poison(*tables):
    """A NaN-filled tensor of the flat gradient buffer's size (functional._prezero_for_backward / _zeros_like2), freed at once."""
    n = sum((t.numel() + 3) // 4 * 4 for t in tables)
    torch.full((n,), float('nan'), device=DEV, dtype=torch.float32)
    n2 = sum(t.numel() for t in tables)
    if n2 != n:
        torch.full((n2,), float('nan'), device=DEV, dtype=torch.float32)


class _deterministic:
    def __init__(self, flag):
        self.flag = flag

    def __enter__(self):
        from recbole_cdr_amd import functional as F_
        self.was = F_._DETERMINISTIC[0]
        F_.set_deterministic(self.flag)

    def __exit__(self, *exc):
        from recbole_cdr_amd import functional as F_
        F_.set_deterministic(self.was)


def _route(kind, D, lists, det):
    from recbole_cdr_amd import functional as F_
    if not det:
        return 'atomic'
    with _deterministic(True):
        return 'ordered' if F_.ordered_fits(D, *lists) else 'sorted'


# ---------------------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize('kind,D,B,table,reg,sep,det', _kernel_cases())
def test_dense_loss_vs_fp64(kind, D, B, table, reg, sep, det):
    from recbole_cdr_amd import binding as B_, functional as F_
    gen = torch.Generator(device=DEV); gen.manual_seed(1000 * D + B + (kind == 'bce'))
    nu, ni = TABLES[table]
    hot = table == 'a' and B >= 2048
    go = f32(GO)
    params = [t.requires_grad_(True) for t in _tables(table, D, gen, 4 if sep else 2)]
    U, I = params[0], params[1]
    detail = {}
    with torch.no_grad():
        if kind == 'bpr':
            u, p, n = _bpr_ids(B, nu, ni, gen, hot)
            loss, *parts = bpr_grads_fp64(U, I, u, p, n, f32(reg), go=go, detail=detail)
        else:
            u, i, y = _point_ids(B, nu, ni, gen, hot)
            loss, *parts = point_grads_fp64(U, I, u, i, y, f32(reg), kind, go=go, RU=params[2] if sep else None, RI=params[3] if sep else None,
                                            detail=detail)
    ref = {'scalars': {'loss': loss, 'main': detail['main'], 'norm_u': detail['nu'], 'norm_i': detail['ni']},
           'coefs': [(detail['g'], detail['delta'])], 'parts': parts}
    route = _route(kind, D, (B, 2 * B) if kind == 'bpr' else (B,), det)
    with _deterministic(det):
        _poison(*params)
        if kind == 'bpr':
            out = F_.BPRGatherLoss.apply(U, I, u, p, n, GAMMA, reg)
        else:
            out, _scores = F_.PointGatherLoss.apply(B_.CDR_LOSS_MSE if kind == 'mse' else B_.CDR_LOSS_BCE, U, I, params[2] if sep else None,
                                                    params[3] if sep else None, u, i, y, reg)
        saved = out.grad_fn.saved_tensors
        gcoef, out4 = saved[-2], saved[-1]
        assert gcoef.shape == (B,) and out4.shape == (4,)
        out.backward(torch.full_like(out, GO))
        torch.cuda.synchronize()
    o4 = out4.tolist()
    got = {'scalars': {'loss': float(out), 'main': o4[1], 'norm_u': o4[2], 'norm_i': o4[3]}, 'coefs': [gcoef],
           'grads': [t.grad for t in params]}
    assert o4[0] == float(out)
    tag = f'{kind} D={D} B={B} table {table} reg={reg}{" sep" if sep else ""} {route}'
    worst = check_dense_result(tag, got, ref, D)
    u_, grid, capped, per, unroll = fwd_launch(kind, D, B)
    print(f'\n{tag}: [{regime(kind, D, B) if D % 4 == 0 else "scalar" + (", capped+tail" if capped else "")}; grid {grid}, {u_} per group] '
          f'worst error / bound: {_fmt(worst)}')


def _pair_ids(shape, Bs, Bt, nu, ni, gen):
    """Both batches on the shared tables: user nu // 3 and item ni // 3 are hot in BOTH domains; the source batch's last row pair occurs
    nowhere else.  'far': an eighth of each batch scores +-2 D (see _far_rows)."""
    su, si, ys = _point_ids(Bs, nu, ni, gen, True)
    tu, ti, yt = _point_ids(Bt, nu, ni, gen, True)
    tu[-1], ti[-1] = nu - 3, ni - 3                       # (the target batch's own last rows: _point_ids gave it the source's)
    if shape == 'far':
        r = lambda n: torch.randint(0, 64, (n,), device=gen.device, generator=gen)
        ks, kt = Bs // 8, Bt // 8
        su[10:10 + ks], si[10:10 + ks], tu[10:10 + kt], ti[10:10 + kt] = r(ks), r(ks), r(kt), r(kt)
    for x, rows in ((su, nu), (tu, nu), (si, ni), (ti, ni)):
        assert int((x == rows // 3).sum()) > 1
    assert int((torch.cat([su, tu]) == nu - 2).sum()) == 1 and int((torch.cat([si, ti]) == ni - 2).sum()) == 1
    return su, si, ys, tu, ti, yt


@pytest.mark.parametrize('Bs,Bt,D,table,reg_s,reg_t,alpha,shape,det', _pair_cases())
def test_two_domain_point_loss_vs_fp64(Bs, Bt, D, table, reg_s, reg_t, alpha, shape, det):
    """TwoDomainPointLoss (CMF's node: cdr_point_fwd_pair + cdr_point_bwd_dense_pair, or cdr_ordered_bwd) on shared tables."""
    from recbole_cdr_amd import binding as B_, functional as F_
    gen = torch.Generator(device=DEV); gen.manual_seed(Bs + 3 * Bt + D)
    nu, ni = TABLES[table]
    go = f32(GO)
    U, I = _tables(table, D, gen)
    if shape == 'far':
        _far_rows(U, I)
    U.requires_grad_(True); I.requires_grad_(True)
    su, si, ys, tu, ti, yt = _pair_ids(shape, Bs, Bt, nu, ni, gen)
    w = (f32(alpha), f32(1.0 - alpha))                          # as functional._pair_weights / the backward's float arguments round them
    detail = []
    with torch.no_grad():
        loss, _, upart, ipart = pair_grads_fp64(U, I, [(su, si, ys, f32(reg_s), w[0]), (tu, ti, yt, f32(reg_t), w[1])], go=go, detail=detail)
    if shape == 'far':
        x = (U.detach()[su] * I.detach()[si]).sum(1)
        assert int((x.abs() > 100).sum()) >= Bs // 16, 'the saturation case does not saturate'
    ref = {'scalars': {'loss': loss}, 'coefs': [(d['g'], d['delta']) for d in detail], 'parts': [upart, ipart]}
    for j, d in enumerate(detail):
        ref['scalars'].update({f'total{j}': d['main'] + (f32(reg_s), f32(reg_t))[j] * (d['nu'] + d['ni']) / (Bs, Bt)[j],
                               f'main{j}': d['main'], f'norm_u{j}': d['nu'], f'norm_i{j}': d['ni']})
    route = _route('pair', D, (Bs + Bt,), det)
    with _deterministic(det):
        _poison(U, I)
        out, losses = F_.TwoDomainPointLoss.apply(B_.CDR_LOSS_BCE, U, I, su, si, ys, reg_s, tu, ti, yt, reg_t, alpha)
        saved = out.grad_fn.saved_tensors
        gs, out8 = [saved[6], saved[7]], saved[8]
        assert gs[0].shape == (Bs,) and gs[1].shape == (Bt,) and out8.shape == (2, 4)
        out.backward(torch.full_like(out, GO))
        torch.cuda.synchronize()
    o8 = out8.tolist()
    got = {'scalars': {'loss': float(out)}, 'coefs': gs, 'grads': [U.grad, I.grad]}
    for j in range(2):
        got['scalars'].update({f'total{j}': o8[j][0], f'main{j}': o8[j][1], f'norm_u{j}': o8[j][2], f'norm_i{j}': o8[j][3]})
    assert losses.tolist() == [o8[0][0], o8[1][0]]
    tag = f'pair {Bs}+{Bt} D={D} table {table} reg={reg_s},{reg_t} alpha={alpha} {shape} {route}'
    worst = check_dense_result(tag, got, ref, D)
    u_, grid, capped, per, unroll = fwd_launch('point', D, max(Bs, Bt))
    print(f'\n{tag}: [{regime("point", D, max(Bs, Bt), K_SIGN_IN_MAX // 2) if D % 4 == 0 else "scalar"}; grid {grid} x 2, {u_} per group] '
          f'worst error / bound: {_fmt(worst)}')


def test_bce_saturation_single_batch_vs_fp64():
    """PointGatherLoss BCE with an eighth of the rows at |x| = 2 D = 128: p is exactly 0 or 1 in fp32, log clamps at -100 and the
    backward's max(pq, 1e-12) gives those rows a zero coefficient (pair_grads_fp64's clamp-aware form with one domain of weight 1)."""
    from recbole_cdr_amd import binding as B_, functional as F_
    D, B, reg = 64, 20000, 0.01
    gen = torch.Generator(device=DEV); gen.manual_seed(99)
    nu, ni = TABLES['a']
    U, I = _tables('a', D, gen)
    _far_rows(U, I)
    U.requires_grad_(True); I.requires_grad_(True)
    u, i, y = _point_ids(B, nu, ni, gen, True)
    k = B // 8
    u[10:10 + k] = torch.randint(0, 64, (k,), device=DEV, generator=gen)
    i[10:10 + k] = torch.randint(0, 64, (k,), device=DEV, generator=gen)
    go = f32(GO)
    detail = []
    with torch.no_grad():
        loss, _, upart, ipart = pair_grads_fp64(U, I, [(u, i, y, f32(reg), 1.0)], go=go, detail=detail)
        sat = (U[u] * I[i]).sum(1).abs() > 100
    assert int(sat.sum()) >= k // 2
    d = detail[0]
    ref = {'scalars': {'loss': loss, 'main': d['main'], 'norm_u': d['nu'], 'norm_i': d['ni']}, 'coefs': [(d['g'], d['delta'])],
           'parts': [upart, ipart]}
    assert d['main'] > 100 * 0.4 * float(sat.sum()) / B            # about half of the saturated rows sit on the wrong side: -100 each
    _poison(U, I)
    out, _ = F_.PointGatherLoss.apply(B_.CDR_LOSS_BCE, U, I, None, None, u, i, y, reg)
    saved = out.grad_fn.saved_tensors
    gcoef, out4 = saved[-2], saved[-1]
    out.backward(torch.full_like(out, GO))
    torch.cuda.synchronize()
    assert bool((gcoef[sat] == 0).all()), 'saturated rows must carry a zero coefficient (pq = 0 under the 1e-12 clamp)'
    o4 = out4.tolist()
    got = {'scalars': {'loss': float(out), 'main': o4[1], 'norm_u': o4[2], 'norm_i': o4[3]}, 'coefs': [gcoef], 'grads': [U.grad, I.grad]}
    worst = check_dense_result('bce saturation', got, ref, D)
    print(f'\nbce saturation D={D} B={B}: {int(sat.sum())} saturated rows; worst error / bound: {_fmt(worst)}')


# ---------------------------------------------------------------------------------------------------------------------- step level
def _bench_ids():
    from oracle.common import IdSpace
    return IdSpace(OU=1, TOU=943, SOU=6040, OI=1604, TOI=61, SOI=2280)


def _all_rows(part, n_rows):
    """A part over the batch's rows spread over ALL rows of the table (G = A = E = 0, no occurrences elsewhere)."""
    rows, G, A, E, occ = part
    full = [torch.zeros(n_rows, G.shape[1], device=G.device, dtype=torch.float64) for _ in range(3)]
    for f, x in zip(full, (G, A, E)):
        f[rows] = x
    o = torch.zeros(n_rows, device=G.device, dtype=occ.dtype)
    o[rows] = occ
    return torch.arange(n_rows, device=G.device), full[0], full[1], full[2], o


def _adam_state(opt, p):
    st = opt.state.get(p, {})
    if not st:
        return {'w': p.detach().clone(), 'm': torch.zeros_like(p), 'v': torch.zeros_like(p)}
    return {'w': p.detach().clone(), 'm': st['exp_avg'].clone(), 'v': st['exp_avg_sq'].clone()}


def _dense_steps(model, tag, trained, batches, reference, lr=1e-3):
    """Three eager steps of calculate_loss -> backward -> DenseAdam.step; ``trained``: the parameter names the phase has gradients for;
    ``reference(before, batch)`` -> (loss, {name: part}) from the device state before the step."""
    from recbole_cdr_amd.trainer.trainer import DenseAdam
    named = dict(model.named_parameters())
    opt = DenseAdam(list(named.values()), lr=lr)
    D = named[trained[0]].shape[1]
    worst = {}
    for t, batch in enumerate(batches, start=1):
        before = {k: _adam_state(opt, named[k]) for k in trained}
        frozen = {k: p.detach().clone() for k, p in named.items() if k not in trained}
        with torch.no_grad():
            loss, parts = reference({k: b['w'] for k, b in before.items()}, batch)
        want = {k: apply_fp64(before[k], _all_rows(parts[k], named[k].shape[0]), D, 'adam', lr, 0.0, t) for k in trained}
        opt.zero_grad(set_to_none=True)
        got = model.calculate_loss(batch)
        got.backward()
        opt.step()
        torch.cuda.synchronize()
        worst['loss'] = max(worst.get('loss', 0.0), check_scalar(f'{tag} step {t}: loss', float(got), loss))
        for k in trained:
            st = opt.state[named[k]]
            assert int(st['step']) == t, f'{tag}: {k} update count'
            after = {'w': named[k].detach(), 'm': st['exp_avg'], 'v': st['exp_avg_sq']}
            every = torch.arange(named[k].shape[0], device=DEV)
            for q, v in _check_table(f'{tag} step {t} {k}', before[k], after, every, want[k]).items():
                worst[f'{k.split("_emb")[0]}.{q}'] = max(worst.get(f'{k.split("_emb")[0]}.{q}', 0.0), v)
            if t == 1:                                # rows the first batch does not touch: weights bit-identical, moments exactly zero
                idle = torch.ones(named[k].shape[0], dtype=torch.bool, device=DEV)
                idle[parts[k][0]] = False
                assert int(idle.sum()) > 0
                assert torch.equal(after['w'][idle].view(torch.int32), before[k]['w'][idle].view(torch.int32)), f'{tag}: {k}: an untouched row moved'
                assert int(after['m'][idle].view(torch.int32).count_nonzero()) == 0 and int(after['v'][idle].view(torch.int32).count_nonzero()) == 0
        for k, p0 in frozen.items():
            assert torch.equal(named[k].detach().view(torch.int32), p0.view(torch.int32)), f'{tag} step {t}: {k} has no gradient and moved'
            assert named[k].grad is None and not opt.state.get(named[k]), f'{tag}: {k} must stay outside the step'
    print(f'\n{tag}: worst error / bound over {len(batches)} steps: {_fmt(worst)}')


def _domain_ids(ids, domain, kind, B, gen):
    """Ids as the benchmark's loaders draw them: the domain's own user and item ranges of the union id space."""
    r = lambda lo, hi: torch.randint(lo, hi, (B,), device=DEV, generator=gen)
    if domain == 'source':                                    # overlap rows [1, O) and the source-only rows behind the target-only ones
        u, i = r(ids.OU + ids.TOU, ids.total_num_users), r(ids.OI + ids.TOI, ids.total_num_items)
        i[::3] = r(1, ids.OI)[::3]
    else:
        u, i = r(1, ids.OU + ids.TOU), r(1, ids.OI + ids.TOI)
    return u, i


def test_cmf_c1_dense_steps_vs_fp64():
    from recbole_cdr_amd.model.cross_domain_recommender.cmf import CMF
    ids, D, B, alpha = _bench_ids(), 64, 2048, 0.5
    torch.manual_seed(2022)
    model = CMF(base_config(DEV, embedding_size=D, alpha=alpha, **{'lambda': 0.0, 'gamma': 0.0}), FakeDataset(ids)).to(DEV)
    assert (model.user_embedding.weight.shape[0], model.item_embedding.weight.shape[0]) == TABLES['a']
    gen = torch.Generator(device=DEV); gen.manual_seed(1)
    batches = []
    for _ in range(3):
        su, si = _domain_ids(ids, 'source', 'point', B, gen)
        tu, ti = _domain_ids(ids, 'target', 'point', B, gen)
        lab = lambda: (torch.rand(B, device=DEV, generator=gen) < 0.5).float()
        batches.append({model.SOURCE_USER_ID: su, model.SOURCE_ITEM_ID: si, model.SOURCE_LABEL: lab(),
                        model.TARGET_USER_ID: tu, model.TARGET_ITEM_ID: ti, model.TARGET_LABEL: lab()})

    def reference(w, b):
        loss, _, upart, ipart = pair_grads_fp64(w['user_embedding.weight'], w['item_embedding.weight'],
                                                [(b[model.SOURCE_USER_ID], b[model.SOURCE_ITEM_ID], b[model.SOURCE_LABEL], 0.0, f32(alpha)),
                                                 (b[model.TARGET_USER_ID], b[model.TARGET_ITEM_ID], b[model.TARGET_LABEL], 0.0, f32(1 - alpha))])
        return loss, {'user_embedding.weight': upart, 'item_embedding.weight': ipart}
    _dense_steps(model, 'C1 CMF D=64 2x2048', ['user_embedding.weight', 'item_embedding.weight'], batches, reference)


@pytest.mark.parametrize('phase', ['SOURCE', 'TARGET'])
@pytest.mark.parametrize('lfm', ['BPR', 'MF'])
def test_emcdr_c2_dense_steps_vs_fp64(lfm, phase):
    from recbole_cdr_amd.model.cross_domain_recommender.emcdr import EMCDR
    ids, D, B, reg = _bench_ids(), 64, 2048, 0.01
    torch.manual_seed(2022)
    model = EMCDR(base_config(DEV, latent_factor_model=lfm, source_embedding_size=D, target_embedding_size=D, reg_weight=reg,
                              mapping_function='non_linear', mlp_hidden_size=[128]), FakeDataset(ids)).to(DEV)
    model.set_phase(phase)
    dom = phase.lower()
    names = [f'{dom}_user_embedding.weight', f'{dom}_item_embedding.weight']
    F = lambda s: getattr(model, f'{phase}_{s}')
    gen = torch.Generator(device=DEV); gen.manual_seed(2 + (phase == 'TARGET'))
    batches = []
    for _ in range(3):
        u, i = _domain_ids(ids, dom, lfm, B, gen)
        b = {F('USER_ID'): u, F('ITEM_ID'): i}
        if lfm == 'BPR':
            b[F('NEG_ITEM_ID')] = _domain_ids(ids, dom, lfm, B, gen)[1]
        else:
            b[F('LABEL')] = (torch.rand(B, device=DEV, generator=gen) < 0.5).float()
        batches.append(b)

    def reference(w, b):
        if lfm == 'BPR':
            loss, upart, ipart = bpr_grads_fp64(w[names[0]], w[names[1]], b[F('USER_ID')], b[F('ITEM_ID')], b[F('NEG_ITEM_ID')], f32(reg))
        else:
            loss, upart, ipart = point_grads_fp64(w[names[0]], w[names[1]], b[F('USER_ID')], b[F('ITEM_ID')], b[F('LABEL')], f32(reg), 'mse')
        return loss, {names[0]: upart, names[1]: ipart}
    _dense_steps(model, f'C2 EMCDR-{lfm} {phase} D=64 B=2048', names, batches, reference)
