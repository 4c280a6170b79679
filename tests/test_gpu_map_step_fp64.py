"""EMCDR's OVERLAP step (fused.FusedMapStep: the two launches of csrc/cdr_mapstep.hip for distinct ids, and the general path) against a
float64 restatement in plain torch of calculate_map_loss -- MSE(mapping(S[idx]), T[idx]) averaged over n Dt, then the lazy row-wise
Adam / SGD on the S and T rows the batch names, then the dense Adam / SGD on the mapping's parameters -- at the benchmark's
OB = 65,536 ids and at the round boundaries of every dispatch branch, held to PER-ELEMENT first-order error bounds carried through
the reference itself.

Teacher forcing: each of a case's three steps is judged from the device's own fp32 state just before it (tables, moments, the
per-table and per-parameter update counts, the mapping), so errors never pile up across steps.  Both tables and the mapping start
from nonzero moments, the source table at update 1,000, the target table at 37 and every mapping parameter at a count of its own,
so a swapped or shared bias correction shows.

Bounds (u = 2^-24, gamma_k = k u / (1 - k u); fp64_bounds: U32, gam, ulp32, apply_fp64 and its K_SUM / K_ADAM; the constants
below are named once and used as written):
  * layer z = h W^T (+ b): gamma_{din + 1} (|h| |W|^T + |b|) + e_h |W|^T  (W exact: it is the device's own state);
    tanh a = tanhf(z): (1 - a^2) e_z + K_TANH ulp(a);
  * d = y - t: e_y + u |d|;  gz = (2 / (n Dt)) d: (2 / (n Dt)) e_d + K_GZ u |gz|;
  * backward through a layer: dL/dh = g W with gamma_{dout} |g| |W| + e_g |W|; through tanh, g' = dL/da (1 - a^2) with a carrying
    its own bound: e_{1 - a^2} = 2 |a| e_a + K_ACTB u (a^2 + |1 - a^2|), then |1 - a^2| e_{dL/da} + |dL/da| e_{1 - a^2} + u |g'|;
  * table rows: apply_fp64 with the contraction depth of dL/dS (layer 0's dout; 0 for dL/dT = -gz) in place of D, so that
    k = depth + occ + K_SUM (occ = 1 on the distinct-id path; the general path sums repeated rows);
  * mapping weight and bias gradients, each a sum over ALL n ids: apply_fp64 with D = the depth of the reduction tree the launch
    geometry implies (_unique_depth, _general_depth) and occ = 0 -- NOT gamma_n: gamma_65536 is ~4e-3 and could not see a block of
    32 ids go missing;
  * the Adam / SGD updates: apply_fp64 (see test_gpu_step_fp64.py's docstring).
The losses are held to LOSS_RTOL relative of the fp64 value.  Every row outside the batch -- the rows just above and below every
touched id in particular -- stays bit-identical in both tables, weights and moments alike; the device counters advance by exactly
one and the host mirrors agree.  Each case prints its worst error / bound per quantity."""
import gc

import pytest
import torch

from fp64_bounds import U32, apply_fp64, gam, ulp32
from helpers import DEV, FakeDataset, base_config

pytestmark = pytest.mark.gpu

K_TANH = 4                  # ulps of tanhf (ocml's tanhf is within 2; the bias add before it is in gamma_{din + 1})
K_GZ = 4                    # roundings of gz: (float) n * Dt, 2 / that, its product with d (general path: the grad_out scale)
K_ACTB = 2                  # roundings of 1 - a^2: the square and the subtraction
LOSS_RTOL = 1e-5
NUM_CU = 256                # CDR_NUM_CU (csrc/cdr_common.h)
ROWS = 32                   # kRows: ids per block of every map kernel (csrc/cdr_mapstep.hip)
WG_WAVES = 8                # kWgWaves: batch-row slices per 32 x 32 tile of linear_wgrad_small_kernel (csrc/cdr_linear.hip)
SRC_STEP, TGT_STEP = 1000, 37
OPTS = {                    # (opt, lr, betas, eps, weight_decay)
    'adam': ('adam', 1e-3, (0.9, 0.999), 1e-8, 0.0),
    'adam_wd': ('adam', 1e-3, (0.9, 0.999), 1e-8, 1e-2),
    'adam_hp': ('adam', 1e-3, (0.8, 0.99), 1e-6, 1e-2),
    'sgd': ('sgd', 0.5, (0.9, 0.999), 1e-8, 0.0),
    'sgd_wd': ('sgd', 0.5, (0.9, 0.999), 1e-8, 1e-2),
}


def _cdiv(a, b):
    return -(-a // b)


def _unique_depth(n, per_cu, bias):
    """Reduction depth of a mapping gradient on the distinct-id path (csrc/cdr_mapstep.hip).  wg_count(n, per_cu) workgroups
    (per_cu = 1 for map_pipe_kernel / map_pipe3_kernel, 2 for map_step_kernel) walk the 32-id blocks
    rb = blockIdx.x, + gridDim.x, ...  A weight element is one MFMA accumulator chain across all of a workgroup's blocks (16
    v_mfma_f32_32x32x2f32 per block: 32 ids, `MF1(wacc[q], ...)`), +1 for the product; a bias element is a 32-row sequential sum per
    block added into `bacc` once per block.  map_finish_kernel then adds workgroups sub, sub + 16, ... in sixteen strided sums
    (`for (int b = sub; b < nwg; b += 16)`) and the sixteen in order (`for (int j = 0; j < 16; ++j)`)."""
    nrb = _cdiv(n, ROWS)
    nwg = max(1, min(nrb, per_cu * NUM_CU))
    bpw = _cdiv(nrb, nwg)
    inner = ROWS + bpw if bias else ROWS * bpw + 1
    return inner + _cdiv(nwg, 16) + 16


def _general_depth(n, bias):
    """Reduction depth of a mapping gradient on the general path: functional.LinearAct.backward takes cdr_linear_wgrad_small
    (csrc/cdr_linear.hip) for every batch up to 2^18 rows whose 32 x 32 tiles fit its tickets.  wgrad_split cuts the n rows into
    min(ceil(n / 512), 64) even-aligned chunks (one workgroup each); linear_wgrad_small_kernel gives each of its WG_WAVES waves an
    even-aligned slice `per` of the chunk (one MFMA chain, +1 for the product; the bias lane sums half of it and the two row
    parities meet in one `__shfl_xor` add), adds the waves in order and the last workgroup adds the chunks in chunk order."""
    nch = min(_cdiv(n, 512), 64)
    chunk = (_cdiv(n, nch) + 1) & ~1
    nz = _cdiv(n, chunk)
    per = (_cdiv(chunk, WG_WAVES) + 1) & ~1
    inner = per // 2 + 1 if bias else per + 1
    return inner + WG_WAVES + nz


# ---------------------------------------------------------------------------------------------------------------------- fp64 reference

def map_grads_fp64(S, T, layers, idx):
    """calculate_map_loss and its gradients in float64 from the fp32 device state.  Returns (loss, S part, T part, parameter parts):
    a table part is (rows, G, A, E, occ, depth) -- unique row ids, summed gradient, summed |terms|, summed first-order error of the
    terms, occurrences, contraction depth; a parameter part is (G, A, E) of the full-batch sum, in the parameter's shape."""
    n = idx.numel()
    rows, inv = torch.unique(idx, return_inverse=True)
    x, t = S[rows].double()[inv], T[rows].double()[inv]
    Ws = [(W.detach().double(), None if b is None else b.detach().double(), act) for W, b, act in layers]
    h, eh = x, torch.zeros_like(x)
    saved = []                                          # (input, its bound, output, its bound, act) per layer
    for W, b, act in Ws:
        Wa = W.abs()
        z = h @ W.T
        Az = h.abs() @ Wa.T
        if b is not None:
            z, Az = z + b, Az + b.abs()
        ez = gam(W.shape[1] + 1) * Az + eh @ Wa.T
        del Az
        if act:
            a = torch.tanh(z)
            ea = (1 - a * a) * ez + K_TANH * ulp32(a)
            saved.append((h, eh, a, ea, act))
            h, eh = a, ea
        else:
            saved.append((h, eh, z, ez, act))
            h, eh = z, ez
        del z, ez
    Dt = h.shape[1]
    d = h - t
    ed = eh + U32 * d.abs()
    loss = float((d * d).sum()) / (n * Dt)
    gs = 2.0 / (n * Dt)
    g = gs * d
    eg = gs * ed + K_GZ * U32 * g.abs()
    del d, ed, x, t
    tparts = (-g, g.abs(), eg)
    pparts = [None] * len(Ws)
    sparts = None
    for l in range(len(Ws) - 1, -1, -1):
        W, b, _ = Ws[l]
        hin, ehin = saved[l][0], saved[l][1]
        ga = g.abs()
        gW = (g.T @ hin, ga.T @ hin.abs(), ga.T @ ehin + eg.T @ hin.abs())
        gb = None if b is None else (g.sum(0), ga.sum(0), eg.sum(0))
        pparts[l] = (gW, gb)
        Wa = W.abs()
        gh = g @ W
        Agh = ga @ Wa
        egh = eg @ Wa
        if l == 0:
            sparts = (gh, Agh, egh)
            break
        egh = gam(W.shape[0]) * Agh + egh
        del Agh
        a, ea = saved[l - 1][2], saved[l - 1][3]
        if saved[l - 1][4]:
            s = 1 - a * a
            es = 2 * a.abs() * ea + K_ACTB * U32 * (a * a + s.abs())
            g = gh * s
            eg = s.abs() * egh + gh.abs() * es + U32 * g.abs()
            del s, es
        else:
            g, eg = gh, egh
        del gh, egh
    occ = torch.bincount(inv, minlength=rows.numel())

    def table(part, depth):
        G = torch.zeros(rows.numel(), part[0].shape[1], device=part[0].device, dtype=torch.float64)
        A, E = torch.zeros_like(G), torch.zeros_like(G)
        G.index_add_(0, inv, part[0]); A.index_add_(0, inv, part[1]); E.index_add_(0, inv, part[2])
        return rows, G, A, E, occ, depth
    return loss, table(sparts, layers[0][0].shape[0]), table(tparts, 0), pparts


# ---------------------------------------------------------------------------------------------------------------------- cases

def _make_mapping(dims, bias, gen, misalign=False):
    """[(W, b, act)] of a linear (2 dims) or tanh-MLP (more) mapping (emcdr.py:59-64, 86-93), its parameters and its mapping_fn.
    Weights ~ N(0, 4 / din) on rows ~ N(0, 0.5^2): pre-activations of order one, so 1 - a^2 and 1 - z^2 differ."""
    from recbole_cdr_amd import binding as B_, functional as F_
    L = len(dims) - 1
    layers, params = [], []
    for l in range(L):
        din, dout = dims[l], dims[l + 1]
        if misalign:                                    # one float off 16-byte alignment: net.vec == 0, scalar weight loads
            W = torch.empty(dout * din + 1, device=DEV)[1:].view(dout, din)
            assert W.data_ptr() % 16 == 4
        else:
            W = torch.empty(dout, din, device=DEV)
        W.normal_(0, 2.0 / din ** 0.5, generator=gen).requires_grad_(True)
        b = torch.empty(dout, device=DEV).normal_(0, 0.3, generator=gen).requires_grad_(True) if bias else None
        layers.append((W, b, B_.ACT_TANH if l < L - 1 else B_.ACT_NONE))
        params += [W] + ([b] if bias else [])

    def fn(x):
        for W, b, act in layers:
            x = F_.linear(x, W, b, act)
        return x
    return layers, params, fn


def _distinct_ids(n, rows, gen):
    """n distinct ids out of [0, rows) (a slice of a permutation, as the OverlapDataloader yields them), 0 and rows - 1 among them."""
    ids = torch.randperm(rows, device=DEV, generator=gen)[:n]
    if n == 1:
        return ids
    if not bool((ids == 0).any()):
        ids[0] = 0
    if not bool((ids == rows - 1).any()):
        ids[-1] = rows - 1
    return ids


def _repeated_ids(n, rows, gen, hot):
    """Zipf(1.05) ids over [0, rows) with one id repeated ``hot`` times (the general path's sort and summed row gradients)."""
    r = torch.rand(n, device=DEV, generator=gen, dtype=torch.float64)
    ids = (((float(rows) ** -0.05 - 1) * r + 1).pow(-1 / 0.05).long().clamp_(1, rows) - 1)
    if hot:
        ids[torch.randperm(n, device=DEV, generator=gen)[:hot]] = rows // 3
    ids[0], ids[-1] = 0, rows - 1
    return ids


def _seed_state(fm, opt, parts, gen):
    """Nonzero moments on every row of both tables and on the mapping (of the scale of the first step's gradients), the source
    table at update SRC_STEP, the target at TGT_STEP, every mapping parameter at a count of its own."""
    fm.sstate.step, fm.tstate.step = SRC_STEP, TGT_STEP
    if opt != 'adam':
        return

    def fill(m, v, scale):
        m.copy_(torch.randn(m.shape, device=DEV, generator=gen) * scale)
        v.copy_((0.25 + 4 * torch.rand(v.shape, device=DEV, generator=gen)) * scale * scale)
    _, sp, tp, pp = parts
    for st, part in ((fm.sstate, sp), (fm.tstate, tp)):
        fill(st.exp_avg, st.exp_avg_sq, float(part[1].pow(2).mean().sqrt()))
    for c, ((W, b, _), (gW, gb)) in enumerate(zip(fm.layers, pp)):
        for k, (p, g) in enumerate(((W, gW), (b, gb))):
            if p is None:
                continue
            st = fm.map_opt.state[p]
            st['step'] = torch.full((1,), 411 + 97 * c + 58 * k, device=DEV, dtype=torch.int64)
            st['exp_avg'], st['exp_avg_sq'] = torch.empty_like(p), torch.empty_like(p)
            fill(st['exp_avg'], st['exp_avg_sq'], float(g[0].pow(2).mean().sqrt()))


def _table_snapshot(st, opt):
    d = {'w': st.table.clone()}
    if opt == 'adam':
        d['m'], d['v'] = st.exp_avg.clone(), st.exp_avg_sq.clone()
    return d


def _table_live(st, opt):
    d = {'w': st.table}
    if opt == 'adam':
        d['m'], d['v'] = st.exp_avg, st.exp_avg_sq
    return d


def _param_snapshot(fm, opt):
    out = []
    for W, b, _ in fm.layers:
        for p in (W, b):
            if p is None:
                out.append(None)
                continue
            d = {'w': p.detach().reshape(p.shape[0] if p.dim() == 2 else 1, -1).clone()}
            if opt == 'adam':
                st = fm.map_opt.state[p]
                d['m'], d['v'] = st['exp_avg'].reshape(d['w'].shape).clone(), st['exp_avg_sq'].reshape(d['w'].shape).clone()
                d['step'] = int(st['step'])
            out.append(d)
    return out


def _ratio_max(tag, got, ref, bound):
    assert bool(torch.isfinite(got).all()), f'{tag}: non-finite values'
    r = (got.double() - ref).abs() / bound
    w = float(r.max())
    if w > 1.0:
        j = int(r.argmax())
        row, col = j // r.shape[1], j % r.shape[1]
        raise AssertionError(f'{tag}: error / bound = {w:.3g} at [{row}, {col}]: got {float(got[row, col])!r} want '
                             f'{float(ref[row, col])!r} bound {float(bound[row, col]):.3g}')
    return w


def _check_table(tag, before, after, rows, want):
    """Touched rows within their bounds; every other row bit-identical, its two neighbours in particular."""
    nrows = before['w'].shape[0]
    touched = torch.zeros(nrows, dtype=torch.bool, device=rows.device)
    touched[rows] = True
    nb = torch.cat([rows - 1, rows + 1]).clamp(0, nrows - 1)
    nb = nb[~touched[nb]]
    worst = {}
    for name, t0 in before.items():
        t1 = after[name]
        bad = (t0.view(torch.int32) != t1.view(torch.int32)).any(1) & ~touched
        assert not bool(bad.any()), f'{tag}.{name}: {int(bad.sum())} rows outside the batch written, e.g. row {int(torch.nonzero(bad)[0])}'
        assert torch.equal(t0[nb].view(torch.int32), t1[nb].view(torch.int32)), f'{tag}.{name}: a neighbour of a touched row moved'
        ref, bound = want[name]
        worst[name] = _ratio_max(f'{tag}.{name}', t1[rows], ref, bound)
    return worst


def _fmt(worst):
    return ' '.join(f'{k}={v:.3g}' for k, v in worst.items())


def _merge(worst, prefix, w):
    for k, v in w.items():
        worst[f'{prefix}.{k}'] = max(worst.get(f'{prefix}.{k}', 0.0), v)


def _run(fm, batches, hp, tag, unique, depth_fn, run=None):
    """Drives the steps (``run(idx)``, default fm.step) and checks each against the fp64 step from the device's state before it.
    hp = (opt, lr, betas, eps, weight_decay) as the step was built with."""
    opt, lr, betas, eps, wd = hp
    adam = opt == 'adam'
    hp = dict(b1=betas[0], b2=betas[1], eps=eps)
    run = run or (lambda i: fm.step(i, unique=unique))
    worst = {}
    for k, idx in enumerate(batches):
        n = idx.numel()
        parts = map_grads_fp64(fm.S, fm.T, fm.layers, idx)
        if k == 0:
            _seed_state(fm, opt, parts, torch.Generator(device=DEV).manual_seed(n))
        loss, sp, tp, pp = parts
        cs, ct = fm.sstate.step, fm.tstate.step
        bs, bt = _table_snapshot(fm.sstate, opt), _table_snapshot(fm.tstate, opt)
        bp = _param_snapshot(fm, opt)
        ws = apply_fp64(bs, sp[:5], sp[5], opt, lr, wd, cs + 1, **hp)
        wt = apply_fp64(bt, tp[:5], tp[5], opt, lr, wd, ct + 1, **hp)
        wps = []
        for q, snap in enumerate(bp):
            if snap is None:
                wps.append(None)
                continue
            G, A, E = pp[q // 2][q % 2]
            if q % 2:
                G, A, E = G.view(1, -1), A.view(1, -1), E.view(1, -1)
            prow = torch.arange(G.shape[0], device=DEV)
            part = (prow, G, A, E, torch.zeros_like(prow))
            wps.append(apply_fp64(snap, part, depth_fn(n, bool(q % 2)), opt, lr, wd, (snap['step'] + 1) if adam else 1, **hp))
        got = float(run(idx.view(-1, 1)))
        torch.cuda.synchronize()
        assert abs(got - loss) <= LOSS_RTOL * abs(loss), f'{tag} step {k + 1}: loss {got!r} vs fp64 {loss!r}'
        assert fm.sstate.step == cs + 1 and fm.tstate.step == ct + 1, f'{tag}: host update counts'
        for st, c in ((fm.sstate, cs), (fm.tstate, ct)):
            if st._step_dev is not None:
                assert int(st._step_dev) == c + 1, f'{tag}: device update count {int(st._step_dev)} != {c + 1}'
        _merge(worst, 'S', _check_table(f'{tag} step {k + 1} S', bs, _table_live(fm.sstate, opt), sp[0], ws))
        _merge(worst, 'T', _check_table(f'{tag} step {k + 1} T', bt, _table_live(fm.tstate, opt), tp[0], wt))
        q = 0
        for l, (W, b, _) in enumerate(fm.layers):
            for name, p in (('W', W), ('b', b)):
                snap, want = bp[q], wps[q]
                q += 1
                if p is None:
                    continue
                live = {'w': p.detach().reshape(snap['w'].shape)}
                if adam:
                    st = fm.map_opt.state[p]
                    assert int(st['step']) == snap['step'] + 1, f'{tag}: {name}{l} update count'
                    live['m'], live['v'] = st['exp_avg'].reshape(snap['w'].shape), st['exp_avg_sq'].reshape(snap['w'].shape)
                w = {k2: _ratio_max(f'{tag} step {k + 1} {name}{l}.{k2}', live[k2], *want[k2]) for k2 in want}
                _merge(worst, f'{name}{l}', w)
        del parts, sp, tp, pp, bs, bt, bp, ws, wt, wps
    print(f'\n{tag}: worst error / bound over {len(batches)} steps: {_fmt(worst)}')
    return worst


def _build(dims, bias, n, rows, optname, seed, misalign=False):
    from recbole_cdr_amd.fused import FusedMapStep
    opt, lr, betas, eps, wd = OPTS[optname]
    gen = torch.Generator(device=DEV); gen.manual_seed(seed)
    S = torch.empty(rows, dims[0], device=DEV).normal_(0, 0.5, generator=gen)
    T = torch.empty(rows, dims[-1], device=DEV).normal_(0, 0.5, generator=gen)
    layers, params, fn = _make_mapping(dims, bias, gen, misalign)
    fm = FusedMapStep(S, T, fn, params, n, opt=opt, lr=lr, betas=betas, eps=eps, weight_decay=wd, layers=layers)
    assert fm.layers is not None, 'the mapping must have a distinct-id path'
    return fm, gen


def _per_cu(dims, bias, misalign):
    """cdr_map_step_unique's workgroups per CU: 1 for the two-wave-group kernels (`pipe`: linear without bias, Ds == Dt in {64, 128};
    `mlp`: tanh D-H-D, D and H in {64, 128}, biases on both layers or on neither; 16-byte aligned weights), else 2."""
    if misalign or dims[0] != dims[-1] or dims[0] not in (64, 128):
        return 2
    if len(dims) == 2:
        return 1 if not bias else 2
    return 1 if len(dims) == 3 and dims[1] in (64, 128) else 2


def _unique_case(dims, bias, n, optname, misalign=False, rows=None):
    rows = rows or n + n // 3 + 64
    fm, gen = _build(dims, bias, n, rows, optname, seed=sum(dims) + n + 7 * misalign)
    per_cu = _per_cu(dims, bias, misalign)
    batches = [_distinct_ids(n, rows, gen) for _ in range(3)]
    tag = f'unique {"-".join(map(str, dims))}{"" if bias else " no-bias"}{" misaligned" if misalign else ""} n={n} {optname}'
    _run(fm, batches, OPTS[optname], tag, True, lambda m, is_b: _unique_depth(m, per_cu, is_b))


# ---------------------------------------------------------------------------------------------------------------------- distinct ids

SWEEP = [(1, 'sgd'), (31, 'adam'), (33, 'adam_wd'), (100, 'adam'), (8191, 'sgd_wd'), (8192, 'adam_hp'), (8193, 'adam'),
         (16385, 'adam_wd'), (65536, 'adam'), (65536, 'adam_hp'), (65536, 'sgd_wd'), (262147, 'adam')]


@pytest.mark.parametrize('n,optname', SWEEP)
def test_map_pipe_linear_128_vs_fp64(n, optname):
    """map_pipe_kernel<4>: linear 128 x 128 without bias (the benchmark's headline OVERLAP leg)."""
    _unique_case((128, 128), False, n, optname)


@pytest.mark.parametrize('n,optname', SWEEP)
def test_map_pipe3_tanh_128_vs_fp64(n, optname):
    """map_pipe3_kernel<4, 4>: tanh 128-128-128 with biases (the reference's default mapping; the benchmark's non_linear leg)."""
    _unique_case((128, 128, 128), True, n, optname)


# (dims, bias, misaligned weight, ragged size, its optimizer): the branch of cdr_map_step_unique each one takes
SHAPES = [
    ((64, 64), False, False, 20011, 'adam_hp'),             # map_pipe_kernel<2>
    ((128, 64, 128), True, False, 8193, 'sgd'),             # map_pipe3_kernel<4, 2>
    ((64, 128, 64), True, False, 16385, 'adam'),            # map_pipe3_kernel<2, 4>
    ((64, 64, 64), True, False, 33, 'adam_hp'),             # map_pipe3_kernel<2, 2>
    ((128, 128, 128), False, False, 8193, 'adam_hp'),       # map_pipe3_kernel<4, 4>, bias-free (biases on both layers or on neither)
    ((128, 64), False, False, 16385, 'sgd_wd'),             # map_step_kernel<4> (Ds != Dt: 8 tiles)
    ((128, 96, 128), True, False, 8193, 'adam'),            # map_step_kernel<8> (12 + 12 = 24 tiles > 16)
    ((64, 48, 32, 64), True, False, 16385, 'adam_hp'),      # map_step_kernel<4> (three layers: 4 + 2 + 2 tiles)
    ((128, 128), False, True, 8193, 'adam'),                # map_step_kernel<4>: weight 4 B off 16-B alignment -> net.vec == 0
]


@pytest.mark.parametrize('dims,bias,misalign,ragged,optname', SHAPES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize('at', ['65536', 'ragged'])
def test_map_step_unique_shapes_vs_fp64(dims, bias, misalign, ragged, optname, at):
    n, o = (65536, 'adam_wd') if at == '65536' else (ragged, optname)
    _unique_case(dims, bias, n, o, misalign)


def test_map_step_unique_ids_above_2_24_vs_fp64():
    """D = 64 (linear, and tanh 64-64-64) on tables of 2^24 + 4,099 rows: half of the 8,193 distinct ids above 2^24 (all that
    4,099 rows above it allow), 2^24 + 1 and rows - 1 among them.  An fp32 cannot hold such an id and at D = 64 their row offsets
    pass 2^32 bytes."""
    nrows, n = (1 << 24) + 4099, 8193
    gc.collect()
    torch.cuda.empty_cache()
    free_b, _ = torch.cuda.mem_get_info()
    if free_b < 60e9:
        pytest.skip('needs ~60 GB of free HBM (two 2^24-row tables with Adam moments and their snapshots)')
    for dims, bias in (((64, 64), False), ((64, 64, 64), True)):
        fm, gen = _build(dims, bias, n, nrows, 'adam_wd', seed=24 + len(dims))
        batches = []
        for _ in range(3):
            lo = torch.randperm(1 << 24, device=DEV, generator=gen)[:n - 4097]
            keep = torch.ones(4099, dtype=torch.bool, device=DEV)
            keep[2 + torch.randperm(4096, device=DEV, generator=gen)[:2]] = False      # offsets 0, 1 and 4,098 (= rows - 1) stay
            hi = (1 << 24) + torch.nonzero(keep).view(-1)
            ids = torch.cat([lo, hi])
            assert torch.unique(ids).numel() == n and int((ids > 1 << 24).sum()) >= n // 2 and int(ids.max()) == nrows - 1
            batches.append(ids[torch.randperm(n, device=DEV, generator=gen)])
        _run(fm, batches, OPTS['adam_wd'], f'unique {"-".join(map(str, dims))} rows={nrows} n={n} adam_wd', True,
             lambda m, is_b: _unique_depth(m, 1, is_b))
        del fm, batches
        gc.collect()
        torch.cuda.empty_cache()


def test_map_step_unique_graph_replay_vs_fp64():
    """capture / replay at OB = 100 (the reference's overlap_batch_size): every replay fp64-checked, update counts on the device."""
    n, rows = 100, 400
    fm, gen = _build((128, 128, 128), True, n, rows, 'adam_hp', seed=100)
    batches = [_distinct_ids(n, rows, gen) for _ in range(3)]
    state = {}

    def run(idx):
        if 'graph' not in state:                        # after _run has seeded the state: capture once, replay every step
            fm.capture(n)
            state['graph'] = True
        return fm.replay(idx)
    _run(fm, batches, OPTS['adam_hp'], 'replay 128-128-128 n=100 adam_hp', True, lambda m, is_b: _unique_depth(m, 1, is_b), run=run)


# ---------------------------------------------------------------------------------------------------------------------- general path

@pytest.mark.parametrize('dims,bias,n,hot,optname', [
    ((128, 128), False, 65536, 5000, 'adam_wd'), ((128, 128, 128), True, 65536, 5000, 'adam_hp'),
    ((128, 128), False, 100, 0, 'sgd_wd'), ((128, 128, 128), True, 100, 0, 'adam')])
def test_map_step_general_path_vs_fp64(dims, bias, n, hot, optname):
    """step(idx) without ``unique``: gather, functional.linear, mse_loss, the id sort, cdr_rowwise_apply (one update per row from its
    summed gradient) and DenseAdam / SGD on the mapping, on Zipf-repeated ids (one id ~5,000 times at 65,536)."""
    rows = max(n, 2048)
    fm, gen = _build(dims, bias, n, rows, optname, seed=sum(dims) + n + 1)
    batches = [_repeated_ids(n, rows, gen, hot) for _ in range(3)]
    assert int(torch.bincount(batches[0]).max()) >= (hot or 2)
    _run(fm, batches, OPTS[optname], f'general {"-".join(map(str, dims))} n={n} hot={hot} {optname}', False, _general_depth)


# ---------------------------------------------------------------------------------------------------------------------- model wiring

def test_emcdr_fused_overlap_step_vs_fp64():
    """EMCDR.fused_train_step in the OVERLAP phase with the non-linear mapping and weight_decay in the config: the hyper-parameters
    CrossDomainTrainer hands the model (_fused_kw) reach FusedMapStep's kernels."""
    from oracle.common import IdSpace
    from recbole_cdr_amd.model.cross_domain_recommender.emcdr import EMCDR
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    D, n, wd, lr = 128, 65536, 1e-2, 1e-3
    ids = IdSpace(OU=90001, TOU=5000, SOU=5000, OI=1, TOI=3000, SOI=3000)
    cfg = base_config(DEV, latent_factor_model='BPR', source_embedding_size=D, target_embedding_size=D, reg_weight=1e-3,
                      mapping_function='non_linear', mlp_hidden_size=[D], learning_rate=lr, weight_decay=wd, optimizer_mode='rowwise',
                      train_modes=['SOURCE', 'TARGET', 'OVERLAP'], epoch_num=['1', '1', '1'], source_split=False, eval_step=1, epochs=1)
    torch.manual_seed(5)
    model = EMCDR(cfg, FakeDataset(ids)).to(DEV)
    model.set_phase('OVERLAP')
    kw = CrossDomainTrainer(cfg, model)._fused_kw()
    assert kw['weight_decay'] == wd and kw['lr'] == lr
    gen = torch.Generator(device=DEV); gen.manual_seed(6)
    first = 1 + torch.randperm(ids.OU - 1, device=DEV, generator=gen)[:n]
    model.fused_train_step({'overlap': first.view(-1, 1)}, **kw)             # builds the step and its states
    fm = model._fused['steps'][('map', 'user')]
    assert fm.layers is not None and fm.wd == wd and fm.lr == lr
    batches = [1 + _distinct_ids(n, ids.OU - 1, gen) for _ in range(3)]                    # ids 1 and OU - 1 in every batch
    _run(fm, batches, ('adam', lr, (0.9, 0.999), 1e-8, wd), f'EMCDR.fused_train_step OVERLAP non_linear D={D} n={n} wd={wd}', True,
         lambda m, is_b: _unique_depth(m, 1, is_b), run=lambda idx: model.fused_train_step({'overlap': idx}, **kw))


@pytest.fixture(scope='module', autouse=True)
def _release_device_memory():
    """The big cases leave tens of GB in torch's caching allocator: hand it back, so that later modules' free-HBM checks see what
    they saw without this module."""
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f'\nmap-step fp64 module: peak device memory {torch.cuda.max_memory_allocated() / 1e9:.1f} GB')
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
