"""The DIMENSION-sharded BPR and pointwise steps (dimshard.NativeDimOps / NativePointDimOps: cdr_ids_pack32 / cdr_ids_unpack32,
cdr_bpr_partial_diff, cdr_bpr_step_presort + cdr_bpr_step_from_diff -- the XD instantiations of bpr_fwd_apply_kernel -- or, two-pass,
cdr_sort_ids_two_tables + cdr_bpr_grad_from_diff + cdr_rowwise_apply, and their pointwise twins) against the float64 restatement of the
ONE-GPU step on the assembled tables (dim_loopback.assemble_cols) and the concatenated batch, at worlds 1, 2, 3, 4, 5 and 8 in one process
(tests/dim_loopback.py: G emulated ranks, the all-gather as a torch.cat, the all-reduce as one fp32 sum).

Teacher forcing as in test_gpu_shard_fp64.py: each of the three steps of a case is judged from the assembled device state before it; steps
2 and 3 reuse rows, so the bias corrections of updates 2 and 3 are checked.  Per step: the touched rows of every column slice and their
moments within fp64_bounds.apply_fp64's per-element bounds (columns [r Ds, (r + 1) Ds) of the reference and of the bound); every other row
of every slice and of its moments -- both neighbours of every touched row among them -- bit-identical to its value before the step; the loss
of every rank to LOSS_RTOL; out[4:6] of every rank to its relative bound (exactly 0 without EmbLoss); out[:9] bit-identical across the ranks
(every rank runs the same arithmetic on the same all-reduced buffer with the same grid); both update counts of every rank == t; the
unpacked ids == the torch.cat of the ranks' ids, the unpacked labels == the ranks' labels as int32 bit patterns, no out-of-range flag.  No
blanket atol anywhere.

What the layout adds to the one-GPU bounds (test_gpu_step_fp64.py's docstring), counted from csrc/cdr_dimshard.hip:
  * Score.  bpr_partial_diff_kernel: a rank's <u, p> and <u, n> over its Ds columns are dot4 (4 products, 3 additions) per lane and
    log2(lanes) additions of group_sum -- Ds products and Ds - 1 additions whatever the order: gamma_Ds of the sum of magnitudes -- and
    ``diff[t] = dp - dn`` rounds once more (K_DIFF = 1).  The all-reduce adds the ranks' values: world - 1 additions (_allreduce_adds).
    So e_x = gamma_{Ds + K_DIFF + world - 1} (sum|u p| + sum|u n|) + u |x| = gamma_{Ds + world}; the pointwise dot has no difference:
    gamma_{Ds + world - 1}.  Passed as ``k_score``; it is <= the one-GPU D + 2 in every case here (asserted), so no bound is loosened.
  * EmbLoss coefficient.  A rank's row sums are fp32 lane-group sums of Ds squares (fewer than the one-GPU D: the D of gamma_{D + K_REG}
    stays), added in fp64 per rank; partial_norms_kernel rounds the rank's sum to fp32 (K_RANK_SUM = 1) and the all-reduce adds world - 1
    times, before coef_finish_kernel's sqrtf and two operations (inside K_REG): k_reg_extra = 1 + (world - 1), as the row shard.
  * Gradient rows, moments, weights: nothing new -- every element lives on one rank and goes through the one-GPU kernels on [rows, Ds].

Ids 0 and rows - 1 of both tables are in every batch and ~1 % of the triples have p == n (_mark_edges); cases h and i, whose ids are
placed by hand, carry rows 0 and rows - 1 of both tables and triples with p == n (i: one of its three; h: the two items that occur twice sit
in one triple each, and the long item segments meet themselves in ~0.5-1 % of the triples by chance).  Every rank brings the same Bl.

The batch builders and the checks take their device from the generator and the tensors they are given, never from helpers.DEV:
test_dim_loopback_host.py runs this checker on CPU tensors and shows that it rejects five mutated stand-ins.

Measured on the MI355X (worst error / bound over three steps and all ranks, every case and both forms): loss <= 0.012, coefficients
<= 0.122 (case i; <= 0.058 elsewhere), weights <= 0.497, first moments <= 0.123, second moments <= 0.304; per case in DESIGN.md section 2."""
import ctypes

import pytest
import torch

from dim_loopback import DimLoopback, assemble_cols, rank_state
from fp64_bounds import K_REG, LOSS_RTOL, apply_fp64, bpr_grads_fp64, gam, point_grads_fp64
from helpers import DEV
from test_gpu_shard_fp64 import SEG_LENGTHS, _check_table, _fmt, _mark_edges, _with_counts, _zipf

pytestmark = pytest.mark.gpu

K_DIFF = 1                  # diff[t] = dp - dn: one rounding on top of the two Ds-term dot products
K_RANK_SUM = 1              # a rank's fp64 norm sum rounded to fp32 (partial_norms_kernel) before the all-reduce


def _allreduce_adds(world):
    """fp32 additions an all-reduced value goes through."""
    return world - 1


def k_score(point, Ds, world):
    return Ds + (0 if point else K_DIFF) + _allreduce_adds(world)


# ---------------------------------------------------------------------------------------------------------------------- batches

def _split_even(fields, world):
    Bl = fields[0].numel() // world
    assert Bl * world == fields[0].numel()
    return [tuple(f[r * Bl:(r + 1) * Bl].contiguous() for f in fields) for r in range(world)]


def _uniform(B, nu, ni, gen):
    dev = gen.device
    return (torch.randint(0, nu, (B,), device=dev, generator=gen), torch.randint(0, ni, (B,), device=dev, generator=gen),
            torch.randint(0, ni, (B,), device=dev, generator=gen))


def _shuffled(fields, gen):
    """(the edge ids _mark_edges puts into the first six rows end up on whichever rank)"""
    o = torch.randperm(fields[0].numel(), device=gen.device, generator=gen)
    return tuple(f[o] for f in fields)


def _batch_uniform(c, t, gen):
    u, p, n = _uniform(c['world'] * c['Bl'], c['nu'], c['ni'], gen)
    if c.get('zipf'):
        p = _zipf(u.numel(), c['ni'], gen)
    _mark_edges(u, p, n, c['nu'], c['ni'], gen)
    return _split_even(_shuffled((u, p, n), gen), c['world'])


def _batch_d(c, t, gen):
    """Half of all triples share one user; one item is a third of the positives and 600 of the negatives."""
    B, dev = c['world'] * c['Bl'], gen.device
    u, p, n = _uniform(B, c['nu'], c['ni'], gen)
    u[torch.randperm(B, device=dev, generator=gen)[:B // 2]] = c['nu'] // 2
    p[torch.randperm(B, device=dev, generator=gen)[:B // 3]] = c['ni'] // 3
    n[torch.randperm(B, device=dev, generator=gen)[:600]] = c['ni'] // 3
    _mark_edges(u, p, n, c['nu'], c['ni'], gen)
    return _split_even(_shuffled((u, p, n), gen), c['world'])


def _batch_h(c, t, gen):
    """User rows and item rows with exactly 32 / 33 / 255 / 256 / 257 / 513 occurrences (kLongSeg and kPiece from both sides, a segment of
    three pieces); the two items that occur twice sit in one triple each (p == n); rows 0 and rows - 1 replace ids that occur once."""
    B, nu, ni, dev = c['world'] * c['Bl'], c['nu'], c['ni'], gen.device
    u = _with_counts(SEG_LENGTHS, B, torch.arange(1, nu - 1, device=dev), gen)
    items = _with_counts(SEG_LENGTHS, 2 * B, torch.arange(1, ni - 1, device=dev), gen)
    twice = torch.nonzero(torch.bincount(items, minlength=ni) == 2).flatten()
    assert twice.numel() == 2
    for k, x in enumerate(twice.tolist()):                               # a permutation of ``items``: the counts stay
        pair = (10 + k, B + 10 + k)
        for dst in pair:
            if int(items[dst]) != x:
                src = next(q for q in torch.nonzero(items == x).flatten().tolist() if q not in pair)
                items[src], items[dst] = int(items[dst]), x
    p, n = items[:B].clone(), items[B:].clone()
    once_u = torch.nonzero(torch.bincount(u, minlength=nu)[u] == 1).flatten()
    u[once_u[0]], u[once_u[1]] = 0, nu - 1
    once_p = torch.nonzero(torch.bincount(items, minlength=ni)[p] == 1).flatten()
    p[once_p[0]], p[once_p[1]] = 0, ni - 1
    return _split_even((u, p, n), c['world'])


def _batch_i(c, t, gen):
    """Bg = 3, one triple per rank, by hand: rows 0 and rows - 1 of both tables (item 0 and item ni - 1 once as a positive and once as a
    negative: two duplicate segments of two), p == n on rank 2, whose user changes from step to step."""
    nu, ni, dev = c['nu'], c['ni'], gen.device
    rows = [(0, 0, ni - 1), (nu - 1, ni - 1, 0), (3 + t, 5, 5)]
    return [tuple(torch.tensor([x], device=dev) for x in r) for r in rows]


def _batch_point(c, t, gen):
    """(user, item, label): Zipf items in step 2; ratings in [0, 5) or labels 0 / 1; ``odd_labels``: -0.0, a denormal and a negative rating
    (bit patterns an integer round trip that is not a bit copy would change)."""
    B, nu, ni, dev = c['world'] * c['Bl'], c['nu'], c['ni'], gen.device
    u = torch.randint(0, nu, (B,), device=dev, generator=gen)
    i = _zipf(B, ni, gen) if t == 2 else torch.randint(0, ni, (B,), device=dev, generator=gen)
    _mark_edges(u, i, None, nu, ni, gen)
    r = torch.rand(B, device=dev, generator=gen)
    y = r * 5 if c['labels'] == 'ratings' else (r < 0.5).float()
    if c.get('odd_labels'):
        y[7:10] = torch.tensor([-0.0, 1e-40, -3.5], dtype=torch.float32).to(dev)
        assert [int(v) for v in y[7:10].view(torch.int32).tolist()][:2] == [-2 ** 31, 71362], 'the odd labels did not survive the batch builder'
    return _split_even(_shuffled((u, i, y), gen), c['world'])


# reg = 0.02 (BPR) / 0.01 (pointwise) and wd = 0 unless given; Bg = world * Bl
CASES = {
    'a': dict(world=1, D=64, opt='adam', Bl=4097, nu=3001, ni=2501, batch=_batch_uniform, anchor=True),
    'b': dict(world=2, D=256, opt='adam', Bl=45000, nu=60001, ni=40001, batch=_batch_uniform, zipf=True),
    'c': dict(world=2, D=512, opt='adam', wd=0.01, Bl=1200, nu=2001, ni=1501, batch=_batch_uniform),
    'd': dict(world=4, D=128, opt='adam', Bl=1000, nu=2003, ni=1501, batch=_batch_d),
    'e': dict(world=8, D=128, opt='adam', Bl=600, nu=3003, ni=2505, batch=_batch_uniform, zipf=True),
    'f': dict(world=8, D=32, opt='adam', reg=0.0, Bl=300, nu=1501, ni=1203, batch=_batch_uniform),
    'g': dict(world=3, D=24, opt='sgd', wd=0.01, Bl=900, nu=2000, ni=1501, batch=_batch_uniform),
    'h': dict(world=5, D=60, opt='adam', Bl=777, nu=3001, ni=7001, batch=_batch_h),
    'i': dict(world=3, D=12, opt='adam', Bl=1, nu=17, ni=13, batch=_batch_i),
}
TWO_PASS = ('b', 'd', 'g', 'h')
POINT_CASES = {
    'w1': dict(world=1, D=64, loss='mse', Bl=2048, nu=4096, ni=1024, labels='ratings', odd_labels=True, batch=_batch_point, anchor=True),
    'w3': dict(world=3, D=96, loss='mse', wd=0.01, Bl=2500, nu=5001, ni=2001, labels='ratings', batch=_batch_point),
    'w8': dict(world=8, D=128, loss='bce', Bl=700, nu=4001, ni=1501, labels='binary', batch=_batch_point),
    'w2': dict(world=2, D=256, loss='bce', Bl=66000, nu=100001, ni=50001, labels='binary', batch=_batch_point),
}
POINT_TWO_PASS = ('w3',)


# ---------------------------------------------------------------------------------------------------------------------- driver

def _native_ops(run, rank, Uc, Ic, Bg):
    import recbole_cdr_amd  # noqa: F401
    from recbole_cdr_amd.dimshard import NativeDimOps, NativePointDimOps
    kw = dict(opt=run.opt, lr=run.lr, weight_decay=run.wd, reg_weight=run.reg, fuse_singles=run.form == 'fused')
    ops = NativePointDimOps(Uc, Ic, Bg, loss=run.c['loss'], **kw) if run.point else NativeDimOps(Uc, Ic, Bg, **kw)
    assert ops.fused == (run.form == 'fused')
    return ops


class _Run:
    """One case: the column slices of seeded tables on ``dev``, one ops object per rank (``make_ops(run, rank, Uc, Ic, Bg)``; default: the
    native kernels) and the loopback over them."""

    def __init__(self, name, c, form='fused', dev=None, make_ops=None):
        dev = torch.device(DEV if dev is None else dev)
        self.c, self.name, self.form, self.dev = c, name, form, dev
        self.point = 'loss' in c
        G, D = c['world'], c['D']
        assert D % (4 * G) == 0
        self.Ds = Ds = D // G
        self.gen = torch.Generator(device=dev); self.gen.manual_seed(sum(map(ord, name)) + D)
        U = torch.empty(c['nu'], D, device=dev).normal_(0, c.get('scale', 0.1), generator=self.gen)
        I = torch.empty(c['ni'], D, device=dev).normal_(0, c.get('scale', 0.1), generator=self.gen)
        self.opt = c.get('opt', 'adam')
        self.lr, self.wd, self.reg = (1e-3 if self.opt == 'adam' else 0.5), c.get('wd', 0.0), c.get('reg', 0.01 if self.point else 0.02)
        self.Us = [U[:, r * Ds:(r + 1) * Ds].contiguous() for r in range(G)]
        self.Is = [I[:, r * Ds:(r + 1) * Ds].contiguous() for r in range(G)]
        make = make_ops if make_ops is not None else _native_ops
        self.ops = [make(self, r, self.Us[r], self.Is[r], G * c['Bl']) for r in range(G)]
        self.lb = DimLoopback(self.ops, c['Bl'], pointwise=self.point)
        self.k_score = k_score(self.point, Ds, G)
        assert self.k_score <= D + 2, 'the layout never loosens the one-GPU score bound'
        what = f"point {c['loss']}" if self.point else 'bpr'
        self.tag = f'{what} case {name} {form}: world={G} D={D} (Ds={Ds}) {self.opt} wd={self.wd} reg={self.reg}'

    def _tables(self, clone):
        out = []
        for ops in self.ops:
            pair = []
            for tab, m, v, _ in rank_state(ops):
                d = {'w': tab, 'm': m, 'v': v} if self.opt == 'adam' else {'w': tab}
                pair.append({k: x.clone() for k, x in d.items()} if clone else d)
            out.append(pair)
        return out

    def checked_step(self, t, worst):
        c, G, D, Ds = self.c, self.c['world'], self.c['D'], self.Ds
        batches = c['batch'](c, t, self.gen)
        a, b, y = (torch.cat([x[k] for x in batches]) for k in range(3))
        before = self._tables(clone=True)
        bu = {k: assemble_cols([before[r][0][k] for r in range(G)]) for k in before[0][0]}
        bi = {k: assemble_cols([before[r][1][k] for r in range(G)]) for k in before[0][1]}
        detail = {}
        k_reg_extra = K_RANK_SUM + _allreduce_adds(G)
        if self.point:
            loss, upart, ipart = point_grads_fp64(bu['w'], bi['w'], a, b, y, self.reg, c['loss'], detail=detail, k_reg_extra=k_reg_extra,
                                                  k_score=self.k_score)
        else:
            loss, upart, ipart = bpr_grads_fp64(bu['w'], bi['w'], a, b, y, self.reg, detail=detail, k_reg_extra=k_reg_extra, k_score=self.k_score)
        wu = apply_fp64(bu, upart, D, self.opt, self.lr, self.wd, t)
        wi = apply_fp64(bi, ipart, D, self.opt, self.lr, self.wd, t)
        rec = self.lb.step(batches)
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()
        tag = f'{self.tag} step {t}'
        out0 = rec['out'][0]
        for r in range(G):
            ids, out = rec['ids'][r], rec['out'][r]
            assert torch.equal(ids[0], a) and torch.equal(ids[1], b), f'{tag}: gathered ids on rank {r} are not the ranks\' ids in rank order'
            if self.point:
                assert torch.equal(rec['labels'][r].view(torch.int32), y.view(torch.int32)), f'{tag}: gathered labels on rank {r} are not the ranks\' labels bit for bit'
            else:
                assert torch.equal(ids[2], y), f'{tag}: gathered negatives on rank {r}'
            fit = getattr(self.ops[r], 'ids_fit', None)
            assert fit is None or fit(), f'{tag}: out-of-range flag set on rank {r}'
            got = float(out[0])
            assert abs(got - loss) <= LOSS_RTOL * abs(loss), f'{tag}: loss on rank {r} {got!r} vs fp64 {loss!r}'
            worst['loss'] = max(worst.get('loss', 0.0), abs(got - loss) / (LOSS_RTOL * abs(loss)))
            for k, name in ((4, 'cu'), (5, 'ci')):
                gc, wc = float(out[k]), detail[name]
                if wc == 0.0:
                    assert gc == 0.0, f'{tag}: coefficient {name} on rank {r} is {gc!r} without EmbLoss'
                    continue
                assert detail['gc'] == gam(D + K_REG + K_RANK_SUM + _allreduce_adds(G))
                ratio = abs(gc - wc) / (detail['gc'] * abs(wc))
                assert ratio <= 1.0, f'{tag}: coefficient {name} on rank {r}: got {gc!r} want {wc!r}, error / bound = {ratio:.3g}'
                worst['coef'] = max(worst.get('coef', 0.0), ratio)
            assert torch.equal(out[:9].view(torch.int32), out0[:9].view(torch.int32)), f'{tag}: out[:9] of rank {r} differs from rank 0: {out[:9].tolist()} vs {out0[:9].tolist()}'
            counts = [s[3] for s in rank_state(self.ops[r])]
            assert counts == [t, t], f'{tag}: update counts on rank {r} are {counts}'
        after = self._tables(clone=False)
        for r in range(G):
            cols = slice(r * Ds, (r + 1) * Ds)
            for k, name, part, want in ((0, 'U', upart, wu), (1, 'I', ipart, wi)):
                wt = _check_table(f'{tag} {name} rank {r}', before[r][k], after[r][k], part[0], {q: (v[0][:, cols], v[1][:, cols]) for q, v in want.items()})
                for q, v in wt.items():
                    worst[f'{name}.{q}'] = max(worst.get(f'{name}.{q}', 0.0), v)
        return rec, batches


def run_case(name, c, form='fused', dev=None, make_ops=None, steps=(1, 2, 3)):
    """The whole check of one case (what the CPU tests drive with stand-in ops); returns (run, worst error / bound per quantity)."""
    run = _Run(name, c, form, dev, make_ops)
    worst = {}
    for t in steps:
        run.checked_step(t, worst)
    return run, worst


def _twin(run):
    """The product's own step object on clones of the one rank's tables (world 1, no process group)."""
    from recbole_cdr_amd.dimshard import DimShardedBPRStep, DimShardedPointStep
    c = run.c
    kw = dict(opt=run.opt, lr=run.lr, weight_decay=run.wd, reg_weight=run.reg)
    if run.point:
        return DimShardedPointStep(run.Us[0].clone(), run.Is[0].clone(), c['Bl'], loss=c['loss'], **kw)
    return DimShardedBPRStep(run.Us[0].clone(), run.Is[0].clone(), c['Bl'], **kw)


def _same_bits(tag, a, b):
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{tag} differs'


def _drive(name, c, form):
    run = _Run(name, c, form)
    twin = _twin(run) if c.get('anchor') and form == 'fused' else None
    worst = {}
    for t in (1, 2, 3):
        rec, batches = run.checked_step(t, worst)
        if twin is not None:
            # the loopback at world 1, pack / unpack included, against the product's step: pins the loopback's stage order to the product's
            out = twin.step(*batches[0])
            torch.cuda.synchronize()
            _same_bits(f'{run.tag} step {t}: out[:9] of the loopback and of {type(twin).__name__}', rec['out'][0][:9], out[:9])
            for mine, theirs, which in zip(rank_state(run.ops[0]), (twin.ustate, twin.istate), 'UI'):
                _same_bits(f'{run.tag} step {t}: table {which}', mine[0], theirs.table)
                _same_bits(f'{run.tag} step {t}: exp_avg {which}', mine[1], theirs.exp_avg)
                _same_bits(f'{run.tag} step {t}: exp_avg_sq {which}', mine[2], theirs.exp_avg_sq)
                assert mine[3] == theirs.step == t
        if name == 'h':
            u, p, n = rec['ids'][0]
            useg, iseg = torch.bincount(u).tolist(), torch.bincount(torch.cat([p, n])).tolist()
            assert all(k in useg for k in SEG_LENGTHS) and all(k in iseg for k in SEG_LENGTHS), 'case h: the segment lengths'
            assert int((p == n).sum()) >= 2
        if name == 'i':
            assert rec['Bg'] == 3
    print(f'\n{run.tag}: worst error / bound over 3 steps: {_fmt(worst)}')


def _bpr_params():
    return [(k, 'fused') for k in CASES] + [(k, 'two_pass') for k in TWO_PASS]


def _point_params():
    return [(k, 'fused') for k in POINT_CASES] + [(k, 'two_pass') for k in POINT_TWO_PASS]


@pytest.mark.parametrize('name,form', _bpr_params(), ids=[f'{k}-{f}' for k, f in _bpr_params()])
def test_dim_sharded_bpr_step_vs_fp64(name, form):
    _drive(name, CASES[name], form)


@pytest.mark.parametrize('name,form', _point_params(), ids=[f'{k}-{f}' for k, f in _point_params()])
def test_dim_sharded_point_step_vs_fp64(name, form):
    _drive(name, POINT_CASES[name], form)


@pytest.mark.parametrize('name', ['d', 'e', 'w8'])
def test_dim_sharded_step_is_bit_reproducible(name):
    """The same step twice from the same state (slices, moments, update counts): every slice, every moment and out bit-identical."""
    c = CASES[name] if name in CASES else POINT_CASES[name]
    run = _Run(name, c, 'fused')
    run.lb.step(c['batch'](c, 1, run.gen))                                # (moments and update counts away from zero)
    batches = c['batch'](c, 2, run.gen)
    states = [st for ops in run.ops for st in (ops.fs.ustate, ops.fs.istate)]
    saved = [(s.table.clone(), s.exp_avg.clone(), s.exp_avg_sq.clone(), s.step) for s in states]
    results = []
    for _ in range(2):
        for s, (w, m, v, step) in zip(states, saved):
            s.table.copy_(w); s.exp_avg.copy_(m); s.exp_avg_sq.copy_(v)
            s.step = step
        rec = run.lb.step(batches)
        torch.cuda.synchronize()
        results.append([t.clone() for s in states for t in (s.table, s.exp_avg, s.exp_avg_sq)] + list(rec['out']) + list(rec['reduced']))
    assert any(not torch.equal(a, w) for a, (w, _, _, _) in zip(results[0][::3], saved)), 'the step moved nothing'
    for i, (a, b) in enumerate(zip(*results)):
        _same_bits(f'case {name}: result tensor {i} of two runs', a, b)


# ---------------------------------------------------------------------------------------------------------------------- refusals

@pytest.mark.parametrize('Ds', [6, 260])
@pytest.mark.parametrize('entry', ['cdr_bpr_partial_diff', 'cdr_bpr_step_from_diff', 'cdr_point_partial_dot', 'cdr_point_step_from_dot'])
def test_dim_entry_points_refuse_the_width_and_launch_nothing(entry, Ds):
    """A slice width that is no multiple of 4, or wider than 256: an error, and tables, moments and the score buffer bit-identical."""
    import recbole_cdr_amd  # noqa: F401
    from recbole_cdr_amd import binding as B_
    B, rows = 64, 32
    gen = torch.Generator(device=DEV); gen.manual_seed(Ds)
    f = lambda *shape: torch.empty(*shape, device=DEV).normal_(0, 0.1, generator=gen)
    U, mU, vU, I, mI, vI = (f(rows, Ds) for _ in range(6))
    diff, label, out9 = f(B + 2), f(B), torch.full((12,), -7.0, device=DEV)
    GU, GP = torch.full((B, Ds), -7.0, device=DEV), torch.full((B, Ds), -7.0, device=DEV)
    ids = torch.randint(0, rows, (B,), device=DEV, generator=gen)
    keys, perm = torch.zeros(3 * B, device=DEV, dtype=torch.int32), torch.zeros(3 * B, device=DEV, dtype=torch.int32)
    flags, heads = torch.zeros(4 * B, device=DEV, dtype=torch.uint8), torch.zeros(4096, device=DEV, dtype=torch.int32)
    watched = [U, mU, vU, I, mI, vI, diff, out9, GU, GP]
    saved = [t.clone() for t in watched]
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    lib, ctx, s = B_.load(), B_.ctx(DEV), B_.stream()
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    if entry == 'cdr_bpr_partial_diff':
        rc = lib.cdr_bpr_partial_diff(ctx, s, P(U), P(I), Ds, P(ids), P(ids), P(ids), B, P(diff))
    elif entry == 'cdr_point_partial_dot':
        rc = lib.cdr_point_partial_dot(ctx, s, P(U), P(I), Ds, P(ids), P(ids), B, P(diff))
    elif entry == 'cdr_bpr_step_from_diff':
        rc = lib.cdr_bpr_step_from_diff(ctx, s, 1, P(U), P(mU), P(vU), P(I), P(mI), P(vI), Ds, P(ids), P(ids), P(ids), B, 1e-10, 0.02, *hp, 1, 1,
                                        P(diff), 0, P(out9), P(GU), P(GP), P(keys), P(perm), P(flags), P(heads))
    else:
        rc = lib.cdr_point_step_from_dot(ctx, s, 0, 1, P(U), P(mU), P(vU), P(I), P(mI), P(vI), Ds, P(ids), P(ids), P(label), B, 0.01, *hp, 1, 1,
                                         P(diff), 0, P(out9), P(GU), P(GP), P(keys), P(perm), P(flags), P(heads))
    torch.cuda.synchronize()
    assert rc != 0 and b'invalid argument' in lib.cdr_last_error(), (entry, Ds, rc)
    for t, w in zip(watched, saved):
        assert torch.equal(t.view(torch.int32), w.view(torch.int32)), f'{entry} Ds={Ds}: a refused call wrote to memory'
