"""The row-sharded BPR step (shard.NativeOps: cdr_route_triples / cdr_bpr_shard_plan / cdr_gather_rows_norms / cdr_shard_norm_sums /
cdr_bpr_shard_step / cdr_shard_owner_apply, and the staged form on cdr_dedup_sorted / cdr_batch_norm_sums / cdr_bpr_shard_local_step /
cdr_segsum_rows) against the float64 restatement of the ONE-GPU step on the assembled tables and the concatenated batch, at worlds 1, 2,
3, 5 and 8 in one process (tests/shard_loopback.py: G emulated ranks, all-to-alls as split / cat, all-reduces as an fp32 sum).

Teacher forcing as in test_gpu_step_fp64.py: each of the three steps of a case is judged from the assembled device state before it
(full[r::G] = shard_r, moments likewise); steps 2 and 3 reuse rows, so the bias corrections of updates 2 and 3 are checked.  Touched rows
are held to the per-element bounds of fp64_bounds.apply_fp64; every other row of every shard and its moments -- both neighbours of every
touched row among them -- are compared bit for bit; the loss of every rank to LOSS_RTOL; the EmbLoss coefficients out[4:6] of every rank
to their own relative bound.  No blanket atol anywhere.

What the sharded form adds to the one-GPU bounds (test_gpu_step_fp64.py's docstring), counted from the kernels:
  * EmbLoss coefficient c = reg / (B ||X||).  One GPU: fp32 row sums of D squares, summed in fp64, then sqrtf and two fp32 operations:
    gamma_{D + K_REG}.  Sharded: the row sums are the same fp32 lane-group sums (shard_norms_kernel / batch_norms_kernel for the user
    rows; gather_rows_norms_kernel at the OWNER for the item rows in the direct form, D products and D - 1 additions, travelling as one
    fp32 per row), added in fp64 per rank, and then
      - norm_sums_kernel rounds the rank's sum to fp32 in sums3:                               K_RANK_SUM = 1 rounding,
      - the all-reduce adds the world fp32 values:                                             world - 1 roundings (_allreduce_adds),
    before cdr_loss_finish_sums' sqrtf and two operations (inside K_REG already).  So gamma_{D + K_REG + K_RANK_SUM + world - 1}
    = gamma_{D + K_REG + world}, passed as bpr_grads_fp64(k_reg_extra=...).  The same count holds for the staged form.
  * Item rows.  A requester sums the occurrences it holds of an item (duplicate segments; in fp32, occurrence order) and adds ITS EmbLoss
    term c_i #positives row; the owner then adds the rows of at most ``world`` requesters, starting from +0: up to ``world`` further
    additions on top of the one-GPU count D + occ + K_SUM (_owner_adds).  The item part's ``occ`` is raised by that.
  * User rows live on the rank that runs the forward pass: nothing new beyond the coefficient.

Ids 0 and rows - 1 of both tables are in every batch and ~1 % of the triples have p == n (_mark_edges); in the two steps of case e that
restrict the owners (all users on owner 3; all items on owners 0 and 7) the edge ids are the first and last row OF THOSE OWNERS -- for
the items these are still rows 0 and ni - 1."""
import pytest
import torch

from fp64_bounds import K_REG, LOSS_RTOL, apply_fp64, bpr_grads_fp64, gam
from helpers import DEV
from shard_loopback import OPT_ADAM, OPT_SGD, ShardLoopback, assemble, shard_rows
from test_gpu_step_fp64 import _check_table, _fmt, _mark_edges, _zipf

pytestmark = pytest.mark.gpu

K_RANK_SUM = 1              # a rank's fp64 norm sum rounded to fp32 (sums3) before the all-reduce


def _allreduce_adds(world):
    """fp32 additions an all-reduced value goes through."""
    return world - 1


def _owner_adds(world):
    """Additions of the owner's per-row sum over the requesters' gradient rows (the accumulator starts at +0)."""
    return world


# ---------------------------------------------------------------------------------------------------------------------- batches

def _split(u, p, n, sizes):
    assert sum(sizes) == u.numel()
    return [tuple(t.contiguous() for t in x) for x in zip(torch.split(u, sizes), torch.split(p, sizes), torch.split(n, sizes))]


def _uniform(B, nu, ni, gen):
    return (torch.randint(0, nu, (B,), device=DEV, generator=gen), torch.randint(0, ni, (B,), device=DEV, generator=gen),
            torch.randint(0, ni, (B,), device=DEV, generator=gen))


def _shuffled(u, p, n, gen):
    """(the edge ids _mark_edges puts into the first six triples end up on whichever rank)"""
    o = torch.randperm(u.numel(), device=DEV, generator=gen)
    return u[o], p[o], n[o]


def _batch_a(c, t, gen):
    u, p, n = _uniform(4097, c['nu'], c['ni'], gen)
    _mark_edges(u, p, n, c['nu'], c['ni'], gen)
    uniq = torch.unique(torch.cat([p, n]))
    if uniq.numel() % 2 == 0:                          # an odd request list: the owner's one-run apply takes (n + 1) / 2 groups
        x, y = uniq[1], uniq[2]
        p[p == x] = y
        n[n == x] = y
    return _split(u, p, n, [4097])


def _batch_uniform(c, t, gen):
    u, p, n = _uniform(sum(c['sizes']), c['nu'], c['ni'], gen)
    _mark_edges(u, p, n, c['nu'], c['ni'], gen)
    return _split(*_shuffled(u, p, n, gen), c['sizes'])


def _batch_d(c, t, gen):
    """Half of all triples share one user; one item is a third of the positives and 600 of the negatives."""
    B = sum(c['sizes'])
    u, p, n = _uniform(B, c['nu'], c['ni'], gen)
    o = torch.randperm(B, device=DEV, generator=gen)
    u[o[:B // 2]] = c['nu'] // 2
    o = torch.randperm(B, device=DEV, generator=gen)
    p[o[:B // 3]] = c['ni'] // 3
    o = torch.randperm(B, device=DEV, generator=gen)
    n[o[:600]] = c['ni'] // 3
    _mark_edges(u, p, n, c['nu'], c['ni'], gen)
    return _split(*_shuffled(u, p, n, gen), c['sizes'])


def _batch_e(c, t, gen):
    """Zipf(1.05) positives.  Step 2: every user on owner 3 (seven ranks receive no triple).  Step 3: items of owners 0 and 7 only."""
    B, nu, ni, G = sum(c['sizes']), c['nu'], c['ni'], 8
    u, p, n = _uniform(B, nu, ni, gen)
    p = _zipf(B, ni, gen)
    if t == 3:
        own = torch.tensor([0, 7], device=DEV)
        p = (p // G) * G + own[torch.randint(0, 2, (B,), device=DEV, generator=gen)]
        n = (n // G) * G + own[torch.randint(0, 2, (B,), device=DEV, generator=gen)]
        p, n = p.clamp(max=ni - 1), n.clamp(max=ni - 1)                  # (ni - 1 is a row of owner 0)
    _mark_edges(u, p, n, nu, ni, gen)
    if t == 2:
        u = torch.randint(0, shard_rows(nu, G, 3), (B,), device=DEV, generator=gen) * G + 3
        u[0], u[1] = 3, (shard_rows(nu, G, 3) - 1) * G + 3                # first and last row of owner 3
    return _split(*_shuffled(u, p, n, gen), c['sizes'])


def _batch_g(c, t, gen):
    """Every uid even: rank 0 of 2 receives all 180,000 triples (3 Bl >= 2^18: the big-sort path under the plan), rank 1 none."""
    B = sum(c['sizes'])
    u, p, n = _uniform(B, c['nu'], c['ni'], gen)
    u = (u // 2) * 2
    _mark_edges(u, p, n, c['nu'], c['ni'], gen)                           # (nu - 1 is even)
    return _split(*_shuffled(u, p, n, gen), c['sizes'])


SEG_LENGTHS = [32, 33, 255, 256, 257, 513]      # kLongSeg = 32 and kPiece = 256 from both sides, and a segment of three pieces


def _with_counts(lengths, total, pool, gen):
    """``total`` ids drawn from ``pool`` (distinct candidates): one id per entry of ``lengths`` with exactly that many occurrences, two
    of the rest twice, every other one once; shuffled."""
    rest = total - sum(lengths) - 4
    dev = pool.device
    counts = torch.tensor(lengths + [2, 2] + [1] * rest, device=dev)
    picked = pool[torch.randperm(pool.numel(), device=dev, generator=gen)[:counts.numel()]]
    ids = torch.repeat_interleave(picked, counts)
    return ids[torch.randperm(total, device=dev, generator=gen)]


def _batch_i(c, t, gen):
    """Every user on owner 1 of 3, so ONE rank holds all triples and the exact segment lengths: user rows and item rows with 32 / 33 /
    255 / 256 / 257 / 513 occurrences (items: 1000 as well) in the duplicate-segment launch of the step."""
    B, nu, ni = sum(c['sizes']), c['nu'], c['ni']
    u = _with_counts(SEG_LENGTHS, B, torch.arange(1, nu, 3, device=DEV), gen)
    items = _with_counts(SEG_LENGTHS + [1000], 2 * B, torch.arange(1, ni - 1, device=DEV), gen)
    p, n = items[:B].clone(), items[B:].clone()
    single = torch.nonzero(torch.bincount(items, minlength=ni)[p] == 1).flatten()
    p[single[0]], p[single[1]] = 0, ni - 1                                # rows 0 and ni - 1 in place of two items that occur once
    return _split(u, p, n, c['sizes'])


CASES = {
    'a': dict(world=1, D=64, opt='adam', nu=3001, ni=2501, sizes=[4097], batch=_batch_a),
    'b1024': dict(world=2, D=128, opt='adam', nu=3001, ni=2048, sizes=[4095, 4097], batch=_batch_uniform),
    'b1025': dict(world=2, D=128, opt='adam', nu=3001, ni=2049, sizes=[4095, 4097], batch=_batch_uniform),
    'c': dict(world=3, D=64, opt='adam', wd=0.01, nu=2999, ni=2501, sizes=[1500, 0, 777], batch=_batch_uniform),
    'd': dict(world=5, D=8, opt='adam', nu=2003, ni=1501, sizes=[900, 1100, 700, 1000, 805], batch=_batch_d),
    'e': dict(world=8, D=128, opt='adam', nu=3003, ni=2505, sizes=[600, 555, 640, 0, 610, 700, 601, 599], batch=_batch_e),
    'f': dict(world=8, D=256, opt='adam', reg=0.0, nu=1501, ni=1203, sizes=[700, 701, 699, 650, 750, 702, 698, 700], batch=_batch_uniform),
    'g': dict(world=2, D=8, opt='adam', nu=20001, ni=30001, sizes=[90000, 90000], batch=_batch_g),
    'h': dict(world=3, D=24, opt='sgd', wd=0.01, nu=2000, ni=1501, sizes=[800, 900, 1000], batch=_batch_uniform),
    'i': dict(world=3, D=64, opt='adam', nu=2999, ni=2501, sizes=[500, 400, 600], batch=_batch_i),
}
STAGED = ('b1024', 'b1025', 'd', 'e', 'h', 'i')


# ---------------------------------------------------------------------------------------------------------------------- driver

class _Run:
    def __init__(self, name, form):
        import recbole_cdr_amd  # noqa: F401
        from recbole_cdr_amd.fused import RowwiseState
        from recbole_cdr_amd.shard import NativeOps
        c = self.c = CASES[name]
        self.name, self.form = name, form
        G, D = c['world'], c['D']
        self.gen = torch.Generator(device=DEV); self.gen.manual_seed(sum(map(ord, name)) + D)
        U = torch.empty(c['nu'], D, device=DEV).normal_(0, 0.1, generator=self.gen)
        I = torch.empty(c['ni'], D, device=DEV).normal_(0, 0.1, generator=self.gen)
        self.opt = c['opt']
        code = OPT_ADAM if self.opt == 'adam' else OPT_SGD
        self.lr, self.wd, self.reg = (1e-3 if self.opt == 'adam' else 0.5), c.get('wd', 0.0), c.get('reg', 0.02)
        self.Us = [U[r::G].contiguous() for r in range(G)]               # ragged shards: the table sizes are no multiples of the world
        self.Is = [I[r::G].contiguous() for r in range(G)]
        self.ust, self.ist = [RowwiseState(t, code) for t in self.Us], [RowwiseState(t, code) for t in self.Is]
        hp = {'lr': self.lr, 'b1': 0.9, 'b2': 0.999, 'eps': 1e-8, 'wd': self.wd}
        self.lb = ShardLoopback([NativeOps(torch.device(DEV)) for _ in range(G)], self.Us, self.Is, self.ust, self.ist, c['ni'], code, hp,
                                reg_weight=self.reg, form=form)
        self.tag = f'case {name} {form}: world={G} D={D} {self.opt} wd={self.wd} reg={self.reg}'

    def state(self, states, rows):
        d = {'w': assemble([s.table for s in states], rows)}
        if self.opt == 'adam':
            d['m'], d['v'] = assemble([s.exp_avg for s in states], rows), assemble([s.exp_avg_sq for s in states], rows)
        return d

    def checked_step(self, t, worst):
        c, G, D = self.c, self.c['world'], self.c['D']
        batches = c['batch'](c, t, self.gen)
        u, p, n = (torch.cat([b[k] for b in batches]) for k in range(3))
        bu, bi = self.state(self.ust, c['nu']), self.state(self.ist, c['ni'])
        detail = {}
        loss, upart, ipart = bpr_grads_fp64(bu['w'], bi['w'], u, p, n, self.reg, detail=detail, k_reg_extra=K_RANK_SUM + _allreduce_adds(G))
        ipart = (*ipart[:4], ipart[4] + _owner_adds(G))
        wu = apply_fp64(bu, upart, D, self.opt, self.lr, self.wd, t)
        wi = apply_fp64(bi, ipart, D, self.opt, self.lr, self.wd, t)
        rec = self.lb.step(batches)
        torch.cuda.synchronize()
        tag = f'{self.tag} step {t}'
        for r in range(G):
            got = float(self.lb.loss(r))
            assert abs(got - loss) <= LOSS_RTOL * abs(loss), f'{tag}: loss on rank {r} {got!r} vs fp64 {loss!r}'
            worst['loss'] = max(worst.get('loss', 0.0), abs(got - loss) / (LOSS_RTOL * abs(loss)))
            for k, name in ((0, 'cu'), (1, 'ci')):
                gc, wc = float(rec['coef'][r][k]), detail[name]
                if wc == 0.0:
                    assert gc == 0.0, f'{tag}: coefficient {name} on rank {r} is {gc!r} without EmbLoss'
                    continue
                assert detail['gc'] == gam(D + K_REG + K_RANK_SUM + _allreduce_adds(G))
                ratio = abs(gc - wc) / (detail['gc'] * abs(wc))
                assert ratio <= 1.0, f'{tag}: coefficient {name} on rank {r}: got {gc!r} want {wc!r}, error / bound = {ratio:.3g}'
                worst['coef'] = max(worst.get('coef', 0.0), ratio)
            assert self.ust[r].step == t and self.ist[r].step == t
        au, ai = self.state(self.ust, c['nu']), self.state(self.ist, c['ni'])
        for name, wt in (('U', _check_table(f'{tag} U', bu, au, upart[0], wu)), ('I', _check_table(f'{tag} I', bi, ai, ipart[0], wi))):
            for k, v in wt.items():
                worst[f'{name}.{k}'] = max(worst.get(f'{name}.{k}', 0.0), v)
        return rec


def _params():
    return [(k, 'direct') for k in CASES] + [(k, 'staged') for k in STAGED]


@pytest.mark.parametrize('name,form', _params(), ids=[f'{k}-{f}' for k, f in _params()])
def test_sharded_step_vs_fp64(name, form):
    run = _Run(name, form)
    c, G = run.c, run.c['world']
    worst = {}
    for t in (1, 2, 3):
        rec = run.checked_step(t, worst)
        Bl = rec['Bl']
        if name == 'a':
            assert rec['i_req'][0].numel() % 2 == 1, 'case a: the owner list has to be odd'
        if name.startswith('b'):
            assert shard_rows(c['ni'], 2, 0) == c['ni'] - 1024                        # item_local_rows = 1024 / 1025
        if name == 'c':
            assert rec['send3'][1].shape[0] == 0 and all(Bl)                          # a rank without a batch still owns rows of others' triples
        if name == 'e' and t == 2:
            assert [b > 0 for b in Bl] == [r == 3 for r in range(8)]
        if name == 'e' and t == 3:
            assert all(rec['i_req'][r].numel() == 0 for r in range(1, 7)) and rec['i_req'][0].numel() and rec['i_req'][7].numel()
        if name == 'g':
            assert Bl == [180000, 0]
        if name == 'i':
            assert Bl == [0, 1500, 0]
            useg = torch.bincount(rec['recv3'][1][:, 0]).tolist()
            iseg = torch.bincount(rec['plan'][1]['umap']).tolist()
            assert all(k in useg for k in SEG_LENGTHS) and all(k in iseg for k in SEG_LENGTHS + [1000])
    print(f'\n{run.tag}: worst error / bound over 3 steps: {_fmt(worst)}')


@pytest.mark.parametrize('name', ['d', 'e'])
def test_sharded_step_is_bit_reproducible(name):
    """The same step twice from the same state (tables, moments, update counts): every shard and every moment bit-identical."""
    run = _Run(name, 'direct')
    c = run.c
    run.lb.step(c['batch'](c, 1, run.gen))                                # (moments and update counts away from zero)
    batches = c['batch'](c, 2 if name == 'd' else 3, run.gen)
    states = run.ust + run.ist
    saved = [(s.table.clone(), s.exp_avg.clone(), s.exp_avg_sq.clone(), s.step) for s in states]
    results = []
    for _ in range(2):
        for s, (w, m, v, step) in zip(states, saved):
            s.table.copy_(w); s.exp_avg.copy_(m); s.exp_avg_sq.copy_(v)
            s.step = step
        rec = run.lb.step(batches)
        torch.cuda.synchronize()
        results.append([t.clone() for s in states for t in (s.table, s.exp_avg, s.exp_avg_sq)] + [o for o in rec['out']] + list(rec['GS']))
    assert any(not torch.equal(a, w) for a, (w, _, _, _) in zip(results[0][::3], saved)), 'the step moved nothing'
    for i, (a, b) in enumerate(zip(*results)):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f'case {name}: result tensor {i} differs between two runs'
