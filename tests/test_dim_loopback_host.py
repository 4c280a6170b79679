"""tests/dim_loopback.py (G emulated ranks of the dimension-sharded step in one process) and the float64 checker of
tests/test_gpu_dim_fp64.py, checked on CPU before any kernel is involved:

  * driven with test_shard_gloo.OracleDimOps / OraclePointDimOps, the assembled tables (torch.cat of the column slices), the moments and
    the loss of three steps equal oracle.train_step.rowwise_step / rowwise_point_step on the concatenated batch at worlds 1, 2, 3, 5, 8;
  * the checker accepts the honest fp32 stand-in on CPU tensors at worlds 2 and 5 and rejects five mutated ones by name;
  * the coverage claims of test_gpu_dim_fp64.py's case tables hold from the kernels' constants."""
import pytest
import torch

from dim_loopback import DimLoopback, assemble_cols
from fp64_bounds import GAMMA, f32
from test_shard_gloo import OracleDimOps, OracleOps, OraclePointDimOps

NU, NI, REG, LR = 41, 29, 0.03, 0.05
HP = {'lr': LR, 'b1': 0.9, 'b2': 0.999, 'eps': 1e-8, 'wd': 0.0}


def _batches(world, step, point):
    """Every rank brings 23 rows (the layout needs the same count on every rank)."""
    out = []
    for r in range(world):
        g = torch.Generator(); g.manual_seed(100 * step + r)
        u, p = torch.randint(0, NU, (23,), generator=g), torch.randint(0, NI, (23,), generator=g)
        out.append((u, p, torch.rand(23, generator=g) * 5 if point else torch.randint(0, NI, (23,), generator=g)))
    return out


@pytest.mark.parametrize('kind,opt', [('bpr', 'adam'), ('bpr', 'sgd'), ('mse', 'adam')])
@pytest.mark.parametrize('world', [1, 2, 3, 5, 8])
def test_loopback_with_oracle_ops_matches_single_process(world, kind, opt):
    from oracle import train_step as ts
    point = kind == 'mse'
    torch.manual_seed(0)
    D = 8 * world
    U, I = torch.randn(NU, D) * 0.3, torch.randn(NI, D) * 0.3
    code = 1 if opt == 'adam' else 0
    Us = [U[:, 8 * r:8 * (r + 1)].clone() for r in range(world)]
    Is = [I[:, 8 * r:8 * (r + 1)].clone() for r in range(world)]
    ops = [OraclePointDimOps(Us[r], Is[r], code, HP, 0.0, REG) if point else OracleDimOps(Us[r], Is[r], code, HP, 1e-10, REG) for r in range(world)]
    lb = DimLoopback(ops, 23, pointwise=point)
    us, is_ = ts.RowwiseAdamState(U), ts.RowwiseAdamState(I)
    for step in range(3):
        batches = _batches(world, step, point)
        rec = lb.step(batches)
        a, b, c = (torch.cat([x[k] for x in batches]) for k in range(3))
        if point:
            loss = float(ts.rowwise_point_step(U, I, us, is_, a, b, c, step + 1, step + 1, loss='mse', opt=opt, lr=LR, reg_weight=REG))
        else:
            loss = float(ts.rowwise_step(U, I, us, is_, a, b, c, step + 1, opt=opt, lr=LR, reg_weight=REG))
        assert rec['Bg'] == a.numel() == 23 * world
        for r in range(world):
            assert torch.equal(rec['ids'][r][0], a) and torch.equal(rec['ids'][r][1], b)
            assert torch.equal(rec['labels'][r], c) if point else torch.equal(rec['ids'][r][2], c)
            assert abs(float(lb.loss(r)) - loss) <= 1e-5 * abs(loss), (step, r, float(lb.loss(r)), loss)
            assert ops[r].t == step + 1
        # the reduced buffer is the sum of the ranks' partials, the same on every rank
        total = torch.stack(rec['partials']).sum(0)
        assert all(torch.equal(x, total) for x in rec['reduced'])
    atol = LR * 1e-2 if opt == 'adam' else 1e-6
    torch.testing.assert_close(assemble_cols(Us), U, rtol=2e-5, atol=atol)
    torch.testing.assert_close(assemble_cols(Is), I, rtol=2e-5, atol=atol)
    if opt == 'adam':
        for got, want in ((assemble_cols([o.state[0][0] for o in ops]), us.m), (assemble_cols([o.state[0][1] for o in ops]), us.v),
                          (assemble_cols([o.state[1][0] for o in ops]), is_.m), (assemble_cols([o.state[1][1] for o in ops]), is_.v)):
            torch.testing.assert_close(got, want, rtol=2e-5, atol=1e-5 * float(want.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------- the checker

class _DropsOneRanksPartial(OracleDimOps):
    """Rank 1's partial scores never reach the sum (its share of the norms does)."""

    def partial(self, uid, pid, nid, diff):
        super().partial(uid, pid, nid, diff)
        if self.rank == 1:
            diff[:uid.numel()] = 0.0


class _NormsFromRankZero(OracleDimOps):
    """The all-reduced norm tail holds rank 0's share alone."""

    def partial(self, uid, pid, nid, diff):
        super().partial(uid, pid, nid, diff)
        if self.rank != 0:
            diff[uid.numel():] = 0.0


class _LabelsOfTheNextRank(OraclePointDimOps):
    """Every rank's rows are paired with the labels of the rank behind it."""

    def unpack_ids(self, gathered32, world, Bl, out64, label_out=None):
        super().unpack_ids(gathered32, world, Bl, out64, label_out)
        label_out.copy_(torch.roll(label_out.clone(), -Bl))


class _StaleBiasCorrection(OracleDimOps):
    """Update 2 is applied with the bias corrections of t - 1 (the update count itself stays right)."""

    def grad_apply(self, uid, pid, nid, diff):
        if self.t != 1:
            return super().grad_apply(uid, pid, nid, diff)
        self.t = 0
        out = super().grad_apply(uid, pid, nid, diff)
        self.t = 2
        return out


class _DropsLastDuplicate(OracleDimOps):
    """OracleDimOps.grad_apply with the last occurrence of one duplicated item row left out of its segment sum."""

    def grad_apply(self, uid, pid, nid, diff):
        B = uid.numel()
        u, p, n = self.U[uid], self.I[pid], self.I[nid]
        s = torch.sigmoid(diff[:B])
        g = -(1.0 / B) * (s * (1 - s)) / (self.gamma + s)
        GU, GP = g[:, None] * (p - n), g[:, None] * u
        OracleOps().finish_sums(torch.stack([(-torch.log(self.gamma + s)).sum(), diff[B], diff[B + 1]]), B, self.reg_weight, self.out)
        self.t += 1
        o = OracleOps()
        o.sort_apply(self.U, self.state[0], uid, GU, self.opt, self.hp, self.t, reg_limit=B, reg_coef=self.out[4:5])
        items, GI = torch.cat([pid, nid]), torch.cat([GP, -GP])
        cnt = torch.bincount(items)
        dup = int(torch.nonzero(cnt >= 2)[0])
        GI[int(torch.nonzero(items == dup)[-1])] = 0.0
        o.sort_apply(self.I, self.state[1], items, GI, self.opt, self.hp, self.t, reg_limit=B, reg_coef=self.out[5:6])
        return self.out


def _stand_in(cls):
    def make(run, rank, Uc, Ic, Bg):
        assert run.wd == 0.0 and (not run.point or run.c['loss'] == 'mse'), 'the oracle stand-ins know neither weight decay nor BCE'
        # the hyper-parameters as a kernel receives them (float launch arguments, fp64_bounds.f32): the stand-in forms 1 - beta in Python
        # floats, and 1 - 0.999 differs from 1 - f32(0.999) by 1.3e-5 relative -- a convention, not a rounding the bounds could hold
        hp = {'lr': f32(run.lr), 'b1': f32(0.9), 'b2': f32(0.999), 'eps': f32(1e-8), 'wd': 0.0}
        ops = cls(Uc, Ic, 1 if run.opt == 'adam' else 0, hp, 0.0 if run.point else GAMMA, run.reg)
        ops.rank = rank
        return ops
    return make


def _cpu_cases(world):
    import test_gpu_dim_fp64 as T
    base = dict(world=world, D=8 * world, nu=211, ni=157, Bl=120, scale=0.3)
    return (dict(base, opt='adam', batch=T._batch_uniform), dict(base, opt='sgd', batch=T._batch_uniform),
            dict(base, loss='mse', labels='ratings', odd_labels=True, batch=T._batch_point))


@pytest.mark.parametrize('world', [2, 5])
def test_fp64_checker_accepts_the_oracle_ops_and_rejects_five_mutations(world):
    import test_gpu_dim_fp64 as T
    adam, sgd, mse = _cpu_cases(world)
    for name, c, cls in (('cpu_adam', adam, OracleDimOps), ('cpu_sgd', sgd, OracleDimOps), ('cpu_mse', mse, OraclePointDimOps)):
        run, worst = T.run_case(name, c, dev='cpu', make_ops=_stand_in(cls))
        assert worst and all(v <= 1.0 for v in worst.values())
        assert ('coef' in worst) and ('U.w' in worst) and ('I.w' in worst) and (c.get('opt') == 'sgd' or ('U.m' in worst and 'I.v' in worst))
        print(f'\n{run.tag}: honest stand-in, worst error / bound: {T._fmt(worst)}')
    for what, c, name, cls, seen_by in (
            ("one rank's partial left out of the all-reduced scores", adam, 'cpu_adam', _DropsOneRanksPartial, r'loss on rank|error / bound'),
            ('the all-reduced norm tail taken from rank 0 alone', adam, 'cpu_adam', _NormsFromRankZero, r'loss on rank|coefficient c[ui] on rank'),
            ("pointwise labels paired with the next rank's rows", mse, 'cpu_mse', _LabelsOfTheNextRank, r'gathered labels on rank'),
            ('Adam bias corrections evaluated at t - 1 on step 2', adam, 'cpu_adam', _StaleBiasCorrection, r'step 2 [UI] rank \d+\.w: error / bound'),
            ('the last occurrence of one duplicated item row dropped from its segment sum', adam, 'cpu_adam', _DropsLastDuplicate,
             r'step 1 I rank \d+\.[wmv]: error / bound')):
        with pytest.raises(AssertionError, match=seen_by):
            T.run_case(name, c, dev='cpu', make_ops=_stand_in(cls))
        print(f'world {world}: rejected: {what}')


def test_norm_tail_mutation_is_seen_by_the_coefficient_bound_alone():
    """With the loss check out of the way (reg so small that the EmbLoss term is below LOSS_RTOL of the loss) the coefficient's own relative
    bound still sees a norm tail that lacks a rank's share."""
    import test_gpu_dim_fp64 as T
    c = dict(_cpu_cases(2)[0], reg=1e-7)
    T.run_case('cpu_adam', c, dev='cpu', make_ops=_stand_in(OracleDimOps))
    with pytest.raises(AssertionError, match=r'coefficient c[ui] on rank'):
        T.run_case('cpu_adam', c, dev='cpu', make_ops=_stand_in(_NormsFromRankZero))


# ---------------------------------------------------------------------------------------------------------------------- coverage
# The kernels' constants, restated (recbole-cdr_amd/csrc):
K_BLOCK = 256               # cdr_common.h:13      constexpr int kBlock = 256
K_UNROLL = 4                # cdr_dimshard.hip:26  constexpr int kUnroll = 4 (rows per lane group and round of the partial / two-pass kernels)
GRID_CAP = 2048             # cdr_common.h:275-281 grid_for: CDR_NUM_CU (256, :9) * 8 blocks, grid-stride beyond
K_BIG_SORT = 1 << 18        # cdr_step.hip:2255    constexpr int64_t kBigSort = 1 << 18 (pairs: 3 Bg for BPR, 2 Bg for pointwise rows)
K_LONG_SEG = 32             # cdr_step.hip:365     constexpr int kLongSeg = 32
K_PIECE = 256               # cdr_step.hip:366     constexpr int kPiece = 256


def lpr_for(D):
    """cdr_common.h:249-253 cdr_lpr_for: lanes per row when a lane moves one float4."""
    q, lanes = (D + 3) // 4, 1
    while lanes < q and lanes < 64:
        lanes <<= 1
    return lanes


def test_case_table_covers_every_regime():
    import test_gpu_dim_fp64 as T
    every = [(k, c, False) for k, c in T.CASES.items()] + [(k, c, True) for k, c in T.POINT_CASES.items()]
    lanes = {}
    for k, c, point in every:
        assert c['D'] % (4 * c['world']) == 0, k
        lanes.setdefault(lpr_for(c['D'] // c['world']), []).append(k)
    assert sorted(lanes) == [1, 2, 4, 8, 16, 32, 64], lanes
    assert sorted(lpr_for(c['D'] // c['world']) for c in T.CASES.values()) == [1, 1, 2, 4, 4, 8, 16, 32, 64]       # BPR alone has every one
    for point in (False, True):
        past = []
        for k, c, pt in every:
            if pt != point:
                continue
            Bg, lpr = c['world'] * c['Bl'], lpr_for(c['D'] // c['world'])
            one_pass_partial = GRID_CAP * (K_BLOCK // lpr) * K_UNROLL          # bpr_partial_diff / grad_from_diff and the pointwise twins
            one_pass_fwd = GRID_CAP * (K_BLOCK // lpr)                         # bpr_fwd_apply_kernel / point_fwd_apply_kernel (XD)
            pairs = (2 if point else 3) * Bg
            if Bg > one_pass_partial and Bg > one_pass_fwd and pairs >= K_BIG_SORT:
                past.append(k)
                # ... and by no more than it takes (the big sort sets the size): these two cases are the only ones that need theirs
                assert pairs < K_BIG_SORT + K_BIG_SORT // 16, (k, Bg)
        assert past == (['w2'] if point else ['b']), (point, past)
    assert 'b' in T.TWO_PASS                                                    # the two-pass kernels' second grid pass too
    # non-temporal row traffic starts at 32 lanes per row (Ds >= 128): case b (32) and c (64), the largest pointwise case (32)
    assert lpr_for(128) == 32 and lpr_for(256) == 64
    # case h: Ds = 12 is 3 float4 on 4 lanes (live = sub < 3), with segments at kLongSeg and kPiece from both sides and one of three pieces
    h = T.CASES['h']
    Ds = h['D'] // h['world']
    assert Ds == 12 and lpr_for(Ds) == 4 and Ds // 4 == 3
    assert {K_LONG_SEG, K_LONG_SEG + 1, K_PIECE - 1, K_PIECE, K_PIECE + 1, 2 * K_PIECE + 1} == set(T.SEG_LENGTHS)
    distinct = lambda total: total - sum(T.SEG_LENGTHS) - 4 + len(T.SEG_LENGTHS) + 2           # _with_counts: the ids a batch of ``total`` draws
    Bg = h['world'] * h['Bl']
    assert sum(T.SEG_LENGTHS) + 4 <= Bg and distinct(Bg) <= h['nu'] - 2 and distinct(2 * Bg) <= h['ni'] - 2
    # the benchmark's own slice widths: 16 (plain dim at 8 GPUs, D = 128) and 32 (domain groups: D = 128 over 4)
    assert (T.CASES['e']['world'], T.CASES['e']['D']) == (8, 128) and (T.CASES['d']['world'], T.CASES['d']['D']) == (4, 128)
    assert T.TWO_PASS == ('b', 'd', 'g', 'h') and T.POINT_TWO_PASS == ('w3',)
    # the layout's score count never exceeds the one-GPU D + 2
    for k, c, point in every:
        assert T.k_score(point, c['D'] // c['world'], c['world']) <= c['D'] + 2, k
