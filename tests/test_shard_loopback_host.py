"""tests/shard_loopback.py (G emulated ranks of the row-sharded BPR step in one process) checked on CPU before any kernel is involved:
driven with test_shard_gloo.OracleOps, the assembled tables (full[r::G] = shard_r), the moments and the loss of three steps equal
oracle.train_step.rowwise_step on the concatenated batch, at worlds 1, 2, 3, 5, 8, in both forms, with Adam and with SGD -- ragged
batches, a rank that brings no triples, and one step whose users all live on a single owner (every other rank has Bl == 0)."""
import pytest
import torch

from shard_loopback import OPT_ADAM, OPT_SGD, ShardLoopback, assemble
from test_shard_gloo import OracleOps

NU, NI, D, REG, LR = 41, 29, 8, 0.03, 0.05


def _batches(world, step):
    """Rank r brings 31 + 3 r triples; the last rank of a world > 1 brings none; in step 1 every user lives on owner world // 2."""
    out = []
    for r in range(world):
        g = torch.Generator(); g.manual_seed(100 * step + r)
        B = 0 if (world > 1 and r == world - 1) else 31 + 3 * r
        u = torch.randint(0, NU, (B,), generator=g)
        if step == 1:
            own = world // 2
            u = torch.randint(0, (NU - own + world - 1) // world, (B,), generator=g) * world + own
        out.append((u, torch.randint(0, NI, (B,), generator=g), torch.randint(0, NI, (B,), generator=g)))
    return out


@pytest.mark.parametrize('opt', ['adam', 'sgd'])
@pytest.mark.parametrize('form', ['direct', 'staged'])
@pytest.mark.parametrize('world', [1, 2, 3, 5, 8])
def test_loopback_with_oracle_ops_matches_single_process(world, form, opt):
    import recbole_cdr_amd  # noqa: F401
    from recbole_cdr_amd.fused import RowwiseState
    from recbole_cdr_amd.shard import shard_of
    from oracle import train_step as ts
    torch.manual_seed(0)
    U, I = torch.randn(NU, D) * 0.3, torch.randn(NI, D) * 0.3
    code = OPT_ADAM if opt == 'adam' else OPT_SGD
    Us, Is = [shard_of(U, world, r).clone() for r in range(world)], [shard_of(I, world, r).clone() for r in range(world)]
    ust, ist = [RowwiseState(t, code) for t in Us], [RowwiseState(t, code) for t in Is]
    hp = {'lr': LR, 'b1': 0.9, 'b2': 0.999, 'eps': 1e-8, 'wd': 0.0}
    lb = ShardLoopback([OracleOps() for _ in range(world)], Us, Is, ust, ist, NI, code, hp, reg_weight=REG, form=form)
    us, is_ = ts.RowwiseAdamState(U), ts.RowwiseAdamState(I)
    for step in range(3):
        batches = _batches(world, step)
        rec = lb.step(batches)
        u, p, n = (torch.cat([b[k] for b in batches]) for k in range(3))
        loss = float(ts.rowwise_step(U, I, us, is_, u, p, n, step + 1, opt=opt, lr=LR, reg_weight=REG))
        assert rec['B_global'] == u.numel() and sum(rec['Bl']) == u.numel()
        if step == 1:
            assert [bl > 0 for bl in rec['Bl']] == [r == world // 2 for r in range(world)]
        for r in range(world):
            assert abs(float(lb.loss(r)) - loss) <= 1e-5 * abs(loss), (step, r, float(lb.loss(r)), loss)
            assert ust[r].step == ist[r].step == step + 1
    atol = LR * 1e-2 if opt == 'adam' else 1e-6
    torch.testing.assert_close(assemble(Us, NU), U, rtol=2e-5, atol=atol)
    torch.testing.assert_close(assemble(Is, NI), I, rtol=2e-5, atol=atol)
    if opt == 'adam':
        # (moments: the same relative tolerance; the floor on the moment tensor's own scale -- m and v are orders of magnitude below the weights)
        for got, want in ((assemble([s.exp_avg for s in ust], NU), us.m), (assemble([s.exp_avg_sq for s in ust], NU), us.v),
                          (assemble([s.exp_avg for s in ist], NI), is_.m), (assemble([s.exp_avg_sq for s in ist], NI), is_.v)):
            torch.testing.assert_close(got, want, rtol=2e-5, atol=1e-5 * float(want.abs().max()))
