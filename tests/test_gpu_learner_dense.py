"""config['learner'] = sgd / adagrad / rmsprop on the dense route: the one-launch native sweep (cdr_opt_multi_dev, csrc/cdr_optim.hip)
against torch.optim.<X> in float64, and a captured dense training step replayed against the eager loop.

Bound of the fp64 comparison: the max-norm error of torch.optim.<X> run in FLOAT32 on the same inputs against the float64 run, times a
margin of 4 (the native update term may differ from torch's by the order of its operations and, had it used the 1-ulp hardware sqrt and
rcp, by <= 3 ulp of the update term), plus one ulp of the largest parameter."""
import ctypes

import pytest
import torch

from helpers import DEV, FakeDataset, base_config

pytestmark = pytest.mark.gpu

SIZES = [(1,), (1003,), (64, 33)]             # odd sizes: the tail lanes of the 16-byte path and the scalar path
KINDS = {'sgd': torch.optim.SGD, 'adagrad': torch.optim.Adagrad, 'rmsprop': torch.optim.RMSprop}


def _native(kind, params, lr, wd):
    from recbole_cdr_amd.trainer.trainer import dense_optimizer
    return dense_optimizer(kind, params, lr, wd)


@pytest.mark.parametrize('wd', [0.0, 1e-2])
@pytest.mark.parametrize('kind', ['sgd', 'adagrad', 'rmsprop'])
def test_dense_learner_kernels_vs_fp64(kind, wd):
    lr, steps = 1e-2, 5
    g = torch.Generator().manual_seed(11)
    init = [torch.randn(*s, generator=g) for s in SIZES]
    grads = [[torch.randn(*s, generator=g) * 0.5 for s in SIZES] for _ in range(steps)]
    if kind == 'adagrad':
        for t in range(steps):
            grads[t][1].zero_()                                   # a whole tensor without gradient signal: it must not move (wd = 0)

    def run_torch(dtype):
        ps = [torch.nn.Parameter(x.to(dtype).clone()) for x in init]
        opt = KINDS[kind](ps, lr=lr, weight_decay=wd)
        for t in range(steps):
            for p, gr in zip(ps, grads[t]):
                p.grad = gr.to(dtype).clone()
            opt.step()
        return [p.detach() for p in ps], opt

    ref64, opt64 = run_torch(torch.float64)
    ref32, _ = run_torch(torch.float32)
    ps = [torch.nn.Parameter(x.clone().to(DEV)) for x in init]
    opt = _native(kind, ps, lr, wd)
    for t in range(steps):
        for p, gr in zip(ps, grads[t]):
            p.grad = gr.clone().to(DEV)
        opt.step()
    torch.cuda.synchronize()
    key = {'adagrad': 'sum', 'rmsprop': 'square_avg'}.get(kind)
    for i, (p, r64, r32) in enumerate(zip(ps, ref64, ref32)):
        got = p.detach().cpu().double()
        e32 = float((r32.double() - r64).abs().max())
        big = r64.abs().max().float()
        ulp = float(torch.nextafter(big, torch.tensor(float('inf'))) - big)
        bound = 4.0 * e32 + ulp
        err = float((got - r64).abs().max())
        print(f'\n{kind} wd={wd} tensor {i} {tuple(p.shape)}: |native - fp64| = {err:.3g}, |torch fp32 - fp64| = {e32:.3g}, '
              f'ratio {err / max(e32, 1e-300):.3g}, bound {bound:.3g}')
        assert err <= bound, f'{kind} wd={wd} tensor {i}: {err:.3g} > {bound:.3g}'
        if key:
            s64 = opt64.state[opt64.param_groups[0]['params'][i]][key]
            s_got = opt.state[p][key].cpu().double()
            assert float(((s_got - s64).abs() / (s64.abs() + 1e-30)).max()) <= 64 * 2.0 ** -24, f'{kind}: {key} of tensor {i}'
            assert float(opt.state[p]['step']) == steps
    if kind == 'adagrad' and wd == 0.0:
        assert torch.equal(ps[1].detach().cpu().view(torch.int32), init[1].view(torch.int32)), 'a zero gradient moved the parameter'
        assert not bool(opt.state[ps[1]]['sum'].view(torch.int32).any()), 'a zero gradient moved the sum'
    if kind == 'sgd':
        assert len(opt.state_dict()['state']) == 0


def test_dense_learner_skips_parameters_without_grad_and_adds_the_loss():
    ps = [torch.nn.Parameter(torch.ones(5, device=DEV)), torch.nn.Parameter(torch.ones(7, device=DEV))]
    opt = _native('adagrad', ps, 0.1, 0.0)
    ps[0].grad = torch.full((5,), 2.0, device=DEV)
    loss, total = torch.tensor(1.5, device=DEV), torch.tensor(10.0, device=DEV)
    opt.loss_pair = (loss, total)
    opt.step()
    torch.cuda.synchronize()
    assert opt.loss_pair is None and float(total) == 11.5
    assert torch.equal(ps[1].detach().cpu(), torch.ones(7)) and ps[1] not in opt.state
    want = 1.0 - 0.1 * (2.0 / (2.0 + 1e-10))
    assert abs(float(ps[0][0]) - want) <= 2.0 ** -23


def test_opt_multi_dev_refuses_adam_and_bad_arguments():
    from recbole_cdr_amd import binding as B_
    lib = B_.load()
    x = torch.ones(8, device=DEV)
    one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    n = (ctypes.c_int64 * 1)(8)
    keep = x.clone()
    assert lib.cdr_opt_multi_dev(None, 1, 1, one(x), one(x), one(x), n, 0.1, 0.99, 1e-8, 0.0, None, None) != 0          # Adam: the other entry
    assert lib.cdr_opt_multi_dev(None, 2, 1, one(x), one(x), None, n, 0.1, 0.99, 1e-8, 0.0, None, None) != 0            # Adagrad without a sum
    assert lib.cdr_opt_multi_dev(None, 0, 0, one(x), one(x), None, n, 0.1, 0.99, 1e-8, 0.0, None, None) != 0            # no tensor
    assert lib.cdr_opt_multi_dev(None, 0, 1, one(x), one(x), None, n, 0.1, 0.99, 1e-8, 0.0, x.data_ptr(), None) != 0    # loss without loss_sum
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


# ---------------------------------------------------------------------------------------------------------------------- captured step

def _model_and_batches(seed):
    from oracle.common import IdSpace
    from recbole_cdr_amd.data.interaction import Interaction
    from recbole_cdr_amd.model.cross_domain_recommender.emcdr import EMCDR
    ids = IdSpace(OU=40, TOU=30, SOU=35, OI=1, TOI=60, SOI=70)
    cfg = base_config(DEV, latent_factor_model='BPR', source_embedding_size=16, target_embedding_size=16, reg_weight=0.01,
                      mapping_function='linear', mlp_hidden_size=[24], learning_rate=0.05, train_modes=['SOURCE'], epoch_num=['1'],
                      source_split=False, eval_step=0, epochs=1)
    torch.manual_seed(seed)
    model = EMCDR(cfg, FakeDataset(ids)).to(DEV)
    model.set_phase('SOURCE')
    model.train()
    g = torch.Generator().manual_seed(seed + 1)
    batches = []
    for _ in range(7):
        # distinct users and distinct items per batch (positives and negatives disjoint): every gradient element receives ONE atomic add,
        # so the dense backward is order-free and the comparison can be bit for bit
        u = 1 + torch.randperm(ids.total_num_users - 1, generator=g)[:32]
        it = 1 + torch.randperm(ids.total_num_items - 1, generator=g)[:64]
        batches.append(Interaction({model.SOURCE_USER_ID: u.to(DEV), model.SOURCE_ITEM_ID: it[:32].to(DEV),
                                    model.SOURCE_NEG_ITEM_ID: it[32:].to(DEV)}))
    return cfg, model, batches


@pytest.mark.parametrize('kind', ['sgd', 'adagrad'])
def test_captured_dense_step_replays_bit_equal_to_the_eager_loop(kind):
    from recbole_cdr_amd.graph_step import GraphedTrainStep, step_and_sum
    _, model, batches = _model_and_batches(5)
    _, ref, _ = _model_and_batches(5)
    opt, ropt = _native(kind, model.parameters(), 0.05, 0.0), _native(kind, ref.parameters(), 0.05, 0.0)
    total, rtotal = torch.zeros((), device=DEV), torch.zeros((), device=DEV)
    gs = GraphedTrainStep(model, opt, batches[0], loss_sum=total)           # warm-up on batch 0 (put back), then the capture
    for name, p in model.named_parameters():
        assert torch.equal(p, dict(ref.named_parameters())[name]), f'{name}: the warm-up was not put back'
    assert float(total) == 0.0
    for b in batches[1:]:
        assert gs.matches(b)
        gs.step(b)
        ropt.zero_grad(set_to_none=True)
        loss = ref.calculate_loss(b)
        loss = loss.reshape(()) if loss.numel() == 1 else loss.sum()
        loss.backward()
        step_and_sum(ropt, loss.detach(), rtotal)
    torch.cuda.synchronize()
    assert float(total) == float(rtotal) and float(total) != 0.0
    rp = dict(ref.named_parameters())
    moved = 0
    for name, p in model.named_parameters():
        assert torch.equal(p.view(torch.int32), rp[name].view(torch.int32)), f'{name}: replay differs from the eager loop'
        if p in opt.state:
            assert torch.equal(opt.state[p]['sum'], ropt.state[rp[name]]['sum']), f'{name}: sum'
            assert float(opt.state[p]['step']) == float(ropt.state[rp[name]]['step']) == len(batches) - 1, f'{name}: step'
            moved += 1
    assert kind == 'sgd' or moved >= 2
