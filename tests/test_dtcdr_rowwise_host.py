"""Host-side checks of DTCDR's O(batch) row-wise training path (no GPU): header, binding and library agree on the new entry points,
the native entry refuses the shapes it documents before any launch, the trainer accepts the model with ``optimizer_mode='rowwise'``, and
the float64 restatement test_gpu_dtcdr_rowwise.py holds the kernel to (dtcdr_fp64.py) passes an fp32 torch-autograd result of the oracle
on the CPU and rejects three mutations of it."""
import ctypes
import os
import re

import pytest
import torch

from dtcdr_fp64 import TABLES, check_dtcdr_result, dtcdr_domain_fp64, dtcdr_grid, n_params
from helpers import FakeDataset, base_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------- boundary

def test_header_binding_and_library_agree_on_the_dtcdr_entry_points():
    from recbole_cdr_amd import binding
    text = open(os.path.join(ROOT, 'include', 'cdr_hip.h')).read()
    assert int(re.search(r'#define CDR_ABI_VERSION (\d+)', text).group(1)) == binding.ABI_VERSION     # (adding entries changes no signature)
    lib = binding.load()
    assert lib.cdr_abi_version() == binding.ABI_VERSION
    plain = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, nargs in (('cdr_dtcdr_fwd_grad', 27), ('cdr_dtcdr_fwd_grad_workspace_bytes', 5)):
        assert name in binding.exported_symbols() and len(binding._SIGNATURES[name]) == nargs
        decl = re.search(r'int %s\((.*?)\);' % name, plain, flags=re.S).group(1)
        assert len(decl.split(',')) == nargs, name
        assert hasattr(lib, name), name
    assert re.search(r'dtcdr\.py:\d+-\d+', text[text.index('DTCDR\'s domain step'):text.index('int cdr_dtcdr_fwd_grad(')])
    tag = int(re.search(r'#define CDR_TAG_DTCDR_FWD_GRAD (\d+)', text).group(1))
    assert tag == 23 and binding.TAGS[tag] == 'dtcdr_fwd_grad_kernel'
    for k, v in (('CDR_DTCDR_MAX_DIM', 128), ('CDR_DTCDR_MAX_HIDDEN', 64), ('CDR_DTCDR_MAX_LAYERS', 3)):
        assert int(re.search(r'#define %s (\d+)' % k, text).group(1)) == v


def test_dtcdr_entry_refuses_bad_shapes_before_any_launch():
    """D = 6, D = 132, a hidden width of 0 or 65, 0 or 4 hidden layers and B = 0 come back as CDR_EINVAL on a machine without a GPU too:
    nothing was launched; the workspace query refuses the same shapes and grows with B up to the persistent grid."""
    from recbole_cdr_amd import binding
    lib = binding.load()
    buf = (ctypes.c_float * 1024)()
    ids = (ctypes.c_int64 * 4)(0, 1, 2, 3)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    ctx = p(buf)                                             # (never dereferenced: the checks come first)
    need = ctypes.c_size_t(0)
    for D, hidden, B in ((6, [12, 6], 4), (132, [12, 6], 4), (8, [0, 6], 4), (8, [12, 65], 4), (8, [], 4), (8, [8, 8, 8, 8], 4),
                         (8, [12, 6], 0), (0, [12, 6], 4), (2, [12, 6], 4)):
        h = (ctypes.c_int * max(len(hidden), 1))(*hidden)
        rc = lib.cdr_dtcdr_fwd_grad(ctx, None, p(buf), p(buf), p(buf), p(buf), D, len(hidden), p(h), p(buf), p(ids), p(ids), p(buf), B, 0.3,
                                    0.0, None, 0, 0, p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), 1 << 20)
        assert rc == -1, (D, hidden, B, rc)                  # CDR_EINVAL
        assert b'cdr_dtcdr_fwd_grad' in lib.cdr_last_error(), (D, hidden, B)
        assert lib.cdr_dtcdr_fwd_grad_workspace_bytes(B, D, len(hidden), p(h), ctypes.byref(need)) == -1, (D, hidden, B)
    # a dropout probability needs its device seed
    h = (ctypes.c_int * 2)(12, 6)
    rc = lib.cdr_dtcdr_fwd_grad(ctx, None, p(buf), p(buf), p(buf), p(buf), 8, 2, p(h), p(buf), p(ids), p(ids), p(buf), 4, 0.3, 0.5, None, 0, 0,
                                p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), 1 << 20)
    assert rc == -1 and b'cdr_dtcdr_fwd_grad' in lib.cdr_last_error()
    one = 4 * n_params(8, [12, 6])
    assert one == 4 * (12 * 16 + 12 + 6 * 12 + 6 + 6 + 1)
    sizes = []
    for B in (1, 33, 32 * 5000):
        assert lib.cdr_dtcdr_fwd_grad_workspace_bytes(B, 8, 2, p(h), ctypes.byref(need)) == 0
        sizes.append(need.value)
    assert sizes[0] == one and sizes[1] == 2 * one and sizes[1] < sizes[2] <= 4096 * one
    assert dtcdr_grid(32 * 5000, 8, [12, 6]) == sizes[2] // one < 5000          # persistent: fewer workgroups than tiles
    # the widest accepted shape is accepted
    h3 = (ctypes.c_int * 3)(64, 64, 64)
    assert lib.cdr_dtcdr_fwd_grad_workspace_bytes(1000, 128, 3, p(h3), ctypes.byref(need)) == 0


def _model(**kw):
    from oracle.common import IdSpace
    from recbole_cdr_amd.model.cross_domain_recommender.dtcdr import DTCDR
    ids = IdSpace(OU=12, TOU=9, SOU=8, OI=4, TOI=14, SOI=16)
    full = dict(embedding_size=8, mlp_hidden_size=[12, 6], dropout_prob=0.0, base_model='NeuMF', alpha=0.3, train_modes=['BOTH'],
                epoch_num=['1'], source_split=False)
    full.update(kw)
    cfg = base_config('cpu', **full)
    torch.manual_seed(0)
    return cfg, DTCDR(cfg, FakeDataset(ids))


def test_trainer_accepts_dtcdr_in_rowwise_mode_and_the_model_has_the_members_it_calls():
    from recbole_cdr_amd.fused import FusedDTCDRStep
    from recbole_cdr_amd.model.cross_domain_recommender.dtcdr import DTCDR
    from recbole_cdr_amd.model.rowwise import RowwiseTraining
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    cfg, model = _model(optimizer_mode='rowwise')
    assert CrossDomainTrainer(cfg, model).optimizer_mode == 'rowwise'
    cfg, model = _model(optimizer_mode='rowwise', rowwise_adam='exact')
    assert CrossDomainTrainer(cfg, model).rowwise_adam == 'exact'
    assert issubclass(DTCDR, RowwiseTraining) and not hasattr(DTCDR, 'fused_graph_key')       # the step runs eagerly
    for name in ('fused_train_step', 'fused_sync', 'fused_replayed', 'fused_optimizer_state', 'load_fused_optimizer_state', '_fused_phase_step'):
        assert callable(getattr(DTCDR, name)), name
    model.fused_sync()                                       # nothing trained yet: a no-op that leaves no state behind
    assert '_fused' not in model.__dict__ and model.fused_optimizer_state() == {}
    assert len([p for tw in model._towers() for p in tw]) == 12 and model.graph_key() == ('DTCDR',)
    FusedDTCDRStep.check_widths(128, [64, 64, 64])
    for D, hidden in ((6, [12]), (132, [12]), (8, []), (8, [1, 2, 3, 4]), (8, [0]), (8, [65])):
        with pytest.raises(ValueError, match='FusedDTCDRStep'):
            FusedDTCDRStep.check_widths(D, hidden)


def test_model_refusals_need_no_gpu_and_leave_no_state():
    """The refusals of fused_train_step come before any launch: they are raised on a CPU model."""
    batch = {f'{d}_{k}': torch.zeros(4, dtype=torch.int64) for d in ('source', 'target') for k in ('user_id', 'item_id')}
    batch.update(source_label=torch.zeros(4), target_label=torch.zeros(4))
    _, m = _model()
    m.set_phase('SOURCE')
    with pytest.raises(ValueError, match='SOURCE batch has no target_user_id, target_item_id, target_label'):
        m.fused_train_step({k: v for k, v in batch.items() if k.startswith('source')})
    with pytest.raises(ValueError, match="opt='adam'"):
        m.fused_train_step(batch, opt='sgd', adam='exact')
    with pytest.raises(ValueError, match="adam must be"):
        m.fused_train_step(batch, adam='dense')
    with pytest.raises(ValueError, match='at least one row per domain'):
        m.fused_train_step(dict(batch, target_user_id=batch['target_user_id'][:0], target_item_id=batch['target_item_id'][:0],
                                target_label=batch['target_label'][:0]))
    with pytest.raises(ValueError, match='ids and labels of equal length'):
        m.fused_train_step(dict(batch, source_label=batch['source_label'][:3]))
    _, md = _model(dist_group=True)
    with pytest.raises(NotImplementedError, match='dist_group'):
        md.fused_train_step(batch)
    for kw, what in ((dict(embedding_size=6), 'embedding_size = 6'), (dict(embedding_size=132), 'embedding_size = 132'),
                     (dict(mlp_hidden_size=[12, 65]), r'mlp_hidden_size = \[12, 65\]'),
                     (dict(mlp_hidden_size=[8, 8, 8, 8]), r'mlp_hidden_size = \[8, 8, 8, 8\]')):
        _, mw = _model(**kw)
        with pytest.raises(ValueError, match=what + '.*optimizer_mode=dense'):
            mw.fused_train_step(batch)
        assert not mw.__dict__.get('_fused')
    assert not m.__dict__.get('_fused', {}).get('states') and not md.__dict__.get('_fused')


# ---------------------------------------------------------------------------------------------------------------------- the yardstick

D_, HIDDEN_, P_ = 8, [12, 6], 0.25


def _case(seed=5, Bs=41, Bt=37, nu=30, ni=26):
    """Tables with exact ties planted: some source rows copied whole into the target table, some in part, and rows in which one table
    loses every element; ids from a range small enough that rows repeat inside a batch and across the two batches."""
    gen = torch.Generator().manual_seed(seed)
    P = {}
    for d in ('source', 'target'):
        P[f'{d}_user_embedding.weight'] = torch.randn(nu, D_, generator=gen) * 0.5
        P[f'{d}_item_embedding.weight'] = torch.randn(ni, D_, generator=gen) * 0.5
        for n, (i, o) in enumerate(zip([2 * D_] + HIDDEN_[:-1], HIDDEN_)):
            P[f'{d}_mlp_layers.mlp_layers.{3 * n + 1}.weight'] = torch.randn(o, i, generator=gen) * (2.0 / (i + o)) ** 0.5
            P[f'{d}_mlp_layers.mlp_layers.{3 * n + 1}.bias'] = torch.randn(o, generator=gen) * 0.1
        P[f'{d}_predict_layer.weight'] = torch.randn(1, HIDDEN_[-1], generator=gen) * 0.5
        P[f'{d}_predict_layer.bias'] = torch.randn(1, generator=gen) * 0.1
    for kind, n in (('user', nu), ('item', ni)):
        S, T = P[f'source_{kind}_embedding.weight'], P[f'target_{kind}_embedding.weight']
        T[0:6] = S[0:6]                                      # whole rows tie
        T[6:12, ::2] = S[6:12, ::2]                          # every other element ties
        T[12:15] = S[12:15] - 1.0                            # the target table loses every element
        T[15:18] = S[15:18] + 1.0                            # the source table loses every element
    r = lambda n, hi: torch.randint(0, hi, (n,), generator=gen)
    inter = {'source_user_id': r(Bs, nu), 'source_item_id': r(Bs, ni), 'source_label': (torch.rand(Bs, generator=gen) < 0.5).float(),
             'target_user_id': r(Bt, nu), 'target_item_id': r(Bt, ni), 'target_label': (torch.rand(Bt, generator=gen) < 0.5).float()}
    inter['source_user_id'][:4] = torch.tensor([0, 7, 13, 16])      # a tied, a half-tied and the two all-loser rows are in both batches
    inter['target_user_id'][:4] = torch.tensor([0, 7, 13, 16])
    inter['source_item_id'][:4] = torch.tensor([1, 8, 14, 17])
    inter['target_item_id'][:4] = torch.tensor([1, 8, 14, 17])
    masks = {}
    for d, B in (('source', Bs), ('target', Bt)):
        for n, w in enumerate([2 * D_] + HIDDEN_[:-1]):
            masks[(d, n)] = (torch.rand(B, w, generator=gen) >= P_).float() * torch.tensor(1.0 / (1.0 - P_), dtype=torch.float32)
    return P, inter, masks


class _MaxFirstWins(torch.autograd.Function):
    """torch.maximum whose backward sends a tie's gradient to the first operand alone (1 : 0 instead of 1/2 : 1/2)."""
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a >= b)
        return torch.maximum(a, b)

    @staticmethod
    def backward(ctx, g):
        first, = ctx.saved_tensors
        return g * first, g * ~first


class _ReluNoMask(torch.autograd.Function):
    """relu whose backward forgets the mask."""
    @staticmethod
    def forward(ctx, x):
        return torch.relu(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _MaskForwardOnly(torch.autograd.Function):
    """x * m whose backward forgets the mask."""
    @staticmethod
    def forward(ctx, x, m):
        return x * m

    @staticmethod
    def backward(ctx, g):
        return g, None


def _mutated_loss(P, inter, alpha, masks, mutation):
    """oracle.dtcdr.calculate_loss restated with one of its three pieces replaced (``mutation`` None: the same function)."""
    from oracle.losses import bce_loss
    mx = _MaxFirstWins.apply if mutation == 'ties' else torch.maximum
    total = 0.0
    for d, w in (('source', alpha), ('target', 1 - alpha)):
        u, i = inter[f'{d}_user_id'], inter[f'{d}_item_id']
        x = torch.cat((mx(P['source_user_embedding.weight'][u], P['target_user_embedding.weight'][u]),
                       mx(P['source_item_embedding.weight'][i], P['target_item_embedding.weight'][i])), -1)
        for n in range(len(HIDDEN_)):
            x = _MaskForwardOnly.apply(x, masks[(d, n)]) if mutation == 'dropout' else x * masks[(d, n)]
            x = x @ P[f'{d}_mlp_layers.mlp_layers.{3 * n + 1}.weight'].t() + P[f'{d}_mlp_layers.mlp_layers.{3 * n + 1}.bias']
            x = _ReluNoMask.apply(x) if mutation == 'relu' and n == 1 else torch.relu(x)
        p = torch.sigmoid(x @ P[f'{d}_predict_layer.weight'].t() + P[f'{d}_predict_layer.bias']).squeeze(-1)
        total = total + w * bce_loss(p, inter[f'{d}_label'])
    return total


def _tower(P, d):
    names = [f'{d}_mlp_layers.mlp_layers.{3 * n + 1}' for n in range(len(HIDDEN_))] + [f'{d}_predict_layer']
    return [P[f'{n}.{k}'] for n in names for k in ('weight', 'bias')]


def _f32_autograd(P0, inter, alpha, masks, mutation='oracle'):
    from oracle import dtcdr as o_dt
    P = {k: v.detach().clone().requires_grad_(True) for k, v in P0.items()}
    loss = o_dt.calculate_loss(P, None, inter, alpha, masks) if mutation == 'oracle' else _mutated_loss(P, inter, alpha, masks, mutation)
    loss.backward()
    return {'loss': float(loss.detach()), 'tables': {t: P[f'{t}_embedding.weight'].grad for t in TABLES},
            'towers': ([p.grad for p in _tower(P, 'source')], [p.grad for p in _tower(P, 'target')])}


def test_fp64_restatement_holds_fp32_autograd_and_rejects_three_mutations():
    """The restatement with any-order depths must hold torch's fp32 autograd of oracle.dtcdr.calculate_loss (every element of the four table
    gradients and the twelve tower gradients, the loss within LOSS_RTOL) and must reject: ties routed 1 : 0 instead of 1/2 : 1/2, the
    second layer's ReLU mask dropped in the backward, and the dropout mask applied in the forward only.  The inputs carry exact ties and
    all-loser rows, and no ReLU unit of the un-mutated result is ambiguous (an ambiguous unit would widen a bound)."""
    alpha = 0.3
    P, inter, masks = _case()
    tabs = tuple(P[f'{t}_embedding.weight'] for t in TABLES)
    ids = [inter[k] for k in ('source_user_id', 'source_item_id', 'target_user_id', 'target_item_id')]
    refs = []
    for d, w in (('source', alpha), ('target', 1 - alpha)):
        refs.append(dtcdr_domain_fp64(tabs, _tower(P, d), inter[f'{d}_user_id'], inter[f'{d}_item_id'], inter[f'{d}_label'], w,
                                      masks=[masks[(d, n)] for n in range(len(HIDDEN_))]))
    assert refs[0]['ambiguous'] == 0 and refs[1]['ambiguous'] == 0
    # the planted rows are what they are meant to be
    su = inter['source_user_id']
    Su, Tu = tabs[0], tabs[2]
    assert bool((Su[su[0]] == Tu[su[0]]).all()) and 0 < int((Su[su[1]] == Tu[su[1]]).sum()) < D_
    assert bool((Su[su[2]] > Tu[su[2]]).all()) and bool((Su[su[3]] < Tu[su[3]]).all())
    assert bool((refs[0]['G']['target_user'].v[2] == 0).all()) and bool((refs[0]['G']['source_user'].v[3] == 0).all())
    assert int(torch.bincount(torch.cat([su, inter['target_user_id']])).max()) > 2          # rows repeat inside and across the batches

    got = _f32_autograd(P, inter, alpha, masks)
    worst = check_dtcdr_result('fp32 autograd', got, refs[0], refs[1], *ids)
    assert len(worst) == 1 + 4 + 12 and all(v <= 1.0 for v in worst.values()), worst
    print('\nfp32 autograd worst error / bound: ' + ' '.join(f'{k}={v:.3g}' for k, v in worst.items()))
    same = _f32_autograd(P, inter, alpha, masks, mutation=None)
    assert max(check_dtcdr_result('restated', same, refs[0], refs[1], *ids).values()) <= 1.0          # the restated loss itself is sound

    for mutation in ('ties', 'relu', 'dropout'):
        with pytest.raises(AssertionError, match='error / bound'):
            check_dtcdr_result(mutation, _f32_autograd(P, inter, alpha, masks, mutation=mutation), refs[0], refs[1], *ids)
    # ties 1 : 0 is caught in the tables, where it lives: the tower gradients do not see the routing
    ties = _f32_autograd(P, inter, alpha, masks, mutation='ties')
    with pytest.raises(AssertionError, match='gradient source_user: error / bound'):
        check_dtcdr_result('ties', ties, refs[0], refs[1], *ids)
