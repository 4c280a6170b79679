"""Host-side checks of DeepAPF's O(batch) row-wise training path (no GPU): header, binding and library agree on the new entry points,
the native entry refuses the shapes it documents before any launch, the trainer accepts the model with ``optimizer_mode='rowwise'``, and
the float64 restatement test_gpu_deepapf_rowwise.py holds the kernel to (deepapf_fp64.py) passes an fp32 torch-autograd result of the
oracle on the CPU, in both overlap modes, and rejects three mutations of it."""
import ctypes
import os
import re

import pytest
import torch

from deepapf_fp64 import PARAMS, ROLES, check_deepapf_result, deepapf_domain_fp64, deepapf_grid, n_params
from helpers import FakeDataset, base_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------- boundary

def test_header_binding_and_library_agree_on_the_deepapf_entry_points():
    from recbole_cdr_amd import binding
    text = open(os.path.join(ROOT, 'include', 'cdr_hip.h')).read()
    assert int(re.search(r'#define CDR_ABI_VERSION (\d+)', text).group(1)) == binding.ABI_VERSION == 64     # (adding entries changes no signature)
    lib = binding.load()
    assert lib.cdr_abi_version() == binding.ABI_VERSION
    plain = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, nargs in (('cdr_deepapf_fwd_grad', 21), ('cdr_deepapf_fwd_grad_workspace_bytes', 3)):
        assert name in binding.exported_symbols() and len(binding._SIGNATURES[name]) == nargs
        decl = re.search(r'int %s\((.*?)\);' % name, plain, flags=re.S).group(1)
        assert len(decl.split(',')) == nargs, name
        assert hasattr(lib, name), name
    assert re.search(r'deepapf\.py:\d+-\d+', text[text.index('DeepAPF\'s domain step'):text.index('int cdr_deepapf_fwd_grad(')])
    tag = int(re.search(r'#define CDR_TAG_DEEPAPF_FWD_GRAD (\d+)', text).group(1))
    assert tag == 24 and binding.TAGS[tag] == 'deepapf_fwd_grad_kernel'
    assert int(re.search(r'#define CDR_DEEPAPF_MAX_DIM (\d+)', text).group(1)) == 128


def test_deepapf_entry_refuses_bad_shapes_before_any_launch():
    """D = 6, D = 132, D = 0, D = 2 and B = 0 come back as CDR_EINVAL on a machine without a GPU too: nothing was launched; the workspace
    query refuses the same shapes, grows with B up to the persistent grid and is grid x (D D + 3 D) x 4."""
    from recbole_cdr_amd import binding
    lib = binding.load()
    buf = (ctypes.c_float * 1024)()
    ids = (ctypes.c_int64 * 4)(0, 1, 2, 3)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    ctx = p(buf)                                             # (never dereferenced: the checks come first)
    need = ctypes.c_size_t(0)
    for D, B in ((6, 4), (132, 4), (0, 4), (2, 4), (8, 0)):
        rc = lib.cdr_deepapf_fwd_grad(ctx, None, p(buf), p(buf), p(buf), D, p(buf), p(ids), p(ids), p(buf), B, 2, 1.0, 0, p(buf), p(buf), p(buf),
                                      p(buf), p(buf), p(buf), 1 << 20)
        assert rc == -1, (D, B, rc)                          # CDR_EINVAL
        assert b'cdr_deepapf_fwd_grad' in lib.cdr_last_error() and b'workspace_bytes' not in lib.cdr_last_error(), (D, B)
        assert lib.cdr_deepapf_fwd_grad_workspace_bytes(B, D, ctypes.byref(need)) == -1, (D, B)
        assert b'cdr_deepapf_fwd_grad_workspace_bytes' in lib.cdr_last_error(), (D, B)
    one = 4 * n_params(8)
    assert one == 4 * (8 * 8 + 3 * 8)
    sizes = []
    for B in (1, 33, 32 * 5000):
        assert lib.cdr_deepapf_fwd_grad_workspace_bytes(B, 8, ctypes.byref(need)) == 0
        sizes.append(need.value)
    assert sizes[0] == one and sizes[1] == 2 * one and sizes[1] < sizes[2] <= 4096 * one
    assert deepapf_grid(32 * 5000, 8) == sizes[2] // one < 5000          # persistent: fewer workgroups than tiles
    # the widest accepted shape is accepted, and there the grid is one workgroup per compute unit
    assert lib.cdr_deepapf_fwd_grad_workspace_bytes(1 << 20, 128, ctypes.byref(need)) == 0
    assert need.value == 256 * 4 * n_params(128)


def _ids(mode):
    from oracle.common import IdSpace
    return IdSpace(OU=10, TOU=10, SOU=10, OI=1, TOI=12, SOI=13) if mode == 'overlap_users' else \
        IdSpace(OU=1, TOU=12, SOU=13, OI=10, TOI=10, SOI=10)


def _model(mode='overlap_users', **kw):
    from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
    full = dict(embedding_size=8, beta=0.5, train_modes=['BOTH'], epoch_num=['1'], source_split=False)
    full.update(kw)
    cfg = base_config('cpu', **full)
    torch.manual_seed(0)
    return cfg, DeepAPF(cfg, FakeDataset(_ids(mode)))


def test_trainer_accepts_deepapf_in_rowwise_mode_and_the_model_has_the_members_it_calls():
    from recbole_cdr_amd.fused import FusedDeepAPFStep
    from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
    from recbole_cdr_amd.model.rowwise import RowwiseTraining
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    cfg, model = _model(optimizer_mode='rowwise')
    assert CrossDomainTrainer(cfg, model).optimizer_mode == 'rowwise'
    cfg, model = _model(optimizer_mode='rowwise', rowwise_adam='exact')
    assert CrossDomainTrainer(cfg, model).rowwise_adam == 'exact'
    assert issubclass(DeepAPF, RowwiseTraining) and not hasattr(DeepAPF, 'fused_graph_key')       # the step runs eagerly
    for name in ('fused_train_step', 'fused_sync', 'fused_replayed', 'fused_optimizer_state', 'load_fused_optimizer_state', '_fused_phase_step'):
        assert callable(getattr(DeepAPF, name)), name
    model.fused_sync()                                       # nothing trained yet: a no-op that leaves no state behind
    assert '_fused' not in model.__dict__ and model.fused_optimizer_state() == {}
    assert model.graph_key() == ('DeepAPF',)
    # the roles follow the mode: the other share table and the other MLP are not part of the step
    names, mlp, n_over, kind = model._roles()
    assert names[0] == 'share_user_embedding' and kind == 'user' and mlp is model.user_mlp and n_over == 10
    assert [tuple(q.shape) for q in model._attention_params()] == [(8, 8), (8,), (1, 8), (1, 8)]
    _, mi = _model('overlap_items')
    names, mlp, n_over, kind = mi._roles()
    assert names == ('share_item_embedding', 'source_item_embedding', 'source_user_embedding', 'target_item_embedding', 'target_user_embedding')
    assert kind == 'item' and mlp is mi.item_mlp and n_over == 10
    FusedDeepAPFStep.check_widths(128)
    FusedDeepAPFStep.check_widths(4)
    for D in (6, 132, 0, 2):
        with pytest.raises(ValueError, match='FusedDeepAPFStep'):
            FusedDeepAPFStep.check_widths(D)


def test_model_refusals_need_no_gpu_and_leave_no_state():
    """The refusals of fused_train_step come before any launch: they are raised on a CPU model."""
    batch = {f'{d}_{k}': torch.zeros(4, dtype=torch.int64) for d in ('source', 'target') for k in ('user_id', 'item_id')}
    batch.update(source_label=torch.zeros(4), target_label=torch.zeros(4))
    _, m = _model()
    m.set_phase('SOURCE')
    with pytest.raises(ValueError, match='SOURCE batch has no target_user_id, target_item_id, target_label'):
        m.fused_train_step({k: v for k, v in batch.items() if k.startswith('source')})
    m.set_phase('BOTH')
    with pytest.raises(ValueError, match="opt='adam'"):
        m.fused_train_step(batch, opt='sgd', adam='exact')
    with pytest.raises(ValueError, match="adam must be"):
        m.fused_train_step(batch, adam='dense')
    with pytest.raises(ValueError, match='BOTH batch needs at least one row per domain'):
        m.fused_train_step(dict(batch, target_user_id=batch['target_user_id'][:0], target_item_id=batch['target_item_id'][:0],
                                target_label=batch['target_label'][:0]))
    with pytest.raises(ValueError, match='ids and labels of equal length'):
        m.fused_train_step(dict(batch, source_label=batch['source_label'][:3]))
    _, md = _model(dist_group=True)
    with pytest.raises(NotImplementedError, match='dist_group'):
        md.fused_train_step(batch)
    for D in (6, 132):
        _, mw = _model(embedding_size=D)
        with pytest.raises(ValueError, match=f'embedding_size = {D}.*optimizer_mode=dense'):
            mw.fused_train_step(batch)
        assert '_fused' not in mw.__dict__
    assert '_fused' not in m.__dict__ and '_fused' not in md.__dict__


# ---------------------------------------------------------------------------------------------------------------------- the yardstick

D_, N_OVER = 12, 10


def _case(mode, seed=3, Bs=40, Bt=33):
    """Both id spaces small enough that rows repeat inside a batch and across the two batches; the keys n_overlap - 1, n_overlap (not
    masked) and n_overlap + 1 (masked) are in both batches."""
    ids = _ids(mode)
    key, oth = ('user', 'item') if mode == 'overlap_users' else ('item', 'user')
    nk, no = (ids.total_num_users, ids.total_num_items) if key == 'user' else (ids.total_num_items, ids.total_num_users)
    gen = torch.Generator().manual_seed(seed)
    P = {}
    for name, n in ((f'share_{key}', nk), (f'share_{oth}', no), (f'source_{key}', nk), (f'target_{key}', nk), (f'source_{oth}', no),
                    (f'target_{oth}', no)):
        P[f'{name}_embedding.weight'] = torch.randn(n, D_, generator=gen) * 0.5
    for pre in ('user_mlp', 'seq'):
        P[f'{pre}.0.weight'] = torch.randn(D_, D_, generator=gen) * (1.0 / D_) ** 0.5
        P[f'{pre}.0.bias'] = torch.randn(D_, generator=gen) * 0.1
        P[f'{pre}.2.weight'] = torch.randn(1, D_, generator=gen) * 0.5
    P['predict_layer.weight'] = torch.randn(1, D_, generator=gen) * 0.5
    r = lambda n, hi: torch.randint(0, hi, (n,), generator=gen)
    inter = {}
    for d, B in (('source', Bs), ('target', Bt)):
        inter[f'{d}_{key}_id'] = r(B, nk)
        inter[f'{d}_{oth}_id'] = r(B, no)
        inter[f'{d}_label'] = (torch.rand(B, generator=gen) < 0.5).float()
        inter[f'{d}_{key}_id'][:3] = torch.tensor([N_OVER - 1, N_OVER, N_OVER + 1])
    return ids, P, inter, key, oth


class _SoftmaxNoDot(torch.autograd.Function):
    """The pair softmax whose backward forgets the ``- dot`` term: ga = al (.) d instead of al (.) (d - <al, d>)."""
    @staticmethod
    def forward(ctx, a):
        al = torch.softmax(a, dim=1)
        ctx.save_for_backward(al)
        return al

    @staticmethod
    def backward(ctx, g):
        al, = ctx.saved_tensors
        return al * g


def _domain_loss(P, ids, inter, d, key, oth, mutation):
    """oracle.deepapf.forward + bce_loss of one domain restated, with one piece replaced by ``mutation``."""
    from oracle.losses import bce_loss
    k, o = inter[f'{d}_{key}_id'], inter[f'{d}_{oth}_id']
    share, only, other = P[f'share_{key}_embedding.weight'][k], P[f'{d}_{key}_embedding.weight'][k], P[f'{d}_{oth}_embedding.weight'][o]
    pre = 'user_mlp' if key == 'user' else 'seq'
    att = lambda x: torch.relu(x @ P[f'{pre}.0.weight'].t() + P[f'{pre}.0.bias']) @ P[f'{pre}.2.weight'].t()
    n_over = ids.overlapped_num_users if key == 'user' else ids.overlapped_num_items
    mask = ((k >= n_over) if mutation == 'mask' else (k > n_over)).unsqueeze(-1)
    a = torch.cat([att(share * other).masked_fill(mask, -1e31), att(only * other)], dim=1)
    al = (_SoftmaxNoDot.apply(a) if mutation == 'softmax' else torch.softmax(a, dim=1)).unsqueeze(1)
    e = (al * torch.cat([share.unsqueeze(2), only.unsqueeze(2)], dim=2)).sum(dim=2)
    p = torch.sigmoid((e * other) @ P['predict_layer.weight'].t()).squeeze(-1)
    return bce_loss(p, inter[f'{d}_label'])


def _f32_autograd(P0, ids, inter, key, oth, mutation='oracle'):
    from oracle import deepapf as o_apf
    P = {n: v.detach().clone().requires_grad_(True) for n, v in P0.items()}
    if mutation == 'oracle':
        loss = o_apf.calculate_loss(P, ids, inter)
    else:
        loss = _domain_loss(P, ids, inter, 'source', key, oth, mutation) + _domain_loss(P, ids, inter, 'target', key, oth, mutation)
    loss.backward()
    pre = 'user_mlp' if key == 'user' else 'seq'
    names = (f'{pre}.0.weight', f'{pre}.0.bias', f'{pre}.2.weight', 'predict_layer.weight')
    params = [P[n].grad for n in names]
    if mutation == 'one_domain':                             # dP of the source domain alone
        Q = {n: v.detach().clone().requires_grad_(True) for n, v in P0.items()}
        _domain_loss(Q, ids, inter, 'source', key, oth, None).backward()
        params = [Q[n].grad for n in names]
    tables = {'share': P[f'share_{key}_embedding.weight'].grad, 'source_only': P[f'source_{key}_embedding.weight'].grad,
              'source_other': P[f'source_{oth}_embedding.weight'].grad, 'target_only': P[f'target_{key}_embedding.weight'].grad,
              'target_other': P[f'target_{oth}_embedding.weight'].grad}
    unused = [n for n, v in P.items() if v.grad is None]
    return {'loss': float(loss.detach()), 'tables': tables, 'params': params}, unused


@pytest.mark.parametrize('mode', ['overlap_users', 'overlap_items'])
def test_fp64_restatement_holds_fp32_autograd_and_rejects_three_mutations(mode):
    """The restatement with any-order depths must hold torch's fp32 autograd of oracle.deepapf.calculate_loss (every element of the five
    table gradients and of the four parameter gradients, the loss within LOSS_RTOL) and must reject: ``>=`` in place of ``>`` in the mask,
    the softmax gradient without the ``- dot`` term, and the parameter gradient of one domain only.  D = 12, 40 + 33 rows; the keys
    n_overlap - 1, n_overlap and n_overlap + 1 are in both batches; no ReLU unit of the seeded input is ambiguous (an ambiguous unit would
    widen a bound)."""
    ids, P, inter, key, oth = _case(mode)
    pre = 'user_mlp' if key == 'user' else 'seq'
    params = [P[f'{pre}.0.weight'], P[f'{pre}.0.bias'], P[f'{pre}.2.weight'], P['predict_layer.weight']]
    refs = []
    for d in ('source', 'target'):
        refs.append(deepapf_domain_fp64(P[f'share_{key}_embedding.weight'], P[f'{d}_{key}_embedding.weight'], P[f'{d}_{oth}_embedding.weight'],
                                        params, inter[f'{d}_{key}_id'], inter[f'{d}_{oth}_id'], inter[f'{d}_label'], N_OVER))
    assert refs[0]['ambiguous'] == 0 and refs[1]['ambiguous'] == 0
    id4 = [inter[f'{d}_{x}_id'] for d in ('source', 'target') for x in (key, oth)]
    # the planted keys are what they are meant to be: n_overlap keeps its share row, n_overlap + 1 does not
    for ref in refs:
        assert ref['masked'][:3].tolist() == [False, False, True]
        assert float(ref['al_s'].v[1]) > 0 and float(ref['al_s'].v[2]) == 0 and bool((ref['GS'].v[2] == 0).all()) and bool((ref['GS'].v[1] != 0).any())
        assert 0 < int(ref['masked'].sum()) < ref['masked'].numel()
    assert int(torch.bincount(torch.cat([id4[0], id4[2]])).max()) > 2              # rows repeat inside and across the batches

    got, unused = _f32_autograd(P, ids, inter, key, oth)
    # the MLP the mode does not use and the other side's share table have no gradient in the reference
    other_pre = 'seq' if key == 'user' else 'user_mlp'
    assert sorted(unused) == sorted([f'{other_pre}.0.weight', f'{other_pre}.0.bias', f'{other_pre}.2.weight', f'share_{oth}_embedding.weight'])
    worst = check_deepapf_result('fp32 autograd', got, refs[0], refs[1], *id4)
    assert len(worst) == 1 + len(ROLES) + len(PARAMS) and all(v <= 1.0 for v in worst.values()), worst
    print('\nfp32 autograd worst error / bound: ' + ' '.join(f'{k}={v:.3g}' for k, v in worst.items()))
    same, _ = _f32_autograd(P, ids, inter, key, oth, mutation=None)
    assert max(check_deepapf_result('restated', same, refs[0], refs[1], *id4).values()) <= 1.0          # the restated loss itself is sound

    # (the mask moves the forward too: it is caught at the first comparison, the loss; the other two leave the loss alone)
    for mutation, caught in (('mask', 'loss: .* vs fp64'), ('softmax', 'error / bound'), ('one_domain', 'error / bound')):
        with pytest.raises(AssertionError, match=caught):
            check_deepapf_result(mutation, _f32_autograd(P, ids, inter, key, oth, mutation=mutation)[0], refs[0], refs[1], *id4)
    # with the right loss in its place, the mask mutation is caught in the share table's rows of key == n_overlap
    masked = dict(_f32_autograd(P, ids, inter, key, oth, mutation='mask')[0], loss=got['loss'])
    with pytest.raises(AssertionError, match='gradient share: error / bound'):
        check_deepapf_result('mask', masked, refs[0], refs[1], *id4)
    # the one-domain parameter gradient is caught in the parameters, where it lives: the tables do not see it
    with pytest.raises(AssertionError, match='gradient W1: error / bound'):
        check_deepapf_result('one_domain', _f32_autograd(P, ids, inter, key, oth, mutation='one_domain')[0], refs[0], refs[1], *id4)
