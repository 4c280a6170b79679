"""Host-side checks of DCDCSR's O(batch) row-wise training path (no GPU): header, binding and library agree on the new entry points,
the native entry refuses the shapes it documents before any launch, the trainer accepts the model with ``optimizer_mode='rowwise'``, and
the float64 restatement test_gpu_dcdcsr_rowwise.py holds the kernel to (dcdcsr_fp64.py) passes an fp32 torch-autograd result of the
oracle's map loss on the CPU, in both overlap modes, and rejects three mutations of it."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dcdcsr_fp64 import check_dcdcsr_result, dcdcsr_grid, dcdcsr_map_fp64, n_params
from helpers import FakeDataset, base_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------- boundary

def test_header_binding_and_library_agree_on_the_dcdcsr_entry_points():
    from recbole_cdr_amd import binding
    text = open(os.path.join(ROOT, 'include', 'cdr_hip.h')).read()
    assert int(re.search(r'#define CDR_ABI_VERSION (\d+)', text).group(1)) == binding.ABI_VERSION == 64     # (adding entries changes no signature)
    lib = binding.load()
    assert lib.cdr_abi_version() == binding.ABI_VERSION
    plain = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, nargs in (('cdr_dcdcsr_map_fwd_grad', 14), ('cdr_dcdcsr_map_fwd_grad_workspace_bytes', 4)):
        assert name in binding.exported_symbols() and len(binding._SIGNATURES[name]) == nargs
        decl = re.search(r'int %s\((.*?)\);' % name, plain, flags=re.S).group(1)
        assert len(decl.split(',')) == nargs, name
        assert hasattr(lib, name), name
    assert re.search(r'dcdcsr\.py:172-187', text[text.index('DCDCSR\'s BOTH-phase map step'):text.index('int cdr_dcdcsr_map_fwd_grad(')])
    tag = int(re.search(r'#define CDR_TAG_DCDCSR_MAP_FWD_GRAD (\d+)', text).group(1))
    assert tag == 25 and binding.TAGS[tag] == 'dcdcsr_map_kernel'
    assert int(re.search(r'#define CDR_DCDCSR_MAX_DIM (\d+)', text).group(1)) == 128
    assert int(re.search(r'#define CDR_DCDCSR_MAX_LAYERS (\d+)', text).group(1)) == 3


def _cdims(dims):
    return (ctypes.c_int * len(dims))(*dims)


def test_dcdcsr_entry_refuses_bad_shapes_before_any_launch():
    """A width of 6, 132 or 0, L = 0, L = 4, dims[0] != dims[L] and n = 0 come back as CDR_EINVAL on a machine without a GPU too: nothing
    was launched; NULL for bench and for the id list likewise; the workspace query refuses the same shapes, grows with n up to the
    persistent grid and is grid x packed-parameter-count x 4."""
    from recbole_cdr_amd import binding
    lib = binding.load()
    buf = (ctypes.c_float * 1024)()
    ids = (ctypes.c_int64 * 4)(0, 1, 2, 3)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    ctx = p(buf)                                             # (never dereferenced: the checks come first)
    need = ctypes.c_size_t(0)
    bad = [((8, 6, 8), 4), ((8, 132, 8), 4), ((8, 0, 8), 4), ((132, 132), 4), ((8,), 4), ((8, 8, 8, 8, 8), 4), ((8, 12, 12), 4), ((8, 12, 8), 0)]
    for dims, n in bad:
        L = len(dims) - 1
        rc = lib.cdr_dcdcsr_map_fwd_grad(ctx, None, p(buf), p(buf), p(ids), n, L, _cdims(dims), p(buf), p(buf), p(buf), p(buf), p(buf), 1 << 20)
        assert rc == -1, (dims, n, rc)                       # CDR_EINVAL
        assert b'cdr_dcdcsr_map_fwd_grad' in lib.cdr_last_error() and b'workspace_bytes:' not in lib.cdr_last_error(), (dims, n)
        assert lib.cdr_dcdcsr_map_fwd_grad_workspace_bytes(n, L, _cdims(dims), ctypes.byref(need)) == -1, (dims, n)
        assert b'cdr_dcdcsr_map_fwd_grad_workspace_bytes' in lib.cdr_last_error(), (dims, n)
    ok = (8, 12, 8)
    for bench, idl in ((None, p(ids)), (p(buf), None)):
        rc = lib.cdr_dcdcsr_map_fwd_grad(ctx, None, p(buf), bench, idl, 4, 2, _cdims(ok), p(buf), p(buf), p(buf), p(buf), p(buf), 1 << 20)
        assert rc == -1 and b'cdr_dcdcsr_map_fwd_grad' in lib.cdr_last_error()
    one = 4 * n_params(ok)
    assert one == 4 * (12 * 8 + 12 + 8 * 12 + 8)
    sizes = []
    for n in (1, 33, 32 * 5000):
        assert lib.cdr_dcdcsr_map_fwd_grad_workspace_bytes(n, 2, _cdims(ok), ctypes.byref(need)) == 0
        sizes.append(need.value)
    assert sizes[0] == one and sizes[1] == 2 * one and sizes[1] < sizes[2] <= 4096 * one
    assert dcdcsr_grid(32 * 5000, ok) == sizes[2] // one < 5000           # persistent: fewer workgroups than tiles
    # the default shape, 128-[128]-128 and the widest three-layer shape are accepted
    for dims in ((64, 128, 64), (128, 128, 128), (128, 128, 128, 128), (4, 4)):
        assert lib.cdr_dcdcsr_map_fwd_grad_workspace_bytes(1 << 20, len(dims) - 1, _cdims(dims), ctypes.byref(need)) == 0, dims
        assert need.value % (4 * n_params(dims)) == 0 and 256 <= need.value // (4 * n_params(dims)) <= 512


def _ids(mode):
    from oracle.common import IdSpace
    return IdSpace(OU=10, TOU=10, SOU=10, OI=1, TOI=12, SOI=13) if mode == 'overlap_users' else \
        IdSpace(OU=1, TOU=12, SOU=13, OI=10, TOI=10, SOI=10)


def _pairs(ids, seed=0):
    """Every source / target user and item appears (the popularities are divided by)."""
    rng = np.random.RandomState(seed)
    src_u = np.r_[1:ids.OU, ids.OU + ids.TOU:ids.total_num_users]
    src_i = np.r_[1:ids.OI, ids.OI + ids.TOI:ids.total_num_items]
    tgt_u, tgt_i = np.arange(1, ids.OU + ids.TOU), np.arange(1, ids.OI + ids.TOI)
    full = lambda us, its: np.concatenate([np.stack([us, rng.choice(its, len(us))], 1), np.stack([rng.choice(us, len(its)), its], 1)])
    return full(src_u, src_i), full(tgt_u, tgt_i)


def _model(mode='overlap_users', **kw):
    from recbole_cdr_amd.model.cross_domain_recommender.dcdcsr import DCDCSR
    full = dict(latent_factor_model='BPR', embedding_size=8, mlp_hidden_size=[12], k=3, map_batch_size=9,
                train_modes=['SOURCE', 'TARGET', 'BOTH', 'TARGET'], epoch_num=['1', '1', '1', '1'], source_split=False)
    full.update(kw)
    cfg = base_config('cpu', **full)
    torch.manual_seed(0)
    ids = _ids(mode)
    return cfg, DCDCSR(cfg, FakeDataset(ids, *_pairs(ids)))


def test_trainer_accepts_dcdcsr_in_rowwise_mode_and_the_model_has_the_members_it_calls():
    from recbole_cdr_amd.fused import FusedDCDCSRMapStep, FusedFrozenSideBPRStep
    from recbole_cdr_amd.model.cross_domain_recommender.dcdcsr import DCDCSR
    from recbole_cdr_amd.model.rowwise import RowwiseTraining
    from recbole_cdr_amd.trainer import DCDCSRTrainer
    cfg, model = _model(optimizer_mode='rowwise')
    assert DCDCSRTrainer(cfg, model).optimizer_mode == 'rowwise'
    cfg, model = _model(optimizer_mode='rowwise', rowwise_adam='exact')
    assert DCDCSRTrainer(cfg, model).rowwise_adam == 'exact'
    assert issubclass(DCDCSR, RowwiseTraining) and not hasattr(DCDCSR, 'fused_graph_key')         # every phase runs eagerly
    for name in ('fused_train_step', 'fused_sync', 'fused_replayed', 'fused_optimizer_state', 'load_fused_optimizer_state', '_fused_phase_step',
                 '_fused_bpr_domain_step'):
        assert callable(getattr(DCDCSR, name)), name
    model.fused_sync()                                       # nothing trained yet: a no-op that leaves no state behind
    assert '_fused' not in model.__dict__ and model.fused_optimizer_state() == {}
    assert [tuple(q.shape) for pair in model._mlp_pairs() for q in pair] == [(12, 8), (12,), (8, 12), (8,)]
    assert callable(FusedFrozenSideBPRStep.step)
    for dims in ([64, 128, 64], [128, 128, 128], [4, 4], [8, 12, 16, 8]):
        FusedDCDCSRMapStep.check_widths(dims)
    for dims in ([8, 6, 8], [8, 132, 8], [8, 0, 8], [8], [8, 8, 8, 8, 8], [8, 12, 12]):
        with pytest.raises(ValueError, match='FusedDCDCSRMapStep'):
            FusedDCDCSRMapStep.check_widths(dims)


def test_model_refusals_need_no_gpu_and_leave_no_state():
    """The refusals of fused_train_step come before any launch: they are raised on a CPU model."""
    z = torch.zeros(4, dtype=torch.int64)
    batch = {'target_user_id': z, 'target_item_id': z, 'neg_target_item_id': z, 'source_user_id': z, 'source_item_id': z, 'neg_source_item_id': z}
    _, m = _model()
    m.set_phase('SOURCE')
    with pytest.raises(ValueError, match="adam must be"):
        m.fused_train_step(batch, adam='dense')
    with pytest.raises(ValueError, match="opt='adam'"):
        m.fused_train_step(batch, opt='sgd', adam='exact')
    with pytest.raises(ValueError, match='SOURCE phase on SOURCE triples; the batch has no source_user_id, source_item_id, neg_source_item_id'):
        m.fused_train_step({k: v for k, v in batch.items() if 'target' in k})
    with pytest.raises(ValueError, match='at least one triple and id lists of equal length'):
        m.fused_train_step(dict(batch, source_user_id=z[:0], source_item_id=z[:0], neg_source_item_id=z[:0]))
    with pytest.raises(ValueError, match='id lists of equal length'):
        m.fused_train_step(dict(batch, neg_source_item_id=z[:3]))
    m.set_phase('SOURCE')                                    # a second SOURCE visit: calculate_loss has no loss there
    assert m.calculate_loss(batch) is None
    with pytest.raises(ValueError, match="visit 2 of phase 'SOURCE'"):
        m.fused_train_step(batch)
    m.phase = 'OVERLAP'
    with pytest.raises(ValueError, match="visit 0 of phase 'OVERLAP'"):
        m.fused_train_step(batch)
    _, md = _model(dist_group=True)
    md.set_phase('SOURCE')
    with pytest.raises(NotImplementedError, match='dist_group'):
        md.fused_train_step(batch)
    for hidden in ([6], [132], [8, 8, 8]):
        _, mw = _model(mlp_hidden_size=hidden)
        mw.set_phase('SOURCE')                               # (the widths are refused in every phase, not only in BOTH)
        with pytest.raises(ValueError, match=r'mapping MLP widths \[8, .*optimizer_mode=dense$'):
            mw.fused_train_step(batch)
        assert '_fused' not in mw.__dict__
    _, me = _model(embedding_size=6, mlp_hidden_size=[8])
    me.set_phase('SOURCE')
    with pytest.raises(ValueError, match='embedding_size % 4 == 0.*got 6; use optimizer_mode=dense'):
        me.fused_train_step(batch)
    assert '_fused' not in m.__dict__ and '_fused' not in md.__dict__ and '_fused' not in me.__dict__


# ---------------------------------------------------------------------------------------------------------------------- the yardstick

D_, HID, N_ = 12, [20], 40


def _case(mode, seed=3):
    """The unit table, a benchmark table, the MLP and n = 40 ids over the 19 or 10 target units (rows repeat); unit row 3 has two tied
    maxima, unit row 5 two tied minima, and both are sampled."""
    ids = _ids(mode)
    unit = 'user' if mode == 'overlap_users' else 'item'
    total, n_tgt = (ids.total_num_users, ids.target_num_users) if unit == 'user' else (ids.total_num_items, ids.target_num_items)
    gen = torch.Generator().manual_seed(seed)
    T = torch.randn(total, D_, generator=gen) * 0.5
    T[3, 7] = T[3, 2] = T[3].max() + 0.25
    T[5, 1] = T[5, 9] = T[5].min() - 0.25
    bench = torch.randn(total, D_, generator=gen) * 0.5
    dims = [D_] + HID + [D_]
    P = {f'target_{unit}_embedding.weight': T}
    for l in range(len(dims) - 1):
        P[f'mapping_mlp_layers.mlp_layers.{3 * l + 1}.weight'] = torch.randn(dims[l + 1], dims[l], generator=gen) * (1.0 / dims[l]) ** 0.5
        P[f'mapping_mlp_layers.mlp_layers.{3 * l + 1}.bias'] = torch.randn(dims[l + 1], generator=gen) * 0.1
    idx = torch.randint(0, n_tgt, (N_,), generator=gen)
    idx[:3] = torch.tensor([3, 5, 3])
    return ids, unit, P, bench, idx


def _first_max_normalize(w):
    """maxmin_normalize with torch.max / torch.min over a dimension: their backward gives the whole gradient to ONE arg-max / arg-min."""
    min_ = torch.min(w, dim=1, keepdim=True).values
    max_ = torch.max(w, dim=1, keepdim=True).values
    mean_ = (max_ + min_) / 2
    return (w - mean_) / (max_ - mean_)


def _restated_loss(P, unit, bench, idx, mutation):
    """oracle.dcdcsr.map_loss restated, with one piece replaced by ``mutation``."""
    from oracle.dcdcsr import maxmin_normalize
    norm = _first_max_normalize if mutation == 'tie_first' else (lambda w: maxmin_normalize(w)[0])
    x = norm(P[f'target_{unit}_embedding.weight'][idx])
    b = maxmin_normalize(bench[idx])[0]
    n = 1
    while f'mapping_mlp_layers.mlp_layers.{n}.weight' in P:
        x = x @ P[f'mapping_mlp_layers.mlp_layers.{n}.weight'].t() + P[f'mapping_mlp_layers.mlp_layers.{n}.bias']
        last = f'mapping_mlp_layers.mlp_layers.{n + 3}.weight' not in P
        if not (last and mutation == 'no_last_tanh'):
            x = torch.tanh(x)
        n += 3
    sq = (x - b) ** 2
    return sq.sum() / idx.numel() if mutation == 'mean_n' else sq.mean()


def _names(P):
    out, n = [], 1
    while f'mapping_mlp_layers.mlp_layers.{n}.weight' in P:
        out += [f'mapping_mlp_layers.mlp_layers.{n}.weight', f'mapping_mlp_layers.mlp_layers.{n}.bias']
        n += 3
    return out


def _f32_autograd(P0, ids, unit, bench, idx, mutation='oracle'):
    from oracle import dcdcsr as o
    P = {n: v.detach().clone().requires_grad_(True) for n, v in P0.items()}
    loss = o.map_loss(P, ids, bench, idx) if mutation == 'oracle' else _restated_loss(P, unit, bench, idx, mutation)
    loss.backward()
    return {'loss': float(loss.detach()), 'table': P[f'target_{unit}_embedding.weight'].grad, 'params': [P[n].grad for n in _names(P)]}


@pytest.mark.parametrize('mode', ['overlap_users', 'overlap_items'])
def test_fp64_restatement_holds_fp32_autograd_and_rejects_three_mutations(mode):
    """The restatement with any-order depths must hold torch's fp32 autograd of oracle.dcdcsr.map_loss (every element of the unit table's
    gradient and of the four parameter gradients, the loss within LOSS_RTOL) and must reject: the tie split given wholly to the first
    arg-max (and arg-min), the last layer's tanh dropped, and the mean taken over n instead of n D.  D = 12, hidden [20], n = 40 over at
    most 19 units; a row with two tied maxima and one with two tied minima are sampled, the first of them twice."""
    ids, unit, P, bench, idx = _case(mode)
    params = [P[n] for n in _names(P)]
    T = P[f'target_{unit}_embedding.weight']
    ref = dcdcsr_map_fp64(T, bench, params, idx)
    nmax, nmin = ref['ties']
    assert nmax[:3].tolist() == [2, 1, 2] and nmin[:3].tolist() == [1, 2, 1]
    assert int(torch.bincount(idx).max()) > 2                 # rows repeat

    got = _f32_autograd(P, ids, unit, bench, idx)
    worst = check_dcdcsr_result('fp32 autograd', got, ref, idx)
    assert len(worst) == 2 + len(params) and all(v <= 1.0 for v in worst.values()), worst
    print('\nfp32 autograd worst error / bound: ' + ' '.join(f'{k}={v:.3g}' for k, v in worst.items()))
    same = _f32_autograd(P, ids, unit, bench, idx, mutation=None)
    assert max(check_dcdcsr_result('restated', same, ref, idx).values()) <= 1.0            # the restated loss itself is sound

    # (the tie split leaves the forward alone: caught in the table's gradient; the other two move the loss: caught at the first comparison)
    for mutation, caught in (('tie_first', 'gradient table: error / bound'), ('no_last_tanh', 'loss: .* vs fp64'), ('mean_n', 'loss: .* vs fp64')):
        with pytest.raises(AssertionError, match=caught):
            check_dcdcsr_result(mutation, _f32_autograd(P, ids, unit, bench, idx, mutation=mutation), ref, idx)
    # with the right loss in their place, those two are caught in the gradients
    for mutation in ('no_last_tanh', 'mean_n'):
        with pytest.raises(AssertionError, match='gradient table: error / bound'):
            check_dcdcsr_result(mutation, dict(_f32_autograd(P, ids, unit, bench, idx, mutation=mutation), loss=got['loss']), ref, idx)
    # the tie mutation moves nothing but the tied rows' elements
    tie = _f32_autograd(P, ids, unit, bench, idx, mutation='tie_first')
    moved = (tie['table'] != got['table']).any(1).nonzero().flatten().tolist()
    assert moved == [3, 5], moved
