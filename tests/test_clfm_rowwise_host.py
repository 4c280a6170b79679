"""Host-side checks of CLFM's O(batch) row-wise training path (no GPU): header, binding and library agree on the new entry points,
the trainer accepts the model with ``optimizer_mode='rowwise'``, and the float64 restatement test_gpu_clfm_rowwise.py holds the kernel
to (clfm_fp64.py) passes an fp32 torch-autograd CLFM result on the CPU and rejects three mutations of it."""
import ctypes
import os
import re

import pytest
import torch

from clfm_fp64 import check_clfm_result, clfm_domain_fp64
from helpers import FakeDataset, base_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------- boundary

def test_header_binding_and_library_agree_on_the_clfm_entry_points():
    from recbole_cdr_amd import binding
    text = open(os.path.join(ROOT, 'include', 'cdr_hip.h')).read()
    assert int(re.search(r'#define CDR_ABI_VERSION (\d+)', text).group(1)) == binding.ABI_VERSION == 64
    lib = binding.load()
    assert lib.cdr_abi_version() == binding.ABI_VERSION
    plain = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, nargs in (('cdr_clfm_fwd_grad', 19), ('cdr_clfm_fwd_grad_workspace_bytes', 4)):
        assert name in binding.exported_symbols() and len(binding._SIGNATURES[name]) == nargs
        decl = re.search(r'int %s\((.*?)\);' % name, plain, flags=re.S).group(1)
        assert len(decl.split(',')) == nargs, name
        assert hasattr(lib, name), name
    assert re.search(r'clfm\.py:\d+-\d+', text[text.index('CLFM\'s domain step'):text.index('int cdr_clfm_fwd_grad(')])
    tag = int(re.search(r'#define CDR_TAG_CLFM_FWD_GRAD (\d+)', text).group(1))
    assert binding.TAGS[tag] == 'clfm_fwd_grad_kernel'
    assert int(re.search(r'#define CDR_CLFM_MAX_DIM (\d+)', text).group(1)) == 128


def test_clfm_entry_refuses_bad_shapes_before_any_launch():
    """Du = 6, Di = 132 and B = 0 (and the other edges of 4 <= D <= 128, D % 4 == 0) come back as CDR_EINVAL on a machine without a GPU
    too: nothing was launched; the workspace query refuses the same shapes and grows with B up to the persistent grid."""
    from recbole_cdr_amd import binding
    lib = binding.load()
    buf = (ctypes.c_float * 1024)()
    ids = (ctypes.c_int64 * 4)(0, 1, 2, 3)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    ctx = p(buf)                                             # (never dereferenced: the checks come first)
    need = ctypes.c_size_t(0)
    for Du, Di, B in ((6, 16, 4), (12, 132, 4), (12, 16, 0), (0, 16, 4), (12, 2, 4), (132, 16, 4), (12, 18, 4)):
        rc = lib.cdr_clfm_fwd_grad(ctx, None, p(buf), p(buf), Du, Di, p(buf), p(ids), p(ids), p(buf), B, 0.3, 0.01, p(buf), p(buf), p(buf),
                                   p(buf), p(buf), 1 << 20)
        assert rc == -1, (Du, Di, B, rc)                     # CDR_EINVAL
        assert b'cdr_clfm_fwd_grad' in lib.cdr_last_error(), (Du, Di, B)
        assert lib.cdr_clfm_fwd_grad_workspace_bytes(B, Du, Di, ctypes.byref(need)) == -1, (Du, Di, B)
    sizes = []
    for B in (1, 33, 32 * 5000):
        assert lib.cdr_clfm_fwd_grad_workspace_bytes(B, 12, 16, ctypes.byref(need)) == 0
        sizes.append(need.value)
    assert sizes[0] == 16 * 12 * 4 and sizes[1] == 2 * sizes[0] and sizes[1] < sizes[2] <= 4096 * sizes[0]


def _model(**kw):
    from oracle.common import IdSpace
    from recbole_cdr_amd.model.cross_domain_recommender.clfm import CLFM
    ids = IdSpace(OU=12, TOU=9, SOU=8, OI=4, TOI=14, SOI=16)
    full = dict(user_embedding_size=12, source_item_embedding_size=16, target_item_embedding_size=16, share_embedding_size=6, alpha=0.3,
                reg_weight=0.01, train_modes=['BOTH'], epoch_num=['1'], source_split=False)
    full.update(kw)
    cfg = base_config('cpu', **full)
    torch.manual_seed(0)
    return cfg, CLFM(cfg, FakeDataset(ids))


def test_trainer_accepts_clfm_in_rowwise_mode_and_the_model_has_the_members_it_calls():
    from recbole_cdr_amd.model.cross_domain_recommender.clfm import CLFM
    from recbole_cdr_amd.model.rowwise import RowwiseTraining
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    cfg, model = _model(optimizer_mode='rowwise')
    assert CrossDomainTrainer(cfg, model).optimizer_mode == 'rowwise'
    cfg, model = _model(optimizer_mode='rowwise', rowwise_adam='exact')
    assert CrossDomainTrainer(cfg, model).rowwise_adam == 'exact'
    assert issubclass(CLFM, RowwiseTraining) and not hasattr(CLFM, 'fused_graph_key')       # the step runs eagerly
    for name in ('fused_train_step', 'fused_sync', 'fused_replayed', 'fused_optimizer_state', 'load_fused_optimizer_state', '_fused_phase_step'):
        assert callable(getattr(CLFM, name)), name
    model.fused_sync()                                       # nothing trained yet: a no-op that leaves no state behind
    assert '_fused' not in model.__dict__ and model.fused_optimizer_state() == {}


def test_model_refusals_need_no_gpu_and_leave_no_state():
    """The refusals of fused_train_step come before any launch: they are raised on a CPU model, in the documented order of severity."""
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
    for kw, what in ((dict(user_embedding_size=6, share_embedding_size=6), 'user_embedding_size = 6'),
                     (dict(source_item_embedding_size=132), 'source_item_embedding_size = 132'),
                     (dict(user_embedding_size=18), 'user_embedding_size = 18')):
        _, mw = _model(**kw)
        with pytest.raises(ValueError, match=what):
            mw.fused_train_step(batch)
        assert not mw.__dict__.get('_fused')
    assert not m.__dict__.get('_fused', {}).get('states') and not md.__dict__.get('_fused')


# ---------------------------------------------------------------------------------------------------------------------- the yardstick

def _case(seed=3, Du=16, Di=16, share=8, Bs=300, Bt=257, nu=90, ni=70):
    gen = torch.Generator().manual_seed(seed)
    tabs = [torch.randn(n, D, generator=gen) * 0.1 for n, D in ((nu, Du), (ni, Di), (nu, Du), (ni, Di))]
    xav = lambda r: torch.randn(r, Du, generator=gen) * (2.0 / (r + Du)) ** 0.5
    ws = {'shared': xav(share), 'source_only': xav(Di - share), 'target_only': xav(Di - share)}
    r = lambda n, hi: torch.randint(0, hi, (n,), generator=gen)
    doms = [(r(Bs, nu), r(Bs, ni), (torch.rand(Bs, generator=gen) < 0.5).float()), (r(Bt, nu), r(Bt, ni), (torch.rand(Bt, generator=gen) < 0.5).float())]
    return tabs, ws, doms


def _f32_autograd(tabs, ws, doms, alpha, reg, reg_outside_w=False):
    """CLFM.calculate_loss in fp32 torch autograd on the CPU (clfm.py:74-124): index_select, two linears, cat, BCE, EmbLoss."""
    import torch.nn.functional as tf
    P = [t.detach().clone().requires_grad_(True) for t in tabs]
    Wp = {k: v.detach().clone().requires_grad_(True) for k, v in ws.items()}
    total = 0.0
    for d, ((uid, iid, y), w) in enumerate(zip(doms, (alpha, 1 - alpha))):
        u, i = P[2 * d].index_select(0, uid), P[2 * d + 1].index_select(0, iid)
        only = Wp['source_only' if d == 0 else 'target_only']
        f = torch.cat([tf.linear(u, Wp['shared']), tf.linear(u, only)], 1)
        bce = tf.binary_cross_entropy(torch.sigmoid((f * i).sum(1)), y)
        emb = ((u * u).sum().sqrt() + (i * i).sum().sqrt()) / uid.numel()
        total = total + (w * bce + reg * emb if reg_outside_w else w * (bce + reg * emb))
    total.backward()
    return {'loss': float(total.detach()), 'tables': [p.grad for p in P], 'weights': {k: v.grad for k, v in Wp.items()}}


def test_fp64_restatement_holds_fp32_autograd_and_rejects_three_mutations():
    """The restatement with any-order depths must hold torch's fp32 autograd (every element of the four table gradients and the three
    weight gradients, the loss within LOSS_RTOL), and must reject: the EmbLoss coefficient without the domain weight, W used where W^T
    belongs in the user gradient, and one occurrence dropped from a duplicated row."""
    alpha, reg, share = 0.3, 0.01, 8
    tabs, ws, doms = _case()
    W = [torch.cat([ws['shared'], ws['source_only']]), torch.cat([ws['shared'], ws['target_only']])]
    refs = [clfm_domain_fp64(tabs[2 * d], tabs[2 * d + 1], W[d], *doms[d], w, reg) for d, w in enumerate((alpha, 1 - alpha))]
    got = _f32_autograd(tabs, ws, doms, alpha, reg)
    worst = check_clfm_result('fp32 autograd', got, refs[0], refs[1], share)
    assert len(worst) == 8 and all(v <= 1.0 for v in worst.values()), worst
    print('\nfp32 autograd worst error / bound: ' + ' '.join(f'{k}={v:.3g}' for k, v in worst.items()))
    # (the per-occurrence coefficient and the weight gradient of each domain, from the same autograd pass)
    for d, ref in enumerate(refs):
        assert ref['dW'].v.shape == (16, 16) and ref['GU'].v.shape == (doms[d][0].numel(), 16)

    with pytest.raises(AssertionError, match='error / bound|vs fp64'):
        check_clfm_result('reg coefficient without w', _f32_autograd(tabs, ws, doms, alpha, reg, reg_outside_w=True), refs[0], refs[1], share)

    # the source domain's user gradient rebuilt in fp32 with W in the place of W^T (Du == Di, so the shapes agree)
    uid, iid, y = doms[0]
    u, i = tabs[0][uid], tabs[1][iid]
    p = torch.sigmoid(((u @ W[0].t()) * i).sum(1))
    g = (alpha * (p - y) / uid.numel()).unsqueeze(1)
    cu = alpha * reg / (uid.numel() * u.norm())
    def user_grad(M, keep=None):
        rows = g * (i @ M) + cu * u
        if keep is not None:
            rows = rows * keep.unsqueeze(1)
        return torch.zeros_like(tabs[0]).index_add_(0, uid, rows)
    right = dict(got, tables=[user_grad(W[0])] + got['tables'][1:])
    assert max(check_clfm_result('rebuilt', right, refs[0], refs[1], share).values()) <= 1.0          # the rebuild itself is sound
    wrong = dict(got, tables=[user_grad(W[0].t().contiguous())] + got['tables'][1:])
    with pytest.raises(AssertionError, match='gradient source_user: error / bound'):
        check_clfm_result('W for W^T', wrong, refs[0], refs[1], share)

    counts = torch.bincount(uid, minlength=tabs[0].shape[0])
    dup_row = int(torch.nonzero(counts > 1)[0])
    keep = torch.ones(uid.numel())
    keep[int(torch.nonzero(uid == dup_row)[-1])] = 0.0
    dropped = dict(got, tables=[user_grad(W[0], keep)] + got['tables'][1:])
    with pytest.raises(AssertionError, match=f'gradient source_user: error / bound .* at table row {dup_row} '):
        check_clfm_result('one occurrence dropped', dropped, refs[0], refs[1], share)
