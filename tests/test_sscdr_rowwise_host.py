"""Host-side checks of SSCDR's O(batch) row-wise training path (no GPU): the trainer accepts the model with
``optimizer_mode='rowwise'``, the model carries the members the trainer calls, and the boundary lists the new entry."""
import os
import re

import numpy as np
import torch

from helpers import FakeDataset, base_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(**kw):
    from oracle.common import IdSpace
    from recbole_cdr_amd.model.cross_domain_recommender.sscdr import SSCDR
    ids = IdSpace(OU=12, TOU=9, SOU=8, OI=1, TOI=14, SOI=16)
    rng = np.random.RandomState(0)
    pairs = np.stack([rng.randint(1, ids.OU, 40), rng.randint(ids.OI + ids.TOI, ids.total_num_items, 40)], 1).astype(np.int64)
    ds = FakeDataset(ids, s_pairs=pairs, t_pairs=np.zeros((1, 2), dtype=np.int64))
    cfg = base_config('cpu', embedding_size=16, margin=0.3, mlp_hidden_size=[24], train_modes=['SOURCE', 'TARGET', 'OVERLAP'],
                      epoch_num=['1', '1', '1'], source_split=False, **{'lambda': 0.5}, **kw)
    torch.manual_seed(0)
    return cfg, SSCDR(cfg, ds)


def test_trainer_accepts_sscdr_in_rowwise_mode():
    from recbole_cdr_amd.trainer import CrossDomainTrainer
    cfg, model = _model(optimizer_mode='rowwise')
    trainer = CrossDomainTrainer(cfg, model)
    assert trainer.optimizer_mode == 'rowwise' and trainer.rowwise_adam == 'lazy'
    cfg, model = _model(optimizer_mode='rowwise', rowwise_adam='exact')
    assert CrossDomainTrainer(cfg, model).rowwise_adam == 'exact'


def test_sscdr_has_the_members_the_rowwise_trainer_calls():
    from recbole_cdr_amd.model.cross_domain_recommender.sscdr import SSCDR
    from recbole_cdr_amd.model.rowwise import RowwiseTraining
    assert issubclass(SSCDR, RowwiseTraining)
    for name in ('fused_train_step', 'fused_sync', 'fused_graph_key', 'fused_replayed', 'fused_optimizer_state',
                 'load_fused_optimizer_state', '_fused_phase_step'):
        assert callable(getattr(SSCDR, name)), name
    _, model = _model()
    for phase in ('SOURCE', 'TARGET', 'BOTH', 'OVERLAP'):
        model.set_phase(phase)
        assert model.fused_graph_key({}) is None and model.fused_graph_key({}, adam='exact') is None
    model.fused_sync()                                       # nothing trained yet: a no-op that leaves no state behind
    assert '_fused' not in model.__dict__ and model.fused_optimizer_state() == {}


def test_binding_lists_the_triplet_entry_and_the_abi_version_of_the_header():
    from recbole_cdr_amd import binding
    assert 'cdr_triplet_fwd_grad' in binding.exported_symbols()
    assert len(binding._SIGNATURES['cdr_triplet_fwd_grad']) == 14
    text = open(os.path.join(ROOT, 'include', 'cdr_hip.h')).read()
    assert int(re.search(r'#define CDR_ABI_VERSION (\d+)', text).group(1)) == binding.ABI_VERSION
    assert binding.load().cdr_abi_version() == binding.ABI_VERSION
    decl = re.search(r'int cdr_triplet_fwd_grad\((.*?)\);', re.sub(r'/\*.*?\*/', '', text, flags=re.S), flags=re.S).group(1)
    assert len(decl.split(',')) == 14


def test_triplet_entry_refuses_bad_widths_before_any_launch():
    """D % 4 != 0, D > 256 and B = 0 come back as the argument error on a machine without a GPU too: nothing was launched."""
    import ctypes
    from recbole_cdr_amd import binding
    lib = binding.load()
    buf = (ctypes.c_float * 1024)()
    ids = (ctypes.c_int64 * 4)(0, 1, 2, 3)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    ctx = p(buf)                                             # (never dereferenced: the checks come first)
    for D, B in ((6, 4), (260, 4), (0, 4), (8, 0)):
        rc = lib.cdr_triplet_fwd_grad(ctx, None, p(buf), p(buf), D, p(ids), p(ids), p(ids), B, 0.2, 1e-6, p(buf), p(buf), p(buf))
        assert rc != 0, (D, B)
        assert b'cdr_triplet_fwd_grad' in lib.cdr_last_error(), (D, B)
