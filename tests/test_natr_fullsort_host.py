"""NATR's one-launch full sort without a GPU: the rewritten algebra of csrc/cdr_natr_fullsort.hip equals the oracle's phase2_forward in
float64 on both golden fixtures, the fp64 yardstick of test_gpu_natr_fullsort.py accepts an fp32 CPU result and rejects three mutations of
it, the C entry points refuse bad arguments before any launch, the top-k workspace never grows with U x N, and the model's opt-in
attribute contract holds on a CPU-constructed model."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

from golden_util import Golden, cases
from helpers import FakeDataset, base_config
from natr_fullsort_fp64 import make_case, natr_fullsort_fp64, natr_pair_fp64, natr_summary_fp64, pair_fp32


@pytest.mark.parametrize('name', cases('natr_'))
def test_natr_fullsort_algebra_equals_the_oracle_in_float64(name):
    """Over ALL (user, item) pairs of a fixture: summary + three-dot-product form == oracle.natr.phase2_forward, both in float64, to 1e-12
    (the helper's pair stage is fed the float64 summary itself here, not its fp32 rounding)."""
    from oracle import natr as o_natr
    g = Golden(name)
    ids = g.idspace()
    P = {k: v.double() for k, v in g.group('param').items()}
    hist = o_natr.history_info(ids, g['aux/t_pairs'], int(g.meta('max_inter_length')))
    nu, N = ids.total_num_users, ids.target_num_items
    users = torch.arange(nu)
    want = o_natr.phase2_forward(P, ids, hist, users.repeat_interleave(N), torch.arange(N).repeat(nu)).view(nu, N)
    key_is_item = ids.mode == 'overlap_users'
    src = P['source_user_embedding.weight'] if key_is_item else P['source_item_embedding.weight']
    key_tab = P['target_item_embedding.weight'] if key_is_item else P['target_user_embedding.weight']
    other_tab = P['target_user_embedding.weight'] if key_is_item else P['target_item_embedding.weight']
    keys = torch.arange(N) if key_is_item else users
    su = natr_summary_fp64(src, hist[0], hist[2], key_tab, keys, P['transfer_layer.weight'], P['transfer_layer.bias'],
                           P['unit_attention_layer.weight'], P['unit_attention_layer.bias'])
    got = natr_pair_fp64(key_is_item, su.v, key_tab, other_tab, users, N, P['domain_attention_layer.weight'])
    assert got.v.dtype == torch.float64 and tuple(got.v.shape) == (nu, N)
    err = float((got.v - want).abs().max())
    print(f'{name} ({ids.mode}): {nu} x {N} pairs, largest |rewritten - oracle| in float64 {err:.3e}')
    assert err <= 1e-12


@pytest.mark.parametrize('key_is_item', [False, True])
def test_natr_fp64_yardstick_accepts_fp32_and_rejects_mutations(key_is_item):
    """An fp32 CPU evaluation of the kernel's formula lies within the any-order bounds everywhere; dropping the |q| term, swapping beta and
    1 - beta, and keeping b_d in one logit only each leave them (Dt = 16, Ds = 8, L = 5, 9 users x 50 items)."""
    c = make_case(16, 8, 5, 9, 50, key_is_item)
    su = natr_summary_fp64(c['src'], c['hist'], c['mask_mat'], c['key_tab'], c['keys'], c['Wt'], c['bt'], c['wu'], c['bu']).v.float()
    ref = natr_fullsort_fp64(c, su=su)
    args = (key_is_item, su, c['key_tab'], c['other_tab'], c['uid'], c['N'], c['wd'])
    good = pair_fp32(*args)
    assert tuple(good.shape) == (9, 50)
    worst = float(ref.ratio(good).max())
    print(f'fp32 CPU result, key_is_item={key_is_item}: worst error / bound {worst:.3f}')
    assert worst <= 1.0
    for nm, kw in (('dropped |q| term', dict(drop_absq=True)), ('swapped beta', dict(swap=True)),
                   ('b_d in one logit only', dict(one_sided_bd=True, bd=c['bd']))):
        r = float(ref.ratio(pair_fp32(*args, **kw)).max())
        print(f'  {nm}: worst error / bound {r:.3g}')
        assert r > 1.0, nm


def test_natr_summary_yardstick_accepts_fp32():
    """The summary stage in fp32 torch (the oracle's operation sequence on the case's tensors) lies within the summary bounds, for the
    planted keys too: length 0 (all padding), length 1, longer than L."""
    c = make_case(16, 8, 5, 9, 50, False)
    lens = c['lens'][c['keys']]
    assert int(lens[0]) == 0 and int(lens[1]) == 1 and int(lens[2]) > 5
    ref = natr_summary_fp64(c['src'], c['hist'], c['mask_mat'], c['key_tab'], c['keys'], c['Wt'], c['bt'], c['wu'], c['bu'])
    keys = c['keys']
    he = c['src'][c['hist'][keys]] @ c['Wt'].t() + c['bt']
    x = (torch.relu(c['key_tab'][keys].unsqueeze(1) * he) @ c['wu'].t()).squeeze(2) + c['bu']
    att = torch.softmax(x + torch.where(c['mask_mat'][keys].bool(), 0., -10000.0), 1)
    su = torch.bmm(att.unsqueeze(1), he).squeeze(1)
    worst = float(ref.ratio(su).max())
    print(f'fp32 CPU summary: worst error / bound {worst:.3f}')
    assert worst <= 1.0


def _host_call(lib, buf, U, N, Dt, k, nbytes, topk=True):
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)                          # 16-byte aligned, as the entries require of tables
    head = (None, 0, ptr, Dt, ptr, Dt, ptr, Dt, ptr, U, N, Dt, ptr)
    if topk:
        return lib.cdr_natr_fullsort_topk(*head, k, None, None, 1, ptr, ptr, ptr, nbytes)
    return lib.cdr_natr_fullsort(*head, ptr, N)


def test_natr_fullsort_entries_refuse_bad_arguments_without_a_device():
    """k = 0 / 65, Dt = 6 / 132, U or N < 1, N >= 2^31 and a workspace one byte short return CDR_EINVAL with an error text before anything
    is launched -- so also on a machine without a GPU (host dummy pointers stand in for every array: a refused call reads none)."""
    from recbole_cdr_amd import binding
    lib = binding.load()
    assert [lib.cdr_natr_fullsort_supported(D) for D in (4, 8, 12, 64, 128, 6, 132, 0, 2)] == [1, 1, 1, 1, 1, 0, 0, 0, 0]
    need = ctypes.c_size_t(0)
    for k in (0, 65, -1):
        assert lib.cdr_natr_fullsort_topk_workspace_bytes(64, 1000, k, ctypes.byref(need)) != 0
        assert lib.cdr_last_error()
    assert lib.cdr_natr_fullsort_topk_workspace_bytes(0, 1000, 10, ctypes.byref(need)) != 0
    assert lib.cdr_natr_fullsort_topk_workspace_bytes(64, 0, 10, ctypes.byref(need)) != 0
    assert lib.cdr_natr_fullsort_topk_workspace_bytes(64, 1 << 31, 10, ctypes.byref(need)) != 0
    U, N, k = 5, 77, 10
    assert lib.cdr_natr_fullsort_topk_workspace_bytes(U, N, k, ctypes.byref(need)) == 0 and need.value > 0
    buf = (ctypes.c_float * 4096)()
    for k_bad in (0, 65):
        assert _host_call(lib, buf, U, N, 16, k_bad, need.value) != 0
        assert b'k = ' in lib.cdr_last_error()
    for D_bad in (6, 132):
        assert _host_call(lib, buf, U, N, D_bad, k, need.value) != 0 and b'outside the kernel' in lib.cdr_last_error()
        assert _host_call(lib, buf, U, N, D_bad, k, 0, topk=False) != 0 and b'outside the kernel' in lib.cdr_last_error()
    for U_bad, N_bad in ((0, N), (U, 0), (U, 1 << 31)):
        assert _host_call(lib, buf, U_bad, N_bad, 16, k, need.value) != 0 and lib.cdr_last_error()
        assert _host_call(lib, buf, U_bad, N_bad, 16, k, 0, topk=False) != 0 and lib.cdr_last_error()
    assert _host_call(lib, buf, U, N, 16, k, need.value - 1) != 0 and b'workspace' in lib.cdr_last_error()


@pytest.mark.parametrize('U,N,k', [(1024, 10_000_000, 10), (1024, 1_000_000, 64), (64, 1_000_000, 10), (1, 1, 1)])
def test_natr_fullsort_topk_workspace_is_bounded(U, N, k):
    """Partial lists of at most 2,048 item stripes and their first merge level: at most 160 MB, never U x N."""
    from recbole_cdr_amd import binding
    need = ctypes.c_size_t(0)
    assert binding.load().cdr_natr_fullsort_topk_workspace_bytes(U, N, k, ctypes.byref(need)) == 0
    stripes = 2048
    assert 0 < need.value <= 2 * (stripes + stripes // 64 + 1) * U * k * 4 + 4 * 256
    assert need.value <= 160 << 20


def _cpu_model(mode, **extra):
    from oracle.common import IdSpace
    from recbole_cdr_amd.model.cross_domain_recommender.natr import NATR
    ids = IdSpace(OU=40, TOU=30, SOU=35, OI=1, TOI=500, SOI=70) if mode == 'overlap_users' else \
        IdSpace(OU=1, TOU=70, SOU=22, OI=18, TOI=483, SOI=16)
    rng = np.random.RandomState(0)
    tu, ti = np.arange(1, ids.target_num_users), np.arange(1, ids.target_num_items)
    t_pairs = np.unique(np.stack([rng.choice(tu, 300), rng.choice(ti, 300)], 1), axis=0)
    s_pairs = np.stack([np.full(4, ids.total_num_users - 1), np.full(4, ids.total_num_items - 1)], 1)
    ds = FakeDataset(ids, s_pairs, t_pairs)
    model = NATR(base_config('cpu', source_embedding_size=16, target_embedding_size=24, reg_weight=1e-3, max_inter_length=6, **extra), ds)
    assert model.mode == mode
    return model


@pytest.mark.parametrize('mode', ['overlap_users', 'overlap_items'])
def test_natr_native_full_sort_is_opt_in(mode):
    """Flag absent or false: the reference's contract (no ``full_sort_topk`` attribute, ``full_sort_predict`` raises NotImplementedError),
    and freeze_for_eval / unfreeze_eval leave no cache state.  Flag on: both are callable attributes in every phase but 'SOURCE', where the
    contract of the flag-off model holds; pickle and deepcopy keep the choice and drop the evaluation caches."""
    from recbole_cdr_amd.model.cross_domain_recommender.natr import NATR
    for extra in ({}, {'native_full_sort': False}):
        off = _cpu_model(mode, **extra)
        for phase in (None, 'SOURCE', 'TARGET', 'BOTH'):
            off.phase = phase
            assert not hasattr(off, 'full_sort_topk')
            with pytest.raises(NotImplementedError):
                off.full_sort_predict(None)
        off.eval()
        off.freeze_for_eval()
        assert '_eval_frozen' not in off.__dict__ and '_eval_su' not in off.__dict__
        off.unfreeze_eval()
        for clone in (pickle.loads(pickle.dumps(off)), copy.deepcopy(off)):
            assert not hasattr(clone, 'full_sort_topk')
    on = _cpu_model(mode, native_full_sort=True)
    for phase in (None, 'TARGET', 'BOTH'):
        on.phase = phase
        assert hasattr(on, 'full_sort_topk') and callable(on.full_sort_topk) and callable(on.full_sort_predict)
        assert on.full_sort_predict.__func__ is NATR._native_full_sort_predict
    on.phase = 'SOURCE'
    assert not hasattr(on, 'full_sort_topk')
    with pytest.raises(NotImplementedError):
        on.full_sort_predict(None)
    on.phase = 'TARGET'
    on.eval()
    on.freeze_for_eval()
    on.__dict__['_eval_su'] = torch.zeros(3)                                         # stands in for the cached item summary
    assert on.__dict__.get('_eval_frozen') is True
    for clone in (pickle.loads(pickle.dumps(on)), copy.deepcopy(on)):
        assert hasattr(clone, 'full_sort_topk') and clone.full_sort_predict.__func__ is NATR._native_full_sort_predict
        assert '_eval_su' not in clone.__dict__ and '_eval_frozen' not in clone.__dict__
        assert set(clone.state_dict()) == set(on.state_dict())
    on.unfreeze_eval()
    assert '_eval_su' not in on.__dict__ and '_eval_frozen' not in on.__dict__
    on.freeze_for_eval()
    on.train()
    assert '_eval_frozen' not in on.__dict__
