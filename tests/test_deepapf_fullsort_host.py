"""DeepAPF's one-launch full sort without a GPU: the C entry points refuse bad arguments before any launch, the top-k workspace never
grows with U x N, the model's opt-in attribute contract holds on a CPU-constructed model, and the fp64 yardstick of
test_gpu_deepapf_fullsort.py (deepapf_fullsort_fp64) accepts an fp32 CPU result and rejects three mutations of it."""
import copy
import ctypes
import pickle

import pytest

from deepapf_fullsort_fp64 import deepapf_fullsort_fp64, fullsort_fp32, make_case
from helpers import FakeDataset, base_config


def _host_call(lib, buf, U, N, D, k, nbytes, topk=True):
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)                          # 16-byte aligned, as the entries require of tables
    head = (None, 0, ptr, D, ptr, D, ptr, D, ptr, U, N, D, 3, ptr, ptr, ptr, ptr)
    if topk:
        return lib.cdr_deepapf_fullsort_topk(*head, k, None, None, 1, ptr, ptr, ptr, nbytes)
    return lib.cdr_deepapf_fullsort(*head, ptr, N)


def test_deepapf_fullsort_entries_refuse_bad_arguments_without_a_device():
    """k = 0 / 65, D = 6 / 132, U or N < 1, N >= 2^31 and a workspace one byte short return CDR_EINVAL with an error text before anything
    is launched -- so also on a machine without a GPU (host dummy pointers stand in for every array: a refused call reads none)."""
    from recbole_cdr_amd import binding
    lib = binding.load()
    assert [lib.cdr_deepapf_fullsort_supported(D) for D in (4, 8, 12, 64, 128, 6, 132, 0, 2)] == [1, 1, 1, 1, 1, 0, 0, 0, 0]
    need = ctypes.c_size_t(0)
    for k in (0, 65, -1):
        assert lib.cdr_deepapf_fullsort_topk_workspace_bytes(64, 1000, k, ctypes.byref(need)) != 0
        assert lib.cdr_last_error()
    assert lib.cdr_deepapf_fullsort_topk_workspace_bytes(0, 1000, 10, ctypes.byref(need)) != 0
    assert lib.cdr_deepapf_fullsort_topk_workspace_bytes(64, 0, 10, ctypes.byref(need)) != 0
    assert lib.cdr_deepapf_fullsort_topk_workspace_bytes(64, 1 << 31, 10, ctypes.byref(need)) != 0
    U, N, k = 5, 77, 10
    assert lib.cdr_deepapf_fullsort_topk_workspace_bytes(U, N, k, ctypes.byref(need)) == 0 and need.value > 0
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
def test_deepapf_fullsort_topk_workspace_is_bounded(U, N, k):
    """Partial lists of at most 2,048 item stripes and their first merge level: at most 160 MB, never U x N."""
    from recbole_cdr_amd import binding
    need = ctypes.c_size_t(0)
    assert binding.load().cdr_deepapf_fullsort_topk_workspace_bytes(U, N, k, ctypes.byref(need)) == 0
    stripes = 2048
    assert 0 < need.value <= 2 * (stripes + stripes // 64 + 1) * U * k * 4 + 4 * 256
    assert need.value <= 160 << 20


@pytest.mark.parametrize('mode', ['overlap_users', 'overlap_items'])
def test_deepapf_native_full_sort_is_opt_in(mode):
    """Flag absent or false: the reference's contract (no ``full_sort_topk`` attribute, ``full_sort_predict`` raises NotImplementedError).
    Flag on: both are callable attributes; pickle and deepcopy keep the choice."""
    from oracle.common import IdSpace
    from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
    ids = IdSpace(OU=40, TOU=30, SOU=35, OI=1, TOI=500, SOI=70) if mode == 'overlap_users' else \
        IdSpace(OU=1, TOU=70, SOU=22, OI=18, TOI=483, SOI=16)
    for extra in ({}, {'native_full_sort': False}):
        off = DeepAPF(base_config('cpu', embedding_size=16, beta=0.5, **extra), FakeDataset(ids))
        assert off.mode == mode
        assert not hasattr(off, 'full_sort_topk')
        with pytest.raises(NotImplementedError):
            off.full_sort_predict(None)
        for clone in (pickle.loads(pickle.dumps(off)), copy.deepcopy(off)):
            assert not hasattr(clone, 'full_sort_topk')
    on = DeepAPF(base_config('cpu', embedding_size=16, beta=0.5, native_full_sort=True), FakeDataset(ids))
    assert hasattr(on, 'full_sort_topk') and callable(on.full_sort_topk) and callable(on.full_sort_predict)
    assert on.full_sort_predict.__func__ is DeepAPF._native_full_sort_predict
    for clone in (pickle.loads(pickle.dumps(on)), copy.deepcopy(on)):
        assert hasattr(clone, 'full_sort_topk') and clone.full_sort_predict.__func__ is DeepAPF._native_full_sort_predict
        assert set(clone.state_dict()) == set(on.state_dict())


@pytest.mark.parametrize('key_is_item', [False, True])
def test_fullsort_fp64_yardstick_accepts_fp32_and_rejects_mutations(key_is_item):
    """An fp32 CPU evaluation of the kernel's operation sequence lies within the any-order bounds everywhere; a non-strict mask, a dropped
    b1 and swapped softmax weights each leave them (D = 16, 9 users x 50 items, key ids n_overlap and n_overlap + 1 among them)."""
    case = make_case(16, 9, 50, 20, key_is_item)
    ref, _amb = deepapf_fullsort_fp64(**case)
    good = fullsort_fp32(**case)
    assert tuple(good.shape) == (9, 50)
    worst = float(ref.ratio(good).max())
    print(f'fp32 CPU result, key_is_item={key_is_item}: worst error / bound {worst:.3f}')
    assert worst <= 1.0
    for name, kw in (('non-strict mask', dict(strict=False)), ('dropped b1', dict(drop_b1=True)), ('swapped weights', dict(swap=True))):
        bad = fullsort_fp32(**case, **kw)
        r = float(ref.ratio(bad).max())
        print(f'  {name}: worst error / bound {r:.3g}')
        assert r > 1.0, name
