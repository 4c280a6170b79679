"""The wide mask + top-k entries (cdr_fullsort_topk_wide_f32, cdr_fullsort_neg_sqdist_topk_wide_f32, cdr_topk_rows_f32 and their
workspace queries) where no GPU is needed: they are declared, exported and bound; the workspace never exceeds the staging of one column
pass plus the partial lists; bad arguments are refused before anything is launched; the trainer accepts ``eval_route='topk'`` above 64."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_ENTRIES = ('cdr_fullsort_topk_wide_workspace_bytes', 'cdr_fullsort_topk_wide_f32', 'cdr_fullsort_neg_sqdist_topk_wide_workspace_bytes',
                'cdr_fullsort_neg_sqdist_topk_wide_f32', 'cdr_topk_rows_workspace_bytes', 'cdr_topk_rows_f32')
STAGING_MAX = (256 << 20) + 256


def _partial_lists_max(U, k):
    """8 k bytes per user and column stripe, at most max(1, ceil(1024 / U)) stripes per user (include/cdr_hip.h), rounded up to 256"""
    return 8 * k * U * max(1, -(-1024 // U)) + 256


def test_wide_entries_are_declared_and_the_abi_version_stands():
    from recbole_cdr_amd import binding
    from recbole_cdr_amd import functional as F_
    header = open(os.path.join(ROOT, 'include', 'cdr_hip.h')).read()
    for name in WIDE_ENTRIES:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in binding._SIGNATURES and name in binding.exported_symbols()
    assert int(re.search(r'#define\s+CDR_ABI_VERSION\s+(\d+)', header).group(1)) == binding.ABI_VERSION == 64
    assert F_.WIDE_TOPK_MAX == 1024 and F_.FUSED_TOPK_MAX == 64
    for fn in ('topk_rows', 'fullsort_topk_wide', 'fullsort_neg_sqdist_topk_wide'):
        assert callable(getattr(F_, fn))


def test_wide_workspace_is_one_pass_of_staging_plus_the_partial_lists():
    from recbole_cdr_amd import binding
    lib, need = binding.load(), ctypes.c_size_t(0)
    for U, D, n0, n1, k in ((1024, 128, 10_000_000, 0, 1000), (64, 64, 5_000_000, 5_000_000, 1024), (1, 64, 10_000_000, 0, 100),
                            (5, 64, 77, 0, 1), (1024, 128, 0, 81_920, 100)):
        assert lib.cdr_fullsort_topk_wide_workspace_bytes(U, D, n0, n1, k, ctypes.byref(need)) == 0, lib.cdr_last_error()
        dot = need.value
        assert 0 < dot <= STAGING_MAX + _partial_lists_max(U, k), (U, n0, n1, k, dot)
        assert dot <= 4 * U * max(n0, n1) + 256 + _partial_lists_max(U, k)              # never more than the scores of one slab
        assert lib.cdr_fullsort_neg_sqdist_topk_wide_workspace_bytes(U, D, n0, n1, k, ctypes.byref(need)) == 0
        assert need.value == dot + ((4 * (U + n0 + n1) + 255) & ~255)
        assert lib.cdr_topk_rows_workspace_bytes(U, max(n0, n1), k, ctypes.byref(need)) == 0
        assert 0 < need.value <= _partial_lists_max(U, k)
    # the fused entries keep their limit
    assert lib.cdr_fullsort_topk_workspace_bytes(64, 64, 1000, 0, 65, ctypes.byref(need)) != 0


def test_wide_entries_refuse_bad_arguments_without_a_device():
    """k = 0 / 1025, NULL outputs, a short workspace, 2^31 columns, 2^30 users and a lone history pointer return CDR_EINVAL with an error text
    before anything is launched (host dummy pointers stand in for every array: a refused call reads none)."""
    from recbole_cdr_amd import binding
    lib = binding.load()
    EINVAL = -1                                                                         # CDR_EINVAL (include/cdr_hip.h)
    need = ctypes.c_size_t(12345)
    for q in (lib.cdr_fullsort_topk_wide_workspace_bytes, lib.cdr_fullsort_neg_sqdist_topk_wide_workspace_bytes):
        for U, n0, n1, k in ((64, 1000, 0, 0), (64, 1000, 0, 1025), (64, 1000, 0, -1), (0, 1000, 0, 100), (1 << 30, 1000, 0, 100),
                             (64, 1 << 30, 1 << 30, 100), (64, 0, 0, 100), (64, -1, 5, 100)):
            assert q(U, 64, n0, n1, k, ctypes.byref(need)) != 0, (U, n0, n1, k)
            assert lib.cdr_last_error() and need.value == 12345                         # a refused query writes nothing
        assert q(64, 64, 1000, 0, 100, None) != 0
    for U, N, k in ((64, 1000, 0), (64, 1000, 1025), (0, 1000, 100), (64, 0, 100), (64, 1 << 31, 100), (1 << 30, 10, 100)):
        assert lib.cdr_topk_rows_workspace_bytes(U, N, k, ctypes.byref(need)) != 0 and need.value == 12345
    U, D, N, k = 5, 16, 77, 100
    assert lib.cdr_fullsort_topk_wide_workspace_bytes(U, D, N, 0, k, ctypes.byref(need)) == 0
    ws_dot = need.value
    assert lib.cdr_fullsort_neg_sqdist_topk_wide_workspace_bytes(U, D, N, 0, k, ctypes.byref(need)) == 0
    ws_dist = need.value
    assert lib.cdr_topk_rows_workspace_bytes(U, N, k, ctypes.byref(need)) == 0
    ws_rows = need.value
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dot(k=k, n0=N, vals=p, idx=p, ws=p, nbytes=ws_dot, hi=None, hc=None, U=U):
        return lib.cdr_fullsort_topk_wide_f32(None, p, U, D, p, n0, None, 0, k, hi, hc, 1, vals, idx, ws, nbytes)

    def dist(k=k, n0=N, vals=p, idx=p, ws=p, nbytes=ws_dist, hi=None, hc=None, U=U):
        return lib.cdr_fullsort_neg_sqdist_topk_wide_f32(None, p, U, D, p, n0, None, 0, None, k, hi, hc, 1, vals, idx, ws, nbytes)

    def rows(k=k, n0=N, vals=p, idx=p, ws=p, nbytes=ws_rows, hi=None, hc=None, U=U, ld=None, col_off=0):
        return lib.cdr_topk_rows_f32(None, p, n0 if ld is None else ld, U, n0, col_off, k, hi, hc, 1, vals, idx, 0, ws, nbytes)

    for call, short in ((dot, ws_dot - 1), (dist, ws_dist - 1), (rows, ws_rows - 1)):
        for bad in (dict(k=0), dict(k=1025), dict(vals=None), dict(idx=None), dict(ws=None), dict(n0=1 << 31), dict(U=1 << 30), dict(U=0),
                    dict(hi=p), dict(hc=p)):
            assert call(**bad) == EINVAL, (call.__name__, bad)
            assert lib.cdr_last_error(), (call.__name__, bad)
        assert call(nbytes=short) == EINVAL and b'workspace' in lib.cdr_last_error()
    assert rows(ld=N - 1) == EINVAL and rows(col_off=-1) == EINVAL and rows(n0=1000, ld=1000, col_off=(1 << 31) - 1000) == EINVAL


def test_trainer_accepts_the_topk_route_above_64():
    import pytest
    from recbole_cdr_amd.trainer.trainer import FUSED_TOPK_MAX, WIDE_TOPK_MAX, Trainer
    model = torch.nn.Linear(2, 2)
    tr = Trainer({'device': 'cpu', 'eval_route': 'topk', 'topk': [100]}, model)
    assert tr.eval_route == 'topk' and (FUSED_TOPK_MAX, WIDE_TOPK_MAX) == (64, 1024)
    for fused in (False, True):
        for kmax in (10, 64, 65, 100, 1024):
            assert tr._takes_rank_route(fused, kmax) is False
    assert tr._takes_rank_route(False, 5000) is False                                   # (the unfused route lists any k)
    with pytest.raises(ValueError, match='1024'):
        tr._takes_rank_route(True, 1025)
    auto = Trainer({'device': 'cpu', 'topk': [100]}, model)                             # 'auto' routes exactly as before
    assert [auto._takes_rank_route(f, k) for f in (False, True) for k in (10, 64, 65, 1024, 5000)] == \
        [False, False, False, False, False, False, False, True, True, True]
    rank = Trainer({'device': 'cpu', 'topk': [100], 'eval_route': 'rank'}, model)
    assert all(rank._takes_rank_route(f, k) for f in (False, True) for k in (10, 100, 5000))
    gauc = Trainer({'device': 'cpu', 'topk': [10], 'metrics': ['GAUC']}, model)
    assert gauc._takes_rank_route(False, 10) and gauc._takes_rank_route(True, 10)
