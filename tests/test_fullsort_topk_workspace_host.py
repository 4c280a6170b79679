"""The three one-launch fused top-k entries (MLP tower, DeepAPF, NATR) size their workspace from one stripe plan (csrc/cdr_topk.h).  The
sizes are pinned to tests/golden/fullsort_topk_workspace_bytes.json: what the three separate plan families returned before they were
merged, recorded from that library over users x items x k, around every edge of the plan (one user group / two, the tile and workgroup
tails, the seeding threshold at 8 x 1024 x max(k, 8) items, k below and at the sample's floor of 8, the largest catalogue).  Only the
query entries are called: nothing here can launch, no GPU is needed."""
import ctypes
import json
import os

import pytest

from recbole_cdr_amd import binding

ENTRIES = ('conet', 'deepapf', 'natr')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fullsort_topk_workspace_bytes.json')


def _query(name):
    return getattr(binding.load(), f'cdr_{name}_fullsort_topk_workspace_bytes')


@pytest.mark.parametrize('name', ENTRIES)
def test_fullsort_topk_workspace_bytes_match_the_recorded_table(name):
    tab = json.load(open(GOLDEN))
    Us, Ns, ks, want = tab['U'], tab['N'], tab['k'], tab['bytes'][name]
    assert (len(Us), len(Ns), len(ks)) == (13, 9, 5) and len(want) == 13 * 9 * 5
    fn, need, bad = _query(name), ctypes.c_size_t(0), []
    for iu, U in enumerate(Us):
        for i_n, N in enumerate(Ns):
            for ik, k in enumerate(ks):
                assert fn(U, N, k, ctypes.byref(need)) == 0, (U, N, k, binding.load().cdr_last_error())
                if need.value != want[(iu * len(Ns) + i_n) * len(ks) + ik]:
                    bad.append((U, N, k, need.value, want[(iu * len(Ns) + i_n) * len(ks) + ik]))
    assert not bad, f'{len(bad)} of {len(want)} sizes differ; first (U, N, k, got, recorded): {bad[:5]}'


@pytest.mark.parametrize('name', ENTRIES)
def test_fullsort_topk_workspace_query_refusals(name):
    fn, lib, need = _query(name), binding.load(), ctypes.c_size_t(12345)
    for U, N, k in ((64, 1000, 0), (64, 1000, 65), (64, 1 << 31, 10), (0, 1000, 10)):
        assert fn(U, N, k, ctypes.byref(need)) != 0, (U, N, k)
        assert f'cdr_{name}_fullsort_topk_workspace_bytes'.encode() in lib.cdr_last_error()
        assert need.value == 12345                                     # a refused query writes nothing
    assert fn(64, 1000, 10, None) != 0 and lib.cdr_last_error()
    assert fn(64, 1000, 10, ctypes.byref(need)) == 0 and need.value not in (0, 12345)
