"""The id sort's own launch list (csrc/cdr_step.hip, "the id sort's own launch list"): from 2^18 pairs up the two-table id sort runs
rocPRIM's Onesweep device code from launches of its own, with no memset between them.  A stable sort's output is a function of the keys
alone, so ``keys_sorted`` / ``perm`` of ``cdr_sort_ids_two_tables`` are held, element for element, to ``torch.sort(stable=True)`` of the
same keys -- at the first n on the new path, at a whole number of blocks, at the last n on the library path, for 1 to 4 digit places (both
parities of the ping-pong), on a reused workspace and on one filled with 0xFF -- and the fused BPR step on the new list (key making,
histogram and scan in one launch) is held bit for bit to the same steps in a child process that keeps the library call (CDR_OWN_SORT=0)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# n = 3 B pairs: 262,146 = 32 full blocks of 8,192 + a block of 2 (the first n on the own list); 270,336 = 33 blocks exactly;
# 262,143 = the last n on the library path
BATCHES = [87382, 90112, 87381]
# (rows_a, rows_b) -> key bits (the wider table's bits + the table bit) -> 9-bit digit places
ROWS = {'1place': (256, 256), '2places': (300, 40), '3places': (50_000_001, 20_000_001), '4places': (2 ** 27 + 1, 40)}
PLACES = {'1place': (9, 1), '2places': (10, 2), '3places': (27, 3), '4places': (29, 4)}


def _ids(kind, B, rows_a, rows_b, seed):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    u, p, n = (torch.randint(0, hi, (B,), device=DEV, generator=g) for hi in (rows_a, rows_b, rows_b))
    if kind == 'equal':                                          # one bin of every digit holds the whole list: stability over all of it
        u.fill_(rows_a - 1); p.fill_(rows_b - 1); n.fill_(rows_b - 1)
    elif kind == 'hot':                                          # one item in 40 % of the positives and among the negatives
        p[: (2 * B) // 5] = 7
        n[B // 2: B // 2 + 50] = 7
    return u, p, n


def _key_base(rows_a, rows_b):
    return 1 << max((rows_a - 1).bit_length(), (rows_b - 1).bit_length())


def _workspace(n, rows_a, rows_b):
    from recbole_cdr_amd import binding as B_
    need = ctypes.c_size_t(0)
    B_._check(B_.load().cdr_sort_workspace_bytes(n, 2 * _key_base(rows_a, rows_b), ctypes.byref(need)), 'cdr_sort_workspace_bytes')
    return torch.empty(int(need.value), device=DEV, dtype=torch.uint8)


def _sort(u, p, n, rows_a, rows_b, ws):
    from recbole_cdr_amd import binding as B_
    B = u.numel()
    keys = torch.full((3 * B,), -1, device=DEV, dtype=torch.int32)
    perm = torch.full((3 * B,), -1, device=DEV, dtype=torch.int32)
    kb = ctypes.c_uint32(0)
    B_.call('cdr_sort_ids_two_tables', B_.ctx(DEV), B_.stream(), B_.i64(u), B, rows_a, B_.i64(p), B, B_.i64(n), B, rows_b, B_.raw(keys),
            B_.raw(perm), ctypes.byref(kb), B_.raw(ws), ws.numel())
    assert kb.value == _key_base(rows_a, rows_b)
    return keys, perm


def _check(u, p, n, rows_a, rows_b, keys, perm, what):
    B = u.numel()
    kb = _key_base(rows_a, rows_b)
    all_keys = torch.cat([u, kb + p, kb + n])
    occ = torch.cat([torch.arange(B, device=DEV), torch.arange(2 * B, device=DEV)])      # users: index in the list; items: index in [pid | nid]
    want_keys, order = torch.sort(all_keys, stable=True)
    assert torch.equal(keys.long() & 0xFFFFFFFF, want_keys), (what, 'keys')
    assert torch.equal(perm.long() & 0xFFFFFFFF, occ[order]), (what, 'perm')


def test_the_shapes_cover_what_they_claim():
    from recbole_cdr_amd import binding as B_
    assert [3 * b for b in BATCHES] == [2 ** 18 + 2, 33 * 8192, 2 ** 18 - 1]
    for name, (ra, rb) in ROWS.items():
        bits, places = PLACES[name]
        assert (2 * _key_base(ra, rb) - 1).bit_length() == bits and -(-bits // 9) == places, name
    # the own list needs its state, the look-back regions of every pass and the ping-pong arrays behind {keys_in | vals_in}
    n = 3 * BATCHES[0]
    need = _workspace(n, *ROWS['3places']).numel()
    assert need >= 4 * 4 * n + 3 * 512 * 33 * 4 + 3 * 512 * 8


@pytest.mark.parametrize('kind', ['uniform', 'equal', 'hot'])
@pytest.mark.parametrize('rows', list(ROWS))
@pytest.mark.parametrize('B', BATCHES)
def test_sorted_keys_and_perm_are_the_stable_sort(B, rows, kind):
    rows_a, rows_b = ROWS[rows]
    ws = _workspace(3 * B, rows_a, rows_b)
    u, p, n = _ids(kind, B, rows_a, rows_b, seed=1)
    keys, perm = _sort(u, p, n, rows_a, rows_b, ws)
    _check(u, p, n, rows_a, rows_b, keys, perm, (B, rows, kind))


@pytest.mark.parametrize('rows', list(ROWS))
@pytest.mark.parametrize('B', BATCHES)
def test_a_reused_and_a_garbage_workspace(B, rows):
    """The sort's state is cleared per call: nothing is left over from the call before, nothing relies on the allocator handing out zeros."""
    rows_a, rows_b = ROWS[rows]
    ws = _workspace(3 * B, rows_a, rows_b)
    ws.fill_(0xFF)
    for seed, kind in ((2, 'uniform'), (3, 'hot'), (4, 'uniform')):
        u, p, n = _ids(kind, B, rows_a, rows_b, seed)
        keys, perm = _sort(u, p, n, rows_a, rows_b, ws)
        _check(u, p, n, rows_a, rows_b, keys, perm, (B, rows, seed))


def test_a_workspace_sized_for_a_larger_batch():
    """Step objects size the workspace once for their largest batch: a smaller sort lays its state out for its own n inside it."""
    rows_a, rows_b = ROWS['3places']
    ws = _workspace(3 * 120000, rows_a, rows_b)
    ws.fill_(0xFF)
    for B in (120000, BATCHES[0], BATCHES[2], BATCHES[1]):
        u, p, n = _ids('uniform', B, rows_a, rows_b, seed=B)
        keys, perm = _sort(u, p, n, rows_a, rows_b, ws)
        _check(u, p, n, rows_a, rows_b, keys, perm, B)


# ---- the fused step: key making, histogram and scan in one launch, against the same steps on the library call in a process of their own
FUSED = dict(nu=50021, ni=100003, D=8, B=BATCHES[0], steps=3)


def _fused_run():
    from recbole_cdr_amd.fused import FusedBPRStep
    c = FUSED
    g = torch.Generator(device=DEV); g.manual_seed(5)
    U = torch.randn(c['nu'], c['D'], device=DEV, generator=g) * 0.1
    I = torch.randn(c['ni'], c['D'], device=DEV, generator=g) * 0.1
    st = FusedBPRStep(U, I, c['B'], opt='adam', lr=0.01, reg_weight=0.02, id_path='sort')
    st.ws.fill_(0xFF)
    outs = []
    for k in range(c['steps']):
        u, p, n = _ids('hot' if k == 1 else 'uniform', c['B'], c['nu'], c['ni'], seed=20 + k)
        st.step(u, p, n)
        outs.append(st.out6[:9].clone())
    torch.cuda.synchronize()
    res = {'U': st.U, 'I': st.I, 'mU': st.ustate.exp_avg, 'vU': st.ustate.exp_avg_sq, 'mI': st.istate.exp_avg, 'vI': st.istate.exp_avg_sq,
           'out': torch.stack(outs)}
    return {k: v.cpu() for k, v in res.items()}


def test_fused_step_is_bit_equal_to_the_library_sort_in_a_child_process(tmp_path):
    assert os.environ.get('CDR_OWN_SORT', '') not in ('0', '1'), 'this process must run the default list'
    got = _fused_run()
    out = tmp_path / 'library.pt'
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=dict(os.environ, CDR_OWN_SORT='0'), capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    want = torch.load(str(out))
    assert set(got) == set(want)
    for name in got:
        assert torch.equal(got[name], want[name]), name
    assert float(got['out'][0][4]) != 0.0 and float(got['out'][0][5]) != 0.0, 'the EmbLoss coefficients are in play'
    assert float(got['mU'].abs().max()) > 0.0 and float(got['mI'].abs().max()) > 0.0, 'the steps moved the moments'


if __name__ == '__main__':                                      # the child: the same steps, tensors to the file named
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert os.environ.get('CDR_OWN_SORT') == '0'
    torch.save(_fused_run(), sys.argv[1])
