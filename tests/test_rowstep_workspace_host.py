"""The four row-wise forward entries with dense weights (CLFM, DTCDR, DeepAPF, DCDCSR's map step) size their workspace as one packed
parameter vector per workgroup, and the workgroup count comes from one grid rule (csrc/cdr_rowstep.h).  The sizes are pinned to
tests/golden/rowstep_workspace_bytes.json: what the four separate copies of that rule returned before they were merged, recorded from
that library over batch x shape -- one row, one tile and one row more, one tile below, at and one row above every grid cap a shape can
have (256 CUs x 1..4 workgroups), 2^20 rows; widths 4 .. 128 with Du != Di for CLFM; DTCDR towers of one to three layers; DCDCSR
maps of one to three layers on both sides of the weights-in-LDS switch ([128, 64, 128] stages them, [128, 128, 128] does not).
Only the query entries are called: nothing here can launch, no GPU is needed."""
import ctypes
import json
import os

import pytest

from recbole_cdr_amd import binding

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rowstep_workspace_bytes.json')
BATCHES = [1, 32, 33] + [b for cap in (256, 512, 768, 1024) for b in ((cap - 1) * 32, cap * 32, cap * 32 + 1)] + [1 << 20]
WIDTHS = [4, 24, 32, 64, 100, 128]
SHAPES = {
    'clfm': [[du, di] for du in WIDTHS for di in WIDTHS],
    'dtcdr': [[d] + h for d in WIDTHS for h in ([1], [32], [64], [32, 16], [64, 64], [24, 40, 8], [64, 64, 64])],
    'deepapf': [[d] for d in WIDTHS],
    'dcdcsr': [[d, d] for d in WIDTHS] + [[24, 40, 24], [64, 128, 64], [100, 128, 100], [128, 64, 128], [128, 128, 128], [4, 4, 4, 4],
                                         [64, 128, 128, 64], [128, 32, 64, 128], [128, 128, 128, 128]],
}


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def query(name, B, shape, need):
    """The entry's status for one (batch, shape); ``need`` (a c_size_t) receives the size."""
    lib = binding.load()
    if name == 'clfm':
        return lib.cdr_clfm_fwd_grad_workspace_bytes(B, shape[0], shape[1], ctypes.byref(need))
    if name == 'dtcdr':
        return lib.cdr_dtcdr_fwd_grad_workspace_bytes(B, shape[0], len(shape) - 1, _ints(shape[1:]), ctypes.byref(need))
    if name == 'deepapf':
        return lib.cdr_deepapf_fwd_grad_workspace_bytes(B, shape[0], ctypes.byref(need))
    return lib.cdr_dcdcsr_map_fwd_grad_workspace_bytes(B, len(shape) - 1, _ints(shape), ctypes.byref(need))


def table(name):
    """[shape][batch] sizes from the loaded library (what the golden file was recorded with)."""
    need, rows = ctypes.c_size_t(0), []
    for shape in SHAPES[name]:
        rows.append([])
        for B in BATCHES:
            assert query(name, B, shape, need) == 0, (name, B, shape, binding.load().cdr_last_error())
            rows[-1].append(need.value)
    return rows


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_rowstep_workspace_bytes_match_the_recorded_table(name):
    tab = json.load(open(GOLDEN))
    assert tab['batches'] == BATCHES and tab['shapes'][name] == SHAPES[name]
    want, got = tab['bytes'][name], table(name)
    assert len(want) == len(SHAPES[name]) and all(len(r) == len(BATCHES) == 16 for r in want)
    bad = [(s, B, g, w) for s, gr, wr in zip(SHAPES[name], got, want) for B, g, w in zip(BATCHES, gr, wr) if g != w]
    assert not bad, f'{len(bad)} sizes differ; first (shape, batch, got, recorded): {bad[:5]}'
    assert len({tuple(r) for r in want}) > 1 and all(r[0] < r[-1] for r in want)     # (the table is not degenerate)


REFUSED = {
    'clfm': [(0, [64, 64]), (64, [6, 64]), (64, [64, 132]), (64, [0, 64])],
    'dtcdr': [(0, [64, 32]), (64, [6, 32]), (64, [132, 32]), (64, [64, 0]), (64, [64, 65]), (64, [64, 8, 8, 8, 8])],
    'deepapf': [(0, [64]), (64, [6]), (64, [132]), (64, [0])],
    'dcdcsr': [(0, [64, 64]), (64, [64, 32]), (64, [6, 6]), (64, [132, 132]), (64, [64, 64, 64, 64, 64])],
}


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_rowstep_workspace_query_refusals(name):
    lib, need = binding.load(), ctypes.c_size_t(12345)
    entry = {'dcdcsr': 'cdr_dcdcsr_map_fwd_grad_workspace_bytes'}.get(name, f'cdr_{name}_fwd_grad_workspace_bytes')
    for B, shape in REFUSED[name]:
        assert query(name, B, shape, need) != 0, (B, shape)
        assert entry.encode() in lib.cdr_last_error()
        assert need.value == 12345                                     # a refused query writes nothing
    good = SHAPES[name][0]
    assert getattr(lib, entry)(*_null_out(name, good)) != 0 and lib.cdr_last_error()
    assert need.value == 12345
    assert query(name, 64, good, need) == 0 and need.value not in (0, 12345)


def _null_out(name, shape):
    """The entry's arguments for a valid shape with a null ``bytes`` pointer."""
    if name == 'clfm':
        return 64, shape[0], shape[1], None
    if name == 'dtcdr':
        return 64, shape[0], len(shape) - 1, _ints(shape[1:]), None
    if name == 'deepapf':
        return 64, shape[0], None
    return 64, len(shape) - 1, _ints(shape), None
