"""The six row-wise steps with dense weights (CLFM, DTCDR, DeepAPF, DCDCSR's map step and frozen-side BPR step, SSCDR's map step) compute,
bit for bit, what they computed before their host and kernel code was merged into shared helpers (fused._Step / _DenseStep,
csrc/cdr_rowstep.h).  tools/record_rowstep_bits.py ran two consecutive Adam steps with weight decay per case at that commit -- twice,
with identical recordings -- and tests/golden/rowstep_parent_bits_<step>.npz keeps the touched table rows, moments and update counts,
out8 / out16, dP / dW and the dense parameters; the run is repeated here and every array must be equal.  Every sum in these steps runs
in a fixed order, so nothing is left out.  The cases (the tool's ``run``): D = 24 (pad and column guards) and D = 128 (non-temporal rows,
four tiles per wave, LDS above 64 KiB); 33 rows (a tail tile, two workgroups) and grid cap x 32 + 33 rows (the grid-stride loop); DTCDR
with dropout 0.25 from a fixed seed tensor; DeepAPF with half the keys above n_overlap; DCDCSR with the weights in LDS and read through
L2; both ``frozen`` sides."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = ('clfm', 'dtcdr', 'deepapf', 'dcdcsr', 'frozen', 'sscdr')


def _tool():
    spec = importlib.util.spec_from_file_location('record_rowstep_bits', os.path.join(HERE, '..', 'tools', 'record_rowstep_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('step', STEPS)
def test_rowstep_bits_match_the_parent(step):
    tool = _tool()
    assert tuple(tool.STEPS) == STEPS
    want = dict(np.load(tool.golden_path(os.path.join(HERE, 'golden'), step)))
    got = tool.run(step)
    assert sorted(got) == sorted(want) and len(want) >= 20
    for k in sorted(want):
        a, b = torch.from_numpy(got[k]), torch.from_numpy(want[k])
        assert a.dtype == b.dtype and torch.equal(a, b), f'{step}: {k} differs from the recording'
        if k.endswith('rest_moved'):
            assert int(a) == 0, f'{step}: {k}: a row no batch named has moved'
        elif k.endswith(('.w', '.m', '.v', '/dP', '/dW')):
            assert bool(a.isfinite().all()) and float(a.abs().max()) > 0, f'{step}: {k} is degenerate'
