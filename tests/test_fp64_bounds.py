"""Self-tests of the bound helpers in fp64_bounds.py (no GPU): the gradient-free Adam recurrence that test_gpu_conet_fp64.py carries
through a row's postponed updates must hold an fp32 replay of the kernels' arithmetic (cdr_adam_math.h) and must NOT hold one whose bias
corrections are those of the neighbouring update."""
import pytest
import torch

from fp64_bounds import adam_idle_fp64, adam_replay_fp64


def _hp(t, lr, b1, b2):
    """cdr_adam_hp: step size and 1 / sqrt(bias correction 2) of update t, rounded once from fp64 to fp32."""
    return (torch.tensor(lr / (1.0 - b1 ** t), dtype=torch.float32), torch.tensor(1.0 / (1.0 - b2 ** t) ** 0.5, dtype=torch.float32))


def _replay_f32(w, m, v, t_from, n, lr, wd, b1, b2, eps, shift=0):
    """cdr_adam_elem with g = 0 in fp32, every operation rounded on its own; ``shift`` = -1 takes the bias corrections of update t - 1."""
    lr32, wd32, b132, b232, eps32 = (torch.tensor(x, dtype=torch.float32) for x in (lr, wd, b1, b2, eps))
    one = torch.tensor(1.0, dtype=torch.float32)
    for t in range(t_from + 1, t_from + n + 1):
        ss, bc2 = _hp(t + shift, float(lr32), float(b132), float(b232))
        g = wd32 * w if wd else torch.zeros_like(w)
        m = m + (g - m) * (one - b132)
        v = b232 * v + ((one - b232) * g) * g
        w = w - ss * (m * (one / (v.sqrt() * bc2 + eps32)))
    return w, m, v


def _rows(seed, n=4096, D=64):
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(n, D, generator=gen) * 0.5
    m = torch.randn(n, D, generator=gen) * 1e-3
    v = m * m * (0.25 + torch.rand(n, D, generator=gen)) + 1e-12
    return w, m, v


@pytest.mark.parametrize('wd,betas,eps', [(0.0, (0.9, 0.999), 1e-8), (1e-2, (0.9, 0.999), 1e-8), (1e-2, (0.8, 0.99), 1e-6)],
                         ids=['default', 'wd', 'betas'])
@pytest.mark.parametrize('t_from,n', [(1000, 1), (1000, 6), (0, 12), (3, 40)])
def test_idle_adam_bound_holds_fp32_and_sees_shifted_bias_correction(wd, betas, eps, t_from, n):
    lr = 1e-3
    b1, b2 = betas
    w, m, v = _rows(t_from + n)
    z = torch.zeros_like(w, dtype=torch.float64)
    ref, err = adam_replay_fp64({'w': w.double(), 'm': m.double(), 'v': v.double()}, {'w': z, 'm': z, 'v': z}, t_from, n, lr, wd, b1, b2, eps)
    got = _replay_f32(w, m, v, t_from, n, lr, wd, b1, b2, eps)
    for k, x in zip('wmv', got):
        r = float(((x.double() - ref[k]).abs() / err[k].clamp(min=1e-300)).max())
        assert r <= 1.0, (k, r)
    if t_from == 0 or (t_from >= 1000 and b2 != 0.999):
        return                  # (update 0 has no predecessor; b2 = 0.99 has forgotten its bias correction long before update 1,000)
    # bias corrections one update off: near update 1,000 (b2 = 0.999) that moves the update term by ~3e-4 of itself, in the first
    # updates by far more -- outside the bound, which is a few ulps of the term
    bad = _replay_f32(w, m, v, t_from, n, lr, wd, b1, b2, eps, shift=-1)[0]
    r = (bad.double() - ref['w']).abs() / err['w']
    assert float(r.max()) > 20, float(r.max())
    assert float((r > 1).double().mean()) > 0.5, float((r > 1).double().mean())


def test_idle_adam_bound_fixed_point_and_weight_decay():
    """wd = 0 and zero moments: the recurrence is the identity (the replay's fixed-point shortcut may skip it); with wd != 0 it moves."""
    w = torch.randn(64, 16, dtype=torch.float64)
    z = torch.zeros_like(w)
    st, er = adam_idle_fp64({'w': w, 'm': z, 'v': z}, {'w': z, 'm': z, 'v': z}, 1001, 1e-3)
    assert torch.equal(st['w'], w) and torch.equal(st['m'], z) and torch.equal(st['v'], z)
    st, er = adam_idle_fp64({'w': w, 'm': z, 'v': z}, {'w': z, 'm': z, 'v': z}, 1001, 1e-3, wd=1e-2)
    assert float(((st['w'] - w).abs() > 8 * er['w']).double().mean()) > 0.99
