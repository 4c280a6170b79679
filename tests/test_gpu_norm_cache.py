"""EmbLoss norms from a per-row cache (csrc/cdr_step.hip, "EmbLoss norms from a per-row cache"; fused.py: RowwiseState.n2): the fused BPR
step with norm_cache='on' against the same step gathering rows (norm_cache='off') from the same state -- tables, both moments and the loss
vector BIT-equal over free-running steps at every lane width; the records of every row bit-equal to a fresh build; every other writer of
a table leaves the records marked stale and the step on the gather path until the fifth eligible step; nothing of it under capture; a
refused allocation."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

BIG = (100003, 50021)          # almost every row of a 4,096-triple batch occurs once
SMALL = (300, 40)              # every row a duplicate: medium user segments, long item segments (> 32 occurrences: pieces + long finish)


def _pair(nu, ni, D, B, opt='adam', seed=0, **kw):
    from recbole_cdr_amd.fused import FusedBPRStep
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    U0 = torch.randn(nu, D, device=DEV, generator=g) * 0.1
    I0 = torch.randn(ni, D, device=DEV, generator=g) * 0.1
    mk = lambda mode, **k2: FusedBPRStep(U0.clone(), I0.clone(), B, opt=opt, lr=0.01 if opt == 'adam' else 0.05, reg_weight=0.02, id_path='sort',
                                         norm_cache=mode, **k2)
    return mk('on', **kw), mk('off')


def _tensors(s):
    out = [('U', s.U), ('I', s.I)]
    if s.ustate.exp_avg is not None:
        out += [('mU', s.ustate.exp_avg), ('vU', s.ustate.exp_avg_sq), ('mI', s.istate.exp_avg), ('vI', s.istate.exp_avg_sq)]
    return out


def _same(a, b, what=''):
    for (name, x), (_, y) in zip(_tensors(a), _tensors(b)):
        assert torch.equal(x, y), (what, name)
    assert torch.equal(a.out6[:9], b.out6[:9]), (what, a.out6[:9], b.out6[:9])


def _batch(case, nu, ni, B, g):
    u, p, n = (torch.randint(0, hi, (B,), device=DEV, generator=g) for hi in (nu, ni, ni))
    if case == 'hot':                                           # one item in 40 % of the positives and among the negatives
        p[: (2 * B) // 5] = 7
        n[B // 2: B // 2 + 50] = 7
    return u, p, n


def _fresh_norms(table):
    from recbole_cdr_amd import binding as B_
    rec = int(B_.load().cdr_norm_rec_floats())
    n2 = torch.full((table.shape[0], rec), 7.0, device=table.device)
    B_.call('cdr_row_norms_build', B_.stream(), B_.f32(table), table.shape[0], table.shape[1], B_.f32(n2))
    return n2


CASES = {'singles': (BIG, 4096, 'uniform'), 'dups': (SMALL, 4096, 'uniform'), 'hot': (SMALL, 4096, 'hot'), 'tail5': (BIG, 5, 'uniform'),
         'tail4093': (SMALL, 4093, 'hot')}


@pytest.mark.parametrize('opt', ['adam', 'sgd'])
@pytest.mark.parametrize('D', [12, 64, 128, 256])               # lanes per row: 4 (one of them dead), 16, 32, 64
@pytest.mark.parametrize('case', list(CASES))
def test_cached_step_is_bit_equal_to_the_gather_and_keeps_the_records_current(case, D, opt):
    (nu, ni), B, kind = CASES[case]
    a, b = _pair(nu, ni, D, B, opt)
    U_start = a.U.clone()
    g = torch.Generator(device=DEV); g.manual_seed(11)
    outs = []
    for step in range(6):
        u, p, n = _batch(kind, nu, ni, B, g)
        a.step(u, p, n); b.step(u, p, n)
        outs.append((a.out6[:9].clone(), b.out6[:9].clone()))
        assert a.ustate.n2_valid and a.istate.n2_valid, 'every step of the on object runs cached (the first one builds)'
    torch.cuda.synchronize()
    assert b.ustate.n2 is None and b.istate.n2 is None
    for step, (x, y) in enumerate(outs):
        assert torch.equal(x, y), (step, x, y)
    assert float(outs[0][0][4]) != 0.0 and float(outs[0][0][5]) != 0.0, 'the EmbLoss coefficients are in play'
    _same(a, b)
    for st in (a.ustate, a.istate):
        fresh = _fresh_norms(st.table)
        assert torch.equal(st.n2[:, 0], fresh[:, 0]), 'a record differs from a fresh build'
        assert int(torch.count_nonzero(st.n2[:, 1:])) == 0 and int(torch.count_nonzero(fresh[:, 1:])) == 0, 'records are written whole: padding 0'
        # D squares, all positive, summed in fp32 in some order: relative error at most ~(D + 3) * 2^-24 (products rounded or fused, D - 1 additions)
        want = (st.table.double() ** 2).sum(1)
        assert bool(((fresh[:, 0].double() - want).abs() <= (D + 3) * 2.0 ** -24 * want).all())
    assert float((a.U - U_start).abs().max()) > 0.0, 'the steps moved the table'


def _sync(a, b):
    """b := a (tables, moments, update counts on host and device): whatever the other writer did to a, the two go on from the same state."""
    for (_, x), (_, y) in zip(_tensors(a), _tensors(b)):
        y.copy_(x)
    for sa, sb in ((a.ustate, b.ustate), (a.istate, b.istate)):
        sb._step = sa._step
        if sa._step_dev is not None:
            sb.step_dev.copy_(sa._step_dev)
    torch.cuda.synchronize()


def _point(a, g):
    from recbole_cdr_amd.fused import FusedPointStep
    ps = FusedPointStep(a.U, a.I, 512, opt='adam', lr=0.01, reg_weight=0.02, user_state=a.ustate, item_state=a.istate)
    u, i = (torch.randint(0, t.shape[0], (512,), device=DEV, generator=g) for t in (a.U, a.I))
    ps.step(u, i, (torch.rand(512, device=DEV, generator=g) < 0.5).float())
    return a.ustate, a.istate


def _kmajor(a, g):
    from recbole_cdr_amd.fused import KMajorBPRStep
    ks = KMajorBPRStep(a.U, a.I, max_positives=256, k=2, opt='adam', lr=0.01, reg_weight=0.02, user_state=a.ustate, item_state=a.istate)
    u = torch.randint(0, a.U.shape[0], (256,), device=DEV, generator=g)
    p = torch.randint(0, a.I.shape[0], (256,), device=DEV, generator=g)
    n = torch.randint(0, a.I.shape[0], (512,), device=DEV, generator=g)
    ks.step(u, p, n)
    return a.ustate, a.istate


def _map(a, g):
    from recbole_cdr_amd.fused import FusedMapStep
    D = a.U.shape[1]
    W = (torch.eye(D, device=DEV) * 0.9).requires_grad_(True)
    T = torch.randn(a.U.shape[0], D, device=DEV, generator=g) * 0.1
    ms = FusedMapStep(a.U, T, lambda x: x @ W.t(), [W], 256, opt='adam', lr=0.01, source_state=a.ustate)
    ms.step(torch.randperm(a.U.shape[0], device=DEV, generator=g)[:256])
    return (a.ustate,)


def _mul(a, g):
    a.U.mul_(1.0001); a.I.mul_(1.0001)
    return a.ustate, a.istate


def _set_step(a, g):
    a.ustate.step = 3; a.istate.step = 3
    return a.ustate, a.istate


def _replayed(a, g):
    a.replayed()
    return a.ustate, a.istate


@pytest.mark.parametrize('writer', [_point, _kmajor, _map, _mul, _set_step, _replayed], ids=lambda f: f.__name__.strip('_'))
def test_another_writer_marks_the_records_stale_and_the_fifth_eligible_step_rebuilds(writer):
    nu, ni, D, B = 5003, 3001, 64, 4096
    a, b = _pair(nu, ni, D, B)
    g = torch.Generator(device=DEV); g.manual_seed(3)
    for _ in range(2):
        u, p, n = _batch('uniform', nu, ni, B, g)
        a.step(u, p, n); b.step(u, p, n)
    assert a.ustate.n2_valid and a.istate.n2_valid
    _same(a, b, 'before')
    touched = writer(a, g)
    for st in touched:
        assert not st.n2_valid, 'the writer must leave the records marked stale'
    _sync(a, b)
    for k in range(1, 6):
        u, p, n = _batch('uniform', nu, ni, B, g)
        a.step(u, p, n); b.step(u, p, n)
        torch.cuda.synchronize()
        _same(a, b, 'eligible step %d after %s' % (k, writer.__name__))
        valid = a.ustate.n2_valid and a.istate.n2_valid
        assert valid == (k == 5), 'the rebuild belongs to the fifth eligible step, not to step %d' % k
    for st in (a.ustate, a.istate):
        assert torch.equal(st.n2[:, 0], _fresh_norms(st.table)[:, 0])
    u, p, n = _batch('uniform', nu, ni, B, g)
    a.step(u, p, n); b.step(u, p, n)
    _same(a, b, 'cached again')


def test_alternating_writers_never_rebuild():
    """A phase that alternates the BPR step with another writer of its tables stays on the gather path: no table-sized pass per step."""
    nu, ni, D, B = 5003, 3001, 64, 4096
    a, b = _pair(nu, ni, D, B)
    g = torch.Generator(device=DEV); g.manual_seed(4)
    u, p, n = _batch('uniform', nu, ni, B, g)
    a.step(u, p, n); b.step(u, p, n)
    for _ in range(6):
        _set_step(a, g); _set_step(b, g)
        for _ in range(3):
            u, p, n = _batch('uniform', nu, ni, B, g)
            a.step(u, p, n); b.step(u, p, n)
            assert not a.ustate.n2_valid and not a.istate.n2_valid
    _same(a, b)


def test_capture_records_no_cached_launch():
    from recbole_cdr_amd import binding as B_
    nu, ni, D, B = 20011, 9001, 128, 4096
    a, b = _pair(nu, ni, D, B)
    u, p, n = (torch.randint(0, hi, (B,), device=DEV) for hi in (nu, ni, ni))
    su, sp, sn = u.clone(), p.clone(), n.clone()
    gr = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.step(su, sp, sn)                                      # warm on the capture stream (builds the records: an eligible eager step)
    torch.cuda.synchronize()
    assert a.ustate.n2_valid and a.istate.n2_valid
    b.step(u, p, n)
    with torch.cuda.stream(s):
        with B_.capturing(gr, s):
            a.step(su, sp, sn)
    torch.cuda.current_stream().wait_stream(s)
    assert not a.ustate.n2_valid and not a.istate.n2_valid
    # a captured reader would now take these for norms, a captured writer would overwrite them
    a.ustate.n2.fill_(1e30); a.istate.n2.fill_(1e30)
    for _ in range(3):
        u, p, n = (torch.randint(0, hi, (B,), device=DEV) for hi in (nu, ni, ni))
        su.copy_(u); sp.copy_(p); sn.copy_(n)
        gr.replay(); a.replayed(1)
        b.step(u, p, n)
    torch.cuda.synchronize()
    _same(a, b)
    assert bool((a.ustate.n2 == 1e30).all()) and bool((a.istate.n2 == 1e30).all())
    assert not a.ustate.n2_valid and not a.istate.n2_valid


def test_refused_allocation_keeps_the_gather():
    nu, ni, D, B = 5003, 3001, 64, 4096
    a, b = _pair(nu, ni, D, B, norm_cache_max_bytes=1024)
    g = torch.Generator(device=DEV); g.manual_seed(6)
    for _ in range(7):                                          # (past the retry after four eligible steps: refused again)
        u, p, n = _batch('uniform', nu, ni, B, g)
        a.step(u, p, n); b.step(u, p, n)
        assert a.ustate.n2 is None and a.istate.n2 is None and not a.ustate.n2_valid
    _same(a, b)


def test_auto_leaves_small_batches_and_exact_states_alone():
    from recbole_cdr_amd import binding as B_
    from recbole_cdr_amd.fused import FusedBPRStep, RowwiseState
    nu, ni, D, B = 5003, 3001, 64, 4096
    torch.manual_seed(8)
    U, I = torch.randn(nu, D, device=DEV) * 0.1, torch.randn(ni, D, device=DEV) * 0.1
    st = FusedBPRStep(U, I, B, opt='adam', lr=0.01, reg_weight=0.02)
    assert st.norm_cache == 'auto' and B <= st.COUNT_MAX_B
    st.step(*(torch.randint(0, hi, (B,), device=DEV) for hi in (nu, ni, ni)))
    assert st.ustate.n2 is None and st.istate.n2 is None, 'objects that never qualify allocate nothing'
    ex = FusedBPRStep(U, I, B, opt='adam', lr=0.01, reg_weight=0.02, norm_cache='on', id_path='sort',
                      user_state=RowwiseState(U, 1, exact=True), item_state=RowwiseState(I, 1, exact=True))
    assert not ex._select_norm_cache(B) and ex.ustate.n2 is None
    assert int(B_.load().cdr_norm_rec_floats()) in (16, 32)
