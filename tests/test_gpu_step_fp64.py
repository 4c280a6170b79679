"""The row-wise fused steps (FusedBPRStep, KMajorBPRStep, FusedPointStep) against a float64 restatement in plain torch, at the batch
sizes the benchmark runs and at every id-path threshold of csrc/cdr_step.hip (16,448 / 131,072 triples for the id counters,
3 B >= 2^18 for the big sort), held to PER-ELEMENT error bounds derived from the reference itself instead of a blanket atol.

Teacher forcing: each of the three steps of a case is judged from the device's own fp32 state before that step (tables, moments,
update count), so errors never pile up across steps; steps 2 and 3 reuse rows and check the bias corrections of update 2 and 3.

Bounds (u = 2^-24, gamma_k = k u / (1 - k u); every constant below is named and used once):
  * score x of an occurrence: e_x = gamma_{D+2} (sum|u p| + sum|u n|) + u |x|; carried through the loss derivative as
    delta = |dg/dx| e_x + K_COEF u (|dg/ds| s + |g|)  (sigmoid by expf, the subtraction 1 - s, the division and 1/B: <= K_COEF ulp);
  * EmbLoss coefficient c = reg / (B ||X||): relative gamma_{D+4} (fp32 row sums of D squares, then fp64, a sqrt and two fp32 ops);
  * summed row gradient: e_g = gamma_{D + occ + K_SUM} sum|terms| + (1 + gamma) sum(delta |row|)   (sum|terms| includes reg and wd);
  * SGD w: lr e_g + 2 u lr |g| + ulp(w);  Adam m, v: the two recurrences with e_g propagated + 3-4 u of their terms + ulp;
  * Adam w: the update lr/bc1 * m / (sqrt(v) / sqrt(bc2) + eps) evaluated over the m and v error intervals (not linearised), plus
    K_ADAM u of it (v_sqrt_f32 and v_rcp_f32 at 1 ulp each, four roundings, step_size and 1/sqrt(bc2) rounded to fp32), plus ulp(w).
The losses are held to 1e-5 relative of the fp64 value.  Rows outside the batch -- in particular the rows just above and below every
touched row -- and their moments are compared bit for bit."""
import pytest
import torch

from fp64_bounds import GAMMA, K_COEF, LOSS_RTOL, U32, _occ_sums, apply_fp64, bpr_grads_fp64, gam, point_grads_fp64   # noqa: F401 (re-exported)
from helpers import DEV

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------- checks

def _snapshot(st, opt):
    d = {'w': st.table.clone()}
    if opt == 'adam':
        d['m'], d['v'] = st.exp_avg.clone(), st.exp_avg_sq.clone()
    return d


def _live(st, opt):
    d = {'w': st.table}
    if opt == 'adam':
        d['m'], d['v'] = st.exp_avg, st.exp_avg_sq
    return d


def _check_table(tag, before, after, rows, want):
    """Touched rows within their bounds (returns the worst error / bound per quantity); every other row bit-identical, checked
    in particular on each touched row's two neighbours."""
    nrows = before['w'].shape[0]
    touched = torch.zeros(nrows, dtype=torch.bool, device=rows.device)
    touched[rows] = True
    nb = torch.cat([rows - 1, rows + 1]).clamp(0, nrows - 1)
    nb = nb[~touched[nb]]
    worst = {}
    for name, t0 in before.items():
        t1 = after[name]
        changed = (t0.view(torch.int32) != t1.view(torch.int32)).any(1)
        bad = changed & ~touched
        assert not bool(bad.any()), f'{tag}.{name}: {int(bad.sum())} rows outside the batch written, e.g. row {int(torch.nonzero(bad)[0])}'
        assert torch.equal(t0[nb].view(torch.int32), t1[nb].view(torch.int32)), f'{tag}.{name}: a neighbour of a touched row moved'
        ref, bound = want[name]
        got = t1[rows].double()
        assert bool(torch.isfinite(got).all()), f'{tag}.{name}: non-finite values'
        r = (got - ref).abs() / bound
        worst[name] = float(r.max())
        if worst[name] > 1.0:
            j = int(r.argmax())
            row, col = j // r.shape[1], j % r.shape[1]
            raise AssertionError(f'{tag}.{name}: error / bound = {worst[name]:.3g} at table row {int(rows[row])} col {col}: '
                                 f'got {float(got[row, col])!r} want {float(ref[row, col])!r} bound {float(bound[row, col]):.3g}')
    return worst


def _fmt(worst):
    return ' '.join(f'{k}={v:.3g}' for k, v in worst.items())


def _mark_edges(uid, pid, nid, nu, ni, gen):
    """Every batch: ids 0 and rows - 1 of both tables, and ~1 % of the triples with p == n."""
    uid[0], uid[1], pid[2], pid[3] = 0, nu - 1, 0, ni - 1
    if nid is not None:
        nid[4], nid[5] = 0, ni - 1
        same = torch.randint(0, uid.numel(), (max(1, uid.numel() // 100),), device=uid.device, generator=gen)
        nid[same] = pid[same]


def _zipf(n, rows, gen, a=1.05):
    """Zipf(a) ids over [0, rows) by inverse transform, as tests/test_gpu_trainer_graph.py builds the C5 positives."""
    r = torch.rand(n, device=gen.device, generator=gen, dtype=torch.float64)
    return (((float(rows) ** (1 - a) - 1) * r + 1).pow(1 / (1 - a)).long().clamp_(1, rows) - 1)


def _bpr_ids(shape, B, nu, ni, gen):
    u = torch.randint(0, nu, (B,), device=DEV, generator=gen)
    n = torch.randint(0, ni, (B,), device=DEV, generator=gen)
    if shape == 'zipf':
        p = _zipf(B, ni, gen)
    else:
        p = torch.randint(0, ni, (B,), device=DEV, generator=gen)
        if shape == 'hot':                               # one item with 20,000 occurrences (> 16,384: the count path's global list)
            p[torch.randperm(B, device=DEV, generator=gen)[:20000]] = ni // 3
    _mark_edges(u, p, n, nu, ni, gen)
    return u, p, n


# ---------------------------------------------------------------------------------------------------------------------- FusedBPRStep

def _bpr_cases():
    out = []
    for D in (64, 128):
        out += [(16447, D, 'adam', 'auto', 0.01, 0.0, 'uniform'),
                (16448, D, 'adam', 'count', 0.0, 0.0, 'uniform'), (16448, D, 'adam', 'sort', 0.01, 0.0, 'uniform'),
                (65536, D, 'adam', 'count', 0.01, 0.01, 'hot'), (65536, D, 'adam', 'sort', 0.01, 0.01, 'hot'),
                (100000, D, 'adam', 'count', 0.01, 0.0, 'zipf'), (100000, D, 'adam', 'sort', 0.01, 0.0, 'zipf'),
                (131072, D, 'adam', 'count', 0.01, 0.0, 'hot'), (131072, D, 'adam', 'sort', 0.0, 0.0, 'uniform'),
                (131073, D, 'adam', 'auto', 0.01, 0.0, 'uniform'),
                (1 << 20, D, 'adam', 'auto', 0.01, 0.0, 'zipf' if D == 128 else 'uniform')]
    out += [(65536, 128, 'sgd', 'count', 0.01, 0.01, 'uniform'), (1 << 20, 64, 'sgd', 'auto', 0.01, 0.01, 'hot')]
    out += [(65536, D, 'adam', 'count', 0.01, 0.0, 'uniform') for D in (8, 24, 256)]
    return out


def _run_bpr(fs, ust, ist, opt, lr, wd, reg, steps, tag, kmajor=0):
    """Drives ``steps`` (a list of (u, p, n) in the step's own layout) and checks each against the fp64 step from the device's state."""
    D = fs.D
    worst = {}
    for t, (u, p, n) in enumerate(steps, start=1):
        bu, bi = _snapshot(ust, opt), _snapshot(ist, opt)
        if kmajor:
            uf, pf = u.repeat(kmajor), p.repeat(kmajor)               # the B = S k triples the k-major step stands for
        else:
            uf, pf = u, p
        loss, upart, ipart = bpr_grads_fp64(bu['w'], bi['w'], uf, pf, n, reg)
        del uf, pf
        wu = apply_fp64(bu, upart, D, opt, lr, wd, t)
        wi = apply_fp64(bi, ipart, D, opt, lr, wd, t)
        out = fs.step(u, p, n)
        torch.cuda.synchronize()
        got = float(out[0])
        assert abs(got - loss) <= LOSS_RTOL * abs(loss), f'{tag} step {t}: loss {got!r} vs fp64 {loss!r}'
        assert ust.step == t and ist.step == t
        if ust._step_dev is not None:
            assert int(ust.step_dev) == t and int(ist.step_dev) == t, f'{tag}: device update counts'
        for name, wt in (('U', _check_table(f'{tag} step {t} U', bu, _live(ust, opt), upart[0], wu)),
                         ('I', _check_table(f'{tag} step {t} I', bi, _live(ist, opt), ipart[0], wi))):
            for k, v in wt.items():
                worst[f'{name}.{k}'] = max(worst.get(f'{name}.{k}', 0.0), v)
        del bu, bi, wu, wi, upart, ipart
    print(f'\n{tag}: worst error / bound over {len(steps)} steps: {_fmt(worst)}')
    return worst


@pytest.mark.parametrize('B,D,opt,path,reg,wd,shape', _bpr_cases())
def test_fused_bpr_step_vs_fp64(B, D, opt, path, reg, wd, shape):
    from recbole_cdr_amd.fused import FusedBPRStep
    gen = torch.Generator(device=DEV); gen.manual_seed(B + D)
    nu, ni = max(2 * B, 4096), max(B, 2048)                 # tables of the batch's order: rows recur across the three steps
    U = torch.empty(nu, D, device=DEV).normal_(0, 0.1, generator=gen)
    I = torch.empty(ni, D, device=DEV).normal_(0, 0.1, generator=gen)
    lr = 1e-3 if opt == 'adam' else 0.5
    fs = FusedBPRStep(U, I, B, opt=opt, lr=lr, reg_weight=reg, weight_decay=wd, id_path=path)
    steps = [_bpr_ids(shape, B, nu, ni, gen) for _ in range(3)]
    _run_bpr(fs, fs.ustate, fs.istate, opt, lr, wd, reg, steps, f'FusedBPRStep B={B} D={D} {opt} {path} reg={reg} wd={wd} {shape}')


def test_fused_bpr_step_user_ids_above_2_24_vs_fp64():
    """A user table of more than 2^24 rows with ids above 2^24 (an fp32 cannot hold them: any float round trip of an id shows)."""
    from recbole_cdr_amd.fused import FusedBPRStep
    D, B = 64, 65536
    nu, ni = (1 << 24) + 4099, 65536
    free_b, _ = torch.cuda.mem_get_info()
    if free_b < 36e9:
        pytest.skip('needs ~30 GB of free HBM (a 2^24-row table with Adam moments and their snapshots)')
    gen = torch.Generator(device=DEV); gen.manual_seed(24)
    U = torch.empty(nu, D, device=DEV).normal_(0, 0.1, generator=gen)
    I = torch.empty(ni, D, device=DEV).normal_(0, 0.1, generator=gen)
    fs = FusedBPRStep(U, I, B, opt='adam', lr=1e-3, reg_weight=0.01, id_path='count')
    steps = []
    for _ in range(3):
        u, p, n = _bpr_ids('uniform', B, nu, ni, gen)
        u[B // 2:] = (1 << 24) + torch.randint(0, 4099, (B - B // 2,), device=DEV, generator=gen)    # half the users above 2^24
        u[7] = (1 << 24) + 1
        steps.append((u, p, n))
    _run_bpr(fs, fs.ustate, fs.istate, 'adam', 1e-3, 0.0, 0.01, steps, f'FusedBPRStep users={nu} D={D} adam count')


def test_kmajor_bpr_step_vs_fp64():
    """KMajorBPRStep, k = 4, S = 262,144 positives (B = 1,048,576 triples): the same loss and row updates as the B = S k triples."""
    from recbole_cdr_amd.fused import KMajorBPRStep
    S, k, D, reg, lr = 262144, 4, 128, 0.01, 1e-3
    nu, ni = 2 * S, S
    gen = torch.Generator(device=DEV); gen.manual_seed(4)
    U = torch.empty(nu, D, device=DEV).normal_(0, 0.1, generator=gen)
    I = torch.empty(ni, D, device=DEV).normal_(0, 0.1, generator=gen)
    fs = KMajorBPRStep(U, I, S, k=k, opt='adam', lr=lr, reg_weight=reg)
    assert fs.fuse_singles
    steps = []
    for _ in range(3):
        u = torch.randint(0, nu, (S,), device=DEV, generator=gen)
        p = _zipf(S, ni, gen)
        n = torch.randint(0, ni, (S * k,), device=DEV, generator=gen)
        u[0], u[1], p[2], p[3], n[4], n[5] = 0, nu - 1, 0, ni - 1, 0, ni - 1
        n[S + 9] = p[9]                                          # p == n in the second negative round
        steps.append((u, p, n))
    _run_bpr(fs, fs.ustate, fs.istate, 'adam', lr, 0.0, reg, steps, f'KMajorBPRStep S={S} k={k} D={D} adam', kmajor=k)


# ---------------------------------------------------------------------------------------------------------------------- FusedPointStep

@pytest.mark.parametrize('B', [2048, 131071, 131072, 524288])
@pytest.mark.parametrize('kind', ['mse', 'bce'])
def test_fused_point_step_vs_fp64(kind, B):
    from recbole_cdr_amd.fused import FusedPointStep
    D, reg, lr = 128, 0.01, 1e-3
    wd = 0.01 if kind == 'bce' else 0.0
    nu, ni = max(2 * B, 4096), max(B // 2, 1024)
    gen = torch.Generator(device=DEV); gen.manual_seed(B + (kind == 'bce'))
    U = torch.empty(nu, D, device=DEV).normal_(0, 0.1, generator=gen)
    I = torch.empty(ni, D, device=DEV).normal_(0, 0.1, generator=gen)
    fs = FusedPointStep(U, I, B, loss=kind, opt='adam', lr=lr, reg_weight=reg, weight_decay=wd)
    ust, ist = fs.ustate, fs.istate
    tag = f'FusedPointStep {kind} B={B} D={D} adam wd={wd}'
    worst = {}
    for t in range(1, 4):
        u = torch.randint(0, nu, (B,), device=DEV, generator=gen)
        i = _zipf(B, ni, gen) if t == 2 else torch.randint(0, ni, (B,), device=DEV, generator=gen)
        _mark_edges(u, i, None, nu, ni, gen)
        y = (torch.rand(B, device=DEV, generator=gen) < 0.5).float()
        bu, bi = _snapshot(ust, 'adam'), _snapshot(ist, 'adam')
        loss, upart, ipart = point_grads_fp64(bu['w'], bi['w'], u, i, y, reg, kind)
        wu, wi = apply_fp64(bu, upart, D, 'adam', lr, wd, t), apply_fp64(bi, ipart, D, 'adam', lr, wd, t)
        got = float(fs.step(u, i, y)[0])
        assert abs(got - loss) <= LOSS_RTOL * abs(loss), f'{tag} step {t}: loss {got!r} vs fp64 {loss!r}'
        for name, wt in (('U', _check_table(f'{tag} step {t} U', bu, _live(ust, 'adam'), upart[0], wu)),
                         ('I', _check_table(f'{tag} step {t} I', bi, _live(ist, 'adam'), ipart[0], wi))):
            for k, v in wt.items():
                worst[f'{name}.{k}'] = max(worst.get(f'{name}.{k}', 0.0), v)
    print(f'\n{tag}: worst error / bound over 3 steps: {_fmt(worst)}')


# ---------------------------------------------------------------------------------------------------------------------- id_path='auto'

def test_auto_id_path_is_bit_equal_to_the_sorted_path_while_it_switches():
    """id_path='auto' next to an id_path='sort' twin at B = 32,768 on a stream that alternates 20 skewed steps (one item in a
    quarter of the positives) and 20 uniform steps, twice: the switch must never change a result.  After every step out6[:9]
    is bit-equal and the id counters are back to zero; after every burst the tables and moments are bit-equal; the auto
    step changes its path at least three times."""
    from recbole_cdr_amd.fused import FusedBPRStep
    B, D, nu, ni = 32768, 64, 1 << 20, 1 << 20
    gen = torch.Generator(device=DEV); gen.manual_seed(32)
    U = torch.empty(nu, D, device=DEV).normal_(0, 0.1, generator=gen)
    I = torch.empty(ni, D, device=DEV).normal_(0, 0.1, generator=gen)
    auto = FusedBPRStep(U, I, B, opt='adam', lr=1e-3, reg_weight=0.01, id_path='auto')
    twin = FusedBPRStep(U.clone(), I.clone(), B, opt='adam', lr=1e-3, reg_weight=0.01, id_path='sort')
    flags, changes = [auto._use_count], 0
    for burst in range(4):
        skewed = burst % 2 == 0
        for _ in range(20):
            u = torch.randint(0, nu, (B,), device=DEV, generator=gen)
            p = torch.randint(0, ni, (B,), device=DEV, generator=gen)
            n = torch.randint(0, ni, (B,), device=DEV, generator=gen)
            if skewed:
                p[torch.randperm(B, device=DEV, generator=gen)[:B // 4]] = 12345
            a = auto.step(u, p, n)[:9].clone()
            b = twin.step(u, p, n)[:9].clone()
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'burst {burst}: out6 differs (use_count={auto._use_count})'
            if auto._count is not None:
                assert int(auto._count[0].count_nonzero()) == 0 and int(auto._count[1].count_nonzero()) == 0, 'id counters not cleared'
            if auto._use_count != flags[-1]:
                changes += 1
            flags.append(auto._use_count)
        for x, y in ((auto.U, twin.U), (auto.I, twin.I), (auto.ustate.exp_avg, twin.ustate.exp_avg),
                     (auto.ustate.exp_avg_sq, twin.ustate.exp_avg_sq), (auto.istate.exp_avg, twin.istate.exp_avg),
                     (auto.istate.exp_avg_sq, twin.istate.exp_avg_sq)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f'burst {burst}: tables / moments differ'
    print(f'\nauto id path: {changes} switches, path per step (1 = counters): {"".join(str(int(f)) for f in flags)}')
    assert changes >= 3
