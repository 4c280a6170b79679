"""The yardstick of test_gpu_sscdr_map_fp64.py must be able to fail (no GPU): ``sscdr_map_fp64.check_map_loss`` -- the comparison the device
result of functional.SSCDRMapLoss goes through -- is run on the CPU with an fp32 restatement of sscdr_map_loss_kernel's own formulas
(csrc/cdr_elem.hip: the row sums, sq_norm_bwd, the coefficients 2 / (n D) and lamda / n) in place of the device result.  The unmutated
restatement must pass at every shape, margin, lamda and upstream gradient the GPU test uses; each of twelve single mutations of it must be
rejected at (n, D) = (100, 20) and (300, 128).  The same run asserts the input conditions the GPU tests rely on -- branch populations, the
exclusion cap, 4 E_ref <= 1e-3 max |G64| -- on the very tensors they use (the cases are drawn from CPU generators), so a bad recipe shows
before a GPU is involved; for fused.SSCDRMapStep's cases the three steps are played through on the CPU with the fp32 reference standing in
for the device."""
import pytest
import torch

import sscdr_map_fp64 as R
from fp64_bounds import apply_fp64

MUTATIONS = ['div_L_always', 'sqrt_L', 'dot_over_L', 'no_dot_term', 'cu_over_nD', 'cs_half', 'GT_without_gs', 'GT_u1_plus_u2', 'no_eps',
             'closed_hinge_gradient', 'rows_swapped', 'row_of_32_left_zero']


def kernel_restated(M3, T, margin, lamda, go=1.0, mutation=None):
    """sscdr_map_loss_kernel + sscdr_map_finish_kernel + scale2_unless_one_kernel in fp32 torch, formula by formula (no autograd), with one
    piece replaced by ``mutation``.  Returns what check_map_loss takes."""
    assert mutation is None or mutation in MUTATIONS
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    n, D = T.shape
    ms, mp, mq, t = M3[:n], M3[n:2 * n], M3[2 * n:], T
    eps = f32(0.0 if mutation == 'no_eps' else R.EPS)
    cs = f32(1.0 if mutation == 'cs_half' else 2.0) / f32(float(n * D))
    cu = f32(lamda) / f32(float(n * D if mutation == 'cu_over_nD' else n))
    d = ms - t
    se, lt, lp, lq = (d * d).sum(1), (t * t).sum(1), (mp * mp).sum(1), (mq * mq).sum(1)

    def divisor(L):
        if mutation == 'div_L_always':
            return L
        return torch.where(L > 1, L.sqrt() if mutation == 'sqrt_L' else L, torch.ones_like(L))
    av, bp, bq = t / divisor(lt)[:, None], mp / divisor(lp)[:, None], mq / divisor(lq)[:, None]
    dp, dn = av - bp + eps, av - bq + eps
    d1, d2 = (dp * dp).sum(1).sqrt(), (dn * dn).sum(1).sqrt()
    hinge = d1 - d2 + f32(margin)
    active = torch.ones_like(hinge, dtype=torch.bool) if mutation == 'closed_hinge_gradient' else hinge > 0
    zero = torch.zeros_like(dp)
    u1 = torch.where((active & (d1 > 0))[:, None], dp / d1[:, None], zero)
    u2 = torch.where((active & (d2 > 0))[:, None], dn / d2[:, None], zero)
    ga = cu * (u1 + u2 if mutation == 'GT_u1_plus_u2' else u1 - u2)
    gp, gq = -cu * u1, cu * u2

    def sq_norm_bwd(x, g, L):
        dot = (x * g).sum(1)[:, None]
        L = L[:, None]
        if mutation == 'no_dot_term':
            inner = g / L
        else:
            inner = g / L - (2.0 * dot / (L if mutation == 'dot_over_L' else L * L)) * x
        return inner if mutation == 'div_L_always' else torch.where(L > 1, inner, g)
    gs = cs * d
    G3 = torch.cat([gs, sq_norm_bwd(mp, gp, lp), sq_norm_bwd(mq, gq, lq)])
    GT = (0 if mutation == 'GT_without_gs' else -gs) + sq_norm_bwd(t, ga, lt)
    if mutation == 'rows_swapped':
        G3 = torch.cat([G3[:n], G3[2 * n:], G3[n:2 * n]])
    if mutation == 'row_of_32_left_zero':
        G3 = G3.clone()
        for blk in (G3[:n], G3[n:2 * n], G3[2 * n:], GT):
            blk[31::32] = 0
    ls = (se.double().sum() / (n * D)).float()
    lu = (hinge.clamp(min=0).double().sum() / n).float()
    total = ls + f32(lamda) * lu
    G3, GT = G3 + 0.0, GT + 0.0                     # (a closed hinge leaves -cu x 0 = -0.0: the gradients leave the kernel as +0.0)
    if go != 1.0:
        G3, GT = G3 * f32(go), GT * f32(go)
    return {'total': total, 'parts': torch.stack([total, ls, lu]), 'G3': G3, 'GT': GT}


@pytest.mark.parametrize('margin', R.MARGINS)
@pytest.mark.parametrize('n,D', R.LOSS_SHAPES)
def test_fp32_restatement_passes_and_the_inputs_meet_their_conditions(n, D, margin):
    """Every (n, D, margin) of the GPU test's map-loss cases, with both lamda and both upstream gradients: the conditions on the reference
    (inside check_map_loss) hold and the kernel's formulas in fp32 are within the bound."""
    M3, T = R.loss_case(n, D)
    worst = {}
    for lamda, go in ((R.LAMDA, 1.0), (R.LAMDA, 2.5), (0.0, 1.0)):
        got = kernel_restated(M3, T, margin, lamda, go)
        *_, h, L, ex = R.check_map_loss(f'restated n={n} D={D} margin={margin} lamda={lamda} go={go}', got, M3, T, margin, lamda, go, worst)
    if n >= 100:
        assert int((L[:, 30] > 1).sum()) == 3 and bool((h[20:24] == margin).all()) and not bool(ex[10:14].any())     # the planted triples
    print(f'n={n} D={D} margin={margin}: worst restated / E_ref ' + ' '.join(f'{k}={v:.3f}' for k, v in worst.items()))


def _mutation_case(n, D):
    """The recipe with its planted triples; triples 10..13 (interacted == target) get a non-interacted row 0.005 away from the target in one
    column, so that their hinges are open at either margin and the eps of the distance carries their whole gradient."""
    gen = torch.Generator().manual_seed(77 * D + n)
    M3, T = R.rows(3 * n, D, gen), R.rows(n, D, gen)
    R.plant(M3, T)
    M3[2 * n + 10:2 * n + 14] = T[10:14]
    M3[2 * n + 10:2 * n + 14, 0] += 0.005
    return M3, T


@pytest.mark.parametrize('n,D', [(100, 20), (300, 128)])
def test_every_mutation_of_the_kernels_formulas_is_rejected(n, D):
    M3, T = _mutation_case(n, D)
    margin, lamda = 0.02, R.LAMDA
    *_, h, L, ex = R.check_map_loss(f'unmutated n={n} D={D}', kernel_restated(M3, T, margin, lamda), M3, T, margin, lamda)
    assert bool((h[10:14] > 0).all()) and not bool(ex[10:14].any())
    for mutation in MUTATIONS:
        with pytest.raises(AssertionError):
            R.check_map_loss(f'{mutation} n={n} D={D}', kernel_restated(M3, T, margin, lamda, mutation=mutation), M3, T, margin, lamda)
        # with the reference's own scalars in their place the mutation is caught in the gradients (or, for the forward-only ones that
        # move no kept gradient beyond the bound, nowhere: none of the twelve is such a one)
        got = kernel_restated(M3, T, margin, lamda, mutation=mutation)
        good = kernel_restated(M3, T, margin, lamda)
        with pytest.raises(AssertionError, match=r'E_ref|bit for bit'):
            R.check_map_loss(f'{mutation} (gradients) n={n} D={D}', dict(got, total=good['total'], parts=good['parts']), M3, T, margin, lamda)


def test_a_negative_zero_in_a_closed_hinge_is_rejected():
    """-0.0 where the triplet blocks must be +0.0 bit for bit (what -cu x 0 leaves) does not pass as a zero."""
    M3, T = R.loss_case(100, 20)
    got = kernel_restated(M3, T, 0.02, R.LAMDA)
    *_, h, _, ex = R.check_map_loss('unmutated', got, M3, T, 0.02, R.LAMDA)
    r = int(torch.nonzero((h <= 0) & ~ex)[0])
    got['G3'][100 + r, 3] = -0.0
    with pytest.raises(AssertionError, match='bit for bit'):
        R.check_map_loss('negative zero', got, M3, T, 0.02, R.LAMDA)


# ---------------------------------------------------------------------------------------------------------------------- the step's inputs

def _sgd_played_on_the_cpu(case):
    """The three SGD steps with the fp32 reference standing in for the device: the conditions of every step, from the state before it."""
    n, D = case['n'], case['D']
    lr = R.sgd_lr(n)
    tabs = {k: case[k].clone() for k in ('SA', 'TA', 'SB')}
    out = []
    for t, (idx, pos, neg) in enumerate(case['batches'], 1):
        args = (tabs['SA'], tabs['TA'], tabs['SB'], case['layers'], idx, pos, neg, case['margin'], case['lamda'])
        r64, r32 = R.map_step(*args, torch.float64), R.map_step(*args, torch.float32, bias_sum=R.bias_sum_of(n))
        tag = f'step case D={D} n={n} step {t}'
        R.populations(tag, r64['h'], r64['L'], case['margin'], need_hinges=False)
        mapped = float((r64['L'][1:] > 1).double().mean())
        assert 0.2 <= mapped <= 0.8, f'{tag}: {mapped:.3f} of the mapped rows have L > 1'
        ex = R.excluded(tag, r64['h'], r64['L'])
        out.append(int(ex.sum()))
        skip = R.skip_rows(case, (idx, pos, neg), ex)
        for name in ('SA', 'TA', 'SB'):
            rows_, G64 = r64[name]
            keep = ~skip[name][rows_]
            w0 = tabs[name][rows_]
            ref64, ref32 = w0.double() - lr * G64, (w0 - torch.tensor(lr, dtype=torch.float32) * r32[name][1]).double()
            e_ref, upd = float((ref32 - ref64)[keep].abs().max()), float((lr * G64)[keep].abs().max())
            assert 4 * e_ref <= 1e-3 * upd, f'{tag} {name}: 4 E_ref {4 * e_ref:.3e} does not resolve the update {upd:.3e}'
            tabs[name][rows_] = ref32.float()
        for g64, g32 in zip(r64['params'], r32['params']):
            e_ref, big = float((g32.double() - g64).abs().max()), float(g64.abs().max())
            assert 4 * e_ref <= 1e-3 * big, f'{tag}: 4 E_ref {4 * e_ref:.3e} does not resolve a parameter gradient {big:.3e}'
    return out


@pytest.mark.parametrize('shape', list(R.STEP_SHAPES))
@pytest.mark.parametrize('D', R.STEP_DIMS)
def test_step_cases_meet_their_conditions(D, shape):
    """fused.SSCDRMapStep's cases: 0.2..0.8 of the rows (and of the mapped rows alone) above L = 1 in every step, the exclusion cap, the
    bound resolving every table update and parameter gradient, no excluded triple in the first step, and the batch's planted ids."""
    case = R.step_case(D, shape)
    n, ra, rb = R.STEP_SHAPES[shape]
    for idx, pos, neg in case['batches']:
        hot = R.hot_count(n)
        assert int((pos == 7).sum()) >= hot and int((neg == 7).sum()) >= 1 and int((pos == neg).sum()) >= 4
        assert all(int(x.min()) == 0 for x in (idx, pos, neg)) and int(idx.max()) == ra - 1 and int(pos.max()) == int(neg.max()) == rb - 1
        assert torch.unique(idx).numel() < n
    excl = _sgd_played_on_the_cpu(case)
    assert excl[0] == 0, f'the first step must hold no near-threshold triple (the mapping is checked there), has {excl[0]}'


@pytest.mark.parametrize('D', R.DENSE_DIMS)
def test_dense_route_cases_meet_their_conditions(D):
    """The dense route's case: the ids repeat as described, no near-threshold triple, both sides of L = 1, the bound resolving the three
    table gradients and the four parameter gradients."""
    case = R.step_case(D, 'dense')
    n, ra, rb = R.DENSE_SHAPE
    idx, pos, neg = case['batches'][0]
    assert torch.unique(idx).numel() < n and int(torch.bincount(pos).max()) >= 40 and int(torch.bincount(neg).max()) >= 40
    assert len(set(pos.tolist()) & set(neg.tolist())) > 4 and int(torch.cat([pos, neg]).max()) < rb - 3
    args = (case['SA'], case['TA'], case['SB'], case['layers'], idx, pos, neg, case['margin'], case['lamda'])
    r64, r32 = R.map_step(*args, torch.float64), R.map_step(*args, torch.float32)
    R.populations(f'dense case D={D}', r64['h'], r64['L'], case['margin'], need_hinges=False)
    assert not bool(R.near(r64['h'], r64['L']).any())
    for g64, g32 in [(r64[k][1], r32[k][1]) for k in ('SA', 'TA', 'SB')] + list(zip(r64['params'], r32['params'])):
        e_ref, big = float((g32.double() - g64).abs().max()), float(g64.abs().max())
        assert 4 * e_ref <= 1e-3 * big, f'dense case D={D}: 4 E_ref {4 * e_ref:.3e} does not resolve {big:.3e}'


def test_apply_fp64_takes_the_parts_the_step_test_hands_it():
    """The Adam reference of the step test: rows, a summed gradient, zero bounds, one occurrence each."""
    case = R.step_case(8, 'batch100')
    idx, pos, neg = case['batches'][0]
    ref = R.map_step(case['SA'], case['TA'], case['SB'], case['layers'], idx, pos, neg, case['margin'], case['lamda'], torch.float64)
    mom = R.step_moments(case, ref)
    rows_, G = ref['SB']
    zero = torch.zeros_like(G)
    want = apply_fp64({'w': case['SB'], 'm': mom['SB'][0], 'v': mom['SB'][1]}, (rows_, G, zero, zero, torch.ones(rows_.numel(), dtype=torch.int64)),
                      8, 'adam', R.ADAM_LR, 0.0, R.TABLE_STEPS[2] + 1)
    assert set(want) == {'w', 'm', 'v'} and want['w'][0].shape == G.shape and bool((mom['SB'][1] > 0).all())
    moved = (want['w'][0] - case['SB'][rows_].double()).abs()
    assert 0 < float(moved.max()) < 10 * R.ADAM_LR
