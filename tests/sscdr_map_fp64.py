"""SSCDR's OVERLAP phase (sscdr.py:161-187) restated in plain torch, in any dtype, on any device: the squared-norm "normalize", the map loss
MSE(mapped source, target) + lamda x triplet(normalize(target), normalize(mapped interacted), normalize(mapped non-interacted)) with its
gradients through torch.autograd, and the whole step -- gather, tanh MLP, loss, gradients summed per distinct table row.  Shared by
test_gpu_sscdr_map_fp64.py (the kernels and fused.SSCDRMapStep on the device) and test_sscdr_map_fp64_host.py (an fp32 restatement of the
kernel's formulas and twelve mutations of it on the CPU: the check is shown to bite before it is trusted on the GPU).

The method is test_gpu_triplet_step.py's.  The loss has two kinks -- L = sum x^2 = 1 for each of the three normalised rows and the hinge
h = d1 - d2 + margin = 0 -- near which fp32 and fp64 may take different branches: triples with |h| < 1e-5 or any |L - 1| < 1e-5 (``near``)
are left out of the value comparison (they must be finite) and may be at most 0.1 % of n.  The error bound is the REFERENCE's own: the same
restatement in float32 gives E_ref = max |ref32 - ref64| over the compared elements of a gradient block, the result under test must stay
within 4 E_ref (another, fixed summation order), and 4 E_ref <= 1e-3 max |ref64| is asserted too, so that the bound resolves the block.
``check_map_loss`` is that comparison for SSCDRMapLoss's outputs; ``check_block`` the rule for one tensor."""
import torch
import torch.nn.functional as F

from fp64_bounds import LOSS_RTOL

EPS = 1e-6                  # nn.TripletMarginLoss's eps (sscdr.py:69 leaves the default)
NEAR = 1e-5                 # the same rule and value as NEAR in test_gpu_triplet_step.py
FACTOR = 4.0                # device within FACTOR x E_ref (test_gpu_triplet_step.py: another, fixed summation order; it measured 1.05)
RESOLVE = 1e-3              # FACTOR x E_ref <= RESOLVE x max |ref64|
CAP = 0.001                 # at most this share of the triples may be near a threshold
SMALL = 32                  # blocks of fewer compared numbers: E_ref is floored at half an ulp of the largest (check_block)


def normalize(x):
    """y = x / max(L, 1) with L = sum x^2 per row (the SQUARED length: the reference's quirk); returns (y, L detached [rows])."""
    L = (x * x).sum(1, keepdim=True)
    return x / torch.where(L > 1, L, torch.ones_like(L)), L.detach().squeeze(1)


def map_loss(M3, T, margin, lamda, dtype, go=1.0):
    """M3 [3 n, D] = [mapped source ; mapped interacted ; mapped non-interacted], T [n, D].  Returns (total, loss_s, loss_u, G3, GT, h [n],
    L [3, n]) in ``dtype``: the gradients are those of go x total, h the hinge values, L the squared lengths of (T, interacted, non-int.)."""
    n = T.shape[0]
    M3 = M3.detach().to(dtype).requires_grad_(True)
    T = T.detach().to(dtype).requires_grad_(True)
    loss_s = F.mse_loss(M3[:n], T)
    (yt, Lt), (yp, Lp), (yq, Lq) = normalize(T), normalize(M3[n:2 * n]), normalize(M3[2 * n:])
    loss_u = F.triplet_margin_loss(yt, yp, yq, margin=margin, p=2, eps=EPS)
    total = loss_s + lamda * loss_u
    G3, GT = torch.autograd.grad(go * total, (M3, T))
    with torch.no_grad():
        h = F.pairwise_distance(yt, yp, eps=EPS) - F.pairwise_distance(yt, yq, eps=EPS) + margin
    return total.detach(), loss_s.detach(), loss_u.detach(), G3, GT, h, torch.stack([Lt, Lp, Lq])


def near(h, L, tol=NEAR):
    """[n] bool: the triples within ``tol`` of a threshold -- the hinge, or L = 1 of any of their three rows."""
    return (h.abs() < tol) | ((L - 1).abs() < tol).any(0)


def mlp(x, layers):
    """sscdr.MLPLayers: tanh after every layer, the last included.  layers: [(W [out, in], b [out])]."""
    for W, b in layers:
        x = torch.tanh(x @ W.t() + b)
    return x


def wgrad_bias_sum(t):
    """The column sums of t [N, out] in t's dtype in the order of cdr_linear_wgrad_small's bias gradient (csrc/cdr_linear.hip): wgrad_split
    cuts the N rows into min(ceil(N / 512), 64) even-aligned chunks; each of a chunk's eight waves takes an even-aligned slice and adds its
    even and its odd rows in row order (`bsum += a[u]`), the two parities meet in one add, the waves are added in wave order and the chunks
    in chunk order."""
    N, out = t.shape
    nch = min(-(-N // 512), 64)
    chunk = (-(-N // nch) + 1) & ~1
    total = None
    for c0 in range(0, N, chunk):
        part = t[c0:c0 + chunk]
        per = (-(-part.shape[0] // 8) + 1) & ~1
        pad = torch.zeros(8 * per, out, dtype=t.dtype, device=t.device)            # (rows past the edge add +0.0: exact)
        pad[:part.shape[0]] = part
        pad = pad.view(8, per, out)
        acc = torch.zeros(8, 2, out, dtype=t.dtype, device=t.device)
        for j in range(per // 2):
            acc = acc + pad[:, 2 * j:2 * j + 2]
        s = acc[:, 0] + acc[:, 1]
        v = s[0]
        for w in range(1, 8):
            v = v + s[w]
        total = v if total is None else total + v
    return total


def bias_sum_of(n):
    """How the float32 reference of a step with n ids adds the 3 n per-row terms of a bias gradient.  At n = 4,099 (12,297 rows, 25 chunks)
    in the device's own order, ``wgrad_bias_sum``: a bias gradient is 8 to 256 numbers, each a sum with heavy cancellation, and torch's
    sum over the rows is several times more accurate than a chain of the device's depth -- against it the first layer's bias gradient
    (16 numbers, D = 8) measured 5.2 and 5.8 E_ref at an error of 3.7e-7 of its largest element, every other tensor below 4; in the device's
    order it measures 1.00.  At n = 100 and on the dense route torch's sum: no bias gradient there measured above 2.7."""
    return wgrad_bias_sum if n >= 1000 else None


def map_step(SA, TA, SB, layers, idx, pos, neg, margin, lamda, dtype, bias_sum=None):
    """The step's loss and gradients in ``dtype`` from the fp32 state (teacher forcing): gather, tanh MLP, ``map_loss``, the gradients
    summed per distinct row of each table (SB's id list is pos ++ neg).  Returns a dict: total / loss_s / loss_u, 'SA' / 'TA' / 'SB' =
    (distinct rows, summed gradient), 'params' = the gradients in ``layers`` order (W, b, W, b, ...), h [n], L [3, n].
    ``bias_sum``: how the per-row terms [3 n, out] of a bias gradient are added (default: torch's sum over the rows)."""
    n = idx.numel()
    ra, inv_a = torch.unique(idx, return_inverse=True)
    rb, inv_b = torch.unique(torch.cat([pos, neg]), return_inverse=True)
    # a bias as one leaf per row (the same values: the forward is unchanged), so that its gradient arrives as the per-row terms
    Ws = [W.detach().to(dtype).requires_grad_(True) for W, _ in layers]
    bs = [b.detach().to(dtype).expand(3 * n, -1).clone().requires_grad_(True) for _, b in layers]
    X3 = torch.cat([SA[ra].to(dtype)[inv_a], SB[rb].to(dtype)[inv_b]]).requires_grad_(True)
    Tt = TA[ra].to(dtype)[inv_a].requires_grad_(True)
    M3 = mlp(X3, list(zip(Ws, bs)))
    loss_s = F.mse_loss(M3[:n], Tt)
    (yt, Lt), (yp, Lp), (yq, Lq) = normalize(Tt), normalize(M3[n:2 * n]), normalize(M3[2 * n:])
    loss_u = F.triplet_margin_loss(yt, yp, yq, margin=margin, p=2, eps=EPS)
    total = loss_s + lamda * loss_u
    gX, gT, *g = torch.autograd.grad(total, [X3, Tt] + Ws + bs)
    gP = [x for gW, terms in zip(g[:len(Ws)], g[len(Ws):]) for x in (gW, terms.sum(0) if bias_sum is None else bias_sum(terms))]
    with torch.no_grad():
        h = F.pairwise_distance(yt, yp, eps=EPS) - F.pairwise_distance(yt, yq, eps=EPS) + margin

    def summed(rows, inv, g):
        return rows, torch.zeros(rows.numel(), g.shape[1], device=g.device, dtype=dtype).index_add_(0, inv, g)
    return {'total': total.detach(), 'loss_s': loss_s.detach(), 'loss_u': loss_u.detach(), 'SA': summed(ra, inv_a, gX[:n]),
            'TA': summed(ra, inv_a, gT), 'SB': summed(rb, inv_b, gX[n:]), 'params': gP, 'h': h, 'L': torch.stack([Lt, Lp, Lq])}


def rows(n, D, gen):
    """The input recipe: randn x 0.6 / sqrt(D), a random half of the rows multiplied by 4 -- about half of them on each side of L = 1."""
    dev = gen.device
    t = torch.randn(n, D, device=dev, generator=gen) * (0.6 / D ** 0.5)
    t[torch.randperm(n, device=dev, generator=gen)[:n // 2]] *= 4.0
    return t


def plant(M3, T):
    """The planted triples of a map-loss case with n >= 100, in place: four with interacted == target (a distance of exactly
    eps sqrt(D)), four with interacted == non-interacted, one made of three rows of 10.0."""
    n = T.shape[0]
    assert n >= 100
    M3[n + 10:n + 14] = T[10:14]
    M3[n + 20:n + 24] = M3[2 * n + 20:2 * n + 24]
    M3[n + 30] = 10.0; M3[2 * n + 30] = 10.0; T[30] = 10.0
    return M3, T


def populations(tag, h, L, margin, need_hinges=True):
    """Both sides of both branches are exercised, asserted on the reference: 0.2 <= share of L > 1 <= 0.8 and, where asked (the balanced
    margin), at least 8 open and 8 closed hinges."""
    n = h.numel()
    above = float((L > 1).double().mean())
    assert 0.2 <= above <= 0.8, f'{tag}: {above:.3f} of the rows have L > 1'
    n_open = int((h > 0).sum())
    if need_hinges:
        assert n_open >= 8 and n - n_open >= 8, f'{tag}: {n_open} of {n} hinges open'
    return above, n_open


def excluded(tag, h, L):
    """The near-threshold mask [n], at most CAP of the triples (n >= 100; smaller cases may hold none at all)."""
    ex = near(h, L)
    n = h.numel()
    assert int(ex.sum()) <= CAP * n, f'{tag}: {int(ex.sum())} near-threshold triples of {n}'
    return ex


def half_ulp32(x):
    """Half an ulp of the fp32 value nearest to the float ``x`` (0 for 0)."""
    a = torch.tensor(abs(x), dtype=torch.float32)
    return float(torch.nextafter(a, torch.tensor(float('inf'))) - a) / 2 if x else 0.0


def check_block(tag, got, ref64, ref32, keep=None):
    """One tensor under the rule: over the kept rows, max |got - ref64| <= FACTOR E_ref with E_ref = max |ref32 - ref64|, and FACTOR E_ref
    <= RESOLVE max |ref64|; everything finite, kept or not.  Returns the ratio max |got - ref64| / E_ref (0 where both are 0).

    Over fewer than SMALL = 32 compared numbers E_ref has a floor, half an ulp (fp32) of max |ref64|: max |ref32 - ref64| is the largest of
    the block's rounding errors, and over the 4 to 24 numbers of the cases with n = 1 and n = 3 (a closed hinge zeroes most of them) it can
    by chance lie far below the half ulp of the block's largest value -- 2.8e-9 against 1.5e-8 at (n, D) = (3, 8), where the kernel's
    own formulas in float32 on the CPU then stand at 5 E_ref -- which is what the float32 format itself gives for that value and no fp32
    result is entitled to beat.  The floor also covers the other blocks below 32 numbers: the mapping's bias gradients and updated biases
    (8 to 24 numbers), the 1 x 4 normalize case and the saved length of the 5-row one.  Every block of 32 numbers or more is held to the
    reference's own error alone."""
    assert got.shape == ref64.shape == ref32.shape, (tag, got.shape, ref64.shape, ref32.shape)
    assert bool(torch.isfinite(got).all()), f'{tag}: non-finite values'
    g, r64, r32 = got.detach().to(ref64.device).double(), ref64.double(), ref32.double()
    if keep is not None:
        g, r64, r32 = g[keep], r64[keep], r32[keep]
    if g.numel() == 0:
        return 0.0
    e_stat, e_dev, big = float((r32 - r64).abs().max()), float((g - r64).abs().max()), float(r64.abs().max())
    floor = half_ulp32(big) if g.numel() < SMALL else 0.0
    e_ref = max(e_stat, floor)
    ratio = e_dev / e_ref if e_ref > 0 else (0.0 if e_dev == 0 else float('inf'))
    print(f'{tag}: max |got - ref64| {e_dev:.3e}  E_ref {e_ref:.3e} (max |ref32 - ref64| {e_stat:.3e}, floor '
          f'{floor:.3e})  ratio {ratio:.3f}  max |ref64| {big:.3e}')
    assert FACTOR * e_ref <= RESOLVE * big, f'{tag}: {FACTOR:g} E_ref {FACTOR * e_ref:.3e} does not resolve max |ref64| {big:.3e}'
    assert e_dev <= FACTOR * e_ref, f'{tag}: max |got - ref64| {e_dev:.3e} > {FACTOR:g} E_ref {FACTOR * e_ref:.3e}'
    return ratio


def _bits_zero(t):
    return t.contiguous().view(torch.int32) == 0


def check_map_loss(tag, got, M3, T, margin, lamda, go=1.0, worst=None):
    """SSCDRMapLoss's outputs -- got = {'total', 'parts' [3], 'G3', 'GT'} in fp32 -- for the inputs M3, T against ``map_loss`` in float64:
      * total, loss_s, loss_u within LOSS_RTOL of fp64, parts[0] == total;
      * each of the four gradient blocks over the non-excluded rows under ``check_block``; excluded rows finite;
      * rows of closed, non-excluded hinges: both triplet blocks bit-zero, GT[r] == -G3[r] bit for bit;
      * lamda == 0: both triplet blocks bit-zero everywhere.
    At n >= 100 the branch populations (the hinge's at the balanced margin 0.02 only) and the exclusion cap are asserted first.
    Returns the reference (total, loss_s, loss_u, G3, GT, h, L, excluded)."""
    n, D = T.shape
    t64, s64, u64, G3_64, GT_64, h, L = map_loss(M3, T, margin, lamda, torch.float64, go)
    _, _, _, G3_32, GT_32, _, _ = map_loss(M3, T, margin, lamda, torch.float32, go)
    if n >= 100:
        populations(tag, h, L, margin, need_hinges=margin < 0.1)
        ex = excluded(tag, h, L)
    else:
        ex = near(h, L)
    keep = ~ex
    parts = got['parts']
    assert float(parts[0]) == float(got['total']), f'{tag}: parts[0] {float(parts[0])!r} != total {float(got["total"])!r}'
    for name, g, w in (('total', parts[0], t64), ('loss_s', parts[1], s64), ('loss_u', parts[2], u64)):
        g, w = float(g), float(w)
        print(f'{tag} {name}: {g:.9g} fp64 {w:.9g}')
        assert abs(g - w) <= LOSS_RTOL * abs(w), f'{tag}: {name} {g!r} vs fp64 {w!r}'
    G3, GT = got['G3'], got['GT']
    assert G3.dtype == GT.dtype == torch.float32 and tuple(G3.shape) == (3 * n, D) and tuple(GT.shape) == (n, D), tag
    for name, g, r64, r32 in (('G3[:n]', G3[:n], G3_64[:n], G3_32[:n]), ('G3[n:2n]', G3[n:2 * n], G3_64[n:2 * n], G3_32[n:2 * n]),
                              ('G3[2n:]', G3[2 * n:], G3_64[2 * n:], G3_32[2 * n:]), ('GT', GT, GT_64, GT_32)):
        ratio = check_block(f'{tag} {name}', g, r64, r32, keep)
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), ratio)
    closed = keep & (h <= 0)
    for name, blk in (('G3[n:2n]', G3[n:2 * n]), ('G3[2n:]', G3[2 * n:])):
        where = closed if lamda != 0 else torch.ones_like(closed)
        bad = ~_bits_zero(blk[where]).all(1)
        assert not bool(bad.any()), (f'{tag} {name}: {int(bad.sum())} of {int(where.sum())} rows that must be +0.0 bit for bit are not, e.g. '
                                     f'row {int(torch.nonzero(where).view(-1)[torch.nonzero(bad)[0, 0]])}')
    neg = (-G3[:n][closed]).contiguous().view(torch.int32)
    assert torch.equal(GT[closed].contiguous().view(torch.int32), neg), f'{tag}: GT[r] != -G3[r] bit for bit in a closed hinge'
    return t64, s64, u64, G3_64, GT_64, h, L, ex


# ---------------------------------------------------------------------------------------------------------------------- cases
# Every input is drawn from a CPU generator, so that test_sscdr_map_fp64_host.py can assert the conditions the GPU tests rely on (branch
# populations, the exclusion cap, 4 E_ref resolving the gradients) on exactly the tensors the GPU tests move to the device.

LOSS_SHAPES = [(1, 4), (3, 8), (100, 20), (100, 64), (4099, 100), (4099, 128), (8197, 8), (2048, 256), (700, 260)]
MARGINS = (0.2, 0.02)       # the model's setting (few closed hinges at D >= 64) and the balanced one
LAMDA = 0.5
STEP_SHAPES = {'batch100': (100, 512, 256), 'blocks': (4099, 8192, 4096)}      # n, rows of source_a and target_a, rows of source_b
DENSE_SHAPE = (257, 300, 200)                   # the dense route's one shape (the key 'dense' of step_case); its mapping is [D, 12, D]
DENSE_DIMS = [8, 20, 64]
DENSE_HIDDEN = 12
STEP_DIMS = [8, 24, 64, 128, 256]
STEP_HIDDEN = 16
STEPS = 3
ADAM_LR = 1e-3
TABLE_STEPS = (1000, 37, 5)                     # update counts of source_a, target_a, source_b before the first step
PARAM_STEP0 = 411


def loss_case(n, D):
    """(M3 [3 n, D], T [n, D]) of the ``rows`` recipe on the CPU, with the planted triples where n >= 100."""
    gen = torch.Generator().manual_seed(1000 * D + n)
    M3, T = rows(3 * n, D, gen), rows(n, D, gen)
    if n >= 100:
        plant(M3, T)
    return M3, T


def hot_count(n):
    """Occurrences of the hot id among the positives: 300 (past 256: the piece kernels of the segmented apply) where the batch has them."""
    return 300 if n >= 1000 else n // 2


def step_batch(n, ra, rb, gen):
    """idx / pos / neg [n]: idx repeats by chance, one id ``hot_count(n)`` times in pos and once in neg, pos[r] == neg[r] in four places,
    ids 0 and rows - 1 in every list."""
    idx = torch.randint(0, ra, (n,), generator=gen)
    pos = torch.randint(0, rb, (n,), generator=gen)
    neg = torch.randint(0, rb, (n,), generator=gen)
    hot = hot_count(n)
    pos[:hot] = 7
    neg[hot + 5:hot + 9] = pos[hot + 5:hot + 9]
    neg[hot + 12] = 7
    idx[-1], idx[-2], pos[-3], pos[-4], neg[-5], neg[-6] = 0, ra - 1, 0, rb - 1, 0, rb - 1
    return idx, pos, neg


def dense_batch(n, ra, rb, gen):
    """idx / pos / neg [n] of the dense route: idx repeats, pos and neg share ids with each other and each repeats one id 40 times."""
    idx = torch.randint(0, ra, (n,), generator=gen)
    pos = torch.randint(0, rb // 2, (n,), generator=gen)
    neg = torch.randint(rb // 4, rb - 3, (n,), generator=gen)                      # (the last three rows of source_b are named by no id)
    idx[:9] = 11
    pos[50:90] = 5
    neg[120:160] = rb // 4 + 1
    return idx, pos, neg


def _step_case(D, shape, margin, seed):
    n, ra, rb = DENSE_SHAPE if shape == 'dense' else STEP_SHAPES[shape]
    hidden, make_batch = (DENSE_HIDDEN, dense_batch) if shape == 'dense' else (STEP_HIDDEN, step_batch)
    gen = torch.Generator().manual_seed(seed)
    SA, TA, SB = rows(ra, D, gen), rows(ra, D, gen), rows(rb, D, gen)
    W1 = torch.randn(hidden, D, generator=gen)
    b1 = torch.randn(hidden, generator=gen) * 0.1
    W2 = torch.randn(D, hidden, generator=gen)
    b2 = torch.randn(D, generator=gen) * (0.1 / D ** 0.5)
    batches = [make_batch(n, ra, rb, gen) for _ in range(STEPS)]
    idx, pos, neg = batches[0]
    z = torch.tanh(torch.cat([SA[idx], SB[pos], SB[neg]]).double() @ W1.double().t() + b1.double()) @ W2.double().t()
    sq_len = lambda s: torch.tanh(s * z + b2.double()).pow(2).sum(1)
    lo, hi = 1e-4, 1e2
    for _ in range(60):
        mid = (lo * hi) ** 0.5
        lo, hi = (mid, hi) if float(sq_len(mid).median()) < 1.0 else (lo, mid)
    for _ in range(200):                            # (the median row itself -- the hot id's, in a small batch -- sits at 1)
        if float((sq_len(lo) - 1).abs().min()) >= 4 * NEAR:
            break
        lo *= 1.0005
    W2 = W2 * float(torch.tensor(lo, dtype=torch.float32))
    return {'n': n, 'D': D, 'SA': SA, 'TA': TA, 'SB': SB, 'layers': [(W1, b1), (W2, b2)], 'batches': batches, 'margin': margin, 'lamda': LAMDA,
            'gen': gen, 'seed': seed}


_CASES = {}


def step_case(D, shape, margin=0.2):
    """Tables, the [D, 16, D] tanh mapping and the three batches of an SSCDRMapStep case ('dense': [D, 12, D], the dense route's shape and
    batches; it uses the first), on the CPU.  The mapping's first layer is N(0, 1) (pre-activations of order one on rows of squared length
    0.36 or 5.76); its last layer is scaled so that the median squared length of the first batch's mapped rows is 1 (bisection on the
    scale, then steps of 0.05 % until no row is within 4e-5 of 1), which puts both sides of L = 1 among them.  The seed is the first of
    100000 + 1000 D + n + {0, 7, 14, ...} whose FIRST step has no near-threshold triple in float64 (the mapping's gradients are checked in
    such steps only, and the first must be one).  Returns fresh copies."""
    key = (D, shape, margin)
    if key not in _CASES:
        n = DENSE_SHAPE[0] if shape == 'dense' else STEP_SHAPES[shape][0]
        for k in range(16):
            case = _step_case(D, shape, margin, 100000 + 1000 * D + n + 7 * k)
            ref = map_step(case['SA'], case['TA'], case['SB'], case['layers'], *case['batches'][0], margin, LAMDA, torch.float64)
            if not bool(near(ref['h'], ref['L']).any()):
                break
        else:
            raise AssertionError(f'no seed gives D={D} {shape} a first step without a near-threshold triple')
        case['gen_state'] = case.pop('gen').get_state()
        _CASES[key] = case
    case = dict(_CASES[key])
    for name in ('SA', 'TA', 'SB'):
        case[name] = case[name].clone()
    case['layers'] = [(W.clone(), b.clone()) for W, b in case['layers']]
    case['gen'] = torch.Generator()
    case['gen'].set_state(case['gen_state'])
    return case


def skip_rows(case, batch, ex):
    """{table: bool [rows]} -- the rows of near-threshold triples, left out of the value comparison: target_a[idx[r]], source_b[pos[r]] and
    source_b[neg[r]].  source_a's rows are never left out: the MSE branch has no kink."""
    idx, pos, neg = batch
    dev = ex.device
    out = {name: torch.zeros(case[name].shape[0], dtype=torch.bool, device=dev) for name in ('SA', 'TA', 'SB')}
    out['TA'][idx[ex]] = True
    out['SB'][pos[ex]] = True
    out['SB'][neg[ex]] = True
    return out


def step_moments(case, ref):
    """Nonzero Adam moments of the scale of the first step's gradients ``ref`` (map_step's result) for the three tables and the four
    mapping parameters: m ~ N(0, s^2), v in [0.25, 4.25) s^2."""
    gen = case['gen']

    def fill(shape, s):
        return torch.randn(shape, generator=gen) * s, (0.25 + 4 * torch.rand(shape, generator=gen)) * s * s
    out = {name: fill(case[name].shape, float(ref[name][1].pow(2).mean().sqrt())) for name in ('SA', 'TA', 'SB')}
    out['params'] = [fill(g.shape, float(g.pow(2).mean().sqrt())) for g in ref['params']]
    return out


def sgd_lr(n):
    """An update of the row's own magnitude: the triplet term's gradient of a row is lamda / n times a unit vector over max(L, 1), a row
    has length 0.6 or 2.4."""
    return n / 16.0
