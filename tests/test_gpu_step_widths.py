"""Every lane width of the fused row-wise steps other than FusedBPRStep (which test_gpu_parity.py already sweeps): FusedPointStep,
FusedPointPairStep, KMajorBPRStep and KMajorPointStep at D = 4 .. 256 -- lanes per row 1, 2, 4, 8, 16, 32 and 64, and D = 24 with dead
lanes inside a lane group -- for both optimizers.  The row helpers of csrc/cdr_step.hip (row_moments, row_store) are instantiated per
(lanes per row, optimizer): a helper can be right for one pair and wrong-shaped for another.

Each case runs three free-running steps against the oracle's row-wise step (oracle/train_step.py) on a batch in which most rows occur
once (updated in place by the forward kernel), some twice (gradient rows spilled, segmented apply) and one row more than 32 times (the
piece kernels).  Tables are held to the tolerances the existing tests of these classes use: rtol 2e-5 and atol lr * 1e-2 for Adam (one
last-bit difference in a gradient of the order of eps moves m / (sqrt(v) + eps) by up to 1e-2 of one update), 1e-6 for SGD.  A rerun
must be bit-equal.

The Adam bound rests on the fp32 oracle's own error staying below it, which depends on the draw: on these batches the oracle in fp32
is within 3.1e-4 of the oracle in fp64 on every element, and the device was measured within 1.7e-4 of the fp32 oracle.  A first cut of
the k-major cases drew users from 40,000 rows; there ONE element of 5.12 M (KMajorPointStep, D = 128, Adam, BCE) sat 5.83e-4 from the
fp32 oracle -- and the fp32 oracle sat 5.83e-4 from the fp64 oracle at its worst element of that draw: a gradient that cancels to ~eps,
the reference's error, not the kernel's.  Should a later change of draw trip the bound on a single element, compare the oracle with
itself in fp64 first."""
import pytest
import torch

from helpers import DEV, assert_close

pytestmark = pytest.mark.gpu

WIDTHS = [4, 8, 16, 24, 64, 128, 256]
LR, REG, STEPS = 0.05, 0.03, 3


def _tables(nu, ni, D):
    g = torch.Generator().manual_seed(1000 + D)
    return torch.randn(nu, D, generator=g) * 0.3, torch.randn(ni, D, generator=g) * 0.3


def _check(tag, opt, make, feed, oracle, U, I):
    """make(Ud, Id) -> step object; feed(step object, batch) -> loss scalar; oracle(Uo, Io, su, si, batch, t) -> loss.  Two device runs
    on the same batches: the first is compared with the oracle step by step, the second must repeat the first bit for bit."""
    from oracle import train_step as ts
    Uo, Io = U.clone(), I.clone()
    su, si = ts.RowwiseAdamState(Uo), ts.RowwiseAdamState(Io)
    runs = []
    for rep in range(2):
        Ud, Id = U.clone().to(DEV), I.clone().to(DEV)
        fs = make(Ud, Id)
        losses = []
        for t, batch in enumerate(feed.batches(), start=1):
            got = feed(fs, [b.to(DEV) for b in batch]).clone()
            losses.append(got)
            if rep == 0:
                want = oracle(Uo, Io, su, si, batch, t)
                print(f'{tag} step {t}: loss {float(got):.8f} oracle {float(want):.8f}')
                assert_close(got, want, what=f'{tag}: loss, step {t}')
        if rep == 0:
            atol = LR * 1e-2 if opt == 'adam' else 1e-6
            for name, d, o in (('U', Ud, Uo), ('I', Id, Io)):
                print(f'{tag} {name}: max |device - oracle| {float((d.cpu() - o).abs().max()):.3e} (atol {atol:.1e})')
                assert_close(d, o, rtol=2e-5, atol=atol, what=f'{tag}: {name} after {STEPS} steps')
            assert float((Ud.cpu() - U).abs().max()) > 0 and float((Id.cpu() - I).abs().max()) > 0
        runs.append((torch.stack(losses), Ud, Id))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), f'{tag}: rerun differs'


class _PointBatches:
    """700 (user, item, label) rows over 4,000 users and 2,500 items: most rows once, some twice, user 3 forty times."""
    nu, ni, B = 4000, 2500, 700

    def batches(self):
        g = torch.Generator().manual_seed(11)
        for t in range(STEPS):
            u = torch.randint(1, self.nu, (self.B,), generator=g); i = torch.randint(1, self.ni, (self.B,), generator=g)
            y = (torch.rand(self.B, generator=g) < 0.4).float()
            u[100:140] = 3                                       # 40 occurrences: past the head-only limit of the segmented apply
            if t == 1:
                i[300:340] = 5
            yield u, i, y

    def __call__(self, fs, b):
        return fs.step(*b)[0]


@pytest.mark.parametrize('opt', ['sgd', 'adam'])
@pytest.mark.parametrize('D', WIDTHS)
def test_point_step_widths(opt, D):
    from oracle import train_step as ts
    from recbole_cdr_amd.fused import FusedPointStep
    feed = _PointBatches()
    loss = 'bce' if D % 8 else 'mse'                            # both loss kinds over the sweep
    U, I = _tables(feed.nu, feed.ni, D)
    _check(f'FusedPointStep D={D} {opt} {loss}', opt,
           lambda Ud, Id: FusedPointStep(Ud, Id, feed.B, loss=loss, opt=opt, lr=LR, reg_weight=REG), feed,
           lambda Uo, Io, su, si, b, t: ts.rowwise_point_step(Uo, Io, su, si, *b, t, t, opt=opt, lr=LR, reg_weight=REG, loss=loss), U, I)


class _PairBatches(_PointBatches):
    """The same 700 rows as a source half and a target half (350 + 350) on the shared tables."""

    def __call__(self, fs, b):
        u, i, y = b
        h = self.B // 2
        return fs.step(u[:h], i[:h], y[:h], u[h:], i[h:], y[h:])[0]


@pytest.mark.parametrize('opt', ['sgd', 'adam'])
@pytest.mark.parametrize('D', WIDTHS)
def test_point_pair_step_widths(opt, D):
    """alpha = 1/2, two halves of equal size and no EmbLoss: the joint loss alpha BCE_s + (1 - alpha) BCE_t is the BCE mean over the 700
    rows, and ONE update per touched row from both halves' contributions is the oracle's pointwise step on the concatenated batch.  (The
    oracle's step has no per-domain weights, so the EmbLoss coefficients of this class stay with test_gpu_cmf_rowwise.py's fp64 check.)"""
    from oracle import train_step as ts
    from recbole_cdr_amd.fused import FusedPointPairStep
    feed = _PairBatches()
    U, I = _tables(feed.nu, feed.ni, D)
    h = feed.B // 2
    _check(f'FusedPointPairStep D={D} {opt}', opt,
           lambda Ud, Id: FusedPointPairStep(Ud, Id, h, h, 0.5, 0.0, 0.0, opt=opt, lr=LR), feed,
           lambda Uo, Io, su, si, b, t: ts.rowwise_point_step(Uo, Io, su, si, *b, t, t, opt=opt, lr=LR, reg_weight=0.0, loss='bce'), U, I)


class _KMajorBatches:
    """S positives with k negatives each (k-major), users over 4 S rows, items over S (1 + k) / 2 rows: users mostly once and some twice,
    items about half duplicated, item 5 seventy times, a positive that is its own first negative."""

    def __init__(self, S, k, point):
        self.S, self.k, self.point = S, k, point
        self.nu, self.ni = 4 * S, S * (1 + k) // 2

    def batches(self):
        g = torch.Generator().manual_seed(13)
        S, k = self.S, self.k
        for t in range(STEPS):
            u = torch.randint(1, self.nu, (S,), generator=g); p = torch.randint(1, self.ni, (S,), generator=g)
            n = torch.randint(1, self.ni, (S * k,), generator=g)
            n[:4] = p[:4]
            p[50:120] = 5
            if t == 1:
                u[300:309] = u[0]
            yield u, p, n

    def __call__(self, fs, b):
        u, p, n = b
        if not self.point:
            return fs.step(u, p, n)[0]
        y = torch.cat([torch.ones(self.S), torch.zeros(self.S * self.k)]).to(u.device)
        return fs.step(u.repeat(1 + self.k), torch.cat([p, n]), y)[0]


@pytest.mark.parametrize('opt', ['sgd', 'adam'])
@pytest.mark.parametrize('D', WIDTHS)
def test_kmajor_bpr_step_widths(opt, D):
    """S (1 + k) = 12,012 > 8,192: past the small-batch form, so bpr_fwd_apply_kmajor_kernel runs (asserted).  The oracle steps on the
    equivalent per-row batch [S k]: users and positives tiled k times."""
    from oracle import train_step as ts
    from recbole_cdr_amd.fused import KMajorBPRStep
    S, k = 2002, 5
    feed = _KMajorBatches(S, k, point=False)
    U, I = _tables(feed.nu, feed.ni, D)

    def make(Ud, Id):
        st = KMajorBPRStep(Ud, Id, max_positives=S, k=k, opt=opt, lr=LR, reg_weight=REG)
        assert not st.small and st.fuse_singles
        return st
    _check(f'KMajorBPRStep D={D} {opt}', opt, make, feed,
           lambda Uo, Io, su, si, b, t: ts.rowwise_step(Uo, Io, su, si, b[0].repeat(k), b[1].repeat(k), b[2], t, opt=opt, lr=LR, reg_weight=REG), U, I)


@pytest.mark.parametrize('opt', ['sgd', 'adam'])
@pytest.mark.parametrize('D', WIDTHS)
def test_kmajor_point_step_widths(opt, D):
    """700 positives with two negatives each; the oracle steps on the 2,100 rows of recbole's pointwise layout (user column tiled 1 + k
    times, items [positives | k-major negatives], labels [1] * S + [0] * S k)."""
    from oracle import train_step as ts
    from recbole_cdr_amd.fused import KMajorPointStep
    S, k = 700, 2
    feed = _KMajorBatches(S, k, point=True)
    loss = 'mse' if D % 8 else 'bce'
    U, I = _tables(feed.nu, feed.ni, D)
    y = torch.cat([torch.ones(S), torch.zeros(S * k)])
    _check(f'KMajorPointStep D={D} {opt} {loss}', opt,
           lambda Ud, Id: KMajorPointStep(Ud, Id, S, k=k, loss=loss, opt=opt, lr=LR, reg_weight=REG), feed,
           lambda Uo, Io, su, si, b, t: ts.rowwise_point_step(Uo, Io, su, si, b[0].repeat(1 + k), torch.cat([b[1], b[2]]), y, t, t, opt=opt,
                                                              lr=LR, reg_weight=REG, loss=loss), U, I)
