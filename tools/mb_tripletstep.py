"""SSCDR's triplet step (fused.FusedTripletStep) next to the BPR step of the same launch structure (FusedBPRStep(fuse_singles=False):
forward-grad, one sort, two segmented applies): 1,048,576 triples per step, D = 128, tables of 4 M x 1 M rows, row-wise Adam.
ms per step, per-kernel HIP-event times and algorithmic bytes/s of both."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import recbole_cdr_amd  # noqa: F401
from recbole_cdr_amd import binding as B_
from recbole_cdr_amd.fused import FusedBPRStep, FusedTripletStep

dev = torch.device('cuda', 0)
nu, ni, D, B = int(os.environ.get('NU', 4 << 20)), int(os.environ.get('NI', 1 << 20)), 128, int(os.environ.get('B', 1 << 20))
g = torch.Generator(device=dev); g.manual_seed(1)
# rows on both sides of sum x^2 = 1 (the normalisation's two branches), a margin that leaves most hinges open
mk = lambda rows: torch.randn(rows, D, device=dev, generator=g) * (0.6 / D ** 0.5) * (1 + 3 * (torch.rand(rows, 1, device=dev, generator=g) < 0.5))
bs = [(torch.randint(0, nu, (B,), device=dev, generator=g), torch.randint(0, ni, (B,), device=dev, generator=g),
       torch.randint(0, ni, (B,), device=dev, generator=g)) for _ in range(4)]
uq_u, uq_i = int(torch.unique(bs[0][0]).numel()), int(torch.unique(torch.cat(bs[0][1:])).numel())
row = 4 * D
# per step: ids + gathered rows + gradient rows written; per occurrence key + permutation + its gradient row; per distinct row the row and
# both moments read and written
applies = 3 * B * (8 + row) + (uq_u + uq_i) * 6 * row
runs = (('FusedTripletStep', lambda U, I: FusedTripletStep(U, I, B, margin=0.2, opt='adam'), 'triplet_fwd_grad_kernel', B * (24 + 6 * row)),
        ('FusedBPRStep(fuse_singles=False)', lambda U, I: FusedBPRStep(U, I, B, opt='adam', reg_weight=0.01, fuse_singles=False),
         'bpr_fwd_grad_kernel', B * (24 + 5 * row)))
for name, make, fwd, fwd_bytes in runs:
    U, I = mk(nu), mk(ni)
    st = make(U, I)
    for i in range(3): st.step(*bs[i % 4])
    B_.timing_enable(dev, 256)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(20): st.step(*bs[i % 4])
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 20 * 1e3
    tm = {}
    for k, ms in B_.timing_collect(dev): tm.setdefault(k, []).append(ms)
    B_.timing_enable(dev, 0)
    total = fwd_bytes + applies
    print(f'{name}: {dt:.3f} ms per step of {B} triples = {B / dt / 1e3:.1f} M triples/s, {total / dt / 1e9:.2f} TB/s algorithmic '
          f'({total / B:.0f} B per triple; {uq_u} + {uq_i} distinct rows)', flush=True)
    for k, v in tm.items():
        ms = sum(v) / len(v)
        extra = f'  {fwd_bytes / ms / 1e9:.2f} TB/s algorithmic' if k == fwd else ''
        print(f'  {k}: {ms:.3f} ms{extra}')
    del st, U, I
    torch.cuda.empty_cache()
