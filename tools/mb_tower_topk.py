"""MLP-tower full-sort, top-10 with a history mask: the fused epilogue (conet_fullsort_topk: no [U, N] matrix) against the route it
replaces on the same build -- conet_fullsort (writes [U, N]) + mask + torch.topk.  CoNet's default tower [2D -> 64 -> 32 -> 16 -> 8] -> 1 and
DTCDR's [2D -> 32 -> 16] -> 1 at U = 64 / 256 / 1,024 x N = 1 M, HIP-event timed, median of MB_REPS (7) runs per arm, the arms alternating.
  python tools/mb_tower_topk.py [N]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recbole_cdr_amd  # noqa: F401,E402
from recbole_cdr_amd import functional as F_  # noqa: E402

dev = 'cuda:0'
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
D, H, K = 64, 50, 10
REPS = int(os.environ.get('MB_REPS', '7'))
US = [int(x) for x in os.environ.get('MB_U', '64,256,1024').split(',')]
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def once(fn):
    e0.record()
    r = fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


for name, layers in (('CoNet [64,32,16,8]', [64, 32, 16, 8]), ('DTCDR [32,16]', [32, 16])):
    g = torch.Generator().manual_seed(0)
    dims = [2 * D] + layers
    Ws = [(torch.randn(b, a, generator=g) * (2.0 / (a + b)) ** 0.5).to(dev) for a, b in zip(dims[:-1], dims[1:])]
    bs = [(torch.randn(b, generator=g) * 0.1).to(dev) for b in dims[1:]]
    wo, bo = (torch.randn(1, dims[-1], generator=g) * 0.5).to(dev), (torch.randn(1, generator=g) * 0.1).to(dev)
    items = torch.randn(N, D, device=dev) * 0.3
    P = F_.gemm(items, Ws[0][:, D:], trans_b=True)
    flop_pair = 2 * sum(a * b for a, b in zip(layers[:-1], layers[1:])) + 2 * layers[-1]
    for U in US:
        users = torch.randn(U, D, device=dev) * 0.3
        Q = F_.gemm(users, Ws[0][:, :D], trans_b=True, bias=bs[0])
        cols = torch.sort(torch.randint(1, N, (U, H), device=dev), dim=1).values.reshape(-1)      # 50 history items per user, ascending
        indptr = torch.arange(0, U * H + 1, H, device=dev, dtype=torch.int64)
        rows = torch.arange(U, device=dev).repeat_interleave(H)
        out = torch.empty(U, N, device=dev)

        def unfused():
            s = F_.conet_fullsort(P, Q, Ws[1:], bs[1:], wo, bo, out=out)
            s[:, 0] = -float('inf')
            s[rows, cols] = -float('inf')
            return torch.topk(s, K, dim=1)

        def scores_only():
            return F_.conet_fullsort(P, Q, Ws[1:], bs[1:], wo, bo, out=out)

        def fused():
            return F_.conet_fullsort_topk(P, Q, Ws[1:], bs[1:], wo, bo, K, hist_indptr=indptr, hist_cols=cols)

        for fn in (unfused, scores_only, fused):                         # warm-up of every shape that is timed
            fn()
        torch.cuda.synchronize()
        t = {'unfused': [], 'scores': [], 'fused': []}
        for _ in range(REPS):
            ms, want = once(unfused); t['unfused'].append(ms)
            ms, _ = once(scores_only); t['scores'].append(ms)
            ms, got = once(fused); t['fused'].append(ms)
        assert torch.equal(got[0], want.values), 'fused values differ from the unfused route'
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = {k: (min(v), max(v)) for k, v in t.items()}
        tf = lambda ms: U * N * flop_pair / ms / 1e9
        print(f'{name} U={U} N={N} k={K}: scores only {med["scores"]:.2f} ms ({tf(med["scores"]):.1f} TFLOP/s)   '
              f'scores + mask + torch.topk {med["unfused"]:.2f} ms [{spread["unfused"][0]:.2f}..{spread["unfused"][1]:.2f}]   '
              f'fused top-{K} {med["fused"]:.2f} ms [{spread["fused"][0]:.2f}..{spread["fused"][1]:.2f}] ({tf(med["fused"]):.1f} TFLOP/s)   '
              f'fused / unfused {med["fused"] / med["unfused"]:.3f}', flush=True)
        del out
        torch.cuda.empty_cache()
