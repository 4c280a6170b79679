"""SSCDR's distance full-sort, top-10 with a history mask: the fused form (fullsort_neg_sqdist_topk: no [U, N] matrix, no cat) against the
route it replaces on the same build -- fullsort_neg_sqdist (writes [U, N]) + mask + torch.topk.  U = 64 / 1,024 x D = 64 / 128 x
N = 20,000 / 81,920 / 250,000 / 1,052,673 items.  The normalised table is prepared outside the timed region in both arms.  The norms: the
unfused entry forms both vectors on every call (no entry takes them), so the fused form is timed twice -- with ``col_sqnorm=None`` (its
norms per call as well: like for like, the ratio the threshold is set from) and with the column norms prepared outside (what SSCDR's
evaluation bracket runs).  HIP-event timed loops of at least MB_WINDOW_MS (200) each, median of MB_REPS (5) per arm, the arms alternating.
  python tools/mb_sqdist_topk.py"""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recbole_cdr_amd  # noqa: F401,E402
from recbole_cdr_amd import functional as F_  # noqa: E402

dev = 'cuda:0'
H, K = 50, 10
REPS = int(os.environ.get('MB_REPS', '5'))
WINDOW = float(os.environ.get('MB_WINDOW_MS', '200'))
US = [int(x) for x in os.environ.get('MB_U', '64,1024').split(',')]
DS = [int(x) for x in os.environ.get('MB_D', '64,128').split(',')]
NS = [int(x) for x in os.environ.get('MB_N', '20000,81920,250000,1052673').split(',')]
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def loop_ms(fn, iters):
    e0.record()
    for _ in range(iters):
        r = fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, r


for D in DS:
    for N in NS:
        g = torch.Generator(device=dev); g.manual_seed(N + D)
        items = F_.sqnorm_normalize(torch.randn(N, D, device=dev, generator=g))
        col_sq = F_.row_sqnorm(items)
        for U in US:
            users = F_.sqnorm_normalize(torch.randn(U, D, device=dev, generator=g))
            cols = torch.sort(torch.randint(1, N, (U, H), device=dev, generator=g), dim=1).values.reshape(-1)   # 50 history items per user
            indptr = torch.arange(0, U * H + 1, H, device=dev, dtype=torch.int64)
            rows = torch.arange(U, device=dev).repeat_interleave(H)

            def unfused():
                s = F_.fullsort_neg_sqdist(users, items)
                s[:, 0] = -float('inf')
                s[rows, cols] = -float('inf')
                return torch.topk(s, K, dim=1)

            def fused():
                return F_.fullsort_neg_sqdist_topk(users, items, None, k=K, hist_indptr=indptr, hist_cols=cols)

            def fused_cached():
                return F_.fullsort_neg_sqdist_topk(users, items, None, k=K, hist_indptr=indptr, hist_cols=cols, col_sqnorm=col_sq)

            arms = {'unfused': unfused, 'fused': fused, 'fused_cached': fused_cached}
            iters = {}
            for name, fn in arms.items():                        # warm-up of every shape that is timed, and the loop length
                fn()
                ms, _ = loop_ms(fn, 3)
                iters[name] = max(3, int(math.ceil(WINDOW / max(ms, 1e-3))))
            t = {name: [] for name in arms}
            res = {}
            for _ in range(REPS):
                for name, fn in arms.items():
                    ms, res[name] = loop_ms(fn, iters[name])
                    t[name].append(ms)
            assert torch.equal(res['fused'][0], res['unfused'].values), 'fused values differ from the unfused route'
            assert torch.equal(res['fused_cached'][0], res['unfused'].values) and torch.equal(res['fused_cached'][1], res['fused'][1])
            med = {k: statistics.median(v) for k, v in t.items()}
            sp = {k: (min(v), max(v)) for k, v in t.items()}
            tf = lambda ms: 2.0 * U * N * D / ms / 1e9
            print(f'U={U} D={D} N={N} k={K}: scores + mask + torch.topk {med["unfused"]:.3f} ms [{sp["unfused"][0]:.3f}..{sp["unfused"][1]:.3f}]   '
                  f'fused {med["fused"]:.3f} ms [{sp["fused"][0]:.3f}..{sp["fused"][1]:.3f}] ({tf(med["fused"]):.1f} TFLOP/s)   '
                  f'fused, column norms kept {med["fused_cached"]:.3f} ms [{sp["fused_cached"][0]:.3f}..{sp["fused_cached"][1]:.3f}]   '
                  f'fused / unfused {med["fused"] / med["unfused"]:.3f}   kept / unfused {med["fused_cached"] / med["unfused"]:.3f}', flush=True)
            torch.cuda.empty_cache()
        del items, col_sq
