"""DeepAPF full-sort (csrc/cdr_deepapf_fullsort.hip), top-10 with a history mask, HIP-event timed, median of MB_REPS (5) runs per arm, the
arms alternating.  Both overlap modes at D = 64 and 128 (MB_D), half of the keys masked.
  python tools/mb_deepapf_fullsort.py topk [N ...]     fused epilogue (deepapf_fullsort_topk: no [U, N] matrix) against deepapf_fullsort
                                                       (writes [U, N]) + mask + torch.topk, U = 64 and 1,024 (MB_U); FLOP rate of the
                                                       scoring launch at 4 D^2 FLOP per pair (unmasked pairs: both candidates)
  python tools/mb_deepapf_fullsort.py parent [N]       the model's routes against the one they replace: Trainer._predict_all_pairs (every
                                                       pair through chunked ``predict``) at eval_batch_size 4,096 and 1 << 20, U = 64,
                                                       N = 100,000, D = 64"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import recbole_cdr_amd  # noqa: F401,E402
from recbole_cdr_amd import functional as F_  # noqa: E402

dev = 'cuda:0'
K, H = 10, 50
REPS = int(os.environ.get('MB_REPS', '5'))
US = [int(x) for x in os.environ.get('MB_U', '64,1024').split(',')]
DS = [int(x) for x in os.environ.get('MB_D', '64,128').split(',')]
PEAK = 157.3                                                             # fp32 MFMA TFLOP/s
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def once(fn):
    e0.record()
    r = fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def topk_arms(N):
    for D in DS:
        g = torch.Generator().manual_seed(0)
        W1 = (torch.randn(D, D, generator=g) * (2.0 / (2 * D)) ** 0.5).to(dev)
        b1 = (torch.randn(D, generator=g) * 0.1).to(dev)
        w2, wp = (torch.randn(1, D, generator=g) * 0.5).to(dev), (torch.randn(1, D, generator=g) * 0.5).to(dev)
        for key_is_item in (False, True):
            for U in US:
                n_users = 2 * U + 2
                it = [torch.randn(N, D, device=dev) * 0.3 for _ in range(2 if key_is_item else 1)]
                us = [torch.randn(n_users, D, device=dev) * 0.3 for _ in range(1 if key_is_item else 2)]
                share, only, other = (it[0], it[1], us[0]) if key_is_item else (us[0], us[1], it[0])
                uid = torch.arange(1, 2 * U + 1, 2, device=dev)                          # every second id: half of them <= n_overlap
                n_over = N // 2 if key_is_item else U
                cols = torch.sort(torch.randint(1, N, (U, H), device=dev), dim=1).values.reshape(-1)
                indptr = torch.arange(0, U * H + 1, H, device=dev, dtype=torch.int64)
                rows = torch.arange(U, device=dev).repeat_interleave(H)
                out = torch.empty(U, N, device=dev)
                args = (key_is_item, share, only, other, uid, N, n_over, W1, b1, w2, wp)

                def unfused():
                    s = F_.deepapf_fullsort(*args, out=out)
                    s[:, 0] = -float('inf')
                    s[rows, cols] = -float('inf')
                    return torch.topk(s, K, dim=1)

                def scores_only():
                    return F_.deepapf_fullsort(*args, out=out)

                def fused():
                    return F_.deepapf_fullsort_topk(*args, K, hist_indptr=indptr, hist_cols=cols)

                for fn in (unfused, scores_only, fused):
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
                flop = 0.75 * U * N * 4 * D * D                                          # half of the pairs run one candidate
                tf = lambda ms: flop / ms / 1e9
                print(f'D={D} {"overlap_items" if key_is_item else "overlap_users"} U={U} N={N} k={K}: scores only {med["scores"]:.2f} ms '
                      f'({tf(med["scores"]):.1f} TFLOP/s executed, {tf(med["scores"]) / PEAK:.2f} of peak)   scores + mask + torch.topk '
                      f'{med["unfused"]:.2f} ms [{spread["unfused"][0]:.2f}..{spread["unfused"][1]:.2f}]   fused top-{K} {med["fused"]:.2f} ms '
                      f'[{spread["fused"][0]:.2f}..{spread["fused"][1]:.2f}]   fused / unfused {med["fused"] / med["unfused"]:.3f}', flush=True)
                del out, it, us, share, only, other
                torch.cuda.empty_cache()


def parent_arms(N):
    from helpers import FakeDataset, base_config
    from oracle.common import IdSpace
    from recbole_cdr_amd.data.interaction import Interaction
    from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
    from recbole_cdr_amd.trainer.evaluation import Evaluation
    U, D = 64, 64
    for mode, ids in (('overlap_users', IdSpace(OU=40, TOU=60, SOU=35, OI=1, TOI=N - 1, SOI=70)),
                      ('overlap_items', IdSpace(OU=1, TOU=99, SOU=22, OI=N // 2, TOI=N - N // 2, SOI=16))):
        torch.manual_seed(0)
        model = DeepAPF(base_config(dev, embedding_size=D, beta=0.5, native_full_sort=True), FakeDataset(ids)).to(dev)
        model.eval()
        assert model.mode == mode and model.target_num_items == N
        model.fullsort_topk_min_items = 0
        inter = Interaction({'target_user_id': torch.arange(1, U + 1, device=dev)})
        cols = torch.sort(torch.randint(1, N, (U, H), device=dev), dim=1).values.reshape(-1)
        indptr = torch.arange(0, U * H + 1, H, device=dev, dtype=torch.int64)
        chunked = lambda n: Evaluation(base_config(dev, embedding_size=D, beta=0.5, eval_batch_size=n, topk=[K]), model)._predict_all_pairs(inter, U)
        arms = {'predict chunks of 4,096': lambda: chunked(4096), 'predict chunks of 1 << 20': lambda: chunked(1 << 20),
                'full_sort_predict': lambda: model.full_sort_predict(inter),
                'full_sort_topk (fused)': lambda: model.full_sort_topk(inter, K, hist_indptr=indptr, hist_cols=cols)}
        med = {}
        for name, fn in arms.items():
            fn()
            torch.cuda.synchronize()
            med[name] = statistics.median(once(fn)[0] for _ in range(3))
        a, b = med['predict chunks of 4,096'], med['predict chunks of 1 << 20']
        print(f'{mode} U={U} N={N} D={D}: ' + '   '.join(f'{k} {v:.2f} ms' for k, v in med.items()), flush=True)
        print(f'    full_sort_predict: {a / med["full_sort_predict"]:.1f}x / {b / med["full_sort_predict"]:.1f}x faster than the chunked routes; '
              f'fused top-{K}: {a / med["full_sort_topk (fused)"]:.1f}x / {b / med["full_sort_topk (fused)"]:.1f}x', flush=True)


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'topk'
    ns = [int(x) for x in sys.argv[2:]]
    if what == 'parent':
        parent_arms(ns[0] if ns else 100_000)
    else:
        for n in ns or [81_920, 250_000, 1_000_000]:
            topk_arms(n)
