"""NATR full-sort (csrc/cdr_natr_fullsort.hip behind functional.natr_history_summary), HIP-event timed after a warm-up call, median of
MB_REPS (5) runs per arm, the arms alternating; both overlap modes.
  python tools/mb_natr_fullsort.py parent [N]          (a) the model's routes against the one they replace: Trainer._predict_all_pairs (every
                                                       pair through chunked ``predict``, the parent commit's only route) at eval_batch_size
                                                       4,096 and 1 << 20; 64 users x 100,000 items, L = 50, Ds = Dt = 64
  python tools/mb_natr_fullsort.py peak [N]            (b) the scoring launch alone at 1,024 users x 1 M items, Dt = 64 and 128 (MB_D), as a
                                                       fraction of the fp32 MFMA peak at 8 Dt FLOP per pair
  python tools/mb_natr_fullsort.py topk [N ...]        (c) fused epilogue (natr_fullsort_topk: no [U, N] matrix) against natr_fullsort (writes
                                                       [U, N]) + mask + torch.topk, top-10 with a history mask, U = 64 and 1,024 (MB_U),
                                                       N = 100 k, 1 M, 10 M, Dt = 64
  python tools/mb_natr_fullsort.py summary [keys]      (d) the key-side summary alone for 1 M item keys (L = 50, Ds = Dt = 64)"""
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


def operands(key_is_item, U, N, Dt):
    """(su, key table, other table, uid, w) with random rows of the size the tests use (s^2 sqrt(Dt) = 0.8)."""
    s = (0.8 / Dt ** 0.5) ** 0.5
    n_users = 2 * U + 2
    uid = torch.arange(1, 2 * U + 1, 2, device=dev)
    items, users = torch.randn(N, Dt, device=dev) * s, torch.randn(n_users, Dt, device=dev) * s
    su = torch.randn(N if key_is_item else U, Dt, device=dev) * (0.5 * s)
    w = torch.randn(1, Dt, device=dev)
    return (su, items, users, uid, w) if key_is_item else (su, users, items, uid, w)


def peak_arms(N, U=1024):
    for Dt in DS:
        for key_is_item in (False, True):
            su, key_tab, other_tab, uid, w = operands(key_is_item, U, N, Dt)
            out = torch.empty(U, N, device=dev)
            fn = lambda: F_.natr_fullsort(key_is_item, su, key_tab, other_tab, uid, N, w, out=out)
            fn(); fn()
            torch.cuda.synchronize()
            t = [once(fn)[0] for _ in range(REPS)]
            med = statistics.median(t)
            tf = 8.0 * Dt * U * N / med / 1e9
            print(f'Dt={Dt} {"overlap_users" if key_is_item else "overlap_items"} U={U} N={N}: scoring launch {med:.2f} ms '
                  f'[{min(t):.2f}..{max(t):.2f}]   {tf:.1f} TFLOP/s at 8 Dt FLOP per pair, {tf / PEAK:.2f} of the fp32 MFMA peak', flush=True)
            del out, su, key_tab, other_tab
            torch.cuda.empty_cache()


def topk_arms(N, Dt=64):
    for key_is_item in (False, True):
        for U in US:
            su, key_tab, other_tab, uid, w = operands(key_is_item, U, N, Dt)
            cols = torch.sort(torch.randint(1, N, (U, H), device=dev), dim=1).values.reshape(-1)
            indptr = torch.arange(0, U * H + 1, H, device=dev, dtype=torch.int64)
            rows = torch.arange(U, device=dev).repeat_interleave(H)
            out = torch.empty(U, N, device=dev)
            args = (key_is_item, su, key_tab, other_tab, uid, N, w)

            def unfused():
                s = F_.natr_fullsort(*args, out=out)
                s[:, 0] = -float('inf')
                s[rows, cols] = -float('inf')
                return torch.topk(s, K, dim=1)

            def fused():
                return F_.natr_fullsort_topk(*args, K, hist_indptr=indptr, hist_cols=cols)

            for fn in (unfused, fused):
                fn()
            torch.cuda.synchronize()
            t = {'unfused': [], 'fused': []}
            for _ in range(REPS):
                ms, want = once(unfused); t['unfused'].append(ms)
                ms, got = once(fused); t['fused'].append(ms)
            assert torch.equal(got[0], want.values), 'fused values differ from the unfused route'
            med = {k: statistics.median(v) for k, v in t.items()}
            sp = {k: (min(v), max(v)) for k, v in t.items()}
            print(f'Dt={Dt} {"overlap_users" if key_is_item else "overlap_items"} U={U} N={N} k={K}: scores + mask + torch.topk '
                  f'{med["unfused"]:.2f} ms [{sp["unfused"][0]:.2f}..{sp["unfused"][1]:.2f}]   fused top-{K} {med["fused"]:.2f} ms '
                  f'[{sp["fused"][0]:.2f}..{sp["fused"][1]:.2f}]   fused / unfused {med["fused"] / med["unfused"]:.3f}', flush=True)
            del out, su, key_tab, other_tab
            torch.cuda.empty_cache()


def summary_arm(n_keys, L=50, Ds=64, Dt=64):
    g = torch.Generator().manual_seed(0)
    src = torch.randn(200_000, Ds, device=dev) * 0.5
    hist = torch.randint(1, 200_000, (n_keys, L), generator=g).to(dev)
    lens = torch.randint(0, L + 4, (n_keys,), generator=g).to(dev)
    mask = (torch.arange(L, device=dev) < lens.unsqueeze(1)).float()
    hist = hist * (mask != 0)
    tab = torch.randn(n_keys, Dt, device=dev) * 0.3
    Wt, bt = torch.randn(Dt, Ds, device=dev) * Ds ** -0.5, torch.randn(Dt, device=dev) * 0.05
    wu, wd, bu, bd = torch.randn(1, Dt, device=dev), torch.randn(1, Dt, device=dev), torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    keys = torch.arange(n_keys, device=dev)
    fn = lambda: F_.natr_history_summary(src, hist, mask, tab, keys, Wt, bt, wu, bu, wd, bd)
    fn()
    torch.cuda.synchronize()
    t = [once(fn)[0] for _ in range(REPS)]
    print(f'natr_history_summary, {n_keys} item keys, L={L} Ds={Ds} Dt={Dt}: {statistics.median(t):.2f} ms [{min(t):.2f}..{max(t):.2f}]', flush=True)


def parent_arms(N):
    import numpy as np
    from helpers import FakeDataset, base_config
    from oracle.common import IdSpace
    from recbole_cdr_amd.data.interaction import Interaction
    from recbole_cdr_amd.model.cross_domain_recommender.natr import NATR
    from recbole_cdr_amd.trainer.evaluation import Evaluation
    U, D, L = 64, 64, 50
    for mode, ids in (('overlap_items', IdSpace(OU=1, TOU=99, SOU=22, OI=N // 2, TOI=N - N // 2, SOI=16)),
                      ('overlap_users', IdSpace(OU=40, TOU=60, SOU=35, OI=1, TOI=N - 1, SOI=70))):
        torch.manual_seed(0)
        rng = np.random.RandomState(0)
        tu, ti = np.arange(1, ids.target_num_users), np.arange(1, ids.target_num_items)
        t_pairs = np.unique(np.stack([rng.choice(tu, 40 * N), rng.choice(ti, 40 * N)], 1), axis=0)
        s_pairs = np.stack([np.full(2, ids.total_num_users - 1), np.full(2, ids.total_num_items - 1)], 1)
        ds = FakeDataset(ids, s_pairs, t_pairs)
        ds.device = dev
        kw = dict(source_embedding_size=D, target_embedding_size=D, reg_weight=1e-3, max_inter_length=L)
        model = NATR(base_config(dev, native_full_sort=True, **kw), ds).to(dev)
        model.set_phase('TARGET')
        model.eval()
        assert model.mode == mode and model.target_num_items == N
        model.fullsort_topk_min_items = 0
        inter = Interaction({'target_user_id': torch.arange(1, U + 1, device=dev)})
        cols = torch.sort(torch.randint(1, N, (U, H), device=dev), dim=1).values.reshape(-1)
        indptr = torch.arange(0, U * H + 1, H, device=dev, dtype=torch.int64)
        chunked = lambda n: Evaluation(base_config(dev, eval_batch_size=n, topk=[K], **kw), model)._predict_all_pairs(inter, U)
        arms = {'predict chunks of 4,096': lambda: chunked(4096), 'predict chunks of 1 << 20': lambda: chunked(1 << 20),
                'full_sort_predict': lambda: model.full_sort_predict(inter),
                'full_sort_topk (fused)': lambda: model.full_sort_topk(inter, K, hist_indptr=indptr, hist_cols=cols)}
        med = {}
        for name, fn in arms.items():
            fn()
            torch.cuda.synchronize()
            med[name] = statistics.median(once(fn)[0] for _ in range(3))
        a, b = med['predict chunks of 4,096'], med['predict chunks of 1 << 20']
        print(f'{mode} U={U} N={N} L={L} Ds=Dt={D}: ' + '   '.join(f'{k} {v:.2f} ms' for k, v in med.items()), flush=True)
        print(f'    full_sort_predict (summary included): {a / med["full_sort_predict"]:.1f}x / {b / med["full_sort_predict"]:.1f}x faster than '
              f'the chunked routes; fused top-{K}: {a / med["full_sort_topk (fused)"]:.1f}x / {b / med["full_sort_topk (fused)"]:.1f}x', flush=True)


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'topk'
    ns = [int(x) for x in sys.argv[2:]]
    if what == 'parent':
        parent_arms(ns[0] if ns else 100_000)
    elif what == 'peak':
        peak_arms(ns[0] if ns else 1_000_000)
    elif what == 'summary':
        summary_arm(ns[0] if ns else 1_000_000)
    else:
        for n in ns or [100_000, 1_000_000, 10_000_000]:
            topk_arms(n)
