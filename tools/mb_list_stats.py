"""The accumulation behind the non-accuracy metrics (functional.ListStats.add -> cdr_list_stats_accumulate), three arms on the same build:
  (a) ListStats.add of one batch's lists -- one native launch: a 4-byte integer atomic per entry, the column sums through LDS;
  (b) the same accumulation in torch: bincount per bucket of positions, two gathers (counts, tail flags), column sums;
  (c) the batch's own list call at D = 64, 50 history columns per user: F_.fullsort_topk (k <= 64) / F_.fullsort_topk_wide -- what the
      lists cost to produce.
1,024 users x k = 10 / 100 / 1,000 x N = 10 M items, topk = [10, k]; on random lists and on the worst case for the histogram atomics,
every user holding the same list.  HIP-event timed loops of at least MB_WINDOW_MS (100) each, median of MB_REPS (5) per arm, the arms
alternating; (a) and (b) are compared bit for bit at the timed size.  Without arguments the tool runs every k in a child process of its
own under a time limit (MB_SHAPE_SECONDS, 150), stops at the first one that fails and writes the table to MB_OUT
(profiles/mb_list_stats.txt); ``--k K`` is one such child.
  python tools/mb_list_stats.py"""
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, D = 50, 64
REPS = int(os.environ.get('MB_REPS', '5'))
WINDOW = float(os.environ.get('MB_WINDOW_MS', '100'))
U = int(os.environ.get('MB_U', '1024'))
N = int(os.environ.get('MB_N', '10000000'))
KS = [int(x) for x in os.environ.get('MB_K', '10,100,1000').split(',')]
OUT = os.environ.get('MB_OUT', os.path.join(ROOT, 'profiles', 'mb_list_stats.txt'))


def one_k(k):
    import torch
    sys.path.insert(0, ROOT)
    import recbole_cdr_amd  # noqa: F401
    from recbole_cdr_amd import functional as F_
    dev = 'cuda:0'
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def loop_ms(fn, iters):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    g = torch.Generator(device=dev); g.manual_seed(N + k + U)
    cnt = torch.randint(0, 1000, (N,), device=dev, generator=g)
    tail = torch.rand(N, device=dev, generator=g) < 0.1
    topk = sorted({10, k})
    items = torch.randn(N, D, device=dev, generator=g)
    users = torch.randn(U, D, device=dev, generator=g)
    width = (N - 2) // H
    hcols = (torch.arange(H, device=dev).unsqueeze(0) * width + torch.randint(0, width, (U, H), device=dev, generator=g) + 1).reshape(-1)
    hindptr = torch.arange(0, U * H + 1, H, device=dev, dtype=torch.int64)

    def lists():
        if k <= F_.FUSED_TOPK_MAX:
            return F_.fullsort_topk(users, items, None, k, hindptr, hcols)
        return F_.fullsort_topk_wide(users, items, None, k, hindptr, hcols)

    one = torch.randperm(N - 1, device=dev, generator=g)[:k] + 1
    cases = {'random': torch.randint(1, N, (U, k), device=dev, generator=g), 'same': one.unsqueeze(0).repeat(U, 1).contiguous()}
    for case, idx in cases.items():
        stats = F_.ListStats(cnt, topk, tail_mask=tail)
        rec = torch.zeros(len(topk), N, device=dev, dtype=torch.int64)
        pop, tl = torch.zeros(k, device=dev, dtype=torch.int64), torch.zeros(k, device=dev, dtype=torch.int64)

        def native():
            stats.add(idx)

        def in_torch():
            lo = 0
            for b, kk in enumerate(topk):
                rec[b] += torch.bincount(idx[:, lo:kk].reshape(-1), minlength=N)
                lo = kk
            pop.add_(cnt[idx].sum(0))
            tl.add_(tail[idx].sum(0))

        arms = {'native': native, 'torch': in_torch, 'lists': lists}
        iters = {}
        for name, fn in arms.items():                                    # warm-up of every arm, and the loop length
            fn()
            iters[name] = max(2, int(math.ceil(WINDOW / max(loop_ms(fn, 2), 1e-3))))
        calls = {'native': 3, 'torch': 3}
        t = {name: [] for name in arms}
        for _ in range(REPS):
            for name, fn in arms.items():
                t[name].append(loop_ms(fn, iters[name]))
                if name in calls:
                    calls[name] += iters[name]
        # both arms have accumulated calls[arm] copies of the same batch: integer sums, so they must agree exactly
        assert torch.equal(stats.rec_count.long() * calls['torch'], rec * calls['native']), 'native and torch histograms differ'
        assert torch.equal(stats.col_pop * calls['torch'], pop * calls['native']) and torch.equal(stats.col_tail * calls['torch'], tl * calls['native'])
        med = {a: statistics.median(v) for a, v in t.items()}
        sp = {a: f'[{min(v):.4f}..{max(v):.4f}]' for a, v in t.items()}
        print(f'U={U} N={N} k={k} {case} lists: (a) ListStats.add {med["native"]:.4f} ms {sp["native"]}   (b) torch bincount + gathers '
              f'{med["torch"]:.4f} ms {sp["torch"]}   (c) {"fullsort_topk" if k <= F_.FUSED_TOPK_MAX else "fullsort_topk_wide"} D={D} '
              f'{med["lists"]:.3f} ms {sp["lists"]}   (a)/(b) {med["native"] / med["torch"]:.4f}   (a)/(c) {med["native"] / med["lists"]:.5f}',
              flush=True)
        del stats, rec
        torch.cuda.empty_cache()


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--k':
        one_k(int(sys.argv[2]))
        sys.exit(0)
    limit = float(os.environ.get('MB_SHAPE_SECONDS', '150'))
    os.makedirs(os.path.dirname(OUT) or '.', exist_ok=True)
    with open(OUT, 'w') as table:
        for k in KS:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--k', str(k)], timeout=limit, stdout=subprocess.PIPE, text=True)
                rc, text = r.returncode, r.stdout
            except subprocess.TimeoutExpired as e:
                rc, text = 124, (e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout or '')
            if rc != 0:
                text += f'U={U} N={N} k={k}: exit status {rc}; stopping\n'
            sys.stdout.write(text); sys.stdout.flush()
            table.write(text); table.flush()
            if rc != 0:
                sys.exit(rc)
