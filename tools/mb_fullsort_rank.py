"""Rank of the positives over the masked catalogue (what any topk, MAP and GAUC are computed from), four arms on the same build:
  (i)   F_.fullsort_rank -- native column passes into the workspace staging + rank_rows_kernel, no [U, N] matrix;
  (ii)  F_.fullsort_topk, k = 10 -- the evaluation a default configuration runs at the same shape: the cost (i) is read against;
  (iii) the same passes driven from Python: F_.fullsort_scores over blocks of 64 M scores + F_.rank_rows with accumulate;
  (iv)  where U x N <= MB_SORT_MAX (2^30) scores: F_.fullsort_scores + mask + torch.sort -- what GAUC costs in stock torch.
U = 64 / 1,024 x D = 64 / 128 x N = 100,000 / 1 M / 10 M items x 1 / 10 / 100 positives per user, 50 history columns per user.
HIP-event timed loops of at least MB_WINDOW_MS (100) each, median of MB_REPS (5) per arm, the arms alternating.  Without arguments the
tool runs every (U, D, N) shape in a child process of its own under a time limit (MB_SHAPE_SECONDS, 150) and stops at the first one that
fails; ``--shape U,D,N`` is one such child.
  python tools/mb_fullsort_rank.py"""
import math
import os
import statistics
import subprocess
import sys

H, K = 50, 10
REPS = int(os.environ.get('MB_REPS', '5'))
WINDOW = float(os.environ.get('MB_WINDOW_MS', '100'))
US = [int(x) for x in os.environ.get('MB_U', '64,1024').split(',')]
DS = [int(x) for x in os.environ.get('MB_D', '64,128').split(',')]
NS = [int(x) for x in os.environ.get('MB_N', '100000,1000000,10000000').split(',')]
PS = [int(x) for x in os.environ.get('MB_P', '1,10,100').split(',')]
SORT_MAX = int(os.environ.get('MB_SORT_MAX', str(1 << 30)))
PASS_SCORES = 64 << 20


def spread(U, N, per_user, dev, g, phase):
    """per user ``per_user`` distinct ascending columns in [1, N): one random pick inside each of per_user equal bins (``phase`` keeps the
    history and the positives of a user apart: odd and even columns)"""
    import torch
    width = (N - 2) // (2 * per_user)
    base = torch.arange(per_user, device=dev).unsqueeze(0) * width
    pick = torch.randint(0, width, (U, per_user), device=dev, generator=g)
    return (2 * (base + pick) + 1 + phase).reshape(-1).contiguous()


def one_shape(U, D, N):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import recbole_cdr_amd  # noqa: F401
    from recbole_cdr_amd import functional as F_
    dev = 'cuda:0'
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def loop_ms(fn, iters):
        e0.record()
        for _ in range(iters):
            r = fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters, r

    g = torch.Generator(device=dev); g.manual_seed(N + D + U)
    items = torch.randn(N, D, device=dev, generator=g)
    users = torch.randn(U, D, device=dev, generator=g)
    hcols = spread(U, N, H, dev, g, 0)
    hindptr = torch.arange(0, U * H + 1, H, device=dev, dtype=torch.int64)
    hrows = torch.arange(U, device=dev).repeat_interleave(H)
    for P in PS:
        pcols = spread(U, N, P, dev, g, 1)
        pindptr = torch.arange(0, U * P + 1, P, device=dev, dtype=torch.int64)
        prows = torch.arange(U, device=dev).repeat_interleave(P)

        def rank():
            return F_.fullsort_rank(users, items, None, pindptr, pcols, hindptr, hcols)

        def topk():
            return F_.fullsort_topk(users, items, None, k=K, hist_indptr=hindptr, hist_cols=hcols)

        def passes():
            step = max(PASS_SCORES // U // 64 * 64, 64)
            score = torch.empty(U * P, device=dev)
            blocks = []
            for c in range(0, N, step):                                   # thresholds first, as the native entry: one walk for them ...
                s = F_.fullsort_scores(users, items[c:c + step])
                inside = (pcols >= c) & (pcols < c + s.shape[1])
                score[inside] = s[prows[inside], pcols[inside] - c]
                blocks.append(c)
                if N > step:
                    del s
            out = None
            for c in blocks:                                             # ... and one for the counts (a single block is scored once)
                if N > step:
                    s = F_.fullsort_scores(users, items[c:c + step])
                r = F_.rank_rows(s, pindptr, pcols, hindptr, hcols, pos_score=score, col_off=c, out=out, accumulate=out is not None)
                out = r[1:]
            return r

        def sort():
            s = F_.fullsort_scores(users, items)
            s[:, 0] = -float('inf')
            s[hrows, hcols] = -float('inf')
            return torch.sort(s, dim=1, descending=True)

        arms = {'rank': rank, 'topk': topk, 'passes': passes}
        if U * N <= SORT_MAX:
            arms['sort'] = sort
        iters = {}
        for name, fn in arms.items():                                    # warm-up of every shape that is timed, and the loop length
            fn()
            ms, _ = loop_ms(fn, 2)
            iters[name] = max(2, int(math.ceil(WINDOW / max(ms, 1e-3))))
        t = {name: [] for name in arms}
        res = {}
        for _ in range(REPS):
            for name, fn in arms.items():
                ms, r = loop_ms(fn, iters[name])
                t[name].append(ms)
                if name in ('rank', 'passes'):
                    res[name] = r
        for a, b in zip(res['rank'], res['passes']):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'the native passes and the Python passes disagree'
        del res
        med = {k: statistics.median(v) for k, v in t.items()}
        sp = {k: f'[{min(v):.3f}..{max(v):.3f}]' for k, v in t.items()}
        line = (f'U={U} D={D} N={N} P={P}: (i) fullsort_rank {med["rank"]:.3f} ms {sp["rank"]}   (ii) fullsort_topk k={K} {med["topk"]:.3f} ms '
                f'{sp["topk"]}   (iii) scores + rank_rows passes {med["passes"]:.3f} ms {sp["passes"]}   ')
        if 'sort' in med:
            line += f'(iv) scores + mask + torch.sort {med["sort"]:.3f} ms {sp["sort"]}   '
        line += f'(i)/(ii) {med["rank"] / med["topk"]:.2f}   (i)/(iii) {med["rank"] / med["passes"]:.2f}'
        if 'sort' in med:
            line += f'   (i)/(iv) {med["rank"] / med["sort"]:.3f}'
        print(line, flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--shape':
        one_shape(*(int(x) for x in sys.argv[2].split(',')))
        sys.exit(0)
    limit = float(os.environ.get('MB_SHAPE_SECONDS', '150'))
    for D in DS:
        for N in NS:
            for U in US:
                try:
                    rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--shape', f'{U},{D},{N}'], timeout=limit).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:
                    print(f'U={U} D={D} N={N}: exit status {rc}; stopping', flush=True)
                    sys.exit(rc)
