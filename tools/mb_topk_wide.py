"""Mask + top-k lists beyond 64 entries (k = 100 / 1,000), three arms on the same build:
  (i)   F_.fullsort_topk_wide -- native column passes into the workspace staging + the wide selection (csrc/cdr_topk_wide.h), ONE scoring
        walk, no [U, N] matrix;
  (ii)  where U x N <= MB_MATRIX_MAX (2^30) scores: F_.fullsort_scores + mask + torch.topk -- the route below the catalogue thresholds, and
        what stock torch costs;
  (iii) F_.fullsort_rank with 10 positives per user at the same shape -- the route that answers the accuracy metrics at these k without a
        list: TWO scoring walks.
U = 64 / 1,024 x D = 64 / 128 x N = 81,920 / 1 M / 10 M items x k = 100 / 1,000, 50 history columns per user.  HIP-event timed loops of at
least MB_WINDOW_MS (100) each, median of MB_REPS (5) per arm, the arms alternating; the values of (i) and (ii) are compared bit for bit at
the timed size.  Without arguments the tool runs every (U, D, N) shape in a child process of its own under a time limit (MB_SHAPE_SECONDS,
150), stops at the first one that fails and writes the table to MB_OUT (profiles/mb_topk_wide.txt); ``--shape U,D,N`` is one such child.
  python tools/mb_topk_wide.py"""
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, P = 50, 10
REPS = int(os.environ.get('MB_REPS', '5'))
WINDOW = float(os.environ.get('MB_WINDOW_MS', '100'))
US = [int(x) for x in os.environ.get('MB_U', '64,1024').split(',')]
DS = [int(x) for x in os.environ.get('MB_D', '64,128').split(',')]
NS = [int(x) for x in os.environ.get('MB_N', '81920,1000000,10000000').split(',')]
KS = [int(x) for x in os.environ.get('MB_K', '100,1000').split(',')]
MATRIX_MAX = int(os.environ.get('MB_MATRIX_MAX', str(1 << 30)))
OUT = os.environ.get('MB_OUT', os.path.join(ROOT, 'profiles', 'mb_topk_wide.txt'))


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
    sys.path.insert(0, ROOT)
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
    pcols = spread(U, N, P, dev, g, 1)
    pindptr = torch.arange(0, U * P + 1, P, device=dev, dtype=torch.int64)
    for k in KS:
        def wide():
            return F_.fullsort_topk_wide(users, items, None, k, hindptr, hcols)

        def matrix():
            s = F_.fullsort_scores(users, items)
            s[:, 0] = -float('inf')
            s[hrows, hcols] = -float('inf')
            return torch.topk(s, k, dim=1)

        def rank():
            return F_.fullsort_rank(users, items, None, pindptr, pcols, hindptr, hcols)

        arms = {'wide': wide, 'rank': rank}
        if U * N <= MATRIX_MAX:
            arms['matrix'] = matrix
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
                res[name] = r
        if 'matrix' in res:
            assert torch.equal(res['wide'][0].view(torch.int32), res['matrix'][0].view(torch.int32)), 'the two routes list different values'
        del res
        med = {a: statistics.median(v) for a, v in t.items()}
        sp = {a: f'[{min(v):.3f}..{max(v):.3f}]' for a, v in t.items()}
        line = f'U={U} D={D} N={N} k={k}: (i) fullsort_topk_wide {med["wide"]:.3f} ms {sp["wide"]}   '
        if 'matrix' in med:
            line += f'(ii) scores + mask + torch.topk {med["matrix"]:.3f} ms {sp["matrix"]}   '
        line += f'(iii) fullsort_rank P={P} {med["rank"]:.3f} ms {sp["rank"]}   '
        if 'matrix' in med:
            line += f'(i)/(ii) {med["wide"] / med["matrix"]:.3f}   '
        line += f'(i)/(iii) {med["wide"] / med["rank"]:.2f}'
        print(line, flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--shape':
        one_shape(*(int(x) for x in sys.argv[2].split(',')))
        sys.exit(0)
    limit = float(os.environ.get('MB_SHAPE_SECONDS', '150'))
    os.makedirs(os.path.dirname(OUT) or '.', exist_ok=True)
    with open(OUT, 'w') as table:
        for D in DS:
            for N in NS:
                for U in US:
                    try:
                        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--shape', f'{U},{D},{N}'], timeout=limit,
                                           stdout=subprocess.PIPE, text=True)
                        rc, text = r.returncode, r.stdout
                    except subprocess.TimeoutExpired as e:
                        rc, text = 124, (e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout or '')
                    if rc != 0:
                        text += f'U={U} D={D} N={N}: exit status {rc}; stopping\n'
                    sys.stdout.write(text); sys.stdout.flush()
                    table.write(text); table.flush()
                    if rc != 0:
                        sys.exit(rc)
