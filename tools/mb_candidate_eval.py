"""Sampled-candidate evaluation (eval_args mode uniN / popN) of one batch of users, the routes on the SAME candidate lists:
  (i)    native: F_.candidate_scores + F_.candidate_rank -- two launches, one item row per candidate, no pairs, no [U, N] matrix;
  (ii)   the default route: the list expanded to (user, item) pairs, ``predict`` (EMCDR's TARGET-phase pair kernel: two row gathers and a
         dot) over all pairs in ONE call, + F_.candidate_rank;
  (iii)  the same in chunks of eval_batch_size = 4,096 pairs (what ``CrossDomainRecommender.candidate_scores`` does by default);
  (iv)   the reference's formulation: the pair scores of (ii) scattered into a [U, N] matrix of -inf + torch.topk(k = 10), where U x N <=
         MB_SCATTER_MAX (2^31) entries;
  (v/vi) the OVERLAP phase's mapping in front (one D x D linear layer): per user in front of (i), per pair in front of (ii).
U = 1,024 users x 10 positives x 100 negatives each (about 1.03 M candidates), D = 64 / 128, N = 100 K / 1 M / 10 M items.
MB_NT_LIB=<a libcdrhip.so built with -DCDR_CAND_NT> adds the scoring launch alone, plain against non-temporal item-row loads, alternating.
HIP-event timed loops of at least MB_WINDOW_MS (100) each after a warm-up of every arm, median of MB_REPS (5), the arms alternating.
Without arguments every (D, N) shape runs in a child process of its own under a time limit (MB_SHAPE_SECONDS, 170); the first failure stops
the tool.
  python tools/mb_candidate_eval.py"""
import ctypes
import math
import os
import statistics
import subprocess
import sys

U, P, NEG, K, CHUNK = 1024, 10, 100, 10, 4096
REPS = int(os.environ.get('MB_REPS', '5'))
WINDOW = float(os.environ.get('MB_WINDOW_MS', '100'))
DS = [int(x) for x in os.environ.get('MB_D', '64,128').split(',')]
NS = [int(x) for x in os.environ.get('MB_N', '100000,1000000,10000000').split(',')]
SCATTER_MAX = int(os.environ.get('MB_SCATTER_MAX', str(1 << 31)))
NT_LIB = os.environ.get('MB_NT_LIB')


def one_shape(D, N):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import recbole_cdr_amd  # noqa: F401
    from recbole_cdr_amd import binding as B_, functional as F_
    dev = 'cuda:0'
    torch.set_grad_enabled(False)                                        # (as the models' predict: no autograd bookkeeping)
    e0, e1 =torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def loop_ms(fn, iters):
        e0.record()
        for _ in range(iters):
            r = fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters, r

    g = torch.Generator(device=dev); g.manual_seed(N + D)
    items = torch.randn(N, D, device=dev, generator=g) * 0.1
    users = torch.randn(U, D, device=dev, generator=g) * 0.1
    uids = torch.arange(U, device=dev)
    W = torch.randn(D, D, device=dev, generator=g) * 0.1
    # per user P positives and P * NEG uniform negatives in [1, N): distinct, ascending (one sort of user * N + item keys, as the loader's)
    draw = torch.randint(1, N, (U, P * (1 + NEG)), device=dev, generator=g)
    key = torch.unique(torch.arange(U, device=dev).unsqueeze(1) * N + draw)
    cand_cols = (key % N).contiguous()
    cand_indptr = torch.zeros(U + 1, device=dev, dtype=torch.int64)
    cand_indptr[1:] = torch.cumsum(torch.bincount(key // N, minlength=U), 0)
    C = cand_cols.numel()
    cand_row = torch.repeat_interleave(torch.arange(U, device=dev), cand_indptr[1:] - cand_indptr[:-1], output_size=C)
    pkey = torch.unique(torch.arange(U, device=dev).unsqueeze(1) * N + draw[:, :P])          # the first P draws of a user are its positives
    pos_cols = (pkey % N).contiguous()
    pos_indptr = torch.zeros(U + 1, device=dev, dtype=torch.int64)
    pos_indptr[1:] = torch.cumsum(torch.bincount(pkey // N, minlength=U), 0)
    zeros = torch.zeros(C, device=dev)

    def pair_scores(utab, rows, cols):
        return F_.PointGatherLoss.apply(B_.CDR_LOSS_MSE, utab, items, None, None, rows, cols, zeros[:rows.numel()], 0.0)[1]

    def native():
        return F_.candidate_rank(cand_indptr, cand_cols, F_.candidate_scores(users, items, None, cand_indptr, cand_cols), pos_indptr, pos_cols)

    def pairs():
        rows = torch.repeat_interleave(uids, cand_indptr[1:] - cand_indptr[:-1], output_size=C)
        return F_.candidate_rank(cand_indptr, cand_cols, pair_scores(users, rows, cand_cols), pos_indptr, pos_cols)

    def pairs_chunked():
        rows = torch.repeat_interleave(uids, cand_indptr[1:] - cand_indptr[:-1], output_size=C)
        s = torch.cat([pair_scores(users, rows[c:c + CHUNK], cand_cols[c:c + CHUNK]) for c in range(0, C, CHUNK)])
        return F_.candidate_rank(cand_indptr, cand_cols, s, pos_indptr, pos_cols)

    def scatter_topk():
        rows = torch.repeat_interleave(uids, cand_indptr[1:] - cand_indptr[:-1], output_size=C)
        full = torch.full((U, N), -float('inf'), device=dev)
        full[rows, cand_cols] = pair_scores(users, rows, cand_cols)
        return torch.topk(full, K, dim=1)

    def native_mapped():
        mapped = F_.linear(users, W, None, B_.ACT_NONE)
        return F_.candidate_rank(cand_indptr, cand_cols, F_.candidate_scores(mapped, items, None, cand_indptr, cand_cols), pos_indptr, pos_cols)

    def pairs_mapped():
        rows = torch.repeat_interleave(uids, cand_indptr[1:] - cand_indptr[:-1], output_size=C)
        mapped = F_.linear(F_.gather_rows(users, rows), W, None, B_.ACT_NONE)
        s = F_.PointGatherLoss.apply(B_.CDR_LOSS_MSE, mapped, items, None, None, torch.arange(C, device=dev), cand_cols, zeros, 0.0)[1]
        return F_.candidate_rank(cand_indptr, cand_cols, s, pos_indptr, pos_cols)

    arms = {'native': native, 'pairs': pairs, 'pairs4096': pairs_chunked, 'native+map': native_mapped, 'pairs+map': pairs_mapped}
    if U * N <= SCATTER_MAX:
        arms['scatter+topk'] = scatter_topk
    if NT_LIB:
        out = torch.empty(C, device=dev)
        sig = B_._SIGNATURES['cdr_candidate_scores_f32']
        libs = {'scores': B_.load(), 'scores_nt': ctypes.CDLL(NT_LIB)}
        for lib in libs.values():
            lib.cdr_candidate_scores_f32.argtypes, lib.cdr_candidate_scores_f32.restype = sig, ctypes.c_int

        def scores_of(lib):
            def fn():
                rc = lib.cdr_candidate_scores_f32(B_.stream(), users.data_ptr(), U, D, items.data_ptr(), N, None, 0, cand_row.data_ptr(),
                                                  cand_cols.data_ptr(), C, 0, out.data_ptr())
                assert rc == 0
                return out
            return fn
        arms.update({name: scores_of(lib) for name, lib in libs.items()})

    iters = {}
    for name, fn in arms.items():                                        # warm-up of every arm, and the loop length
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
    for name in ('pairs', 'pairs4096'):                                  # the same positives at the same ranks, up to reordered fp32 sums
        same = (res['native'][1] == res[name][1]).float().mean()
        assert float(same) > 0.99, (name, float(same))
    med = {k: statistics.median(v) for k, v in t.items()}
    line = f'D={D} N={N} U={U} C={C}:'
    for name in arms:
        line += f'   {name} {med[name]:.3f} ms [{min(t[name]):.3f}..{max(t[name]):.3f}]'
    line += f'   pairs/native {med["pairs"] / med["native"]:.2f}   pairs4096/native {med["pairs4096"] / med["native"]:.1f}'
    line += f'   (pairs+map)/(native+map) {med["pairs+map"] / med["native+map"]:.2f}'
    if 'scatter+topk' in med:
        line += f'   (scatter+topk)/native {med["scatter+topk"] / med["native"]:.1f}'
    if NT_LIB:
        line += f'   scores_nt/scores {med["scores_nt"] / med["scores"]:.3f}'
    print(line, flush=True)


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--shape':
        one_shape(*(int(x) for x in sys.argv[2].split(',')))
        sys.exit(0)
    limit = float(os.environ.get('MB_SHAPE_SECONDS', '170'))
    for D in DS:
        for N in NS:
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--shape', f'{D},{N}'], timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f'D={D} N={N}: exit status {rc}; stopping', flush=True)
                sys.exit(rc)
