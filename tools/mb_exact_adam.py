"""rowwise_adam='exact' against the lazy row-wise Adam: steady-state times (after >= 300 steps, when every row's lag has reached the
moving window's bound) of
  (1) the catch-up launch alone (cdr_rowwise_adam_catch_up) in front of the C5 domain step,
  (2) the domain step, exact (catch-up + step) vs lazy (step), at the reference batch: 2,048 rows, k-major (KMajorBPRStep, 4 launches),
  (3) the same at the C5 shape: 1,048,576 triples (FusedBPRStep) on the C5 tables (50 M users, 20 M items, D = 128) unless smaller
      row counts are given.
The lazy leg runs the same step objects without the catch-up (the step kernels do not read `last` or the ring).
Trained-table conditions: every row's moments start nonzero (after an epoch of real training no row has zero moments, and the replay
skips a zero-moment row without arithmetic, so zero moments would time a load where training pays the replay), and every step draws a
fresh uniform batch (no row is caught up by an earlier copy of the same batch).
usage: python tools/mb_exact_adam.py [users] [items] [steps]     env CDR_ROWWISE_SWEEP: the window's period (default 256)"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import recbole_cdr_amd  # noqa: F401
from recbole_cdr_amd.fused import FusedBPRStep, KMajorBPRStep, RowwiseState, OPT_ADAM, rowwise_catch_up

nu = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_001
ni = int(sys.argv[2]) if len(sys.argv) > 2 else 20_000_001
steps = max(int(sys.argv[3]) if len(sys.argv) > 3 else 300, 300)
D = 128
dev = torch.device('cuda', 0)
g = torch.Generator(device=dev); g.manual_seed(2022)
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)


def tables(nu, ni):
    out = []
    for n in (nu, ni):
        st = RowwiseState(torch.empty(n, D, device=dev).normal_(0, 0.01, generator=g), OPT_ADAM, exact=True)
        st.exp_avg.normal_(0, 1e-4, generator=g)                                   # a trained table's moments: nonzero on every row
        st.exp_avg_sq.normal_(0, 1e-4, generator=g).square_().add_(1e-12)
        out.append(st)
    return out


def batch(nu, ni, S, k):
    half = ni // 2
    return (torch.randint(1, nu, (S,), device=dev, generator=g), torch.randint(1 + half, ni, (S,), device=dev, generator=g),
            torch.randint(1 + half, ni, (S * k,), device=dev, generator=g))


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': round(ms[len(ms) // 2], 4), 'mean_ms': round(sum(ms) / len(ms), 4), 'min_ms': round(ms[0], 4)}


def leg(step, us, its, draw, n=50):
    """Exact steps to steady state, then n timed exact steps (events: catch-up | step), then n timed lazy steps (the same step objects
    without the catch-up: last thing on these tables, since the ring is not written for them)."""
    catch = lambda b: rowwise_catch_up([(us, [b[0]]), (its, [b[1], b[2]])], **HP)
    for i in range(steps):
        b = draw()
        catch(b); step.step(*b)
    torch.cuda.synchronize()
    lag = int(us.step - int(us.last.min()))
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
    for i in range(n):
        b = draw()
        ev[i][0].record(); catch(b); ev[i][1].record(); step.step(*b); ev[i][2].record()
    torch.cuda.synchronize()
    out = {'catch_up_alone': stats([e[0].elapsed_time(e[1]) for e in ev]), 'exact_step': stats([e[0].elapsed_time(e[2]) for e in ev])}
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(n)]
    for i in range(n):
        b = draw()
        ev[i][0].record(); step.step(*b); ev[i][1].record()
    torch.cuda.synchronize()
    out['lazy_step'] = stats([e[0].elapsed_time(e[1]) for e in ev])
    out['user_rows_max_lag_at_steady_state'] = lag
    out['zero_moment_rows_in_first_1M_users'] = int((us.exp_avg[:1 << 20].abs().amax(1) == 0).sum())
    return out


res = {'warmup_steps': steps, 'D': D}
# (2) the reference batch: 2,048 rows, k = 1 (k-major; the four-launch cdr_bpr_step_small form)
us, its = tables(nu, ni)
res['sweep_period'] = us.sweep_period
S = 2048
st = KMajorBPRStep(us.table, its.table, S, k=1, reg_weight=0.01, user_state=us, item_state=its, **HP)
res['ref_batch_2048'] = dict(leg(st, us, its, lambda: batch(nu, ni, S, 1)), users=nu, items=ni)
del st, us, its
torch.cuda.synchronize()
torch.cuda.empty_cache()
# (3) the C5 shape: 1,048,576 triples, per-triple step (one call, bench.py's C5 path)
B = 1 << 20
us, its = tables(nu, ni)                                     # (fresh state: the lazy steps above left rows the ring does not cover)
st = FusedBPRStep(us.table, its.table, B, reg_weight=0.01, user_state=us, item_state=its, **HP)
res['c5_1048576'] = dict(leg(st, us, its, lambda: batch(nu, ni, B, 1)), users=nu, items=ni)
print(json.dumps(res))
