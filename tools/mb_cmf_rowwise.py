"""CMF's row-wise BOTH-phase step (FusedPointPairStep: cdr_point_step_fused_pair_dev) -- device-event medians after warm-up of
  (a) the reference batch: 2,048 + 2,048 rows on C1-sized shared tables (6,984 users x 3,945 items, D = 64), replayed as a hipGraph,
  (b) 1,048,576 + 1,048,576 rows at D = 128 on shared tables of 50 M users x 20 M items (~107 GB with the moments) unless smaller row
      counts are given,
  (c) for (b): lazy against exact (rowwise_catch_up in front of the step), and the joint step against two back-to-back FusedPointStep
      calls on the same two batches -- NOT the same optimizer (a row in both batches gets two updates there), but the byte-for-byte yardstick.
Trained-table conditions as in tools/mb_exact_adam.py: nonzero moments on every row, a fresh uniform batch every step.
usage: python tools/mb_cmf_rowwise.py [users] [items] [rows_per_domain] [steps]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import recbole_cdr_amd  # noqa: F401
from recbole_cdr_amd import binding as B_
from recbole_cdr_amd.fused import FusedPointPairStep, FusedPointStep, RowwiseState, OPT_ADAM, rowwise_catch_up

nu = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_001
ni = int(sys.argv[2]) if len(sys.argv) > 2 else 20_000_001
BB = int(sys.argv[3]) if len(sys.argv) > 3 else 1 << 20
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 300
dev = torch.device('cuda', 0)
g = torch.Generator(device=dev); g.manual_seed(2022)
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
ALPHA, LAM, GAM = 0.5, 0.0, 0.0                              # CMF's defaults (properties/model/CMF.yaml): no EmbLoss


def tables(nu, ni, D, exact):
    out = []
    for n in (nu, ni):
        st = RowwiseState(torch.empty(n, D, device=dev).normal_(0, 0.01, generator=g), OPT_ADAM, exact=exact)
        st.exp_avg.normal_(0, 1e-4, generator=g)
        st.exp_avg_sq.normal_(0, 1e-4, generator=g).square_().add_(1e-12)
        out.append(st)
    return out


def batch(nu, ni, B):
    r = lambda hi: torch.randint(0, hi, (B,), device=dev, generator=g)
    return r(nu), r(ni), (torch.rand(B, device=dev, generator=g) < 0.5).float(), r(nu), r(ni), (torch.rand(B, device=dev, generator=g) < 0.5).float()


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': round(ms[len(ms) // 2], 4), 'mean_ms': round(sum(ms) / len(ms), 4), 'min_ms': round(ms[0], 4)}


def timed(fn, draw, warm, n=50):
    for _ in range(warm):
        fn(draw())
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(n)]
    bs = [draw() for _ in range(n)]
    for i in range(n):
        ev[i][0].record(); fn(bs[i]); ev[i][1].record()
    torch.cuda.synchronize()
    return stats([e[0].elapsed_time(e[1]) for e in ev])


res = {'warmup_steps': steps}

# (a) the reference batch on C1 tables, one graph replay per step (ids copied into the captured buffers first, as the device loader does)
D = 64
us, its = tables(6984, 3945, D, False)
S = 2048
fs = FusedPointPairStep(us.table, its.table, S, S, ALPHA, LAM, GAM, user_state=us, item_state=its, **HP)
static = batch(6984, 3945, S)
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    for _ in range(2):
        fs.step(*static)                                     # contexts, device counts: created before the capture
torch.cuda.current_stream().wait_stream(side)
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with B_.capturing(graph, side):
    fs.step(*static)


def replay(b):
    for x, y in zip(static, b):
        x.copy_(y)
    graph.replay()
    fs.replayed(1)


res['c1_2048_2048_graph'] = dict(step=timed(replay, lambda: batch(6984, 3945, S), steps), eager=timed(lambda b: fs.step(*b), lambda: batch(6984, 3945, S), 20),
                                 users=6984, items=3945, D=D)
del fs, graph, us, its
torch.cuda.synchronize(); torch.cuda.empty_cache()

# (b) + (c) at scale: lazy joint step, two FusedPointStep calls (same tables, same batches), exact joint step (fresh exact state)
D = 128
big = {'users': nu, 'items': ni, 'rows_per_domain': BB, 'D': D}
us, its = tables(nu, ni, D, False)
fs = FusedPointPairStep(us.table, its.table, BB, BB, ALPHA, LAM, GAM, user_state=us, item_state=its, **HP)
big['lazy_joint'] = timed(lambda b: fs.step(*b), lambda: batch(nu, ni, BB), steps)
del fs
torch.cuda.synchronize(); torch.cuda.empty_cache()
ps = FusedPointStep(us.table, its.table, BB, loss='bce', user_state=us, item_state=its, **HP)
big['two_point_steps'] = timed(lambda b: (ps.step(b[0], b[1], b[2]), ps.step(b[3], b[4], b[5])), lambda: batch(nu, ni, BB), steps)
del ps
big['lazy_over_two_calls'] = round(big['lazy_joint']['median_ms'] / big['two_point_steps']['median_ms'], 3)
for st in (us, its):                                         # the same tables as an exact state: every row current at update 0
    st.exp_avg = st.exp_avg_sq = None
    torch.cuda.empty_cache()
    st.__init__(st.table, OPT_ADAM, exact=True)
    st.exp_avg.normal_(0, 1e-4, generator=g)
    st.exp_avg_sq.normal_(0, 1e-4, generator=g).square_().add_(1e-12)
torch.cuda.synchronize(); torch.cuda.empty_cache()
fs = FusedPointPairStep(us.table, its.table, BB, BB, ALPHA, LAM, GAM, user_state=us, item_state=its, **HP)


def exact(b):
    rowwise_catch_up([(us, [b[0], b[3]]), (its, [b[1], b[4]])], **HP)
    fs.step(*b)


big['exact_joint'] = timed(exact, lambda: batch(nu, ni, BB), steps)
big['exact_over_lazy'] = round(big['exact_joint']['median_ms'] / big['lazy_joint']['median_ms'], 3)
res['scale'] = big
print(json.dumps(res))
