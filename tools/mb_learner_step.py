"""config['learner']: the C5-shape domain step of FusedBPRStep (B = 1,048,576 triples) under 'adam' and 'adagrad', at D = 128 and D = 64,
with uniform and Zipf(1.05) positives.  Per (D, id shape) both learners' step objects live side by side and are timed in ALTERNATING
rounds inside one process (measuring-on-mi355x: compare two versions in the same call, alternating them; the spread over the rounds is
printed next to every median).  A timed round is ``steps`` steps between two device events; a second pass with the library's HIP-event
brackets on gives the per-kernel medians (bpr_fwd_apply_kernel dominates) and its fraction of the HBM peak on the byte model of
DESIGN sections 4 and 5: 4 D bytes per row the kernel only gathers, and for a row it updates in place the row and its state read
and written -- 4 D (1 + n_state) * 2 bytes: 3,072 B (Adam, D = 128) against 2,048 B (Adagrad).
Also printed: optimizer-state bytes allocated per table for both learners.

usage: python tools/mb_learner_step.py [--users N] [--items N] [--steps N] [--rounds N] [--learners adam,adagrad] [--dims 128,64] [--out FILE]
(the default tables are C5's: 50,000,001 x D users, 20,000,001 x D items; --learners adam runs in a checkout of another commit too: the
Adam column of two builds on the same box)"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import recbole_cdr_amd  # noqa: F401
from recbole_cdr_amd import binding as B_
from recbole_cdr_amd.fused import FusedBPRStep

HBM_PEAK = 8.0e12          # B/s, MI355X

ap = argparse.ArgumentParser()
ap.add_argument('--users', type=int, default=50_000_001)
ap.add_argument('--items', type=int, default=20_000_001)
ap.add_argument('--batch', type=int, default=1 << 20)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--learners', default='adam,adagrad')
ap.add_argument('--dims', default='128,64')
ap.add_argument('--out', default=None)
a = ap.parse_args()
dev = torch.device('cuda', 0)
g = torch.Generator(device=dev); g.manual_seed(2022)
learners = a.learners.split(',')
B, nu, ni = a.batch, a.users, a.items
EPS = {'adam': 1e-8, 'adagrad': 1e-10}


def zipf(n, rows):
    r = torch.rand(n, device=dev, generator=g, dtype=torch.float64)
    al = 1.05
    return (((float(rows) ** (1 - al) - 1) * r + 1).pow(1 / (1 - al)).long().clamp_(1, rows) - 1)


def batches(shape):
    out = []
    for _ in range(4):
        p = zipf(B, ni) if shape == 'zipf' else torch.randint(0, ni, (B,), device=dev, generator=g)
        out.append((torch.randint(0, nu, (B,), device=dev, generator=g), p, torch.randint(0, ni, (B,), device=dev, generator=g)))
    return out


def state_bytes(st):
    return sum(t.numel() * t.element_size() for t in (st.exp_avg, st.exp_avg_sq) if t is not None)


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


report = {'batch': B, 'users': nu, 'items': ni, 'steps_per_round': a.steps, 'rounds': a.rounds, 'cases': []}
for D in map(int, a.dims.split(',')):
    steps = {}
    for ln in learners:
        U = torch.empty(nu, D, device=dev).normal_(0, 0.01, generator=g)
        I = torch.empty(ni, D, device=dev).normal_(0, 0.01, generator=g)
        steps[ln] = FusedBPRStep(U, I, B, opt=ln, lr=1e-3, eps=EPS[ln], reg_weight=0.01)
    sb = {ln: {'user_table': state_bytes(s.ustate), 'item_table': state_bytes(s.istate), 'tables': 4 * D * (nu + ni)} for ln, s in steps.items()}
    for shape in ('uniform', 'zipf'):
        bs = batches(shape)
        for s in steps.values():                            # warm-up: every buffer, the norm records, the id path's choice
            for i in range(8):
                s.step(*bs[i % 4])
        torch.cuda.synchronize()
        rounds = {ln: [] for ln in learners}
        for r in range(a.rounds):
            for ln in learners:                             # alternating: learner A, learner B, learner A, ...
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.steps):
                    steps[ln].step(*bs[i % 4])
                e1.record(); torch.cuda.synchronize()
                rounds[ln].append(e0.elapsed_time(e1) / a.steps)
        kern = {}
        for ln in learners:                                 # per-kernel times: a pass of their own (the brackets cost host time)
            B_.timing_enable(dev, 4096)
            B_.timing_collect(dev)
            for i in range(8):
                steps[ln].step(*bs[i % 4])
            torch.cuda.synchronize()
            kt = {}
            for nm, ms in B_.timing_collect(dev):
                kt.setdefault(nm, []).append(ms)
            B_.timing_enable(dev, 0)
            kern[ln] = {k: round(med(v), 4) for k, v in kt.items()}
        flags = steps[learners[0]].flags[:4 * B].view(B, 4)[:, :3].bool()
        singles = flags.sum(0).tolist()                    # rows the forward kernel updated in place: user, positive, negative
        case = {'D': D, 'ids': shape, 'single_rows': singles, 'learners': {}}
        for ln in learners:
            ms = rounds[ln]
            n_state = 2 if ln == 'adam' else 1
            # bpr_fwd_apply_kernel's bytes, DESIGN section 4's model: (2 + 2 n_state) 4D per row the launch updates in place (row and
            # state read and written) + 4D per row it only gathers
            upd = sum(singles)
            model_bytes = 4 * D * (upd * (2 + 2 * n_state) + (3 * B - upd))
            dom = max(kern[ln].items(), key=lambda kv: kv[1]) if kern[ln] else (None, None)
            fwd = kern[ln].get('bpr_fwd_apply_kernel')
            case['learners'][ln] = {'median_ms': round(med(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
                                    'spread': round((max(ms) - min(ms)) / med(ms), 4), 'kernels_ms': kern[ln], 'dominant_kernel': dom[0],
                                    'fwd_apply_model_bytes': int(model_bytes),
                                    'fwd_apply_hbm_fraction': None if not fwd else round(model_bytes / (fwd * 1e-3) / HBM_PEAK, 3),
                                    'single_row_bytes': 4 * D * 2 * (1 + n_state), 'state_bytes': sb[ln]}
        if 'adam' in rounds and 'adagrad' in rounds:
            case['adagrad_over_adam'] = round(med(rounds['adagrad']) / med(rounds['adam']), 4)
        report['cases'].append(case)
        print(json.dumps(case), flush=True)
    del steps
    torch.cuda.empty_cache()
if a.out:
    with open(a.out, 'w') as f:
        json.dump(report, f, indent=1)
