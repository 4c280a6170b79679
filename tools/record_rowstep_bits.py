#!/usr/bin/env python3
"""Record what the six row-wise steps with dense weights compute, bit for bit (GPU).

    python tools/record_rowstep_bits.py --out DIR        # one rowstep_parent_bits_<step>.npz per step class into DIR
    python tools/record_rowstep_bits.py --check DIR      # rerun and compare with the files in DIR (exit status 1 on any difference)

Only the public step classes of recbole_cdr_amd.fused are used, so the same file runs at any commit that has them: record at the commit
before a change of the steps' host or kernel code, check at the commit with it (tests/test_gpu_rowstep_parent_bits.py does, against
tests/golden/).  Every case runs two consecutive steps with opt='adam' and weight_decay=0.01 on seeded tables of 600 to 2,000 rows and
keeps, after the second step: every touched table's rows, moments and update count, out8 / out16, dP / dW, the dense parameters, and
a sample of the forward kernels' gradient rows (GU / GI / GS / GO / GT / G: every row of a batch of up to 128 rows, else about 96 rows
at an odd stride plus the last 33, so that both rounds of the grid-stride loop and the tail tile are seen directly and not only through
the tables' sums).

A table is kept as the rows the two batches named (``<table>.rows`` and the ``w`` / ``m`` / ``v`` rows at them) plus the number of
elements that moved anywhere else (``*.rest_moved``, 0: the lazy update touches named rows only).  The ids are drawn with repeats from a
seeded pool of 6 to 256 rows of each table, so that a case with 32,801 occurrences still names few rows: the whole record of a step
class has to stay well below the 1 MiB limit of a committed file, and 600 x 128 floats x (row, two moments) of ONE table is already 0.9 MiB.
All random input comes from a CPU generator, so it does not depend on the device's generator.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = 'cuda:0'
HP = dict(opt='adam', lr=1e-2, weight_decay=0.01)
STEPS = ('clfm', 'dtcdr', 'deepapf', 'dcdcsr', 'frozen', 'sscdr')


def golden_path(directory, step):
    return os.path.join(directory, f'rowstep_parent_bits_{step}.npz')


class _Rand:
    def __init__(self, seed):
        self.g = torch.Generator(); self.g.manual_seed(seed)

    def table(self, rows, D, std=0.1):
        return torch.empty(rows, D).normal_(0, std, generator=self.g).to(DEV)

    def dense(self, *shape):
        fan = shape[0] + shape[-1]
        return torch.nn.Parameter(torch.empty(*shape).normal_(0, (2.0 / fan) ** 0.5, generator=self.g).to(DEV))

    def bias(self, n):
        return torch.nn.Parameter(torch.empty(n).normal_(0, 0.1, generator=self.g).to(DEV))

    def ids(self, n, rows, pool, lo=0):
        """n ids in [lo, rows) drawn with repeats from ``pool`` distinct rows."""
        p = torch.randperm(rows - lo, generator=self.g)[:pool] + lo
        return p[torch.randint(0, p.numel(), (n,), generator=self.g)].to(DEV)

    def labels(self, n):
        return (torch.rand(n, generator=self.g) < 0.5).float().to(DEV)


def _keep_table(out, key, st, init, id_lists):
    rows = torch.unique(torch.cat([i.reshape(-1) for i in id_lists]))
    rest = torch.ones(init.shape[0], dtype=torch.bool, device=init.device)
    rest[rows] = False
    out[f'{key}.rows'] = rows
    out[f'{key}.step'] = torch.tensor(st.step)
    for nm, t, t0 in (('w', st.table, init), ('m', st.exp_avg, torch.zeros_like(init)), ('v', st.exp_avg_sq, torch.zeros_like(init))):
        out[f'{key}.{nm}'] = t[rows]
        out[f'{key}.{nm}.rest_moved'] = (t[rest] != t0[rest]).sum()


def _keep_grad_rows(out, key, G, n):
    """A sample of the first n rows of a gradient buffer, as the second step left it."""
    rows = torch.arange(n) if n <= 128 else torch.unique(torch.cat([torch.arange(0, n, n // 96 | 1), torch.arange(n - 33, n)]))
    out[key] = G[rows.to(G.device)]


def _cap_batch(fs):
    """The smallest batch that makes the forward kernel's persistent grid walk a second round of tiles, plus a tail tile."""
    return fs.grid(1 << 20) * 32 + 33


def _clfm(out, tag, Du, Di, share, big, seed):
    from recbole_cdr_amd import binding as B_
    from recbole_cdr_amd.fused import FusedCLFMStep
    import ctypes
    r = _Rand(seed)
    nu, ni = 997, 601
    tabs = [r.table(n, D) for n, D in ((nu, Du), (ni, Di), (nu, Du), (ni, Di))]
    init = [t.clone() for t in tabs]
    weights = tuple(r.dense(n, Du) if n else None for n in (share, Di - share, Di - share))
    Bs, Bt = 33, 33
    if big:
        need = ctypes.c_size_t(0)
        B_._check(B_.load().cdr_clfm_fwd_grad_workspace_bytes(1 << 20, Du, Di, ctypes.byref(need)), 'cdr_clfm_fwd_grad_workspace_bytes')
        Bt = need.value // (4 * Du * Di) * 32 + 33
    fs = FusedCLFMStep(*tabs, weights, Bs, Bt, 0.3, 0.01, **HP)
    pool = 96 if big else 10
    seen = [[] for _ in tabs]
    for _ in range(2):
        b = (r.ids(Bs, nu, pool), r.ids(Bs, ni, pool), r.labels(Bs), r.ids(Bt, nu, pool), r.ids(Bt, ni, pool), r.labels(Bt))
        fs.step(*b)
        for k, i in zip(range(4), (b[0], b[1], b[3], b[4])):
            seen[k].append(i)
    for d, n in enumerate((Bs, Bt)):
        _keep_grad_rows(out, f'{tag}/GU{d}', fs.GU[d], n)
        _keep_grad_rows(out, f'{tag}/GI{d}', fs.GI[d], n)
    for k, nm in enumerate(('source_user', 'source_item', 'target_user', 'target_item')):
        _keep_table(out, f'{tag}/{nm}', fs.states[k], init[k], seen[k])
    out[f'{tag}/out16'], out[f'{tag}/dW'] = fs.out16, fs.dW
    out[f'{tag}/batch'] = torch.tensor([Bs, Bt])
    for nm, w in zip(('shared', 'source_only', 'target_only'), weights):
        if w is not None:
            out[f'{tag}/{nm}'] = w


def _dtcdr(out, tag, D, hidden, p, big, seed):
    from recbole_cdr_amd.fused import FusedDTCDRStep
    r = _Rand(seed)
    nu, ni = 809, 1201
    tabs = [r.table(n, D) for n in (nu, ni, nu, ni)]
    init = [t.clone() for t in tabs]
    widths = [2 * D] + list(hidden)
    towers = [[q for i, o in zip(widths, hidden) for q in (r.dense(o, i), r.bias(o))] + [r.dense(1, hidden[-1]), r.bias(1)]
              for _ in range(2)]
    Bs, Bt = 33, 33
    if big:
        Bs = _cap_batch(FusedDTCDRStep(*tabs, towers, 1, 1, 0.3, dropout_prob=p, **HP))
    fs = FusedDTCDRStep(*tabs, towers, Bs, Bt, 0.3, dropout_prob=p, **HP)
    pool = 32 if big else 10
    users, items = [], []
    for t in range(2):
        b = (r.ids(Bs, nu, pool), r.ids(Bs, ni, pool), r.labels(Bs), r.ids(Bt, nu, pool), r.ids(Bt, ni, pool), r.labels(Bt))
        fs.step(*b, seed=torch.full((1,), 12345 + t, device=DEV, dtype=torch.int64) if p > 0 else None)
        users += [b[0], b[3]]; items += [b[1], b[4]]
    for k in range(4):
        _keep_grad_rows(out, f'{tag}/G{k}', fs.G[k], Bs + Bt)
    for k, nm in enumerate(('source_user', 'source_item', 'target_user', 'target_item')):
        _keep_table(out, f'{tag}/{nm}', fs.states[k], init[k], items if k & 1 else users)
    out[f'{tag}/out16'], out[f'{tag}/dP'] = fs.out16, fs.dP
    out[f'{tag}/batch'] = torch.tensor([Bs, Bt])
    for d, tw in enumerate(towers):
        out[f'{tag}/tower{d}'] = torch.cat([q.reshape(-1) for q in tw])


def _deepapf(out, tag, D, big, seed):
    from recbole_cdr_amd.fused import FusedDeepAPFStep
    r = _Rand(seed)
    nk, no = 701, 1103
    n_over = nk // 2
    tabs = [r.table(n, D) for n in (nk, nk, no, nk, no)]
    init = [t.clone() for t in tabs]
    params = [r.dense(D, D), r.bias(D), r.dense(1, D), r.dense(1, D)]
    Bs, Bt = 33, 33
    if big:
        Bt = _cap_batch(FusedDeepAPFStep(*tabs, params, n_over, 1, 1, **HP))
    fs = FusedDeepAPFStep(*tabs, params, n_over, Bs, Bt, **HP)
    pool = 48 if big else 6

    def keys(n):                                   # half of the keys above n_overlap (strictly): their share candidate is masked
        lo = r.ids(n - n // 2, n_over + 1, pool, lo=1)
        hi = r.ids(n // 2, nk, pool, lo=n_over + 1)
        both = torch.cat([lo, hi])
        return both[torch.randperm(n, generator=r.g).to(DEV)]

    seen = [[] for _ in tabs]
    for _ in range(2):
        b = (keys(Bs), r.ids(Bs, no, 2 * pool), r.labels(Bs), keys(Bt), r.ids(Bt, no, 2 * pool), r.labels(Bt))
        assert int((b[0] > n_over).sum()) == Bs // 2 and int((b[3] > n_over).sum()) == Bt // 2
        fs.step(*b)
        for k, i in ((0, b[0]), (0, b[3]), (1, b[0]), (2, b[1]), (3, b[3]), (4, b[4])):
            seen[k].append(i)
    _keep_grad_rows(out, f'{tag}/GS', fs.GS, Bs + Bt)
    for d, n in enumerate((Bs, Bt)):
        _keep_grad_rows(out, f'{tag}/GO{d}', fs.GO[d], n)
        _keep_grad_rows(out, f'{tag}/GT{d}', fs.GT[d], n)
    for k, nm in enumerate(('share', 'source_only', 'source_other', 'target_only', 'target_other')):
        _keep_table(out, f'{tag}/{nm}', fs.states[k], init[k], seen[k])
    out[f'{tag}/out16'], out[f'{tag}/dP'] = fs.out16, fs.dP
    out[f'{tag}/batch'] = torch.tensor([Bs, Bt])
    out[f'{tag}/params'] = torch.cat([q.reshape(-1) for q in params])


def _dcdcsr(out, tag, dims, big, wlds, seed):
    from recbole_cdr_amd.fused import FusedDCDCSRMapStep
    r = _Rand(seed)
    rows = 1500
    T, bench = r.table(rows, dims[0]), r.table(rows, dims[0])
    init = T.clone()
    layers = [(r.dense(o, i), r.bias(o)) for i, o in zip(dims, dims[1:])]
    n = 33
    if big:
        n = _cap_batch(FusedDCDCSRMapStep(T, bench, layers, 1, **HP))
    fs = FusedDCDCSRMapStep(T, bench, layers, n, **HP)
    seen = []
    for _ in range(2):
        seen.append(r.ids(n, rows, 256 if big else 10))
        fs.step(seen[-1])
    _keep_grad_rows(out, f'{tag}/G', fs.G, n)
    _keep_table(out, f'{tag}/table', fs.state, init, seen)
    out[f'{tag}/out8'], out[f'{tag}/dP'] = fs.out8, fs.dP
    out[f'{tag}/batch'] = torch.tensor([n])
    out[f'{tag}/weights_in_lds'] = torch.tensor(wlds)
    out[f'{tag}/params'] = torch.cat([q.reshape(-1) for pair in layers for q in pair])


def _frozen(out, tag, frozen, D, B, seed):
    from recbole_cdr_amd.fused import FusedFrozenSideBPRStep
    r = _Rand(seed)
    nu, ni = 653, 911
    U, I = r.table(nu, D), r.table(ni, D)
    trained = I if frozen == 'user' else U
    init, other0 = trained.clone(), (U if frozen == 'user' else I).clone()
    fs = FusedFrozenSideBPRStep(U, I, frozen, B, **HP)
    seen = []
    for _ in range(2):
        u, p, n = r.ids(B, nu, 24), r.ids(B, ni, 24), r.ids(B, ni, 24)
        fs.step(u, p, n)
        seen += [p, n] if frozen == 'user' else [u]
    _keep_table(out, f'{tag}/trained', fs.state, init, seen)
    out[f'{tag}/out6'] = fs.out6
    out[f'{tag}/frozen_moved'] = ((U if frozen == 'user' else I) != other0).sum()


def _sscdr(out, tag, D, n, seed):
    from recbole_cdr_amd.fused import SSCDRMapStep
    r = _Rand(seed)
    na, nb = 751, 1301
    SA, TA, SB = r.table(na, D), r.table(na, D), r.table(nb, D)
    init = [t.clone() for t in (SA, TA, SB)]
    lin = torch.nn.Linear(D, D).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(r.dense(D, D).data); lin.bias.copy_(r.bias(D).data)
    fs = SSCDRMapStep(SA, TA, SB, lin, list(lin.parameters()), 0.3, 0.5, **HP)
    a, b = [], []
    for _ in range(2):
        idx, pos, neg = r.ids(n, na, 20), r.ids(n, nb, 20), r.ids(n, nb, 20)
        out[f'{tag}/loss'] = fs.step(idx, pos, neg)
        a.append(idx); b += [pos, neg]
    for nm, st, t0, ids in (('source_a', fs.sa_state, init[0], a), ('target_a', fs.ta_state, init[1], a), ('source_b', fs.sb_state, init[2], b)):
        _keep_table(out, f'{tag}/{nm}', st, t0, ids)
    out[f'{tag}/weight'], out[f'{tag}/bias'] = lin.weight.detach(), lin.bias.detach()


def run(step):
    """{key: numpy array} of one step class: every case, after its second step."""
    out = {}
    if step == 'clfm':
        _clfm(out, 'd24x40_cap', 24, 40, 16, True, 11)           # pad and column guards, Du != Di, the grid-stride loop, a tail tile
        _clfm(out, 'd128_b33', 128, 128, 64, False, 12)          # non-temporal rows, four dW tiles per wave, LDS above 64 KiB, two workgroups
    elif step == 'dtcdr':
        _dtcdr(out, 'd24_drop_cap', 24, [32, 16], 0.25, True, 21)
        _dtcdr(out, 'd128_b33', 128, [64], 0.0, False, 22)
        _dtcdr(out, 'd24_h3_b33', 24, [24, 40, 8], 0.25, False, 23)
    elif step == 'deepapf':
        _deepapf(out, 'd24_cap', 24, True, 31)
        _deepapf(out, 'd128_b33', 128, False, 32)
    elif step == 'dcdcsr':
        _dcdcsr(out, 'd24_cap', [24, 40, 24], True, True, 41)
        _dcdcsr(out, 'd128_lds_b33', [128, 64, 128], False, True, 42)       # weights in LDS, above 64 KiB
        _dcdcsr(out, 'd128_l2_b33', [128, 128, 128], False, False, 43)      # weights read through L2
    elif step == 'frozen':
        _frozen(out, 'user_d24_b33', 'user', 24, 33, 51)
        _frozen(out, 'item_d128_b300', 'item', 128, 300, 52)
    elif step == 'sscdr':
        _sscdr(out, 'd24_n100', 24, 100, 61)
        _sscdr(out, 'd128_n33', 128, 33, 62)
    else:
        raise ValueError(step)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def differences(got, want):
    """Keys whose arrays are not bit-equal (or missing on one side)."""
    bad = sorted(set(got) ^ set(want))
    for k in sorted(set(got) & set(want)):
        a, b = got[k], want[k]
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            bad.append(k)
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out'); ap.add_argument('--check')
    ap.add_argument('--steps', default=','.join(STEPS))
    a = ap.parse_args()
    assert (a.out is None) != (a.check is None), 'one of --out DIR, --check DIR'
    status = 0
    for step in a.steps.split(','):
        got = run(step)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            np.savez_compressed(golden_path(a.out, step), **got)
            print(step, len(got), 'arrays', os.path.getsize(golden_path(a.out, step)), 'bytes', flush=True)
        else:
            bad = differences(got, dict(np.load(golden_path(a.check, step))))
            print(step, len(got), 'arrays', 'identical' if not bad else f'DIFFER: {bad}', flush=True)
            status |= bool(bad)
    return status


if __name__ == '__main__':
    sys.exit(main())
