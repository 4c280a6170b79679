"""The index kernels of the row-sharded BPR step (csrc/cdr_route.hip, cdr_dedup.hip, the plan of cdr_step.hip, the owner's gather of
cdr_rows.hip) against exact references in plain torch: integer results with torch.equal, the two floating-point ones
(cdr_gather_rows_norms' squared norms, cdr_segsum_rows) against float64 with first-order bounds.

Shapes sit where the code takes another path: route_sort_config merge-sorts below 4,096 items and runs Onesweep from there (n = 4095 /
4096 / 4097); the owner key has one 9-bit digit up to 512 ranks and two past them (world = 512 / 513 / 1024); worlds 3 and 5 leave owner
values unused in bits_for(world) bits; owners that receive nothing sit at the start, the end and in the middle of ``counts``;
3 Bl = 2^18 is where the plan's sort switches to the big-sort path (Bl = 87381 / 87382); the plan's table bit comes from the user side
(user_rows >> item_local_rows * world) or from the item key's owner and local-row bits; item_local_rows = 1024 / 1025 moves the local-row
field by one bit; cdr_segsum_rows sums segments of up to kLongSeg = 32 occurrences in their head and cuts longer ones into pieces of
kPiece = 256 (lengths 32 / 33 / 255 / 256 / 257 / 513 / 1000), and launches no piece kernel at all for n <= 32."""
import ctypes

import pytest
import torch

from fp64_bounds import _grad_bound, gam
from helpers import DEV
from test_shard_gloo import OracleOps

pytestmark = pytest.mark.gpu

NS = [1, 4095, 4096, 4097, 20011]


def _ops():
    import recbole_cdr_amd  # noqa: F401
    from recbole_cdr_amd.shard import NativeOps
    return NativeOps(torch.device(DEV))


def _gen(seed):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    return g


def _owner_sets(world):
    """Owner subsets that leave the first, the last or the middle owners without an id."""
    sets = {'all': list(range(world))}
    if world >= 2:
        sets['first_empty'] = list(range(1, world))
        sets['last_empty'] = list(range(world - 1))
    if world >= 3:
        sets['middle_empty'] = [0, world - 1]
        sets['one_owner'] = [world // 2]
    return sets


def _ids(owners, n, world, max_local, gen, hot=0):
    """n global ids local * world + owner with owner from ``owners``; ``hot``: half of the locals from [0, hot) (duplicates)."""
    ow = torch.tensor(owners, device=DEV)[torch.randint(0, len(owners), (n,), device=DEV, generator=gen)]
    local = torch.randint(0, max_local, (n,), device=DEV, generator=gen)
    if hot:
        pick = torch.rand(n, device=DEV, generator=gen) < 0.5
        local = torch.where(pick, torch.randint(0, min(hot, max_local), (n,), device=DEV, generator=gen), local)
    return local * world + ow


def _bits_for(v):
    b = 1
    while b < 32 and (1 << b) < v:
        b += 1
    return b


# ---------------------------------------------------------------------------------------------------------------------- routing

@pytest.mark.parametrize('world', [1, 2, 3, 5, 8, 512, 513, 1024])
@pytest.mark.parametrize('n', NS)
def test_route_permute_inverse(n, world):
    ops, gen = _ops(), _gen(n + world)
    for name, owners in _owner_sets(world).items():
        ids = _ids(owners, n, world, 1 << 40, gen)
        owner = ids % world
        want_perm = torch.argsort(owner, stable=True)
        want_counts = torch.bincount(owner, minlength=world)
        for n1 in ((0,) if n == 1 else (0, n // 3)):
            tag = f'n={n} world={world} {name} n1={n1}'
            ids0, ids1 = ids[:n - n1].contiguous(), (ids[n - n1:].contiguous() if n1 else None)
            perm, counts = ops.route(ids0, ids1, world)
            p = perm.long()
            assert torch.equal(p, want_perm), f'{tag}: perm is not the stable argsort of id % world'
            assert torch.equal(counts, want_counts), f'{tag}: counts'
            for div in sorted({1, world}):
                for fb in sorted({0, 1, n - n1, n // 2, n}):
                    out = ops.permute(ids0, ids1, perm, div, flag_below=fb)
                    want = (ids[p] // div) | ((p < fb).long() << 62)
                    assert torch.equal(out, want), f'{tag}: permute divisor={div} flag_below={fb}'
            want_pos = torch.empty(n, device=DEV, dtype=torch.int64)
            want_pos[p] = torch.arange(n, device=DEV)
            assert torch.equal(ops.inverse_perm(perm), want_pos), f'{tag}: inverse_perm'


@pytest.mark.parametrize('world', [1, 2, 3, 5, 8])
@pytest.mark.parametrize('n', NS)
def test_route_triples(n, world):
    ops, gen, oracle = _ops(), _gen(3 * n + world), OracleOps()
    for name, owners in _owner_sets(world).items():
        uid = _ids(owners, n, world, 1 << 30, gen)
        pid = torch.randint(0, 1 << 40, (n,), device=DEV, generator=gen)
        nid = torch.randint(0, 1 << 40, (n,), device=DEV, generator=gen)
        send3, counts = ops.route_triples(uid, pid, nid, world)
        w3, wc = oracle.route_triples(uid.cpu(), pid.cpu(), nid.cpu(), world)
        assert torch.equal(send3.cpu(), w3), f'n={n} world={world} {name}: send3'
        assert torch.equal(counts.cpu(), wc), f'n={n} world={world} {name}: counts'


# ---------------------------------------------------------------------------------------------------------------------- dedup

def _dedup_sorted_again(plan, world, lb):
    """cdr_dedup_sorted once more on the plan's sorted keys, into buffers of this test: NativeOps.dedup does not hand n_uniq out."""
    from recbole_cdr_amd import binding as B_
    n = plan['n']
    need = ctypes.c_size_t(0)
    B_._check(B_.load().cdr_dedup_workspace_bytes(n, ctypes.byref(need)), 'cdr_dedup_workspace_bytes')
    ws = torch.empty(need.value, device=DEV, dtype=torch.uint8)
    uidx = torch.empty(n, device=DEV, dtype=torch.int32)
    uniq_local, umap = torch.empty(n, device=DEV, dtype=torch.int64), torch.empty(n, device=DEV, dtype=torch.int64)
    counts, n_uniq = torch.empty(world + 1, device=DEV, dtype=torch.int64), torch.empty(1, device=DEV, dtype=torch.int64)
    B_.call('cdr_dedup_sorted', B_.stream(), B_.raw(plan['keys']), B_.raw(plan['perm']), n, int(world), lb, B_.raw(uidx), B_.i64(uniq_local),
            B_.i64(umap), B_.i64(counts), B_.i64(n_uniq), B_.raw(ws), ws.numel())
    return uidx, uniq_local, umap, counts[:world], n_uniq


@pytest.mark.parametrize('local_rows', [1024, 1025])
@pytest.mark.parametrize('world', [2, 3, 5, 8])
def test_dedup_sorted(world, local_rows):
    ops, gen, oracle = _ops(), _gen(world + local_rows), OracleOps()
    lb = max(int(local_rows - 1).bit_length(), 1)
    for name, owners in _owner_sets(world).items():
        for n0 in (1, 1500):
            tag = f'world={world} local_rows={local_rows} {name} n0={n0}'
            ids0 = _ids(owners, n0, world, local_rows, gen, hot=40)
            ids1 = _ids(owners, n0, world, local_rows, gen, hot=40)
            ids0[0] = (local_rows - 1) * world + owners[-1]                  # the last local row of the last owner that has any
            if n0 > 1:
                ids1[1] = owners[0]                                          # local row 0
            plan = ops.dedup(ids0, ids1, world, local_rows)
            want = oracle.dedup(ids0.cpu(), ids1.cpu(), world, local_rows)
            nu = want['uniq_local'].numel()
            n = 2 * n0
            keys, perm = plan['keys'].long() & 0xFFFFFFFF, plan['perm'].long()
            both = torch.cat([ids0, ids1])
            wkey = torch.sort(((both % world) << lb) | (both // world), stable=True)
            assert torch.equal(keys, wkey.values) and torch.equal(perm, wkey.indices), f'{tag}: sorted keys / stable perm'
            for label, (uidx, uniq_local, umap, counts, n_uniq) in (
                    ('NativeOps.dedup', (plan['uidx'], plan['uniq_local'], plan['umap'], plan['counts'], None)),
                    ('second call', _dedup_sorted_again(plan, world, lb))):
                assert torch.equal(counts.cpu(), want['counts']), f'{tag} {label}: counts {counts.tolist()} vs {want["counts"].tolist()}'
                assert torch.equal(uniq_local[:nu].cpu(), want['uniq_local']), f'{tag} {label}: uniq_local'
                assert torch.equal(umap.cpu(), want['umap']), f'{tag} {label}: umap'
                uidx = uidx.long()
                assert bool((uidx[1:] >= uidx[:-1]).all()), f'{tag} {label}: uniq_index decreases'
                assert torch.equal(uidx, umap[perm]), f'{tag} {label}: uniq_index[q] != umap[perm[q]]'
                assert int(uidx[0]) == 0 and int(uidx[n - 1]) == nu - 1
                if n_uniq is not None:
                    assert int(n_uniq[0]) == nu, f'{tag}: n_uniq {int(n_uniq[0])} vs {nu}'


# ---------------------------------------------------------------------------------------------------------------------- plan

def _check_plan(tag, ops, recv3, world, user_rows, il):
    """The whole contract of cdr_bpr_shard_plan (include/cdr_hip.h)."""
    Bl = recv3.shape[0]
    plan = ops.plan(recv3, world, user_rows, il, 8)
    buf = plan['buf']
    u, items = recv3[:, 0], torch.cat([recv3[:, 1], recv3[:, 2]])
    assert torch.equal(plan['u_loc'], u), f'{tag}: u_loc'
    lb, ob = _bits_for(il), (_bits_for(world) if world > 1 else 0)
    hb = max(_bits_for(user_rows), lb + ob)
    base = 1 << hb
    wa = torch.sort(u, stable=True)
    wb = torch.sort(base + (((items % world) << lb) | (items // world)), stable=True)
    keys, perm = buf['keys'][:3 * Bl].long() & 0xFFFFFFFF, buf['perm'][:3 * Bl].long()
    assert torch.equal(keys[:Bl], wa.values) and torch.equal(keys[Bl:], wb.values), f'{tag}: sorted keys (table bit {hb}, local bits {lb})'
    assert torch.equal(perm[:Bl], wa.indices) and torch.equal(perm[Bl:], wb.indices), f'{tag}: perm is not stable inside equal keys'
    assert bool((keys[1:Bl] >= keys[:Bl - 1]).all()) and bool((keys[Bl + 1:] >= keys[Bl:-1]).all())
    # the request list
    want = OracleOps().plan(recv3.cpu(), world, user_rows, il, 8)
    nu = want['uniq_local'].numel()
    assert int(buf['n_uniq'][0]) == nu, f'{tag}: n_uniq {int(buf["n_uniq"][0])} vs {nu}'
    assert torch.equal(plan['counts'].cpu(), want['counts']), f'{tag}: counts {plan["counts"].tolist()} vs {want["counts"].tolist()}'
    assert torch.equal(plan['uniq_local'][:nu].cpu(), want['uniq_local']), f'{tag}: uniq_local'
    assert torch.equal(plan['umap'].cpu(), want['umap']), f'{tag}: umap'
    uidx = buf['uidx'][:2 * Bl].long()
    assert bool((uidx[1:] >= uidx[:-1]).all()) and torch.equal(uidx, plan['umap'][perm[Bl:]]), f'{tag}: uidx'
    # byte 0 / 1 / 2 of a triple's flag word: this occurrence is the only one of its row in its list; byte 3 stays zero
    wkeys = torch.cat([wa.values, wb.values])
    same = wkeys[1:] == wkeys[:-1]
    first = torch.ones(3 * Bl, dtype=torch.bool, device=DEV); first[1:] = ~same
    last = torch.ones(3 * Bl, dtype=torch.bool, device=DEV); last[:-1] = ~same
    wperm = torch.cat([wa.indices, wb.indices])
    occ = torch.cat([4 * wperm[:Bl], torch.where(wperm[Bl:] < Bl, 4 * wperm[Bl:] + 1, 4 * (wperm[Bl:] - Bl) + 2)])
    want_flags = torch.zeros(4 * Bl, dtype=torch.uint8, device=DEV); want_flags[occ] = (first & last).to(torch.uint8)
    got_flags = buf['flags'][:4 * Bl]
    assert torch.equal(got_flags, want_flags), (f'{tag}: {int((got_flags != want_flags).sum())} flag bytes differ, first at byte '
                                                f'{int(torch.nonzero(got_flags != want_flags)[0])}')
    # the two duplicate-head lists: exactly the heads of the segments of two and more occurrences (any order)
    heads = buf['heads'].long()
    nA, nB = int(heads[0]), int(heads[1])
    hd = first & ~last
    assert nA == int(hd[:Bl].sum()) and nB == int(hd[Bl:].sum()), f'{tag}: head counts {nA}, {nB}'
    oB = 4 + Bl // 2 + 1
    assert torch.equal(torch.sort(heads[4:4 + nA]).values, torch.nonzero(hd[:Bl]).flatten()), f'{tag}: duplicate user heads'
    assert torch.equal(torch.sort(heads[oB:oB + nB]).values, torch.nonzero(hd[Bl:]).flatten()), f'{tag}: duplicate item heads'
    return plan


def _recv3(Bl, world, user_rows, il, gen):
    u = torch.randint(0, user_rows, (Bl,), device=DEV, generator=gen)
    hot = torch.rand(Bl, device=DEV, generator=gen) < 0.5
    u = torch.where(hot, torch.randint(0, min(user_rows, 64), (Bl,), device=DEV, generator=gen), u)
    p = _ids(list(range(world)), Bl, world, il, gen, hot=50)
    n = _ids(list(range(world)), Bl, world, il, gen, hot=50)
    u[0], p[0], n[0] = user_rows - 1, il * world - 1, 0
    if Bl > 1:
        u[1], p[1], n[1] = 0, 0, il * world - 1
    return torch.stack([u, p, n], 1).contiguous()


@pytest.mark.parametrize('il', [1024, 1025])
@pytest.mark.parametrize('user_rows', [50, 1 << 22])                # the table bit from the item key's bits / from the user side
@pytest.mark.parametrize('world', [1, 3, 8])
@pytest.mark.parametrize('Bl', [1, 2, 1000, 87381, 87382])
def test_shard_plan(Bl, world, user_rows, il):
    lb, ob = _bits_for(il), (_bits_for(world) if world > 1 else 0)
    assert (_bits_for(user_rows) > lb + ob) == (user_rows > 50)      # both branches of the table bit are taken
    gen = _gen(Bl + world + il)
    _check_plan(f'Bl={Bl} world={world} user_rows={user_rows} il={il}', _ops(), _recv3(Bl, world, user_rows, il, gen), world, user_rows, il)


@pytest.mark.parametrize('world', [3, 5, 8])
def test_shard_plan_owners_that_are_asked_nothing(world):
    """Empty buckets at the start, the end and in the middle of ``counts`` (shard_emit_kernel fills the owners' starts without atomics)."""
    il, user_rows, Bl = 1024, 777, 1000
    gen, ops = _gen(world), _ops()
    for name, owners in _owner_sets(world).items():
        r3 = _recv3(Bl, world, user_rows, il, gen)
        r3[:, 1], r3[:, 2] = _ids(owners, Bl, world, il, gen, hot=50), _ids(owners, Bl, world, il, gen, hot=50)
        plan = _check_plan(f'world={world} {name}', ops, r3, world, user_rows, il)
        assert [int(c) > 0 for c in plan['counts'].tolist()] == [k in owners for k in range(world)]


@pytest.mark.parametrize('world', [1, 3, 8])
def test_shard_plan_one_hot_item_and_p_equals_n(world):
    il, user_rows, Bl = 1025, 777, 1000
    gen = _gen(world)
    ops = _ops()
    # every positive is ONE item, which also occurs as a negative
    r3 = _recv3(Bl, world, user_rows, il, gen)
    hot = 5 * world + (world - 1)
    r3[:, 1] = hot
    r3[7::50, 2] = hot
    plan = _check_plan(f'one positive item, world={world}', ops, r3, world, user_rows, il)
    slot = plan['umap'][0]
    assert bool((plan['umap'][:Bl] == slot).all()) and int((plan['umap'][Bl:] == slot).sum()) == int((r3[:, 2] == hot).sum()) >= len(range(7, Bl, 50))
    # p == n inside a triple: alone among the triples (a segment of exactly two), and next to further occurrences
    r3 = _recv3(Bl, world, user_rows, il, gen)
    r3[10:40, 2] = r3[10:40, 1]
    lonely = il * world - 2
    r3[:, 1:][r3[:, 1:] == lonely] = 3
    r3[500, 1] = r3[500, 2] = lonely
    plan = _check_plan(f'p == n, world={world}', ops, r3, world, user_rows, il)
    assert int(plan['umap'][500]) == int(plan['umap'][Bl + 500])
    assert plan['buf']['flags'][4 * 500 + 1:4 * 500 + 3].tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------------- owner's gather

@pytest.mark.parametrize('n', [1, 3, 1025])
@pytest.mark.parametrize('D', [4, 8, 24, 64, 128, 256])
def test_gather_rows_norms(D, n):
    ops, gen = _ops(), _gen(D + n)
    rows = 777
    table = torch.empty(rows, D, device=DEV).normal_(0, 0.3, generator=gen)
    lists = [torch.tensor([0], device=DEV), torch.tensor([rows - 1], device=DEV)] if n == 1 else []
    if n > 1:
        ids = torch.randint(0, rows, (n,), device=DEV, generator=gen)
        ids[0], ids[1], ids[2] = 0, rows - 1, rows - 1                    # row 0, the last row, a repeat
        if n > 3:
            ids[n // 2:] = ids[:n - n // 2].clone()
        lists.append(ids)
    for ids in lists:
        got, nrm2 = ops.gather_rows_norms(table, ids)
        assert torch.equal(got.view(torch.int32), table[ids].view(torch.int32)), f'D={D} n={n}: rows are not bit-equal to table[ids]'
        want = (table[ids].double() ** 2).sum(1)
        err = (nrm2.double() - want).abs()
        # D products and D - 1 additions of non-negative terms, in any order: relative gamma_{D+1}
        assert bool((err <= gam(D + 1) * want).all()), f'D={D} n={n}: squared norm off by {float((err / want).max()):.3g} relative (bound {gam(D + 1):.3g})'


# ---------------------------------------------------------------------------------------------------------------------- segment sums

def _segsum_case(ops, lengths, D, gen, world=3, local_rows=1024):
    """Items with the given occurrence counts, shuffled over a positive and a negative list of n / 2 each."""
    n = sum(lengths)
    assert n % 2 == 0
    Bl = n // 2
    distinct = torch.randperm(local_rows * world, device=DEV, generator=gen)[:len(lengths)]
    occ = torch.repeat_interleave(distinct, torch.tensor(lengths, device=DEV))[torch.randperm(n, device=DEV, generator=gen)]
    ids0, ids1 = occ[:Bl].contiguous(), occ[Bl:].contiguous()
    plan = ops.dedup(ids0, ids1, world, local_rows)
    nu = len(lengths)
    G = torch.empty(Bl, D, device=DEV).normal_(0, 1.0, generator=gen)
    rows = torch.empty(nu, D, device=DEV).normal_(0, 1.0, generator=gen)
    coef = torch.tensor([0.37], device=DEV)
    out = ops.segsum(plan, G, Bl, rows, coef, nu)
    again = ops.segsum(plan, G, Bl, rows, coef, nu)
    umap = plan['umap']
    seglen = torch.bincount(umap, minlength=nu)
    assert sorted(seglen.tolist()) == sorted(lengths)
    sign = torch.cat([torch.ones(Bl, device=DEV), -torch.ones(Bl, device=DEV)]).double()
    terms = torch.cat([G, G]).double() * sign[:, None]
    npos = torch.bincount(umap[:Bl], minlength=nu).double()
    reg = float(coef[0]) * npos[:, None] * rows.double()
    want = torch.zeros(nu, D, device=DEV, dtype=torch.float64).index_add_(0, umap, terms) + reg
    A = torch.zeros(nu, D, device=DEV, dtype=torch.float64).index_add_(0, umap, terms.abs()) + reg.abs()
    return out, again, want, _grad_bound(D, want, A, torch.zeros_like(A), seglen), seglen, npos


@pytest.mark.parametrize('D', [4, 64, 128, 256])
def test_segsum_rows(D):
    ops, gen = _ops(), _gen(D)
    for lengths in ([1, 2, 32, 33, 255, 256, 257, 513, 1000, 1], [1, 2, 3, 10, 16]):        # the second: n = 32, no piece launch
        out, again, want, bound, seglen, npos = _segsum_case(ops, lengths, D, gen)
        tag = f'cdr_segsum_rows D={D} n={sum(lengths)}'
        assert bool(torch.isfinite(out).all()), f'{tag}: non-finite values'
        r = (out.double() - want).abs() / bound
        worst = r.max(1).values
        print(f'\n{tag}: worst error / bound per segment length: ' + ' '.join(f'{int(l)}:{float(w):.3g}' for l, w in sorted(zip(seglen.tolist(), worst.tolist()))))
        if float(worst.max()) > 1.0:
            j = int(worst.argmax())
            raise AssertionError(f'{tag}: error / bound = {float(worst[j]):.3g} in the segment of {int(seglen[j])} occurrences ({int(npos[j])} positives), '
                                 f'col {int(r[j].argmax())}: got {float(out[j, int(r[j].argmax())])!r} want {float(want[j, int(r[j].argmax())])!r}')
        assert torch.equal(out.view(torch.int32), again.view(torch.int32)), f'{tag}: a second call on the same inputs differs'


# ---------------------------------------------------------------------------------------------------------------------- full-sort movers

@pytest.mark.parametrize('U', [1, 5])
@pytest.mark.parametrize('world', [1, 3, 8])
def test_interleave_shards_and_gather_owned_rows(world, U):
    import recbole_cdr_amd  # noqa: F401
    from recbole_cdr_amd import binding as B_
    gen = _gen(world + U)
    N = 1001                                                 # odd, N % 4 != 0: the rows of out start unaligned
    Nl = N // world + 1                                      # N < Nl * world: padded columns in the gathered layout
    assert N % 2 == 1 and N % 4 != 0 and N < Nl * world
    gathered = torch.empty(world * U, Nl, device=DEV).normal_(0, 1, generator=gen)
    out = torch.full((U, N), float('nan'), device=DEV)
    B_.call('cdr_interleave_shards', B_.stream(), B_.f32(gathered), world, U, Nl, N, B_.f32(out))
    c = torch.arange(N, device=DEV)
    want = gathered.view(world, U, Nl)[c % world, :, c // world].t().contiguous()      # out[u][c] = gathered[c % world][u][c / world]
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)), f'cdr_interleave_shards world={world} U={U}'

    D, n = 24, 200 * U + 1
    full = torch.empty(N, D, device=DEV).normal_(0, 1, generator=gen)
    ids = torch.randint(0, N, (n,), device=DEV, generator=gen)
    ids[0], ids[n - 1] = 0, N - 1
    if n > 3:
        ids[2] = ids[1]
    total = torch.zeros(n, D, device=DEV)
    for rank in range(world):
        shard = full[rank::world].contiguous()
        got = torch.full((n, D), float('nan'), device=DEV)
        B_.call('cdr_gather_owned_rows', B_.stream(), B_.f32(shard), D, B_.i64(ids), n, world, rank, B_.f32(got))
        own = (ids % world == rank)
        want = torch.where(own[:, None], shard[(ids // world).clamp(max=shard.shape[0] - 1)], torch.zeros((), device=DEV))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f'cdr_gather_owned_rows world={world} rank={rank}'
        total += got
    assert torch.equal(total.view(torch.int32), full[ids].view(torch.int32)), 'the sum over the ranks is not table_full[ids]'
