"""Host-side mirrors of the reference's interface (CPU): native overlap remap bit-exact against the golden vectors, the
four-state loader against the reference's recorded traces, batch layouts."""
import numpy as np
import pytest
import torch

import recbole_cdr_amd  # noqa: F401
from recbole_cdr_amd.data import overlap_remap, CrossDomainDataloader, OverlapDataloader, DomainTrainLoader
from recbole_cdr_amd.utils import CrossDomainDataLoaderState, InputType, train_mode2state
from golden_util import Golden, cases


# The integer paths (a11 overlap remap, a13 batch layout) are host code, but the driver's round-end record is the `-m gpu` session on
# the GPU box: these tests run in BOTH sessions (one unmarked instance, one gpu-marked instance) so that the record covers them.
both_sessions = pytest.mark.parametrize('session', ['host', pytest.param('gpu_box', marks=pytest.mark.gpu)])


def _tokens(g, key):
    toks = [str(t) for t in g[f'in/{key}_tokens']]
    nan = g[f'in/{key}_isnan'] if g.has(f'in/{key}_isnan') else np.zeros(len(toks), bool)
    return [None if m else t for t, m in zip(toks, nan)]


@both_sessions
@pytest.mark.parametrize('name', cases('remap_'))
def test_native_remap_bit_exact(name, session):
    g = Golden(name)
    su, si, tu, ti = (_tokens(g, k) for k in ('source_user', 'source_item', 'target_user', 'target_item'))
    sfeat = [str(t) for t in g['in/source_user_feat_tokens']] if g.has('in/source_user_feat_tokens') else []
    tfeat = [str(t) for t in g['in/target_user_feat_tokens']] if g.has('in/target_user_feat_tokens') else []
    ru = overlap_remap(su + sfeat, tu + tfeat)
    ri = overlap_remap(si, ti)
    np.testing.assert_array_equal(ru.source_ids[:len(su)], g['applied/source_user'])
    np.testing.assert_array_equal(ru.target_ids[:len(tu)], g['applied/target_user'])
    np.testing.assert_array_equal(ri.source_ids, g['applied/source_item'])
    np.testing.assert_array_equal(ri.target_ids, g['applied/target_item'])
    assert (ru.num_overlap, ru.num_source_only, ru.num_target_only, ru.num_total) == tuple(
        int(g[f'count/{k}']) for k in ('num_overlap_user', 'num_source_only_user', 'num_target_only_user', 'num_total_user'))
    assert (ri.num_overlap, ri.num_source_only, ri.num_target_only, ri.num_total) == tuple(
        int(g[f'count/{k}']) for k in ('num_overlap_item', 'num_source_only_item', 'num_target_only_item', 'num_total_item'))
    # every (token -> id) pair of the reference's dictionaries
    for prefix, toks, ids in (('source_user', su + sfeat, ru.source_ids), ('target_user', tu + tfeat, ru.target_ids),
                              ('source_item', si, ri.source_ids), ('target_item', ti, ri.target_ids)):
        want = dict(zip((str(t) for t in g[f'{prefix}/tokens']), g[f'{prefix}/ids'].tolist()))
        for t, i in zip(toks, ids):
            if t is not None:
                assert want[t] == i, (prefix, t)


@both_sessions
def test_remap_large_random_matches_oracle(session):
    from oracle import remap as oremap
    rng = np.random.RandomState(1)
    s = [f'tok{n}' for n in rng.randint(0, 50000, 200000)]
    t = [f'tok{n}' for n in rng.randint(25000, 90000, 150000)]
    r = overlap_remap(s, t)
    ms, _, mt, _, counts = oremap.overlap_remap(s, ['x'], t, ['y'])
    np.testing.assert_array_equal(r.source_ids, oremap.apply_remap(s, ms))
    np.testing.assert_array_equal(r.target_ids, oremap.apply_remap(t, mt))
    assert r.num_total == counts['num_total_user']


def _loader(name, n_batches, bs):
    inter = {f'{name}_user_id': torch.arange(n_batches * bs) // bs, f'{name}_item_id': torch.arange(n_batches * bs)}
    sampler = lambda u, i, k: torch.zeros(u.numel() * k, dtype=torch.int64)
    return DomainTrainLoader(inter, f'{name}_user_id', f'{name}_item_id', f'{name}_label', 'neg_', bs, 1,
                             InputType.PAIRWISE, sampler)


@both_sessions
def test_four_state_loader_matches_reference_trace(session):
    g = Golden('revoke_layout')
    dl = CrossDomainDataloader(_loader('source', 2, 3), _loader('target', 5, 4), OverlapDataloader(6, 2))
    for state in ('BOTH', 'SOURCE', 'TARGET', 'OVERLAP'):
        dl.set_mode(train_mode2state[state])
        assert len(dl) == int(g[f'layout/{state}/len'])
        ep = []
        it = iter(dl)
        while True:
            try:
                b = dl.__next__()
            except StopIteration:
                break
            ep.append([int(b['source_user_id'][0]) if 'source_user_id' in b else -1,
                       int(b['target_user_id'][0]) if 'target_user_id' in b else -1,
                       int(b['overlap'][0, 0]) // 2 if 'overlap' in b else -1,
                       len(b['source_user_id']) if 'source_user_id' in b else 0,
                       len(b['target_user_id']) if 'target_user_id' in b else 0])
        assert it is not None
        np.testing.assert_array_equal(np.array(ep, dtype=np.int64), g[f'layout/{state}/trace'])
        assert (dl.source_dataloader.pr, dl.target_dataloader.pr, dl.overlap_dataloader.pr) == (0, 0, 0)
    dl.set_mode(CrossDomainDataLoaderState.BOTH)
    iter(dl)
    dl.__next__()
    with pytest.raises(PermissionError):
        dl.set_mode(CrossDomainDataLoaderState.SOURCE)


@both_sessions
def test_train_loader_layouts(session):
    """k-major negatives; POINTWISE = repeat(1+k) with labels [1]*S + [0]*(S k)  (SURVEY App. A)."""
    inter = {'source_user_id': torch.tensor([5, 6, 7]), 'source_item_id': torch.tensor([10, 11, 12])}
    sampler = lambda u, i, k: torch.arange(100, 100 + u.numel() * k)
    pw = DomainTrainLoader(inter, 'source_user_id', 'source_item_id', 'source_label', 'neg_', 6, 2, InputType.PAIRWISE, sampler)
    b = next(iter(pw))
    assert b['source_user_id'].tolist() == [5, 6, 7, 5, 6, 7] and b['neg_source_item_id'].tolist() == list(range(100, 106))
    pt = DomainTrainLoader(inter, 'source_user_id', 'source_item_id', 'source_label', 'neg_', 9, 2, InputType.POINTWISE, sampler)
    b = next(iter(pt))
    assert b['source_item_id'].tolist() == [10, 11, 12] + list(range(100, 106))
    assert b['source_label'].tolist() == [1.0] * 3 + [0.0] * 6
    ov = next(iter(OverlapDataloader(7, 3)))
    assert tuple(ov['overlap'].shape) == (3, 1) and ov['overlap'][:, 0].tolist() == [0, 1, 2]


def test_evaluate_topk_path_equals_full_matrix_path():
    """Trainer.evaluate's two routes -- the model's ``full_sort_topk`` (CSR history mask + sorted-key hit matching on the
    host side) and the reference's full score matrix + in-place -inf + torch.topk -- give identical metrics.  The model
    here is a CPU stand-in with both methods written in plain torch, so only the host logic is under test."""
    from recbole_cdr_amd.trainer.trainer import Trainer

    class Stub(torch.nn.Module):
        target_num_items = 57

        def __init__(self):
            super().__init__()
            g = torch.Generator(); g.manual_seed(0)
            self.w = torch.nn.Parameter(torch.randn(40, 8, generator=g))
            self.items = torch.randn(57, 8, generator=g)

        def full_sort_predict(self, inter):
            return (self.w[inter['uid']] @ self.items.t()).reshape(-1)

        def full_sort_topk(self, inter, k, hist_indptr=None, hist_cols=None):
            s = (self.w[inter['uid']] @ self.items.t()).detach().clone()
            s[:, 0] = -float('inf')
            if hist_indptr is not None:
                for u in range(s.shape[0]):
                    s[u, hist_cols[hist_indptr[u]:hist_indptr[u + 1]]] = -float('inf')
            return torch.topk(s, k, dim=1)

    class Inter(dict):
        def to(self, dev):
            return self

        def __len__(self):
            return self['uid'].numel()

    rng = np.random.RandomState(3)
    batches = []
    for lo in (0, 16, 32):
        uid = torch.arange(lo, min(lo + 16, 40))
        n = uid.numel()
        hr = np.repeat(np.arange(n), 5); hc = rng.randint(1, 57, hr.size)
        pu = np.repeat(np.arange(n), 3); pi = rng.randint(1, 57, pu.size)
        pairs = np.unique(np.stack([pu, pi], 1), axis=0)                      # (user, item) positives, deduplicated
        hist = (torch.from_numpy(hr), torch.from_numpy(hc)) if lo != 16 else None     # one batch without history
        batches.append((Inter(uid=uid), hist, torch.from_numpy(pairs[:, 0]), torch.from_numpy(pairs[:, 1])))
    cfg = {'device': 'cpu', 'topk': [5, 10], 'valid_metric': 'Recall@10'}
    model = Stub()
    tr = Trainer.__new__(Trainer)
    tr.config, tr.model, tr.device, tr.topk = cfg, model, 'cpu', [5, 10]
    tr.fused_topk = True
    a = tr.evaluate(batches)
    tr.fused_topk = False
    b = tr.evaluate(batches)
    assert set(a) == set(b) and a['recall@10'] > 0
    for k in a:
        assert abs(a[k] - b[k]) < 1e-7, (k, a[k], b[k])


@pytest.mark.parametrize('users_per_batch', [None, 16])
def test_full_sort_eval_loader_batches(users_per_batch):
    """Every batch of FullSortEvalLoader carries exactly the positives / history pairs of its own users, as rows relative
    to the batch (recbole FullSortEvalDataLoader's (interaction, history_index, positive_u, positive_i) contract); the batch is
    eval_batch_size // item_num users, or the throughput-sized override for the fused top-k evaluation."""
    from recbole_cdr_amd.data import FullSortEvalLoader
    rng = np.random.RandomState(1)
    ev = np.stack([rng.randint(1, 60, 300), rng.randint(1, 40, 300)], 1)
    hi = np.stack([rng.randint(1, 80, 900), rng.randint(1, 40, 900)], 1)          # includes users that are not evaluated
    loader = FullSortEvalLoader('uid', ev, hi, item_num=40, eval_batch_size=40 * 7, device='cpu', users_per_batch=users_per_batch)
    assert loader.step == (users_per_batch or 7)
    ev_set, hi_set = {tuple(p) for p in ev.tolist()}, {tuple(p) for p in hi.tolist()}
    users_seen = []
    for inter, (hr, hc), pu, pi in loader:
        us = inter['uid'].tolist()
        users_seen += us
        got_pos = {(us[r], c) for r, c in zip(pu.tolist(), pi.tolist())}
        got_hist = {(us[r], c) for r, c in zip(hr.tolist(), hc.tolist())}
        assert got_pos == {p for p in ev_set if p[0] in us}
        assert got_hist == {p for p in hi_set if p[0] in us}
    assert users_seen == sorted({p[0] for p in ev_set})
    assert len(loader) == (len(users_seen) + loader.step - 1) // loader.step
    # the same users re-cut into other batch sizes (what Trainer.evaluate does for the fused top-k path): every batch still carries
    # exactly its own users' pairs, rows relative to the batch
    for step in (1, 5, 64, 10_000):
        assert loader.rebatch(step).step == step
        seen = []
        for inter, (hr, hc), pu, pi in loader:
            us = inter['uid'].tolist()
            assert 1 <= len(us) <= step
            seen += us
            assert {(us[r], c) for r, c in zip(pu.tolist(), pi.tolist())} == {p for p in ev_set if p[0] in us}
            assert {(us[r], c) for r, c in zip(hr.tolist(), hc.tolist())} == {p for p in hi_set if p[0] in us}
        assert seen == users_seen and len(loader) == (len(seen) + step - 1) // step


def test_alias_table_matches_reference_construction():
    """build_alias_table == the reference's _build_alias_table (crossdomain_sampler.py:66-94) restated with its dicts and lists:
    same keys, same probabilities, same aliases; and the table reproduces the item frequencies exactly."""
    from collections import Counter
    from recbole_cdr_amd.sampler import build_alias_table
    rng = np.random.RandomState(0)
    cand = (rng.zipf(1.3, 5000) % 97 + 3).tolist()
    prob = dict(Counter(cand)); alias = prob.copy()
    large_q, small_q = [], []
    for i in prob:
        alias[i] = -1
        prob[i] = prob[i] / len(cand) * len(prob)
        if prob[i] > 1:
            large_q.append(i)
        elif prob[i] < 1:
            small_q.append(i)
    while len(large_q) != 0 and len(small_q) != 0:
        l = large_q.pop(0); s = small_q.pop(0)
        alias[s] = l
        prob[l] = prob[l] - (1 - prob[s])
        if prob[l] < 1:
            small_q.append(l)
        elif prob[l] > 1:
            large_q.append(l)
    keys, p, a = build_alias_table(np.array(cand))
    assert keys.tolist() == list(prob.keys())
    np.testing.assert_allclose(p, np.array(list(prob.values())), rtol=1e-12)
    assert a.tolist() == [alias[k] for k in prob]
    # mass of item x = (prob[x] + sum over columns c with alias[c] == x of (1 - prob[c])) / n  must be its frequency
    mass = {int(k): min(pv, 1.0) for k, pv in zip(keys, p)}
    for k, pv, al in zip(keys, p, a):
        if al >= 0:
            mass[int(al)] += 1.0 - min(pv, 1.0)
    cnt = Counter(cand)
    for k in cnt:
        assert abs(mass[k] / len(keys) - cnt[k] / len(cand)) < 1e-9


def _fake_bench_result(bloat=1):
    """A result dict with the CURRENT schema of bench.py's legs (the keys run_c5 / the leg functions fill), with prose fields and
    per-leg objects inflated `bloat` times: what bench.compact_line has to bound."""
    B, ms = 1 << 20, 3.977
    prose = 'x' * (400 * bloat)
    leg = {'value': 1.0e6, 'unit': 'interactions/s', 'ms_per_step': 0.177, 'steps': 200, 'roofline': {'what': prose, 'frac': 0.1},
           'kernels': [{'kernel': 'k%d' % i, 'avg_ms': 0.01, 'note': prose} for i in range(12)], 'workload': prose}
    return {
        'metric': 'training interactions/sec', 'value': 2 * B / (ms * 1e-3), 'unit': 'interactions/s', 'n_gpus': 1, 'steps': 20, 'warmup': 5,
        'ms_per_step': ms, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
        'config': {'workload': 'C5: EMCDR-BPR D=128 ' + prose, 'batch_per_domain_per_rank': B, 'k_neg': 1, 'optimizer': 'rowwise-adam',
                   'sharding': 'none', 'streams': prose, 'nested': {'dropped': True}},
        'roofline': {'bound': 'hbm', 'kernel': 'bpr_fwd_apply_kernel', 'achieved': 5776.0, 'peak': 8000.0, 'unit': 'GB/s', 'frac': 0.722,
                     'avg_launch_ms': 1.4877, 'algorithmic_bytes': 8593278976, 'bytes_model': prose, 'rocprof': prose,
                     'traffic': {'bytes': 8905212672, 'source': prose}},
        'cpu_baseline': {'value': 2.2e5, 'unit': 'interactions/s', 'cores': 4, 'host_cores': 16, 'kind': 'port', 'cpu_model': 'EPYC',
                         'sample': prose, 'all_cores': {'value': 1.0, 'sample': prose}, 'one_thread': {'value': 1.0, 'sample': prose}},
        'kernels': leg['kernels'], 'roofline_step': {'frac': 0.61, 'what': prose}, 'overlap_phase': leg, 'synthetic_grid': [leg] * 6,
        'fullsort': {'U=1': {'items_per_s': 1.1e10, 'ms': 0.89}, 'U=1024': {'items_per_s': 4.4e11, 'ms': 23.2}, 'conet': {'cases': {'a': leg}}},
        'configs': {n: leg for n in ('c1', 'c2', 'c3', 'c4_full_last_layer', 'c4')}, 'e2e': {'phases': [leg] * 3},
        'leg_errors': {'e2e': prose}, 'deterministic_backward': False, 'bench_wall_s': 102.1,
    }


@pytest.mark.parametrize('bloat', [1, 40])
def test_bench_line_builder_keeps_the_driver_contract(bloat, tmp_path, capsys):
    """VERDICT r4 missing #1: BENCH_r04.json had `parsed: null` -- the one line had grown to 24.7 KB.  bench.emit() now writes every
    leg to bench_detail.json and prints a bounded line LAST on stdout: the contract keys, config, roofline (traffic = bytes or null),
    cpu_baseline.  This runs the line builder on the current schema, at the size a real run produces and 40 times inflated."""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    res = _fake_bench_result(bloat)
    bench.emit(res, detail_dir=str(tmp_path))
    out = capsys.readouterr()
    assert out.err == ''
    lines = out.out.splitlines()
    assert len(lines) == 1 and len(lines[-1]) <= bench.LINE_LIMIT <= 4096
    d = json.loads(lines[-1])
    for k, t in (('metric', str), ('value', float), ('unit', str), ('n_gpus', int), ('steps', int), ('warmup', int),
                 ('ms_per_step', float), ('higher_is_better', bool), ('scaling', str), ('dtype', str), ('data', str), ('config', dict)):
        assert isinstance(d[k], t), (k, type(d[k]))
    assert 'vs_baseline' in d and d['vs_baseline'] is None and d['higher_is_better'] is True and d['scaling'] == 'weak'
    assert 'workload' in d['config'] and 'model' not in d['config'] and all(not isinstance(v, (dict, list)) for v in d['config'].values())
    r = d['roofline']
    assert r['bound'] in ('hbm', 'mfma') and r['unit'] in ('GB/s', 'TFLOP/s') and r['kernel']
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9
    assert r['traffic'] is None or (isinstance(r['traffic'], int) and r['traffic'] > 0)          # a number of bytes, not an object
    c = d['cpu_baseline']
    assert c['kind'] in ('port', 'reference') and c['cores'] >= 1 and c['value'] > 0 and isinstance(c['sample'], str) and c['unit'] == d['unit']
    B = d['config']['batch_per_domain_per_rank']
    assert abs(d['value'] - 2 * B * d['n_gpus'] / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-6
    assert d['detail_file'] == bench.DETAIL_FILE and d['bench_wall_s'] == 102.1
    full = json.load(open(tmp_path / bench.DETAIL_FILE))                                            # nothing is lost: the legs are in the file
    assert full['configs']['c3']['ms_per_step'] == 0.177 and len(full['synthetic_grid']) == 6 and full['roofline']['traffic']['bytes'] > 0


def test_bench_line_builder_takes_a_plain_run(tmp_path, capsys, monkeypatch):
    """A plain bench.py run (no --full, the default) has the contract keys and none of the legs, rooflines or baselines: the line and the
    detail file carry it as it is."""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1'])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1', '--full'])
    assert bench.parse().full is True
    res = {k: v for k, v in _fake_bench_result(1).items() if k in bench.CONTRACT_KEYS + ('config', 'final_loss', 'bench_wall_s')}
    bench.emit(res, detail_dir=str(tmp_path))
    out = capsys.readouterr()
    assert out.err == '' and len(out.out.splitlines()) == 1
    d = json.loads(out.out)
    for k in bench.CONTRACT_KEYS:
        assert d[k] == res[k], k
    assert 'roofline' not in d and 'cpu_baseline' not in d and 'vs_cpu' not in d and d['bench_wall_s'] == res['bench_wall_s']
    assert json.load(open(tmp_path / bench.DETAIL_FILE)) == res


def test_filed_bench_lines_of_this_round_parse():
    """Every `profiles/r05_bench*_line.json` (the last stdout line of a bench.py run on the GPU box, filed as printed) is one bounded
    JSON object with the contract's keys."""
    import glob
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in glob.glob(os.path.join(root, 'profiles', 'r05_bench*_line.json')):
        txt = open(path).read().strip()
        assert '\n' not in txt and len(txt) <= 4096, path
        d = json.loads(txt)
        assert isinstance(d['value'], float) and isinstance(d['roofline'], dict) and d['detail_file'], path
        for k in ('metric', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config'):
            assert k in d, (path, k)
        if os.path.basename(path) == 'r05_bench_c5_line.json':            # the driver's command: the CPU baseline rides on the same line
            assert isinstance(d['cpu_baseline'], dict) and d['cpu_baseline']['kind'] == 'port' and d['roofline']['traffic'] > 0


@both_sessions
def test_history_matrix_builder_bit_exact(session):
    """data/history.py (torch sort / scatter; runs on whatever device it is given) against the reference's get_history_matrix
    output recorded in NATR's fixtures (dataset.py:181-249) and against the oracle's loop restatement on a larger random case."""
    from golden_util import Golden
    from oracle.history import history_matrix as oracle_hist
    from recbole_cdr_amd.data.history import history_matrix
    for name, row in (('natr_users', 'item'), ('natr_items', 'user')):
        g = Golden(name)
        ids = g.idspace()
        t = g['aux/t_pairs']
        mat, val, lens = history_matrix(t[:, 0], t[:, 1], ids.total_num_users, ids.total_num_items, row, 'cpu')
        L = int(g.meta('max_inter_length'))
        np.testing.assert_array_equal(mat[:, :L].numpy(), g['aux/history_matrix'])
        np.testing.assert_array_equal(lens.numpy(), g['aux/history_lens'])
    rng = np.random.RandomState(0)
    u, i = rng.randint(0, 300, 5000), rng.randint(0, 200, 5000)
    for row in ('user', 'item'):
        want = oracle_hist(u, i, 300, 200, row)
        got = history_matrix(u, i, 300, 200, row, 'cpu')
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a.numpy(), b.numpy())


# ---- round 4 host logic ---------------------------------------------------------------------------------------------------------------
def test_interaction_update_keeps_the_k_major_hint_only_when_both_sides_agree():
    """merging a k-major batch into rows WITHOUT the hint (or with another k) must not mark the mixture k-major; an empty
    Interaction adopts the other side's hint; equal hints survive (the BOTH-mode merge of two pairwise loaders with the same k)."""
    from recbole_cdr_amd.data.interaction import Interaction
    a = Interaction({'x': torch.arange(4)}); a.k_major = 2
    b = Interaction({'y': torch.arange(4)}); b.k_major = 2
    assert a.update(b).k_major == 2
    c = Interaction({'x': torch.arange(4)})                           # rows without a hint
    assert c.update(b).k_major is None
    d = Interaction({'x': torch.arange(4)}); d.k_major = 3
    assert d.update(b).k_major is None
    assert Interaction().update(b).k_major == 2                       # nothing there yet: adopt
    e = Interaction({'x': torch.arange(4)}); e.k_major = 2
    assert e.update(Interaction({'z': torch.arange(4)})).k_major is None


def test_domain_loader_pin_shuffles_in_place_with_the_same_permutation():
    """DomainTrainLoader.pin() (what a captured batch producer needs: fixed addresses): an epoch shuffle permutes the columns IN PLACE
    with the permutation the un-pinned loader would have applied, and the caller's tensors are left alone."""
    from recbole_cdr_amd.data import DomainTrainLoader
    from recbole_cdr_amd.utils import InputType
    u, i = torch.arange(100), torch.arange(100) * 7
    smp = lambda uu, ii, k: torch.zeros(uu.numel() * k, dtype=torch.int64)
    mk = lambda: DomainTrainLoader({'u': u.clone(), 'i': i.clone()}, 'u', 'i', 'l', 'neg_', 16, 1, InputType.PAIRWISE, smp, shuffle=True,
                                   generator=torch.Generator().manual_seed(5))
    a, b = mk(), mk()
    src = a.inter['u']
    b.pin()
    addr = b.inter['u'].data_ptr()
    for _ in range(3):
        iter(a); iter(b)
        assert torch.equal(a.inter['u'], b.inter['u']) and torch.equal(a.inter['i'], b.inter['i'])
        assert torch.equal(b.inter['i'], b.inter['u'] * 7) and b.inter['u'].data_ptr() == addr
    assert torch.equal(src, torch.arange(100)) or a.inter['u'] is not src


def test_trainer_row_shard_keeps_the_k_major_hint_only_when_every_field_divides():
    """Trainer._my_rows checks EVERY field's length (BOTH-mode batches carry columns of two lengths)."""
    from recbole_cdr_amd.data.interaction import Interaction
    from recbole_cdr_amd.trainer.trainer import Trainer
    t = Trainer.__new__(Trainer)
    t.__dict__['_row_group'] = (1, 2)                                  # rank 1 of 2, no process group needed
    ok = Interaction({'a': torch.arange(8), 'b': torch.arange(8)}); ok.k_major = 2
    assert t._my_rows(ok).k_major == 2
    bad = Interaction({'a': torch.arange(8), 'b': torch.arange(10)}); bad.k_major = 2   # 10 / 2 = 5 positives: not divisible by 2 ranks
    assert t._my_rows(bad).k_major is None
