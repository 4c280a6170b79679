"""DCDCSR's BOTH-phase map step and its second-TARGET-visit BPR step, row-wise against dense, on identical inputs:
  rowwise  model.fused_train_step: fused.FusedDCDCSRMapStep (csrc/cdr_dcdcsr.hip's forward-and-backward launch + its finishing launch + one
           id sort + one segmented apply + DenseAdam on the mapping MLP) and fused.FusedFrozenSideBPRStep (cdr_bpr_fwd_grad + one sort + one
           apply)
  dense    calculate_loss -> backward into a table-sized gradient -> DenseAdam over every parameter with a gradient (the only way to train
           DCDCSR before the row-wise steps).  The dense path is older than the row-wise one: ``--root <tree>`` imports the package from
           another checkout (a build of the parent commit), so that the baseline is measured on the code that had nothing else.
Default shape: 4 M users x 1 M items per table, D = 64, hidden [128], overlap_users mode with half the user ids overlapped; the BOTH step
at map_batch_size 1,024 (the default) and 65,536, the frozen-side step at 65,536 triples.  The benchmark and affine tables are random
(building them is a phase switch, not a step).  Per case: device-event time of ``steps`` steps after a warm-up loop, divided by the step
count (median over ``epochs`` loops); each timed loop runs under its own alarm (SIGALRM's default action ends the process).  The map kernel
is timed by the library's own event brackets (binding.timing_enable) in a separate pass; its algorithmic traffic is n x (two D-wide rows
read, one D-wide gradient row written, one id) + the parameters + one packed parameter vector per workgroup.
usage: python tools/mb_dcdcsr_step.py [rowwise|dense|all] [--root TREE] [users] [items] [steps] [epochs] [seconds_per_timed_loop]"""
import ctypes, json, os, signal, sys
args = sys.argv[1:]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if '--root' in args:
    j = args.index('--root')
    root = os.path.abspath(args[j + 1])
    del args[j:j + 2]
sys.path.insert(0, root)
import numpy as np
import torch
import recbole_cdr_amd  # noqa: F401
from recbole_cdr_amd import binding as B_
from recbole_cdr_amd.data.interaction import Interaction
from recbole_cdr_amd.model.cross_domain_recommender.dcdcsr import DCDCSR
from recbole_cdr_amd.trainer.trainer import DenseAdam

which = args[0] if args and args[0] in ('rowwise', 'dense', 'all') else 'all'
nums = [int(a) for a in args if a.isdigit()]
nu = nums[0] if len(nums) > 0 else 4_000_000
ni = nums[1] if len(nums) > 1 else 1_000_000
steps = nums[2] if len(nums) > 2 else 20
epochs = nums[3] if len(nums) > 3 else 5
LIMIT = nums[4] if len(nums) > 4 else 60
D, HIDDEN, TRIPLES = 64, [128], 65536
HBM_PEAK = 8.0e12
dev = torch.device('cuda', 0)


class _Single:
    def __init__(self, d):
        self.uid_field, self.iid_field, self.label_field = f'{d}_user_id', f'{d}_item_id', f'{d}_label'

    def num(self, field):
        return nu if field == self.uid_field else ni


class _Dataset:
    """What CrossDomainRecommender.__init__ and DCDCSR.build_unit2pop read: both domains over the same union id space, half the users
    overlapped, every user with one interaction."""
    source_domain_dataset, target_domain_dataset = _Single('source'), _Single('target')
    num_total_user, num_total_item, num_overlap_user, num_overlap_item = nu, ni, nu // 2, 1
    num_target_only_user, num_source_only_user, num_target_only_item, num_source_only_item = nu // 2, 0, ni - 1, 0
    overlap_id_field = 'overlap'

    def history_item_matrix(self, value_field=None, domain='source'):
        return None, None, torch.ones(nu)

    def history_user_matrix(self, value_field=None, domain='source'):
        return None, None, torch.ones(ni)


def timed(fn):
    """One timed loop under its own time limit."""
    signal.alarm(LIMIT)
    try:
        return fn()
    finally:
        signal.alarm(0)


def model_for(map_batch):
    cfg = {'source_domain': {'NEG_PREFIX': 'neg_'}, 'target_domain': {'NEG_PREFIX': 'neg_'}, 'device': dev, 'latent_factor_model': 'BPR',
           'embedding_size': D, 'mlp_hidden_size': HIDDEN, 'k': 10, 'map_batch_size': map_batch}
    torch.manual_seed(7)
    return DCDCSR(cfg, _Dataset()).to(dev)


def loops(step):
    def epoch():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(steps):
            step(s)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps
    timed(epoch)                                             # warm-up loop: buffers, contexts, optimizer state
    ms = sorted(timed(epoch) for _ in range(epochs))
    return {'median_ms_per_step': round(ms[len(ms) // 2], 4), 'min_ms_per_step': round(ms[0], 4), 'max_ms_per_step': round(ms[-1], 4),
            'peak_mem_gb': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}, epoch


def dense_step(model, opt, interaction):
    opt.zero_grad(set_to_none=True)
    loss = model.calculate_loss(interaction)
    loss.backward()
    opt.step()


def run_both(mode, n):
    model = model_for(n)
    model.phase, model.phase2count['BOTH'] = 'BOTH', 1
    g = torch.Generator(device=dev); g.manual_seed(11)
    model.benchmark_embedding = torch.empty(nu, D, device=dev).normal_(0, 0.1, generator=g)
    np.random.seed(2024)                                     # the same draws for both modes
    if mode == 'rowwise':
        out, epoch = loops(lambda s: model.fused_train_step(None, lr=1e-3))
        B_.timing_enable(dev, 4096)
        timed(epoch)
        stamps = B_.timing_collect(dev)
        B_.timing_enable(dev, 0)
        t = sorted(v for k, v in stamps if k == 'dcdcsr_map_kernel')
        dims = [D] + HIDDEN + [D]
        need = ctypes.c_size_t(0)
        B_.load().cdr_dcdcsr_map_fwd_grad_workspace_bytes(n, len(dims) - 1, (ctypes.c_int * len(dims))(*dims), ctypes.byref(need))
        n_par = sum(dims[l + 1] * dims[l] + dims[l + 1] for l in range(len(dims) - 1))
        nbytes = n * (3 * 4 * D + 8) + 4 * n_par + need.value
        flop = 3 * 2 * n * sum(dims[l + 1] * dims[l] for l in range(len(dims) - 1))     # three contractions per layer
        med = t[len(t) // 2]
        out['map_kernel'] = {'launches_timed': len(t), 'median_ms': round(med, 4), 'min_ms': round(t[0], 4), 'algorithmic_bytes': nbytes,
                             'fraction_of_8TBs': round(nbytes / (med * 1e-3) / HBM_PEAK, 4), 'gflop': round(flop / 1e9, 3),
                             'tflops': round(flop / (med * 1e-3) / 1e12, 2), 'workgroups': need.value // (4 * n_par)}
        other = {}
        for k, v in stamps:
            if k != 'dcdcsr_map_kernel':
                other.setdefault(k, []).append(v)
        out['other_kernels_median_ms'] = {k: round(sorted(v)[len(v) // 2], 4) for k, v in other.items()}
    else:
        opt = DenseAdam(model.parameters(), lr=1e-3)
        out, _ = loops(lambda s: dense_step(model, opt, None))
    del model
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    return out


def run_frozen(mode):
    model = model_for(1024)
    model.phase, model.phase2count['TARGET'] = 'TARGET', 2
    g = torch.Generator(device=dev); g.manual_seed(12)
    n_tgt = model.target_num_users
    model.affine_embedding = torch.empty(n_tgt, D, device=dev).normal_(0, 0.1, generator=g)
    r = lambda hi: torch.randint(1, hi, (TRIPLES,), device=dev, generator=g)
    data = [Interaction({'target_user_id': r(n_tgt), 'target_item_id': r(ni), 'neg_target_item_id': r(ni)}) for _ in range(steps)]
    if mode == 'rowwise':
        out, _ = loops(lambda s: model.fused_train_step(data[s], lr=1e-3))
    else:
        opt = DenseAdam(model.parameters(), lr=1e-3)
        out, _ = loops(lambda s: dense_step(model, opt, data[s]))
    del model, data
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    return out


res = {'users': nu, 'items': ni, 'overlapped_users': nu // 2, 'D': D, 'hidden': HIDDEN, 'steps_per_loop': steps, 'loops_timed': epochs,
       'package_root': os.path.relpath(root, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))}
for mode in (('rowwise', 'dense') if which == 'all' else (which,)):
    res[mode] = {'both_1024': run_both(mode, 1024), 'both_65536': run_both(mode, 65536), 'target2_65536': run_frozen(mode)}
print(json.dumps(res))
