"""DeepAPF's BOTH-phase training step, row-wise against dense, on identical batches through ``CrossDomainTrainer.fit``:
  rowwise  optimizer_mode='rowwise': fused.FusedDeepAPFStep (csrc/cdr_deepapf.hip's forward per domain + three sorts + five segmented
           applies + DenseAdam on the four attention / predict parameters)
  dense    optimizer_mode='dense': calculate_loss -> backward into five table-sized gradients -> DenseAdam over every parameter (the only
           way to train DeepAPF before the row-wise step; the step is replayed as a hipGraph, as fit does by default)
Default shape: 4 M users x 1 M items per table, D = 64, 65,536 rows per domain, overlap_users mode with half the user ids overlapped (the
other half's share scores are masked).  Per mode: device-event time of whole epochs of ``steps`` batches after a warm-up epoch, divided
by the batch count (median over the epochs); each timed loop runs under its own alarm (SIGALRM's default action ends the process).  The
forward kernel is timed by the library's own event brackets (binding.timing_enable) in a separate pass; its algorithmic traffic per domain
is B rows x (three D-wide table rows read -- two for a masked occurrence --, three D-wide gradient rows written, two ids and a label) +
the parameters + one packed parameter vector per workgroup.
usage: python tools/mb_deepapf_step.py [users] [items] [rows_per_domain] [steps] [epochs] [seconds_per_timed_loop]"""
import ctypes, json, os, signal, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import recbole_cdr_amd  # noqa: F401
from recbole_cdr_amd import binding as B_
from recbole_cdr_amd.data.interaction import Interaction
from recbole_cdr_amd.model.cross_domain_recommender.deepapf import DeepAPF
from recbole_cdr_amd.trainer import CrossDomainTrainer

nu = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
ni = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
BB = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
epochs = int(sys.argv[5]) if len(sys.argv) > 5 else 5
LIMIT = int(sys.argv[6]) if len(sys.argv) > 6 else 60
D = 64
HBM_PEAK = 8.0e12
dev = torch.device('cuda', 0)


class _Single:
    def __init__(self, d):
        self.uid_field, self.iid_field, self.label_field = f'{d}_user_id', f'{d}_item_id', f'{d}_label'

    def num(self, field):
        return nu if field == self.uid_field else ni


class _Dataset:
    """What CrossDomainRecommender.__init__ reads: both domains over the same union id space, half the users overlapped."""
    source_domain_dataset, target_domain_dataset = _Single('source'), _Single('target')
    num_total_user, num_total_item, num_overlap_user, num_overlap_item = nu, ni, nu // 2, 1
    overlap_id_field = 'overlap'


class _Batches(list):
    state = None

    def set_mode(self, state):
        self.state = state


def batches(n, seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    r = lambda hi: torch.randint(1, hi, (BB,), device=dev, generator=g)
    y = lambda: (torch.rand(BB, device=dev, generator=g) < 0.5).float()
    return _Batches(Interaction({'source_user_id': r(nu), 'source_item_id': r(ni), 'source_label': y(),
                                 'target_user_id': r(nu), 'target_item_id': r(ni), 'target_label': y()}) for _ in range(n))


def timed(fn):
    """One timed loop under its own time limit."""
    signal.alarm(LIMIT)
    try:
        return fn()
    finally:
        signal.alarm(0)


def run(mode):
    cfg = {'source_domain': {'NEG_PREFIX': 'neg_'}, 'target_domain': {'NEG_PREFIX': 'neg_'}, 'device': dev, 'embedding_size': D, 'beta': 0.5,
           'learning_rate': 1e-3, 'train_modes': ['BOTH'], 'epoch_num': ['1'], 'source_split': False, 'eval_step': 0, 'epochs': 1,
           'optimizer_mode': mode}
    torch.manual_seed(7)
    model = DeepAPF(cfg, _Dataset()).to(dev)
    trainer = CrossDomainTrainer(cfg, model)
    data = batches(steps, 2024)                              # the same batches for both modes

    def epoch():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); trainer.fit(data); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    timed(epoch)                                             # warm-up epoch: buffers, contexts, the dense mode's capture
    ms = sorted(timed(epoch) for _ in range(epochs))
    out = {'median_ms_per_step': round(ms[len(ms) // 2], 4), 'min_ms_per_step': round(ms[0], 4), 'max_ms_per_step': round(ms[-1], 4),
           'graph_stats': dict(trainer.graph_stats), 'peak_mem_gb': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    if mode == 'rowwise':
        B_.timing_enable(dev, 4096)
        timed(epoch)
        stamps = B_.timing_collect(dev)
        t = sorted(v for k, v in stamps if k == 'deepapf_fwd_grad_kernel')
        B_.timing_enable(dev, 0)
        need = ctypes.c_size_t(0)
        B_.load().cdr_deepapf_fwd_grad_workspace_bytes(BB, D, ctypes.byref(need))
        n_par = D * D + 3 * D
        # half the occurrences masked: 2.5 rows read on average, 3 written
        nbytes = BB * (int(5.5 * 4 * D) + 20) + 4 * n_par + need.value
        med = t[len(t) // 2]
        flop = 3 * 2 * (2 * BB) * D * D                      # three contractions over the 2 B candidates
        out['fwd_kernel'] = {'launches_timed': len(t), 'median_ms': round(med, 4), 'min_ms': round(t[0], 4), 'algorithmic_bytes': nbytes,
                             'fraction_of_8TBs': round(nbytes / (med * 1e-3) / HBM_PEAK, 3), 'gflop': round(flop / 1e9, 3),
                             'tflops': round(flop / (med * 1e-3) / 1e12, 2), 'workgroups': need.value // (4 * n_par)}
        other = {}
        for k, v in stamps:
            if k != 'deepapf_fwd_grad_kernel':
                other.setdefault(k, []).append(v)
        out['other_kernels_median_ms'] = {k: round(sorted(v)[len(v) // 2], 4) for k, v in other.items()}
    del trainer, model, data
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    return out


res = {'users': nu, 'items': ni, 'overlapped_users': nu // 2, 'rows_per_domain': BB, 'D': D, 'steps_per_epoch': steps, 'epochs_timed': epochs}
res['rowwise'] = run('rowwise')
res['dense'] = run('dense')
res['dense_over_rowwise'] = round(res['dense']['median_ms_per_step'] / res['rowwise']['median_ms_per_step'], 2)
print(json.dumps(res))
