"""DTCDR's BOTH-phase training step, row-wise against dense, on identical batches through ``CrossDomainTrainer.fit``:
  rowwise  optimizer_mode='rowwise': fused.FusedDTCDRStep (csrc/cdr_dtcdr.hip's forward + one sort + four segmented applies + DenseAdam
           on the twelve tower parameters)
  dense    optimizer_mode='dense': calculate_loss -> backward into four table-sized gradients -> DenseAdam over every parameter (the only
           way to train DTCDR before the row-wise step; the step is replayed as a hipGraph, as fit does by default)
Default shape: 4 M users x 1 M items per table, D = 64, hidden [32, 16], 65,536 rows per domain, dropout_prob 0 and 0.1.  Per mode:
device-event time of whole epochs of ``steps`` batches after a warm-up epoch, divided by the batch count (median over the epochs).  The
forward kernel is timed by the library's own event brackets (binding.timing_enable) in a separate pass; its algorithmic traffic per domain
is B rows x (four D-wide table rows read, four D-wide gradient rows written, two ids and a label) + the tower + one packed parameter
vector per workgroup.
usage: python tools/mb_dtcdr_step.py [users] [items] [rows_per_domain] [steps] [epochs]"""
import ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import recbole_cdr_amd  # noqa: F401
from recbole_cdr_amd import binding as B_
from recbole_cdr_amd.data.interaction import Interaction
from recbole_cdr_amd.model.cross_domain_recommender.dtcdr import DTCDR
from recbole_cdr_amd.trainer import CrossDomainTrainer

nu = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
ni = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
BB = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
epochs = int(sys.argv[5]) if len(sys.argv) > 5 else 5
D = 64
HIDDEN = [32, 16]
HBM_PEAK = 8.0e12
dev = torch.device('cuda', 0)


class _Single:
    def __init__(self, d):
        self.uid_field, self.iid_field, self.label_field = f'{d}_user_id', f'{d}_item_id', f'{d}_label'

    def num(self, field):
        return nu if field == self.uid_field else ni


class _Dataset:
    """What CrossDomainRecommender.__init__ reads: both domains over the same union id space."""
    source_domain_dataset, target_domain_dataset = _Single('source'), _Single('target')
    num_total_user, num_total_item, num_overlap_user, num_overlap_item = nu, ni, nu, 1
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


def run(mode, p_drop):
    cfg = {'source_domain': {'NEG_PREFIX': 'neg_'}, 'target_domain': {'NEG_PREFIX': 'neg_'}, 'device': dev, 'embedding_size': D,
           'mlp_hidden_size': HIDDEN, 'dropout_prob': p_drop, 'base_model': 'NeuMF', 'alpha': 0.5,
           'learning_rate': 1e-3, 'train_modes': ['BOTH'], 'epoch_num': ['1'], 'source_split': False, 'eval_step': 0, 'epochs': 1,
           'optimizer_mode': mode}
    torch.manual_seed(7)
    model = DTCDR(cfg, _Dataset()).to(dev)
    trainer = CrossDomainTrainer(cfg, model)
    data = batches(steps, 2024)                              # the same batches for both modes
    trainer.fit(data)                                        # warm-up epoch: buffers, contexts, the dense mode's capture
    torch.cuda.synchronize()
    ms = []
    for _ in range(epochs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); trainer.fit(data); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    ms.sort()
    out = {'median_ms_per_step': round(ms[len(ms) // 2], 4), 'min_ms_per_step': round(ms[0], 4), 'max_ms_per_step': round(ms[-1], 4),
           'graph_stats': dict(trainer.graph_stats), 'peak_mem_gb': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    if mode == 'rowwise':
        B_.timing_enable(dev, 4096)
        trainer.fit(data)
        torch.cuda.synchronize()
        timed = B_.timing_collect(dev)
        t = sorted(v for k, v in timed if k == 'dtcdr_fwd_grad_kernel')
        B_.timing_enable(dev, 0)
        need = ctypes.c_size_t(0)
        B_.load().cdr_dtcdr_fwd_grad_workspace_bytes(BB, D, len(HIDDEN), (ctypes.c_int * len(HIDDEN))(*HIDDEN), ctypes.byref(need))
        w = [2 * D] + HIDDEN
        n_par = sum(o * i + o for i, o in zip(w[:-1], w[1:])) + w[-1] + 1
        mac = sum(o * i for i, o in zip(w[:-1], w[1:]))
        nbytes = BB * (8 * 4 * D + 20) + 4 * n_par + need.value
        med = t[len(t) // 2]
        out['fwd_kernel'] = {'launches_timed': len(t), 'median_ms': round(med, 4), 'min_ms': round(t[0], 4), 'algorithmic_bytes': nbytes,
                             'fraction_of_8TBs': round(nbytes / (med * 1e-3) / HBM_PEAK, 3),
                             'gflop': round(3 * 2 * BB * mac / 1e9, 3), 'tflops': round(3 * 2 * BB * mac / (med * 1e-3) / 1e12, 2)}
        other = {}
        for k, v in timed:
            if k != 'dtcdr_fwd_grad_kernel':
                other.setdefault(k, []).append(v)
        out['other_kernels_median_ms'] = {k: round(sorted(v)[len(v) // 2], 4) for k, v in other.items()}
    del trainer, model, data
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    return out


res = {'users': nu, 'items': ni, 'rows_per_domain': BB, 'D': D, 'hidden': HIDDEN, 'steps_per_epoch': steps, 'epochs_timed': epochs}
for p_drop in (0.0, 0.1):
    r = {'rowwise': run('rowwise', p_drop), 'dense': run('dense', p_drop)}
    r['dense_over_rowwise'] = round(r['dense']['median_ms_per_step'] / r['rowwise']['median_ms_per_step'], 2)
    res[f'dropout_{p_drop}'] = r
print(json.dumps(res))
