"""CLFM's BOTH-phase training step, row-wise against dense, on identical batches through ``CrossDomainTrainer.fit``:
  rowwise  optimizer_mode='rowwise': fused.FusedCLFMStep (csrc/cdr_clfm.hip's forward + sort + segmented applies + DenseAdam on the weights)
  dense    optimizer_mode='dense': calculate_loss -> backward into four table-sized gradients -> DenseAdam over every parameter (the only
           way to train CLFM before the row-wise step; the step is replayed as a hipGraph, as fit does by default)
Default shape: 4 M users x 1 M items per domain, Du = Di = 64, share 32, 65,536 rows per domain.  Per mode: device-event time of whole
epochs of ``steps`` batches after a warm-up epoch, divided by the batch count (median over the epochs).  The forward kernel is timed by
the library's own event brackets (binding.timing_enable) in a separate pass; its algorithmic traffic per domain is B rows x (a Du and a
Di row read, a Du and a Di gradient row written, two ids and a label) + W + one [Di, Du] partial per workgroup.
usage: python tools/mb_clfm_step.py [users] [items] [rows_per_domain] [steps] [epochs]"""
import ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import recbole_cdr_amd  # noqa: F401
from recbole_cdr_amd import binding as B_
from recbole_cdr_amd.data.interaction import Interaction
from recbole_cdr_amd.model.cross_domain_recommender.clfm import CLFM
from recbole_cdr_amd.trainer import CrossDomainTrainer

nu = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
ni = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
BB = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
epochs = int(sys.argv[5]) if len(sys.argv) > 5 else 5
Du = Di = 64
SHARE = 32
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


def run(mode):
    cfg = {'source_domain': {'NEG_PREFIX': 'neg_'}, 'target_domain': {'NEG_PREFIX': 'neg_'}, 'device': dev, 'user_embedding_size': Du,
           'source_item_embedding_size': Di, 'target_item_embedding_size': Di, 'share_embedding_size': SHARE, 'alpha': 0.5, 'reg_weight': 0.01,
           'learning_rate': 1e-3, 'train_modes': ['BOTH'], 'epoch_num': ['1'], 'source_split': False, 'eval_step': 0, 'epochs': 1,
           'optimizer_mode': mode}
    torch.manual_seed(7)
    model = CLFM(cfg, _Dataset()).to(dev)
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
        t = sorted(v for k, v in B_.timing_collect(dev) if k == 'clfm_fwd_grad_kernel')
        B_.timing_enable(dev, 0)
        need = ctypes.c_size_t(0)
        B_.load().cdr_clfm_fwd_grad_workspace_bytes(BB, Du, Di, ctypes.byref(need))
        nbytes = BB * (2 * 4 * (Du + Di) + 20) + 4 * Di * Du + need.value
        med = t[len(t) // 2]
        out['fwd_kernel'] = {'launches_timed': len(t), 'median_ms': round(med, 4), 'min_ms': round(t[0], 4), 'algorithmic_bytes': nbytes,
                             'fraction_of_8TBs': round(nbytes / (med * 1e-3) / HBM_PEAK, 3),
                             'gflop': round(3 * 2 * BB * Du * Di / 1e9, 3), 'tflops': round(3 * 2 * BB * Du * Di / (med * 1e-3) / 1e12, 2)}
    del trainer, model, data
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    return out


res = {'users': nu, 'items': ni, 'rows_per_domain': BB, 'Du': Du, 'Di': Di, 'share': SHARE, 'steps_per_epoch': steps, 'epochs_timed': epochs}
res['rowwise'] = run('rowwise')
res['dense'] = run('dense')
res['dense_over_rowwise'] = round(res['dense']['median_ms_per_step'] / res['rowwise']['median_ms_per_step'], 2)
print(json.dumps(res))
assert res['rowwise']['median_ms_per_step'] < res['dense']['median_ms_per_step'], 'the row-wise step must beat the dense step at this size'
