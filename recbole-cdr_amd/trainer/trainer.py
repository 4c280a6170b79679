"""CrossDomainTrainer: the caller of the hot path (recbole_cdr/trainer/trainer.py:18-76).

The reference subclasses third-party ``recbole.trainer.Trainer``; the part of it the phase loop relies on is restated
here (optimizer built ONCE and kept across phases, ``_train_epoch`` = zero_grad -> calculate_loss ->
(tuple => sum) -> nan check -> backward -> clip -> step, ``fit`` with eval_step / early stopping, ``evaluate`` =
full-sort scores -> mask PAD column and history -> top-k).  Metrics are computed on device with torch.topk (plumbing);
the dense optimizer is the one ``config['learner']`` names, as recbole's ``_build_optimizer`` builds it: the native exact Adam
(csrc/cdr_rows.hip ``cdr_adam_multi_dev``) by default, or SGD / Adagrad / RMSprop with torch's defaults (csrc/cdr_optim.hip
``cdr_opt_multi_dev``).
"""
import numpy as np
import torch

from ..utils import train_mode2state, total_loss as _total


class DenseAdam(torch.optim.Optimizer):
    """torch.optim.Adam semantics (amsgrad=False), each parameter updated by one native kernel launch.  The step count is
    a device scalar bumped by a kernel, so ``step()`` is hipGraph-capturable (graph_step.GraphedTrainStep)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        # (loss, loss_sum) device scalars handed over by the training loop before ``step()``: the launch that bumps the step counters
        # also adds this step's loss to the epoch's total (no launch of its own).  ``step`` sets it back to None once it has done so.
        self.loss_pair = None
        # cdr_batch_job's handed over by the training loop before ``step()`` (graph_step: the loader's NEXT batch): produced in workgroups
        # behind the update's own, in the same launch (cdr_adam_multi_dev_produce).  ``step`` sets it back to None once it has done so.
        self.produce_jobs = None

    @torch.no_grad()
    def step(self, closure=None):
        import ctypes
        from .. import binding as B_
        jobs, self.produce_jobs = self.produce_jobs, None
        try:
            self._step_groups(jobs)
        finally:
            jobs = self.__dict__.pop('_jobs_left', jobs)
            if jobs:                                   # no parameter had a gradient (or several groups): the batch is produced all the same
                from ..data.producer import launch_jobs
                launch_jobs(jobs)

    def _step_groups(self, jobs):
        import ctypes
        from .. import binding as B_
        self._jobs_left = jobs
        for group in self.param_groups:
            ps, gs, ms, vs, ns, ss, keep = [], [], [], [], [], [], []
            for p in group['params']:
                if p.grad is None:
                    continue                      # like torch: a parameter without a gradient keeps its own step count
                st = self.state[p]
                if not st:
                    st['step'] = torch.zeros(1, device=p.device, dtype=torch.int64)     # per-parameter, on device
                    st['exp_avg'] = torch.zeros_like(p)
                    st['exp_avg_sq'] = torch.zeros_like(p)
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                keep.append(g)
                ps.append(B_.f32(p.data)); gs.append(B_.f32(g)); ms.append(B_.f32(st['exp_avg'])); vs.append(B_.f32(st['exp_avg_sq']))
                ns.append(p.numel()); ss.append(B_.i64(st['step']))
                ps_dev = p.device
            if not ps:
                continue
            n = len(ps)
            arr = lambda xs: (ctypes.c_void_p * n)(*[x.value if hasattr(x, 'value') else x for x in xs])
            lp, self.loss_pair = self.loss_pair, None
            tk = self.__dict__.get('_ticket')
            if tk is None or tk.device != ps_dev:
                tk = self._ticket = torch.zeros(B_.SIGNIN_WORDS, device=ps_dev, dtype=torch.int32)        # sign-in words of the one-launch form
            jl = self._jobs_left
            if jl:
                self._jobs_left = None
                jarr = (B_.BatchJob * len(jl))(*jl)
                B_.call('cdr_adam_multi_dev_produce', B_.stream(), n, arr(ps), arr(gs), arr(ms), arr(vs), (ctypes.c_int64 * n)(*ns), arr(ss),
                        float(group['lr']), float(group['betas'][0]), float(group['betas'][1]), float(group['eps']),
                        float(group['weight_decay']), None if lp is None else B_.f32(lp[0]), None if lp is None else B_.f32(lp[1]), B_.raw(tk),
                        jarr, len(jl))
                continue
            B_.call('cdr_adam_multi_dev', B_.stream(), n, arr(ps), arr(gs), arr(ms), arr(vs), (ctypes.c_int64 * n)(*ns), arr(ss),
                    float(group['lr']), float(group['betas'][0]), float(group['betas'][1]), float(group['eps']),
                    float(group['weight_decay']), None if lp is None else B_.f32(lp[0]), None if lp is None else B_.f32(lp[1]), B_.raw(tk))


def _dense_adam_load(self, state_dict):
    """torch.optim.Adam checkpoints keep ``step`` as a Python float or a 0-d tensor: convert to this optimizer's device int64 [1]."""
    torch.optim.Optimizer.load_state_dict(self, state_dict)
    for p, st in self.state.items():
        if 'step' in st and not (torch.is_tensor(st['step']) and st['step'].dtype == torch.int64 and st['step'].numel() == 1
                                 and st['step'].dim() == 1):
            st['step'] = torch.full((1,), int(float(st['step'])), device=p.device, dtype=torch.int64)


DenseAdam.load_state_dict = _dense_adam_load


LEARNERS = ('adam', 'sgd', 'adagrad', 'rmsprop')       # config['learner'] values with a native optimizer ('sparse_adam' is refused)


class _DenseLearner(torch.optim.Optimizer):
    """What recbole's ``_build_optimizer`` builds for ``learner`` = sgd / adagrad / rmsprop -- ``torch.optim.<X>(params, lr=..,
    weight_decay=..)`` with torch's defaults for everything else -- on one native launch for all parameters (``cdr_opt_multi_dev``).
    None of the three has a bias correction: the launch reads no step count, so ``step()`` is hipGraph-capturable as it stands.
    ``state_dict()`` has torch's key names and param-group keys (``_STATE``: the state tensor; ``step``: a CPU float scalar as torch
    keeps it), so a checkpoint loads under ``torch.optim.<X>`` and back.  ``step`` is host bookkeeping only: a replayed graph runs no
    Python, ``on_replay`` counts its update for the parameters the captured step updated."""
    kind, _STATE = None, None

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self.loss_pair = None              # (loss, loss_sum) handed over before ``step()``, as for DenseAdam: added inside the update's launch
        self._last = ()                    # the parameters the last ``step()`` updated (``on_replay``)

    @torch.no_grad()
    def step(self, closure=None):
        import ctypes
        from .. import binding as B_
        last = []
        for group in self.param_groups:
            ps, gs, ss, ns, keep = [], [], [], [], []
            for p in group['params']:
                if p.grad is None:
                    continue                      # like torch: a parameter without a gradient is skipped
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                keep.append(g)
                ps.append(B_.f32(p.data)); gs.append(B_.f32(g)); ns.append(p.numel())
                if self._STATE is not None:
                    st = self.state[p]
                    if not st:
                        st['step'] = torch.tensor(0.0)
                        st[self._STATE] = torch.zeros_like(p)
                    if not (p.is_cuda and torch.cuda.is_current_stream_capturing()):      # (a capture records the launch: no update runs)
                        st['step'] += 1
                    ss.append(B_.f32(st[self._STATE]))
                last.append(p)
            if not ps:
                continue
            n = len(ps)
            arr = lambda xs: (ctypes.c_void_p * n)(*[x.value if hasattr(x, 'value') else x for x in xs])
            lp, self.loss_pair = self.loss_pair, None
            B_.call('cdr_opt_multi_dev', B_.stream(), self._code(), n, arr(ps), arr(gs), arr(ss) if ss else None,
                    (ctypes.c_int64 * n)(*ns), float(group['lr']), float(group.get('alpha', 0.0)), float(group.get('eps', 0.0)),
                    float(group['weight_decay']), None if lp is None else B_.f32(lp[0]), None if lp is None else B_.f32(lp[1]))
        self._last = tuple(last)

    def _code(self):
        from ..fused import OPT_NAMES                      # (the package's one table of CDR_OPT_* codes)
        return {name: code for code, name in OPT_NAMES.items()}[self.kind]

    def state_dict(self):
        """torch.optim.Adagrad / RMSprop create ``step`` and the state tensor of EVERY parameter in ``__init__`` and their ``step()`` reads
        them without a check; this class creates them at a parameter's first gradient.  So that a checkpoint written in between (EMCDR
        after its SOURCE phase: the target tables have had no gradient yet) steps under torch's class, an optimizer that has updated
        anything writes a zero state tensor and ``step`` 0 for the parameters it has not -- what torch holds for them.  One that has
        updated nothing (the unused dense optimizer of optimizer_mode='rowwise') writes an empty state: no table-sized zeros."""
        sd = super().state_dict()
        if self._STATE is None or not sd['state']:
            return sd
        i = 0
        for g in self.param_groups:
            for p in g['params']:
                if i not in sd['state']:
                    sd['state'][i] = {'step': torch.tensor(0.0), self._STATE: torch.zeros_like(p)}
                i += 1
        return sd

    def on_replay(self):
        if self._STATE is not None:
            for p in self._last:
                self.state[p]['step'] += 1

    def load_state_dict(self, state_dict):
        """A checkpoint of this class or of ``torch.optim.<X>``; ``step`` comes back as the CPU float scalar torch keeps (a checkpoint
        loaded with ``map_location`` hands it over on the device)."""
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if 'step' in st:
                st['step'] = torch.tensor(float(st['step']))


def _refuse(name, **must):
    for k, (got, want) in must.items():
        if got != want:
            raise ValueError(f'{name}: {k}={got!r} is not supported (only {want!r}: the reference builds its optimizer with torch defaults)')


class DenseSGD(_DenseLearner):
    """``torch.optim.SGD(params, lr, weight_decay=wd)``: no momentum.  g += wd p; p -= lr g."""
    kind = 'sgd'

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0.0, nesterov=False):
        _refuse('DenseSGD', momentum=(momentum, 0), dampening=(dampening, 0), nesterov=(nesterov, False))
        super().__init__(params, dict(lr=lr, momentum=0, dampening=0, weight_decay=weight_decay, nesterov=False, maximize=False, foreach=None,
                                      differentiable=False, fused=None))


class DenseAdagrad(_DenseLearner):
    """``torch.optim.Adagrad(params, lr, weight_decay=wd)``: lr_decay = 0, initial_accumulator_value = 0, eps = 1e-10.
    g += wd p; sum += g g; p -= lr g / (sqrt(sum) + eps)."""
    kind, _STATE = 'adagrad', 'sum'

    def __init__(self, params, lr=1e-2, lr_decay=0, weight_decay=0.0, initial_accumulator_value=0, eps=1e-10):
        _refuse('DenseAdagrad', lr_decay=(lr_decay, 0), initial_accumulator_value=(initial_accumulator_value, 0))
        super().__init__(params, dict(lr=lr, lr_decay=0, eps=eps, weight_decay=weight_decay, initial_accumulator_value=0, foreach=None,
                                      maximize=False, differentiable=False, fused=None))


class DenseRMSprop(_DenseLearner):
    """``torch.optim.RMSprop(params, lr, weight_decay=wd)``: alpha = 0.99, eps = 1e-8, not centered, no momentum.
    g += wd p; square_avg = alpha square_avg + (1 - alpha) g g; p -= lr g / (sqrt(square_avg) + eps)."""
    kind, _STATE = 'rmsprop', 'square_avg'

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0, centered=False):
        _refuse('DenseRMSprop', momentum=(momentum, 0), centered=(centered, False))
        super().__init__(params, dict(lr=lr, momentum=0, alpha=alpha, eps=eps, centered=False, weight_decay=weight_decay, capturable=False,
                                      foreach=None, maximize=False, differentiable=False))


def dense_optimizer(learner, params, lr, weight_decay):
    """The native dense optimizer of ``learner`` with torch's defaults, as recbole's ``_build_optimizer`` builds it."""
    cls = {'adam': DenseAdam, 'sgd': DenseSGD, 'adagrad': DenseAdagrad, 'rmsprop': DenseRMSprop}[learner]
    return cls(params, lr=lr, weight_decay=weight_decay)


def resolve_learner(config):
    """config['learner'] -> one of LEARNERS (default 'adam', case-insensitive).  'sparse_adam' is refused: the tables are dense
    parameters, and torch.optim.SparseAdam refuses dense gradients too.  Any other name: a warning and Adam, as recbole does."""
    name = config['learner'] if 'learner' in config and config['learner'] is not None else 'adam'
    name = str(name).lower()
    if name == 'sparse_adam':
        raise ValueError("learner='sparse_adam' is not supported: the embedding tables are dense parameters with dense gradients, which "
                         "torch.optim.SparseAdam refuses too; use 'adam', or optimizer_mode='rowwise' for an O(batch) update")
    if name not in LEARNERS:
        import warnings
        warnings.warn(f'Received unrecognized optimizer {name!r}, set default Adam optimizer', stacklevel=3)
        return 'adam'
    return name


class RowAwareAdam(DenseAdam):
    """``DenseAdam`` for a model whose embedding tables take the deferred row-wise form of the SAME optimizer
    (``model.enable_deferred_adam``; lazyadam.DeferredRowAdam: exact dense-Adam results, O(batch) traffic).  ``step()`` = the
    dense kernels for every parameter that has a ``.grad`` (the MLP / mapping weights) + the row-wise update of the tables the
    model's backward left pending.  Drop-in for the reference's loop: zero_grad -> calculate_loss -> backward -> step."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(model.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.row_opt = model.enable_deferred_adam(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)

    @torch.no_grad()
    def step(self, closure=None):
        super().step(closure)
        self.row_opt.step()

    def on_replay(self):
        self.row_opt.on_replay()

    def state_dict(self):
        """The layout ``torch.optim.Adam.state_dict()`` writes -- the tables' flushed moments and update count under the standard
        per-parameter 'state' entries -- so that a checkpoint resumes under DenseAdam, torch.optim.Adam or this class alike
        (the moments used to sit under an extra key that the dense loaders silently ignored)."""
        sd = super().state_dict()
        rows = self.row_opt.state_dict()                                  # (flushes: every row at the current update)
        index, i = {}, 0
        for g in self.param_groups:
            for p_ in g['params']:
                index[id(p_)] = i
                i += 1
        for t, m, v in zip(self.row_opt.tables, rows['exp_avg'], rows['exp_avg_sq']):
            sd['state'][index[id(t)]] = {'step': torch.full((1,), int(rows['step']), device=t.device, dtype=torch.int64),
                                         'exp_avg': m, 'exp_avg_sq': v}
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        rows = sd.pop('deferred_rows', None)
        super().load_state_dict(sd)
        if rows is not None:                          # (checkpoints written before round 5 kept the tables' moments under this key)
            self.row_opt.load_state_dict(rows)
            return
        # a checkpoint written by DenseAdam / torch.optim.Adam: the tables' moments sit in the per-parameter state -- take them over
        # (a dense optimizer leaves every row at the same update count, which is what the row-wise form resumes from)
        ro = self.row_opt
        got = [self.state.get(t) for t in ro.tables]
        if all(st and 'exp_avg' in st for st in got):
            steps = {int(float(st['step'])) for st in got}
            if len(steps) != 1:
                raise ValueError('RowAwareAdam.load_state_dict: the tables carry different update counts (%s); the deferred row-wise '
                                 'form keeps ONE count for its tables' % sorted(steps))
            ro.load_state_dict({'step': steps.pop(), 'exp_avg': [st['exp_avg'] for st in got], 'exp_avg_sq': [st['exp_avg_sq'] for st in got]})
            for t in ro.tables:
                self.state.pop(t, None)
        elif any(st and 'exp_avg' in st for st in got):
            raise ValueError('RowAwareAdam.load_state_dict: optimizer state for only some of the embedding tables')


def early_stopping(value, best, cur_step, max_step, bigger=True):
    """recbole.utils.early_stopping."""
    stop_flag, update_flag = False, False
    if (bigger and value >= best) or (not bigger and value <= best):
        cur_step, best, update_flag = 0, value, True
    else:
        cur_step += 1
        if cur_step > max_step:
            stop_flag = True
    return best, cur_step, stop_flag, update_flag


DEFAULT_METRICS = ('recall', 'hit', 'precision', 'mrr', 'ndcg')     # what evaluate returned before config['metrics'] was read
TOPK_METRICS = ('recall', 'mrr', 'ndcg', 'hit', 'precision', 'map')  # keys name@k
VALUE_METRICS = ('auc', 'mae', 'rmse', 'logloss')
# recbole's non-accuracy metrics (keys name@k): the only ones that need to know WHICH items are in the lists, so they are answered by the
# list route alone -- the lists of the mask + top-k kernels (k <= 1024) folded on the device by functional.ListStats, batch after batch --
# and they need the training set's item counts over the evaluated loader's column space: config['item_counts'] (data.train_item_counts of
# the target domain's training pairs), or the loader's own ``item_counts`` attribute.  tailpercentage reads config['tail_ratio'] (0.1).
NON_ACCURACY_METRICS = ('itemcoverage', 'averagepopularity', 'shannonentropy', 'giniindex', 'tailpercentage')
FUSED_TOPK_MAX = 64                   # the fused mask + top-k kernels keep a list in one wave: k <= 64
WIDE_TOPK_MAX = 1024                  # the wide mask + top-k behind them (model.full_sort_topk_wide): k <= 1024


def resolve_metrics(config):
    """config['metrics'] as recbole reads it (a name or a list of names, any letter case) -> tuple of lower-case names, or None when the
    key is absent (evaluate then returns what it always did).  Refused here, before anything is built: recbole's value metrics (they need
    the labeled evaluation mode), its non-accuracy metrics unless config['item_counts'] is given (they need the training set's item
    counts), unknown names."""
    if 'metrics' not in config or config['metrics'] is None:
        return None
    names = config['metrics']
    names = [names] if isinstance(names, str) else list(names)
    out = []
    for n in names:
        m = str(n).lower()
        if m in VALUE_METRICS:
            raise ValueError(f"metrics: {n!r} is a value metric: it needs recbole's labeled evaluation mode, which this trainer does not "
                             f"have (full-sort ranking only)")
        if m in NON_ACCURACY_METRICS and ('item_counts' not in config or config['item_counts'] is None):
            raise ValueError(f"metrics: {n!r} is a non-accuracy metric: it needs the training set's item counts, which evaluate() is not "
                             f"given: set config['item_counts'] (data.train_item_counts of the target domain's training pairs)")
        if m not in TOPK_METRICS and m not in NON_ACCURACY_METRICS and m != 'gauc':
            raise ValueError(f"metrics: unknown metric {n!r}; supported: {', '.join(TOPK_METRICS + NON_ACCURACY_METRICS)} (keys name@k) "
                             f"and gauc")
        if m not in out:
            out.append(m)
    if not out:
        raise ValueError('metrics: the list is empty')
    return tuple(out)


def resolve_eval_mode(config):
    """config['eval_args']['mode'] as recbole's ``Config._set_eval_neg_sample_args`` reads it -> (strategy, sample_by, distribution):
    absent or 'full' -> ('full', None, 'uniform'); 'uniN' -> ('by', N, 'uniform'); 'popN' -> ('by', N, 'popularity'), N a positive integer.
    Case-sensitive, as recbole is ('Uni5' is refused).  'labeled' and everything else raise ValueError, before anything is built."""
    args = config['eval_args'] if 'eval_args' in config and config['eval_args'] is not None else {}
    mode = args['mode'] if 'mode' in args and args['mode'] is not None else 'full'
    if mode == 'full':
        return 'full', None, 'uniform'
    if mode == 'labeled':
        raise ValueError("the mode [labeled] in eval_args is not provided: labeled evaluation and the value metrics (auc, mae, rmse, "
                         "logloss) need label-carrying evaluation data and training without negative sampling; use full, uniN or popN")
    if isinstance(mode, str) and mode[:3] in ('uni', 'pop') and mode[3:].isascii() and mode[3:].isdigit() and int(mode[3:]) > 0:
        return 'by', int(mode[3:]), 'uniform' if mode[:3] == 'uni' else 'popularity'
    raise ValueError(f'the mode [{mode}] in eval_args is not supported.')


def resolve_eval_route(config, metrics):
    """config['eval_route'] ('auto' | 'topk' | 'rank'): which of the two FULL-SORT routes a full-sort loader takes.  It does not concern a
    sampled-candidate loader (``eval_mode = 'sampled'``), which always ranks its positives inside the candidate lists."""
    route = config['eval_route'] if 'eval_route' in config and config['eval_route'] is not None else 'auto'
    if route not in ('auto', 'topk', 'rank'):
        raise ValueError(f"eval_route must be 'auto', 'topk' or 'rank', got {route!r}")
    if route == 'topk' and metrics is not None and 'gauc' in metrics:
        raise ValueError("eval_route='topk' cannot answer gauc: a top-k list does not hold the rank of every positive over the whole "
                         "catalogue; use eval_route='rank' or 'auto'")
    return route


def metrics_from_hits(hit, n_pos, topk, names=DEFAULT_METRICS):
    """{name@k: value} from the hit matrix [U, kmax] (hit[u, j] = 1 where position j of user u's ranking is a ground-truth positive) and
    the positives per user ``n_pos`` [U] (clamped to >= 1 by the caller): recbole's Recall / Hit / Precision / MRR / NDCG / MAP, averaged
    over the users.  The one copy of this arithmetic: both evaluation routes end here."""
    kmax = hit.shape[1]
    result = {}
    ranks = torch.arange(1, kmax + 1, device=hit.device, dtype=torch.float32)
    for k in topk:
        h = hit[:, :k]
        for name in names:
            if name == 'recall':
                value = (h.sum(1) / n_pos).mean()
            elif name == 'hit':
                value = (h.sum(1) > 0).float().mean()
            elif name == 'precision':
                value = (h.sum(1) / k).mean()
            elif name == 'mrr':
                value = (h * (1.0 / ranks[:k])).max(1).values.mean()
            elif name == 'ndcg':
                dcg = (h / torch.log2(ranks[:k] + 1)).sum(1)
                ideal = torch.cumsum(1.0 / torch.log2(ranks[:k] + 1), 0)
                idcg = ideal[(n_pos.clamp(max=k).long() - 1)]
                value = (dcg / idcg).mean()
            elif name == 'map':
                # recbole MAP: the mean of precision@j over the hit positions j <= k, divided by min(n_pos, k)
                pre = torch.cumsum(h, 1) / ranks[:k]
                value = ((pre * h).sum(1) / n_pos.clamp(max=k)).mean()
            else:
                continue                                   # (gauc has no @k: gauc_from_counts)
            result[f'{name}@{k}'] = float(value)
    return result


def gauc_from_counts(pos_len, user_len, rank_sum):
    """recbole's GAUC in float64 from per-user integers: ``pos_len`` positives, ``user_len`` unmasked items (positives included),
    ``rank_sum`` = the sum of the positives' average ranks gt + (eq + 1) / 2 (descending order, 1 = best, ties share the mean position).
    pair = (user_len + 1) pos_len - pos_len (pos_len + 1) / 2 - rank_sum counts the (positive, negative) pairs in the right order, ties
    half; auc_u = pair / (neg pos_len); users without positives or without negatives are dropped; the mean is pos_len-weighted."""
    pos_len, user_len, rank_sum = pos_len.double(), user_len.double(), rank_sum.double()
    neg = user_len - pos_len
    keep = (pos_len > 0) & (neg > 0)
    if not bool(keep.any()):
        return float('nan')
    pos_len, neg, user_len, rank_sum = pos_len[keep], neg[keep], user_len[keep], rank_sum[keep]
    pair = (user_len + 1) * pos_len - pos_len * (pos_len + 1) / 2 - rank_sum
    return float((pair / (neg * pos_len) * pos_len).sum() / pos_len.sum())


def rank_counts_reference(scores, pos_rows, pos_cols):
    """The counts of ``functional.fullsort_rank`` in plain torch over a materialised, already masked matrix (masked entries NaN): what the
    trainer uses where there is no device to run the kernel on (``device: cpu``)."""
    valid = ~torch.isnan(scores)
    t = scores[pos_rows, pos_cols]
    rows, ok = scores[pos_rows], valid[pos_rows]
    col = torch.arange(scores.shape[1], device=scores.device).unsqueeze(0)
    gt = ((rows > t.unsqueeze(1)) & ok).sum(1)
    same = (rows == t.unsqueeze(1)) & ok
    eq, eqb = same.sum(1), (same & (col < pos_cols.unsqueeze(1))).sum(1)
    bad = torch.isnan(t)
    gt, eq, eqb = (torch.where(bad, torch.full_like(x, -1), x).to(torch.int32) for x in (gt, eq, eqb))
    return t, gt, eq, eqb, valid.sum(1).to(torch.int32)


class Trainer:
    metrics = None                    # (class defaults: objects built without __init__ evaluate as before)
    list_metrics = ()
    eval_route = 'auto'
    learner = 'adam'                  # (class default, as rowwise_adam below)
    rowwise_adam = 'lazy'             # (class default: loops driven on objects built without __init__ keep the lazy row-wise Adam)

    def __init__(self, config, model):
        self.config, self.model = config, model
        self.learning_rate = config['learning_rate'] if 'learning_rate' in config else 1e-3
        self.epochs = int(config['epochs']) if 'epochs' in config else 1
        self.eval_step = min(config['eval_step'] if 'eval_step' in config else 1, self.epochs)
        self.stopping_step = config['stopping_step'] if 'stopping_step' in config else 10
        self.clip_grad_norm = config['clip_grad_norm'] if 'clip_grad_norm' in config else None
        self.valid_metric = (config['valid_metric'] if 'valid_metric' in config else 'MRR@10').lower()
        self.valid_metric_bigger = config['valid_metric_bigger'] if 'valid_metric_bigger' in config else True
        self.topk = config['topk'] if 'topk' in config else [10]
        # config['metrics'] (absent: recall / hit / precision / mrr / ndcg, as always) and config['eval_route']: 'auto' keeps the model's
        # mask + top-k route whenever it can answer (no gauc, and max(topk) <= 64 or the route is unfused), 'rank' derives every metric
        # from the rank of each positive over the masked catalogue (model.full_sort_rank: any k, MAP, GAUC), 'topk' insists on the lists
        # (max(topk) <= 1024; above 64 on a GPU they come from model.full_sort_topk_wide)
        self.metrics = resolve_metrics(config)
        self.eval_route = resolve_eval_route(config, self.metrics)
        # config['eval_args']['mode'] (full | uniN | popN): which evaluation loader data.dataloader.eval_loader_for builds for the target
        # domain; evaluate() itself dispatches on the loader it is handed.  A mode that is not provided is refused here
        self.eval_mode = resolve_eval_mode(config)
        self.device = config['device']
        # the non-accuracy metrics among config['metrics'] (NON_ACCURACY_METRICS): what they cannot be combined with is refused here
        self.list_metrics = tuple(m for m in (self.metrics or ()) if m in NON_ACCURACY_METRICS)
        self.item_counts = None
        if self.list_metrics:
            self.item_counts = self._check_list_metrics(config)
        self.weight_decay = config['weight_decay'] if 'weight_decay' in config else 0.0
        self.start_epoch, self.cur_step = 0, 0
        self.best_valid_score = -np.inf if self.valid_metric_bigger else np.inf
        self.best_valid_result = None
        self.train_loss_dict = dict()
        # 'dense'   : the reference's literal loop -- autograd into table-sized gradients + Adam over every parameter
        # 'rowwise' : the model's O(batch) fused step (tables too large for dense gradients, e.g. BASELINE config C5)
        self.optimizer_mode = config['optimizer_mode'] if 'optimizer_mode' in config else 'dense'
        on_gpu = torch.device(self.device).type == 'cuda'
        # config['learner'] (recbole Trainer._build_optimizer: adam | sgd | adagrad | rmsprop, torch defaults beyond lr and weight_decay;
        # default 'adam').  Every refusal comes before any optimizer or state object exists.
        self.learner = resolve_learner(config)
        if self.optimizer_mode == 'rowwise' and self.learner == 'rmsprop':
            raise ValueError("learner='rmsprop' is not available with optimizer_mode='rowwise': an untouched row's square_avg decays "
                             "every step (square_avg *= alpha), so a lazy row-wise form that leaves untouched rows alone is not the "
                             "optimizer asked for; use optimizer_mode='dense'")
        if self.learner == 'adagrad' and 'dist_group' in config and config['dist_group'] not in (None, False):
            raise ValueError("learner='adagrad' is not available with dist_group: the sharded steps implement SGD and Adam only")
        if self.learner != 'adam' and self.optimizer_mode == 'rowwise' and 'rowwise_adam' in config and config['rowwise_adam'] == 'exact':
            raise ValueError(f"rowwise_adam='exact' is the reference's dense Adam: it needs learner='adam', got {self.learner!r}")
        # The reference's Adam over every parameter.  A model that offers ``enable_deferred_adam`` (CoNet on its fused tower kernels)
        # gets the SAME optimizer with its embedding tables evaluated lazily per row -- bit-identical to the dense sweep
        # (lazyadam.py), O(batch) instead of O(table) traffic per step.  config['deferred_adam'] = False keeps the literal sweep;
        # gradient clipping needs the whole gradient, so it does too.
        deferred = (config['deferred_adam'] if 'deferred_adam' in config else True) and self.optimizer_mode == 'dense' and on_gpu \
            and not self.clip_grad_norm and hasattr(self.model, 'enable_deferred_adam') and getattr(self.model, 'fused_towers', True) \
            and all(p.is_cuda for p in self.model.parameters())
        if self.learner != 'adam':
            # built once and kept across phases, like the Adam below; the deferred row-wise form is Adam's alone (CoNet then takes its
            # plain dense route)
            self.optimizer = dense_optimizer(self.learner, self.model.parameters(), self.learning_rate, self.weight_decay)
        elif deferred:
            self.optimizer = RowAwareAdam(self.model, lr=self.learning_rate, weight_decay=self.weight_decay)
        else:
            self.optimizer = DenseAdam(self.model.parameters(), lr=self.learning_rate, weight_decay=self.weight_decay)
        # Dense mode on a GPU: each (phase, batch shape) is captured ONCE as a hipGraph -- batch production by the device loader,
        # calculate_loss, backward, optimizer -- and an epoch is a run of replays (graph_step.GraphedTrainStep); ragged tails and
        # models whose loss needs the host (``model.graph_key()`` is None) take the eager loop below.  config['graph_step'] = False
        # switches it off.
        self.graph_step = bool(config['graph_step'] if 'graph_step' in config else True) and on_gpu and self.optimizer_mode == 'dense' \
            and not self.clip_grad_norm
        # ... and rowwise mode on a device loader: {producer -> model.fused_train_step -> loss total} replayed where the model says its fused
        # step is capturable (model.fused_graph_key)
        self.graph_step_rowwise = bool(config['graph_step'] if 'graph_step' in config else True) and on_gpu and self.optimizer_mode == 'rowwise'
        # steps per graph launch on a device loader (the idle time between two graph launches is ~5-9 us: amortised over this many steps)
        # config['graph_unroll']; default 8 -- 16 for a step that runs software-pipelined over two streams (below): a two-stream graph's launch
        # boundary costs ~30-40 us of idle chip, 8 steps per graph leave ~4 us of it in every step (C3: 0.1535 -> 0.149 ms; 32: 0.1475;
        # the single-stream steps of C1 / C2 / C4 gain <= 1.5 % and keep 8 -- an epoch's tail of < unroll steps runs one step per launch)
        self.graph_unroll = int(config['graph_unroll']) if 'graph_unroll' in config else None
        # ... and, for models that can run part of the next step ahead (CoNet on the deferred Adam), those steps software-pipelined over two streams
        gp = config['graph_pipeline'] if 'graph_pipeline' in config else True
        self.graph_pipeline = gp if isinstance(gp, str) else bool(gp)          # True (one batch ahead) | 'two_ahead' | False
        self._graphs = {}
        self._loss_sum = None
        self.graph_stats = {'replayed': 0, 'eager': 0, 'captures': 0}
        # evaluation through the model's fused mask + top-k kernel when it has one (False: full score matrix + torch.topk)
        self.fused_topk = config['fused_topk'] if 'fused_topk' in config else True
        # config['dist_group'] (a torch.distributed group, or True for WORLD) with optimizer_mode='rowwise': the model's tables are
        # sharded over the group's GPUs; every rank runs the SAME loaders and trains on rows rank::world of every batch (a ragged
        # tail of < world rows is skipped, as a DistributedSampler(drop_last=True) would); evaluation is replicated.
        self.dist_group = None
        if 'dist_group' in config and config['dist_group'] not in (None, False):
            import torch.distributed as dist
            self.dist_group = dist.group.WORLD if config['dist_group'] is True else config['dist_group']
            if self.optimizer_mode != 'rowwise':
                raise ValueError("dist_group needs optimizer_mode='rowwise' (small-table models: dp.ShardedDataParallel)")
        if self.optimizer_mode not in ('dense', 'rowwise'):
            raise ValueError(f"optimizer_mode must be 'dense' or 'rowwise', got {self.optimizer_mode!r}")
        if self.optimizer_mode == 'rowwise' and not hasattr(self.model, 'fused_train_step'):
            raise NotImplementedError(f'{type(self.model).__name__} has no fused_train_step; use optimizer_mode=dense')
        # config['rowwise_adam'] with optimizer_mode='rowwise': 'lazy' (default) -- rows a batch does not touch keep their state -- or
        # 'exact': the reference's Adam over whole tables (recbole_cdr/properties/overall.yaml:20-21), evaluated per row by a catch-up launch
        # in front of every fused step; the tables are brought up to date (model.fused_sync) before evaluation, checkpoints and the end of fit
        self.rowwise_adam = config['rowwise_adam'] if 'rowwise_adam' in config and config['rowwise_adam'] is not None else 'lazy'
        if self.rowwise_adam not in ('lazy', 'exact'):
            raise ValueError(f"rowwise_adam must be 'lazy' or 'exact', got {self.rowwise_adam!r}")
        if self.rowwise_adam == 'exact':
            if self.optimizer_mode != 'rowwise':
                raise ValueError("rowwise_adam='exact' applies to optimizer_mode='rowwise' (optimizer_mode='dense' already runs the dense Adam)")
            if self.dist_group is not None:
                raise ValueError("rowwise_adam='exact' is not available with dist_group (sharded tables)")
            if not hasattr(self.model, 'fused_sync'):
                raise NotImplementedError(f"{type(self.model).__name__}.fused_train_step has no rowwise_adam='exact' mode")
        if self.optimizer_mode == 'rowwise' and self.clip_grad_norm:
            # the fused step never materialises the gradient, so there is no norm to clip: refuse rather than ignore silently
            raise ValueError("clip_grad_norm is not supported with optimizer_mode='rowwise' (the fused step applies per-row updates "
                             "without forming the full gradient); use optimizer_mode='dense' or unset clip_grad_norm")
        if 'parallel_domains' in config and config['parallel_domains'] and self.dist_group is not None:
            import warnings
            warnings.warn('parallel_domains: the SOURCE and TARGET phases of a parallel stage run WITHOUT validation, early stopping, '
                          'best_valid_score updates and callback_fn (evaluation needs every rank); later phases evaluate as usual',
                          stacklevel=2)

    def _check_list_metrics(self, config):
        """The refusals of the non-accuracy metrics; returns config['item_counts'] as an int64 vector on the trainer's device."""
        what = f"metrics {', '.join(self.list_metrics)}"
        if self.eval_route == 'rank':
            raise ValueError(f"{what}: eval_route='rank' holds no list -- the rank of a positive does not say which items were recommended; "
                             f"use eval_route='auto' or 'topk'")
        if max(self.topk) > WIDE_TOPK_MAX:
            raise ValueError(f"{what}: the mask + top-k lists hold k <= {WIDE_TOPK_MAX}, topk asks for {max(self.topk)}")
        if self.eval_mode[0] != 'full':
            raise ValueError(f"{what}: eval_args mode {config['eval_args']['mode']!r} ranks the positives inside sampled candidate lists, "
                             f"whose positions are not recommendations over the catalogue; use mode 'full'")
        if 'dist_group' in config and config['dist_group'] not in (None, False):
            raise ValueError(f"{what}: not available with dist_group (the lists are counted on one GPU only, as on the rank route)")
        return self._as_item_counts(config['item_counts'])

    def _as_item_counts(self, counts):
        counts = torch.as_tensor(counts)
        if counts.dim() != 1 or counts.numel() == 0 or counts.dtype.is_floating_point or counts.dtype == torch.bool:
            raise ValueError("item_counts must be a non-empty 1-D integer tensor or array: the training-set count of every column of the "
                             "evaluated loader (data.train_item_counts)")
        return counts.to(device=self.device, dtype=torch.int64)

    def _list_stats_for(self, eval_data):
        """The ``functional.ListStats`` of one evaluate call when a non-accuracy metric is asked (None otherwise): the loader's own
        ``item_counts`` ahead of config['item_counts'], the tail set of config['tail_ratio'] when tailpercentage is asked."""
        if not self.list_metrics:
            return None
        from .. import functional as F_
        from ..data.popularity import tail_items
        own = getattr(eval_data, 'item_counts', None)
        counts = self._as_item_counts(own) if own is not None else self.item_counts
        tail = None
        if 'tailpercentage' in self.list_metrics:
            tail = tail_items(counts, self.config['tail_ratio'] if 'tail_ratio' in self.config else None)
        return F_.ListStats(counts, self.topk, tail_mask=tail)

    # ---- dense mode, one hipGraph replay per step --------------------------------------------------------------------------------
    def _graph_for(self, key, example=None, producer=None):
        """The captured step for ``key`` (built on first use; False once a capture has failed: that key stays eager)."""
        gs = self._graphs.get(key)
        if gs is None:
            from ..graph_step import GraphedTrainStep
            try:
                unroll = self.graph_unroll
                if unroll is None:
                    pipelined = (producer is not None and bool(self.graph_pipeline) and hasattr(self.model, 'prepare_batch')
                                 and hasattr(self.model, 'apply_rows_early') and getattr(self.optimizer, 'row_opt', None) is not None)
                    unroll = 16 if pipelined else 8
                gs = GraphedTrainStep(self.model, self.optimizer, example, producer=producer, loss_sum=self._loss_sum,
                                      unroll=unroll, pipeline=self.graph_pipeline)
                self.graph_stats['captures'] += 1
            except Exception as e:                                      # noqa: BLE001 -- reported, and the eager loop still trains
                import warnings
                back = 'parameters / optimizer state / loader counters restored to their values before the warm-up' \
                    if getattr(e, 'state_restored', False) else 'the warm-up steps that ran before the failure stay applied'
                warnings.warn(f'hipGraph capture of the training step failed for {key!r} ({type(e).__name__}: {e}); running it eagerly ({back})')
                gs = False
            self._graphs[key] = gs
        return gs

    def _eager_step(self, interaction):
        self.optimizer.zero_grad(set_to_none=True)
        losses = self.model.calculate_loss(interaction)
        loss = _total(losses)
        loss = loss.reshape(()) if loss.numel() == 1 else loss.sum()
        loss.backward()
        from ..graph_step import step_and_sum
        step_and_sum(self.optimizer, loss.detach(), self._loss_sum)
        self.graph_stats['eager'] += 1

    def _train_epoch_graphed(self, train_data, mkey):
        """recbole ``Trainer._train_epoch`` (zero_grad -> calculate_loss -> backward -> step per batch) with every full-shape batch
        served by ONE hipGraph replay.  With a device loader (``train_data.device_producer()``) the replay also produces the batch
        -- slice of the shuffled interactions, tiling, negative sampling -- so the host's part of a step is the replay call; the
        loader's own ``__next__`` serves what a capture cannot (ragged tails, the BOTH-mode source wrap) and ends the epoch."""
        if self._loss_sum is None:
            self._loss_sum = torch.zeros((), device=self.device, dtype=torch.float32)
        self._loss_sum.zero_()
        state = getattr(train_data, 'state', None)
        it = iter(train_data)                                  # (epoch shuffle; in place once a producer has pinned the columns)
        prod = train_data.device_producer() if hasattr(train_data, 'device_producer') else None
        if prod is not None:
            prod.resync()
            key = (mkey, state, 'device-loader')
            while True:
                gs = self._graphs.get(key)
                if prod.full_ahead() and gs is not False:
                    if gs is None:
                        gs = self._graph_for(key, producer=prod)
                        if gs is False:
                            prod.resync()
                            continue
                    k = gs.unroll
                    if k > 1 and prod.full_count() >= k:
                        gs.replay_many()                          # k steps, one graph launch
                        prod.advance(k)
                        self.graph_stats['replayed'] += k
                        continue
                    gs.replay()
                    prod.advance()
                    self.graph_stats['replayed'] += 1
                    continue
                try:
                    interaction = next(it)
                except StopIteration:
                    break
                self._eager_step(interaction)
                prod.resync()
        else:
            for interaction in it:
                interaction = interaction.to(self.device)
                sig = tuple((k, tuple(v.shape), str(v.dtype)) for k, v in interaction.items())
                key = (mkey, state, sig, getattr(interaction, 'k_major', None))
                gs = self._graphs.get(key)
                if gs is None and not any(k[:2] == key[:2] for k in self._graphs):
                    gs = self._graph_for(key, example=interaction)         # the first batch shape of this (model key, loader state)
                if gs and gs.matches(interaction):
                    gs.step(interaction)
                    self.graph_stats['replayed'] += 1
                else:
                    self._eager_step(interaction)                          # ragged tail (another shape), or a failed capture
        if self.graph_stats['replayed'] and hasattr(self.model, 'on_train_steps'):
            self.model.on_train_steps()                                    # replays ran no model Python: host-side caches are stale now
        value = float(self._loss_sum)
        if value != value:
            raise ValueError('Training loss is nan')
        return value

    def _train_epoch(self, train_data, epoch_idx):
        self.model.train()
        if self.graph_step and self.optimizer_mode == 'dense' and self.dist_group is None:
            mkey = self.model.graph_key() if hasattr(self.model, 'graph_key') else None
            if mkey is not None:
                return self._train_epoch_graphed(train_data, mkey)
        total = None                              # accumulated on device: no per-step host sync
        if self.optimizer_mode == 'rowwise' and self.dist_group is None and hasattr(train_data, 'device_producer'):
            prod = train_data.device_producer()
            if prod is not None:
                return self._train_epoch_rowwise_produced(train_data, prod)
        for interaction in train_data:
            interaction = interaction.to(self.device)
            if self.dist_group is not None:
                interaction = self._my_rows(interaction)
            if self.optimizer_mode == 'rowwise':
                loss = self.model.fused_train_step(interaction, **self._fused_kw())
                total = loss.detach().clone() if total is None else total + loss.detach()
                continue
            self.optimizer.zero_grad()
            losses = self.model.calculate_loss(interaction)
            loss = _total(losses)
            loss = loss.reshape(()) if loss.numel() == 1 else loss.sum()   # (a [1]-shaped loss: a view, not a reduction launch)
            loss.backward()
            if self.clip_grad_norm:
                torch.nn.utils.clip_grad_norm_(self.model.parameters(), **self.clip_grad_norm)
            self.optimizer.step()
            total = loss.detach() if total is None else total + loss.detach()
        value = float(total) if total is not None else 0.0
        if value != value:
            raise ValueError('Training loss is nan')
        return value

    def _train_epoch_rowwise_produced(self, train_data, prod):
        """The rowwise loop on a device loader: every full batch is ONE producer launch (slice of the shuffled interactions + tiling +
        negative sampling into fixed buffers, data/producer.py) followed by the model's fused O(batch) step; the loader's own
        ``__next__`` serves ragged tails and ends the epoch.  (The fused steps of large batches read host-side update counts, so
        they are launched, not replayed; at >= 1 M rows per step the host's part is < 2 % of the step.)"""
        if self._loss_sum is None:
            self._loss_sum = torch.zeros((), device=self.device, dtype=torch.float32)
        self._loss_sum.zero_()
        it = iter(train_data)
        prod.resync()
        # full batches of a capturable phase (model.fused_graph_key): the first two run eagerly on the capture stream -- real steps, they
        # create every buffer and context the capture needs -- then {producer -> fused step -> loss total} is replayed, 4 steps per launch
        gkw = {'adam': 'exact'} if self.rowwise_adam == 'exact' else {}
        if self.learner != 'adam':
            gkw['opt'] = self.learner
        gkey = self.model.fused_graph_key(prod.fields, **gkw) if (self.graph_step_rowwise and hasattr(self.model, 'fused_graph_key')) else None
        gs = None
        if gkey is not None:
            gkey = (gkey, getattr(train_data, 'state', None), id(prod))
            gs = self._graphs.get(gkey)
            if gs is None:
                from ..graph_step import GraphedRowwiseStep
                gs = self._graphs[gkey] = GraphedRowwiseStep(self.model, prod, self._loss_sum, self._fused_kw(), unroll=4)
        while True:
            if gs is not None and gs is not False and prod.full_ahead():
                if gs.graph is None:
                    if gs.eager_steps < 2:
                        gs.eager(); prod.advance()
                        continue
                    try:
                        gs.capture()
                        self.graph_stats['captures'] += 1
                    except Exception as e:                              # noqa: BLE001 -- reported, and the eager loop still trains
                        import warnings
                        warnings.warn(f'hipGraph capture of the rowwise step failed for {gkey!r} ({type(e).__name__}: {e}); running it eagerly')
                        gs = self._graphs[gkey] = False
                        prod.resync()
                        continue
                many = gs.graph_k is not None and prod.full_count() >= gs.unroll
                gs.replay(many)
                prod.advance(gs.unroll if many else 1)
                self.graph_stats['replayed'] += gs.unroll if many else 1
                continue
            if prod.full_ahead():
                prod.launch()
                prod.advance()
                interaction = prod.fields
            else:
                try:
                    interaction = next(it)
                except StopIteration:
                    break
                prod.resync()
            loss = self.model.fused_train_step(interaction, **self._fused_kw())
            self._loss_sum.add_(loss.detach().reshape(()))
        value = float(self._loss_sum)
        if value != value:
            raise ValueError('Training loss is nan')
        return value

    def _my_rows(self, interaction):
        import torch.distributed as dist
        from ..data.interaction import Interaction
        if self.__dict__.get('_row_group') is not None:        # a domain's half of the ranks (parallel_domains): rows grank::half
            rank, world = self._row_group
        else:
            world, rank = dist.get_world_size(self.dist_group), dist.get_rank(self.dist_group)
        out = Interaction({k: v[:v.shape[0] - v.shape[0] % world][rank::world].contiguous() for k, v in interaction.items()})
        # rows j + m S of a k-major batch: every world-th row is again k-major (S / world positives) when world divides S
        # (EVERY field: in BOTH mode the source and target columns of one batch may differ in length)
        km = getattr(interaction, 'k_major', None)
        if km and all(v.shape[0] % km == 0 and (v.shape[0] // km) % world == 0 for v in interaction.values()):
            out.k_major = km
        return out

    def _topk_lists(self, interaction, n_user, history_index, kmax, wide=False):
        """idx [U, kmax] of the model's fused mask + top-k (no [U, N] score matrix), pads -1: the history (rows, cols) pairs become a CSR
        with ascending columns.  ``wide``: the list comes from ``full_sort_topk_wide`` (kmax > 64; every model has it, those with
        ``predict`` only through ``_predict_all_pairs``)."""
        dev = self.device
        indptr = cols = None
        if history_index is not None:
            rows, hc = (torch.as_tensor(t, device=dev, dtype=torch.int64) for t in history_index)
            span = int(hc.max()) + 1 if hc.numel() else 1
            key = torch.sort(rows * span + hc).values
            cols = (key % span).contiguous()
            indptr = torch.zeros(n_user + 1, device=dev, dtype=torch.int64)
            indptr[1:] = torch.cumsum(torch.bincount(key // span, minlength=n_user), 0)
            if cols.numel() == 0:
                indptr = cols = None
        if wide:
            _vals, idx = self.model.full_sort_topk_wide(interaction, kmax, hist_indptr=indptr, hist_cols=cols,
                                                        predict_fallback=self._predict_all_pairs)
        else:
            _vals, idx = self.model.full_sort_topk(interaction, kmax, hist_indptr=indptr, hist_cols=cols)
        return idx

    def _topk_hits(self, interaction, n_user, history_index, positive_u, positive_i, kmax, wide=False, stats=None):
        """Hit matrix [U, kmax] and positives per user from ``_topk_lists``: positives are matched by sorted (user, item) keys.  The lists
        are handed on to ``stats`` (``functional.ListStats``): no second top-k call for the non-accuracy metrics."""
        dev = self.device
        N = int(self.model.target_num_items) if hasattr(self.model, 'target_num_items') else None
        idx = self._topk_lists(interaction, n_user, history_index, kmax, wide=wide)
        if stats is not None:
            stats.add(idx)
        pu = torch.as_tensor(positive_u, device=dev, dtype=torch.int64)
        pi = torch.as_tensor(positive_i, device=dev, dtype=torch.int64)
        span = max(int(idx.max()) + 1, int(pi.max()) + 1 if pi.numel() else 1, N or 1)
        pkey = torch.sort(pu * span + pi).values
        qkey = (torch.arange(n_user, device=dev).unsqueeze(1) * span + idx.clamp(min=0)).reshape(-1)
        at = torch.searchsorted(pkey, qkey).clamp(max=max(pkey.numel() - 1, 0))
        hit = (pkey[at] == qkey).view(n_user, kmax) & (idx >= 0) if pkey.numel() else torch.zeros_like(idx, dtype=torch.bool)
        return hit.float(), torch.bincount(pu, minlength=n_user).float()

    @torch.no_grad()
    def evaluate(self, eval_data):
        """eval_data yields (interaction, history_index (rows, cols) or None, positive_u, positive_i) like recbole's
        FullSortEvalDataLoader; returns {metric@k: value} for config['metrics'] (default recall / mrr / ndcg / hit / precision; also map, and
        gauc under the key 'gauc') at every k of config['topk'].  A loader whose ``eval_mode`` is 'sampled' (``NegSampleEvalLoader``, eval_args
        mode uniN / popN) yields (interaction, (cand_indptr, cand_cols), positive_u, positive_i) instead and every positive is ranked inside
        its user's candidate list (``_evaluate_sampled_batches``)."""
        self._fused_sync()
        self.model.eval()
        kmax = max(self.topk)
        # dispatch per loader, on its own attribute: a (source full-sort, target sampled) pair of valid loaders evaluates each its way
        sampled = getattr(eval_data, 'eval_mode', 'full') == 'sampled'
        fused = self.fused_topk and hasattr(self.model, 'full_sort_topk') and not sampled
        if sampled and self.list_metrics:
            raise ValueError(f"evaluate: metrics {', '.join(self.list_metrics)} cannot be answered on a sampled-candidate loader (its lists "
                             f"are positions inside a sample); hand evaluate a full-sort loader")
        # recbole cuts the evaluated users so that the [U, N] score matrix fits eval_batch_size entries (ONE user per call over a 10 M-item
        # catalogue at the default 4,096).  The fused mask + top-k path never forms that matrix, so it re-cuts a loader that allows it
        # into throughput-sized batches (config['eval_users_per_batch'], default 1,024; 0 keeps recbole's cut): same users, same metrics
        want = int(self.config['eval_users_per_batch']) if 'eval_users_per_batch' in self.config else 1024
        restore = None
        if (fused or sampled) and want > 0 and hasattr(eval_data, 'rebatch') and getattr(eval_data, 'step', want) < want:
            restore = eval_data.step                      # (the caller's cut comes back afterwards: another consumer may need [U, N] to fit)
            eval_data.rebatch(want)
        # the model's evaluation-mode caches (CoNet: the item half of layer 1, the packed one-user call) live exactly as long as this loop:
        # nothing trains inside it
        frozen = hasattr(self.model, 'freeze_for_eval')
        if frozen:
            self.model.freeze_for_eval()
        try:
            if sampled:
                return self._evaluate_sampled_batches(eval_data, kmax)
            return self._evaluate_batches(eval_data, fused, kmax)
        finally:
            if frozen:
                self.model.unfreeze_eval()
            if restore is not None:
                eval_data.rebatch(restore)

    def _predict_all_pairs(self, interaction, n_user):
        """[U, N] scores of a model that defines ``predict`` only (DeepAPF, NATR, as in the reference), the way recbole's
        ``Trainer._full_sort_batch_eval`` / ``_spilt_predict`` get them: every user row repeated ``target_num_items`` times, item ids
        0..N-1 attached, ``predict`` in chunks of at most ``eval_batch_size`` pairs (recbole's default 4,096).  Plumbing in torch: correct
        for any model, one ``predict`` per chunk -- slow by construction."""
        N = int(self.model.target_num_items)
        chunk = int(self.config['eval_batch_size']) if 'eval_batch_size' in self.config else 4096
        pairs = interaction.repeat_interleave(N)
        pairs.update({self.model.TARGET_ITEM_ID: torch.arange(N, device=self.device).repeat(n_user)})
        out = [self.model.predict(pairs[s:s + chunk]).reshape(-1) for s in range(0, n_user * N, max(chunk, 1))]
        return torch.cat(out).view(n_user, N).float()

    def _evaluate_batches(self, eval_data, fused, kmax):
        names = self.metrics if self.metrics is not None else DEFAULT_METRICS
        # the non-accuracy metrics: the lists of every batch are folded into ``stats`` on the device, the arithmetic comes at the end
        stats = self._list_stats_for(eval_data)
        wide = self._takes_wide_lists(kmax)
        if self._takes_rank_route(fused, kmax):
            # (with ``stats``: gauc is asked too -- the rank route answers the accuracy metrics and gauc, one list call per batch feeds stats)
            lists = (lambda *batch: self._count_lists(stats, fused, wide, kmax, *batch)) if stats is not None else None
            result, n_users = self._evaluate_batches_by_rank(eval_data, kmax, names, lists)
        else:
            hits, pos_len = [], []
            for interaction, history_index, positive_u, positive_i in eval_data:
                interaction = interaction.to(self.device)
                n_user = len(interaction)
                if fused or wide:
                    h, npos = self._topk_hits(interaction, n_user, history_index, positive_u, positive_i, kmax, wide=wide, stats=stats)
                    hits.append(h); pos_len.append(npos)
                    continue
                scores = self._masked_scores(interaction, n_user, history_index)
                topk_vals, topk_idx = torch.topk(scores, kmax, dim=-1)
                if stats is not None:
                    stats.add(topk_idx, topk_vals)                 # (a masked entry comes back with value -inf: a pad)
                pos = torch.zeros_like(scores, dtype=torch.bool)
                pos[positive_u, positive_i] = True
                hits.append(torch.gather(pos, 1, topk_idx).float())
                pos_len.append(pos.sum(1).float())
            hits = torch.cat(hits)
            result, n_users = metrics_from_hits(hits, torch.cat(pos_len).clamp(min=1), self.topk, names), hits.shape[0]
        if stats is not None:
            result.update(stats.result(n_users, self.list_metrics))
        return result

    def _masked_scores(self, interaction, n_user, history_index):
        """The [U, N] matrix of the unfused route, PAD column and history at -inf."""
        try:
            scores = self.model.full_sort_predict(interaction).view(n_user, -1)
        except NotImplementedError:
            scores = self._predict_all_pairs(interaction, n_user)
        scores[:, 0] = -np.inf
        if history_index is not None:
            scores[history_index] = -np.inf
        return scores

    def _takes_wide_lists(self, kmax):
        """Lists beyond the fused kernels' 64 entries -- eval_route='topk', or a non-accuracy metric under 'auto': on a GPU they come from
        the wide mask + top-k, for every model (a model without full_sort_topk included: its scores go through the selection in chunks,
        not as one [U, N] matrix)."""
        return ((self.eval_route == 'topk' or bool(self.list_metrics)) and self.fused_topk and FUSED_TOPK_MAX < kmax <= WIDE_TOPK_MAX
                and torch.device(self.device).type == 'cuda' and hasattr(self.model, 'full_sort_topk_wide'))

    def _count_lists(self, stats, fused, wide, kmax, interaction, n_user, history_index):
        """One batch's lists by the list route (fused, wide, or torch.topk of the masked matrix where the route is unfused), into ``stats``."""
        if wide or (fused and kmax <= FUSED_TOPK_MAX):
            return stats.add(self._topk_lists(interaction, n_user, history_index, kmax, wide=wide))
        vals, idx = torch.topk(self._masked_scores(interaction, n_user, history_index), kmax, dim=-1)
        stats.add(idx, vals)

    def _takes_rank_route(self, fused, kmax):
        gauc = self.metrics is not None and 'gauc' in self.metrics
        if self.list_metrics:
            return gauc                       # the list route answers everything but gauc (k <= 1024: checked at construction)
        if self.eval_route == 'rank':
            return True
        if self.eval_route == 'topk':
            if fused and kmax > WIDE_TOPK_MAX:
                raise ValueError(f"eval_route='topk': the mask + top-k lists hold k <= {WIDE_TOPK_MAX}, topk asks for {kmax}; use "
                                 f"eval_route='rank' or 'auto', or fused_topk=False")
            return False
        return gauc or (fused and kmax > FUSED_TOPK_MAX)

    @staticmethod
    def _csr(rows, cols, n_user):
        """(indptr [n_user + 1], cols ascending and distinct inside each user's range) of (row, column) pairs, by one sort of the keys"""
        span = int(cols.max()) + 1 if cols.numel() else 1
        key = torch.unique(rows * span + cols)                       # (sorted)
        indptr = torch.zeros(n_user + 1, device=rows.device, dtype=torch.int64)
        indptr[1:] = torch.cumsum(torch.bincount(key // span, minlength=n_user), 0)
        return indptr, (key % span).contiguous()

    def _positives_csr(self, positive_u, positive_i, n_user):
        """(indptr [n_user + 1], columns [P], positives per user [n_user], user row of each positive [P]) of a batch's ground truth"""
        pu = torch.as_tensor(positive_u, device=self.device, dtype=torch.int64)
        pi = torch.as_tensor(positive_i, device=self.device, dtype=torch.int64)
        pindptr, pcols = self._csr(pu, pi, n_user)
        npos = pindptr[1:] - pindptr[:-1]
        return pindptr, pcols, npos, torch.repeat_interleave(torch.arange(n_user, device=pu.device), npos)

    def _rank_counts(self, interaction, n_user, history_index, positive_u, positive_i):
        """(user of each positive [P], gt, eq, eq_before [P], n_unmasked [U], positives per user [U]) of one batch: the model's
        ``full_sort_rank`` on a GPU; a torch restatement over the materialised matrix where there is none (plumbing, as the unfused
        route)."""
        dev = self.device
        pindptr, pcols, npos, prow = self._positives_csr(positive_u, positive_i, n_user)
        hindptr = hcols = hrows = None
        if history_index is not None:
            hr, hc = (torch.as_tensor(t, device=dev, dtype=torch.int64) for t in history_index)
            if hc.numel():
                hindptr, hcols = self._csr(hr, hc, n_user)
                hrows = hr
        if torch.device(dev).type == 'cuda':
            _score, gt, eq, eqb, nun = self.model.full_sort_rank(interaction, pindptr, pcols, hist_indptr=hindptr, hist_cols=hcols,
                                                                 predict_fallback=self._predict_all_pairs)
        else:
            try:
                scores = self.model.full_sort_predict(interaction).view(n_user, -1).float().clone()
            except NotImplementedError:
                scores = self._predict_all_pairs(interaction, n_user)
            scores[:, 0] = float('nan')
            if hrows is not None:
                scores[history_index] = float('nan')
            _score, gt, eq, eqb, nun = rank_counts_reference(scores, prow, pcols)
        if bool((gt < 0).any()):
            p = int(torch.nonzero(gt < 0)[0])
            raise ValueError(f'evaluate: the positive item {int(pcols[p])} of user row {int(prow[p])} of this batch is masked (PAD column or '
                             f'in the user\'s history) or has a NaN score: the rank route does not rank such a positive')
        return prow, gt, eq, eqb, nun, npos

    def _evaluate_batches_by_rank(self, eval_data, kmax, names, lists=None):
        """Every metric from the rank of each positive over the masked catalogue: a positive at top-k position r = 1 + gt + eq_before
        (ties to the smaller column) is a hit at position r of the list for every k >= r -- the same hit matrix the top-k route builds,
        for any kmax; GAUC from the average ranks gt + (eq + 1) / 2.  ``lists(interaction, n_user, history_index)`` is called once per
        batch when a non-accuracy metric rides along.  Returns (result, evaluated users)."""
        acc = ([], [], [], [])
        n_users = 0
        for interaction, history_index, positive_u, positive_i in eval_data:
            interaction = interaction.to(self.device)
            n_user = len(interaction)
            n_users += n_user
            self._rank_batch_tail(acc, n_user, kmax, *self._rank_counts(interaction, n_user, history_index, positive_u, positive_i))
            if lists is not None:
                lists(interaction, n_user, history_index)
        return self._rank_result(acc, names), n_users

    @staticmethod
    def _rank_batch_tail(acc, n_user, kmax, prow, gt, eq, eqb, nun, npos):
        """One batch's (hit matrix, positives per user, ranked items per user, sum of average ranks per user) from its rank counts,
        appended to ``acc``: the one copy both rank routes (full-sort and sampled candidates) end in."""
        at = gt.long() + eqb.long()
        hit = torch.zeros(n_user, kmax, device=gt.device, dtype=torch.float32)
        sel = at < kmax
        hit[prow[sel], at[sel]] = 1.0
        acc[0].append(hit); acc[1].append(npos)
        acc[2].append(nun.long())
        acc[3].append(torch.zeros(n_user, device=gt.device, dtype=torch.float64).index_add_(
            0, prow, gt.double() + (eq.double() + 1) / 2))

    def _rank_result(self, acc, names):
        hits, pos_len, user_len, rank_sum = acc
        n_pos = torch.cat(pos_len)
        result = metrics_from_hits(torch.cat(hits), n_pos.float().clamp(min=1), self.topk, names)
        if 'gauc' in names:
            result['gauc'] = gauc_from_counts(n_pos, torch.cat(user_len), torch.cat(rank_sum))
        return result

    def _evaluate_sampled_batches(self, eval_data, kmax):
        """Sampled-candidate evaluation (a ``NegSampleEvalLoader``): per batch the model's ``candidate_scores`` over the ragged candidate
        lists, then the rank of every positive inside its user's list (``functional.candidate_rank``; its torch restatement on
        ``device: cpu``), then the rank route's arithmetic.  ``n_unmasked`` is the user's distinct candidate count: what recbole's
        collector sees in a row of -inf with the candidates' scores scattered in."""
        from .. import functional as F_
        names = self.metrics if self.metrics is not None else DEFAULT_METRICS
        chunk = int(self.config['eval_batch_size']) if 'eval_batch_size' in self.config else 4096
        on_gpu = torch.device(self.device).type == 'cuda'
        acc = ([], [], [], [])
        for interaction, (cand_indptr, cand_cols), positive_u, positive_i in eval_data:
            interaction = interaction.to(self.device)
            n_user = len(interaction)
            cand_indptr, cand_cols = cand_indptr.to(self.device), cand_cols.to(self.device)
            pindptr, pcols, npos, prow = self._positives_csr(positive_u, positive_i, n_user)
            scores = self.model.candidate_scores(interaction, cand_indptr, cand_cols, chunk).float().contiguous()
            rank = F_.candidate_rank if on_gpu else F_.candidate_rank_reference
            _score, gt, eq, eqb, nun = rank(cand_indptr, cand_cols, scores, pindptr, pcols)
            if bool((gt < 0).any()):
                p = int(torch.nonzero(gt < 0)[0])
                raise ValueError(f'evaluate: the positive item {int(pcols[p])} of user row {int(prow[p])} of this batch is not among the '
                                 f'user\'s candidates or has a NaN score: the rank route does not rank such a positive')
            self._rank_batch_tail(acc, n_user, kmax, prow, gt, eq, eqb, nun, npos)
        return self._rank_result(acc, names)

    def save_checkpoint(self, path, epoch=None):
        """recbole ``Trainer._save_checkpoint``: config-free subset -- epoch, early-stopping state, model ``state_dict``,
        ``other_parameter`` and the optimizer state (dense: ``DenseAdam.state_dict()``; rowwise: the model's per-table
        moments and update counts).  With a ``dist_group``: one file per rank, ``<path>.rank<r>``."""
        self._fused_sync()
        if self.dist_group is not None:
            # a sharded model: every rank writes ITS shards (tables + moments in their current layout) next to the replicated parts
            import torch.distributed as dist
            state = {'epoch': epoch, 'cur_step': self.cur_step, 'best_valid_score': self.best_valid_score,
                     'phase': getattr(self.model, 'phase', None), 'dist': self.model.dist_checkpoint()}
            torch.save(state, f'{path}.rank{dist.get_rank(self.dist_group)}')
            return
        state = {'epoch': epoch, 'cur_step': self.cur_step, 'best_valid_score': self.best_valid_score,
                 'state_dict': self.model.state_dict(), 'other_parameter': self.model.other_parameter(),
                 'optimizer_mode': self.optimizer_mode, 'optimizer': self.optimizer.state_dict(), 'learner': self.learner,
                 'phase': getattr(self.model, 'phase', None)}
        if self.optimizer_mode == 'rowwise' and hasattr(self.model, 'fused_optimizer_state'):
            state['rowwise'] = self.model.fused_optimizer_state()
        torch.save(state, path)

    def resume_checkpoint(self, path):
        """recbole ``Trainer.resume_checkpoint``."""
        if self.dist_group is not None:
            import torch.distributed as dist
            state = torch.load(f'{path}.rank{dist.get_rank(self.dist_group)}', map_location=self.device, weights_only=False)
            self.start_epoch = (state['epoch'] + 1) if state['epoch'] is not None else 0
            self.cur_step, self.best_valid_score = state['cur_step'], state['best_valid_score']
            self.model.load_dist_checkpoint(state['dist'])
            if state.get('phase') is not None:
                self.model.set_phase(state['phase'])
            return
        state = torch.load(path, map_location=self.device, weights_only=False)
        mine = self.learner
        if state.get('learner', 'adam') != mine:          # (checkpoints written before config['learner'] existed are Adam's)
            raise ValueError(f"the checkpoint was written with learner={state.get('learner', 'adam')!r}; this trainer runs learner={mine!r} "
                             f"(the optimizer state of one does not resume the other)")
        self.start_epoch = (state['epoch'] + 1) if state['epoch'] is not None else 0
        self.cur_step, self.best_valid_score = state['cur_step'], state['best_valid_score']
        self._graphs.clear()                       # captured steps point at the optimizer state tensors about to be replaced
        self.model.load_state_dict(state['state_dict'])
        self.model.load_other_parameter(state.get('other_parameter'))
        if state.get('phase') is not None and hasattr(self.model, 'set_phase'):
            self.model.set_phase(state['phase'])
        self.optimizer.load_state_dict(state['optimizer'])
        if 'rowwise' in state and hasattr(self.model, 'load_fused_optimizer_state'):
            if self.rowwise_adam == 'exact':
                self.model.load_fused_optimizer_state(state['rowwise'], adam='exact')
            elif mine != 'adam':
                self.model.load_fused_optimizer_state(state['rowwise'], opt=mine)
            else:
                self.model.load_fused_optimizer_state(state['rowwise'])

    def fit(self, train_data, valid_data=None, verbose=True, saved=True, show_progress=False, callback_fn=None):
        for epoch_idx in range(self.start_epoch, self.epochs):
            train_loss = self._train_epoch(train_data, epoch_idx)
            self.train_loss_dict[epoch_idx] = train_loss
            if self.eval_step <= 0 or not valid_data:
                continue
            if (epoch_idx + 1) % self.eval_step == 0:
                valid_result = self.evaluate(valid_data)
                valid_score = valid_result[self.valid_metric]
                self.best_valid_score, self.cur_step, stop_flag, update_flag = early_stopping(
                    valid_score, self.best_valid_score, self.cur_step, max_step=self.stopping_step,
                    bigger=self.valid_metric_bigger)
                if update_flag:
                    self.best_valid_result = valid_result
                if callback_fn:
                    callback_fn(epoch_idx, valid_score)
                if stop_flag:
                    break
        self._fused_sync()
        return self.best_valid_score, self.best_valid_result

    def _fused_kw(self):
        """Keyword arguments of ``model.fused_train_step`` (optimizer_mode='rowwise')."""
        kw = {'opt': self.learner, 'lr': self.learning_rate, 'weight_decay': self.weight_decay}
        if kw['opt'] == 'adagrad':
            kw['eps'] = 1e-10                          # torch.optim.Adagrad's default (the steps' own default is Adam's 1e-8)
        if self.rowwise_adam == 'exact':
            kw['adam'] = 'exact'
        return kw

    def _fused_sync(self):
        """rowwise_adam='exact': every row of the model's tables at its update count (the reference's dense-Adam state)."""
        if self.rowwise_adam == 'exact':
            self.model.fused_sync()


class CrossDomainTrainer(Trainer):
    """Phase loop over ``train_modes`` (SOURCE / TARGET / BOTH / OVERLAP) -- trainer.py:43-76."""

    def __init__(self, config, model):
        super().__init__(config, model)
        self.train_modes = config['train_modes']
        self.train_epochs = config['epoch_num']
        self.split_valid_flag = config['source_split']

    def _reinit(self, phase):
        """Reset per-phase state; the optimizer (and its Adam moments) is NOT rebuilt (trainer.py:30-41, Q13)."""
        self.start_epoch = 0
        self.cur_step = 0
        self.best_valid_score = -np.inf if self.valid_metric_bigger else np.inf
        self.best_valid_result = None
        self.item_tensor = None
        self.tot_item_num = None
        self.train_loss_dict = dict()
        self.epochs = int(self.train_epochs[phase])
        self.eval_step = min(self.config['eval_step'] if 'eval_step' in self.config else 1, self.epochs)

    def _fit_domains_in_parallel(self, train_data, phase, both, verbose, saved, show_progress, callback_fn):
        """config['parallel_domains'] with a dist_group: a SOURCE phase followed by a TARGET phase (or the reverse) touches
        disjoint tables and disjoint optimizer state, so the lower half of the ranks runs the SOURCE epochs while the upper half
        runs the TARGET epochs -- each domain's tables cut into world/2 column slices instead of world (twice the slice width,
        half the replicated index work: DESIGN.md 6.1).  Same result as running the two phases one after the other; no
        evaluation inside (it needs every rank); the halves meet again at a barrier.  ``both`` False: a SOURCE or TARGET phase
        on its own -- only that domain's half trains, the other half waits."""
        import torch.distributed as dist
        world, rank = dist.get_world_size(self.dist_group), dist.get_rank(self.dist_group)
        half = world // 2
        mine = 'SOURCE' if rank < half else 'TARGET'
        schemes = [self.train_modes[phase]] + ([self.train_modes[phase + 1]] if both else [])
        if hasattr(self.model, 'dist_prepare'):
            self.model.dist_prepare([s_.lower() for s_ in schemes])          # collective: every rank, also the idle half
        if mine in schemes:
            self._reinit(phase + schemes.index(mine))
            train_data.set_mode(train_mode2state[mine])
            self.model.set_phase(mine)
            self._row_group = (rank % half, half)
            try:
                Trainer.fit(self, train_data, None, verbose, saved, show_progress, callback_fn)
            finally:
                self._row_group = None
        dist.barrier(group=self.dist_group)

    def _fit_domains_on_two_streams(self, train_data, phase):
        """config['parallel_domains'] on ONE GPU (optimizer_mode='rowwise'): a SOURCE phase directly followed by a TARGET phase (or the
        reverse) touches disjoint tables and disjoint optimizer state, so their epochs are enqueued side by side on two HIP streams --
        the tails and small launches of one domain's step run under the other domain's kernels (measured on the headline step: 4.27 ->
        3.99 ms for a source + target step).  Bit-identical to running the two phases one after the other; no evaluation inside (the
        caller falls back to the sequential phases when validation is requested).  Returns {scheme: [epoch loss sums]}."""
        from ..data.producer import DeviceBatchProducer
        schemes = [self.train_modes[phase], self.train_modes[phase + 1]]
        epochs = {sc: int(self.train_epochs[phase + j]) for j, sc in enumerate(schemes)}
        loaders = {'SOURCE': train_data.source_dataloader, 'TARGET': train_data.target_dataloader}
        cache = self.__dict__.setdefault('_two_stream', {})
        if 'streams' not in cache:
            cache['streams'] = {sc: torch.cuda.Stream(device=self.device) for sc in ('SOURCE', 'TARGET')}
            cache['loss'] = {sc: torch.zeros((), device=self.device, dtype=torch.float32) for sc in ('SOURCE', 'TARGET')}
            cache['prod'] = {}
        streams, sums = cache['streams'], cache['loss']
        for sc in schemes:
            if sc not in cache['prod']:
                cache['prod'][sc] = DeviceBatchProducer(loaders[sc]) if DeviceBatchProducer.supports(loaders[sc]) else None
        prods = cache['prod']
        cur = torch.cuda.current_stream()
        log = {sc: [] for sc in schemes}
        self.model.train()
        for e in range(max(epochs.values())):
            active = [sc for sc in schemes if e < epochs[sc]]
            its = {}
            for sc in active:
                streams[sc].wait_stream(cur)
                with torch.cuda.stream(streams[sc]):
                    its[sc] = iter(loaders[sc])                          # (the epoch shuffle, on the domain's own stream)
                    if prods[sc] is not None:
                        prods[sc].resync()
                    sums[sc].zero_()
            live = list(active)
            while live:
                for sc in list(live):
                    with torch.cuda.stream(streams[sc]):
                        pr = prods[sc]
                        if pr is not None and pr.full_ahead():
                            pr.launch(); pr.advance()
                            batch = pr.fields
                        else:
                            try:
                                batch = next(its[sc]).to(self.device)
                            except StopIteration:
                                live.remove(sc)
                                continue
                            if pr is not None:
                                pr.resync()
                        self.model.set_phase(sc)                          # (host-side switch: which tables the fused step takes)
                        loss = self.model.fused_train_step(batch, **self._fused_kw())
                        sums[sc].add_(loss.detach().reshape(()))
            for sc in active:
                cur.wait_stream(streams[sc])
            for sc in active:
                v = float(sums[sc])
                if v != v:
                    raise ValueError('Training loss is nan')
                log[sc].append(v)
        for ld in loaders.values():
            ld.pr = 0
        self.train_loss_dict = {sc: dict(enumerate(v)) for sc, v in log.items()}
        self.model.set_phase(schemes[-1])
        return log

    def fit(self, train_data, valid_data=None, verbose=True, saved=True, show_progress=False, callback_fn=None):
        parallel = False
        if self.dist_group is not None and 'parallel_domains' in self.config and self.config['parallel_domains']:
            import torch.distributed as dist
            parallel = dist.get_world_size(self.dist_group) % 2 == 0
        two_streams = (self.dist_group is None and 'parallel_domains' in self.config and bool(self.config['parallel_domains'])
                       and self.optimizer_mode == 'rowwise' and torch.device(self.device).type == 'cuda'
                       and (valid_data is None or self.config['eval_step'] <= 0 if 'eval_step' in self.config else valid_data is None))
        skip = False
        for phase in range(len(self.train_modes)):
            if skip:                                 # ran together with the previous phase
                skip = False
                continue
            nxt = self.train_modes[phase + 1] if phase + 1 < len(self.train_modes) else None
            if two_streams and {self.train_modes[phase], nxt} == {'SOURCE', 'TARGET'}:
                self._reinit(phase)
                self._fit_domains_on_two_streams(train_data, phase)
                skip = True
                continue
            if parallel and self.train_modes[phase] in ('SOURCE', 'TARGET'):
                both = {self.train_modes[phase], nxt} == {'SOURCE', 'TARGET'}
                self._fit_domains_in_parallel(train_data, phase, both, verbose, saved, show_progress, callback_fn)
                skip = both
                continue
            self._reinit(phase)
            scheme = self.train_modes[phase]
            train_data.set_mode(train_mode2state[scheme])
            self.model.set_phase(scheme)
            if self.split_valid_flag and valid_data is not None:
                source_valid_data, target_valid_data = valid_data
                if scheme == 'SOURCE':
                    super().fit(train_data, source_valid_data, verbose, saved, show_progress, callback_fn)
                else:
                    super().fit(train_data, target_valid_data, verbose, saved, show_progress, callback_fn)
            else:
                super().fit(train_data, valid_data, verbose, saved, show_progress, callback_fn)
        self._fused_sync()
        self.model.set_phase('OVERLAP')
        return self.best_valid_score, self.best_valid_result


class DCDCSRTrainer(CrossDomainTrainer):
    """trainer.py:79-139: the same phase loop, except that the BOTH phase (DCDCSR's mapping phase: the loss ignores the batch and
    nothing can be ranked before the second TARGET visit builds the affine table) runs WITHOUT validation data.
    ``train_modes`` typically ['SOURCE', 'TARGET', 'BOTH', 'TARGET'] (properties/model/DCDCSR.yaml): ``epoch_num`` is indexed by the
    phase's POSITION, and the model counts its visits of each phase (dcdcsr.py:90-92)."""

    def fit(self, train_data, valid_data=None, verbose=True, saved=True, show_progress=False, callback_fn=None):
        for phase in range(len(self.train_modes)):
            self._reinit(phase)
            scheme = self.train_modes[phase]
            train_data.set_mode(train_mode2state[scheme])
            self.model.set_phase(scheme)
            if scheme == 'BOTH':
                Trainer.fit(self, train_data, None, verbose, saved, show_progress, callback_fn)
            elif self.split_valid_flag and valid_data is not None:
                source_valid_data, target_valid_data = valid_data
                Trainer.fit(self, train_data, source_valid_data if scheme == 'SOURCE' else target_valid_data, verbose, saved,
                            show_progress, callback_fn)
            else:
                Trainer.fit(self, train_data, valid_data, verbose, saved, show_progress, callback_fn)
        self.model.set_phase('OVERLAP')
        return self.best_valid_score, self.best_valid_result
