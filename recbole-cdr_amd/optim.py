"""The native dense optimizers: what ``config['learner']`` names, as recbole's ``_build_optimizer`` builds it -- the exact Adam
(csrc/cdr_rows.hip ``cdr_adam_multi_dev``) by default, or SGD / Adagrad / RMSprop with torch's defaults (csrc/cdr_optim.hip
``cdr_opt_multi_dev``) -- and ``RowAwareAdam``, the same Adam with a model's embedding tables in the deferred row-wise form.
"""
import torch


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
        from . import binding as B_
        jobs, self.produce_jobs = self.produce_jobs, None
        try:
            self._step_groups(jobs)
        finally:
            jobs = self.__dict__.pop('_jobs_left', jobs)
            if jobs:                                   # no parameter had a gradient (or several groups): the batch is produced all the same
                from .data.producer import launch_jobs
                launch_jobs(jobs)

    def _step_groups(self, jobs):
        import ctypes
        from . import binding as B_
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
        from . import binding as B_
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
        from .fused import OPT_NAMES                      # (the package's one table of CDR_OPT_* codes)
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
