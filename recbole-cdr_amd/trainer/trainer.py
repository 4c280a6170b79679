"""CrossDomainTrainer: the caller of the hot path (recbole_cdr/trainer/trainer.py:18-76).

The reference subclasses third-party ``recbole.trainer.Trainer``; the part of it the phase loop relies on is restated
here (optimizer built ONCE and kept across phases, ``_train_epoch`` = zero_grad -> calculate_loss ->
(tuple => sum) -> nan check -> backward -> clip -> step, ``fit`` with eval_step / early stopping, ``evaluate`` =
full-sort scores -> mask PAD column and history -> top-k).  This module keeps the loop: ``evaluate`` lives in ``evaluation.Evaluation``,
which ``Trainer`` inherits, and the dense optimizer ``config['learner']`` names in ``optim``.  Both modules' names are importable from
here, as they always were.
"""
import numpy as np
import torch

from ..utils import train_mode2state, total_loss as _total
from ..optim import (DenseAdam, DenseSGD, DenseAdagrad, DenseRMSprop, RowAwareAdam, LEARNERS, dense_optimizer, resolve_learner,  # noqa: F401
                     _DenseLearner, _dense_adam_load, _refuse)
from .evaluation import (Evaluation, DEFAULT_METRICS, TOPK_METRICS, VALUE_METRICS, NON_ACCURACY_METRICS, FUSED_TOPK_MAX,  # noqa: F401
                         WIDE_TOPK_MAX, resolve_metrics, resolve_eval_mode, resolve_eval_route, metrics_from_hits, gauc_from_counts,
                         rank_counts_reference)


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


class Trainer(Evaluation):
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
        self._init_evaluation(config)              # (topk, metrics, eval_route, eval_mode, device, list_metrics, item_counts, fused_topk)
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
        self._zero_loss_sum()
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
        return self._epoch_loss(self._loss_sum)

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
        return self._epoch_loss(total) if total is not None else 0.0

    def _train_epoch_rowwise_produced(self, train_data, prod):
        """The rowwise loop on a device loader: every full batch is ONE producer launch (slice of the shuffled interactions + tiling +
        negative sampling into fixed buffers, data/producer.py) followed by the model's fused O(batch) step; the loader's own
        ``__next__`` serves ragged tails and ends the epoch.  (The fused steps of large batches read host-side update counts, so
        they are launched, not replayed; at >= 1 M rows per step the host's part is < 2 % of the step.)"""
        self._zero_loss_sum()
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
            try:
                interaction = self._next_batch(prod, it)
            except StopIteration:
                break
            loss = self.model.fused_train_step(interaction, **self._fused_kw())
            self._loss_sum.add_(loss.detach().reshape(()))
        return self._epoch_loss(self._loss_sum)

    def _zero_loss_sum(self):
        """The epoch's loss total, a device scalar the steps add to (created once: captured graphs point at it), set to 0."""
        if self._loss_sum is None:
            self._loss_sum = torch.zeros((), device=self.device, dtype=torch.float32)
        self._loss_sum.zero_()

    @staticmethod
    def _epoch_loss(total):
        """An epoch's loss total as a float (the epoch's one read-back); NaN is refused."""
        value = float(total)
        if value != value:
            raise ValueError('Training loss is nan')
        return value

    def _next_batch(self, prod, it):
        """The next training batch of a rowwise loop: ONE producer launch where the device producer ``prod`` (None: the loader has none)
        has a full batch ahead, the loader's own ``__next__`` otherwise -- ragged tails; StopIteration ends the epoch."""
        if prod is not None and prod.full_ahead():
            prod.launch()
            prod.advance()
            return prod.fields
        batch = next(it).to(self.device)
        if prod is not None:
            prod.resync()
        return batch

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
    PHASES_WITHOUT_VALIDATION = ()

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

    def _fit_phase(self, phase, train_data, valid_data, *fit_args):
        """One phase on its own: per-phase state reset, loader and model switched to the phase's scheme, ``Trainer.fit`` with that
        scheme's validation loader -- the source or the target one of a (source, target) pair, none in ``PHASES_WITHOUT_VALIDATION``."""
        self._reinit(phase)
        scheme = self.train_modes[phase]
        train_data.set_mode(train_mode2state[scheme])
        self.model.set_phase(scheme)
        if scheme in self.PHASES_WITHOUT_VALIDATION:
            valid_data = None
        elif self.split_valid_flag and valid_data is not None:
            source_valid_data, target_valid_data = valid_data
            valid_data = source_valid_data if scheme == 'SOURCE' else target_valid_data
        Trainer.fit(self, train_data, valid_data, *fit_args)

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
                        try:
                            batch = self._next_batch(prods[sc], its[sc])
                        except StopIteration:
                            live.remove(sc)
                            continue
                        self.model.set_phase(sc)                          # (host-side switch: which tables the fused step takes)
                        loss = self.model.fused_train_step(batch, **self._fused_kw())
                        sums[sc].add_(loss.detach().reshape(()))
            for sc in active:
                cur.wait_stream(streams[sc])
            for sc in active:
                log[sc].append(self._epoch_loss(sums[sc]))
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
            self._fit_phase(phase, train_data, valid_data, verbose, saved, show_progress, callback_fn)
        self._fused_sync()
        self.model.set_phase('OVERLAP')
        return self.best_valid_score, self.best_valid_result


class DCDCSRTrainer(CrossDomainTrainer):
    """trainer.py:79-139: the same phase loop, except that the BOTH phase (DCDCSR's mapping phase: the loss ignores the batch and
    nothing can be ranked before the second TARGET visit builds the affine table) runs WITHOUT validation data.
    ``train_modes`` typically ['SOURCE', 'TARGET', 'BOTH', 'TARGET'] (properties/model/DCDCSR.yaml): ``epoch_num`` is indexed by the
    phase's POSITION, and the model counts its visits of each phase (dcdcsr.py:90-92)."""
    PHASES_WITHOUT_VALIDATION = ('BOTH',)

    def fit(self, train_data, valid_data=None, verbose=True, saved=True, show_progress=False, callback_fn=None):
        for phase in range(len(self.train_modes)):
            self._fit_phase(phase, train_data, valid_data, verbose, saved, show_progress, callback_fn)
        self.model.set_phase('OVERLAP')
        return self.best_valid_score, self.best_valid_result
