"""Fused row-wise training steps: forward + backward + optimizer for one batch without table-sized gradients
(FusedBPRStep: pairwise BPR; FusedPointStep: pointwise MSE / BCE; FusedPointPairStep: CMF's two domains on shared tables;
FusedTripletStep: SSCDR's triplet margin loss; FusedCLFMStep: CLFM's two domains, four tables and stacked factor weights;
FusedDTCDRStep: DTCDR's two NeuMF towers over the maximum of both domains' rows, four tables fed by both batches;
FusedDeepAPFStep: DeepAPF's two-candidate attention, a share table fed by both batches and two tables per domain;
FusedDCDCSRMapStep: DCDCSR's max-min normalised tanh-MLP map loss on sampled unit ids; FusedFrozenSideBPRStep: DCDCSR's second TARGET
visit, BPR against a detached operand;
FusedMapStep / SSCDRMapStep: EMCDR's / SSCDR's OVERLAP-phase mapping loss).

This is the large-table counterpart of ``loss.backward(); optimizer.step()`` in the reference's loop
(recbole_cdr/trainer/trainer.py:59-73 -> recbole ``Trainer._train_epoch``): dense ``[rows, D]`` gradients and a dense
Adam sweep are O(table) per step and impossible at BASELINE config C5 (72 GB of tables).  Here every step touches
only the batch's rows: see csrc/cdr_step.hip for the kernels and DESIGN.md for the (lazy-Adam) semantic note.
"""
import ctypes
import os

import torch

from . import binding as B_

OPT_SGD, OPT_ADAM, OPT_ADAGRAD, OPT_RMSPROP = 0, 1, 2, 3      # CDR_OPT_* of include/cdr_hip.h: THE table of this package
OPT_NAMES = {OPT_SGD: 'sgd', OPT_ADAM: 'adam', OPT_ADAGRAD: 'adagrad', OPT_RMSPROP: 'rmsprop'}
_OPT_CODES = {name: code for code, name in OPT_NAMES.items() if code != OPT_RMSPROP}      # what a row-wise step can be asked for
ADAGRAD_EPS = 1e-10                                  # torch.optim.Adagrad's default (Adam's is 1e-8: pass it with opt='adagrad')


def opt_code(opt):
    """'sgd' | 'adam' | 'adagrad' -> the native optimizer code.  Any other name is an error (it used to mean SGD, silently).
    Row-wise RMSprop does not exist: an untouched row's square_avg decays every step, so leaving untouched rows alone is another
    optimizer."""
    try:
        return _OPT_CODES[opt]
    except (KeyError, TypeError):
        raise ValueError(f"opt must be one of {sorted(_OPT_CODES)}, got {opt!r}") from None


def refuse_adagrad(who, code):
    """For the step forms whose kernels implement SGD and Adam only (k-major, small-batch, two-launch map, sharded)."""
    if code == OPT_ADAGRAD:
        raise ValueError(f"{who} has no Adagrad form (opt='adagrad' is served by FusedBPRStep, FusedPointStep and the steps on the "
                         f"general segmented apply)")


class RowwiseState:
    """Per-table optimizer state for the row-wise Adam (SGD needs no moments; Adagrad keeps ONE table-sized tensor, the sum of squared
    gradients, in ``exp_avg_sq`` with ``exp_avg`` None -- no ``last``, no ring, no device step mirror is needed: a row whose gradient is
    zero keeps its sum and its weights bit for bit, so the row-wise Adagrad IS the dense one at weight_decay = 0).  ``step`` counts the updates this TABLE
    has received -- like torch.optim.Adam's per-parameter ``state['step']`` -- so one state object can be shared by the
    step objects of several phases (SOURCE / TARGET BPR steps and the OVERLAP map step touch the same user tables).

    ``exact=True``: the reference's dense Adam instead of the lazy one (``rowwise_catch_up`` in front of every step on the table).
    The state then also holds ``last`` (int32 [rows]: the update each row reflects) and its own ring of per-update scalars, so that
    tables stepped on different streams (parallel domains) share nothing mutable; ``flush()`` brings every row to ``step``.

    ``n2`` / ``n2_valid``: the table's squared-norm records (float [rows, cdr_norm_rec_floats()], slot 0 = ||table[r]||^2; csrc/cdr_step.hip,
    "EmbLoss norms from a per-row cache"), allocated on the first fused BPR step that can use them.  Only that step's sorted path keeps them
    current (``advance(keeps_norms=True)``); every other writer of the table -- any other ``advance``, the ``step`` setter, ``restored()``, a
    replayed graph, an in-place torch op (seen by ``table._version``) -- leaves them stale, and the BPR step goes back to gathering rows
    until it rebuilds them (``norms_ready``)."""
    _step = 0                 # class-level defaults: objects built with __new__ (layout transposes in dimshard.py) start consistent
    _step_dev = None
    exact = False
    n2 = None
    _n2_ok = False            # the records followed every native update since they were built
    _n2_version = -1          # table._version the records were built at (an in-place torch op on the table moves it; the native steps do not)
    _n2_tried = False         # a build was attempted (the first eligible step builds at once, later ones wait: NORMS_REBUILD_AFTER)
    _n2_run = 0               # consecutive eligible BPR steps on the gather path since the records went stale

    NORMS_REBUILD_AFTER = 4   # stale records are rebuilt after this many consecutive eligible gather steps (a phase that alternates writers
                              # would otherwise stream the whole table through the build every step)
    NORMS_MARGIN_BYTES = 4 << 30

    HP_CAPACITY = 1 << 12     # ring entries: with the moving window (period <= capacity / 2) no row falls a ring behind

    def __init__(self, table, opt, exact=False):
        self.table = table
        self._step = 0
        self.exp_avg = torch.zeros_like(table) if opt == OPT_ADAM else None
        self.exp_avg_sq = torch.zeros_like(table) if opt in (OPT_ADAM, OPT_ADAGRAD) else None
        self.opt = opt
        self._step_dev = None
        self.exact = bool(exact)
        if self.exact:
            if opt != OPT_ADAM:
                raise ValueError('RowwiseState(exact=True) is the dense Adam: it needs opt=adam')
            self.last = torch.zeros(table.shape[0], device=table.device, dtype=torch.int32)
            self.hp = torch.zeros(self.HP_CAPACITY, 2, device=table.device, dtype=torch.float32)
            self.hparams = None       # (lr, beta1, beta2, eps, weight_decay) of the catch-ups: the flush replays with the same
            self._flushed_at = 0
            self.sweep_period = rowwise_sweep_period()     # fixed for the table's life: the lag bound rests on it

    @property
    def step(self):
        return self._step

    @step.setter
    def step(self, value):                       # (checkpoint restore, layout changes) keeps the device mirror in step
        self._step = int(value)
        self.n2_valid, self._n2_run = False, 0
        if self._step_dev is not None:
            self._step_dev.fill_(self._step)

    @property
    def n2_valid(self):
        """The squared-norm records describe the table as it stands."""
        return self._n2_ok and self.n2 is not None and self.table._version == self._n2_version

    @n2_valid.setter
    def n2_valid(self, value):
        self._n2_ok = bool(value)

    @property
    def step_dev(self):
        """The update count as a device int64 [1] (read by the capturable applies); created on first use from ``step``."""
        if self._step_dev is None:
            self._step_dev = torch.full((1,), int(self._step), device=self.table.device, dtype=torch.int64)
        return self._step_dev

    def advance(self, device_bumped=False, keeps_norms=False):
        """One more update of this table.  ``device_bumped``: a kernel already incremented the device counter.  ``keeps_norms``: the
        update also wrote the squared-norm record of every row it moved (the cached BPR step alone)."""
        self._step += 1
        if not keeps_norms:
            self.n2_valid, self._n2_run = False, 0
        if self._step_dev is not None and not device_bumped:
            B_.call('cdr_inc_i64', B_.stream(), B_.i64(self._step_dev))

    @torch.no_grad()
    def flush(self):
        """Exact mode: every row of the table up to ``step`` -- what the dense sweep would have left in memory (evaluation, checkpoint).
        Reads the device count (``step_dev``), as the catch-ups do."""
        if not self.exact or self.hparams is None:
            return
        lr, b1, b2, eps, wd = self.hparams
        B_.call('cdr_lazy_adam_flush', B_.stream(), self.table.shape[1], B_.f32(self.table), B_.f32(self.exp_avg), B_.f32(self.exp_avg_sq),
                B_.raw(self.last), self.table.shape[0], lr, b1, b2, eps, wd, B_.raw(self.hp), self.HP_CAPACITY, B_.i64(self.step_dev))
        self._flushed_at = self._step

    @torch.no_grad()
    def norms_build(self, max_bytes=None):
        """Fill the squared-norm records from the table as it stands (one streaming pass on the current stream).  The array is allocated
        on first use, and only if it fits ``max_bytes`` (when given) and leaves NORMS_MARGIN_BYTES of device memory free; False if refused."""
        rec = int(B_.load().cdr_norm_rec_floats())
        rows, D = self.table.shape
        if self.n2 is None:
            need = rows * rec * 4
            dev = self.table.device
            free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
            if (max_bytes is not None and need > max_bytes) or free < need + self.NORMS_MARGIN_BYTES:
                self.n2_valid, self._n2_run = False, 0
                return False
            self.n2 = torch.empty(rows, rec, device=dev, dtype=torch.float32)
        B_.call('cdr_row_norms_build', B_.stream(), B_.f32(self.table), rows, D, B_.f32(self.n2))
        self._n2_ok, self._n2_version, self._n2_run = True, self.table._version, 0
        return True

    def norms_ready(self, max_bytes=None):
        """Before an eligible BPR step: True if the records are current -- building them if this is the first such step on the table, or
        the NORMS_REBUILD_AFTER-th in a row since they went stale."""
        if self.n2_valid:
            return True
        self.n2_valid = False
        if self._n2_tried and self._n2_run < self.NORMS_REBUILD_AFTER:
            return False
        self._n2_tried = True
        return self.norms_build(max_bytes)

    def restored(self):
        """Exact mode, after the table, moments and ``step`` were loaded: every row is current at ``step``."""
        self.n2_valid, self._n2_run = False, 0
        if self.exact:
            self.last.fill_(self._step)
            self._flushed_at = self._step


def rowwise_sweep_period():
    """Updates after which the catch-up's moving window has visited every row of a table: 256, at most half the ring.
    CDR_ROWWISE_SWEEP=0 switches the window off (A/B runs: ``rowwise_catch_up`` then flushes each table every half ring of updates)."""
    p = int(os.environ.get('CDR_ROWWISE_SWEEP', '256'))
    return 0 if p <= 0 else max(2, min(p, RowwiseState.HP_CAPACITY // 2))


def rowwise_bound_lag(state):
    """Without the window: keep every row of an exact table less than a ring behind by a flush every half ring of its updates."""
    if state.exact and state.sweep_period == 0 and state.step - state._flushed_at >= RowwiseState.HP_CAPACITY // 2:
        state.flush()


@torch.no_grad()
def rowwise_catch_up(tables, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """ONE launch in front of a fused step that makes its row-wise Adam the reference's dense one (cdr_rowwise_adam_catch_up).
    ``tables``: [(RowwiseState with exact=True, [int64 id tensors: the rows the step updates in this table, one or two lists])], one to
    four tables.  Every listed row replays its postponed gradient-free updates and is then exactly where the dense sweep would have left
    it before the step's update; the step itself is unchanged.  Issue it BEFORE the step advances the counts; capturable."""
    n = len(tables)
    assert 1 <= n <= 4
    hp = (float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay))
    capturing = torch.cuda.is_current_stream_capturing()
    period = tables[0][0].sweep_period if tables[0][0].exact else 0
    for st, ids in tables:
        if not st.exact:
            raise ValueError('rowwise_catch_up needs RowwiseState(..., exact=True)')
        if st.sweep_period != period:
            raise ValueError(f'rowwise_catch_up: tables with different window periods in one launch ({st.sweep_period} vs {period})')
        if not 1 <= len(ids) <= 2:
            raise ValueError('rowwise_catch_up: one or two id lists per table')
        for x in ids:                 # (the launch reads raw pointers and moves `last` of the rows it reads: check before, not after)
            if x.dtype != torch.int64 or x.device != st.table.device:
                raise ValueError(f'rowwise_catch_up: ids must be int64 on {st.table.device}, got {x.dtype} on {x.device}')
        if st.hparams is not None and st.hparams != hp:
            raise ValueError(f'exact row-wise Adam: one table stepped with two sets of hyperparameters ({st.hparams} vs {hp})')
        st.hparams = hp
        if not capturing:
            rowwise_bound_lag(st)
    lists = [[x.reshape(-1).contiguous() for x in ids] + [None] * (2 - len(ids)) for _, ids in tables]
    arr = lambda xs: (ctypes.c_void_p * n)(*xs)
    i64s = lambda xs: (ctypes.c_int64 * n)(*xs)
    ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
    keep = [[st.step_dev for st, _ in tables], lists]              # (step_dev: created here on first use)
    B_.call('cdr_rowwise_adam_catch_up', B_.stream(), n, (ctypes.c_int * n)(*[st.table.shape[1] for st, _ in tables]),
            arr([st.table.data_ptr() for st, _ in tables]), arr([st.exp_avg.data_ptr() for st, _ in tables]),
            arr([st.exp_avg_sq.data_ptr() for st, _ in tables]), arr([st.last.data_ptr() for st, _ in tables]),
            i64s([st.table.shape[0] for st, _ in tables]), arr([st.hp.data_ptr() for st, _ in tables]), RowwiseState.HP_CAPACITY,
            arr([c.data_ptr() for c in keep[0]]), arr([ptr(l[0]) for l in lists]), i64s([0 if l[0] is None else l[0].numel() for l in lists]),
            arr([ptr(l[1]) for l in lists]), i64s([0 if l[1] is None else l[1].numel() for l in lists]), *hp, period)
    del keep


class _Step:
    """What every step class keeps: the optimizer settings (and their native-call form), the host side of a hipGraph replay, and what
    the steps composed of a forward, an id sort and segmented applies share: the size queries, the sort buffers, the states and the apply."""

    def __init__(self, opt, lr, betas, eps, weight_decay):
        self.opt = opt_code(opt)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay

    def _hp(self):
        """(lr, beta1, beta2, eps, weight_decay) in the order the native calls take them."""
        return tuple(map(float, (self.lr, self.betas[0], self.betas[1], self.eps, self.wd)))

    def replayed(self, n=1):
        """Host bookkeeping of ``n`` hipGraph replays of a step whose update counts live on the device: their host mirrors."""
        for _ in range(n):
            for st in self._states():
                st.advance(device_bumped=True)

    @staticmethod
    def _query_bytes(entry, *args):
        """What the native size query ``entry(*args, &bytes)`` reports."""
        need = ctypes.c_size_t(0)
        B_._check(getattr(B_.load(), entry)(*args, ctypes.byref(need)), entry)
        return int(need.value)

    @staticmethod
    def _sort_rows_of(*tables):
        return 2 << (max(t.shape[0] for t in tables) - 1).bit_length()

    @classmethod
    def _sort_scratch(cls, dev, rows, *n_keys):
        """uint8 scratch of an id sort over ``rows`` table rows: enough for each of the key counts given."""
        return torch.empty(max(cls._query_bytes('cdr_sort_workspace_bytes', n, rows) for n in n_keys), device=dev, dtype=torch.uint8)

    @classmethod
    def _sort_buffers(cls, n_keys, rows, dev):
        """(keys, perm, scratch) of an id sort of up to ``n_keys`` keys.  The sort switches configuration at 2^18 keys: a short tail
        batch may need more scratch than a full one, so the scratch covers the full count and min(count, 2^18 - 1)."""
        return (torch.empty(n_keys, device=dev, dtype=torch.int32), torch.empty(n_keys, device=dev, dtype=torch.int32),
                cls._sort_scratch(dev, rows, n_keys, min(n_keys, (1 << 18) - 1)))

    def _own_states(self, tables, states):
        """One ``RowwiseState`` per table: the caller's where one is given, a fresh one otherwise."""
        states = states if states is not None else (None,) * len(tables)
        return tuple(st if st is not None else RowwiseState(t, self.opt) for st, t in zip(states, tables))

    def _apply(self, ctxh, st, D, keys, perm, n, G, neg_start, reg_limit, coef, key_base, advance=True):
        """One segmented update of ``st``'s table from the sorted occurrence list: occurrence o takes G[o] below ``neg_start`` and
        -G[o - neg_start] from it on; EmbLoss with the device coefficient ``coef`` (None: none) on occurrences below ``reg_limit``.
        ``advance=False``: the caller has counted the update already."""
        if advance:
            st.advance()
        B_.call('cdr_rowwise_apply', ctxh, B_.stream(), self.opt, B_.f32(st.table), B_.f32(st.exp_avg), B_.f32(st.exp_avg_sq), D,
                B_.raw(keys), B_.raw(perm), n, B_.f32(G), neg_start, reg_limit, None if coef is None else B_.f32(coef), *self._hp(),
                st.step, None, int(key_base))

    def _dense_optimizer(self, params):
        """The dense optimizer of the step's own learner for its small parameters (None: plain SGD, done in torch by the caller)."""
        from .optim import DenseAdam, DenseAdagrad
        if self.opt == OPT_ADAM:
            return DenseAdam(params, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.wd)
        if self.opt == OPT_ADAGRAD:
            return DenseAdagrad(params, lr=self.lr, eps=self.eps, weight_decay=self.wd)
        return None

    def _check_pair_batch(self, source, target):
        """(B_s, B_t) of a two-domain batch: every tensor of a domain of one length, within the sizes the step was built for."""
        Bs, Bt = source[0].numel(), target[0].numel()
        if not (1 <= Bs <= self.max_source and 1 <= Bt <= self.max_target):
            raise ValueError(f'{type(self).__name__}: batches of {Bs} + {Bt} rows, sized for 1..{self.max_source} + 1..{self.max_target}')
        if any(x.numel() != Bs for x in source) or any(x.numel() != Bt for x in target):
            raise ValueError(f'{type(self).__name__}: ids and labels of a domain must have the same length')
        return Bs, Bt


class _DenseStep(_Step):
    """A step that also owns small dense parameters: they keep the exact dense Adam (plain SGD with opt='sgd') while the tables are
    updated row-wise.  ``params`` are the parameters themselves: the step sets their ``.grad`` and updates them in place."""

    def _dense_init(self, params):
        self.params = list(params)
        self.w_opt = self._dense_optimizer(self.params)

    def _dense_update(self, packed=None):
        """``packed``: the gradients as one vector in ``params`` order, each ``.grad`` becomes a view of it (None: the caller has set
        them).  Then the update; a parameter whose ``.grad`` is None does not move (torch.optim.Adam skips it too)."""
        if packed is not None:
            off = 0
            for q in self.params:
                q.grad = packed[off:off + q.numel()].view(q.shape)
                off += q.numel()
        if self.w_opt is not None:
            self.w_opt.step()
        else:
            with torch.no_grad():
                for q in self.params:
                    if q.grad is not None:
                        q.add_(q.grad + self.wd * q if self.wd else q.grad, alpha=-self.lr)


class _TwoTableStep(_Step):
    """What the steps on one (user table, item table) pair share: the tables, one ``RowwiseState`` per table (the caller's, or a fresh
    one) and the sizing of the scratch buffers."""

    def __init__(self, user_table, item_table, opt, lr, betas, eps, weight_decay, user_state, item_state):
        assert user_table.is_cuda and item_table.is_cuda, f'{type(self).__name__} needs ROCm device tensors'
        assert user_table.shape[1] == item_table.shape[1]
        super().__init__(opt, lr, betas, eps, weight_decay)
        self.U, self.I = user_table, item_table
        self.D = user_table.shape[1]
        self.ustate = user_state if user_state is not None else RowwiseState(user_table, self.opt)
        self.istate = item_state if item_state is not None else RowwiseState(item_table, self.opt)
        self._sort_rows = self._sort_rows_of(user_table, item_table)

    def _states(self):
        return self.ustate, self.istate

    def _sort_workspace(self, *n_keys):
        """(uint8 scratch, its size in bytes) of the two-table id sort: enough for each of the key counts given."""
        ws = self._sort_scratch(self.U.device, self._sort_rows, *n_keys)
        return ws, ws.numel()

    def _single_row_buffers(self, n):
        """(flags, heads) of the forward kernels that update single-occurrence rows themselves: four flag bytes per batch row."""
        words = ctypes.c_int64(0)
        B_._check(B_.load().cdr_bpr_step_fused_heads_words(n, ctypes.byref(words)), 'cdr_bpr_step_fused_heads_words')
        return (torch.zeros(4 * n, device=self.U.device, dtype=torch.uint8),
                torch.empty(int(words.value), device=self.U.device, dtype=torch.int32))


class FusedBPRStep(_TwoTableStep):
    """One object per (user table, item table) pair; buffers are sized for ``max_batch`` triples and reused."""

    def __init__(self, user_table, item_table, max_batch, opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, gamma=1e-10, reg_weight=0.0, user_state=None, item_state=None, fuse_singles=True, device_counts=True,
                 id_path='auto', norm_cache='auto', norm_cache_max_bytes=None):
        super().__init__(user_table, item_table, opt, lr, betas, eps, weight_decay, user_state, item_state)
        self.gamma, self.reg_weight = gamma, reg_weight
        dev = user_table.device
        Bm = int(max_batch)
        self.max_batch = Bm
        self.GU = torch.empty(Bm, self.D, device=dev, dtype=torch.float32)
        self.GP = torch.empty(Bm, self.D, device=dev, dtype=torch.float32)
        self.out6 = torch.zeros(12, device=dev, dtype=torch.float32)
        # one sort per step for BOTH tables (the radix sort costs the same ~0.16 ms for 1 M or 3 M pairs): the user keys
        # come out first, the item keys behind them with a table bit (key_base) the apply kernel subtracts again
        self.keys = torch.empty(3 * Bm, device=dev, dtype=torch.int32)
        self.perm = torch.empty(3 * Bm, device=dev, dtype=torch.int32)
        self.ws, self.ws_bytes = self._sort_workspace(3 * Bm)
        self._key_base = ctypes.c_uint32(0)
        # single-occurrence rows updated by the forward kernel (cdr_bpr_step_fused): D <= 256 like cdr_bpr_fwd_grad
        self.fuse_singles = bool(fuse_singles) and self.D % 4 == 0 and self.D <= 256 and os.environ.get('CDR_FUSE_SINGLES', '1') != '0'   # env: A/B runs
        # Adam update counts on the device (cdr_bpr_step_fused_dev): the step can then be captured in a hipGraph (``replayed`` keeps the
        # host mirrors in step); the host-count form stays available (device_counts=False: the sharded layouts drive it)
        self.device_counts = bool(device_counts) and self.fuse_singles
        self._hp_dev = None
        if self.fuse_singles:
            self.flags, self.heads = self._single_row_buffers(Bm)               # flags: {user, positive, negative, -} per triple
        # Ids without a sort (round 6, csrc/cdr_step.hip): batches of 16,448 ... 131,072 triples take their single-occurrence flags from one
        # counter per table row and sort only the duplicate occurrences.  'auto': on, and moved to the sorted path (and back) by the
        # duplicate statistics the step leaves in heads[2:4] -- read back asynchronously, one step late, never waited for; 'count' / 'sort' pin it.
        self.id_path = os.environ.get('CDR_ID_PATH', id_path)
        assert self.id_path in ('auto', 'count', 'sort')
        self._count = None
        self._use_count = self.id_path != 'sort'
        self._stat = None
        self._count_on = False
        # EmbLoss norms from the tables' squared-norm records (RowwiseState.n2) instead of a gather of two rows per triple: sorted path,
        # reg_weight != 0, lazy Adam / SGD, not while capturing.  'auto': batches above COUNT_MAX_B (a table-sized array per table pays for
        # itself only where the gather is a visible share of the step); 'on': any batch; 'off': never.  ``norm_cache_max_bytes``: the most
        # one table's records may take (None: whatever leaves RowwiseState.NORMS_MARGIN_BYTES free).
        self.norm_cache = os.environ.get('CDR_NORM_CACHE', norm_cache)          # env: A/B runs
        assert self.norm_cache in ('auto', 'on', 'off')
        self.norm_cache_max_bytes = norm_cache_max_bytes
        self._nc_runs = None

    COUNT_MIN_B, COUNT_MAX_B = 16448, 131072

    def _count_buffers(self):
        if self._count is None:
            dev = self.U.device
            need = self._query_bytes('cdr_id_count_workspace_bytes', min(self.max_batch, self.COUNT_MAX_B))
            self._count = (torch.zeros(self.U.shape[0], device=dev, dtype=torch.int32), torch.zeros(self.I.shape[0], device=dev, dtype=torch.int32),
                           torch.empty(need, device=dev, dtype=torch.uint8))
        return self._count

    def _select_id_path(self, B):
        """Hands the counters to (or takes them from) the native context of the current stream before a fused step; folds in the statistics
        of an EARLIER step if their copy has landed (never waits)."""
        ctxh = B_.ctx(self.U.device)
        in_range = self.fuse_singles and self.COUNT_MIN_B <= B <= self.COUNT_MAX_B
        capturing = torch.cuda.is_current_stream_capturing()
        if in_range and self.id_path == 'auto' and not capturing:
            if self._stat is not None and self._stat[1].query():
                nd, maxc = int(self._stat[0][2]), int(self._stat[0][3])
                nB = self._stat[2]
                if self._use_count and (nd > 10240 or maxc > 256):
                    self._use_count = False                  # a skewed stream: same-address counter updates and a long duplicate list -- the sort serves it better
                elif not self._use_count and nd <= 8192:     # (the sorted path reports the duplicate occurrences only: heads[3] stays 0 there)
                    self._use_count = True
                self._stat = None
        on = in_range and self._use_count and not (capturing and self._count is None)     # (never allocate + zero-fill 4 B per table row inside a capture)
        self._count_on = on
        if on:
            cu, ci, ws = self._count_buffers()
            B_.call('cdr_ctx_set_id_counters', ctxh, B_.raw(cu), cu.numel(), B_.raw(ci), ci.numel(), B_.raw(ws), ws.numel())
        else:
            B_.call('cdr_ctx_set_id_counters', ctxh, None, 0, None, 0, None, 0)
        return in_range and self.id_path == 'auto' and not capturing

    def _select_norm_cache(self, B):
        """Hands the two tables' squared-norm records to the native context of the current stream if this step can use them and they are
        current (or due to be built: RowwiseState.norms_ready); True if the step runs cached."""
        states = (self.ustate, self.istate)
        self._nc_runs = None
        if torch.cuda.is_current_stream_capturing():
            for st in states:                                    # (the captured launches gather, and their replays move rows)
                st.n2_valid, st._n2_run = False, 0
            return False
        eligible = (self.norm_cache != 'off' and self.fuse_singles and not self._count_on and self.reg_weight != 0
                    and (self.norm_cache == 'on' or B > self.COUNT_MAX_B) and not any(st.exact for st in states))
        if not eligible:
            return False
        ready = [st.norms_ready(self.norm_cache_max_bytes) for st in states]         # (both: two stale tables are rebuilt in the same step)
        if all(ready):
            us, its = states
            B_.call('cdr_ctx_set_norm_cache', B_.ctx(self.U.device), B_.f32(us.n2), us.table.shape[0], B_.f32(its.n2), its.table.shape[0])
            return True
        self._nc_runs = [st._n2_run for st in states]
        return False

    def _advance(self, cached, device_bumped=False):
        for i, st in enumerate((self.ustate, self.istate)):
            st.advance(device_bumped=device_bumped, keeps_norms=cached)
            if self._nc_runs is not None:                        # an eligible step that gathered: one more towards the rebuild
                st._n2_run = self._nc_runs[i] + 1

    def _note_stats(self, B):
        if self._stat is None:
            host = torch.empty(4, dtype=torch.int32, pin_memory=True)
            host.copy_(self.heads[:4], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._stat = (host, ev, B)

    def step(self, uid, pid, nid):
        """uid/pid/nid: int64 device tensors [B].  Returns the device tensor out6 (view; [0] = total loss)."""
        B = uid.numel()
        assert B <= self.max_batch
        if self.fuse_singles:
            return self._step_fused(uid, pid, nid, B)
        B_.call('cdr_bpr_fwd_grad', B_.ctx(self.U.device), B_.stream(), B_.f32(self.U), B_.f32(self.I), self.D, B_.i64(uid),
                B_.i64(pid), B_.i64(nid), B, 0, float(self.gamma), float(self.reg_weight), B_.f32(self.out6), B_.f32(self.GU),
                B_.f32(self.GP), 0)
        return self.sort_apply(uid, pid, nid)

    def _step_fused(self, uid, pid, nid, B):
        """Batch norms and sort first, then ONE pass that also applies the optimizer to every row occurring once in the batch; the
        segmented applies see the duplicate rows only (csrc/cdr_step.hip, "single-occurrence rows in the forward")."""
        us, its = self.ustate, self.istate
        watch = self._select_id_path(B)
        try:
            cached = self._select_norm_cache(B)
            return self._step_fused_call(uid, pid, nid, B, us, its, cached)
        finally:
            # (the context is shared by every step object of this stream: it must not keep pointers into this object's buffers)
            B_.call('cdr_ctx_set_id_counters', B_.ctx(self.U.device), None, 0, None, 0, None, 0)
            B_.call('cdr_ctx_set_norm_cache', B_.ctx(self.U.device), None, 0, None, 0)
            self._steps_seen = self.__dict__.get('_steps_seen', 0) + 1
            if watch and (self._steps_seen & 15) == 1:          # every 16th step: one 16-byte copy, read when it has landed
                self._note_stats(B)

    def _step_fused_call(self, uid, pid, nid, B, us, its, cached=False):
        if self.opt == OPT_ADAM and self.device_counts:
            # the capturable form: the update counts live on the device and the call advances them itself (the host mirrors follow)
            if self._hp_dev is None:
                self._hp_dev = torch.zeros(4, device=self.U.device, dtype=torch.float32)
            su, si = us.step_dev, its.step_dev
            B_.call('cdr_bpr_step_fused_dev', B_.ctx(self.U.device), B_.stream(), self.opt, B_.f32(us.table), B_.f32(us.exp_avg),
                    B_.f32(us.exp_avg_sq), us.table.shape[0], B_.f32(its.table), B_.f32(its.exp_avg), B_.f32(its.exp_avg_sq),
                    its.table.shape[0], self.D, B_.i64(uid), B_.i64(pid), B_.i64(nid), B, float(self.gamma),
                    float(self.reg_weight), *self._hp(), B_.i64(su), B_.i64(si), B_.f32(self._hp_dev), B_.f32(self.out6), B_.f32(self.GU),
                    B_.f32(self.GP), B_.raw(self.keys), B_.raw(self.perm), B_.raw(self.flags), B_.raw(self.heads), B_.raw(self.ws), self.ws_bytes)
            if not torch.cuda.is_current_stream_capturing():
                self._advance(cached, device_bumped=True)
            return self.out6
        self._advance(cached)
        B_.call('cdr_bpr_step_fused', B_.ctx(self.U.device), B_.stream(), self.opt, B_.f32(us.table), B_.f32(us.exp_avg),
                B_.f32(us.exp_avg_sq), us.table.shape[0], B_.f32(its.table), B_.f32(its.exp_avg), B_.f32(its.exp_avg_sq),
                its.table.shape[0], self.D, B_.i64(uid), B_.i64(pid), B_.i64(nid), B, float(self.gamma),
                float(self.reg_weight), *self._hp(), us.step, its.step, B_.f32(self.out6), B_.f32(self.GU), B_.f32(self.GP), B_.raw(self.keys),
                B_.raw(self.perm), B_.raw(self.flags), B_.raw(self.heads), B_.raw(self.ws), self.ws_bytes)
        return self.out6

    def sort_apply(self, uid, pid, nid):
        """Second half of the step: GU / GP / out6[4:6] are in place (written by the forward kernel); one sort for both tables,
        two row-wise applies."""
        self.sort_ids(uid, pid, nid)
        return self.apply_sorted(uid.numel())

    def sort_ids(self, uid, pid, nid):
        """The id sort alone -- it needs nothing but the ids, so dimshard.py runs it under the all-reduce of the partial scores."""
        B = uid.numel()
        B_.call('cdr_sort_ids_two_tables', B_.ctx(self.U.device), B_.stream(), B_.i64(uid), B, self.U.shape[0], B_.i64(pid), B,
                B_.i64(nid), B, self.I.shape[0], B_.raw(self.keys), B_.raw(self.perm), ctypes.byref(self._key_base), B_.raw(self.ws),
                self.ws_bytes)

    def apply_sorted(self, B):
        ctxh = B_.ctx(self.U.device)
        self._apply(ctxh, self.ustate, self.D, self.keys[:B], self.perm[:B], B, self.GU, B, B, self.out6[4:5], 0)
        self._apply(ctxh, self.istate, self.D, self.keys[B:3 * B], self.perm[B:3 * B], 2 * B, self.GP, B, B, self.out6[5:6],
                    self._key_base.value)
        return self.out6


class KMajorBPRStep(_TwoTableStep):
    """The fused BPR step cut along recbole's pairwise batch layout (crossdomain_sampler.py:148-152; emcdr.py:123-131): S positives
    tiled k times with k-major negatives.  One lane group per POSITIVE in the forward (u, p gathered once, not k times), one
    gradient row per positive for the user table, and no item gradient rows at all: the item apply rebuilds each occurrence's
    row as coefficient * user row (csrc/cdr_kstep.hip).  Same loss and same per-row gradients as FusedBPRStep on the B = S k
    rows.  Batches whose item list fits the small rank sort (S k + S <= 8192) run as 4 launches behind one native call with device-side Adam
    counters and can be replayed as a hipGraph (``capture``)."""

    def __init__(self, user_table, item_table, max_positives, k=1, opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, gamma=1e-10, reg_weight=0.0, user_state=None, item_state=None, fuse_singles=True):
        refuse_adagrad('KMajorBPRStep', opt_code(opt))                           # (before the base allocates any optimizer state)
        super().__init__(user_table, item_table, opt, lr, betas, eps, weight_decay, user_state, item_state)
        self.k = int(k)
        self.gamma, self.reg_weight = gamma, reg_weight
        dev = user_table.device
        Sm = int(max_positives)
        Bm = Sm * self.k
        self.max_positives = Sm
        self.GU = torch.empty(Sm, self.D, device=dev, dtype=torch.float32)
        # large batches: rows that occur once are updated by the forward kernel (cdr_bpr_step_fused_kmajor); the duplicate item
        # occurrences get their gradient row written (the user row it is made of is updated by that same kernel) instead of a record
        self.fuse_singles = (bool(fuse_singles) and (Sm + Bm) > 8192 and self.D % 4 == 0 and self.D <= 256 and self.k <= 64
                             and os.environ.get('CDR_FUSE_SINGLES', '1') != '0')
        if self.fuse_singles:
            fb, hw = ctypes.c_int64(0), ctypes.c_int64(0)
            B_._check(B_.load().cdr_bpr_step_fused_kmajor_sizes(Sm, self.k, ctypes.byref(fb), ctypes.byref(hw)), 'cdr_bpr_step_fused_kmajor_sizes')
            self.GI = torch.empty(Sm + Bm, self.D, device=dev, dtype=torch.float32)
            self.flags = torch.zeros(int(fb.value), device=dev, dtype=torch.uint8)
            self.heads = torch.empty(int(hw.value), device=dev, dtype=torch.int32)
            self.rec = None
        else:
            self.rec = torch.empty(2 * (Sm + Bm), device=dev, dtype=torch.int32)      # 8-byte {user row, coefficient} records
        self.out6 = torch.zeros(12, device=dev, dtype=torch.float32)
        n_all = 2 * Sm + Bm                                                           # user list [S] ++ item list [S + B]
        self.keys = torch.empty(n_all, device=dev, dtype=torch.int32)
        self.perm = torch.empty(n_all, device=dev, dtype=torch.int32)
        self.small = (Sm + Bm) <= 8192                # the rank sort is quadratic: past this the radix sort wins
        self.rank = torch.zeros(n_all, device=dev, dtype=torch.int32) if self.small else None   # scratch of the rank sort
        self.ws = None
        self._key_base = ctypes.c_uint32(0)
        if not self.small:
            self.ws, _ = self._sort_workspace(n_all)
        self._graph = None

    def step(self, uid, pid, nid):
        """uid / pid: int64 [S] (or the reference's tiled [S k]: the first S entries are read), nid: int64 [S k] k-major.
        Returns out6 (view; [0] = total loss)."""
        B = nid.numel()
        S = B // self.k
        assert S * self.k == B and S <= self.max_positives and uid.numel() >= S and pid.numel() >= S
        if self.fuse_singles:
            us, its = self.ustate, self.istate
            us.advance(); its.advance()
            B_.call('cdr_bpr_step_fused_kmajor', B_.ctx(self.U.device), B_.stream(), self.opt, B_.f32(us.table), B_.f32(us.exp_avg),
                    B_.f32(us.exp_avg_sq), us.table.shape[0], B_.f32(its.table), B_.f32(its.exp_avg), B_.f32(its.exp_avg_sq),
                    its.table.shape[0], self.D, B_.i64(uid), B_.i64(pid), B_.i64(nid), S, self.k, float(self.gamma), float(self.reg_weight),
                    *self._hp(), us.step, its.step, B_.f32(self.out6), B_.f32(self.GU), B_.f32(self.GI), B_.raw(self.keys), B_.raw(self.perm),
                    B_.raw(self.flags), B_.raw(self.heads), B_.raw(self.ws), self.ws.numel())
            return self.out6
        self._enqueue(uid, pid, nid, S)
        self.ustate.advance(device_bumped=True)
        self.istate.advance(device_bumped=True)
        return self.out6

    def _enqueue(self, uid, pid, nid, S):
        dev = self.U.device
        ctxh, s = B_.ctx(dev), B_.stream()
        B = S * self.k
        adam = self.opt == OPT_ADAM
        ud, idv = (self.ustate.step_dev, self.istate.step_dev) if adam else (None, None)
        hp = self._hp()
        if self.small:
            # four launches behind one call: {forward || rank count}, {scatter || loss finish}, item apply, user apply
            us, its = self.ustate, self.istate
            B_.call('cdr_bpr_step_small', ctxh, s, self.opt, B_.f32(us.table), B_.f32(us.exp_avg), B_.f32(us.exp_avg_sq),
                    B_.f32(its.table), B_.f32(its.exp_avg), B_.f32(its.exp_avg_sq), self.D, B_.i64(uid), B_.i64(pid), B_.i64(nid), S,
                    self.k, float(self.gamma), float(self.reg_weight), *hp, B_.i64(ud), B_.i64(idv), B_.f32(self.out6),
                    B_.f32(self.GU), B_.raw(self.rec), B_.raw(self.keys), B_.raw(self.perm), B_.raw(self.rank),
                    max(self.U.shape[0], self.I.shape[0]))
            return
        B_.call('cdr_bpr_fwd_grad_kmajor', ctxh, s, B_.f32(self.U), B_.f32(self.I), self.D, B_.i64(uid), B_.i64(pid), B_.i64(nid), S,
                self.k, float(self.gamma), float(self.reg_weight), B_.f32(self.out6), B_.f32(self.GU), B_.raw(self.rec),
                B_.i64(ud), B_.i64(idv))
        base = self._sort(uid, pid, nid, S, ctxh)
        # the item apply reads the PRE-step user rows: it runs first
        st = self.istate
        tab, m, v = self._offset(st, base)
        B_.call('cdr_rowwise_apply_scaled', ctxh, s, self.opt, tab, m, v, self.D, B_.raw(self.keys[S:2 * S + B]),
                B_.raw(self.perm[S:2 * S + B]), S + B, B_.raw(self.rec), B_.f32(self.U), S, B_.f32(self.out6[5:6]), *hp,
                st.step + 1, B_.i64(idv), 0)
        st = self.ustate
        B_.call('cdr_rowwise_apply_rows', ctxh, s, self.opt, B_.f32(st.table), B_.f32(st.exp_avg), B_.f32(st.exp_avg_sq), self.D,
                B_.raw(self.keys[:S]), B_.raw(self.perm[:S]), S, B_.f32(self.GU), S, B_.f32(self.out6[4:5]), *hp, st.step + 1,
                B_.i64(ud), 0)

    def _sort(self, uid, pid, nid, S, ctxh):
        """User list [S] at keys[0:S], item list [pid | nid] at keys[S:2S+B]; returns the item keys' table bit (0 for the rank sort)."""
        B = S * self.k
        if self.small:
            arr = lambda xs: (ctypes.c_void_p * 2)(*xs)
            i64s = lambda xs: (ctypes.c_int64 * 2)(*xs)
            B_._alive.extend([uid, pid, nid])
            B_.call('cdr_sort_ids_small', B_.stream(), 2, arr([uid.data_ptr(), pid.data_ptr()]), i64s([S, S]), arr([None, nid.data_ptr()]),
                    i64s([0, B]), i64s([0, S]), B_.raw(self.keys), B_.raw(self.perm), B_.raw(self.rank), max(self.U.shape[0], self.I.shape[0]))
            return 0
        B_.call('cdr_sort_ids_two_tables', ctxh, B_.stream(), B_.i64(uid), S, self.U.shape[0], B_.i64(pid), S, B_.i64(nid), B,
                self.I.shape[0], B_.raw(self.keys), B_.raw(self.perm), ctypes.byref(self._key_base), B_.raw(self.ws), self.ws.numel())
        return int(self._key_base.value)

    def _offset(self, st, key_base):
        """Table pointers moved back by key_base rows (keys of a two-table sort carry the table bit; see cdr_rowwise_apply)."""
        off = 4 * key_base * self.D
        f = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() - off)
        B_._alive.extend([st.table, st.exp_avg, st.exp_avg_sq])
        return f(st.table), f(st.exp_avg), f(st.exp_avg_sq)

    # ---- hipGraph replay of the whole step (small batches: the reference's default train_batch_size is 2,048) ----------
    def capture(self, S):
        """Capture the 6-launch step for batches of exactly S positives.  ``replay(uid, pid, nid)`` then costs three small id
        copies + one graph launch on the host."""
        assert self.small and self.opt in (OPT_ADAM, OPT_SGD)
        dev = self.U.device
        B = S * self.k
        self._S = S
        self._ids = (torch.zeros(S, device=dev, dtype=torch.int64), torch.zeros(S, device=dev, dtype=torch.int64),
                     torch.zeros(B, device=dev, dtype=torch.int64))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            B_.ctx(dev)                                   # the native context of the capture stream must exist beforehand
            if self.opt == OPT_ADAM:
                self.ustate.step_dev, self.istate.step_dev
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        with B_.capturing(self._graph, side):
            self._enqueue(self._ids[0], self._ids[1], self._ids[2], S)
        return self

    @property
    def static_ids(self):
        """(uid [S], pid [S], nid [S k]): the buffers the captured graph reads.  A producer that writes its batch straight into
        them (the device sampler / loader) can call ``replay()`` without arguments: no id copies at all."""
        return self._ids

    def replay(self, uid=None, pid=None, nid=None):
        S = self._S
        if uid is not None:
            self._ids[0].copy_(uid[:S]); self._ids[1].copy_(pid[:S]); self._ids[2].copy_(nid)
        self._graph.replay()
        self.replayed()
        return self.out6


class FusedPointStep(_TwoTableStep):
    """Pointwise counterpart of FusedBPRStep: rows (user, item, label) -- recbole's pointwise layout, sampled negatives stacked
    behind the positives with label 0 -- MSE on the raw dot (EMCDR's default MF latent factor model, emcdr.py:111-122) or BCE
    on sigmoid(dot), plus ``reg_weight * EmbLoss(u_rows, i_rows)``; both tables updated row-wise on the batch's rows."""

    def __init__(self, user_table, item_table, max_batch, loss='mse', opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, reg_weight=0.0, user_state=None, item_state=None, fuse_singles=True):
        super().__init__(user_table, item_table, opt, lr, betas, eps, weight_decay, user_state, item_state)
        self.kind = B_.CDR_LOSS_MSE if loss == 'mse' else B_.CDR_LOSS_BCE
        self.reg_weight = reg_weight
        dev = user_table.device
        Bm = int(max_batch)
        self.max_batch = Bm
        self.GU = torch.empty(Bm, self.D, device=dev, dtype=torch.float32)
        self.GI = torch.empty(Bm, self.D, device=dev, dtype=torch.float32)
        self.out6 = torch.zeros(12, device=dev, dtype=torch.float32)
        self.keys = torch.empty(2 * Bm, device=dev, dtype=torch.int32)        # one sort for both tables (see FusedBPRStep)
        self.perm = torch.empty(2 * Bm, device=dev, dtype=torch.int32)
        self.ws, _ = self._sort_workspace(2 * Bm)
        self._key_base = ctypes.c_uint32(0)
        # round 5: rows that occur once in the batch are updated by the forward kernel itself (cdr_point_step_fused), as in FusedBPRStep;
        # fuse_singles=False (or CDR_FUSE_SINGLES=0) keeps the two-pass form (the dimension-sharded step drives its halves)
        self.fuse_singles = bool(fuse_singles) and self.D % 4 == 0 and self.D <= 256 and os.environ.get('CDR_FUSE_SINGLES', '1') != '0'
        if self.fuse_singles:
            self.flags, self.heads = self._single_row_buffers(Bm)               # flags: {user, item, -, -} per row

    def step(self, uid, iid, label):
        """uid / iid int64 [B], label fp32 [B].  Returns out6 (view; [0] = total loss)."""
        B = uid.numel()
        assert B <= self.max_batch
        if self.fuse_singles:
            us, its = self.ustate, self.istate
            us.advance(); its.advance()
            B_.call('cdr_point_step_fused', B_.ctx(self.U.device), B_.stream(), self.kind, self.opt, B_.f32(us.table), B_.f32(us.exp_avg),
                    B_.f32(us.exp_avg_sq), us.table.shape[0], B_.f32(its.table), B_.f32(its.exp_avg), B_.f32(its.exp_avg_sq), its.table.shape[0],
                    self.D, B_.i64(uid), B_.i64(iid), B_.f32(label), B, float(self.reg_weight), *self._hp(), us.step, its.step, B_.f32(self.out6),
                    B_.f32(self.GU), B_.f32(self.GI), B_.raw(self.keys), B_.raw(self.perm), B_.raw(self.flags), B_.raw(self.heads), B_.raw(self.ws),
                    self.ws.numel())
            return self.out6
        B_.call('cdr_point_fwd_grad', B_.ctx(self.U.device), B_.stream(), self.kind, B_.f32(self.U), B_.f32(self.I), self.D, B_.i64(uid),
                B_.i64(iid), B_.f32(label), B, float(self.reg_weight), B_.f32(self.out6), B_.f32(self.GU), B_.f32(self.GI))
        return self.sort_apply(uid, iid)

    def sort_apply(self, uid, iid):
        """Second half of the step (GU / GI / out6[4:6] in place): one sort for both tables, two row-wise applies."""
        self.sort_ids(uid, iid)
        return self.apply_sorted(uid.numel())

    def sort_ids(self, uid, iid):
        B = uid.numel()
        B_.call('cdr_sort_ids_two_tables', B_.ctx(self.U.device), B_.stream(), B_.i64(uid), B, self.U.shape[0], B_.i64(iid), B, None, 0,
                self.I.shape[0], B_.raw(self.keys), B_.raw(self.perm), ctypes.byref(self._key_base), B_.raw(self.ws), self.ws.numel())

    def apply_sorted(self, B):
        ctxh = B_.ctx(self.U.device)
        for st, lo, G, coef, base in ((self.ustate, 0, self.GU, self.out6[4:5], 0),
                                      (self.istate, B, self.GI, self.out6[5:6], self._key_base.value)):
            self._apply(ctxh, st, self.D, self.keys[lo:lo + B], self.perm[lo:lo + B], B, G, B, B, coef, base)
        return self.out6


class FusedTripletStep(_TwoTableStep):
    """SSCDR's domain step (sscdr.py:120-128, 133-159): TripletMarginLoss(margin) on the squared-norm "normalised" rows of (user,
    positive, negative) triples, both tables updated row-wise on the batch's rows.  The loss has no EmbLoss.  Five calls: forward +
    one compact gradient row per occurrence (cdr_triplet_fwd_grad), one sort for both tables, two segmented applies.  The update counts
    are the host's: not capturable."""

    def __init__(self, user_table, item_table, max_batch, margin=1.0, opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, user_state=None, item_state=None):
        if user_table.shape[1] % 4 != 0 or user_table.shape[1] > 256:            # (before the base allocates any optimizer state)
            raise ValueError(f'FusedTripletStep: D must be a multiple of 4 and <= 256, got {user_table.shape[1]}')
        super().__init__(user_table, item_table, opt, lr, betas, eps, weight_decay, user_state, item_state)
        self.margin = float(margin)
        self.loss_eps = 1e-6                                                     # nn.TripletMarginLoss's eps (sscdr.py:69)
        dev = user_table.device
        Bm = int(max_batch)
        self.max_batch = Bm
        self.GU = torch.empty(Bm, self.D, device=dev, dtype=torch.float32)
        self.GI = torch.empty(2 * Bm, self.D, device=dev, dtype=torch.float32)
        self.out3 = torch.zeros(3, device=dev, dtype=torch.float32)
        self.keys = torch.empty(3 * Bm, device=dev, dtype=torch.int32)          # one sort for both tables (see FusedBPRStep)
        self.perm = torch.empty(3 * Bm, device=dev, dtype=torch.int32)
        # (the sort switches configuration at 2^18 keys: a short tail batch may need more scratch than a full one)
        self.ws, _ = self._sort_workspace(3 * Bm, min(3 * Bm, (1 << 18) - 1))
        self._key_base = ctypes.c_uint32(0)

    def step(self, uid, pid, nid):
        """uid / pid / nid: int64 device tensors [B].  Returns out3 (view): [0] the loss, [1] the triples with an open hinge."""
        B = uid.numel()
        if not 1 <= B <= self.max_batch or pid.numel() != B or nid.numel() != B:
            raise ValueError(f'FusedTripletStep: {B} / {pid.numel()} / {nid.numel()} ids, sized for 1..{self.max_batch} triples')
        ctxh, s = B_.ctx(self.U.device), B_.stream()
        GI = self.GI[:2 * B]                                                     # negatives at row B of THIS batch
        B_.call('cdr_triplet_fwd_grad', ctxh, s, B_.f32(self.U), B_.f32(self.I), self.D, B_.i64(uid), B_.i64(pid), B_.i64(nid), B,
                self.margin, self.loss_eps, B_.f32(self.out3), B_.f32(self.GU), B_.f32(GI))
        B_.call('cdr_sort_ids_two_tables', ctxh, s, B_.i64(uid), B, self.U.shape[0], B_.i64(pid), B, B_.i64(nid), B, self.I.shape[0],
                B_.raw(self.keys), B_.raw(self.perm), ctypes.byref(self._key_base), B_.raw(self.ws), self.ws.numel())
        self.ustate.advance(); self.istate.advance()
        # every occurrence has its own gradient row: neg_start = n (nothing is negated), reg_limit = 0 (no EmbLoss)
        for st, lo, n, G, base in ((self.ustate, 0, B, self.GU, 0), (self.istate, B, 2 * B, GI, self._key_base.value)):
            self._apply(ctxh, st, self.D, self.keys[lo:lo + n], self.perm[lo:lo + n], n, G, n, 0, None, base, advance=False)
        return self.out3


class FusedCLFMStep(_DenseStep):
    """CLFM's BOTH-phase step (clfm.py:74-124): per domain  p = sigmoid(<W_d U_d[uid], I_d[iid]>)  with the stacked weight
    W_d = [shared_linear ; <domain>_only_linear] [Di, Du], loss = alpha (BCE_s + reg EmbLoss_s) + (1 - alpha) (BCE_t + reg EmbLoss_t).  The
    four tables (user and item table of each domain, widths Du and Di) are updated row-wise on the batch's rows; the three small
    weights keep the exact dense Adam (plain SGD with opt='sgd'), as in SSCDRMapStep.  Per domain: cdr_clfm_fwd_grad (csrc/cdr_clfm.hip:
    the factor map, the loss and the three gradient contractions in one pass, + its finishing launch), one sort for both tables, two
    segmented applies; both forwards run before anything is updated, so both domains see the pre-step weights.  The shared weight's
    gradient is the sum of the two domains' first ``share`` rows of dW.  The update counts are the host's: not capturable.

    ``weights``: (shared_linear.weight or None, source_only_linear.weight or None, target_only_linear.weight or None) -- the
    parameters themselves: the step sets their ``.grad`` and updates them in place."""

    MAX_DIM = 128                                                                # CDR_CLFM_MAX_DIM

    @classmethod
    def check_widths(cls, Du, Di):
        if not (4 <= Du <= cls.MAX_DIM and 4 <= Di <= cls.MAX_DIM and Du % 4 == 0 and Di % 4 == 0):
            raise ValueError(f'FusedCLFMStep: user_embedding_size and item embedding size must be multiples of 4 in 4..{cls.MAX_DIM} '
                             f'(the weight tile lives in LDS), got {Du} and {Di}')

    def __init__(self, source_user, source_item, target_user, target_item, weights, max_source, max_target, alpha, reg_weight, opt='adam',
                 lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, states=None):
        tables = (source_user, source_item, target_user, target_item)
        assert all(t.is_cuda for t in tables), 'FusedCLFMStep needs ROCm device tensors'
        Du, Di = source_user.shape[1], source_item.shape[1]
        if target_user.shape[1] != Du or target_item.shape[1] != Di:
            raise ValueError(f'FusedCLFMStep: the domains\' tables differ in width ({tuple(t.shape[1] for t in tables)})')
        self.check_widths(Du, Di)                                                # (before anything is allocated)
        shared, s_only, t_only = weights
        self.share = 0 if shared is None else shared.shape[0]
        for w, rows in ((shared, self.share), (s_only, Di - self.share), (t_only, Di - self.share)):
            if (w is None) != (rows == 0) or (w is not None and tuple(w.shape) != (rows, Du)):
                raise ValueError(f'FusedCLFMStep: the stacked weights must be [{self.share} ; {Di - self.share}] x {Du}')
        super().__init__(opt, lr, betas, eps, weight_decay)
        self.Du, self.Di = Du, Di
        self.tables = tables
        self.weights = (shared, s_only, t_only)
        self.alpha, self.reg_weight = float(alpha), float(reg_weight)
        self.states = self._own_states(tables, states)
        self._dense_init(w for w in self.weights if w is not None)
        dev = source_user.device
        self.max_source, self.max_target = int(max_source), int(max_target)
        Bm = max(self.max_source, self.max_target)
        self.GU = tuple(torch.empty(n, Du, device=dev, dtype=torch.float32) for n in (self.max_source, self.max_target))
        self.GI = tuple(torch.empty(n, Di, device=dev, dtype=torch.float32) for n in (self.max_source, self.max_target))
        self.dW = torch.zeros(2, Di, Du, device=dev, dtype=torch.float32)
        self.out16 = torch.zeros(16, device=dev, dtype=torch.float32)           # out8 of the source, out8 of the target
        # (the grid, and with it the size, grows with B)
        self.fws = torch.empty(self._query_bytes('cdr_clfm_fwd_grad_workspace_bytes', Bm, Du, Di), device=dev, dtype=torch.uint8)
        # one sort per domain: user keys, then item keys
        self.keys, self.perm, self.ws = self._sort_buffers(2 * Bm, self._sort_rows_of(*tables), dev)
        self._key_base = ctypes.c_uint32(0)

    def _states(self):
        return self.states

    def _stacked(self, only):
        """[shared ; only] as one contiguous [Di, Du] matrix, exactly as ``CLFM._factors`` stacks it."""
        ws = [w.data for w in (self.weights[0], only) if w is not None]
        return ws[0].contiguous() if len(ws) == 1 else torch.cat(ws, dim=0)

    @torch.no_grad()
    def step(self, su, si, ys, tu, ti, yt):
        """su / si int64 [B_s], ys fp32 [B_s] (source rows); tu / ti int64 [B_t], yt fp32 [B_t] (target rows).  Returns the total loss
        (device [1]); ``out16`` keeps each domain's {weighted total, BCE, EmbLoss, ||U rows||, ||I rows||, c_u, c_i, 0}."""
        Bs, Bt = self._check_pair_batch((su, si, ys), (tu, ti, yt))
        dev = self.tables[0].device
        ctxh, s = B_.ctx(dev), B_.stream()
        S, Du, Di = self.share, self.Du, self.Di
        doms = ((0, su, si, ys, Bs, self.alpha, self._stacked(self.weights[1])),
                (1, tu, ti, yt, Bt, 1.0 - self.alpha, self._stacked(self.weights[2])))
        for d, uid, iid, y, n, w, W in doms:                       # both forwards first: both domains see the pre-step weights
            B_.call('cdr_clfm_fwd_grad', ctxh, s, B_.f32(self.tables[2 * d]), B_.f32(self.tables[2 * d + 1]), Du, Di, B_.f32(W), B_.i64(uid),
                    B_.i64(iid), B_.f32(y), n, w, self.reg_weight, B_.f32(self.out16[8 * d:8 * d + 8]), B_.f32(self.GU[d][:n]),
                    B_.f32(self.GI[d][:n]), B_.f32(self.dW[d]), B_.raw(self.fws), self.fws.numel())
        for d, uid, iid, y, n, w, W in doms:
            ust, ist = self.states[2 * d], self.states[2 * d + 1]
            B_.call('cdr_sort_ids_two_tables', ctxh, s, B_.i64(uid), n, ust.table.shape[0], B_.i64(iid), n, None, 0, ist.table.shape[0],
                    B_.raw(self.keys), B_.raw(self.perm), ctypes.byref(self._key_base), B_.raw(self.ws), self.ws.numel())
            # one gradient row per occurrence (neg_start = n), EmbLoss on every occurrence (reg_limit = n) with the domain's coefficient
            for st, lo, D, G, coef, base in ((ust, 0, Du, self.GU[d], 8 * d + 5, 0), (ist, n, Di, self.GI[d], 8 * d + 6, self._key_base.value)):
                self._apply(ctxh, st, D, self.keys[lo:lo + n], self.perm[lo:lo + n], n, G[:n], n, n, self.out16[coef:coef + 1], base)
        shared, s_only, t_only = self.weights
        if shared is not None:
            shared.grad = self.dW[0, :S] + self.dW[1, :S]
        if s_only is not None:
            s_only.grad = self.dW[0, S:]
            t_only.grad = self.dW[1, S:]
        self._dense_update()
        return self.out16[0:1] + self.out16[8:9]


class FusedDTCDRStep(_DenseStep):
    """DTCDR's BOTH-phase step with the NeuMF tower (dtcdr.py:112-126, 182-199): per domain  p = sigmoid(head_d(mlp_d([max(Us[u], Ut[u]) |
    max(Is[i], It[i])])))  with dropout in front of every hidden layer, loss = alpha BCE_s + (1 - alpha) BCE_t.  Every occurrence feeds
    BOTH domains' tables (the maximum routes each element's gradient to the table that won it, half to each on an exact tie) and each of
    the four tables receives rows from both batches, so the gradient rows of both domains go into joint [B_s + B_t, D] buffers (source rows
    at 0, target rows at B_s) and each table advances ONCE per step, from the sum of a row's contributions, as in FusedPointPairStep.
    Per step: cdr_dtcdr_fwd_grad per domain (csrc/cdr_dtcdr.hip: the tower forward and backward, the routing and every parameter gradient in
    one pass, + its finishing launch) -- both before anything is updated --, ONE cdr_sort_ids_two_tables over ([su | tu], si ++ ti) (the
    user list is concatenated on the host side: one copy launch and one sort, against two cdr_sort_ids), four segmented applies (each
    sorted list serves both tables of its id space), then the exact dense Adam on the 12 tower parameters (plain SGD with opt='sgd'), as in
    FusedCLFMStep.  The update counts are the host's: not capturable.

    ``towers``: ((W_0, b_0, ..., w_out, b_out) of the source, the same of the target) -- the parameters themselves: the step sets their
    ``.grad`` and updates them in place."""

    MAX_DIM, MAX_HIDDEN, MAX_LAYERS = 128, 64, 3                                 # CDR_DTCDR_MAX_*

    @classmethod
    def check_widths(cls, D, hidden):
        hidden = list(hidden)
        if not (4 <= D <= cls.MAX_DIM and D % 4 == 0):
            raise ValueError(f'FusedDTCDRStep: embedding_size must be a multiple of 4 in 4..{cls.MAX_DIM}, got {D}')
        if not (1 <= len(hidden) <= cls.MAX_LAYERS and all(isinstance(h, int) and 1 <= h <= cls.MAX_HIDDEN for h in hidden)):
            raise ValueError(f'FusedDTCDRStep: mlp_hidden_size must be 1..{cls.MAX_LAYERS} layers of 1..{cls.MAX_HIDDEN} units '
                             f'(the tower lives in LDS), got {hidden}')

    def __init__(self, source_user, source_item, target_user, target_item, towers, max_source, max_target, alpha, dropout_prob=0.0,
                 opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, states=None):
        tables = (source_user, source_item, target_user, target_item)
        assert all(t.is_cuda for t in tables), 'FusedDTCDRStep needs ROCm device tensors'
        D = source_user.shape[1]
        if any(t.shape[1] != D for t in tables) or source_user.shape[0] != target_user.shape[0] or source_item.shape[0] != target_item.shape[0]:
            raise ValueError(f'FusedDTCDRStep: the four tables must share one width and the domains one id space '
                             f'({tuple(tuple(t.shape) for t in tables)})')
        hidden = [int(towers[0][2 * l].shape[0]) for l in range(len(towers[0]) // 2 - 1)]
        self.check_widths(D, hidden)                                             # (before anything is allocated)
        shapes = [s for i, o in zip([2 * D] + hidden, hidden) for s in ((o, i), (o,))] + [(1, hidden[-1]), (1,)]
        for tw in towers:
            if [tuple(p.shape) for p in tw] != shapes:
                raise ValueError(f'FusedDTCDRStep: a tower must be {shapes}, got {[tuple(p.shape) for p in tw]}')
        if not 0.0 <= float(dropout_prob) < 1.0:
            raise ValueError(f'FusedDTCDRStep: dropout_prob must be in [0, 1), got {dropout_prob}')
        super().__init__(opt, lr, betas, eps, weight_decay)
        self.D, self.hidden = D, hidden
        self._hidden_c = (ctypes.c_int * len(hidden))(*hidden)
        self.tables = tables
        self.towers = tuple(tuple(tw) for tw in towers)
        self.alpha, self.p = float(alpha), float(dropout_prob)
        self.states = self._own_states(tables, states)
        self._dense_init(p for tw in self.towers for p in tw)
        dev = source_user.device
        self.max_source, self.max_target = int(max_source), int(max_target)
        Nm = self.max_source + self.max_target
        self.G = tuple(torch.empty(Nm, D, device=dev, dtype=torch.float32) for _ in range(4))      # rows for Us, Is, Ut, It
        self.n_params = sum(p.numel() for p in self.towers[0])
        self.dP = torch.zeros(2, self.n_params, device=dev, dtype=torch.float32)
        self.out16 = torch.zeros(16, device=dev, dtype=torch.float32)           # out8 of the source, out8 of the target
        self.zero = torch.zeros(1, device=dev, dtype=torch.float32)             # the applies' EmbLoss coefficient: none
        # (the grid, and with it the size, grows with B)
        self.fws = torch.empty(self._workspace_bytes(max(self.max_source, self.max_target)), device=dev, dtype=torch.uint8)
        # one sort: user keys [su | tu], then item keys [si | ti]
        self.keys, self.perm, self.ws = self._sort_buffers(2 * Nm, self._sort_rows_of(*tables), dev)
        self._key_base = ctypes.c_uint32(0)

    def _states(self):
        return self.states

    def _workspace_bytes(self, B):
        return self._query_bytes('cdr_dtcdr_fwd_grad_workspace_bytes', B, self.D, len(self.hidden), self._hidden_c)

    def grid(self, B):
        """Workgroups cdr_dtcdr_fwd_grad launches for a batch of B rows (the workspace is one packed parameter vector per workgroup)."""
        return self._workspace_bytes(B) // (4 * self.n_params)

    @torch.no_grad()
    def forward_grads(self, su, si, ys, tu, ti, yt, seed=None):
        """Both domains' cdr_dtcdr_fwd_grad: fills ``G`` (rows [0, B_s) source, [B_s, B_s + B_t) target), ``dP`` and ``out16``."""
        Bs, Bt = self._check_pair_batch((su, si, ys), (tu, ti, yt))
        if seed is not None and (seed.dtype != torch.int64 or not seed.is_cuda):
            raise ValueError('FusedDTCDRStep: the dropout seed is a device int64 [1]')
        ctxh, s = B_.ctx(self.tables[0].device), B_.stream()
        p = self.p if seed is not None else 0.0
        Us, Is, Ut, It = self.tables
        for d, uid, iid, y, n, w, salt, row0 in ((0, su, si, ys, Bs, self.alpha, 0, 0), (1, tu, ti, yt, Bt, 1.0 - self.alpha, 64, Bs)):
            packed = torch.cat([q.data.reshape(-1) for q in self.towers[d]])
            B_.call('cdr_dtcdr_fwd_grad', ctxh, s, B_.f32(Us), B_.f32(Ut), B_.f32(Is), B_.f32(It), self.D, len(self.hidden), self._hidden_c,
                    B_.f32(packed), B_.i64(uid), B_.i64(iid), B_.f32(y), n, w, p, B_.i64(seed) if p > 0 else None, salt, row0,
                    B_.f32(self.out16[8 * d:8 * d + 8]), B_.f32(self.G[0]), B_.f32(self.G[2]), B_.f32(self.G[1]), B_.f32(self.G[3]),
                    B_.f32(self.dP[d]), B_.raw(self.fws), self.fws.numel())

    @torch.no_grad()
    def step(self, su, si, ys, tu, ti, yt, seed=None):
        """su / si int64 [B_s], ys fp32 [B_s] (source rows); tu / ti int64 [B_t], yt fp32 [B_t] (target rows); ``seed``: device int64 [1],
        the step's dropout counter (None: no dropout).  Returns the total loss (device [1]); ``out16`` keeps each domain's {weighted BCE,
        BCE, 0, ...}."""
        self.forward_grads(su, si, ys, tu, ti, yt, seed)            # both forwards first: both domains see the pre-step state
        Bs, Bt = su.numel(), tu.numel()
        n = Bs + Bt
        ctxh, s = B_.ctx(self.tables[0].device), B_.stream()
        users = torch.cat([su, tu])
        B_.call('cdr_sort_ids_two_tables', ctxh, s, B_.i64(users), n, self.tables[0].shape[0], B_.i64(si), Bs, B_.i64(ti), Bt,
                self.tables[1].shape[0], B_.raw(self.keys), B_.raw(self.perm), ctypes.byref(self._key_base), B_.raw(self.ws), self.ws.numel())
        # one gradient row per occurrence (neg_start = n), no EmbLoss (reg_limit = 0); table order: Us, Is, Ut, It
        for st, G, lo, base in ((self.states[0], self.G[0], 0, 0), (self.states[2], self.G[2], 0, 0),
                                (self.states[1], self.G[1], n, self._key_base.value), (self.states[3], self.G[3], n, self._key_base.value)):
            self._apply(ctxh, st, self.D, self.keys[lo:lo + n], self.perm[lo:lo + n], n, G[:n], n, 0, self.zero, base)
        self._dense_update(self.dP.view(-1))                        # (params: the source tower, then the target tower, as dP's rows)
        return self.out16[0:1] + self.out16[8:9]


class FusedDeepAPFStep(_DenseStep):
    """DeepAPF's BOTH-phase step (deepapf.py:69-152, 163-175): per domain the key id's share row and domain-only row, each multiplied with
    the other side's row and scored by the two-layer attention MLP (W1, b1, w2), the pair softmax with the share score masked where
    key > n_overlap (strictly), the merged row through the predict layer wp, loss = BCE_s + BCE_t.  Five live tables, named by role: the
    share table (fed by BOTH domains: their rows go into one joint [B_s + B_t, D] buffer, source rows at 0, target rows at B_s), and per
    domain the only table (indexed by the key id) and the other table.  ``key`` is the user in overlap_users mode and the item in
    overlap_items mode; the step itself does not know which.
    Per step: cdr_deepapf_fwd_grad per domain (csrc/cdr_deepapf.hip: the forward, the backward and every parameter gradient in one pass,
    + its finishing launch) -- both before anything is updated, so both domains see the pre-step state --, one cdr_sort_ids over
    [key_s | key_t] (two lists: no host concatenation) and one apply for the share table, per domain one cdr_sort_ids_two_tables(key |
    other) and two applies: three sorts, five applies, each table advances exactly ONCE per step and a share row named by both domains
    gets one update from the sum.  The four parameters are shared by the domains: their gradient is dP_source + dP_target, applied by the
    exact dense Adam (plain SGD with opt='sgd'), as in FusedCLFMStep.  The MLP the mode does not use and the share table of the other side
    are not given to the step: they get no gradient and do not move (torch.optim.Adam skips a parameter whose .grad is None).
    Lazy mode touches every row a batch names, masked share rows included: a masked occurrence contributes a zero gradient row, and its
    row takes the moment decay (and weight decay) of a zero-gradient update -- the rule DTCDR's losing rows follow.
    The update counts are the host's: not capturable.

    ``params``: (W1 [D, D], b1 [D], w2 [1, D], wp [1, D]) -- the parameters themselves: the step sets their ``.grad`` and updates them in
    place."""

    MAX_DIM = 128                                                                # CDR_DEEPAPF_MAX_DIM

    @classmethod
    def check_widths(cls, D):
        if not (isinstance(D, int) and 4 <= D <= cls.MAX_DIM and D % 4 == 0):
            raise ValueError(f'FusedDeepAPFStep: embedding_size must be a multiple of 4 in 4..{cls.MAX_DIM} (W1 lives in LDS), got {D}')

    def __init__(self, share, source_only, source_other, target_only, target_other, params, n_overlap, max_source, max_target, opt='adam',
                 lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, states=None):
        tables = (share, source_only, source_other, target_only, target_other)
        assert all(t.is_cuda for t in tables), 'FusedDeepAPFStep needs ROCm device tensors'
        D = int(share.shape[1])
        if any(t.shape[1] != D for t in tables) or not (share.shape[0] == source_only.shape[0] == target_only.shape[0]) or \
                source_other.shape[0] != target_other.shape[0]:
            raise ValueError(f'FusedDeepAPFStep: the five tables must share one width, share and only tables the key id space and the other '
                             f'tables theirs ({tuple(tuple(t.shape) for t in tables)})')
        self.check_widths(D)                                                     # (before anything is allocated)
        shapes = [(D, D), (D,), (1, D), (1, D)]
        if [tuple(p.shape) for p in params] != shapes:
            raise ValueError(f'FusedDeepAPFStep: (W1, b1, w2, wp) must be {shapes}, got {[tuple(p.shape) for p in params]}')
        super().__init__(opt, lr, betas, eps, weight_decay)
        self.D = D
        self.tables = tables
        self.n_overlap = int(n_overlap)
        self.states = self._own_states(tables, states)
        self._dense_init(params)
        dev = share.device
        self.max_source, self.max_target = int(max_source), int(max_target)
        Nm = self.max_source + self.max_target
        self.GS = torch.empty(Nm, D, device=dev, dtype=torch.float32)           # the share table's rows of both domains
        self.GO = tuple(torch.empty(n, D, device=dev, dtype=torch.float32) for n in (self.max_source, self.max_target))
        self.GT = tuple(torch.empty(n, D, device=dev, dtype=torch.float32) for n in (self.max_source, self.max_target))
        self.n_params = D * D + 3 * D
        self.dP = torch.zeros(2, self.n_params, device=dev, dtype=torch.float32)
        self.out16 = torch.zeros(16, device=dev, dtype=torch.float32)           # out8 of the source, out8 of the target
        self.zero = torch.zeros(1, device=dev, dtype=torch.float32)             # the applies' EmbLoss coefficient: none
        self.fws = torch.empty(self._workspace_bytes(max(self.max_source, self.max_target)), device=dev, dtype=torch.uint8)
        # one sort at a time: at most 2 max(B_s, B_t) or B_s + B_t keys
        self.keys, self.perm, self.ws = self._sort_buffers(2 * Nm, self._sort_rows_of(*tables), dev)
        self._key_base = ctypes.c_uint32(0)

    def _states(self):
        return self.states

    def _workspace_bytes(self, B):
        return self._query_bytes('cdr_deepapf_fwd_grad_workspace_bytes', B, self.D)

    def grid(self, B):
        """Workgroups cdr_deepapf_fwd_grad launches for a batch of B rows (the workspace is one packed parameter vector per workgroup)."""
        return self._workspace_bytes(B) // (4 * self.n_params)

    @torch.no_grad()
    def forward_grads(self, ks, os_, ys, kt, ot, yt):
        """Both domains' cdr_deepapf_fwd_grad: fills ``GS`` (rows [0, B_s) source, [B_s, B_s + B_t) target), ``GO``, ``GT``, ``dP`` and
        ``out16``."""
        Bs, Bt = self._check_pair_batch((ks, os_, ys), (kt, ot, yt))
        ctxh, s = B_.ctx(self.tables[0].device), B_.stream()
        packed = torch.cat([q.data.reshape(-1) for q in self.params])
        for d, key, oid, y, n, row0 in ((0, ks, os_, ys, Bs, 0), (1, kt, ot, yt, Bt, Bs)):
            B_.call('cdr_deepapf_fwd_grad', ctxh, s, B_.f32(self.tables[0]), B_.f32(self.tables[1 + 2 * d]), B_.f32(self.tables[2 + 2 * d]),
                    self.D, B_.f32(packed), B_.i64(key), B_.i64(oid), B_.f32(y), n, self.n_overlap, 1.0, row0,
                    B_.f32(self.out16[8 * d:8 * d + 8]), B_.f32(self.GS), B_.f32(self.GO[d]), B_.f32(self.GT[d]), B_.f32(self.dP[d]),
                    B_.raw(self.fws), self.fws.numel())

    def _apply_rows(self, ctxh, st, lo, n, G, base):
        # one gradient row per occurrence (neg_start = n), no EmbLoss (reg_limit = 0)
        self._apply(ctxh, st, self.D, self.keys[lo:lo + n], self.perm[lo:lo + n], n, G[:n], n, 0, self.zero, base)

    @torch.no_grad()
    def step(self, ks, os_, ys, kt, ot, yt):
        """ks / os_ int64 [B_s] (key and other ids of the source rows), ys fp32 [B_s]; kt / ot int64 [B_t], yt fp32 [B_t] (target rows).
        Returns the total loss (device [1]); ``out16`` keeps each domain's {BCE, BCE, 0, ...}."""
        self.forward_grads(ks, os_, ys, kt, ot, yt)                 # both forwards first: both domains see the pre-step state
        Bs, Bt = ks.numel(), kt.numel()
        ctxh, s = B_.ctx(self.tables[0].device), B_.stream()
        B_.call('cdr_sort_ids', ctxh, s, B_.i64(ks), Bs, B_.i64(kt), Bt, self.tables[0].shape[0], B_.raw(self.keys), B_.raw(self.perm),
                B_.raw(self.ws), self.ws.numel())
        self._apply_rows(ctxh, self.states[0], 0, Bs + Bt, self.GS, 0)
        for d, key, oid, n in ((0, ks, os_, Bs), (1, kt, ot, Bt)):
            ost, tst = self.states[1 + 2 * d], self.states[2 + 2 * d]
            B_.call('cdr_sort_ids_two_tables', ctxh, s, B_.i64(key), n, ost.table.shape[0], B_.i64(oid), n, None, 0, tst.table.shape[0],
                    B_.raw(self.keys), B_.raw(self.perm), ctypes.byref(self._key_base), B_.raw(self.ws), self.ws.numel())
            self._apply_rows(ctxh, ost, 0, n, self.GO[d], 0)
            self._apply_rows(ctxh, tst, n, n, self.GT[d], self._key_base.value)
        self._dense_update(self.dP[0] + self.dP[1])                 # the towers are shared by the domains
        return self.out16[0:1] + self.out16[8:9]


class FusedDCDCSRMapStep(_DenseStep):
    """DCDCSR's BOTH-phase step (dcdcsr.py:172-187): ``n`` unit ids drawn with repeats, e = maxmin(table[idx]), m = the tanh MLP of e (tanh
    after every layer, the last included), b = maxmin(bench[idx]) without a gradient, loss = MSE(m, b) as a mean over n D.  One live table
    (the target table of the overlapped unit kind) and the MLP.
    Per step: cdr_dcdcsr_map_fwd_grad (csrc/cdr_dcdcsr.hip: the normalisation, the forward, the backward with the even tie split and every
    parameter gradient in one pass, + its finishing launch) leaves one gradient row per occurrence; cdr_sort_ids(idx) and ONE
    cdr_rowwise_apply(neg_start = n, reg_limit = 0) add the rows of a repeated id in occurrence order and update the table's rows; the
    MLP's parameters take the exact dense Adam (plain SGD with opt='sgd') from ``dparams``, as in FusedDeepAPFStep.
    The update count is the host's: not capturable.

    ``layers``: [(weight [d_l, d_{l-1}], bias [d_l])] -- the parameters themselves: the step sets their ``.grad`` and updates them in
    place.  ``bench`` may be replaced between BOTH visits (the ``bench`` attribute, or ``step(idx, bench=...)``)."""

    MAX_DIM, MAX_LAYERS = 128, 3                                                 # CDR_DCDCSR_MAX_DIM, CDR_DCDCSR_MAX_LAYERS

    @classmethod
    def check_widths(cls, dims):
        dims = list(dims)
        if not (2 <= len(dims) <= cls.MAX_LAYERS + 1):
            raise ValueError(f'FusedDCDCSRMapStep: 1..{cls.MAX_LAYERS} layers, got widths {dims}')
        if not all(isinstance(d, int) and 4 <= d <= cls.MAX_DIM and d % 4 == 0 for d in dims):
            raise ValueError(f'FusedDCDCSRMapStep: every width must be a multiple of 4 in 4..{cls.MAX_DIM} (the activations live in LDS), '
                             f'got {dims}')
        if dims[0] != dims[-1]:
            raise ValueError(f'FusedDCDCSRMapStep: the MLP must map the row width onto itself, got {dims}')

    def __init__(self, table, bench, layers, max_batch, state=None, opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        assert table.is_cuda, 'FusedDCDCSRMapStep needs ROCm device tensors'
        layers = [tuple(l) for l in layers]
        dims = [int(layers[0][0].shape[1])] + [int(W.shape[0]) for W, _ in layers] if layers else []
        self.check_widths(dims)                                                  # (before anything is allocated)
        for l, (W, b) in enumerate(layers):
            if tuple(W.shape) != (dims[l + 1], dims[l]) or b is None or tuple(b.shape) != (dims[l + 1],):
                raise ValueError(f'FusedDCDCSRMapStep: layer {l + 1} must be a [{dims[l + 1]}, {dims[l]}] weight with a bias')
        if table.shape[1] != dims[0]:
            raise ValueError(f'FusedDCDCSRMapStep: the table is {table.shape[1]} wide, the MLP {dims[0]}')
        super().__init__(opt, lr, betas, eps, weight_decay)
        self.table, self.D, self.dims = table, dims[0], dims
        self.bench = bench
        self._dense_init(q for pair in layers for q in pair)
        self.state, = self._own_states((table,), (state,))
        dev = table.device
        self.max_batch = int(max_batch)
        self._dims_c = (ctypes.c_int * len(dims))(*dims)
        self.n_params = sum(q.numel() for q in self.params)
        self.G = torch.empty(self.max_batch, self.D, device=dev, dtype=torch.float32)
        self.dP = torch.zeros(self.n_params, device=dev, dtype=torch.float32)
        self.out8 = torch.zeros(8, device=dev, dtype=torch.float32)
        self.zero = torch.zeros(1, device=dev, dtype=torch.float32)             # the apply's EmbLoss coefficient: none
        self.fws = torch.empty(self._workspace_bytes(self.max_batch), device=dev, dtype=torch.uint8)
        self.keys, self.perm, self.ws = self._sort_buffers(self.max_batch, self._sort_rows_of(table), dev)

    def _states(self):
        return (self.state,)

    def _workspace_bytes(self, n):
        return self._query_bytes('cdr_dcdcsr_map_fwd_grad_workspace_bytes', n, len(self.dims) - 1, self._dims_c)

    def grid(self, n):
        """Workgroups cdr_dcdcsr_map_fwd_grad launches for n ids (the workspace is one packed parameter vector per workgroup)."""
        return self._workspace_bytes(n) // (4 * self.n_params)

    @torch.no_grad()
    def forward_grads(self, idx, bench=None):
        """cdr_dcdcsr_map_fwd_grad alone: fills ``G[:n]``, ``dP`` and ``out8``."""
        bench = self.bench if bench is None else bench
        n = idx.numel()
        if not 1 <= n <= self.max_batch:
            raise ValueError(f'FusedDCDCSRMapStep: {n} ids, sized for 1..{self.max_batch}')
        if bench is None or not bench.is_cuda or bench.dtype != torch.float32 or bench.dim() != 2 or bench.shape[1] != self.D or \
                not bench.is_contiguous():
            raise ValueError(f'FusedDCDCSRMapStep: bench must be a contiguous fp32 device tensor [rows, {self.D}]')
        if idx.dtype != torch.int64 or idx.device != self.table.device or not idx.is_contiguous():
            raise ValueError(f'FusedDCDCSRMapStep: idx must be contiguous int64 on {self.table.device}')
        packed = torch.cat([q.data.reshape(-1) for q in self.params])
        B_.call('cdr_dcdcsr_map_fwd_grad', B_.ctx(self.table.device), B_.stream(), B_.f32(self.table), B_.f32(bench), B_.i64(idx), n,
                len(self.dims) - 1, self._dims_c, B_.f32(packed), B_.f32(self.out8), B_.f32(self.G), B_.f32(self.dP), B_.raw(self.fws),
                self.fws.numel())

    @torch.no_grad()
    def step(self, idx, bench=None):
        """idx: int64 device tensor [n], repeats allowed.  Returns the loss (device scalar)."""
        self.forward_grads(idx, bench)
        n = idx.numel()
        ctxh, s, st = B_.ctx(self.table.device), B_.stream(), self.state
        B_.call('cdr_sort_ids', ctxh, s, B_.i64(idx), n, None, 0, self.table.shape[0], B_.raw(self.keys), B_.raw(self.perm), B_.raw(self.ws),
                self.ws.numel())
        # one gradient row per occurrence (neg_start = n), no EmbLoss (reg_limit = 0)
        self._apply(ctxh, st, self.D, self.keys[:n], self.perm[:n], n, self.G[:n], n, 0, self.zero, 0)
        self._dense_update(self.dP)
        return self.out8[0]


class FusedFrozenSideBPRStep(_Step):
    """DCDCSR's second TARGET visit (dcdcsr.py:98-110, 204-213): BPR without a regulariser in which one operand is a detached table (the
    affine embedding stands in for the overlapped side's table) and only the OTHER side's table trains.  Composed from existing entry
    points: cdr_bpr_fwd_grad(reg_weight = 0) reads both operands; the trained side's ids are sorted -- cdr_sort_ids(pid, nid) with
    G = GP, neg_start = B for items, cdr_sort_ids(uid) with G = GU, neg_start = B for users -- and ONE cdr_rowwise_apply updates its rows.
    Only the trained table's ``RowwiseState`` advances; the frozen operand is read only and has no state.  It may have fewer rows than
    the table it stands in for (the affine table has target_num rows): the batch's ids on that side must be below its row count.
    The frozen side's gradient buffer is written and never read (B D 4 bytes per step; DESIGN.md names a one-sided forward as the next step).

    ``frozen``: 'user' (``user_rows`` is the frozen operand, the item table trains) or 'item'."""

    def __init__(self, user_rows, item_rows, frozen, max_batch, state=None, gamma=1e-10, opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0):
        if frozen not in ('user', 'item'):
            raise ValueError(f"FusedFrozenSideBPRStep: frozen must be 'user' or 'item', got {frozen!r}")
        assert user_rows.is_cuda and item_rows.is_cuda, 'FusedFrozenSideBPRStep needs ROCm device tensors'
        D = int(user_rows.shape[1])
        if item_rows.shape[1] != D or D % 4 != 0 or not 4 <= D <= 256:
            raise ValueError(f'FusedFrozenSideBPRStep: both operands must share a width that is a multiple of 4 in 4..256, got '
                             f'{tuple(user_rows.shape)} and {tuple(item_rows.shape)}')
        super().__init__(opt, lr, betas, eps, weight_decay)
        self.U, self.I, self.D, self.frozen, self.gamma = user_rows, item_rows, D, frozen, gamma
        trained = item_rows if frozen == 'user' else user_rows
        self.state, = self._own_states((trained,), (state,))
        if self.state.table.data_ptr() != trained.data_ptr():
            raise ValueError('FusedFrozenSideBPRStep: state belongs to another table than the trained operand')
        dev = trained.device
        self.max_batch = Bm = int(max_batch)
        self.GU = torch.empty(Bm, D, device=dev, dtype=torch.float32)
        self.GP = torch.empty(Bm, D, device=dev, dtype=torch.float32)
        self.out6 = torch.zeros(12, device=dev, dtype=torch.float32)
        self.zero = torch.zeros(1, device=dev, dtype=torch.float32)
        nk = 2 * Bm if frozen == 'user' else Bm
        self.keys, self.perm, self.ws = self._sort_buffers(nk, self._sort_rows_of(trained), dev)

    def _states(self):
        return (self.state,)

    @torch.no_grad()
    def step(self, uid, pid, nid):
        """uid / pid / nid: int64 device tensors [B].  Returns the device tensor out6 (view; [0] = the loss)."""
        B = uid.numel()
        if not 1 <= B <= self.max_batch or pid.numel() != B or nid.numel() != B:
            raise ValueError(f'FusedFrozenSideBPRStep: {B} / {pid.numel()} / {nid.numel()} ids, sized for 1..{self.max_batch} triples')
        ctxh, s, st = B_.ctx(self.U.device), B_.stream(), self.state
        B_.call('cdr_bpr_fwd_grad', ctxh, s, B_.f32(self.U), B_.f32(self.I), self.D, B_.i64(uid), B_.i64(pid), B_.i64(nid), B, 0,
                float(self.gamma), 0.0, B_.f32(self.out6), B_.f32(self.GU), B_.f32(self.GP), 0)
        if self.frozen == 'user':
            n, G = 2 * B, self.GP
            B_.call('cdr_sort_ids', ctxh, s, B_.i64(pid), B, B_.i64(nid), B, st.table.shape[0], B_.raw(self.keys), B_.raw(self.perm),
                    B_.raw(self.ws), self.ws.numel())
        else:
            n, G = B, self.GU
            B_.call('cdr_sort_ids', ctxh, s, B_.i64(uid), B, None, 0, st.table.shape[0], B_.raw(self.keys), B_.raw(self.perm), B_.raw(self.ws),
                    self.ws.numel())
        # occurrences [B, 2 B) of the item list are the negatives: -GP[o - B]; no EmbLoss (reg_limit = 0)
        self._apply(ctxh, st, self.D, self.keys[:n], self.perm[:n], n, G, B, 0, self.zero, 0)
        return self.out6


class SSCDRMapStep(_DenseStep):
    """SSCDR's OVERLAP phase (sscdr.py:161-187: MSE(mapping(source_a[idx]), target_a[idx]) + lambda x triplet(normalize(target_a[idx]),
    normalize(mapping(source_b[pos])), normalize(mapping(source_b[neg])))) as an O(batch) step: the three touched tables are updated
    row-wise -- source_a and target_a on ``idx`` (one sort serves both), source_b on ``pos ++ neg`` -- and the mapping's own parameters
    keep the exact dense Adam (plain SGD with opt='sgd'), as in FusedMapStep.  Repeated ids in any list are summed by the segmented
    applies.  The reference's overlap batch is 100 ids: the step is launch-bound and stays composed on the host (gather, the mapping
    and the loss node through autograd on the gathered rows, sort, applies)."""

    def __init__(self, source_a, target_a, source_b, mapping_fn, mapping_params, margin, lamda, opt='adam', lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, weight_decay=0.0, source_a_state=None, target_a_state=None, source_b_state=None):
        assert source_a.is_cuda and target_a.is_cuda and source_b.is_cuda, 'SSCDRMapStep needs ROCm device tensors'
        assert source_a.shape[1] == target_a.shape[1] == source_b.shape[1]
        super().__init__(opt, lr, betas, eps, weight_decay)
        self.SA, self.TA, self.SB = source_a, target_a, source_b
        self.D = source_a.shape[1]
        self.mapping_fn = mapping_fn
        self.margin, self.lamda = float(margin), float(lamda)
        self.sa_state, self.ta_state, self.sb_state = self._own_states((source_a, target_a, source_b),
                                                                       (source_a_state, target_a_state, source_b_state))
        self._dense_init(mapping_params)
        self.mapping_params = self.params
        self.loss = torch.zeros((), device=source_a.device, dtype=torch.float32)
        self._ws = None

    def _states(self):
        return self.sa_state, self.ta_state, self.sb_state

    @property
    def map_opt(self):
        """The mapping's dense Adam under the name FusedMapStep uses (one object: assigning either name replaces it)."""
        return self.w_opt

    @map_opt.setter
    def map_opt(self, opt):
        self.w_opt = opt

    def step(self, idx, pos, neg, bump=None):
        """idx / pos / neg: int64 device tensors of n ids each (any shape).  ``bump``: optional device int64 [1] advanced once (the
        device sampler's call counter, which the dense path advances in its gather launch).  Returns the loss (device scalar)."""
        from . import functional as F_
        idx, pos, neg = (x.reshape(-1).contiguous() for x in (idx, pos, neg))
        n, D = idx.numel(), self.D
        if pos.numel() != n or neg.numel() != n:
            raise ValueError(f'SSCDRMapStep: {n} / {pos.numel()} / {neg.numel()} ids')
        dev = self.SA.device
        if n == 0:                                     # an empty batch is a no-op: no state advances
            self.loss = torch.zeros((), device=dev, dtype=torch.float32)
            return self.loss
        s = B_.stream()
        for p in self.mapping_params:
            p.grad = None
        X3 = torch.empty(3 * n, D, device=dev, dtype=torch.float32)
        Tt = torch.empty(n, D, device=dev, dtype=torch.float32)
        P4, I4 = ctypes.c_void_p * 4, ctypes.c_int64 * 4
        keep = [idx, pos, neg, X3, Tt]
        B_.call('cdr_gather_rows_multi', s, 4, P4(self.SA.data_ptr(), self.SB.data_ptr(), self.SB.data_ptr(), self.TA.data_ptr()), D,
                P4(idx.data_ptr(), pos.data_ptr(), neg.data_ptr(), idx.data_ptr()), I4(n, n, n, n),
                P4(X3.data_ptr(), X3.data_ptr() + 4 * n * D, X3.data_ptr() + 8 * n * D, Tt.data_ptr()), None if bump is None else B_.i64(bump))
        del keep
        X3.requires_grad_(True); Tt.requires_grad_(True)
        total, _ = F_.SSCDRMapLoss.apply(self.mapping_fn(X3), Tt, self.margin, self.lamda)
        total.backward()
        self.loss = total.detach()
        for st in self._states():
            st.advance()
        ctxh = B_.ctx(dev)
        rows = max(self.SA.shape[0], self.TA.shape[0], self.SB.shape[0])
        need = max(self._query_bytes('cdr_sort_workspace_bytes', m, rows) for m in (n, 2 * n))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, device=dev, dtype=torch.uint8)
        keys = torch.empty(3 * n, device=dev, dtype=torch.int32)
        perm = torch.empty(3 * n, device=dev, dtype=torch.int32)
        # the same ids index source_a and target_a: one sort serves both applies; source_b's list is pos ++ neg, the order of X3[n:]
        B_.call('cdr_sort_ids', ctxh, s, B_.i64(idx), n, None, 0, self.SA.shape[0], B_.raw(keys[:n]), B_.raw(perm[:n]), B_.raw(self._ws),
                self._ws.numel())
        B_.call('cdr_sort_ids', ctxh, s, B_.i64(pos), n, B_.i64(neg), n, self.SB.shape[0], B_.raw(keys[n:]), B_.raw(perm[n:]),
                B_.raw(self._ws), self._ws.numel())
        gX, gT = X3.grad.contiguous(), Tt.grad.contiguous()
        for st, k, pm, m, G in ((self.sa_state, keys[:n], perm[:n], n, gX[:n]), (self.ta_state, keys[:n], perm[:n], n, gT),
                                (self.sb_state, keys[n:], perm[n:], 2 * n, gX[n:])):
            self._apply(ctxh, st, D, k, pm, m, G, m, 0, None, 0, advance=False)
        self._dense_update()
        return self.loss


class FusedPointPairStep(_TwoTableStep):
    """CMF's BOTH-phase step (cmf.py:75-99): a source and a target pointwise batch on ONE user and ONE item table,
    loss = alpha (BCE_s + reg_source EmbLoss_s) + (1 - alpha) (BCE_t + reg_target EmbLoss_t), and ONE update per touched row from the
    sum of its two domains' contributions -- the reference's single Adam step (two FusedPointStep calls would update a row named by both
    batches twice and advance each table twice).  One native call (cdr_point_step_fused_pair_dev) with the update counts on the device:
    capturable in a hipGraph (``replayed`` keeps the host mirrors in step).  opt='adagrad': the same launches through
    cdr_point_step_fused_pair, which reads no update count (host counts; not captured)."""

    def __init__(self, user_table, item_table, max_source, max_target, alpha, reg_source, reg_target, opt='adam', lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, user_state=None, item_state=None, loss='bce'):
        if user_table.shape[1] % 4 != 0 or user_table.shape[1] > 256:            # (before the base allocates any optimizer state)
            raise ValueError(f'FusedPointPairStep: D must be a multiple of 4 and <= 256, got {user_table.shape[1]}')
        super().__init__(user_table, item_table, opt, lr, betas, eps, weight_decay, user_state, item_state)
        self.kind = B_.CDR_LOSS_MSE if loss == 'mse' else B_.CDR_LOSS_BCE
        self.alpha, self.reg_source, self.reg_target = float(alpha), float(reg_source), float(reg_target)
        dev = user_table.device
        self.max_source, self.max_target = int(max_source), int(max_target)
        Nm = self.max_source + self.max_target
        self.GU = torch.empty(Nm, self.D, device=dev, dtype=torch.float32)
        self.GI = torch.empty(Nm, self.D, device=dev, dtype=torch.float32)
        self.out16 = torch.zeros(16, device=dev, dtype=torch.float32)
        self.keys = torch.empty(2 * Nm, device=dev, dtype=torch.int32)       # one sort: user keys [su | tu], item keys [si | ti]
        self.perm = torch.empty(2 * Nm, device=dev, dtype=torch.int32)
        self.flags, self.heads = self._single_row_buffers(Nm)                # flags: {user, item, -, -} per joint row
        # (the sort switches configuration at 2^18 keys: a short tail batch may need more scratch than a full one)
        self.ws, _ = self._sort_workspace(2 * Nm, min(2 * Nm, (1 << 18) - 1))
        self._hp_dev = torch.zeros(4, device=dev, dtype=torch.float32)

    def step(self, su, si, ys, tu, ti, yt):
        """su / si int64 [B_s], ys fp32 [B_s] (source rows); tu / ti int64 [B_t], yt fp32 [B_t] (target rows).  Returns out16 (view):
        [0] total, [1] BCE_s, [2] BCE_t, [3] EmbLoss_s, [4] EmbLoss_t (unweighted parts), [5:9] the four batch norms."""
        Bs, Bt = su.numel(), tu.numel()
        if not (1 <= Bs <= self.max_source and 1 <= Bt <= self.max_target):
            raise ValueError(f'FusedPointPairStep: batches of {Bs} + {Bt} rows, sized for 1..{self.max_source} + 1..{self.max_target}')
        if si.numel() != Bs or ys.numel() != Bs or ti.numel() != Bt or yt.numel() != Bt:
            raise ValueError('FusedPointPairStep: ids and labels of a domain must have the same length')
        us, its = self.ustate, self.istate
        if self.opt == OPT_ADAGRAD:
            # the host-state entry: Adagrad reads no update count (the host counts still advance: checkpoints, one state per table)
            lr, _b1, _b2, eps, wd = self._hp()
            us.advance(); its.advance()
            B_.call('cdr_point_step_fused_pair', B_.ctx(self.U.device), B_.stream(), self.kind, self.opt, B_.f32(us.table), None,
                    B_.f32(us.exp_avg_sq), us.table.shape[0], B_.f32(its.table), None, B_.f32(its.exp_avg_sq), its.table.shape[0],
                    self.D, B_.i64(su), B_.i64(si), B_.f32(ys), Bs, B_.i64(tu), B_.i64(ti), B_.f32(yt), Bt, self.alpha, self.reg_source,
                    self.reg_target, lr, eps, wd, B_.f32(self.out16), B_.f32(self.GU), B_.f32(self.GI), B_.raw(self.keys), B_.raw(self.perm),
                    B_.raw(self.flags), B_.raw(self.heads), B_.raw(self.ws), self.ws.numel())
            return self.out16
        adam = self.opt == OPT_ADAM
        B_.call('cdr_point_step_fused_pair_dev', B_.ctx(self.U.device), B_.stream(), self.kind, self.opt, B_.f32(us.table), B_.f32(us.exp_avg),
                B_.f32(us.exp_avg_sq), us.table.shape[0], B_.f32(its.table), B_.f32(its.exp_avg), B_.f32(its.exp_avg_sq), its.table.shape[0],
                self.D, B_.i64(su), B_.i64(si), B_.f32(ys), Bs, B_.i64(tu), B_.i64(ti), B_.f32(yt), Bt, self.alpha, self.reg_source,
                self.reg_target, *self._hp(), B_.i64(us.step_dev), B_.i64(its.step_dev), B_.f32(self._hp_dev) if adam else None,
                B_.f32(self.out16), B_.f32(self.GU), B_.f32(self.GI), B_.raw(self.keys), B_.raw(self.perm), B_.raw(self.flags), B_.raw(self.heads), B_.raw(self.ws), self.ws.numel())
        if not torch.cuda.is_current_stream_capturing():       # (a capture enqueues nothing: the host counts advance per replay)
            us.advance(device_bumped=True)
            its.advance(device_bumped=True)
        return self.out16


class KMajorPointStep(_TwoTableStep):
    """``FusedPointStep`` cut along recbole's pointwise batch layout: S positives, the user column tiled 1 + k times, items =
    [positives | k-major negatives], labels [1] * S + [0] * S k (TrainDataLoader._neg_sampling).  One lane group per POSITIVE gathers
    the user row once and sums its gradient over the 1 + k rows in registers; users that occur in one positive and item rows that occur
    once are updated by that kernel, the rest by the segmented applies (csrc/cdr_step.hip: point_fwd_apply_kmajor_kernel).  Same loss
    and per-row gradients as ``FusedPointStep`` on the S (1 + k) rows."""

    def __init__(self, user_table, item_table, max_positives, k=1, loss='mse', opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, reg_weight=0.0, user_state=None, item_state=None):
        assert user_table.shape[1] % 4 == 0 and user_table.shape[1] <= 256 and 1 <= int(k) <= 64
        refuse_adagrad('KMajorPointStep', opt_code(opt))
        super().__init__(user_table, item_table, opt, lr, betas, eps, weight_decay, user_state, item_state)
        self.k = int(k)
        self.kind = B_.CDR_LOSS_MSE if loss == 'mse' else B_.CDR_LOSS_BCE
        self.reg_weight = reg_weight
        dev = user_table.device
        Sm = int(max_positives)
        nI = Sm * (1 + self.k)
        self.max_positives = Sm
        self.max_batch = nI
        self.GU = torch.empty(Sm, self.D, device=dev, dtype=torch.float32)
        self.GI = torch.empty(nI, self.D, device=dev, dtype=torch.float32)
        fb, hw = ctypes.c_int64(0), ctypes.c_int64(0)
        B_._check(B_.load().cdr_bpr_step_fused_kmajor_sizes(Sm, self.k, ctypes.byref(fb), ctypes.byref(hw)), 'cdr_bpr_step_fused_kmajor_sizes')
        self.flags = torch.zeros(int(fb.value), device=dev, dtype=torch.uint8)
        self.heads = torch.empty(int(hw.value), device=dev, dtype=torch.int32)
        self.out6 = torch.zeros(12, device=dev, dtype=torch.float32)
        self.keys = torch.empty(Sm + nI, device=dev, dtype=torch.int32)
        self.perm = torch.empty(Sm + nI, device=dev, dtype=torch.int32)
        self.ws, _ = self._sort_workspace(Sm + nI)

    def step(self, uid, iid, label):
        """uid int64 [S (1 + k)] tiled (or [S]: the first S entries are read), iid int64 [S (1 + k)], label fp32 [S (1 + k)].
        Returns out6 (view; [0] = total loss)."""
        n = iid.numel()
        S = n // (1 + self.k)
        assert S * (1 + self.k) == n and S <= self.max_positives and uid.numel() >= S and label.numel() == n
        us, its = self.ustate, self.istate
        us.advance(); its.advance()
        B_.call('cdr_point_step_fused_kmajor', B_.ctx(self.U.device), B_.stream(), self.kind, self.opt, B_.f32(us.table), B_.f32(us.exp_avg),
                B_.f32(us.exp_avg_sq), us.table.shape[0], B_.f32(its.table), B_.f32(its.exp_avg), B_.f32(its.exp_avg_sq), its.table.shape[0],
                self.D, B_.i64(uid), B_.i64(iid), B_.f32(label), S, self.k, float(self.reg_weight), *self._hp(), us.step, its.step, B_.f32(self.out6),
                B_.f32(self.GU), B_.f32(self.GI), B_.raw(self.keys), B_.raw(self.perm), B_.raw(self.flags), B_.raw(self.heads), B_.raw(self.ws),
                self.ws.numel())
        return self.out6


class FusedMapStep(_Step):
    """EMCDR's OVERLAP phase (emcdr.py:133-137 ``calculate_map_loss``: MSE(mapping(source_e[idx]), target_e[idx])) as an
    O(batch) step: the two embedding tables are updated row-wise on the overlapped ids only; the mapping function's own
    parameters (a few hundred KB) keep the exact dense Adam.

    ``mapping_fn``  x [n, Ds] -> [n, Dt] built from functional.linear (autograd through the native GEMM kernels), e.g. a
                    model's ``apply_mapping``;  ``mapping_params`` its parameters.
    ``group``       optional process group: the tables are then this rank's row shards (row r % G == rank at r // G) and
                    ``step`` takes GLOBAL ids.  Both tables use the same sharding rule and an overlapped id names the same
                    entity in both, so after ONE all-to-all of ids everything is local: the "overlapped-user transfer
                    step" moves 8 B per id, never a row.  The MSE mean is over the global batch; the mapping gradients
                    are all-reduced (every rank then takes the same dense Adam step on its replica).
    """

    def __init__(self, source_table, target_table, mapping_fn, mapping_params, max_batch, opt='adam', lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, group=None, source_state=None, target_state=None, layers=None):
        assert source_table.is_cuda and target_table.is_cuda, 'FusedMapStep needs ROCm device tensors'
        self.S, self.T = source_table, target_table
        self.mapping_fn = mapping_fn
        self.mapping_params = list(mapping_params)
        super().__init__(opt, lr, betas, eps, weight_decay)
        # the row-wise moments may be shared with the FusedBPRStep objects of the SOURCE / TARGET phases (one optimizer
        # state per table across phases, like the reference's single Adam instance: trainer.py:30-41)
        self.sstate = source_state if source_state is not None else RowwiseState(source_table, self.opt)
        self.tstate = target_state if target_state is not None else RowwiseState(target_table, self.opt)
        self.map_opt = self._dense_optimizer(self.mapping_params)                    # the dense optimizer of the same learner
        self.group = group
        self.loss = torch.zeros((), device=source_table.device, dtype=torch.float32)
        self._ws = None
        # ``layers``: the mapping function's structure [(weight [out, in], bias or None, ACT_NONE | ACT_TANH), ...] (emcdr.py:59-64,
        # 86-93).  With it, batches of DISTINCT ids -- what the reference's OverlapDataloader yields -- run as two native launches
        # (csrc/cdr_mapstep.hip): ``step(idx, unique=True)``.
        self.layers = None
        self._uws = None
        if layers is not None and group is None:
            dims = [layers[0][0].shape[1]] + [w.shape[0] for w, _, _ in layers]
            need = ctypes.c_size_t(0)
            L = len(layers)
            if L <= 4 and B_.load().cdr_map_step_plan(L, (ctypes.c_int * (L + 1))(*dims), (ctypes.c_int * L)(*[int(b is not None) for _, b, _ in layers]),
                                                       max(int(max_batch), 1), ctypes.byref(need)) == 0:
                self.layers, self._dims = list(layers), dims
                self._loss1 = torch.zeros(1, device=source_table.device, dtype=torch.float32)

    def _states(self):
        return self.sstate, self.tstate

    def _step_unique(self, idx):
        """Two launches: gather + mapping + MSE + backward + in-place row updates + gradient partials, then reduction + dense Adam on
        the mapping.  Update counts are device counters (capturable)."""
        n = idx.numel()
        dev = self.S.device
        L = len(self.layers)
        need = ctypes.c_size_t(0)
        dims_c = (ctypes.c_int * (L + 1))(*self._dims)
        B_._check(B_.load().cdr_map_step_plan(L, dims_c, (ctypes.c_int * L)(*[int(b is not None) for _, b, _ in self.layers]), n,
                                              ctypes.byref(need)), 'cdr_map_step_plan')
        if self._uws is None or self._uws.numel() < need.value:
            self._uws = torch.empty(int(need.value), device=dev, dtype=torch.uint8)
        adam = self.opt == OPT_ADAM
        ptrs = lambda xs: (ctypes.c_void_p * L)(*[None if x is None else x.data_ptr() for x in xs])
        Ws = [w.data for w, _, _ in self.layers]
        bs = [None if b is None else b.data for _, b, _ in self.layers]
        mW = vW = mb = vb = sW = sb = [None] * L
        if adam:
            def st(p):
                d = self.map_opt.state[p]
                if not d:
                    d['step'] = torch.zeros(1, device=dev, dtype=torch.int64)
                    d['exp_avg'] = torch.zeros_like(p); d['exp_avg_sq'] = torch.zeros_like(p)
                return d
            sts = [st(w) for w, _, _ in self.layers]
            stb = [None if b is None else st(b) for _, b, _ in self.layers]
            mW, vW, sW = [d['exp_avg'] for d in sts], [d['exp_avg_sq'] for d in sts], [d['step'] for d in sts]
            mb = [None if d is None else d['exp_avg'] for d in stb]; vb = [None if d is None else d['exp_avg_sq'] for d in stb]
            sb = [None if d is None else d['step'] for d in stb]
        keep = [Ws, bs, mW, vW, mb, vb, sW, sb]                         # alive until the call is enqueued
        ss, ts_ = (self.sstate.step_dev, self.tstate.step_dev) if adam else (None, None)
        B_.call('cdr_map_step_unique', B_.ctx(dev), B_.stream(), self.opt, B_.f32(self.S), B_.f32(self.sstate.exp_avg),
                B_.f32(self.sstate.exp_avg_sq), B_.f32(self.T), B_.f32(self.tstate.exp_avg), B_.f32(self.tstate.exp_avg_sq), B_.i64(idx), n,
                L, dims_c, (ctypes.c_int * L)(*[int(a) for _, _, a in self.layers]), ptrs(Ws), ptrs(bs), ptrs(mW), ptrs(vW), ptrs(mb),
                ptrs(vb), ptrs(sW), ptrs(sb), B_.i64(ss), B_.i64(ts_), *self._hp(), B_.f32(self._loss1), B_.raw(self._uws),
                self._uws.numel())
        del keep
        if not torch.cuda.is_current_stream_capturing():       # (a capture enqueues nothing: the host counts advance per replay)
            self.sstate.advance(device_bumped=True)
            self.tstate.advance(device_bumped=True)
        self.loss = self._loss1[0]
        return self.loss

    # ---- hipGraph replay of the two-launch step (the reference's default overlap_batch_size is 100: launch-bound) ----------------
    def capture(self, OB):
        """Capture the distinct-id step for batches of exactly OB ids.  ``replay(idx)`` then costs one id copy + one graph launch;
        every update count the kernels read lives on the device."""
        assert self.layers is not None and self.group is None
        dev = self.S.device
        self._OB = OB
        self._idx = torch.arange(1, OB + 1, device=dev, dtype=torch.int64)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            B_.ctx(dev)                                   # the native context of the capture stream must exist beforehand
            if self.opt == OPT_ADAM:
                self.sstate.step_dev, self.tstate.step_dev
                for w, b, _ in self.layers:                # the mapping's Adam state and the workspace: created outside the capture
                    for prm in (w, b):
                        if prm is not None and not self.map_opt.state[prm]:
                            d = self.map_opt.state[prm]
                            d['step'] = torch.zeros(1, device=dev, dtype=torch.int64)
                            d['exp_avg'] = torch.zeros_like(prm); d['exp_avg_sq'] = torch.zeros_like(prm)
            need = ctypes.c_size_t(0)
            L = len(self.layers)
            B_._check(B_.load().cdr_map_step_plan(L, (ctypes.c_int * (L + 1))(*self._dims),
                                                  (ctypes.c_int * L)(*[int(b is not None) for _, b, _ in self.layers]), OB,
                                                  ctypes.byref(need)), 'cdr_map_step_plan')
            if self._uws is None or self._uws.numel() < need.value:
                self._uws = torch.empty(int(need.value), device=dev, dtype=torch.uint8)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        host = (self.sstate._step, self.tstate._step)
        self._graph = torch.cuda.CUDAGraph()
        with B_.capturing(self._graph, side):
            self._step_unique(self._idx)
        self.sstate._step, self.tstate._step = host       # the capture enqueued nothing: host counts advance per replay
        return self

    def replay(self, idx=None):
        if idx is not None:
            self._idx.copy_(idx.reshape(-1)[:self._OB])
        self._graph.replay()
        self.replayed()
        self.loss = self._loss1[0]
        return self.loss

    def _route(self, idx):
        """Global ids -> the local row indices this rank owns (one all-to-all of ids), plus the global batch size."""
        import torch.distributed as dist
        from .shard import NativeOps, _a2a, _gather_counts
        G, rank = dist.get_world_size(self.group), dist.get_rank(self.group)
        ops = NativeOps(idx.device) if not hasattr(self, '_ops') else self._ops
        self._ops = ops
        perm, counts = ops.route(idx, None, G)
        send = ops.permute(idx, None, perm, G)
        allc = torch.stack(_gather_counts(counts, idx.numel(), self.group, G)).tolist()          # one host sync
        t_send = [int(c) for c in allc[rank][:G]]
        t_recv = [int(allc[r][rank]) for r in range(G)]
        n_global = sum(int(allc[r][G]) for r in range(G))
        if n_global == 0:                          # nothing anywhere: no zero-byte all-to-all either
            return send, 0
        return _a2a(send, t_send, t_recv, self.group), n_global

    def step(self, idx, unique=False):
        """idx: int64 device tensor of overlapped ids, any shape ([OB,1] from the OverlapDataloader).  Returns the loss
        (device scalar; the global-batch MSE when sharded).  ``unique=True`` asserts that the ids are pairwise distinct (slices of
        a permutation, as the reference's loader yields them): the two-launch path of csrc/cdr_mapstep.hip."""
        idx = idx.reshape(-1).contiguous()
        n_global = idx.numel()
        if unique and self.layers is not None and n_global > 0 and self.opt != OPT_ADAGRAD:     # (Adagrad: the general form below)
            return self._step_unique(idx)
        if self.group is not None:
            idx, n_global = self._route(idx)
        if n_global == 0:                          # an empty batch (on every rank) is a no-op: no state advances
            self.loss = torch.zeros((), device=self.S.device, dtype=torch.float32)
            return self.loss
        n = idx.numel()
        D_s, D_t = self.S.shape[1], self.T.shape[1]
        dev = self.S.device
        s = B_.stream()
        for p in self.mapping_params:
            p.grad = None
        if n:
            src = torch.empty(n, D_s, device=dev, dtype=torch.float32)
            tgt = torch.empty(n, D_t, device=dev, dtype=torch.float32)
            B_.call('cdr_gather_rows', s, B_.f32(self.S), D_s, B_.i64(idx), n, B_.f32(src))
            B_.call('cdr_gather_rows', s, B_.f32(self.T), D_t, B_.i64(idx), n, B_.f32(tgt))
            src.requires_grad_(True); tgt.requires_grad_(True)
            from . import functional as F_
            local = F_.mse_loss(self.mapping_fn(src), tgt)              # mean over n * Dt
            loss = local * (float(n) / float(n_global))                  # this rank's share of the global mean
            loss.backward()
            loss = loss.detach()
        else:
            loss = torch.zeros((), device=dev, dtype=torch.float32)
        if self.group is not None:
            import torch.distributed as dist
            flat = torch.cat([loss.reshape(1)] + [(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                                                  for p in self.mapping_params])
            dist.all_reduce(flat, group=self.group)
            loss, off = flat[0], 1
            for p in self.mapping_params:
                p.grad = flat[off:off + p.numel()].view_as(p).clone()
                off += p.numel()
        self.loss = loss
        self.sstate.advance()                  # per TABLE, also on a rank that received no ids (the shards stay in step)
        self.tstate.advance()
        if n:
            ctxh = B_.ctx(dev)
            need = self._query_bytes('cdr_sort_workspace_bytes', n, self.S.shape[0])
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, device=dev, dtype=torch.uint8)
            keys = torch.empty(n, device=dev, dtype=torch.int32)
            perm = torch.empty(n, device=dev, dtype=torch.int32)
            # the same ids index both tables: one sort serves both applies
            B_.call('cdr_sort_ids', ctxh, s, B_.i64(idx), n, None, 0, self.S.shape[0], B_.raw(keys), B_.raw(perm),
                    B_.raw(self._ws), self._ws.numel())
            for st, g in ((self.sstate, src.grad), (self.tstate, tgt.grad)):
                self._apply(ctxh, st, st.table.shape[1], keys, perm, n, g, n, 0, None, 0, advance=False)
        if self.map_opt is not None:
            self.map_opt.step()
        else:
            with torch.no_grad():
                for p in self.mapping_params:
                    if p.grad is not None:
                        p.add_(p.grad + self.wd * p if self.wd else p.grad, alpha=-self.lr)
        return self.loss
