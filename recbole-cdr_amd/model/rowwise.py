"""Model-side bookkeeping of the O(batch) row-wise training path (``optimizer_mode='rowwise'``), shared by every model with a
``fused_train_step``: the cache of per-table optimizer states and step objects, the checks of the (opt, adam) arguments, and the
methods the trainer calls around the step (``fused_replayed``, ``fused_sync``, ``fused_optimizer_state``,
``load_fused_optimizer_state``).  Which step class a batch gets stays with the model."""
from ..fused import FusedBPRStep, KMajorBPRStep, RowwiseState, OPT_ADAGRAD, OPT_NAMES, opt_code, rowwise_bound_lag, rowwise_catch_up


class RowwiseTraining:
    """Mixin next to ``CrossDomainRecommender``.  State: ``self._fused = {'states': {table name: RowwiseState}, 'steps': {key: step
    object}}``, created by the first accepted ``fused_train_step``.  The model supplies ``_fused_phase_step()``: the step object
    the current phase's captured ``fused_train_step`` runs.  A model whose step also owns dense weights (CLFM, DTCDR, DeepAPF, DCDCSR)
    names that step's key in ``_WEIGHT_STEP``: the weights' dense Adam state then travels with the step cache and the checkpoint."""

    _WEIGHT_STEP = None

    @staticmethod
    def _fused_args(opt, adam, lr, betas, eps, weight_decay):
        """Checks ``fused_train_step``'s (opt, adam) -> (exact, optimizer code, the step classes' optimizer keywords).  Touches nothing:
        the model's own rejections come between this and ``_fused_cache``, so that a rejected call leaves no state behind."""
        if adam not in ('lazy', 'exact'):
            raise ValueError(f"adam must be 'lazy' or 'exact', got {adam!r}")
        exact = adam == 'exact'
        if exact and opt != 'adam':
            raise ValueError(f"adam='exact' is the reference's dense Adam: it needs opt='adam', got {opt!r}")
        return exact, opt_code(opt), dict(opt=opt, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)      # (an unknown opt: ValueError)

    def _fused_cache(self, exact=None):
        """The cache, created on first use.  ``exact`` given: the mode of this ``fused_train_step`` -- one per model."""
        cache = self.__dict__.setdefault('_fused', {'states': {}, 'steps': {}})
        if exact is not None:
            for name, st in cache['states'].items():
                if st.exact != exact:
                    raise ValueError(f"{name} was trained with adam={'exact' if st.exact else 'lazy'!r}; one row-wise Adam mode per model")
        return cache

    def _fused_state(self, name, code, exact):
        """The ``RowwiseState`` of the embedding table ``self.<name>``, created on first use."""
        states = self._fused['states']
        if name not in states:
            states[name] = RowwiseState(getattr(self, name).weight.data, code, exact=exact)
        return states[name]

    def _fused_step(self, key, fits, build):
        """The step object cached under ``key`` if ``fits(step)`` still holds, else ``build()``'s, which replaces it."""
        steps = self._fused['steps']
        step = steps.get(key)
        if step is None or not fits(step):
            step = steps[key] = build()
        return step

    def _fused_weight_step(self, key, fits, make, hp):
        """The step object with dense weights cached under ``key`` if ``fits(step)`` holds and the optimizer settings are ``hp``, else
        ``make()``'s.  The weights' Adam state outlives a re-sized step object, and a checkpoint's (``_pending_weight_state``) is handed
        over when the first one is built."""
        old = self._fused['steps'].get(key)

        def build():
            step = make()
            carry = old.w_opt.state_dict() if old is not None and old.w_opt is not None else self.__dict__.pop('_pending_weight_state', None)
            if carry is not None and step.w_opt is not None:
                step.w_opt.load_state_dict(carry)
                for g in step.w_opt.param_groups:
                    g.update(lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], weight_decay=hp['weight_decay'])
            return step

        step = self._fused_step(key, lambda s: fits(s) and s.hp == hp, build)
        step.hp = hp
        return step

    def _fused_pair_sizes(self, key, Bs, Bt):
        """(max_source, max_target) for a two-domain step under ``key``: a rebuilt step never shrinks."""
        old = self._fused['steps'].get(key)
        return (Bs, Bt) if old is None else (max(Bs, old.max_source), max(Bt, old.max_target))

    def _fused_refuse_dist(self, model):
        if self.__dict__.get('_dist_cfg') not in (None, False):
            raise NotImplementedError(f"{model}.fused_train_step does not shard its tables: config['dist_group'] is not supported (one GPU)")

    @staticmethod
    def _fused_check_widths(model, check, described, *widths):
        """``check(*widths)`` (a step class's ``check_widths``), its refusal re-raised in the model's words: ``described`` is a format
        of the widths (formatted only on refusal: this runs in front of every step)."""
        try:
            check(*widths)
        except ValueError as e:
            raise ValueError(f'{model}.fused_train_step: {described.format(*widths)}: {e}; use optimizer_mode=dense') from None

    def _fused_check_pair_batch(self, model, su, si, ys, tu, ti, yt):
        """(B_s, B_t) of a BOTH-phase batch: at least one row per domain, ids and labels of equal length."""
        Bs, Bt = su.numel(), tu.numel()
        if Bs == 0 or Bt == 0 or si.numel() != Bs or ys.numel() != Bs or ti.numel() != Bt or yt.numel() != Bt:
            raise ValueError(f'{model}.fused_train_step: the {self.phase} batch needs at least one row per domain and ids and labels of equal '
                             f'length, got {Bs} / {si.numel()} / {ys.numel()} source and {Bt} / {ti.numel()} / {yt.numel()} target entries')
        return Bs, Bt

    def _fused_domain_step(self, domain, key, cls, size, sized_by, code, exact, hp, **kw):
        """This domain's ``cls`` object on (``<domain>_user_embedding``, ``<domain>_item_embedding``) for ``size`` rows or positives,
        rebuilt when its ``sized_by`` attribute says it is too small.  The tables' states are the model's shared ones."""
        return self._fused_step(key, lambda s: getattr(s, sized_by) >= size, lambda: cls(
            getattr(self, f'{domain}_user_embedding').weight.data, getattr(self, f'{domain}_item_embedding').weight.data, size,
            user_state=self._fused_state(f'{domain}_user_embedding', code, exact),
            item_state=self._fused_state(f'{domain}_item_embedding', code, exact), **kw, **hp))

    def _fused_bpr_domain_step(self, domain, k_major, user, item, neg, reg_weight, gamma, code, exact, hp):
        """One BPR step on a domain's two tables, in the form the batch layout calls for (EMCDR's BPR branch, DCDCSR's first SOURCE /
        TARGET visit).  recbole's pairwise batches tile S positives k times with k-major negatives (crossdomain_sampler.py:148-152); the
        loader says so (``Interaction.k_major``).  Then the per-positive step serves k >= 2 (u, p gathered once per positive) and every
        batch small enough for its four-launch form (the reference default of 2,048 rows); k = 1 at large batches stays on the
        per-triple step, which is faster there.  In exact mode the catch-up runs in front on (user, [uid]) and
        (item, [pid, nid]).  Returns the loss (device [1] view)."""
        def catch_up(*tables):
            if exact:
                rowwise_catch_up(tables, lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], weight_decay=hp['weight_decay'])

        k, rows = k_major, user.numel()
        # (Adagrad: the per-positive kernels implement SGD and Adam only; the per-triple step below has the same loss and per-row
        # gradients on the B = S k rows -- KMajorBPRStep's docstring)
        if code != OPT_ADAGRAD and k is not None and rows % k == 0 and (k >= 2 or rows + rows // k <= 8192):
            step = self._fused_domain_step(domain, ('bprk', domain, k), KMajorBPRStep, rows // k, 'max_positives', code, exact, hp,
                                           reg_weight=reg_weight, k=k, gamma=gamma)
            catch_up((step.ustate, [user[:rows // k]]), (step.istate, [item[:rows // k], neg]))
            return step.step(user, item, neg)[0]
        step = self._fused_domain_step(domain, ('bpr', domain), FusedBPRStep, rows, 'max_batch', code, exact, hp, reg_weight=reg_weight,
                                       gamma=gamma)
        catch_up((step.ustate, [user]), (step.istate, [item, neg]))
        return step.step(user, item, neg)[0]

    def fused_replayed(self, n=1):
        """Host bookkeeping of ``n`` hipGraph replays of the current phase's ``fused_train_step`` (the update counts' host mirrors)."""
        step = self._fused_phase_step()
        step.replayed(n)
        for st in step._states():
            rowwise_bound_lag(st)                               # (exact mode without the moving window only)

    def fused_sync(self):
        """``fused_train_step(adam='exact')``: bring every row of every table to its update count -- the tables and moments then equal
        the reference's dense Adam (before evaluation, checkpoints, the end of training).  Lazy mode: nothing to do."""
        cache = self.__dict__.get('_fused')
        if cache:
            for st in cache['states'].values():
                if st.exact:
                    st.flush()

    def fused_optimizer_state(self):
        """Row-wise optimizer state of ``fused_train_step`` for a checkpoint: per table the moments and the update count (recbole's
        checkpoint stores ``optimizer.state_dict()``; this is its counterpart for ``optimizer_mode='rowwise'``), and under ``'weights'``
        the dense Adam state of the ``_WEIGHT_STEP`` step's parameters."""
        cache = self.__dict__.get('_fused')
        if not cache:
            return {}
        self.fused_sync()
        out = {'tables': {k: {'step': st.step, 'exp_avg': st.exp_avg, 'exp_avg_sq': st.exp_avg_sq} for k, st in cache['states'].items()}}
        codes = {getattr(st, 'opt', None) for st in cache['states'].values()} - {None}
        if len(codes) == 1:                                    # the learner the state belongs to: a resume under another one is refused
            out['opt'] = OPT_NAMES[codes.pop()]
        step = cache['steps'].get(self._WEIGHT_STEP)
        if step is not None and step.w_opt is not None:
            out['weights'] = step.w_opt.state_dict()
        return out

    def load_fused_optimizer_state(self, state, opt='adam', adam='lazy'):
        """Restore what ``fused_optimizer_state`` returned (before the next ``fused_train_step``).  ``adam``: the mode training goes on
        with; in exact mode every row is current at its table's update count (the checkpoint was written flushed).  The dense weights'
        Adam state is handed to the ``_WEIGHT_STEP`` step when it is next built."""
        code = opt_code(opt)
        if state.get('opt', opt) != opt:                       # (before any state exists)
            raise ValueError(f"the checkpoint's row-wise optimizer state was written under opt={state['opt']!r}; it cannot be resumed under "
                             f"opt={opt!r}")
        self._fused_cache()
        for name, rec in state.get('tables', {}).items():
            st = self._fused_state(name, code, adam == 'exact')
            st.step = int(rec['step'])
            if rec['exp_avg'] is not None:
                st.exp_avg.copy_(rec['exp_avg'])
            if rec['exp_avg_sq'] is not None:
                st.exp_avg_sq.copy_(rec['exp_avg_sq'])
            st.restored()
        if self._WEIGHT_STEP is not None:
            if 'weights' in state:
                self.__dict__['_pending_weight_state'] = state['weights']
            self._fused['steps'].pop(self._WEIGHT_STEP, None)
