"""DeepAPF on libcdrhip -- same class contract as recbole_cdr/model/cross_domain_recommender/deepapf.py:23-175.

Per domain (deepapf.py:69-152): the overlapped side has a share row and a domain-only row; both are multiplied with the other
side's row, scored by the two-layer attention MLP (ONE [2B, D] operand through the fp32-MFMA contraction: cdr_apf_prod), the pair
of scores goes through a masked softmax, the rows are merged and scored by the predict layer (cdr_apf_combine), BCE natively.
Quirks kept: the share score is masked where id > overlapped_num (strictly), i.e. the first non-overlapped id still uses its
share row; ``self.user_mlp = self.seq = ...; self.item_mlp = self.seq = ...`` -- the item MLP is ALSO registered as ``seq`` and
``named_parameters()`` reports it under that name (reference checkpoints carry user_mlp.*, seq.* and item_mlp.*).

``fused_train_step`` (``optimizer_mode='rowwise'``): the BOTH-phase step without table-sized gradients -- fused.FusedDeepAPFStep, the five
live tables (the overlapped side's share table, fed by both batches, and per domain the only table and the other side's table) updated
row-wise from csrc/cdr_deepapf.hip's compact gradient rows, the attention MLP of the mode and the predict layer by the exact dense Adam;
``adam='exact'`` puts the catch-up of the reference's dense Adam in front of it (fused.rowwise_catch_up over the five tables).

Evaluation.  The reference defines ``predict`` only (deepapf.py:157-161), so ``full_sort_predict`` raises NotImplementedError and there is
no ``full_sort_topk``: the trainer scores every (user, item) pair through chunked ``predict``.  ``config['native_full_sort']`` (opt-in)
adds both on csrc/cdr_deepapf_fullsort.hip -- every evaluated user against every target item in one launch, with the evaluation mask +
top-k as the kernel's second epilogue; ``predict`` always scores the target domain, so does the full sort in every phase."""
import torch
import torch.nn as nn

from ... import binding as B_
from ... import functional as F_
from ...utils import InputType
from ..crossdomain_recommender import CrossDomainRecommender, xavier_normal_initialization
from ..rowwise import RowwiseTraining


class DeepAPF(RowwiseTraining, CrossDomainRecommender):
    input_type = InputType.POINTWISE

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.SOURCE_LABEL = dataset.source_domain_dataset.label_field
        self.TARGET_LABEL = dataset.target_domain_dataset.label_field
        self.mode = self.one_sided_overlap_mode()
        self.embedding_size = config['embedding_size']
        self.beta = config['beta']

        self.source_user_embedding = nn.Embedding(self.total_num_users, self.embedding_size)
        self.target_user_embedding = nn.Embedding(self.total_num_users, self.embedding_size)
        self.share_user_embedding = nn.Embedding(self.total_num_users, self.embedding_size)
        self.source_item_embedding = nn.Embedding(self.total_num_items, self.embedding_size)
        self.target_item_embedding = nn.Embedding(self.total_num_items, self.embedding_size)
        self.share_item_embedding = nn.Embedding(self.total_num_items, self.embedding_size)
        self.user_mlp = self.seq = nn.Sequential(nn.Linear(self.embedding_size, self.embedding_size), nn.ReLU(),
                                                 nn.Linear(self.embedding_size, 1, bias=False))
        self.item_mlp = self.seq = nn.Sequential(nn.Linear(self.embedding_size, self.embedding_size), nn.ReLU(),
                                                 nn.Linear(self.embedding_size, 1, bias=False))
        self.predict_layer = nn.Linear(self.embedding_size, 1, bias=False)
        self.apply(xavier_normal_initialization)
        self.phase = 'BOTH'
        self.__dict__['_native_full_sort'] = bool(config['native_full_sort']) if 'native_full_sort' in config else False
        self.__dict__['_dist_cfg'] = config['dist_group'] if 'dist_group' in config else None

    def set_phase(self, phase):
        self.phase = phase

    def _forward(self, user, item, domain):
        if self.mode == 'overlap_users':
            share = F_.gather_rows(self.share_user_embedding.weight, user)
            only = F_.gather_rows(getattr(self, f'{domain}_user_embedding').weight, user)
            other = F_.gather_rows(getattr(self, f'{domain}_item_embedding').weight, item)
            key, n_over, mlp = user, self.overlapped_num_users, self.user_mlp
        else:
            other = F_.gather_rows(getattr(self, f'{domain}_user_embedding').weight, user)
            share = F_.gather_rows(self.share_item_embedding.weight, item)
            only = F_.gather_rows(getattr(self, f'{domain}_item_embedding').weight, item)
            key, n_over, mlp = item, self.overlapped_num_items, self.item_mlp
        x = F_.ApfProduct.apply(share, only, other)                                       # [2B, D]
        a = F_.linear(F_.linear(x, mlp[0].weight, mlp[0].bias, B_.ACT_RELU), mlp[2].weight, None, B_.ACT_NONE)   # [2B, 1]
        return F_.ApfCombine.apply(a, share, only, other, self.predict_layer.weight, key, int(n_over))

    def source_forward(self, user, item):
        return self._forward(user, item, 'source')

    def target_forward(self, user, item):
        return self._forward(user, item, 'target')

    def forward(self):
        pass

    @torch.no_grad()
    def predict(self, interaction):
        return self.target_forward(interaction[self.TARGET_USER_ID], interaction[self.TARGET_ITEM_ID])

    def graph_key(self):
        return ('DeepAPF',)

    # ---- full-sort evaluation, opt-in (config['native_full_sort']) ------------------------------------------------
    # Properties: with the flag off ``full_sort_topk`` raises AttributeError (nn.Module.__getattr__ then reports the attribute missing, so
    # ``hasattr`` is False) and ``full_sort_predict`` is the base class's, which raises NotImplementedError -- the reference's contract, on
    # which the trainer's chunked-``predict`` route rests.  The flag is a plain bool in ``__dict__``: pickle and deepcopy carry it.
    @property
    def full_sort_predict(self):
        if self.__dict__.get('_native_full_sort', False):
            return self._native_full_sort_predict
        return super().full_sort_predict

    @property
    def full_sort_topk(self):
        if self.__dict__.get('_native_full_sort', False):
            return self._native_full_sort_topk
        raise AttributeError("'DeepAPF' object has no attribute 'full_sort_topk' (config['native_full_sort'] is off)")

    def _fullsort_operands(self):
        """(key_is_item, share, only, other, n_overlap, W1, b1, w2, wp) of ``target_forward`` in the dataset's mode."""
        W1, b1, w2, wp = self._attention_params()
        if self.mode == 'overlap_users':
            return (False, self.share_user_embedding.weight, self.target_user_embedding.weight, self.target_item_embedding.weight,
                    int(self.overlapped_num_users), W1, b1, w2, wp)
        return (True, self.share_item_embedding.weight, self.target_item_embedding.weight, self.target_user_embedding.weight,
                int(self.overlapped_num_items), W1, b1, w2, wp)

    @torch.no_grad()
    def _native_full_sort_predict(self, interaction):
        """[U * N]: ``predict`` for every evaluated user against every target item -- one launch for the widths the kernel takes
        (4..128, a multiple of 4); chunked ``predict`` over all pairs otherwise."""
        uid = interaction[self.TARGET_USER_ID].reshape(-1)
        N = int(self.target_num_items)
        if F_.deepapf_fullsort_supported(self.embedding_size):
            ki, share, only, other, n_over, W1, b1, w2, wp = self._fullsort_operands()
            return F_.deepapf_fullsort(ki, share, only, other, uid, N, n_over, W1, b1, w2, wp).view(-1)
        items = torch.arange(N, device=uid.device)
        per = max(1, (1 << 20) // N)                                       # users per ``predict`` call
        rows = [self.target_forward(uid[s:s + per].repeat_interleave(N), items.repeat(min(per, uid.numel() - s))).reshape(-1)
                for s in range(0, uid.numel(), per)]
        return torch.cat(rows).float()

    @torch.no_grad()
    def _native_full_sort_topk(self, interaction, k, hist_indptr=None, hist_cols=None):
        """(values [U,k], item ids [U,k]) of ``full_sort_predict`` after the evaluation mask (PAD column, per-user history CSR): the fused
        launch from ``F_.DEEPAPF_TOPK_MIN_ITEMS`` target items on (``self.fullsort_topk_min_items`` overrides) -- values bit-equal to the
        unfused scores; mask + ``torch.topk`` of ``full_sort_predict`` below it and for widths outside the kernel's range."""
        if k > F_.FUSED_TOPK_MAX:                # beyond the fused kernels' lists: the wide route, whatever the catalogue size
            return self.full_sort_topk_wide(interaction, k, hist_indptr, hist_cols)
        uid = interaction[self.TARGET_USER_ID].reshape(-1)
        N = int(self.target_num_items)
        if not F_.deepapf_fullsort_supported(self.embedding_size) or \
                N < self.__dict__.get('fullsort_topk_min_items', F_.DEEPAPF_TOPK_MIN_ITEMS):
            scores = self._native_full_sort_predict(interaction).view(uid.numel(), -1)
            return F_.masked_topk(scores, k, hist_indptr, hist_cols)
        ki, share, only, other, n_over, W1, b1, w2, wp = self._fullsort_operands()
        return F_.deepapf_fullsort_topk(ki, share, only, other, uid, N, n_over, W1, b1, w2, wp, k, hist_indptr=hist_indptr,
                                        hist_cols=hist_cols)

    def calculate_loss(self, interaction):
        p_source = self.source_forward(interaction[self.SOURCE_USER_ID], interaction[self.SOURCE_ITEM_ID])
        p_target = self.target_forward(interaction[self.TARGET_USER_ID], interaction[self.TARGET_ITEM_ID])
        return F_.BCEProbLoss.apply(p_source, interaction[self.SOURCE_LABEL]) + \
            F_.BCEProbLoss.apply(p_target, interaction[self.TARGET_LABEL])

    # ---- O(batch) training step (large tables) ------------------------------------------------------------------
    def _roles(self):
        """(table attribute names by role: share, source only, source other, target only, target other; the attention MLP; n_overlap;
        key field kind) of the mode -- ``_forward``'s choice.  The other share table and the other MLP are not part of the step."""
        if self.mode == 'overlap_users':
            return (('share_user_embedding', 'source_user_embedding', 'source_item_embedding', 'target_user_embedding',
                     'target_item_embedding'), self.user_mlp, int(self.overlapped_num_users), 'user')
        return (('share_item_embedding', 'source_item_embedding', 'source_user_embedding', 'target_item_embedding',
                 'target_user_embedding'), self.item_mlp, int(self.overlapped_num_items), 'item')

    def _attention_params(self):
        """(W1, b1, w2, wp): the attention MLP of the mode and the predict layer."""
        mlp = self._roles()[1]
        return mlp[0].weight, mlp[0].bias, mlp[2].weight, self.predict_layer.weight

    def _pair_fields(self, interaction):
        fields = (self.SOURCE_USER_ID, self.SOURCE_ITEM_ID, self.SOURCE_LABEL, self.TARGET_USER_ID, self.TARGET_ITEM_ID, self.TARGET_LABEL)
        missing = [f for f in fields if f not in interaction]
        if missing:
            raise ValueError(f'DeepAPF.fused_train_step trains on BOTH-phase batches (source and target rows); the {self.phase} batch '
                             f'has no {", ".join(missing)}')
        return [interaction[f].reshape(-1) for f in fields]

    def fused_train_step(self, interaction, opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adam='lazy'):
        """``calculate_loss -> backward -> optimizer.step`` on a BOTH-phase batch without table-sized gradients or a dense optimizer
        sweep over the tables (fused.FusedDeepAPFStep): what ``CrossDomainTrainer`` runs when ``config['optimizer_mode'] == 'rowwise'``.
        Same loss and gradients as ``calculate_loss``; each of the five live tables advances once per step -- a share row named by both
        batches gets one update from the sum of its contributions -- and the attention MLP and the predict layer take the exact dense
        Adam (the reference has one ``torch.optim.Adam`` over every parameter).  The MLP the mode does not use and the share table of the
        other side have no gradient in the reference either and do not move.  Returns the total loss (device [1]).

        ``adam='lazy'`` (default): table rows the batch does not touch do not move; every row a batch names is touched, a masked
        occurrence's share row included (with a zero gradient row).  ``adam='exact'``: the reference's dense Adam -- two catch-up launches in
        front of every step (fused.rowwise_catch_up takes up to four tables; there are five) replays the gradient-free updates the step's rows missed; the tables hold what
        ``torch.optim.Adam`` over whole tables would have left once ``fused_sync()`` has run.  One mode per model.

        Refused before any state is created: a batch without the BOTH-phase fields, empty or unequal-length domain batches,
        ``config['dist_group']``, and widths outside ``FusedDeepAPFStep.check_widths`` (use optimizer_mode=dense for those)."""
        from ...fused import FusedDeepAPFStep, rowwise_catch_up
        exact, code, hp = self._fused_args(opt, adam, lr, betas, eps, weight_decay)
        self._fused_refuse_dist('DeepAPF')
        self._fused_check_widths('DeepAPF', FusedDeepAPFStep.check_widths, 'embedding_size = {}', self.embedding_size)
        su, si, ys, tu, ti, yt = self._pair_fields(interaction)
        Bs, Bt = self._fused_check_pair_batch('DeepAPF', su, si, ys, tu, ti, yt)
        names, _mlp, n_over, kind = self._roles()
        ks, os_, kt, ot = (su, si, tu, ti) if kind == 'user' else (si, su, ti, tu)
        self._fused_cache(exact)
        states = tuple(self._fused_state(n, code, exact) for n in names)
        ms, mt = self._fused_pair_sizes('deepapf', Bs, Bt)
        step = self._fused_weight_step('deepapf', lambda s: s.max_source >= Bs and s.max_target >= Bt, lambda: FusedDeepAPFStep(
            *(getattr(self, n).weight.data for n in names), self._attention_params(), n_over, ms, mt, states=states, **hp), hp)
        ys = ys if ys.dtype == torch.float32 else ys.float()
        yt = yt if yt.dtype == torch.float32 else yt.float()
        ks, os_, kt, ot = ks.contiguous(), os_.contiguous(), kt.contiguous(), ot.contiguous()
        if exact:
            # [ks, kt] names the share table's rows; each domain's key list its only table's, its other list its other table's
            named = list(zip(states, ([ks, kt], [ks], [os_], [kt], [ot])))
            for part in (named[:3], named[3:]):                         # (a catch-up launch takes up to four tables)
                rowwise_catch_up(part, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        return step.step(ks, os_, ys.contiguous(), kt, ot, yt.contiguous())

    def _fused_phase_step(self):
        return self._fused['steps']['deepapf']

    _WEIGHT_STEP = 'deepapf'                                          # ((W1, b1, w2, wp)'s dense Adam state: the checkpoint's 'weights')
