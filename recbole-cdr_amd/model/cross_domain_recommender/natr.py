"""NATR on libcdrhip -- same class contract as recbole_cdr/model/cross_domain_recommender/natr.py:23-191.

Phase 1 (SOURCE, natr.py:98-110): sigmoid-dot BCE on the source tables -- the fused gather-dot-loss kernel.
Phase 2 (TARGET, natr.py:112-168): the history of the row's user (overlap_items) or item (overlap_users) in the target domain is
looked up in the SOURCE table, pushed through the transfer layer on the fp32-MFMA contraction ([B * n_hist, Ds] x [Ds, Dt]) and
one kernel (cdr_natr_att_fwd / _bwd, one wave per batch row) does unit-level attention, masked softmax, the weighted history
sum, the domain-level gate and the score; BCE + reg_weight * RegLoss (sum of five 2-norms) natively.  The history matrices are
built on the device (data/history.py).  set_phase('TARGET') freezes the source tables as the reference does (natr.py:69-73).

Evaluation.  The reference defines ``predict`` only (natr.py:178-191), so ``full_sort_predict`` raises NotImplementedError and there is no
``full_sort_topk``: the trainer scores every (user, item) pair through chunked ``predict``.  ``config['native_full_sort']`` (opt-in) adds
both for phase 2 (every phase except 'SOURCE', where ``predict`` scores source ids and the reference's contract stays): the history
summary su of every key once (functional.natr_history_summary; in overlap_users mode the keys are all target items and the result is kept
for the length of a ``freeze_for_eval()`` / ``unfreeze_eval()`` bracket), then csrc/cdr_natr_fullsort.hip scores every evaluated user
against every target item in one launch, with the evaluation mask + top-k as the kernel's second epilogue."""
import torch
import torch.nn as nn

from ... import binding as B_
from ... import functional as F_
from ...utils import InputType
from ..crossdomain_recommender import CrossDomainRecommender, xavier_normal_initialization


class NATR(CrossDomainRecommender):
    input_type = InputType.POINTWISE

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.mode = self.one_sided_overlap_mode()
        self.phase = None
        self.source_embedding_size = config['source_embedding_size']
        self.target_embedding_size = config['target_embedding_size']
        self.reg_weight = config['reg_weight']
        self.max_inter_length = config['max_inter_length']
        self.SOURCE_LABEL = dataset.source_domain_dataset.label_field
        self.TARGET_LABEL = dataset.target_domain_dataset.label_field
        if self.mode == 'overlap_users':
            self.history_user_matrix, self.history_lens, self.mask_mat = self.get_history_user_info(dataset)
        if self.mode == 'overlap_items':
            self.history_item_matrix, self.history_lens, self.mask_mat = self.get_history_item_info(dataset)

        self.source_user_embedding = nn.Embedding(self.total_num_users, self.source_embedding_size)
        self.source_item_embedding = nn.Embedding(self.total_num_items, self.source_embedding_size)
        self.target_user_embedding = nn.Embedding(self.total_num_users, self.target_embedding_size)
        self.target_item_embedding = nn.Embedding(self.total_num_items, self.target_embedding_size)
        # (the reference zero-fills the rows a domain never sees, natr.py:61-65, then re-initialises every table, :73)
        self.transfer_layer = nn.Linear(self.source_embedding_size, self.target_embedding_size)
        self.unit_attention_layer = nn.Linear(self.target_embedding_size, 1)
        self.domain_attention_layer = nn.Linear(self.target_embedding_size, 1)
        self.apply(xavier_normal_initialization)
        self.__dict__['_native_full_sort'] = bool(config['native_full_sort']) if 'native_full_sort' in config else False

    def set_phase(self, phase):
        self.phase = phase
        if phase == 'TARGET':
            self.source_item_embedding.weight.requires_grad = False
            self.source_user_embedding.weight.requires_grad = False

    def _history_info(self, triple):
        matrix, _, lens = triple
        matrix = matrix[:, :self.max_inter_length].contiguous().to(self.device)
        lens = lens.to(self.device)
        mask = (torch.arange(matrix.shape[1], device=matrix.device) < lens.unsqueeze(1)).float()
        return matrix, lens, mask

    def get_history_item_info(self, dataset):
        return self._history_info(dataset.history_item_matrix(domain='target'))

    def get_history_user_info(self, dataset):
        return self._history_info(dataset.history_user_matrix(domain='target'))

    def _phase1(self, user, item, label):
        return F_.PointGatherLoss.apply(B_.CDR_LOSS_BCE, self.source_user_embedding.weight, self.source_item_embedding.weight,
                                        None, None, user, item, label, 0.0)

    def phase1_forward(self, user, item):
        with torch.no_grad():
            return self._phase1(user, item, torch.zeros(user.numel(), device=user.device))[1]

    def calculate_phase1_loss(self, interaction):
        return self._phase1(interaction[self.SOURCE_USER_ID], interaction[self.SOURCE_ITEM_ID],
                            interaction[self.SOURCE_LABEL])[0].reshape(())

    def phase2_forward(self, user, item):
        user_e = F_.gather_rows(self.target_user_embedding.weight, user)
        item_e = F_.gather_rows(self.target_item_embedding.weight, item)
        if self.mode == 'overlap_items':
            key, hist, src, pu, qi = user, self.history_item_matrix, self.source_item_embedding.weight, user_e, item_e
        else:
            key, hist, src, pu, qi = item, self.history_user_matrix, self.source_user_embedding.weight, item_e, user_e
        key = key.reshape(-1)
        he = F_.gather_rows(src, hist[key])                                              # [B, n_hist, Ds]
        he = F_.linear(he, self.transfer_layer.weight, self.transfer_layer.bias, B_.ACT_NONE)   # [B, n_hist, Dt]
        return F_.NatrAttention.apply(he, pu, qi, self.mask_mat[key], self.unit_attention_layer.weight,
                                      self.unit_attention_layer.bias, self.domain_attention_layer.weight,
                                      self.domain_attention_layer.bias)

    def calculate_phase2_loss(self, interaction):
        score = self.phase2_forward(interaction[self.TARGET_USER_ID], interaction[self.TARGET_ITEM_ID])
        rec_loss = F_.BCEProbLoss.apply(score, interaction[self.TARGET_LABEL])
        reg_loss = None                                                                  # recbole RegLoss: sum of 2-norms
        for w in (self.target_user_embedding.weight, self.target_item_embedding.weight, self.transfer_layer.weight,
                  self.unit_attention_layer.weight, self.domain_attention_layer.weight):
            n = F_.FrobeniusNorm.apply(w)
            reg_loss = n if reg_loss is None else reg_loss + n
        return rec_loss + self.reg_weight * reg_loss

    def graph_key(self):
        return ('NATR', self.phase)

    def calculate_loss(self, interaction):
        if self.phase == 'SOURCE':
            return self.calculate_phase1_loss(interaction)
        elif self.phase == 'TARGET':
            return self.calculate_phase2_loss(interaction)
        return None

    @torch.no_grad()
    def predict(self, interaction):
        if self.phase == 'SOURCE':
            return self.phase1_forward(interaction[self.SOURCE_USER_ID], interaction[self.SOURCE_ITEM_ID])
        return self.phase2_forward(interaction[self.TARGET_USER_ID], interaction[self.TARGET_ITEM_ID])


    # ---- full-sort evaluation, opt-in (config['native_full_sort']) ------------------------------------------------
    # Properties, as in DeepAPF: with the flag off -- or in phase 'SOURCE', where ``predict`` scores source ids -- ``full_sort_topk`` raises
    # AttributeError (``hasattr`` is False) and ``full_sort_predict`` is the base class's, which raises NotImplementedError: the reference's
    # contract, on which the trainer's chunked-``predict`` route rests.  The flag is a plain bool in ``__dict__``: pickle and deepcopy carry it.
    def _full_sort_on(self):
        return self.__dict__.get('_native_full_sort', False) and self.phase != 'SOURCE'

    @property
    def full_sort_predict(self):
        if self._full_sort_on():
            return self._native_full_sort_predict
        return super().full_sort_predict

    @property
    def full_sort_topk(self):
        if self._full_sort_on():
            return self._native_full_sort_topk
        raise AttributeError("'NATR' object has no attribute 'full_sort_topk' (config['native_full_sort'] is off, or phase 'SOURCE')")

    # The item keys' summary (overlap_users) depends on no user: it is cached only between ``freeze_for_eval()`` and ``unfreeze_eval()``
    # (Trainer.evaluate brackets its loop with the pair: nothing trains in between) and only while ``not self.training``; outside a bracket
    # every call recomputes from the live parameters.  With the flag off both methods leave the model as it is.
    def freeze_for_eval(self):
        if self.__dict__.get('_native_full_sort', False):
            self.__dict__.pop('_eval_su', None)
            self.__dict__['_eval_frozen'] = True
        return self

    def unfreeze_eval(self):
        self.__dict__.pop('_eval_frozen', None)
        self.__dict__.pop('_eval_su', None)
        return self

    def train(self, mode=True):
        if mode:
            self.unfreeze_eval()
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self.unfreeze_eval()
        return super().load_state_dict(*args, **kwargs)

    def __getstate__(self):
        # pickle / copy.deepcopy / torch.save(model): the cache is table-sized and cheap to rebuild
        st = dict(self.__dict__)
        for k in ('_eval_su', '_eval_frozen'):
            st.pop(k, None)
        return st

    def _history_summary(self, keys, chunk_rows=None):
        """su [len(keys), Dt] of the mode's key side (functional.natr_history_summary on the model's tables and layers)."""
        if self.mode == 'overlap_items':
            hist, src, tab = self.history_item_matrix, self.source_item_embedding.weight, self.target_user_embedding.weight
        else:
            hist, src, tab = self.history_user_matrix, self.source_user_embedding.weight, self.target_item_embedding.weight
        return F_.natr_history_summary(src, hist, self.mask_mat, tab, keys, self.transfer_layer.weight, self.transfer_layer.bias,
                                       self.unit_attention_layer.weight, self.unit_attention_layer.bias,
                                       self.domain_attention_layer.weight, self.domain_attention_layer.bias, chunk_rows=chunk_rows)

    def _fullsort_operands(self, uid):
        """(key_is_item, su, key table, other table, w) of ``phase2_forward`` in the dataset's mode for the evaluated users ``uid``."""
        w = self.domain_attention_layer.weight
        if self.mode == 'overlap_items':
            return False, self._history_summary(uid), self.target_user_embedding.weight, self.target_item_embedding.weight, w
        caching = (not self.training) and bool(self.__dict__.get('_eval_frozen', False))
        su = self.__dict__.get('_eval_su') if caching else None
        if su is None:
            su = self._history_summary(torch.arange(int(self.target_num_items), device=uid.device))
            if caching:
                self.__dict__['_eval_su'] = su
        return True, su, self.target_item_embedding.weight, self.target_user_embedding.weight, w

    @torch.no_grad()
    def _native_full_sort_predict(self, interaction):
        """[U * N]: ``predict`` (phase 2) for every evaluated user against every target item -- one scoring launch behind the key side's
        history summary for the widths the kernel takes (Dt in 4..128, a multiple of 4); chunked ``phase2_forward`` over all pairs otherwise."""
        uid = interaction[self.TARGET_USER_ID].reshape(-1)
        N = int(self.target_num_items)
        if F_.natr_fullsort_supported(self.target_embedding_size):
            ki, su, key_tab, other_tab, w = self._fullsort_operands(uid)
            return F_.natr_fullsort(ki, su, key_tab, other_tab, uid, N, w).view(-1)
        items = torch.arange(N, device=uid.device)
        per = max(1, (1 << 20) // N)                                       # users per ``phase2_forward`` call
        rows = [self.phase2_forward(uid[s:s + per].repeat_interleave(N), items.repeat(min(per, uid.numel() - s))).reshape(-1)
                for s in range(0, uid.numel(), per)]
        return torch.cat(rows).float()

    @torch.no_grad()
    def _native_full_sort_topk(self, interaction, k, hist_indptr=None, hist_cols=None):
        """(values [U,k], item ids [U,k]) of ``full_sort_predict`` after the evaluation mask (PAD column, per-user history CSR): the fused
        launch from ``F_.NATR_TOPK_MIN_ITEMS`` target items on (``self.fullsort_topk_min_items`` overrides) -- values bit-equal to the
        unfused scores; mask + ``torch.topk`` of ``full_sort_predict`` below it and for widths outside the kernel's range."""
        if k > F_.FUSED_TOPK_MAX:                # beyond the fused kernels' lists: the wide route, whatever the catalogue size
            return self.full_sort_topk_wide(interaction, k, hist_indptr, hist_cols)
        uid = interaction[self.TARGET_USER_ID].reshape(-1)
        N = int(self.target_num_items)
        if not F_.natr_fullsort_supported(self.target_embedding_size) or \
                N < self.__dict__.get('fullsort_topk_min_items', F_.NATR_TOPK_MIN_ITEMS):
            scores = self._native_full_sort_predict(interaction).view(uid.numel(), -1)
            return F_.masked_topk(scores, k, hist_indptr, hist_cols)
        ki, su, key_tab, other_tab, w = self._fullsort_operands(uid)
        return F_.natr_fullsort_topk(ki, su, key_tab, other_tab, uid, N, w, k, hist_indptr=hist_indptr, hist_cols=hist_cols)
