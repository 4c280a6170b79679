"""CLFM on libcdrhip -- same class contract as recbole_cdr/model/cross_domain_recommender/clfm.py:23-145.

Per domain: user rows [B, Du] -> factors = user_e [shared_linear ; <domain>_only_linear]^T (ONE fp32-MFMA contraction over the stacked
weight) -> sigmoid(factors . item_row) -> BCE in the fused gather-dot-loss kernel (the factors play the "user table", addressed
by row number) + reg_weight * EmbLoss of the gathered ego rows.  Scoring: factors x item slab on the MFMA full-sort kernel.
Quirk kept: ``target_item_embedding_size`` is read from ``config['source_item_embedding_size']`` (clfm.py:39).

``fused_train_step`` (``optimizer_mode='rowwise'``): the BOTH-phase step without table-sized gradients -- fused.FusedCLFMStep, the four
tables updated row-wise from csrc/cdr_clfm.hip's compact gradient rows, the three small weights by the exact dense Adam; ``adam='exact'``
puts the catch-up of the reference's dense Adam in front of it (fused.rowwise_catch_up over the four tables)."""
import torch
import torch.nn as nn

from ... import binding as B_
from ... import functional as F_
from ...utils import InputType
from ..crossdomain_recommender import CrossDomainRecommender, xavier_normal_initialization
from ..contraction import ContractionScoring
from ..rowwise import RowwiseTraining


class CLFM(RowwiseTraining, ContractionScoring, CrossDomainRecommender):
    input_type = InputType.POINTWISE

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.SOURCE_LABEL = dataset.source_domain_dataset.label_field
        self.TARGET_LABEL = dataset.target_domain_dataset.label_field
        self.user_embedding_size = config['user_embedding_size']
        self.source_item_embedding_size = config['source_item_embedding_size']
        self.target_item_embedding_size = config['source_item_embedding_size']
        self.share_embedding_size = config['share_embedding_size']
        self.alpha = config['alpha']
        self.reg_weight = config['reg_weight']
        assert 0 <= self.share_embedding_size <= self.source_item_embedding_size and \
            0 <= self.share_embedding_size <= self.target_item_embedding_size

        self.source_user_embedding = nn.Embedding(self.total_num_users, self.user_embedding_size)
        self.target_user_embedding = nn.Embedding(self.total_num_users, self.user_embedding_size)
        self.source_item_embedding = nn.Embedding(self.total_num_items, self.source_item_embedding_size)
        self.target_item_embedding = nn.Embedding(self.total_num_items, self.target_item_embedding_size)
        if self.share_embedding_size > 0:
            self.shared_linear = nn.Linear(self.user_embedding_size, self.share_embedding_size, bias=False)
        if self.source_item_embedding_size - self.share_embedding_size > 0:
            self.source_only_linear = nn.Linear(self.user_embedding_size,
                                                self.source_item_embedding_size - self.share_embedding_size, bias=False)
        if self.target_item_embedding_size - self.share_embedding_size > 0:
            self.target_only_linear = nn.Linear(self.user_embedding_size,
                                                self.target_item_embedding_size - self.share_embedding_size, bias=False)
        self.apply(xavier_normal_initialization)
        self.phase = 'BOTH'
        self.__dict__['_dist_cfg'] = config['dist_group'] if 'dist_group' in config else None

    def set_phase(self, phase):
        self.phase = phase

    def _tables(self, domain):
        return getattr(self, f'{domain}_user_embedding').weight, getattr(self, f'{domain}_item_embedding').weight

    def _factors(self, user_e, domain):
        """cat([shared_linear(u), <domain>_only_linear(u)], 1) as one contraction over the row-stacked weights (clfm.py:77-85)."""
        ws = []
        if self.share_embedding_size > 0:
            ws.append(self.shared_linear.weight)
        only = getattr(self, f'{domain}_only_linear', None)
        if only is not None:
            ws.append(only.weight)
        w = ws[0] if len(ws) == 1 else torch.cat(ws, dim=0)
        return F_.linear(user_e, w, None, B_.ACT_NONE)

    def _loss_and_prob(self, user, item, label, domain):
        U, I = self._tables(domain)
        fac = self._factors(F_.gather_rows(U, user), domain)
        rows = torch.arange(fac.shape[0], device=fac.device, dtype=torch.int64)
        return F_.PointGatherLoss.apply(B_.CDR_LOSS_BCE, fac, I, None, None, rows, item, label, 0.0)

    def _emb_loss(self, user, item, domain):
        U, I = self._tables(domain)
        if U.shape[1] == I.shape[1]:
            return F_.EmbLossRows.apply(U, I, user, item)
        # recbole EmbLoss with differently sized tables: (||U[u]||_F + ||I[i]||_F) / B
        return (F_.FrobeniusNorm.apply(F_.gather_rows(U, user)) + F_.FrobeniusNorm.apply(F_.gather_rows(I, item))) / item.numel()

    def source_forward(self, user, item):
        with torch.no_grad():
            return self._loss_and_prob(user, item, torch.zeros(user.numel(), device=user.device), 'source')[1]

    def target_forward(self, user, item):
        with torch.no_grad():
            return self._loss_and_prob(user, item, torch.zeros(user.numel(), device=user.device), 'target')[1]

    def _rows(self, n, dev):
        """arange(n) on the device, made once per batch length (the factor rows of a batch are addressed 0..n-1)."""
        cache = self.__dict__.setdefault('_row_ids', {})
        key = (n, str(dev))
        if key not in cache:
            cache[key] = torch.arange(n, device=dev, dtype=torch.int64)
        return cache[key]

    def graph_key(self):
        return ('CLFM',)

    def calculate_loss(self, interaction):
        su, si, sl = interaction[self.SOURCE_USER_ID], interaction[self.SOURCE_ITEM_ID], interaction[self.SOURCE_LABEL]
        tu, ti, tl = interaction[self.TARGET_USER_ID], interaction[self.TARGET_ITEM_ID], interaction[self.TARGET_LABEL]
        (Us, Is), (Ut, It) = self._tables('source'), self._tables('target')
        fs, ft = self._factors(F_.gather_rows(Us, su), 'source'), self._factors(F_.gather_rows(Ut, tu), 'target')
        if fs.shape[1] == ft.shape[1] and fs.shape[1] % 4 == 0:
            # both domains' gather-dot-BCE in one launch each way (functional.TwoPointLoss)
            bce_s, bce_t, _, _ = F_.TwoPointLoss.apply(B_.CDR_LOSS_BCE, fs, Is, ft, It, self._rows(fs.shape[0], fs.device), si, sl,
                                                       self._rows(ft.shape[0], ft.device), ti, tl)
        else:
            bce_s, _ = F_.PointGatherLoss.apply(B_.CDR_LOSS_BCE, fs, Is, None, None, self._rows(fs.shape[0], fs.device), si, sl, 0.0)
            bce_t, _ = F_.PointGatherLoss.apply(B_.CDR_LOSS_BCE, ft, It, None, None, self._rows(ft.shape[0], ft.device), ti, tl, 0.0)
        out = [bce_s + self.reg_weight * self._emb_loss(su, si, 'source'), bce_t + self.reg_weight * self._emb_loss(tu, ti, 'target')]
        return out[0] * self.alpha + out[1] * (1 - self.alpha)

    # ---- O(batch) training step (large tables) ------------------------------------------------------------------
    _TABLES = ('source_user_embedding', 'source_item_embedding', 'target_user_embedding', 'target_item_embedding')

    def _pair_fields(self, interaction):
        fields = (self.SOURCE_USER_ID, self.SOURCE_ITEM_ID, self.SOURCE_LABEL, self.TARGET_USER_ID, self.TARGET_ITEM_ID, self.TARGET_LABEL)
        missing = [f for f in fields if f not in interaction]
        if missing:
            raise ValueError(f'CLFM.fused_train_step trains on BOTH-phase batches (source and target rows); the {self.phase} batch '
                             f'has no {", ".join(missing)}')
        return [interaction[f].reshape(-1) for f in fields]

    def _weights(self):
        return (self.shared_linear.weight if self.share_embedding_size > 0 else None,
                self.source_only_linear.weight if hasattr(self, 'source_only_linear') else None,
                self.target_only_linear.weight if hasattr(self, 'target_only_linear') else None)

    def fused_train_step(self, interaction, opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adam='lazy'):
        """``calculate_loss -> backward -> optimizer.step`` on a BOTH-phase batch without table-sized gradients or a dense optimizer
        sweep over the four tables (fused.FusedCLFMStep): what ``CrossDomainTrainer`` runs when ``config['optimizer_mode'] ==
        'rowwise'``.  Same loss and gradients as ``calculate_loss``; each table advances once per step, and the three linears take the
        exact dense Adam (the reference has one ``torch.optim.Adam`` over every parameter).  Returns the total loss (device [1]).

        ``adam='lazy'`` (default): table rows the batch does not touch do not move.  ``adam='exact'``: the reference's dense Adam -- one
        catch-up launch in front of every step (fused.rowwise_catch_up) replays the gradient-free updates the step's rows missed; the
        tables hold what ``torch.optim.Adam`` over whole tables would have left once ``fused_sync()`` has run.  One mode per model."""
        from ...fused import FusedCLFMStep, rowwise_catch_up
        exact, code, hp = self._fused_args(opt, adam, lr, betas, eps, weight_decay)
        self._fused_refuse_dist('CLFM')
        self._fused_check_widths('CLFM', FusedCLFMStep.check_widths, 'user_embedding_size = {}, source_item_embedding_size = {}',
                                 self.user_embedding_size, self.source_item_embedding_size)
        su, si, ys, tu, ti, yt = self._pair_fields(interaction)
        Bs, Bt = self._fused_check_pair_batch('CLFM', su, si, ys, tu, ti, yt)
        self._fused_cache(exact)
        states = tuple(self._fused_state(n, code, exact) for n in self._TABLES)
        ms, mt = self._fused_pair_sizes('clfm', Bs, Bt)
        step = self._fused_weight_step('clfm', lambda s: s.max_source >= Bs and s.max_target >= Bt, lambda: FusedCLFMStep(
            *(getattr(self, n).weight.data for n in self._TABLES), self._weights(), ms, mt, self.alpha, self.reg_weight, states=states, **hp), hp)
        ys = ys if ys.dtype == torch.float32 else ys.float()
        yt = yt if yt.dtype == torch.float32 else yt.float()
        if exact:
            rowwise_catch_up([(st, [ids]) for st, ids in zip(states, (su, si, tu, ti))], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        return step.step(su.contiguous(), si.contiguous(), ys.contiguous(), tu.contiguous(), ti.contiguous(), yt.contiguous())

    def _fused_phase_step(self):
        return self._fused['steps']['clfm']

    _WEIGHT_STEP = 'clfm'                                             # (the three linears' dense Adam state: the checkpoint's 'weights')

    # (sampled-candidate evaluation keeps the base class's ``candidate_scores``: ``predict`` applies a sigmoid -- clfm.py:100 of the
    # reference, as CMF's -- and two candidates whose probabilities saturate to the same float tie, which the raw dot would rank apart)
    @torch.no_grad()
    def predict(self, interaction):
        return self.target_forward(interaction[self.TARGET_USER_ID], interaction[self.TARGET_ITEM_ID])

    @torch.no_grad()
    def _full_sort_operands(self, interaction):
        """(user factors, slab0, slab1) of the all-items contraction: what ``ContractionScoring`` derives ``full_sort_predict`` /
        ``full_sort_topk`` / ``full_sort_rank`` from."""
        user_e = F_.gather_rows(self.target_user_embedding.weight, interaction[self.TARGET_USER_ID])
        return self._factors(user_e, 'target'), self.target_item_embedding.weight[:self.target_num_items], None
