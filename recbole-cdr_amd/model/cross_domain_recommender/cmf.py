"""CMF on libcdrhip -- same class contract as recbole_cdr/model/cross_domain_recommender/cmf.py:23-112.
Both domains share one user and one item table; each domain's loss is one fused gather-dot-sigmoid-BCE(+EmbLoss)
launch; scoring is the fp32-MFMA contraction over item rows [0, target_num_items).

``fused_train_step`` (``optimizer_mode='rowwise'``): the BOTH-phase step without table-sized gradients -- fused.FusedPointPairStep, one
update per touched row from the sum of both domains' contributions; ``adam='exact'`` puts the catch-up of the reference's dense Adam in
front of it (fused.rowwise_catch_up)."""
import torch
import torch.nn as nn

from ... import binding as B_
from ... import functional as F_
from ...fused import FusedPointPairStep, rowwise_catch_up
from ...utils import InputType
from ..crossdomain_recommender import CrossDomainRecommender, xavier_normal_initialization
from ..contraction import ContractionScoring
from ..rowwise import RowwiseTraining


class CMF(RowwiseTraining, ContractionScoring, CrossDomainRecommender):
    input_type = InputType.POINTWISE

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.SOURCE_LABEL = dataset.source_domain_dataset.label_field
        self.TARGET_LABEL = dataset.target_domain_dataset.label_field
        self.embedding_size = config['embedding_size']
        self.alpha = config['alpha']
        self.lamda = config['lambda']
        self.gamma = config['gamma']
        self.user_embedding = nn.Embedding(self.total_num_users, self.embedding_size)
        self.item_embedding = nn.Embedding(self.total_num_items, self.embedding_size)
        self.apply(xavier_normal_initialization)
        self.phase = 'BOTH'
        self.__dict__['_dist_cfg'] = config['dist_group'] if 'dist_group' in config else None

    def set_phase(self, phase):
        self.phase = phase

    def _loss_and_prob(self, user, item, label, reg):
        return F_.PointGatherLoss.apply(B_.CDR_LOSS_BCE, self.user_embedding.weight, self.item_embedding.weight,
                                        None, None, user, item, label, reg)

    def forward(self, user, item):
        zeros = torch.zeros(user.numel(), device=user.device, dtype=torch.float32)
        with torch.no_grad():
            _, p = self._loss_and_prob(user, item, zeros, 0.0)
        return p

    def graph_key(self):
        return ('CMF',)

    def calculate_loss(self, interaction):
        # both domains' batches on the shared tables as ONE autograd node (two loss launches forward, two scatter launches into one pair
        # of gradient buffers backward)
        total, _ = F_.TwoDomainPointLoss.apply(
            B_.CDR_LOSS_BCE, self.user_embedding.weight, self.item_embedding.weight,
            interaction[self.SOURCE_USER_ID], interaction[self.SOURCE_ITEM_ID], interaction[self.SOURCE_LABEL], self.lamda,
            interaction[self.TARGET_USER_ID], interaction[self.TARGET_ITEM_ID], interaction[self.TARGET_LABEL], self.gamma, self.alpha)
        return total

    # ---- O(batch) training step (large tables) ------------------------------------------------------------------
    def _pair_fields(self, interaction):
        fields = (self.SOURCE_USER_ID, self.SOURCE_ITEM_ID, self.SOURCE_LABEL, self.TARGET_USER_ID, self.TARGET_ITEM_ID, self.TARGET_LABEL)
        missing = [f for f in fields if f not in interaction]
        if missing:
            raise ValueError(f'CMF.fused_train_step trains on BOTH-phase batches (source and target rows); the {self.phase} batch '
                             f'has no {", ".join(missing)}')
        return [interaction[f].reshape(-1) for f in fields]

    def fused_train_step(self, interaction, opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adam='lazy'):
        """``calculate_loss -> backward -> optimizer.step`` on a BOTH-phase batch without table-sized gradients or a dense optimizer
        sweep (fused.FusedPointPairStep on the shared tables): what ``CrossDomainTrainer`` runs when ``config['optimizer_mode'] ==
        'rowwise'``.  Same loss and per-row gradients as ``calculate_loss``; a row named by both domains' batches gets ONE update from
        their sum, and each table advances once per step, as under the reference's single Adam.  Returns the total loss (device [1]).

        ``adam='lazy'`` (default): rows the batch does not touch do not move.  ``adam='exact'``: the reference's dense Adam -- one catch-up
        launch in front of every step (fused.rowwise_catch_up) replays the gradient-free updates the step's rows missed; the tables hold
        what ``torch.optim.Adam`` over whole tables would have left once ``fused_sync()`` has run.  One mode per model."""
        exact, code, hp = self._fused_args(opt, adam, lr, betas, eps, weight_decay)
        if self.__dict__.get('_dist_cfg') not in (None, False):
            raise ValueError("CMF.fused_train_step does not shard its tables: config['dist_group'] is not supported (one GPU)")
        su, si, ys, tu, ti, yt = self._pair_fields(interaction)
        old = self._fused_cache(exact)['steps'].get('pair')
        us, its = self._fused_state('user_embedding', code, exact), self._fused_state('item_embedding', code, exact)
        Bs, Bt = su.numel(), tu.numel()
        ms, mt = (Bs, Bt) if old is None else (max(Bs, old.max_source), max(Bt, old.max_target))
        step = self._fused_step('pair', lambda s: s.max_source >= Bs and s.max_target >= Bt and s.hp == hp,
                                lambda: FusedPointPairStep(self.user_embedding.weight.data, self.item_embedding.weight.data, ms, mt, self.alpha,
                                                           self.lamda, self.gamma, user_state=us, item_state=its, **hp))
        step.hp = hp
        ys = ys if ys.dtype == torch.float32 else ys.float()
        yt = yt if yt.dtype == torch.float32 else yt.float()
        if exact:
            rowwise_catch_up([(us, [su, tu]), (its, [si, ti])], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        return step.step(su, si, ys, tu, ti, yt)[:1]

    def fused_graph_key(self, interaction, adam='lazy', opt='adam'):
        """Hashable tag of the launches ``fused_train_step(interaction)`` would make, or None when they must not be captured in a hipGraph.
        The step keeps its update counts on the device, so it is capturable while its two-table sort (2 (B_s + B_t) keys) stays below the
        size EMCDR.fused_graph_key refuses to capture (rocPRIM's Onesweep configuration: its temporary-storage resets do not survive a
        replay)."""
        if self.__dict__.get('_dist_cfg') not in (None, False) or opt == 'adagrad':    # (Adagrad: host-side update counts; eager)
            return None
        if self.SOURCE_USER_ID not in interaction or self.TARGET_USER_ID not in interaction:
            return None
        Bs, Bt = interaction[self.SOURCE_USER_ID].numel(), interaction[self.TARGET_USER_ID].numel()
        if 2 * (Bs + Bt) > 3 * 65536:
            return None
        return ('cmf', Bs, Bt, adam)

    def _fused_phase_step(self):
        return self._fused['steps']['pair']

    @torch.no_grad()
    def predict(self, interaction):
        return self.forward(interaction[self.TARGET_USER_ID], interaction[self.TARGET_ITEM_ID])

    @torch.no_grad()
    def _full_sort_operands(self, interaction):
        """(user_e, slab0, slab1) of the all-items contraction: what ``ContractionScoring`` derives ``full_sort_predict`` / ``full_sort_topk``
        / ``full_sort_rank`` from."""
        user_e = F_.gather_rows(self.user_embedding.weight, interaction[self.TARGET_USER_ID])
        return user_e, self.item_embedding.weight[:self.target_num_items], None
