"""DCDCSR on libcdrhip -- same class contract as recbole_cdr/model/cross_domain_recommender/dcdcsr.py:25-280 (trained by
DCDCSRTrainer: SOURCE -> TARGET -> BOTH -> TARGET).

* SOURCE / first TARGET (dcdcsr.py:112-127): BPR without a regulariser -- the fused gather-dot-BPR kernel with reg_weight 0.
* set_phase('BOTH') builds the benchmark embedding (dcdcsr.py:129-165).  The reference loops over every unit in Python with a
  [n_overlap] matmul + topk per unit; here the similarity top-k of ALL non-overlapped units is one call of the fused MFMA
  scoring + top-k kernel (cdr_fullsort_topk_f32: the [units, n_overlap] similarity matrix is never written) followed by a few
  [units, k] elementwise ops -- once per phase switch, not per step.
* BOTH (dcdcsr.py:174-182): numpy-sampled unit ids -> gather -> max-min row normalisation (cdr_maxmin_norm, native backward) ->
  tanh MLP on the MFMA contraction -> MSE against the normalised benchmark rows.
* second TARGET: BPR with the detached affine table standing in for the overlapped side's table (dcdcsr.py:98-110, 204-213).
``predict`` / ``full_sort_predict`` follow the reference's phase table, including full_sort_predict returning [U, N].

``fused_train_step`` (``optimizer_mode='rowwise'``): every phase without table-sized gradients -- the first SOURCE / TARGET visit on the
fused BPR step of the domain's two tables, BOTH on fused.FusedDCDCSRMapStep (csrc/cdr_dcdcsr.hip: the normalisation, the tanh MLP, the MSE
and the whole backward in one pass; the unit table row-wise, the MLP by the exact dense Adam), the second TARGET visit on
fused.FusedFrozenSideBPRStep (the affine table read only, the other side's table row-wise).  One optimizer state per table across the
phases; ``adam='exact'`` puts the catch-up of the reference's dense Adam in front of every step, and ``set_phase`` syncs the tables
before it builds the benchmark or the affine table from them."""
import numpy as np
import torch
import torch.nn as nn

from ... import binding as B_
from ... import functional as F_
from ...utils import InputType
from ..contraction import ContractionScoring
from ..crossdomain_recommender import CrossDomainRecommender, xavier_normal_initialization
from ..rowwise import RowwiseTraining
from .sscdr import MLPLayers


class DCDCSR(RowwiseTraining, ContractionScoring, CrossDomainRecommender):
    input_type = InputType.PAIRWISE

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.mode = self.one_sided_overlap_mode()
        self.phase = None
        self.phase2count = {'SOURCE': 0, 'TARGET': 0, 'BOTH': 0, 'OVERLAP': 0}
        self.latent_factor_model = config['latent_factor_model']
        assert self.latent_factor_model in ['BPR'], f'DCDCSR trains its latent factors with BPR only (latent_factor_model={self.latent_factor_model!r})'
        self.embedding_size = config['embedding_size']
        self.mlp_hidden_size = list(config['mlp_hidden_size'])
        self.k = config['k']
        self.map_batch_size = config['map_batch_size']
        self.SOURCE_LABEL = dataset.source_domain_dataset.label_field
        self.TARGET_LABEL = dataset.target_domain_dataset.label_field
        if self.mode == 'overlap_items':
            self.source_item2pop = self.build_unit2pop(dataset, unit='item', domain='source').to(self.device)
            self.target_item2pop = self.build_unit2pop(dataset, unit='item', domain='target').to(self.device)
        elif self.mode == 'overlap_users':
            self.source_user2pop = self.build_unit2pop(dataset, unit='user', domain='source').to(self.device)
            self.target_user2pop = self.build_unit2pop(dataset, unit='user', domain='target').to(self.device)

        self.source_user_embedding = nn.Embedding(self.total_num_users, self.embedding_size)
        self.source_item_embedding = nn.Embedding(self.total_num_items, self.embedding_size)
        self.target_user_embedding = nn.Embedding(self.total_num_users, self.embedding_size)
        self.target_item_embedding = nn.Embedding(self.total_num_items, self.embedding_size)
        self.benchmark_embedding = None
        self.affine_embedding = None
        # (zero fills of dcdcsr.py:72-76 are overwritten by the initialisation below, :86)
        self.mapping_mlp_layers = MLPLayers([self.embedding_size] + self.mlp_hidden_size + [self.embedding_size])
        self.apply(xavier_normal_initialization)
        self.__dict__['_dist_cfg'] = config['dist_group'] if 'dist_group' in config else None

    @staticmethod
    def build_unit2pop(dataset, unit='user', domain='source'):
        if unit == 'user':
            _, _, history_lens = dataset.history_item_matrix(domain=domain)
        else:
            _, _, history_lens = dataset.history_user_matrix(domain=domain)
        return history_lens.float()

    def _unit(self):
        return 'user' if self.mode == 'overlap_users' else 'item'

    def set_phase(self, phase):
        self.phase = phase
        self.phase2count[phase] += 1
        # exact row-wise Adam: the rows lag behind their tables' update counts, and both builds below read whole tables
        self.fused_sync()
        if self.phase == 'BOTH':
            self.build_benchmark_embedding()
        if self.phase == 'TARGET' and self.phase2count[self.phase] == 2:
            unit = self._unit()
            n_tgt = getattr(self, f'target_num_{unit}s')
            with torch.no_grad():
                e, stats = F_.MaxMinNormalize.apply(getattr(self, f'target_{unit}_embedding').weight[:n_tgt].detach())
                mean_, max_ = stats[:, :1], stats[:, 1:]
                self.affine_embedding = (self.mapping_mlp_layers(e) * (max_ - mean_) + mean_).detach()

    @torch.no_grad()
    def build_unit_benchmark_embedding(self, total_num_units, overlapped_num_units, source_unit2pop, target_unit2pop,
                                       source_unit_embeddings, target_unit_embeddings):
        src = source_unit_embeddings.detach().contiguous()
        tgt = target_unit_embeddings.detach()
        no = overlapped_num_units
        bench = torch.empty(total_num_units, self.embedding_size, device=tgt.device, dtype=torch.float32)
        den = source_unit2pop[:no] + target_unit2pop[:no]
        den = torch.where(den == 0, torch.ones_like(den), den)
        a_s = (source_unit2pop[:no] / den).unsqueeze(1)
        bench[:no] = a_s * tgt[:no] + (1 - a_s) * src
        if total_num_units > no:
            rest = tgt[no:].contiguous()
            sim, index = F_.fullsort_topk(rest, src, None, k=self.k, exclude_first_col=False)        # [units, k] each
            sn = source_unit2pop[index].mean(dim=1)
            beta = (sn / (sn + target_unit2pop[no:])).unsqueeze(1)
            sim_e = torch.bmm(sim.unsqueeze(1), src[index]).squeeze(1)                                 # [units, D]
            sum_sim = sim.sum(dim=1, keepdim=True)
            sum_sim = torch.where(sum_sim > 0, sum_sim, torch.ones_like(sum_sim))
            bench[no:] = (1 - beta) * rest + beta * (sim_e / sum_sim)
        self.benchmark_embedding = bench

    def build_benchmark_embedding(self):
        if self.mode == 'overlap_users':
            self.build_unit_benchmark_embedding(self.total_num_users, self.overlapped_num_users, self.source_user2pop,
                                                self.target_user2pop,
                                                self.source_user_embedding.weight[:self.overlapped_num_users],
                                                self.target_user_embedding.weight)
        elif self.mode == 'overlap_items':
            self.build_unit_benchmark_embedding(self.total_num_items, self.overlapped_num_items, self.source_item2pop,
                                                self.target_item2pop,
                                                self.source_item_embedding.weight[:self.overlapped_num_items],
                                                self.target_item_embedding.weight)

    def maxmin_normalize(self, embed_weight):
        y, stats = F_.MaxMinNormalize.apply(embed_weight)
        return y, stats[:, :1], stats[:, 1:]

    def calculate_rec_loss(self, interaction, user_embeds, item_embeds, user_field, item_field, neg_item_field, label_field):
        return F_.BPRGatherLoss.apply(user_embeds, item_embeds, interaction[user_field], interaction[item_field],
                                      interaction[neg_item_field], 1e-10, 0.0).reshape(())

    def calculate_unit_map_loss(self, target_num_units, target_unit_embeddings):
        sampled_index = np.random.randint(0, target_num_units, self.map_batch_size)        # host draw, as the reference (:175)
        idx = torch.from_numpy(sampled_index).to(target_unit_embeddings.device)
        e, _, _ = self.maxmin_normalize(F_.gather_rows(target_unit_embeddings, idx))
        mapped = self.mapping_mlp_layers(e)
        with torch.no_grad():
            b, _, _ = self.maxmin_normalize(F_.gather_rows(self.benchmark_embedding, idx))
        return F_.mse_loss(mapped, b)

    def calculate_map_loss(self):
        if self.mode == 'overlap_users':
            return self.calculate_unit_map_loss(self.target_num_users, self.target_user_embedding.weight)
        elif self.mode == 'overlap_items':
            return self.calculate_unit_map_loss(self.target_num_items, self.target_item_embedding.weight)
        return None

    def _tables(self):
        """(user table, item table, domain tag) of the current phase -- the branch table shared by calculate_loss :192-213,
        full_sort_predict :215-245 and predict :247-280."""
        first = self.phase2count.get(self.phase, 0) == 1
        if self.phase == 'SOURCE' and first:
            return self.source_user_embedding.weight, self.source_item_embedding.weight, 'SOURCE'
        if self.phase == 'TARGET' and first:
            return self.target_user_embedding.weight, self.target_item_embedding.weight, 'TARGET'
        if self.mode == 'overlap_users':
            return self.affine_embedding, self.target_item_embedding.weight, 'TARGET'
        return self.target_user_embedding.weight, self.affine_embedding, 'TARGET'

    def graph_key(self):
        # BOTH: the map loss draws its rows with numpy on the host (:175 of the reference) -- not capturable.  The other phases read
        # tables that depend on how often the phase has been visited (affine_embedding is rebuilt on the second TARGET visit).
        return None if self.phase == 'BOTH' else ('DCDCSR', self.phase, self.phase2count.get(self.phase, 0))

    def calculate_loss(self, interaction):
        count = self.phase2count.get(self.phase, 0)
        if self.phase == 'BOTH':
            return self.calculate_map_loss()
        if (self.phase == 'SOURCE' and count == 1) or (self.phase == 'TARGET' and count in (1, 2)):
            U, I, tag = self._tables()
            return self.calculate_rec_loss(interaction, U, I, getattr(self, f'{tag}_USER_ID'), getattr(self, f'{tag}_ITEM_ID'),
                                           getattr(self, f'{tag}_NEG_ITEM_ID'), getattr(self, f'{tag}_LABEL'))
        return None

    # ---- O(batch) training step (large tables) ------------------------------------------------------------------
    def _mlp_pairs(self):
        """[(weight, bias)] of the mapping MLP's linear layers, first layer first."""
        return [(m.weight, m.bias) for m in self.mapping_mlp_layers.mlp_layers if isinstance(m, nn.Linear)]

    def _triple_fields(self, interaction, tag):
        fields = [getattr(self, f'{tag}_{f}') for f in ('USER_ID', 'ITEM_ID', 'NEG_ITEM_ID')]
        missing = [f for f in fields if f not in interaction]
        if missing:
            raise ValueError(f'DCDCSR.fused_train_step trains the {self.phase} phase on {tag} triples; the batch has no {", ".join(missing)}')
        uid, pid, nid = (interaction[f].reshape(-1).contiguous() for f in fields)
        if uid.numel() == 0 or pid.numel() != uid.numel() or nid.numel() != uid.numel():
            raise ValueError(f'DCDCSR.fused_train_step: the {self.phase} batch needs at least one triple and id lists of equal length, got '
                             f'{uid.numel()} / {pid.numel()} / {nid.numel()} entries')
        return uid, pid, nid

    def fused_train_step(self, interaction, opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adam='lazy'):
        """``calculate_loss -> backward -> optimizer.step`` of the current (phase, visit) without table-sized gradients or a dense optimizer
        sweep over the tables: what ``DCDCSRTrainer`` runs when ``config['optimizer_mode'] == 'rowwise'``.  Same loss and gradients as
        ``calculate_loss``:

        * first SOURCE / TARGET visit: the fused BPR step of the domain's two tables (fused.FusedBPRStep / KMajorBPRStep by the batch
          layout, reg_weight 0, gamma 1e-10);
        * BOTH: ``map_batch_size`` unit ids drawn with ONE ``np.random.randint`` per step exactly as ``calculate_unit_map_loss`` draws them
          (the dense and the row-wise mode consume the same numpy stream), then fused.FusedDCDCSRMapStep on the live benchmark table: the
          target table of the overlapped unit kind row-wise, the mapping MLP by the exact dense Adam;
        * second TARGET visit: fused.FusedFrozenSideBPRStep with the affine table on the overlapped side; only the other side's table trains.

        One optimizer state per table, shared by the phases (the reference has one ``torch.optim.Adam`` over every parameter).  Returns the
        loss (device scalar or [1]).  ``adam='lazy'`` (default): table rows a step does not name do not move.  ``adam='exact'``: the
        reference's dense Adam -- one catch-up launch in front of every step (fused.rowwise_catch_up); the tables hold what
        ``torch.optim.Adam`` over whole tables would have left once ``fused_sync()`` has run, which ``set_phase`` does before it reads them.
        One mode per model.  Every phase runs eagerly: there is no ``fused_graph_key`` (BOTH draws on the host; replaying the BPR phases
        is left for later).

        Refused before any state is created: ``adam`` other than 'lazy' / 'exact', ``adam='exact'`` with SGD, a second Adam mode
        (ValueError); ``config['dist_group']`` (NotImplementedError); an embedding_size the fused BPR step does not take, MLP widths outside
        ``FusedDCDCSRMapStep.check_widths`` (ValueError, use optimizer_mode=dense); a batch without the phase's triple fields, empty or
        unequal-length id lists, and a (phase, visit) pair ``calculate_loss`` has no loss for (ValueError)."""
        from ...fused import FusedDCDCSRMapStep, FusedFrozenSideBPRStep, rowwise_catch_up
        exact, code, hp = self._fused_args(opt, adam, lr, betas, eps, weight_decay)
        self._fused_refuse_dist('DCDCSR')
        D = self.embedding_size
        if D % 4 != 0 or D > 256:
            raise ValueError(f'DCDCSR.fused_train_step needs embedding_size % 4 == 0 and embedding_size <= 256 (one float4 per lane, '
                             f'at most 64 lanes per row), got {D}; use optimizer_mode=dense')
        dims = [D] + [int(h) for h in self.mlp_hidden_size] + [D]
        self._fused_check_widths('DCDCSR', FusedDCDCSRMapStep.check_widths, 'mapping MLP widths {}', dims)
        count = self.phase2count.get(self.phase, 0)
        unit = self._unit()

        def catch_up(st, ids):
            if exact:
                rowwise_catch_up([(st, ids)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)

        if self.phase == 'BOTH':
            n = int(self.map_batch_size)
            if n < 1 or self.benchmark_embedding is None:
                raise ValueError(f'DCDCSR.fused_train_step: the BOTH phase needs map_batch_size >= 1 (got {n}) and the benchmark table '
                                 f"set_phase('BOTH') builds")
            name = f'target_{unit}_embedding'
            old = self._fused_cache(exact)['steps'].get('map')
            st = self._fused_state(name, code, exact)

            step = self._fused_weight_step('map', lambda s: s.max_batch >= n, lambda: FusedDCDCSRMapStep(
                getattr(self, name).weight.data, self.benchmark_embedding, self._mlp_pairs(), n if old is None else max(n, old.max_batch),
                state=st, **hp), hp)
            sampled_index = np.random.randint(0, getattr(self, f'target_num_{unit}s'), n)        # host draw, as the reference (:175)
            idx = torch.from_numpy(sampled_index).to(st.table.device)
            catch_up(st, [idx])
            return step.step(idx, bench=self.benchmark_embedding)
        if self.phase in ('SOURCE', 'TARGET') and count == 1:
            uid, pid, nid = self._triple_fields(interaction, self.phase)
            self._fused_cache(exact)
            return self._fused_bpr_domain_step(self.phase.lower(), getattr(interaction, 'k_major', None), uid, pid, nid, 0.0, 1e-10, code,
                                               exact, hp)
        if self.phase == 'TARGET' and count == 2:
            uid, pid, nid = self._triple_fields(interaction, 'TARGET')
            if self.affine_embedding is None:
                raise ValueError("DCDCSR.fused_train_step: the second TARGET visit needs the affine table set_phase('TARGET') builds")
            trained = 'item' if unit == 'user' else 'user'
            self._fused_cache(exact)
            st = self._fused_state(f'target_{trained}_embedding', code, exact)
            affine, B = self.affine_embedding, uid.numel()
            old = self._fused['steps'].get('frozen')

            def build_frozen():
                U, I = (affine, st.table) if unit == 'user' else (st.table, affine)
                return FusedFrozenSideBPRStep(U, I, unit, B if old is None else max(B, old.max_batch), state=st, gamma=1e-10, **hp)

            step = self._fused_step('frozen', lambda s: s.max_batch >= B and s.hp == hp and (s.U if unit == 'user' else s.I) is affine,
                                    build_frozen)
            step.hp = hp
            catch_up(st, [pid, nid] if trained == 'item' else [uid])
            return step.step(uid, pid, nid)[0]
        raise ValueError(f'DCDCSR.fused_train_step: no loss for visit {count} of phase {self.phase!r} (calculate_loss returns None there): '
                         f'the phases are SOURCE, TARGET, BOTH, TARGET')

    def _fused_phase_step(self):
        if self.phase == 'BOTH':
            return self._fused['steps']['map']
        if self.phase == 'TARGET' and self.phase2count.get('TARGET', 0) == 2:
            return self._fused['steps']['frozen']
        return self._fused['steps'][('bpr', self.phase.lower())]

    _WEIGHT_STEP = 'map'                                              # (the mapping MLP's dense Adam state: the checkpoint's 'weights')

    _FULL_SORT_FLAT = False                                           # (``full_sort_predict`` returns [U, N]: dcdcsr.py:244 of the reference)

    @torch.no_grad()
    def _full_sort_operands(self, interaction):
        """(user_e, slab0, slab1) of the all-items contraction in its three table cases: what ``ContractionScoring`` derives
        ``full_sort_predict`` / ``full_sort_topk`` / ``full_sort_rank`` from."""
        U, I, tag = self._tables()
        user_e = F_.gather_rows(U, interaction[getattr(self, f'{tag}_USER_ID')])
        if tag == 'SOURCE':
            return user_e, I[:self.overlapped_num_items], I[self.target_num_items:]
        if I is self.affine_embedding:
            return user_e, I, None
        return user_e, I[:self.target_num_items], None

    # Sampled-candidate evaluation on the row-gather kernel: ``predict`` is the plain dot of the phase's two tables (dcdcsr.py:249-280 of the
    # reference), the operands of ``_full_sort_operands``.
    candidate_scores = ContractionScoring.candidate_scores_from_operands

    @torch.no_grad()
    def predict(self, interaction):
        U, I, tag = self._tables()
        user, item = interaction[getattr(self, f'{tag}_USER_ID')], interaction[getattr(self, f'{tag}_ITEM_ID')]
        zeros = torch.zeros(user.numel(), device=U.device, dtype=torch.float32)
        return F_.PointGatherLoss.apply(B_.CDR_LOSS_MSE, U.contiguous(), I.contiguous(), None, None, user, item, zeros, 0.0)[1]
