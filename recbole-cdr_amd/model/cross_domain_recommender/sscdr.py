"""SSCDR on libcdrhip -- same class contract as recbole_cdr/model/cross_domain_recommender/sscdr.py:23-259.

Metric-learning losses = row gather -> squared-norm "normalize" -> triplet margin, all native kernels with native
backward; the mapping is recbole's ``MLPLayers(..., 'tanh')`` (Linear + Tanh after EVERY layer, the last included --
SURVEY App. A) on the fp32 MFMA contraction; scoring is the -||u - i||^2 epilogue of the same contraction.
The semi-supervised (interacted, non-interacted) ids are drawn on the host from numpy's global RNG exactly as the
reference does inside its loss (sscdr.py:89-118) so that a seeded run samples the same ids -- or, with
``config['sscdr_device_sampler'] = True``, by a kernel over the device-resident interaction lists (``sample_device``: same
distribution and constraints, counter-based RNG, no host work inside the loss, so the OVERLAP step replays as a hipGraph).

``fused_train_step`` (``optimizer_mode='rowwise'``): every phase without table-sized gradients -- fused.FusedTripletStep on a domain's
pair of tables, fused.SSCDRMapStep on the three tables of the OVERLAP phase; ``adam='exact'`` puts the catch-up of the reference's dense
Adam in front of each (fused.rowwise_catch_up).

``full_sort_topk``: evaluation without the [U, N] distance matrix from ``F_.SQDIST_TOPK_MIN_ITEMS`` items on (the scoring kernel's distance
epilogue under the fused mask + top-k); ``freeze_for_eval()`` ... ``unfreeze_eval()`` keep the normalised item operand and its norms for the
length of an evaluation.
"""
import numpy as np
import torch
import torch.nn as nn

from ... import binding as B_
from ... import functional as F_
from ...utils import InputType
from ..contraction import ContractionScoring
from ..crossdomain_recommender import CrossDomainRecommender, xavier_normal_initialization
from ..rowwise import RowwiseTraining


class MLPLayers(nn.Module):
    """recbole.model.layers.MLPLayers restricted to what SSCDR uses (dropout=0, bn=False): parameter names match
    (``mlp_layers.<3i+1>.weight``) so reference checkpoints load."""

    def __init__(self, layers, activation='tanh'):
        super().__init__()
        mods = []
        for d_in, d_out in zip(layers[:-1], layers[1:]):
            mods += [nn.Dropout(p=0.0), nn.Linear(d_in, d_out), nn.Tanh()]
        self.mlp_layers = nn.Sequential(*mods)

    def forward(self, x):
        for m in self.mlp_layers:
            if isinstance(m, nn.Linear):
                x = F_.linear(x, m.weight, m.bias, B_.ACT_TANH)
        return x


class SSCDR(RowwiseTraining, ContractionScoring, CrossDomainRecommender):
    input_type = InputType.PAIRWISE

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.mode = self.one_sided_overlap_mode()
        self.phase = None
        self.embedding_size = config['embedding_size']
        self.lamda = config['lambda']
        self.margin = config['margin']
        self.mlp_hidden_size = list(config['mlp_hidden_size'])
        self.device_sampler = bool(config['sscdr_device_sampler']) if 'sscdr_device_sampler' in config else False
        self.fused_map = bool(config['sscdr_fused_map']) if 'sscdr_fused_map' in config else True    # (with the device sampler only)
        self.sampler_seed = int(config['seed']) if 'seed' in config else 2022
        self.mapping_layer = MLPLayers([self.embedding_size] + self.mlp_hidden_size + [self.embedding_size])
        if self.mode == 'overlap_users':
            self.user_interacted_items = self.build_interacted_items(dataset, mode='user')
        elif self.mode == 'overlap_items':
            self.item_interacted_users = self.build_interacted_items(dataset, mode='item')
        self.source_user_embedding = nn.Embedding(self.total_num_users, self.embedding_size)
        self.source_item_embedding = nn.Embedding(self.total_num_items, self.embedding_size)
        self.target_user_embedding = nn.Embedding(self.total_num_users, self.embedding_size)
        self.target_item_embedding = nn.Embedding(self.total_num_items, self.embedding_size)
        self.apply(xavier_normal_initialization)
        self.__dict__['_dist_cfg'] = config['dist_group'] if 'dist_group' in config else None

    def build_interacted_items(self, dataset, mode='user'):
        ds = dataset.source_domain_dataset
        uids = ds.inter_feat[ds.uid_field].cpu().numpy()
        iids = ds.inter_feat[ds.iid_field].cpu().numpy()
        if mode == 'user':
            out = [[] for _ in range(self.total_num_users)]
            for uid, iid in zip(uids, iids):
                out[uid].append(iid)
        else:
            out = [[] for _ in range(self.total_num_items)]
            for iid, uid in zip(iids, uids):
                out[iid].append(uid)
        return out

    def sample(self, ids, mode='user'):
        """Host-side, numpy global RNG, same draw order per id as sscdr.py:89-118 (and the same cache mutation).  The reference calls
        ``np.random.choice(<python list>, size=1)``: a list -> array conversion of the whole candidate list per draw (0.33 ms for 7 k
        candidates, 10 ms for a batch of 100 ids).  Legacy ``RandomState.choice`` without ``p`` draws ``randint(0, len(a), size)`` and
        indexes, so ``randint`` on a cached array consumes the global stream identically (golden-pinned: ``aux/sampled_pos|neg``)."""
        ids = ids.cpu().numpy()
        interacted = np.zeros_like(ids)
        non_interacted = np.zeros_like(ids)
        cache = self.__dict__.setdefault('_cand_cache', {})
        if mode not in cache:
            if mode == 'user':
                cand = list(range(self.overlapped_num_items)) + list(range(self.target_num_items, self.total_num_items))
            else:
                cand = list(range(self.overlapped_num_users)) + list(range(self.target_num_users, self.total_num_users))
            cache[mode] = np.asarray(cand)
        cand = cache[mode]
        lists = self.user_interacted_items if mode == 'user' else self.item_interacted_users
        n_cand = len(cand)
        for index, id_ in enumerate(ids):
            h = lists[id_]
            if len(h) == 0:
                h.append(0)
            c = cand[np.random.randint(0, n_cand, size=1)[0]]
            while c in h:
                c = cand[np.random.randint(0, n_cand, size=1)[0]]
            interacted[index] = h[np.random.randint(0, len(h), size=1)[0]]
            non_interacted[index] = c
        return torch.from_numpy(interacted).to(self.device), torch.from_numpy(non_interacted).to(self.device)

    def _device_lists(self, mode):
        """The interaction lists of ``build_interacted_items`` as a device CSR (entries ascending per id, repeats kept), the candidate
        ranges of sscdr.py:94-95,106-107 and the sampler's device state; built once, from the lists the constructor made."""
        cache = self.__dict__.setdefault('_dev_lists', {})
        if mode not in cache:
            lists = self.user_interacted_items if mode == 'user' else self.item_interacted_users
            lens = np.fromiter((len(h) for h in lists), dtype=np.int64, count=len(lists))
            flat = np.fromiter((x for h in lists for x in sorted(h)), dtype=np.int64, count=int(lens.sum()))
            indptr = np.zeros(len(lists) + 1, dtype=np.int64)
            np.cumsum(lens, out=indptr[1:])
            dev = self.source_user_embedding.weight.device
            if mode == 'user':
                rng = (0, self.overlapped_num_items, self.target_num_items, self.total_num_items)
            else:
                rng = (0, self.overlapped_num_users, self.target_num_users, self.total_num_users)
            cache[mode] = (torch.from_numpy(indptr).to(dev), torch.from_numpy(flat if flat.size else np.zeros(1, dtype=np.int64)).to(dev), rng,
                           torch.zeros(1, device=dev, dtype=torch.int64), torch.zeros(1, device=dev, dtype=torch.int32))
        return cache[mode]

    def sample_device(self, ids, mode='user'):
        """``sample`` on the device (csrc/cdr_sampler.hip: sscdr_pair_sample_kernel): same distribution -- interacted uniform over the
        id's interaction list (an empty list counts as [0]), non-interacted uniform over the candidates not in it -- but its own
        counter-based RNG stream (``config['seed']``, a device call counter), and the cached lists are not mutated."""
        indptr, indices, (lo0, hi0, lo1, hi1), calls, fail = self._device_lists(mode)
        ids = ids.reshape(-1).contiguous().to(torch.int64)
        n = ids.numel()
        pos = torch.empty(n, device=ids.device, dtype=torch.int64)
        neg = torch.empty(n, device=ids.device, dtype=torch.int64)
        B_.call('cdr_sscdr_pair_sample', B_.stream(), B_.i64(ids), n, lo0, hi0, lo1, hi1, B_.i64(indptr), B_.i64(indices),
                (self.sampler_seed * 0x9E3779B1) & 0xFFFFFFFFFFFFFFFF, B_.i64(calls), B_.i64(pos), B_.i64(neg), B_.raw(fail))
        if not self.__dict__.get('_bump_in_gather', False):      # (the fused map loss advances the counter in its gather launch)
            B_.call('cdr_inc_i64', B_.stream(), B_.i64(calls))
        return pos, neg

    embedding_normalize = staticmethod(F_.sqnorm_normalize)

    def _domain_loss(self, interaction, domain):
        U = getattr(self, f'{domain}_user_embedding').weight
        I = getattr(self, f'{domain}_item_embedding').weight
        pre = domain.upper()
        ue = F_.gather_rows(U, interaction[getattr(self, f'{pre}_USER_ID')])
        pe = F_.gather_rows(I, interaction[getattr(self, f'{pre}_ITEM_ID')])
        ne = F_.gather_rows(I, interaction[getattr(self, f'{pre}_NEG_ITEM_ID')])
        return F_.TripletMarginLoss.apply(F_.sqnorm_normalize(ue), F_.sqnorm_normalize(pe), F_.sqnorm_normalize(ne),
                                          self.margin)

    def calculate_source_loss(self, interaction):
        return self._domain_loss(interaction, 'source')

    def calculate_target_loss(self, interaction):
        return self._domain_loss(interaction, 'target')

    def calculate_map_loss(self, interaction):
        idx = interaction[self.OVERLAP_ID].squeeze(1)
        a, b = ('user', 'item') if self.mode == 'overlap_users' else ('item', 'user')
        if self.device_sampler and self.fused_map:
            # the same loss in 7 launches instead of 21 (and 11 instead of 45 backward): sampler, ONE gather of the four row sets, the
            # mapping once on the stacked [source ; interacted ; non-interacted] rows, ONE loss kernel that also leaves the gradients
            self.__dict__['_bump_in_gather'] = True
            try:
                pos, neg = self.sample_device(idx, mode=a)
            finally:
                self.__dict__['_bump_in_gather'] = False
            X3, tgt = F_.GatherMapRows.apply(getattr(self, f'source_{a}_embedding').weight, getattr(self, f'target_{a}_embedding').weight,
                                             getattr(self, f'source_{b}_embedding').weight, idx, pos, neg, self._device_lists(a)[3])
            total, _ = F_.SSCDRMapLoss.apply(self.mapping_layer(X3), tgt, self.margin, self.lamda)
            return total
        src = F_.gather_rows(getattr(self, f'source_{a}_embedding').weight, idx)
        tgt = F_.gather_rows(getattr(self, f'target_{a}_embedding').weight, idx)
        loss_s = F_.mse_loss(self.mapping_layer(src), tgt)
        pos, neg = self.sample_device(idx, mode=a) if self.device_sampler else self.sample(idx, mode=a)
        other = getattr(self, f'source_{b}_embedding').weight
        mp = self.mapping_layer(F_.gather_rows(other, pos))
        mn = self.mapping_layer(F_.gather_rows(other, neg))
        loss_u = F_.TripletMarginLoss.apply(F_.sqnorm_normalize(tgt), F_.sqnorm_normalize(mp), F_.sqnorm_normalize(mn),
                                            self.margin)
        return loss_s + self.lamda * loss_u

    def graph_key(self):
        # OVERLAP with the reference's numpy sampler: host draws inside the loss -- not capturable; the device sampler is
        if self.phase == 'OVERLAP' and not self.device_sampler:
            return None
        return ('SSCDR', self.phase, self.device_sampler and self.fused_map)

    def graph_state_tensors(self):
        """Device-side call counters of the in-loss sampler (a captured step's warm-up must put them back)."""
        return [v[3] for v in self.__dict__.get('_dev_lists', {}).values()]

    def calculate_loss(self, interaction):
        if self.phase == 'SOURCE':
            return self.calculate_source_loss(interaction)
        elif self.phase == 'OVERLAP':
            return self.calculate_map_loss(interaction)
        else:
            return self.calculate_target_loss(interaction)

    # ---- O(batch) training step (large tables) ------------------------------------------------------------------
    def fused_train_step(self, interaction, opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adam='lazy'):
        """``calculate_loss -> backward -> optimizer.step`` of the current phase without table-sized gradients or a dense optimizer
        sweep: what ``CrossDomainTrainer`` runs when ``config['optimizer_mode'] == 'rowwise'``.  SOURCE / TARGET / BOTH (the target step,
        as in ``calculate_loss``): fused.FusedTripletStep on the domain's user and item table.  OVERLAP: fused.SSCDRMapStep on
        source_a, target_a (the overlapped ids) and source_b (the semi-supervised ids, drawn ONCE per step by the sampler
        ``calculate_map_loss`` would use: the numpy stream / the device call counter advance as in dense mode); the mapping's own
        parameters take the exact dense Adam.  Same loss and per-row gradients as ``calculate_loss``; one optimizer state per table,
        shared by the phases.  Returns the loss (device tensor).

        ``adam='lazy'`` (default): rows the batch does not touch do not move.  ``adam='exact'``: the reference's dense Adam -- one
        catch-up launch in front of every step (fused.rowwise_catch_up) on the tables and ids that step touches; the tables hold what
        ``torch.optim.Adam`` over whole tables would have left once ``fused_sync()`` has run.  One mode per model."""
        from ...fused import FusedTripletStep, SSCDRMapStep, rowwise_catch_up
        exact, code, hp = self._fused_args(opt, adam, lr, betas, eps, weight_decay)
        if self.__dict__.get('_dist_cfg') not in (None, False):
            raise NotImplementedError("SSCDR.fused_train_step does not shard its tables: config['dist_group'] is not supported (one GPU)")
        D = self.embedding_size
        if D % 4 != 0 or D > 256:
            raise ValueError(f'SSCDR.fused_train_step needs embedding_size % 4 == 0 and embedding_size <= 256 (one float4 per lane, '
                             f'at most 64 lanes per row), got {D}; use optimizer_mode=dense')
        self._fused_cache(exact)

        def state(name):
            return self._fused_state(name, code, exact)

        def catch_up(*tables):
            if exact:
                rowwise_catch_up(tables, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)

        if self.phase == 'OVERLAP':
            a, b = ('user', 'item') if self.mode == 'overlap_users' else ('item', 'user')
            idx = interaction[self.OVERLAP_ID].reshape(-1)
            names = (f'source_{a}_embedding', f'target_{a}_embedding', f'source_{b}_embedding')

            def build_map_step():
                step = SSCDRMapStep(*(getattr(self, n).weight.data for n in names), self.mapping_layer, list(self.mapping_layer.parameters()),
                                    self.margin, self.lamda, source_a_state=state(names[0]), target_a_state=state(names[1]),
                                    source_b_state=state(names[2]), **hp)
                pending = self.__dict__.get('_pending_map_state', {}).pop(a, None)
                if pending is not None and step.map_opt is not None:
                    step.map_opt.load_state_dict(pending)
                return step

            step = self._fused_step(('map', a), lambda s: True, build_map_step)
            if idx.numel() == 0:                                 # (an empty batch is a no-op: nothing is drawn, no table advances)
                return step.step(idx, idx, idx)
            bump = None
            if self.device_sampler:
                # (as the fused dense path: the step's gather launch advances the sampler's call counter)
                self.__dict__['_bump_in_gather'] = True
                try:
                    pos, neg = self.sample_device(idx, mode=a)
                finally:
                    self.__dict__['_bump_in_gather'] = False
                bump = self._device_lists(a)[3]
            else:
                pos, neg = self.sample(idx, mode=a)
            catch_up((step.sa_state, [idx]), (step.ta_state, [idx]), (step.sb_state, [pos, neg]))
            return step.step(idx, pos, neg, bump=bump)
        domain = 'source' if self.phase == 'SOURCE' else 'target'
        pre = domain.upper()
        user = interaction[getattr(self, f'{pre}_USER_ID')].reshape(-1)
        item = interaction[getattr(self, f'{pre}_ITEM_ID')].reshape(-1)
        neg = interaction[getattr(self, f'{pre}_NEG_ITEM_ID')].reshape(-1)
        rows = user.numel()
        step = self._fused_step(('triplet', domain), lambda s: s.max_batch >= rows, lambda: FusedTripletStep(
            getattr(self, f'{domain}_user_embedding').weight.data, getattr(self, f'{domain}_item_embedding').weight.data, rows,
            margin=self.margin, user_state=state(f'{domain}_user_embedding'), item_state=state(f'{domain}_item_embedding'), **hp))
        catch_up((step.ustate, [user]), (step.istate, [item, neg]))
        return step.step(user, item, neg)[0]

    def fused_graph_key(self, interaction, adam='lazy', opt='adam'):
        """None for every phase: the steps read the host's update counts (and the OVERLAP step runs autograd), so the trainer launches
        them and never captures them in a hipGraph."""
        return None

    def _fused_phase_step(self):
        if self.phase == 'OVERLAP':
            return self._fused['steps'][('map', 'user' if self.mode == 'overlap_users' else 'item')]
        return self._fused['steps'][('triplet', 'source' if self.phase == 'SOURCE' else 'target')]

    def fused_optimizer_state(self):
        """The shared per-table state, plus the dense Adam state of the mapping and the device sampler's call counters (a resumed run
        draws the ids the uninterrupted one would)."""
        out = super().fused_optimizer_state()
        for key, step in self.__dict__.get('_fused', {}).get('steps', {}).items():
            if key[0] == 'map' and step.map_opt is not None:
                out.setdefault('mapping', {})[key[1]] = step.map_opt.state_dict()
        for mode, lists in self.__dict__.get('_dev_lists', {}).items():
            out.setdefault('sampler_calls', {})[mode] = int(lists[3])
        return out

    def load_fused_optimizer_state(self, state, opt='adam', adam='lazy'):
        """The shared per-table restore; the mapping's Adam state is handed to the OVERLAP step when it is built."""
        super().load_fused_optimizer_state(state, opt=opt, adam=adam)
        self._pending_map_state = dict(state.get('mapping', {}))
        for mode, calls in state.get('sampler_calls', {}).items():
            self._device_lists(mode)[3].fill_(int(calls))

    # ---- scoring --------------------------------------------------------------------------------------------------
    def _mapped_rows(self, kind, ids, n_overlap):
        src = F_.gather_rows(getattr(self, f'source_{kind}_embedding').weight, ids)
        return F_.select_mapped(self.mapping_layer(src), getattr(self, f'target_{kind}_embedding').weight, ids, n_overlap)

    @staticmethod
    def _neg_rowdist(a, b):
        """-sum((a-b)^2, 1) for explicit pairs: the triplet kernel's distance with eps=0, squared."""
        rows, D = a.shape
        out = torch.empty(1, device=a.device, dtype=torch.float32)
        dap = torch.empty(rows, device=a.device, dtype=torch.float32)
        dan = torch.empty(rows, device=a.device, dtype=torch.float32)
        a_, b_ = a.contiguous(), b.contiguous()
        B_.call('cdr_triplet_fwd', B_.ctx(a.device), B_.stream(), B_.f32(a_), B_.f32(b_), B_.f32(b_), rows, D, 0.0, 0.0,
                B_.f32(out), B_.f32(dap), B_.f32(dan))
        # d^2 with the sign flipped: one more native elementwise pass (mse-style) would only restate dap*dap
        return -(dap * dap)

    @torch.no_grad()
    def predict(self, interaction):
        if self.phase in ('SOURCE', 'TARGET'):
            d = self.phase.lower()
            ue = F_.sqnorm_normalize(F_.gather_rows(getattr(self, f'{d}_user_embedding').weight,
                                                    interaction[getattr(self, f'{self.phase}_USER_ID')]))
            ie = F_.sqnorm_normalize(F_.gather_rows(getattr(self, f'{d}_item_embedding').weight,
                                                    interaction[getattr(self, f'{self.phase}_ITEM_ID')]))
            return self._neg_rowdist(ue, ie)
        user, item = interaction[self.TARGET_USER_ID], interaction[self.TARGET_ITEM_ID]
        if self.mode == 'overlap_users':
            ue = self._mapped_rows('user', user, self.overlapped_num_users)
            ie = F_.gather_rows(self.target_item_embedding.weight, item)
        else:
            ue = F_.gather_rows(self.target_user_embedding.weight, user)
            ie = self._mapped_rows('item', item, self.overlapped_num_items)
        return self._neg_rowdist(F_.sqnorm_normalize(ue), F_.sqnorm_normalize(ie))

    # ---- full-sort evaluation ---------------------------------------------------------------------------------------------------
    # The item operand -- the phase's item rows, normalised -- does not depend on the evaluated users.  Between ``freeze_for_eval()`` and
    # ``unfreeze_eval()`` (CrossDomainTrainer.evaluate brackets its loop with the pair: nothing trains in between) it is kept, as ONE buffer,
    # with its squared row norms; outside a bracket every call recomputes from the live parameters, as the reference does (sscdr.py:228-259).
    def freeze_for_eval(self):
        self.__dict__.pop('_eval_items', None)
        self.__dict__['_eval_frozen'] = True
        return self

    def unfreeze_eval(self):
        self.__dict__.pop('_eval_frozen', None)
        self.__dict__.pop('_eval_items', None)
        return self

    def set_phase(self, phase):
        self.__dict__.pop('_eval_items', None)
        self.phase = phase

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
        for k in ('_eval_items', '_eval_frozen'):
            st.pop(k, None)
        return st

    def _item_slabs(self):
        """The normalised item rows the current phase scores against, as one or two row ranges (normalising is row-wise: the ranges of the
        reference's ``torch.cat`` can be normalised apart, and an empty range drops out)."""
        OI, TI = self.overlapped_num_items, self.target_num_items
        if self.phase == 'SOURCE':
            W = self.source_item_embedding.weight
            parts = [W[:OI], W[TI:]]
        elif self.phase == 'TARGET' or self.mode == 'overlap_users':
            parts = [self.target_item_embedding.weight[:TI]]
        else:
            parts = [self.mapping_layer(self.source_item_embedding.weight[:OI]), self.target_item_embedding.weight[OI:TI]]
        slabs = [F_.sqnorm_normalize(x) for x in parts if x.shape[0]]
        return slabs[0], (slabs[1] if len(slabs) > 1 else None)

    def _eval_item_cache(self):
        """Inside an evaluation bracket: {'items': the normalised item operand as one buffer, 'sqnorm': its squared row norms, formed when
        ``_rank_col_sqnorm`` first asks}.  None outside."""
        if self.training or not self.__dict__.get('_eval_frozen', False):
            return None
        cache = self.__dict__.get('_eval_items')
        if cache is None:
            s0, s1 = self._item_slabs()
            cache = self.__dict__['_eval_items'] = {'items': s0 if s1 is None else torch.cat([s0, s1], dim=0), 'sqnorm': None}
        return cache

    def _full_sort_users(self, interaction):
        if self.phase == 'SOURCE':
            ue = F_.gather_rows(self.source_user_embedding.weight, interaction[self.SOURCE_USER_ID])
        elif self.phase == 'TARGET' or self.mode != 'overlap_users':
            ue = F_.gather_rows(self.target_user_embedding.weight, interaction[self.TARGET_USER_ID])
        else:
            ue = self._mapped_rows('user', interaction[self.TARGET_USER_ID], self.overlapped_num_users)
        return F_.sqnorm_normalize(ue)

    def _full_sort_operands(self, interaction):
        """(user_e, slab0, slab1) of ``full_sort_predict``: the normalised user rows and the normalised item rows as one or two row ranges
        (``slab1`` None: one) -- all three phase cases, both modes.  Inside an evaluation bracket the item operand is the cached buffer."""
        cache = self._eval_item_cache()
        s0, s1 = (cache['items'], None) if cache is not None else self._item_slabs()
        return self._full_sort_users(interaction), s0, s1

    def _rank_distance_form(self):
        return True

    def _rank_col_sqnorm(self):
        """``full_sort_rank`` and ``full_sort_topk``: the column norms of the cached item operand, formed once per evaluation bracket by
        whichever asks first (None outside one)."""
        cache = self._eval_item_cache()
        if cache is None:
            return None
        if cache['sqnorm'] is None:
            cache['sqnorm'] = F_.row_sqnorm(cache['items'])
        return cache['sqnorm']

    # Sampled-candidate evaluation on the row-gather kernel in its distance form: ``predict`` is -sum (u - i)^2 over the normalised rows
    # (sscdr.py:127-128, 197-226 of the reference), the operands of ``_full_sort_operands`` (inside an evaluation bracket the cached
    # normalised item buffer; the mapping MLP runs once per user, not once per pair).
    candidate_scores = ContractionScoring.candidate_scores_from_operands

    @torch.no_grad()
    def full_sort_predict(self, interaction):
        ue, s0, s1 = self._full_sort_operands(interaction)
        return F_.fullsort_neg_sqdist(ue, s0 if s1 is None else torch.cat([s0, s1], dim=0)).view(-1)

    @torch.no_grad()
    def full_sort_topk(self, interaction, k, hist_indptr=None, hist_cols=None):
        """(values [U,k], item columns [U,k]) of ``full_sort_predict`` after the evaluation mask (PAD column, per-user history CSR).  From
        ``F_.SQDIST_TOPK_MIN_ITEMS`` items on (``self.fullsort_topk_min_items`` overrides) without the [U, N] matrix and without the cat of
        the item ranges: the scoring kernel's distance epilogue under the fused mask + top-k (F_.fullsort_neg_sqdist_topk; values bit-equal
        to the unfused scores).  Below it ``full_sort_predict`` + mask + ``torch.topk``."""
        if k > F_.FUSED_TOPK_MAX:                # beyond the fused kernels' lists: the wide route, whatever the catalogue size
            return self.full_sort_topk_wide(interaction, k, hist_indptr, hist_cols)
        OI, TI = self.overlapped_num_items, self.target_num_items
        N = OI + self.total_num_items - TI if self.phase == 'SOURCE' else TI
        if N < self.__dict__.get('fullsort_topk_min_items', F_.SQDIST_TOPK_MIN_ITEMS):
            uid = interaction[self.SOURCE_USER_ID if self.phase == 'SOURCE' else self.TARGET_USER_ID]
            return F_.masked_topk(self.full_sort_predict(interaction).view(uid.numel(), -1), k, hist_indptr, hist_cols)
        return F_.fullsort_neg_sqdist_topk(*self._scored_operands(interaction), k=k, hist_indptr=hist_indptr, hist_cols=hist_cols,
                                           col_sqnorm=self._rank_col_sqnorm())
