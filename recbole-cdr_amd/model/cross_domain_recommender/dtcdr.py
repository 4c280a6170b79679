"""DTCDR on libcdrhip -- same class contract as recbole_cdr/model/cross_domain_recommender/dtcdr.py:23-211, base_model = NeuMF
(the configured default, properties/model/DTCDR.yaml).

NeuMF tower (dtcdr.py:112-126): maximum of the two domains' user rows and of their item rows, written side by side into one
[B, 2D] operand by one gather kernel each (cdr_gather_max2; torch.maximum's tie-splitting backward), recbole ``MLPLayers``
(Dropout -> Linear -> ReLU per layer) on the fp32-MFMA contraction with bias + ReLU in the epilogue, predict layer + sigmoid in
the same kernel, BCE natively.  Dropout: identity in eval; in training the native counter-based mask (functional._dropout) --
not bit-comparable with torch's Philox stream, golden parity is pinned at dropout_prob = 0.
``base_model = 'DMF'`` (dtcdr.py:128-180) is NOT provided: the reference's DMF path indexes the source history with the wrong
batch (``source_history_user_value[user]`` for an item matrix, :156-160), shifts source-only ids with ``>`` instead of ``>=``
(:131,151: id == target_num_items lands outside the [B, source_num_items] matrix whenever target-only >= source-only ids) and
scores the target batch with the source tower (:194); it cannot run on an id space with target-only ids and has no oracle.

``fused_train_step`` (``optimizer_mode='rowwise'``): the BOTH-phase step without table-sized gradients -- fused.FusedDTCDRStep, the four
tables updated row-wise from csrc/cdr_dtcdr.hip's compact gradient rows (each table advances once per step, from both batches), the 12
tower parameters by the exact dense Adam; ``adam='exact'`` puts the catch-up of the reference's dense Adam in front of it
(fused.rowwise_catch_up over the four tables).  Same masks as ``calculate_loss`` under the same seed."""
import torch
import torch.nn as nn

from ... import binding as B_
from ... import functional as F_
from ...utils import InputType
from ..crossdomain_recommender import CrossDomainRecommender, xavier_normal_initialization
from ..rowwise import RowwiseTraining


class MLPLayers(nn.Module):
    """recbole.model.layers.MLPLayers(layers, dropout) with the default ReLU: parameter names ``mlp_layers.<3i+1>.*``."""

    def __init__(self, layers, dropout=0.0):
        super().__init__()
        self.dropout = float(dropout)
        mods = []
        for d_in, d_out in zip(layers[:-1], layers[1:]):
            mods += [nn.Dropout(p=dropout), nn.Linear(d_in, d_out), nn.ReLU()]
        self.mlp_layers = nn.Sequential(*mods)
        self.logger = None

    def forward(self, x, seed=None, salt=0):
        """``seed``: device int64 [1] counter of the step's dropout masks (None: no dropout); layer n uses stream ``salt + n``."""
        n = 0
        for m in self.mlp_layers:
            if isinstance(m, nn.Linear):
                if seed is not None and self.training and self.dropout > 0:
                    x = _Dropout.apply(x, self.dropout, seed, salt + n)
                x = F_.linear(x, m.weight, m.bias, B_.ACT_RELU)
                n += 1
        return x


class _Dropout(torch.autograd.Function):
    """x * mask / (1 - p) with the native counter-based mask (cdr_dropout_dev: the seed is read from device memory, so a captured
    step draws a fresh mask on every replay); the backward re-applies the same mask."""

    @staticmethod
    def forward(ctx, x, p, seed, salt):
        y = x.contiguous().clone()
        F_._dropout(y, y.numel(), p, seed, salt)
        ctx.p, ctx.seed, ctx.salt = p, seed, salt
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().clone()
        F_._dropout(g, g.numel(), ctx.p, ctx.seed, ctx.salt)
        return g, None, None, None


class DTCDR(RowwiseTraining, CrossDomainRecommender):
    input_type = InputType.POINTWISE

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.SOURCE_LABEL = dataset.source_domain_dataset.label_field
        self.TARGET_LABEL = dataset.target_domain_dataset.label_field
        self.embedding_size = config['embedding_size']
        self.mlp_hidden_size = list(config['mlp_hidden_size'])
        self.dropout_prob = config['dropout_prob']
        self.base_model = config['base_model']
        self.alpha = config['alpha']
        assert self.base_model in ['NeuMF', 'DMF'], f'DTCDR base_model must be NeuMF or DMF, got {self.base_model!r}'
        if self.base_model != 'NeuMF':
            raise NotImplementedError("DTCDR base_model 'DMF' is not provided by this build (see the module docstring)")

        self.source_user_embedding = nn.Embedding(self.total_num_users, self.embedding_size)
        self.source_item_embedding = nn.Embedding(self.total_num_items, self.embedding_size)
        self.target_user_embedding = nn.Embedding(self.total_num_users, self.embedding_size)
        self.target_item_embedding = nn.Embedding(self.total_num_items, self.embedding_size)
        # the reference fills the rows a domain never sees with -inf here (dtcdr.py:54-59) and then re-initialises every
        # embedding (:107), so the fill has no effect; it is not repeated
        self.source_mlp_layers = MLPLayers([2 * self.embedding_size] + self.mlp_hidden_size, self.dropout_prob)
        self.source_predict_layer = nn.Linear(self.mlp_hidden_size[-1], 1)
        self.target_mlp_layers = MLPLayers([2 * self.embedding_size] + self.mlp_hidden_size, self.dropout_prob)
        self.target_predict_layer = nn.Linear(self.mlp_hidden_size[-1], 1)
        self.apply(xavier_normal_initialization)
        self.phase = 'BOTH'
        self.__dict__['_dist_cfg'] = config['dist_group'] if 'dist_group' in config else None

    def set_phase(self, phase):
        self.phase = phase

    def _drop_seed(self):
        """Device-resident seed of this step's dropout masks: re-drawn from torch's CPU generator when run eagerly, advanced by a
        captured kernel inside a hipGraph capture (a host draw would be baked into the graph: one mask for every replay)."""
        if not self.training or not self.dropout_prob:
            return None
        dev = self.source_user_embedding.weight.device
        st = self.__dict__.get('_drop_state')
        if st is None or st.device != dev:
            st = torch.zeros(1, device=dev, dtype=torch.int64)
            self.__dict__['_drop_state'] = st
        if torch.cuda.is_current_stream_capturing():
            B_.call('cdr_inc_i64', B_.stream(), B_.i64(st))
        else:
            st.fill_(int(torch.empty((), dtype=torch.int64).random_(0, 2 ** 62).item()))
        return st

    def neumf_forward(self, user, item, domain='source', seed=None):
        x = F_.GatherMaxConcat.apply(self.source_user_embedding.weight, self.target_user_embedding.weight,
                                     self.source_item_embedding.weight, self.target_item_embedding.weight, user, item)
        mlp = self.source_mlp_layers if domain == 'source' else self.target_mlp_layers
        head = self.source_predict_layer if domain == 'source' else self.target_predict_layer
        if seed is None:
            seed = self._drop_seed()
        return F_.linear(mlp(x, seed, 0 if domain == 'source' else 64), head.weight, head.bias, B_.ACT_SIGMOID).squeeze(-1)

    def graph_key(self):
        return ('DTCDR',)           # (dropout: a device-side seed the captured step advances itself, _dropout_args)

    def calculate_loss(self, interaction):
        seed = self._drop_seed()
        ps = self.neumf_forward(interaction[self.SOURCE_USER_ID], interaction[self.SOURCE_ITEM_ID], 'source', seed)
        pt = self.neumf_forward(interaction[self.TARGET_USER_ID], interaction[self.TARGET_ITEM_ID], 'target', seed)
        loss_s = F_.BCEProbLoss.apply(ps, interaction[self.SOURCE_LABEL])
        loss_t = F_.BCEProbLoss.apply(pt, interaction[self.TARGET_LABEL])
        return loss_s * self.alpha + loss_t * (1 - self.alpha)

    # ---- O(batch) training step (large tables) ------------------------------------------------------------------
    _TABLES = ('source_user_embedding', 'source_item_embedding', 'target_user_embedding', 'target_item_embedding')

    def _pair_fields(self, interaction):
        fields = (self.SOURCE_USER_ID, self.SOURCE_ITEM_ID, self.SOURCE_LABEL, self.TARGET_USER_ID, self.TARGET_ITEM_ID, self.TARGET_LABEL)
        missing = [f for f in fields if f not in interaction]
        if missing:
            raise ValueError(f'DTCDR.fused_train_step trains on BOTH-phase batches (source and target rows); the {self.phase} batch '
                             f'has no {", ".join(missing)}')
        return [interaction[f].reshape(-1) for f in fields]

    def _towers(self):
        """((W_0, b_0, ..., w_out, b_out) of the source tower, the same of the target): the 12 parameters at the default depth."""
        out = []
        for d in ('source', 'target'):
            lin = [m for m in getattr(self, f'{d}_mlp_layers').mlp_layers if isinstance(m, nn.Linear)] + [getattr(self, f'{d}_predict_layer')]
            out.append(tuple(p for m in lin for p in (m.weight, m.bias)))
        return tuple(out)

    def fused_train_step(self, interaction, opt='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adam='lazy'):
        """``calculate_loss -> backward -> optimizer.step`` on a BOTH-phase batch without table-sized gradients or a dense optimizer
        sweep over the four tables (fused.FusedDTCDRStep): what ``CrossDomainTrainer`` runs when ``config['optimizer_mode'] ==
        'rowwise'``.  Same loss, masks and gradients as ``calculate_loss`` (the dropout seed is ``_drop_seed()``, drawn once per step);
        each table advances once per step -- a row named by both batches gets one update from the sum of its contributions -- and the
        towers' parameters take the exact dense Adam (the reference has one ``torch.optim.Adam`` over every parameter).  Returns the total
        loss (device [1]).

        ``adam='lazy'`` (default): table rows the batch does not touch do not move.  ``adam='exact'``: the reference's dense Adam -- one
        catch-up launch in front of every step (fused.rowwise_catch_up) replays the gradient-free updates the step's rows missed; the
        tables hold what ``torch.optim.Adam`` over whole tables would have left once ``fused_sync()`` has run.  One mode per model.

        Refused before any state is created: a batch without the BOTH-phase fields, empty or unequal-length domain batches,
        ``config['dist_group']``, and widths outside ``FusedDTCDRStep.check_widths`` (use optimizer_mode=dense for those)."""
        from ...fused import FusedDTCDRStep, rowwise_catch_up
        self.unfreeze_eval()                                           # the step writes the tables in place: no evaluation cache outlives it
        exact, code, hp = self._fused_args(opt, adam, lr, betas, eps, weight_decay)
        self._fused_refuse_dist('DTCDR')
        self._fused_check_widths('DTCDR', FusedDTCDRStep.check_widths, 'embedding_size = {}, mlp_hidden_size = {}', self.embedding_size,
                                 self.mlp_hidden_size)
        su, si, ys, tu, ti, yt = self._pair_fields(interaction)
        Bs, Bt = self._fused_check_pair_batch('DTCDR', su, si, ys, tu, ti, yt)
        self._fused_cache(exact)
        states = tuple(self._fused_state(n, code, exact) for n in self._TABLES)
        ms, mt = self._fused_pair_sizes('dtcdr', Bs, Bt)
        step = self._fused_weight_step('dtcdr', lambda s: s.max_source >= Bs and s.max_target >= Bt, lambda: FusedDTCDRStep(
            *(getattr(self, n).weight.data for n in self._TABLES), self._towers(), ms, mt, self.alpha, dropout_prob=self.dropout_prob,
            states=states, **hp), hp)
        ys = ys if ys.dtype == torch.float32 else ys.float()
        yt = yt if yt.dtype == torch.float32 else yt.float()
        seed = self._drop_seed()                                       # None in eval mode or without dropout: p = 0
        if exact:
            # [su, tu] names the rows of both user tables, [si, ti] those of both item tables
            rowwise_catch_up([(st, ids) for st, ids in zip(states, ([su, tu], [si, ti], [su, tu], [si, ti]))], lr=lr, betas=betas, eps=eps,
                             weight_decay=weight_decay)
        return step.step(su.contiguous(), si.contiguous(), ys.contiguous(), tu.contiguous(), ti.contiguous(), yt.contiguous(), seed=seed)

    def _fused_phase_step(self):
        return self._fused['steps']['dtcdr']

    _WEIGHT_STEP = 'dtcdr'                                            # (the towers' dense Adam state: the checkpoint's 'weights')

    def fused_optimizer_state(self):
        """The shared state, plus the state of the dropout seed (the generator ``_drop_seed`` draws from and the device counter), so that
        a resumed run draws the masks the uninterrupted one would."""
        out = super().fused_optimizer_state()
        if out and self.dropout_prob:
            st = self.__dict__.get('_drop_state')
            out['dropout'] = {'rng': torch.get_rng_state(), 'counter': None if st is None else int(st.item())}
        return out

    def load_fused_optimizer_state(self, state, opt='adam', adam='lazy'):
        """The shared restore, then the dropout seed's."""
        super().load_fused_optimizer_state(state, opt=opt, adam=adam)
        if 'dropout' in state:
            torch.set_rng_state(state['dropout']['rng'].cpu())
            st = self.__dict__.get('_drop_state')
            if st is not None and state['dropout']['counter'] is not None:
                st.fill_(int(state['dropout']['counter']))

    @torch.no_grad()
    def predict(self, interaction):
        return self.neumf_forward(interaction[self.TARGET_USER_ID], interaction[self.TARGET_ITEM_ID], 'target')

    # ---- full-sort evaluation (the reference defines ``predict`` only; recbole's evaluation scores every pair through it) ------------
    # The target tower's first layer is separable over the [B, 2D] operand of dtcdr.py:112-125: with M_u = max of the two user rows and
    # M_i = max of the two item rows, W0 [M_u ; M_i] + b0 = (M_u W0[:, :D]^T + b0) + M_i W0[:, D:]^T =: Q[u] + P[i]; behind it ReLU layers and
    # a sigmoid unit -- the algebra of CoNet's evaluation tower, so the same kernels score it (csrc/cdr_conet_fullsort.hip).  Dropout is the
    # identity (eval mode, as in ``predict``).
    # P [N, h1] is cached only between ``freeze_for_eval()`` and ``unfreeze_eval()`` (CrossDomainTrainer.evaluate brackets its loop with the
    # pair: nothing trains in between); outside a bracket every call recomputes from the live parameters.
    def freeze_for_eval(self):
        self.__dict__.pop('_eval_P', None)
        self.__dict__['_eval_frozen'] = True
        return self

    def unfreeze_eval(self):
        self.__dict__.pop('_eval_frozen', None)
        self.__dict__.pop('_eval_P', None)
        return self

    def train(self, mode=True):
        if mode:
            self.unfreeze_eval()
        return super().train(mode)

    def on_train_steps(self):
        self.unfreeze_eval()

    def load_state_dict(self, *args, **kwargs):
        self.unfreeze_eval()
        return super().load_state_dict(*args, **kwargs)

    def __getstate__(self):
        # pickle / copy.deepcopy / torch.save(model): the cache is table-sized and cheap to rebuild
        st = dict(self.__dict__)
        for k in ('_eval_P', '_eval_frozen'):
            st.pop(k, None)
        return st

    def _fullsort_operands(self, uid):
        """(P [N, h1], Q [U, h1], tail linears, predict layer) of the target tower over every target item."""
        D = self.embedding_size
        lins = [m for m in self.target_mlp_layers.mlp_layers if isinstance(m, nn.Linear)]
        W0, b0 = lins[0].weight, lins[0].bias
        caching = (not self.training) and bool(self.__dict__.get('_eval_frozen', False))
        P = self.__dict__.get('_eval_P') if caching else None
        if P is None:
            N = self.target_num_items
            M_i = torch.maximum(self.source_item_embedding.weight[:N], self.target_item_embedding.weight[:N])
            P = F_.gemm(M_i, W0[:, D:], trans_b=True)
            if caching:
                self.__dict__['_eval_P'] = P
        uid = uid.reshape(-1)
        M_u = torch.maximum(F_.gather_rows(self.source_user_embedding.weight, uid), F_.gather_rows(self.target_user_embedding.weight, uid))
        Q = F_.gemm(M_u, W0[:, :D], trans_b=True, bias=b0)
        return P, Q, lins[1:], self.target_predict_layer

    def _fullsort_kernel_ok(self, tail):
        h1 = self.mlp_hidden_size[0]
        return bool(self.__dict__.get('fullsort_fused', True)) and len(tail) >= 1 and \
            F_.conet_fullsort_supported(h1, [l.weight.shape[0] for l in tail])

    @torch.no_grad()
    def full_sort_predict(self, interaction):
        """[U, N]: ``predict`` for every evaluated user against every target item, in one launch for towers the full-sort kernel takes;
        otherwise (a one-layer ``mlp_hidden_size`` has no tail layer; widths beyond the kernel's) one broadcast-add-ReLU pass and the
        remaining contractions per user."""
        P, Q, tail, head = self._fullsort_operands(interaction[self.TARGET_USER_ID])
        if self._fullsort_kernel_ok(tail):
            return F_.conet_fullsort(P, Q, [l.weight for l in tail], [l.bias for l in tail], head.weight, head.bias)
        rows = []
        for u in range(Q.shape[0]):
            h = F_.bcast_add_act(P, Q[u], B_.ACT_RELU)
            for lin in tail:
                h = F_.linear(h, lin.weight, lin.bias, B_.ACT_RELU)
            rows.append(F_.linear(h, head.weight, head.bias, B_.ACT_SIGMOID).view(1, -1))
        return torch.cat(rows, dim=0)

    @torch.no_grad()
    def full_sort_topk(self, interaction, k, hist_indptr=None, hist_cols=None):
        """(values [U,k], item ids [U,k]) of ``full_sort_predict`` after the evaluation mask (PAD column, per-user history CSR), without the
        [U, N] matrix where the kernel takes the tower and the catalogue has at least ``F_.TOWER_TOPK_MIN_ITEMS`` items (below it the unfused
        route measures faster; ``self.fullsort_topk_min_items`` overrides) -- values bit-equal to the unfused scores; mask + ``torch.topk``
        of ``full_sort_predict`` otherwise."""
        if k > F_.FUSED_TOPK_MAX:                # beyond the fused kernels' lists: the wide route, whatever the catalogue size
            return self.full_sort_topk_wide(interaction, k, hist_indptr, hist_cols)
        uid = interaction[self.TARGET_USER_ID]
        lins = [m for m in self.target_mlp_layers.mlp_layers if isinstance(m, nn.Linear)]
        if not self._fullsort_kernel_ok(lins[1:]) or \
                self.target_num_items < self.__dict__.get('fullsort_topk_min_items', F_.TOWER_TOPK_MIN_ITEMS):
            scores = self.full_sort_predict(interaction).view(uid.numel(), -1)
            return F_.masked_topk(scores, k, hist_indptr, hist_cols)
        P, Q, tail, head = self._fullsort_operands(uid)
        return F_.conet_fullsort_topk(P, Q, [l.weight for l in tail], [l.bias for l in tail], head.weight, head.bias, k,
                                      hist_indptr=hist_indptr, hist_cols=hist_cols)
