"""Abstract cross-domain recommender = the drop-in boundary (recbole_cdr/model/crossdomain_recommender.py:14-51).

Same constructor contract ``(config, dataset)``, same attribute names, same ``set_phase`` hook; the third-party
``recbole.model.abstract_recommender.AbstractRecommender`` surface the trainer relies on (``calculate_loss`` /
``predict`` / ``full_sort_predict`` / ``other_parameter`` / ``load_other_parameter``) is restated here because recbole
is not a dependency of this package.
"""
import numpy as np
import torch
import torch.nn as nn
from torch.nn.init import xavier_normal_, constant_

from ..utils import ModelType


def xavier_normal_initialization(module):
    """recbole.model.init.xavier_normal_initialization: Embedding / Linear weights ~ xavier normal, biases 0."""
    if isinstance(module, nn.Embedding):
        xavier_normal_(module.weight.data)
    elif isinstance(module, nn.Linear):
        xavier_normal_(module.weight.data)
        if module.bias is not None:
            constant_(module.bias.data, 0)


class CrossDomainRecommender(nn.Module):
    type = ModelType.CROSSDOMAIN

    def __init__(self, config, dataset):
        super().__init__()
        # Per domain d in {source, target}: <D>_USER_ID / <D>_ITEM_ID / <D>_NEG_ITEM_ID field names and
        # <d>_num_users / <d>_num_items (overlap + that domain's own ids; the tables themselves are union-sized).
        for dom in ('source', 'target'):
            single = getattr(dataset, dom + '_domain_dataset')
            tag = dom.upper()
            uid, iid = single.uid_field, single.iid_field
            setattr(self, tag + '_USER_ID', uid)
            setattr(self, tag + '_ITEM_ID', iid)
            setattr(self, tag + '_NEG_ITEM_ID', config[dom + '_domain']['NEG_PREFIX'] + iid)
            setattr(self, dom + '_num_users', single.num(uid))
            setattr(self, dom + '_num_items', single.num(iid))
        # Union id space: [0] = PAD, [1, overlapped) shared, then target-only, then source-only ids.
        self.total_num_users, self.total_num_items = dataset.num_total_user, dataset.num_total_item
        self.overlapped_num_users, self.overlapped_num_items = dataset.num_overlap_user, dataset.num_overlap_item
        self.OVERLAP_ID = dataset.overlap_id_field
        self.device = config['device']

    def one_sided_overlap_mode(self):
        """'overlap_users' | 'overlap_items' | 'non_overlap' for the models that need the domains to share EITHER users OR items
        (emcdr.py:33-40 and the same guard in conet / sscdr / natr / deepapf / dcdcsr).  An overlap count of 1 is the PAD id alone."""
        nu, ni = self.overlapped_num_users, self.overlapped_num_items
        if nu > 1 and ni > 1:
            raise AssertionError(f'{type(self).__name__} handles a user-overlapped or an item-overlapped pair of domains, not both '
                                 f'({nu - 1} shared users and {ni - 1} shared items in this dataset)')
        return 'overlap_users' if nu > 1 else 'overlap_items' if ni > 1 else 'non_overlap'

    def set_phase(self, phase):
        pass

    def graph_key(self):
        """Hashable tag of what ``calculate_loss`` would enqueue right now, or None when the step must not be captured in a hipGraph
        (``Trainer`` replays one captured step per batch shape and key: graph_step.GraphedTrainStep).  A model answers with a key
        only when its loss does ALL per-step work on the device -- a host draw, a host counter or a tensor rebuilt per phase visit
        would be frozen into the capture.  Default: not capturable (the eager loop)."""
        return None

    def on_train_steps(self):
        """Called by ``Trainer`` after training steps that ran WITHOUT the model's Python (hipGraph replays): the place to drop
        anything ``calculate_loss`` would have invalidated on the host -- e.g. BiTGCF's cached propagated embeddings
        (bitgcf.py:146-148 of the reference clears them at the top of every ``calculate_loss``).  Default: nothing cached."""

    def calculate_loss(self, interaction):
        raise NotImplementedError

    def predict(self, interaction):
        raise NotImplementedError

    def full_sort_predict(self, interaction):
        raise NotImplementedError

    # [U, N] floats one ``rank_rows`` pass may hold when the scores are not a contraction (64 M = 256 MB: the staging of the native passes)
    RANK_ROWS_MAX_SCORES = 64 << 20

    def _score_chunks(self, interaction, predict_fallback):
        """Yields ``(s, e, scores [e - s, N])`` over blocks of users that tile [0, len(interaction)) in order: ``full_sort_predict`` --
        ``predict_fallback(part, e - s)`` where that raises NotImplementedError -- of all users at once first, and of chunks of at most
        ``RANK_ROWS_MAX_SCORES`` scores when that first block turns out too tall."""
        n_user = len(interaction)
        step = None
        s = 0
        while s < n_user:
            e = n_user if step is None else min(s + step, n_user)
            part = interaction if (s, e) == (0, n_user) else interaction[s:e]
            try:
                scores = self.full_sort_predict(part).view(e - s, -1)
            except NotImplementedError:
                if predict_fallback is None:
                    raise
                scores = predict_fallback(part, e - s)
            if step is None and n_user * scores.shape[1] > self.RANK_ROWS_MAX_SCORES and n_user > 1:
                step = max(self.RANK_ROWS_MAX_SCORES // scores.shape[1], 1)      # (this first block was too tall: redo it in chunks)
                continue
            yield s, e, scores
            s = e

    @torch.no_grad()
    def full_sort_rank(self, interaction, pos_indptr, pos_cols, hist_indptr=None, hist_cols=None, predict_fallback=None):
        """``(pos_score [P], gt, eq, eq_before [P] int32, n_unmasked [U] int32)`` of the ground-truth positives (a CSR over the
        interaction's users, ascending distinct columns) over ``full_sort_predict`` after the evaluation mask (column 0 and the per-user
        history CSR): the contract of ``functional.fullsort_rank``; what ``Trainer.evaluate`` derives any ``topk``, MAP and GAUC from.
        A model whose score is a contraction never forms the [U, N] matrix (``contraction.ContractionScoring.full_sort_rank``); this
        default scores chunks of users with ``full_sort_predict`` -- ``predict_fallback(interaction, n_user)`` where that raises
        NotImplementedError -- and counts with ``functional.rank_rows``."""
        from .. import functional as F_
        self._one_gpu_only('full_sort_rank')
        n_user = len(interaction)
        dev = pos_cols.device
        P = pos_cols.numel()
        score = torch.empty(P, device=dev, dtype=torch.float32)
        out = tuple(torch.empty(n, device=dev, dtype=torch.int32) for n in (P, P, P, n_user))
        counts = (pos_indptr[1:] - pos_indptr[:-1])
        for s, e, scores in self._score_chunks(interaction, predict_fallback):
            scores = scores.float().contiguous()
            p0, p1 = (int(pos_indptr[s]), int(pos_indptr[e])) if (s, e) != (0, n_user) else (0, P)
            rows = torch.repeat_interleave(torch.arange(e - s, device=dev), counts[s:e])
            score[p0:p1] = scores[rows, pos_cols[p0:p1]]
            F_.rank_rows(scores, pos_indptr[s:e + 1].contiguous(), pos_cols, hist_indptr[s:e + 1].contiguous() if hist_indptr is not None
                         else None, hist_cols, pos_score=score, out=(out[0], out[1], out[2], out[3][s:e]))
        return (score,) + out

    @torch.no_grad()
    def full_sort_topk_wide(self, interaction, k, hist_indptr=None, hist_cols=None, predict_fallback=None):
        """``(values [U,k] float32, columns [U,k] int64)`` for lists beyond the fused kernels' 64 entries (``1 <= k <=
        functional.WIDE_TOPK_MAX``): per user the first k unmasked columns of ``full_sort_predict`` after the evaluation mask (column 0 and
        the per-user history CSR) in the order score descending, then column ascending; (-inf, -1) pads a short row -- the contract of
        ``functional.fullsort_topk_wide``, and the tie rule of ``full_sort_rank``.  A model whose score is a contraction never forms the
        [U, N] matrix (``contraction.ContractionScoring.full_sort_topk_wide``); this default scores chunks of users with
        ``full_sort_predict`` -- ``predict_fallback(interaction, n_user)`` where that raises NotImplementedError -- of at most
        ``RANK_ROWS_MAX_SCORES`` scores and selects with ``functional.topk_rows``."""
        from .. import functional as F_
        self._one_gpu_only('full_sort_topk_wide')
        n_user = len(interaction)
        vals = idx = None
        for s, e, scores in self._score_chunks(interaction, predict_fallback):
            if vals is None:
                vals, idx = F_._wide_outputs(scores.device, n_user, int(k))
            F_.topk_rows(scores.float().contiguous(), k, hist_indptr[s:e + 1].contiguous() if hist_indptr is not None else None, hist_cols,
                         out=(vals[s:e], idx[s:e]))
        return vals, idx

    def _one_gpu_only(self, what):
        if self.__dict__.get('_dist_cfg') not in (None, False):
            raise NotImplementedError(f"{type(self).__name__}.{what} does not shard its tables: config['dist_group'] is not "
                                      f"supported (one GPU)")

    def _candidate_guard(self):
        CrossDomainRecommender._one_gpu_only(self, 'candidate_scores')

    @torch.no_grad()
    def candidate_scores(self, interaction, cand_indptr, cand_cols, chunk=4096):
        """Scores [C] of a ragged candidate list -- the users of ``interaction`` [U] against the columns
        ``cand_cols[cand_indptr[u]:cand_indptr[u+1]]`` -- as ``predict`` gives them: sampled-candidate evaluation (eval_args mode uniN /
        popN) ranks ``predict``'s values, as recbole's ``Trainer._neg_sample_batch_eval`` does.  This is the definition of the route and
        works for every model: the list is expanded to (user, item) pairs and ``predict`` runs in chunks of ``chunk`` pairs (the way
        ``Trainer._predict_all_pairs`` chunks).  The columns are those of ``full_sort_predict`` in the model's phase: target item ids, and
        in a SOURCE phase the source loader's revoked columns (ids from ``overlapped_num_items`` on shifted down by the target-only count).
        A model whose ``predict`` is the same function of ``_full_sort_operands`` as ``functional.candidate_scores`` computes overrides this
        with ``contraction.ContractionScoring.candidate_scores_from_operands``."""
        self._candidate_guard()
        C = cand_cols.numel()
        dev = cand_cols.device
        if C == 0:
            return torch.empty(0, device=dev, dtype=torch.float32)
        cand_row = torch.repeat_interleave(torch.arange(len(interaction), device=dev), cand_indptr[1:] - cand_indptr[:-1], output_size=C)
        pairs = interaction.index_select(cand_row)
        if getattr(self, 'phase', None) == 'SOURCE':
            OI, TI = self.overlapped_num_items, self.target_num_items
            pairs.update({self.SOURCE_ITEM_ID: torch.where(cand_cols < OI, cand_cols, cand_cols + (TI - OI))})
        else:
            pairs.update({self.TARGET_ITEM_ID: cand_cols})
        step = max(int(chunk), 1)
        return torch.cat([self.predict(pairs[s:s + step]).reshape(-1) for s in range(0, C, step)]).float()

    def other_parameter(self):
        if hasattr(self, 'other_parameter_name'):
            return {key: getattr(self, key) for key in self.other_parameter_name}
        return dict()

    def load_other_parameter(self, para):
        if para is None:
            return
        for key, value in para.items():
            setattr(self, key, value)

    def __str__(self):
        params = sum(int(np.prod(p.size())) for p in self.parameters() if p.requires_grad)
        return super().__str__() + f'\nTrainable parameters: {params}'
