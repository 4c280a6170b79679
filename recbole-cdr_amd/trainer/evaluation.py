"""Evaluation: full-sort scores -> mask PAD column and history -> metrics, on the model's native routes.

``Evaluation(config, model)`` evaluates on its own (no optimizer is built); ``trainer.Trainer`` inherits it.  Three routes, one per-batch
function each, one accumulator and one finish: the list route (the model's mask + top-k lists, or torch.topk of the masked matrix), the
rank route (the rank of each positive over the masked catalogue: any k, MAP, GAUC) and the sampled-candidate route (eval_args mode uniN /
popN).  Metrics are computed on device in torch (plumbing).
"""
import numpy as np
import torch

from ..eval_config import (DEFAULT_METRICS, TOPK_METRICS, VALUE_METRICS, NON_ACCURACY_METRICS, FUSED_TOPK_MAX, WIDE_TOPK_MAX,  # noqa: F401
                           resolve_metrics, resolve_eval_mode, resolve_eval_route)


def metrics_from_hits(hit, n_pos, topk, names=DEFAULT_METRICS):
    """{name@k: value} from the hit matrix [U, kmax] (hit[u, j] = 1 where position j of user u's ranking is a ground-truth positive) and
    the positives per user ``n_pos`` [U] (clamped to >= 1 by the caller): recbole's Recall / Hit / Precision / MRR / NDCG / MAP, averaged
    over the users.  The one copy of this arithmetic: both evaluation routes end here."""
    kmax = hit.shape[1]
    result = {}
    ranks = torch.arange(1, kmax + 1, device=hit.device, dtype=torch.float32)
    for k in topk:
        h = hit[:, :k]
        for name in names:
            if name == 'recall':
                value = (h.sum(1) / n_pos).mean()
            elif name == 'hit':
                value = (h.sum(1) > 0).float().mean()
            elif name == 'precision':
                value = (h.sum(1) / k).mean()
            elif name == 'mrr':
                value = (h * (1.0 / ranks[:k])).max(1).values.mean()
            elif name == 'ndcg':
                dcg = (h / torch.log2(ranks[:k] + 1)).sum(1)
                ideal = torch.cumsum(1.0 / torch.log2(ranks[:k] + 1), 0)
                idcg = ideal[(n_pos.clamp(max=k).long() - 1)]
                value = (dcg / idcg).mean()
            elif name == 'map':
                # recbole MAP: the mean of precision@j over the hit positions j <= k, divided by min(n_pos, k)
                pre = torch.cumsum(h, 1) / ranks[:k]
                value = ((pre * h).sum(1) / n_pos.clamp(max=k)).mean()
            else:
                continue                                   # (gauc has no @k: gauc_from_counts)
            result[f'{name}@{k}'] = float(value)
    return result


def gauc_from_counts(pos_len, user_len, rank_sum):
    """recbole's GAUC in float64 from per-user integers: ``pos_len`` positives, ``user_len`` unmasked items (positives included),
    ``rank_sum`` = the sum of the positives' average ranks gt + (eq + 1) / 2 (descending order, 1 = best, ties share the mean position).
    pair = (user_len + 1) pos_len - pos_len (pos_len + 1) / 2 - rank_sum counts the (positive, negative) pairs in the right order, ties
    half; auc_u = pair / (neg pos_len); users without positives or without negatives are dropped; the mean is pos_len-weighted."""
    pos_len, user_len, rank_sum = pos_len.double(), user_len.double(), rank_sum.double()
    neg = user_len - pos_len
    keep = (pos_len > 0) & (neg > 0)
    if not bool(keep.any()):
        return float('nan')
    pos_len, neg, user_len, rank_sum = pos_len[keep], neg[keep], user_len[keep], rank_sum[keep]
    pair = (user_len + 1) * pos_len - pos_len * (pos_len + 1) / 2 - rank_sum
    return float((pair / (neg * pos_len) * pos_len).sum() / pos_len.sum())


def rank_counts_reference(scores, pos_rows, pos_cols):
    """The counts of ``functional.fullsort_rank`` in plain torch over a materialised, already masked matrix (masked entries NaN): what the
    trainer uses where there is no device to run the kernel on (``device: cpu``)."""
    valid = ~torch.isnan(scores)
    t = scores[pos_rows, pos_cols]
    rows, ok = scores[pos_rows], valid[pos_rows]
    col = torch.arange(scores.shape[1], device=scores.device).unsqueeze(0)
    gt = ((rows > t.unsqueeze(1)) & ok).sum(1)
    same = (rows == t.unsqueeze(1)) & ok
    eq, eqb = same.sum(1), (same & (col < pos_cols.unsqueeze(1))).sum(1)
    bad = torch.isnan(t)
    gt, eq, eqb = (torch.where(bad, torch.full_like(x, -1), x).to(torch.int32) for x in (gt, eq, eqb))
    return t, gt, eq, eqb, valid.sum(1).to(torch.int32)


class Evaluation:
    """``evaluate(eval_data)`` over ``config``, ``model``, ``device`` and the attributes ``_init_evaluation`` sets -- all it reads."""
    metrics = None                    # (class defaults: objects built without __init__ evaluate as before)
    list_metrics = ()
    eval_route = 'auto'

    def __init__(self, config, model):
        self.config, self.model = config, model
        self._init_evaluation(config)

    def _init_evaluation(self, config):
        self.topk = config['topk'] if 'topk' in config else [10]
        # config['metrics'] (absent: recall / hit / precision / mrr / ndcg, as always) and config['eval_route']: 'auto' keeps the model's
        # mask + top-k route whenever it can answer (no gauc, and max(topk) <= 64 or the route is unfused), 'rank' derives every metric
        # from the rank of each positive over the masked catalogue (model.full_sort_rank: any k, MAP, GAUC), 'topk' insists on the lists
        # (max(topk) <= 1024; above 64 on a GPU they come from model.full_sort_topk_wide)
        self.metrics = resolve_metrics(config)
        self.eval_route = resolve_eval_route(config, self.metrics)
        # config['eval_args']['mode'] (full | uniN | popN): which evaluation loader data.dataloader.eval_loader_for builds for the target
        # domain; evaluate() itself dispatches on the loader it is handed.  A mode that is not provided is refused here
        self.eval_mode = resolve_eval_mode(config)
        self.device = config['device']
        # the non-accuracy metrics among config['metrics'] (NON_ACCURACY_METRICS): what they cannot be combined with is refused here
        self.list_metrics = tuple(m for m in (self.metrics or ()) if m in NON_ACCURACY_METRICS)
        self.item_counts = None
        if self.list_metrics:
            self.item_counts = self._check_list_metrics(config)
        # evaluation through the model's fused mask + top-k kernel when it has one (False: full score matrix + torch.topk)
        self.fused_topk = config['fused_topk'] if 'fused_topk' in config else True

    def _fused_sync(self):
        """Called before anything is scored: a trainer brings row-wise optimizer state up to date here.  Alone there is none."""

    def _check_list_metrics(self, config):
        """The refusals of the non-accuracy metrics; returns config['item_counts'] as an int64 vector on the trainer's device."""
        what = f"metrics {', '.join(self.list_metrics)}"
        if self.eval_route == 'rank':
            raise ValueError(f"{what}: eval_route='rank' holds no list -- the rank of a positive does not say which items were recommended; "
                             f"use eval_route='auto' or 'topk'")
        if max(self.topk) > WIDE_TOPK_MAX:
            raise ValueError(f"{what}: the mask + top-k lists hold k <= {WIDE_TOPK_MAX}, topk asks for {max(self.topk)}")
        if self.eval_mode[0] != 'full':
            raise ValueError(f"{what}: eval_args mode {config['eval_args']['mode']!r} ranks the positives inside sampled candidate lists, "
                             f"whose positions are not recommendations over the catalogue; use mode 'full'")
        if 'dist_group' in config and config['dist_group'] not in (None, False):
            raise ValueError(f"{what}: not available with dist_group (the lists are counted on one GPU only, as on the rank route)")
        return self._as_item_counts(config['item_counts'])

    def _as_item_counts(self, counts):
        counts = torch.as_tensor(counts)
        if counts.dim() != 1 or counts.numel() == 0 or counts.dtype.is_floating_point or counts.dtype == torch.bool:
            raise ValueError("item_counts must be a non-empty 1-D integer tensor or array: the training-set count of every column of the "
                             "evaluated loader (data.train_item_counts)")
        return counts.to(device=self.device, dtype=torch.int64)

    def _list_stats_for(self, eval_data):
        """The ``functional.ListStats`` of one evaluate call when a non-accuracy metric is asked (None otherwise): the loader's own
        ``item_counts`` ahead of config['item_counts'], the tail set of config['tail_ratio'] when tailpercentage is asked."""
        if not self.list_metrics:
            return None
        from .. import functional as F_
        from ..data.popularity import tail_items
        own = getattr(eval_data, 'item_counts', None)
        counts = self._as_item_counts(own) if own is not None else self.item_counts
        tail = None
        if 'tailpercentage' in self.list_metrics:
            tail = tail_items(counts, self.config['tail_ratio'] if 'tail_ratio' in self.config else None)
        return F_.ListStats(counts, self.topk, tail_mask=tail)

    def _topk_lists(self, interaction, n_user, history_index, kmax, wide=False):
        """idx [U, kmax] of the model's fused mask + top-k (no [U, N] score matrix), pads -1: the history (rows, cols) pairs become a CSR
        with ascending columns.  ``wide``: the list comes from ``full_sort_topk_wide`` (kmax > 64; every model has it, those with
        ``predict`` only through ``_predict_all_pairs``)."""
        indptr, cols = self._history_csr(history_index, n_user, distinct=False)
        if wide:
            _vals, idx = self.model.full_sort_topk_wide(interaction, kmax, hist_indptr=indptr, hist_cols=cols,
                                                        predict_fallback=self._predict_all_pairs)
        else:
            _vals, idx = self.model.full_sort_topk(interaction, kmax, hist_indptr=indptr, hist_cols=cols)
        return idx

    def _topk_hits(self, interaction, n_user, history_index, positive_u, positive_i, kmax, wide=False, stats=None):
        """Hit matrix [U, kmax] and positives per user from ``_topk_lists``: positives are matched by sorted (user, item) keys.  The lists
        are handed on to ``stats`` (``functional.ListStats``): no second top-k call for the non-accuracy metrics."""
        dev = self.device
        N = int(self.model.target_num_items) if hasattr(self.model, 'target_num_items') else None
        idx = self._topk_lists(interaction, n_user, history_index, kmax, wide=wide)
        if stats is not None:
            stats.add(idx)
        pu = torch.as_tensor(positive_u, device=dev, dtype=torch.int64)
        pi = torch.as_tensor(positive_i, device=dev, dtype=torch.int64)
        span = max(int(idx.max()) + 1, int(pi.max()) + 1 if pi.numel() else 1, N or 1)
        pkey = torch.sort(pu * span + pi).values
        qkey = (torch.arange(n_user, device=dev).unsqueeze(1) * span + idx.clamp(min=0)).reshape(-1)
        at = torch.searchsorted(pkey, qkey).clamp(max=max(pkey.numel() - 1, 0))
        hit = (pkey[at] == qkey).view(n_user, kmax) & (idx >= 0) if pkey.numel() else torch.zeros_like(idx, dtype=torch.bool)
        return hit.float(), torch.bincount(pu, minlength=n_user).float()

    @torch.no_grad()
    def evaluate(self, eval_data):
        """eval_data yields (interaction, history_index (rows, cols) or None, positive_u, positive_i) like recbole's
        FullSortEvalDataLoader; returns {metric@k: value} for config['metrics'] (default recall / mrr / ndcg / hit / precision; also map, and
        gauc under the key 'gauc') at every k of config['topk'].  A loader whose ``eval_mode`` is 'sampled' (``NegSampleEvalLoader``, eval_args
        mode uniN / popN) yields (interaction, (cand_indptr, cand_cols), positive_u, positive_i) instead and every positive is ranked inside
        its user's candidate list (``_sampled_batch``)."""
        self._fused_sync()
        self.model.eval()
        kmax = max(self.topk)
        # dispatch per loader, on its own attribute: a (source full-sort, target sampled) pair of valid loaders evaluates each its way
        sampled = getattr(eval_data, 'eval_mode', 'full') == 'sampled'
        fused = self.fused_topk and hasattr(self.model, 'full_sort_topk') and not sampled
        if sampled and self.list_metrics:
            raise ValueError(f"evaluate: metrics {', '.join(self.list_metrics)} cannot be answered on a sampled-candidate loader (its lists "
                             f"are positions inside a sample); hand evaluate a full-sort loader")
        # recbole cuts the evaluated users so that the [U, N] score matrix fits eval_batch_size entries (ONE user per call over a 10 M-item
        # catalogue at the default 4,096).  The fused mask + top-k path never forms that matrix, so it re-cuts a loader that allows it
        # into throughput-sized batches (config['eval_users_per_batch'], default 1,024; 0 keeps recbole's cut): same users, same metrics
        want = int(self.config['eval_users_per_batch']) if 'eval_users_per_batch' in self.config else 1024
        restore = None
        if (fused or sampled) and want > 0 and hasattr(eval_data, 'rebatch') and getattr(eval_data, 'step', want) < want:
            restore = eval_data.step                      # (the caller's cut comes back afterwards: another consumer may need [U, N] to fit)
            eval_data.rebatch(want)
        # the model's evaluation-mode caches (CoNet: the item half of layer 1, the packed one-user call) live exactly as long as this loop:
        # nothing trains inside it
        frozen = hasattr(self.model, 'freeze_for_eval')
        if frozen:
            self.model.freeze_for_eval()
        try:
            return self._evaluate_batches(eval_data, sampled, fused, kmax)
        finally:
            if frozen:
                self.model.unfreeze_eval()
            if restore is not None:
                eval_data.rebatch(restore)

    def _predict_all_pairs(self, interaction, n_user):
        """[U, N] scores of a model that defines ``predict`` only (DeepAPF, NATR, as in the reference), the way recbole's
        ``Trainer._full_sort_batch_eval`` / ``_spilt_predict`` get them: every user row repeated ``target_num_items`` times, item ids
        0..N-1 attached, ``predict`` in chunks of at most ``eval_batch_size`` pairs (recbole's default 4,096).  Plumbing in torch: correct
        for any model, one ``predict`` per chunk -- slow by construction."""
        N = int(self.model.target_num_items)
        chunk = int(self.config['eval_batch_size']) if 'eval_batch_size' in self.config else 4096
        pairs = interaction.repeat_interleave(N)
        pairs.update({self.model.TARGET_ITEM_ID: torch.arange(N, device=self.device).repeat(n_user)})
        out = [self.model.predict(pairs[s:s + chunk]).reshape(-1) for s in range(0, n_user * N, max(chunk, 1))]
        return torch.cat(out).view(n_user, N).float()

    def _evaluate_batches(self, eval_data, sampled, fused, kmax):
        """The one batch loop: the route is decided once, every batch goes through its per-batch function into ``acc`` -- (hit matrices,
        positives per user, and on the two rank routes ranked items per user, sums of average ranks per user) -- and ``_result`` finishes."""
        names = self.metrics if self.metrics is not None else DEFAULT_METRICS
        # the non-accuracy metrics: the lists of every batch are folded into ``stats`` on the device, the arithmetic comes at the end
        stats = self._list_stats_for(eval_data)
        route = dict(kmax=kmax, fused=fused, wide=self._takes_wide_lists(kmax), stats=stats)
        batch = self._sampled_batch if sampled else self._rank_batch if self._takes_rank_route(fused, kmax) else self._list_batch
        acc = ([], [], [], [])
        n_users = 0
        for interaction, second, positive_u, positive_i in eval_data:          # second: history_index, or the sampled candidate lists
            interaction = interaction.to(self.device)
            n_users += len(interaction)
            batch(acc, interaction, len(interaction), second, positive_u, positive_i, **route)
        result = self._result(acc, names)
        if stats is not None:
            result.update(stats.result(n_users, self.list_metrics))
        return result

    def _list_batch(self, acc, interaction, n_user, history_index, positive_u, positive_i, kmax, fused, wide, stats):
        """The list route: the hits of the model's mask + top-k lists, or of torch.topk over the masked matrix where the route is unfused."""
        if fused or wide:
            hit, npos = self._topk_hits(interaction, n_user, history_index, positive_u, positive_i, kmax, wide=wide, stats=stats)
        else:
            scores = self._masked_scores(interaction, n_user, history_index, -np.inf)
            topk_vals, topk_idx = torch.topk(scores, kmax, dim=-1)
            if stats is not None:
                stats.add(topk_idx, topk_vals)                 # (a masked entry comes back with value -inf: a pad)
            pos = torch.zeros_like(scores, dtype=torch.bool)
            pos[positive_u, positive_i] = True
            hit, npos = torch.gather(pos, 1, topk_idx).float(), pos.sum(1).float()
        acc[0].append(hit); acc[1].append(npos)

    def _masked_scores(self, interaction, n_user, history_index, fill):
        """The [U, N] matrix where a route forms it, PAD column and history at ``fill`` (-inf for torch.topk, NaN for
        ``rank_counts_reference``): ``full_sort_predict``, or ``_predict_all_pairs`` for a model that defines ``predict`` only."""
        try:
            scores = self.model.full_sort_predict(interaction).view(n_user, -1)
        except NotImplementedError:
            scores = self._predict_all_pairs(interaction, n_user)
        scores[:, 0] = fill
        if history_index is not None:
            scores[history_index] = fill
        return scores

    def _takes_wide_lists(self, kmax):
        """Lists beyond the fused kernels' 64 entries -- eval_route='topk', or a non-accuracy metric under 'auto': on a GPU they come from
        the wide mask + top-k, for every model (a model without full_sort_topk included: its scores go through the selection in chunks,
        not as one [U, N] matrix)."""
        return ((self.eval_route == 'topk' or bool(self.list_metrics)) and self.fused_topk and FUSED_TOPK_MAX < kmax <= WIDE_TOPK_MAX
                and torch.device(self.device).type == 'cuda' and hasattr(self.model, 'full_sort_topk_wide'))

    def _count_lists(self, stats, fused, wide, kmax, interaction, n_user, history_index):
        """One batch's lists by the list route (fused, wide, or torch.topk of the masked matrix where the route is unfused), into ``stats``."""
        if wide or (fused and kmax <= FUSED_TOPK_MAX):
            return stats.add(self._topk_lists(interaction, n_user, history_index, kmax, wide=wide))
        vals, idx = torch.topk(self._masked_scores(interaction, n_user, history_index, -np.inf), kmax, dim=-1)
        stats.add(idx, vals)

    def _takes_rank_route(self, fused, kmax):
        gauc = self.metrics is not None and 'gauc' in self.metrics
        if self.list_metrics:
            return gauc                       # the list route answers everything but gauc (k <= 1024: checked at construction)
        if self.eval_route == 'rank':
            return True
        if self.eval_route == 'topk':
            if fused and kmax > WIDE_TOPK_MAX:
                raise ValueError(f"eval_route='topk': the mask + top-k lists hold k <= {WIDE_TOPK_MAX}, topk asks for {kmax}; use "
                                 f"eval_route='rank' or 'auto', or fused_topk=False")
            return False
        return gauc or (fused and kmax > FUSED_TOPK_MAX)



    @staticmethod
    def _csr(rows, cols, n_user, distinct):
        """(indptr [n_user + 1], cols ascending inside each user's range) of (row, column) pairs, by one pass over the keys: a sort --
        repeated pairs stay, enough for a mask -- or, ``distinct``, a unique: the rank kernels count n_unmasked from the history."""
        span = int(cols.max()) + 1 if cols.numel() else 1
        key = rows * span + cols
        key = torch.unique(key) if distinct else torch.sort(key).values          # (both sorted)
        indptr = torch.zeros(n_user + 1, device=rows.device, dtype=torch.int64)
        indptr[1:] = torch.cumsum(torch.bincount(key // span, minlength=n_user), 0)
        return indptr, (key % span).contiguous()

    def _history_csr(self, history_index, n_user, distinct):
        """``_csr`` of a batch's history (rows, cols) pairs; (None, None) where there is no history."""
        if history_index is None:
            return None, None
        rows, cols = (torch.as_tensor(t, device=self.device, dtype=torch.int64) for t in history_index)
        return self._csr(rows, cols, n_user, distinct) if cols.numel() else (None, None)

    def _positives_csr(self, positive_u, positive_i, n_user):
        """(indptr [n_user + 1], columns [P], positives per user [n_user], user row of each positive [P]) of a batch's ground truth"""
        pu = torch.as_tensor(positive_u, device=self.device, dtype=torch.int64)
        pi = torch.as_tensor(positive_i, device=self.device, dtype=torch.int64)
        pindptr, pcols = self._csr(pu, pi, n_user, distinct=True)
        npos = pindptr[1:] - pindptr[:-1]
        return pindptr, pcols, npos, torch.repeat_interleave(torch.arange(n_user, device=pu.device), npos)

    @staticmethod
    def _refuse_unranked(gt, prow, pcols, why):
        """gt < 0 marks a positive the counting could not rank: refused, with the first one named."""
        if bool((gt < 0).any()):
            p = int(torch.nonzero(gt < 0)[0])
            raise ValueError(f'evaluate: the positive item {int(pcols[p])} of user row {int(prow[p])} of this batch is {why} or has a NaN '
                             f'score: the rank route does not rank such a positive')

    def _rank_counts(self, interaction, n_user, history_index, positive_u, positive_i):
        """(user of each positive [P], gt, eq, eq_before [P], n_unmasked [U], positives per user [U]) of one batch: the model's
        ``full_sort_rank`` on a GPU; a torch restatement over the materialised matrix where there is none (plumbing, as the unfused
        route)."""
        pindptr, pcols, npos, prow = self._positives_csr(positive_u, positive_i, n_user)
        hindptr, hcols = self._history_csr(history_index, n_user, distinct=True)
        if torch.device(self.device).type == 'cuda':
            _score, gt, eq, eqb, nun = self.model.full_sort_rank(interaction, pindptr, pcols, hist_indptr=hindptr, hist_cols=hcols,
                                                                 predict_fallback=self._predict_all_pairs)
        else:
            scores = self._masked_scores(interaction, n_user, history_index, float('nan')).float()
            _score, gt, eq, eqb, nun = rank_counts_reference(scores, prow, pcols)
        self._refuse_unranked(gt, prow, pcols, "masked (PAD column or in the user's history)")
        return prow, gt, eq, eqb, nun, npos

    def _rank_batch(self, acc, interaction, n_user, history_index, positive_u, positive_i, kmax, fused, wide, stats):
        """The rank route.  Every metric from the rank of each positive over the masked catalogue: a positive at top-k position
        r = 1 + gt + eq_before (ties to the smaller column) is a hit at position r of the list for every k >= r -- the same hit matrix the
        top-k route builds, for any kmax; GAUC from the average ranks gt + (eq + 1) / 2.  With ``stats`` (gauc asked beside a non-accuracy
        metric) one list call per batch feeds it."""
        self._rank_batch_tail(acc, n_user, kmax, *self._rank_counts(interaction, n_user, history_index, positive_u, positive_i))
        if stats is not None:
            self._count_lists(stats, fused, wide, kmax, interaction, n_user, history_index)

    @staticmethod
    def _rank_batch_tail(acc, n_user, kmax, prow, gt, eq, eqb, nun, npos):
        """One batch's (hit matrix, positives per user, ranked items per user, sum of average ranks per user) from its rank counts,
        appended to ``acc``: the one copy both rank routes (full-sort and sampled candidates) end in."""
        at = gt.long() + eqb.long()
        hit = torch.zeros(n_user, kmax, device=gt.device, dtype=torch.float32)
        sel = at < kmax
        hit[prow[sel], at[sel]] = 1.0
        acc[0].append(hit); acc[1].append(npos)
        acc[2].append(nun.long())
        acc[3].append(torch.zeros(n_user, device=gt.device, dtype=torch.float64).index_add_(
            0, prow, gt.double() + (eq.double() + 1) / 2))

    def _result(self, acc, names):
        hits, pos_len, user_len, rank_sum = acc
        n_pos = torch.cat(pos_len)
        result = metrics_from_hits(torch.cat(hits), n_pos.float().clamp(min=1), self.topk, names)
        if 'gauc' in names and user_len:                   # (the list route keeps no ranks)
            result['gauc'] = gauc_from_counts(n_pos, torch.cat(user_len), torch.cat(rank_sum))
        return result

    def _sampled_batch(self, acc, interaction, n_user, candidates, positive_u, positive_i, kmax, fused, wide, stats):
        """Sampled-candidate evaluation (a ``NegSampleEvalLoader``): per batch the model's ``candidate_scores`` over the ragged candidate
        lists, then the rank of every positive inside its user's list (``functional.candidate_rank``; its torch restatement on
        ``device: cpu``), then the rank route's arithmetic.  ``n_unmasked`` is the user's distinct candidate count: what recbole's
        collector sees in a row of -inf with the candidates' scores scattered in."""
        from .. import functional as F_
        chunk = int(self.config['eval_batch_size']) if 'eval_batch_size' in self.config else 4096
        cand_indptr, cand_cols = (t.to(self.device) for t in candidates)
        pindptr, pcols, npos, prow = self._positives_csr(positive_u, positive_i, n_user)
        scores = self.model.candidate_scores(interaction, cand_indptr, cand_cols, chunk).float().contiguous()
        rank = F_.candidate_rank if torch.device(self.device).type == 'cuda' else F_.candidate_rank_reference
        _score, gt, eq, eqb, nun = rank(cand_indptr, cand_cols, scores, pindptr, pcols)
        self._refuse_unranked(gt, prow, pcols, "not among the user's candidates")
        self._rank_batch_tail(acc, n_user, kmax, prow, gt, eq, eqb, nun, npos)
