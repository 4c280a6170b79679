"""Evaluation glue of the models whose score of a user against the catalogue is a contraction of two rows -- the dot product (EMCDR,
CMF, CLFM, BiTGCF, DCDCSR) or SSCDR's ``-|u - i|^2``: the model states its operands once and every evaluation route is derived from
them here.  Not part of ``CrossDomainRecommender``: ``Trainer.evaluate`` decides its route with ``hasattr(model, 'full_sort_topk')``, and
the tower models have operands and thresholds of their own."""
import torch

from .. import functional as F_


class ContractionScoring:
    """Mixin next to ``CrossDomainRecommender``.  The model supplies ``_full_sort_operands(interaction) -> (user_e [U, D], slab0, slab1)``:
    the user rows and the item rows of the current phase as at most two contiguous row ranges (the catalogue's columns are ``slab0``'s
    rows followed by ``slab1``'s; a range may be empty or None).  SSCDR overrides the two distance hooks."""

    def _rank_distance_form(self):
        """True when ``_full_sort_operands`` are scored by the distance (SSCDR), not the dot product."""
        return False

    def _rank_col_sqnorm(self):
        return None

    def _scored_operands(self, interaction):
        """``_full_sort_operands`` with an empty or absent row range as None: the one place that decides it."""
        user_e, slab0, slab1 = self._full_sort_operands(interaction)
        return (user_e, slab0 if slab0 is not None and slab0.shape[0] else None, slab1 if slab1 is not None and slab1.shape[0] else None)

    _FULL_SORT_FLAT = True                  # (DCDCSR: False -- its reference returns the [U, N] matrix, the others flatten it)

    @torch.no_grad()
    def full_sort_predict(self, interaction):
        scores = F_.fullsort_scores(*self._scored_operands(interaction))
        return scores.view(-1) if self._FULL_SORT_FLAT else scores

    @torch.no_grad()
    def full_sort_topk(self, interaction, k, hist_indptr=None, hist_cols=None):
        """Evaluation without the [U, N] matrix: (values [U,k], columns [U,k]) of ``full_sort_predict`` after recbole's mask (column 0 and
        the per-user history columns, CSR with ascending columns) on the scoring kernel's fused mask + top-k (``F_.fullsort_topk``: values
        bit-equal to the unfused scores, no catalogue threshold) -- what ``Trainer.evaluate`` needs.  Lists beyond its 64 entries:
        ``full_sort_topk_wide``."""
        if k > F_.FUSED_TOPK_MAX:
            return self.full_sort_topk_wide(interaction, k, hist_indptr, hist_cols)
        return F_.fullsort_topk(*self._scored_operands(interaction), k=k, hist_indptr=hist_indptr, hist_cols=hist_cols,
                                exclude_first_col=True)

    @torch.no_grad()
    def full_sort_topk_wide(self, interaction, k, hist_indptr=None, hist_cols=None, predict_fallback=None):
        """``CrossDomainRecommender.full_sort_topk_wide`` without the [U, N] matrix: the operands are scored in column passes and selected
        there (``F_.fullsort_topk_wide``; SSCDR: the distance form with the column norms of its evaluation bracket)."""
        self._one_gpu_only('full_sort_topk_wide')
        user_e, slab0, slab1 = self._scored_operands(interaction)
        if self._rank_distance_form():
            return F_.fullsort_neg_sqdist_topk_wide(user_e, slab0, slab1, k, hist_indptr, hist_cols, col_sqnorm=self._rank_col_sqnorm())
        return F_.fullsort_topk_wide(user_e, slab0, slab1, k, hist_indptr, hist_cols)

    @torch.no_grad()
    def full_sort_rank(self, interaction, pos_indptr, pos_cols, hist_indptr=None, hist_cols=None, predict_fallback=None):
        """``CrossDomainRecommender.full_sort_rank`` without the [U, N] matrix: the operands are scored in column passes
        (``F_.fullsort_rank``; SSCDR: the distance form with the column norms of its evaluation bracket)."""
        self._one_gpu_only('full_sort_rank')
        user_e, slab0, slab1 = self._scored_operands(interaction)
        if self._rank_distance_form():
            return F_.fullsort_neg_sqdist_rank(user_e, slab0, slab1, pos_indptr, pos_cols, hist_indptr, hist_cols,
                                               col_sqnorm=self._rank_col_sqnorm())
        return F_.fullsort_rank(user_e, slab0, slab1, pos_indptr, pos_cols, hist_indptr, hist_cols)

    @torch.no_grad()
    def candidate_scores_from_operands(self, interaction, cand_indptr, cand_cols, chunk=4096):
        """``candidate_scores`` on the row-gather kernel (``chunk`` is the base-class route's): the user operand is formed once per user
        (EMCDR's and SSCDR's mapping MLP runs U times, not once per pair) and each candidate reads one item row.  A model whose ``predict``
        is this same function of its operands opts in with ``candidate_scores = ContractionScoring.candidate_scores_from_operands``."""
        self._candidate_guard()
        return F_.candidate_scores(*self._scored_operands(interaction), cand_indptr, cand_cols, distance=self._rank_distance_form())
