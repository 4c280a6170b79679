// The mask + top-k pieces shared by the scoring kernels that end in a top-k instead of a score matrix (cdr_gemm.hip: the dot-product
// full-sort; cdr_conet_fullsort.hip: the MLP-tower full-sort): the evaluation mask, the wave-held running list, the LDS-list flush
// of queued candidates and the merge of partial lists.  One copy, internal linkage per translation unit.
#pragma once
#include "cdr_common.h"

namespace {

// ---- running top-k of one user, kept by a whole wave (mask + top-k fused after scoring) -------------------
// Lane j holds entry j of the list (values descending; k <= 64).  A wave "offers" 64 candidate scores at once: a ballot
// against the current k-th value rejects almost all of them after the first few tiles (expected survivors per user over
// N items: k ln(N/k)), the survivors are inserted one at a time with a shuffle (no LDS, no sort).  Masked columns -- the
// PAD item and the user's history, given as a CSR with ascending columns (the reference sets those scores to -inf before
// torch.topk: recbole Trainer._full_sort_batch_eval) -- are tested only for survivors.
struct topk_mask {
    const int64_t* indptr;      // [U + 1] or nullptr
    const int64_t* cols;        // ascending inside each user's range
    int exclude_col0;
};

__device__ __forceinline__ bool topk_masked(const topk_mask& mk, int64_t u, int col) {
    if (mk.exclude_col0 && col == 0) return true;
    if (!mk.indptr) return false;
    int64_t lo = mk.indptr[u], hi = mk.indptr[u + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t c = mk.cols[mid];
        if (c == col) return true;
        if (c < col) lo = mid + 1; else hi = mid;
    }
    return false;
}

// e / ec: this lane's list entry (lanes >= k carry -inf / -1 and never change).  Returns the new k-th value.
// DEDUP: a candidate whose column already sits in the list is dropped (the persistent kernel's overflow recovery re-offers a whole tile,
// part of which may have entered the list through the queues already).
template <bool DEDUP = false>
__device__ __forceinline__ float topk_offer(float v, int col, float thr, float& e, int& ec, int k, const topk_mask& mk, int64_t u) {
    const int lane = threadIdx.x & 63;
    bool pass = v > thr;
    if (__ballot(pass) == 0) return thr;
    // every surviving lane tests ITS column against the mask at the same time (64 binary searches in flight): testing them one
    // after the other inside the insertion loop put ~2.5 us of dependent loads on each of the k ln(n/k) survivors of a wave
    if (pass && (mk.indptr || mk.exclude_col0)) pass = !topk_masked(mk, u, col);
    unsigned long long m = __ballot(pass);
    while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float cv = __shfl(v, l);
        const int cc = __shfl(col, l);
        if (!(cv > thr)) continue;                                             // wave-uniform: the k-th value rose meanwhile
        if (DEDUP && __ballot(lane < k && ec == cc)) continue;
        const int pos = __popcll(__ballot(lane < k && e >= cv));                // entries that stay in front (ties: first seen)
        const float up = __shfl_up(e, 1);
        const int upc = __shfl_up(ec, 1);
        if (lane < k) {
            if (lane == pos) { e = cv; ec = cc; }
            else if (lane > pos) { e = up; ec = upc; }
        }
        thr = __shfl(e, k - 1);
    }
    return thr;
}

struct topk_out {
    int k;
    int col_off;                // column index of this slab's first item
    float* pv;                  // partial lists [producer][M][k]
    int* pc;
    topk_mask mk;
    const float* seed = nullptr;    // optional: seed[u * seed_stride] = a LOWER BOUND of user u's final k-th value (the k-th value over a sample
    int64_t seed_stride = 0;        // of the columns): every stripe's threshold starts just below it instead of at -inf (round 6)
};
// the threshold a seed stands for: the largest float below it, so that a score EQUAL to the sample's k-th value still enters its list
__device__ __forceinline__ float topk_seed_thr(const topk_out& tk, int64_t u, int64_t M) {
    if (!tk.seed || u >= M) return -INFINITY;
    const float s = tk.seed[u * tk.seed_stride];
    return s == -INFINITY ? s : nextafterf(s, -INFINITY);
}

// Mask test for the queued candidates, one per lane (64 binary searches in flight), then the survivors enter their
// user's list one at a time (LDS only).  Thresholds may have risen since a candidate was queued: re-tested on insert.
// (Tried in round 5: row-parallel insertion -- lane l owns row l's list and walks the compacted queue itself: every step of such a
//  per-lane loop is a dependent LDS round trip, 26.7 -> 32.3 ms at U = 1,024, k = 10.)
__device__ __forceinline__ void topk_flush(volatile float* qv, volatile int* qc, volatile int* qu, int qn, volatile float* thr_l,
                                           volatile float* lv, volatile int* lc, const topk_out& tk, int64_t u0) {
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < qn; base += 64) {
        const int i = base + lane;
        const bool valid = i < qn;
        const float v = valid ? qv[i] : -INFINITY;
        const int c = valid ? qc[i] : 0;
        const int ul = valid ? qu[i] : 0;
        const bool ok = valid && v > thr_l[ul] && !topk_masked(tk.mk, u0 + ul, c);
        unsigned long long m = __ballot(ok);
        const topk_mask none{nullptr, nullptr, 0};
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            const float cv = __shfl(v, l);
            const int cc = __shfl(c, l);
            const int cu = __shfl(ul, l);
            const float thr = thr_l[cu];
            if (!(cv > thr)) continue;
            float e = lane < tk.k ? lv[cu * tk.k + lane] : -INFINITY;
            int ec = lane < tk.k ? lc[cu * tk.k + lane] : -1;
            const float nthr = topk_offer<true>(lane == 0 ? cv : -INFINITY, cc, thr, e, ec, tk.k, none, 0);
            if (lane < tk.k) { lv[cu * tk.k + lane] = e; lc[cu * tk.k + lane] = ec; }
            // (a seeded list is not full for a while: its k-th value is -inf, the seed stays the threshold until the list's own passes it)
            if (lane == 0) thr_l[cu] = tk.seed ? fmaxf(nthr, topk_seed_thr(tk, u0 + cu, u0 + cu + 1)) : nthr;
        }
    }
}

// Merge of partial lists (already masked): one wave per (user, group of `gsz` producers).  With `out_pv` set the group's list
// goes to partial list `group` of the next level; the last level (one group) writes the final [U, k] output.
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ pv, const int* __restrict__ pc, int64_t P,
                                                         int64_t U, int k, int64_t gsz, float* __restrict__ out_pv,
                                                         int* __restrict__ out_pc, float* __restrict__ out_v,
                                                         int64_t* __restrict__ out_c) {
    const int lane = threadIdx.x & 63;
    const int64_t groups = (P + gsz - 1) / gsz;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= U * groups) return;
    const int64_t u = w % U, grp = w / U;
    const int64_t p0 = grp * gsz, p1 = p0 + gsz < P ? p0 + gsz : P;
    float e = -INFINITY, thr = -INFINITY;
    int ec = -1;
    const topk_mask none{nullptr, nullptr, 0};
    const int64_t total = (p1 - p0) * k;                             // candidate i = entry i % k of producer p0 + i / k
    for (int64_t i0 = 0; i0 < total; i0 += 64 * 8) {
        float v[8];
        int c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t i = i0 + 64 * j + lane;
            const int64_t o = ((p0 + i / k) * U + u) * k + i % k;
            v[j] = i < total ? pv[o] : -INFINITY;
            c[j] = i < total ? pc[o] : -1;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) thr = topk_offer(v[j], c[j], thr, e, ec, k, none, u);
    }
    if (lane < k) {
        if (out_pv) {
            out_pv[(grp * U + u) * k + lane] = e;
            out_pc[(grp * U + u) * k + lane] = ec;
        } else {
            out_v[u * k + lane] = e;
            out_c[u * k + lane] = ec;
        }
    }
}

constexpr int64_t kTopkMergeGroup = 64;             // partial lists merged per wave and level

// bytes of `producers` partial lists' values (or columns), rounded to 256
inline size_t topk_part_bytes(int64_t producers, int64_t U, int k) {
    return ((size_t)producers * U * k * 4 + 255) & ~(size_t)255;
}

// `prod` partial lists (pv, pc: [prod][U][k]) -> out_vals / out_idx [U, k].  pv1 / pc1: room for ceil(prod / kTopkMergeGroup) lists,
// used when two levels are run (groups of 64 lists, then the group lists).
inline int topk_merge_launch(hipStream_t s, const float* pv, const int* pc, int64_t prod, int64_t U, int k, float* pv1, int* pc1,
                             float* out_vals, int64_t* out_idx) {
    const int64_t l1 = (prod + kTopkMergeGroup - 1) / kTopkMergeGroup;
    if (prod > 2 * kTopkMergeGroup) {                                // two levels: groups of 64 lists, then the l1 group lists
        topk_merge_kernel<<<dim3((unsigned)((U * l1 + 3) / 4)), dim3(256), 0, s>>>(pv, pc, prod, U, k, kTopkMergeGroup, pv1, pc1, nullptr, nullptr);
        CDR_LAUNCH_CHECK();
        topk_merge_kernel<<<dim3((unsigned)((U + 3) / 4)), dim3(256), 0, s>>>(pv1, pc1, l1, U, k, l1, nullptr, nullptr, out_vals, out_idx);
    } else {
        topk_merge_kernel<<<dim3((unsigned)((U + 3) / 4)), dim3(256), 0, s>>>(pv, pc, prod, U, k, prod, nullptr, nullptr, out_vals, out_idx);
    }
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

}  // namespace
