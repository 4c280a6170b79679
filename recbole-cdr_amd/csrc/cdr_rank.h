// Rank of each ground-truth positive over the masked columns of a score matrix that is in memory (a whole [U, N] matrix, or one column
// pass of it in the full-sort staging): for positive p of user u at column c with score t = pos_score[p], the number of unmasked columns
// scoring above t (gt), equal to t (eq, c itself included) and equal to t left of c (eq_before), plus the user's number of unmasked
// columns.  "Unmasked": not column 0 when exclude_col0, not in the user's history (topk_mask, cdr_topk.h), not NaN.  A positive that is
// itself masked, or whose score is NaN, keeps -1 in all three.  Everything is counted in integers and added with integer atomics: the
// result does not depend on the order the workgroups run in.
//
// One workgroup per (user, block of kRankCols columns).  The evaluation mask of the block is a bitmap in LDS, built once from the slice of
// the user's ascending history that falls into the block (two binary searches per workgroup, not one per column); the positives are taken
// kRankBatch at a time with their thresholds in registers, so LDS holds the same few hundred bytes whatever the user's number of
// positives is.  A NaN threshold (padding, masked or NaN positives) compares false against everything and counts nothing.
//
// The walk itself (rank_walk) takes its scores through a small source type, so the ragged candidate rows of sampled evaluation
// (cdr_candidate.hip: a flat score list with its column list, nothing masked) are counted by the same code as the matrix's rows.
#pragma once
#include "cdr_common.h"
#include "cdr_topk.h"

namespace {

constexpr int kRankBatch = 16;            // positives per walk of a workgroup over its columns
constexpr int kRankCols = 8192;           // columns per workgroup (32 per thread)
constexpr int kRankMaskWords = kRankCols / 32;

// first index in [lo, hi) whose column is >= col (cols ascending)
__device__ __forceinline__ int64_t rank_lower_bound(const int64_t* __restrict__ cols, int64_t lo, int64_t hi, int64_t col) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cols[mid] < col) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The evaluation mask of user u over the global columns [g0, g1), g1 - g0 <= kRankCols, as a bitmap in the workgroup's LDS (bit c - g0
// set: column c is masked).  Called by all 256 threads; the bitmap is complete after the caller's next __syncthreads().
__device__ __forceinline__ void rank_build_mask(unsigned* maskw, const topk_mask& mk, int64_t u, int64_t g0, int64_t g1) {
    const int tid = threadIdx.x;
    __syncthreads();                                                     // the previous block's LDS reads are over
    for (int i = tid; i < kRankMaskWords; i += 256) maskw[i] = 0u;
    __syncthreads();
    if (mk.exclude_col0 && g0 == 0 && tid == 0) atomicOr(&maskw[0], 1u);
    if (mk.indptr) {
        const int64_t h1 = mk.indptr[u + 1];
        for (int64_t h = rank_lower_bound(mk.cols, mk.indptr[u], h1, g0) + tid; h < h1; h += 256) {
            const int64_t c = mk.cols[h];
            if (c >= g1) break;
            if (c < g0) continue;                                        // (a history that is not ascending: never outside the bitmap)
            atomicOr(&maskw[(c - g0) >> 5], 1u << ((c - g0) & 31));
        }
    }
}

// stage 0: pos_score[p] = NaN (a positive whose column no pass covers stays flagged).  stage 1: the counters start at 0, at -1 for the
// positives that are masked or whose score is NaN, and n_unmasked at 0.  One wave per user.
__global__ __launch_bounds__(256) void rank_init_kernel(int stage, int64_t U, const int64_t* __restrict__ pos_indptr,
                                                        const int64_t* __restrict__ pos_cols, topk_mask mk, float* __restrict__ pos_score,
                                                        int* __restrict__ gt, int* __restrict__ eq, int* __restrict__ eqb,
                                                        int* __restrict__ n_unmasked) {
    const int lane = threadIdx.x & 63;
    const int64_t TW = (int64_t)gridDim.x * 4;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < U; u += TW) {
        const int64_t p1 = pos_indptr[u + 1];
        for (int64_t p = pos_indptr[u] + lane; p < p1; p += 64) {
            if (stage == 0) { pos_score[p] = __int_as_float(0x7fc00000); continue; }
            const int64_t c = pos_cols[p];
            const float t = pos_score[p];
            const bool ok = t == t && c >= 0 && c < ((int64_t)1 << 31) && !topk_masked(mk, u, (int)c);
            gt[p] = eq[p] = eqb[p] = ok ? 0 : -1;
        }
        if (stage == 1 && lane == 0) n_unmasked[u] = 0;
    }
}

// pos_score[p] = scores[u, c - col_off] for the positives whose column lies in [col_off, col_off + n).  One wave per user.
__global__ __launch_bounds__(256) void rank_gather_kernel(const float* __restrict__ scores, int64_t ld, int64_t U, int64_t n, int64_t col_off,
                                                          const int64_t* __restrict__ pos_indptr, const int64_t* __restrict__ pos_cols,
                                                          float* __restrict__ pos_score) {
    const int lane = threadIdx.x & 63;
    const int64_t TW = (int64_t)gridDim.x * 4;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < U; u += TW) {
        const int64_t p1 = pos_indptr[u + 1];
        for (int64_t p = pos_indptr[u] + lane; p < p1; p += 64) {
            const int64_t c = pos_cols[p] - col_off;
            if (c >= 0 && c < n) pos_score[p] = scores[u * ld + c];
        }
    }
}

// Where the walk below takes a block's scores from.  The matrix form: row `row` of the score matrix, columns [c0, c1) of this pass, the
// evaluation mask as the block's bitmap.
struct rank_src_rows {
    const float* __restrict__ row;
    const unsigned* maskw;
    int64_t c0, col_off;
    topk_mask mk;
    __device__ __forceinline__ float value(int64_t c) const {
        const int lc = (int)(c - c0);
        float v = row[c];
        if ((maskw[lc >> 5] >> (lc & 31)) & 1u) v = __int_as_float(0x7fc00000);
        return v;
    }
    __device__ __forceinline__ int col(int64_t c) const { return (int)(col_off + c); }
    __device__ __forceinline__ bool hidden(int64_t u, int c) const { return topk_masked(mk, u, c); }
};

// The walk of one workgroup (256 threads) over the entries [c0, c1) of `src` for the positives [p0, p1) of user u: the positives are taken
// kRankBatch at a time with their thresholds in registers; the counts of a batch are joined in LDS and ADDED to gt / eq / eqb, the number
// of non-NaN entries (first batch only) to n_unmasked[u].  thr_s, col_s [kRankBatch] and cnt [3 kRankBatch + 1] are the caller's LDS.
template <class Src>
__device__ __forceinline__ void rank_walk(const Src& src, int64_t u, int64_t c0, int64_t c1, int64_t p0, int64_t p1,
                                          const int64_t* __restrict__ pos_cols, const float* __restrict__ pos_score, int* __restrict__ gt,
                                          int* __restrict__ eq, int* __restrict__ eqb, int* __restrict__ n_unmasked, float* thr_s, int* col_s,
                                          int* cnt) {
    const int tid = threadIdx.x;
    bool first = true;                                               // a user without positives still gets n_unmasked
    for (int64_t pb = p0; first || pb < p1; pb += kRankBatch) {
        __syncthreads();                                             // the mask stands; the last batch's counters were read
        if (tid < kRankBatch) {
            const int64_t p = pb + tid;
            float t = __int_as_float(0x7fc00000);
            int64_t c = -1;
            if (p < p1) {
                c = pos_cols[p];
                t = pos_score[p];
                if (c < 0 || c >= ((int64_t)1 << 31) || src.hidden(u, (int)c)) t = __int_as_float(0x7fc00000);
            }
            thr_s[tid] = t;
            col_s[tid] = (int)c;
        }
        if (tid < 3 * kRankBatch + 1) cnt[tid] = 0;
        __syncthreads();
        float t[kRankBatch];
        int pc[kRankBatch], g[kRankBatch], e[kRankBatch], b[kRankBatch];
#pragma unroll
        for (int j = 0; j < kRankBatch; ++j) { t[j] = thr_s[j]; pc[j] = col_s[j]; g[j] = e[j] = b[j] = 0; }
        int nu = 0;
        for (int64_t c = c0 + tid; c < c1; c += 256) {
            const float v = src.value(c);
            nu += v == v ? 1 : 0;
            bool any_eq = false;
#pragma unroll
            for (int j = 0; j < kRankBatch; ++j) { g[j] += v > t[j] ? 1 : 0; any_eq |= v == t[j]; }
            if (any_eq) {
                const int col = src.col(c);
#pragma unroll
                for (int j = 0; j < kRankBatch; ++j) {
                    const bool q = v == t[j];
                    e[j] += q ? 1 : 0;
                    b[j] += q && col < pc[j] ? 1 : 0;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kRankBatch; ++j) {
            if (g[j]) atomicAdd(&cnt[3 * j], g[j]);
            if (e[j]) atomicAdd(&cnt[3 * j + 1], e[j]);
            if (b[j]) atomicAdd(&cnt[3 * j + 2], b[j]);
        }
        if (first && nu) atomicAdd(&cnt[3 * kRankBatch], nu);
        __syncthreads();
        if (tid < kRankBatch && pb + tid < p1) {
            const int64_t p = pb + tid;
            if (cnt[3 * tid]) atomicAdd(&gt[p], cnt[3 * tid]);
            if (cnt[3 * tid + 1]) atomicAdd(&eq[p], cnt[3 * tid + 1]);
            if (cnt[3 * tid + 2]) atomicAdd(&eqb[p], cnt[3 * tid + 2]);
        }
        if (first && tid == 0 && cnt[3 * kRankBatch]) atomicAdd(&n_unmasked[u], cnt[3 * kRankBatch]);
        first = false;
    }
}

__global__ __launch_bounds__(256) void rank_rows_kernel(const float* __restrict__ scores, int64_t ld, int64_t U, int64_t n, int64_t col_off,
                                                        const int64_t* __restrict__ pos_indptr, const int64_t* __restrict__ pos_cols,
                                                        topk_mask mk, const float* __restrict__ pos_score, int* __restrict__ gt,
                                                        int* __restrict__ eq, int* __restrict__ eqb, int* __restrict__ n_unmasked) {
    __shared__ unsigned maskw[kRankMaskWords];
    __shared__ float thr_s[kRankBatch];
    __shared__ int col_s[kRankBatch];
    __shared__ int cnt[3 * kRankBatch + 1];
    const int tid = threadIdx.x;
    const int64_t n_chunks = (n + kRankCols - 1) / kRankCols;
    for (int64_t w = blockIdx.x; w < U * n_chunks; w += gridDim.x) {
        const int64_t u = w / n_chunks;
        const int64_t c0 = (w % n_chunks) * kRankCols, c1 = c0 + kRankCols < n ? c0 + kRankCols : n;
        const int64_t g0 = col_off + c0, g1 = col_off + c1;               // the block's global columns
        rank_build_mask(maskw, mk, u, g0, g1);
        rank_walk(rank_src_rows{scores + u * ld, maskw, c0, col_off, mk}, u, c0, c1, pos_indptr[u], pos_indptr[u + 1], pos_cols, pos_score, gt,
                  eq, eqb, n_unmasked, thr_s, col_s, cnt);
    }
}

static int rank_init_launch(hipStream_t s, int stage, int64_t U, const int64_t* pos_indptr, const int64_t* pos_cols, const topk_mask& mk,
                            float* pos_score, int* gt, int* eq, int* eqb, int* n_unmasked) {
    const int64_t blocks = (U + 3) / 4;
    rank_init_kernel<<<dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s>>>(stage, U, pos_indptr, pos_cols, mk, pos_score, gt, eq,
                                                                                        eqb, n_unmasked);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

static int rank_gather_launch(hipStream_t s, const float* scores, int64_t ld, int64_t U, int64_t n, int64_t col_off, const int64_t* pos_indptr,
                              const int64_t* pos_cols, float* pos_score) {
    const int64_t blocks = (U + 3) / 4;
    rank_gather_kernel<<<dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s>>>(scores, ld, U, n, col_off, pos_indptr, pos_cols,
                                                                                          pos_score);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

// counts of one block of columns, ADDED to what the counters hold (rank_init_launch stage 1 starts them)
static int rank_rows_launch(hipStream_t s, const float* scores, int64_t ld, int64_t U, int64_t n, int64_t col_off, const int64_t* pos_indptr,
                            const int64_t* pos_cols, const topk_mask& mk, const float* pos_score, int* gt, int* eq, int* eqb, int* n_unmasked) {
    const int64_t blocks = U * ((n + kRankCols - 1) / kRankCols), cap = (int64_t)CDR_NUM_CU * 32;
    rank_rows_kernel<<<dim3((unsigned)(blocks > cap ? cap : blocks)), dim3(256), 0, s>>>(scores, ld, U, n, col_off, pos_indptr, pos_cols, mk,
                                                                                      pos_score, gt, eq, eqb, n_unmasked);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

}  // namespace
