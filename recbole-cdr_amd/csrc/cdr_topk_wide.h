// Mask + top-k for lists beyond one wave (1 <= k <= kWideMaxK = 1024) over a score matrix that is in memory (a whole [U, N] matrix, or one
// column pass of it in the full-sort staging): per user the first k unmasked columns in the total order "score descending, then column
// ascending" -- the order of the rank route (cdr_rank.h: position 1 + gt + eq_before), so a positive at position r <= k sits at entry
// r - 1.  "Unmasked": not column 0 when exclude_col0, not in the user's history, score neither NaN nor -inf.  +inf is an ordinary score,
// -0.0 and +0.0 are equal scores (as they are to the rank route's float compares) and keep their bits.
//
// The order is ONE integer compare: an entry is a 64-bit key, the monotone float-to-uint32 transform of the score (zero canonical) in the
// high word; in the low word the inverted column (31 bits: a larger key is a smaller column) above one bit that says the zero was -0.0.
// Columns are distinct, so that bit never decides.  Key 0 is "no entry": every real key has a high word >= 0x00800000 (the most negative
// finite float), and -inf, NaN and masked columns never become keys.  A total order makes the result independent of stripe geometry,
// pass order and run.
//
// wide_stripe_kernel: one 256-thread workgroup per (user, stripe of the pass's columns); the stripe is walked in blocks of kRankCols
// columns with the evaluation mask as the LDS bitmap of rank_rows_kernel (rank_build_mask).  LDS holds kWideSlots keys: the sorted list
// [0, k) and behind it the candidate buffer.  Every score is compared against the threshold -- the list's last entry, or the running
// list's last entry of earlier passes when accumulating, whichever is larger -- as a float first and as a key second; the mask bit is
// tested only for the survivors, which a wave appends with one LDS atomic (ballot + popcount).  Between two looks at the counter a
// workgroup takes kWideStep columns, so the buffer is sorted into the list (one workgroup-wide bitonic sort over the next power of two
// >= k + candidates, then truncated to k) whenever the next step might overflow it.  Once a list is full the expected survivors per user
// are about k ln(N / k): the walk is one read of the scores.
//
// wide_merge_kernel: one workgroup per user merges the stripes' partial lists [U][stripes][k] and, when accumulating, the running list
// (vals / idx of the earlier passes) by the same sort-and-truncate, and writes vals / idx with (-inf, -1) behind the last entry.
//
// Internal linkage per translation unit, like cdr_rank.h.
#pragma once
#include "cdr_common.h"
#include "cdr_rank.h"

namespace {

constexpr int kWideMaxK = 1024;
constexpr int kWideSlots = 4096;          // keys in LDS (32 KB): list [0, k) | candidates [k, kWideSlots)
constexpr int kWideStep = 2048;           // columns of a workgroup between two looks at the candidate counter (2 float4 per thread)
static_assert(kWideSlots - kWideMaxK >= kWideStep + 3, "a step (and the next block's leading scalars) after a sort fits the buffer");
static_assert(kRankCols % kWideStep == 0, "steps tile a block");

__device__ __forceinline__ unsigned long long wide_key(float v, int col) {
    unsigned b = __float_as_uint(v), negzero = 0u;
    if (v == 0.0f) { negzero = b >> 31; b = 0u; }
    const unsigned h = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)h << 32) | (unsigned long long)(((~(unsigned)col) << 1) | negzero);
}

__device__ __forceinline__ float wide_key_value(unsigned long long key) {
    const unsigned h = (unsigned)(key >> 32);
    unsigned b = (h & 0x80000000u) ? (h & 0x7fffffffu) : ~h;
    if ((unsigned)key & 1u) b = 0x80000000u;
    return __uint_as_float(b);
}

__device__ __forceinline__ int wide_key_col(unsigned long long key) { return (int)(~((unsigned)key >> 1) & 0x7fffffffu); }

// keys[0, k) sorted descending and keys[k, k + count) in any order become keys[0, k) = the k largest of both, descending, and zeros behind.
// keys[k + count, kWideSlots) has to be zero.  Called by all 256 threads after a barrier that covers the last write to keys; ends in one.
__device__ __forceinline__ void wide_sort_truncate(unsigned long long* keys, int k, int count) {
    const int tid = threadIdx.x;
    int P = 2;
    while (P < k + count) P <<= 1;
    for (int sz = 2; sz <= P; sz <<= 1) {
        for (int st = sz >> 1; st > 0; st >>= 1) {
            for (int i = tid; i < (P >> 1); i += 256) {
                const int a = ((i & ~(st - 1)) << 1) | (i & (st - 1)), b = a | st;
                const unsigned long long ka = keys[a], kb = keys[b];
                if (((a & sz) == 0) ? ka < kb : ka > kb) { keys[a] = kb; keys[b] = ka; }
            }
            __syncthreads();
        }
    }
    for (int i = k + tid; i < P; i += 256) keys[i] = 0ull;
    __syncthreads();
}

// the running list's last entry as a key (0: the list is not full yet)
__device__ __forceinline__ unsigned long long wide_seed(const float* __restrict__ vals, const int64_t* __restrict__ idx, int64_t u, int k) {
    const int64_t c = idx[u * k + k - 1];
    return c >= 0 ? wide_key(vals[u * k + k - 1], (int)c) : 0ull;
}

__global__ __launch_bounds__(256) void wide_stripe_kernel(const float* __restrict__ scores, int64_t ld, int64_t U, int64_t n, int64_t col_off,
                                                          int k, topk_mask mk, int64_t stripes, int64_t chunks_per_stripe,
                                                          const float* __restrict__ run_vals, const int64_t* __restrict__ run_idx,
                                                          unsigned long long* __restrict__ part) {
    __shared__ unsigned long long keys[kWideSlots];
    __shared__ unsigned maskw[kRankMaskWords];
    __shared__ int cnt_s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int cap = kWideSlots - k;
    const int64_t n_chunks = (n + kRankCols - 1) / kRankCols;
    const float ninf = __uint_as_float(0xff800000u);
    for (int64_t w = blockIdx.x; w < U * stripes; w += gridDim.x) {
        const int64_t u = w / stripes, sp = w % stripes;
        __syncthreads();                                                 // the previous item's list was written out
        for (int i = tid; i < kWideSlots; i += 256) keys[i] = 0ull;
        if (tid == 0) cnt_s = 0;
        unsigned long long thr = run_idx ? wide_seed(run_vals, run_idx, u, k) : 0ull;
        float thrv = thr ? wide_key_value(thr) : ninf;
        const float* __restrict__ row = scores + u * ld;
        const int64_t ch1 = (sp + 1) * chunks_per_stripe < n_chunks ? (sp + 1) * chunks_per_stripe : n_chunks;
        for (int64_t ch = sp * chunks_per_stripe; ch < ch1; ++ch) {
            const int64_t c0 = ch * kRankCols, c1 = c0 + kRankCols < n ? c0 + kRankCols : n;
            rank_build_mask(maskw, mk, u, col_off + c0, col_off + c1);
            __syncthreads();
            // one entry: float compare, key compare, mask bit, then one LDS atomic per wave for its survivors (wave-uniform call)
            auto offer = [&](float v, int64_t c, bool valid) {
                bool pass = valid && v >= thrv && v > ninf;
                unsigned long long key = 0ull;
                if (pass) {
                    key = wide_key(v, (int)(col_off + c));
                    const int lc = (int)(c - c0);
                    pass = key > thr && !((maskw[lc >> 5] >> (lc & 31)) & 1u);
                }
                const unsigned long long m = __ballot(pass);
                if (m) {
                    const int first = __ffsll((long long)m) - 1;
                    int base = 0;
                    if (lane == first) base = atomicAdd(&cnt_s, __popcll(m));
                    base = __shfl(base, first);
                    if (pass) keys[k + base + __popcll(m & ((1ull << lane) - 1ull))] = key;
                }
            };
            // scalars up to the first 16-byte boundary of the row's block, float4 from there
            const int64_t a0 = (4 - (int64_t)(((uintptr_t)(row + c0) >> 2) & 3)) & 3;
            const int64_t cs = c0 + a0 < c1 ? c0 + a0 : c1;
            offer(c0 + tid < cs ? row[c0 + tid] : 0.0f, c0 + tid, c0 + tid < cs);
            for (int64_t b0 = cs; b0 < c1; b0 += kWideStep) {
                __syncthreads();
                const int cnt = cnt_s;
                __syncthreads();                                         // everyone has the same count before anyone appends again
                if (cnt + kWideStep + 3 > cap) {                         // (workgroup-uniform)
                    wide_sort_truncate(keys, k, cnt);
                    if (keys[k - 1] > thr) { thr = keys[k - 1]; thrv = wide_key_value(thr); }
                    if (tid == 0) cnt_s = 0;
                    __syncthreads();
                }
                float v[8];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int64_t c = b0 + 1024 * j + 4 * tid;
                    if (c + 4 <= c1) {
                        const float4 q = *reinterpret_cast<const float4*>(row + c);
                        v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[4 * j + e] = c + e < c1 ? row[c + e] : 0.0f;
                    }
                }
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int64_t c = b0 + 1024 * j + 4 * tid + e;
                        offer(v[4 * j + e], c, c < c1);
                    }
            }
        }
        __syncthreads();
        const int cnt = cnt_s;
        if (cnt) wide_sort_truncate(keys, k, cnt);
        unsigned long long* __restrict__ dst = part + (u * stripes + sp) * k;
        for (int i = tid; i < k; i += 256) dst[i] = keys[i];
    }
}

__global__ __launch_bounds__(256) void wide_merge_kernel(const unsigned long long* __restrict__ part, int64_t U, int64_t stripes, int k,
                                                         int accumulate, float* __restrict__ vals, int64_t* __restrict__ idx) {
    __shared__ unsigned long long keys[kWideSlots];
    const int tid = threadIdx.x;
    const int cap = kWideSlots - k;
    for (int64_t u = blockIdx.x; u < U; u += gridDim.x) {
        __syncthreads();                                                 // the previous user's list was written out
        for (int i = tid; i < kWideSlots; i += 256) {
            unsigned long long key = 0ull;
            if (accumulate && i < k) {
                const int64_t c = idx[u * k + i];
                if (c >= 0) key = wide_key(vals[u * k + i], (int)c);
            }
            keys[i] = key;
        }
        const unsigned long long* __restrict__ src = part + u * stripes * k;
        const int64_t total = stripes * k;
        for (int64_t t0 = 0; t0 < total; t0 += cap) {
            const int m = (int)(total - t0 < cap ? total - t0 : cap);
            __syncthreads();
            for (int i = tid; i < m; i += 256) keys[k + i] = src[t0 + i];
            __syncthreads();
            wide_sort_truncate(keys, k, m);
        }
        __syncthreads();
        for (int i = tid; i < k; i += 256) {
            const unsigned long long key = keys[i];
            vals[u * k + i] = key ? wide_key_value(key) : __uint_as_float(0xff800000u);
            idx[u * k + i] = key ? (int64_t)wide_key_col(key) : (int64_t)-1;
        }
    }
}

// Stripes per user for a pass of n columns: enough workgroups to fill the chip for few users, one stripe for many; at most
// wide_stripes_max(U, n'), for every n <= n'.
static int64_t wide_stripes_max(int64_t U, int64_t n) {
    const int64_t chunks = (n + kRankCols - 1) / kRankCols, want = ((int64_t)CDR_NUM_CU * 4 + U - 1) / U;
    return chunks < want ? chunks : want;
}

static size_t wide_part_bytes(int64_t U, int64_t n, int k) {
    return ((size_t)U * (size_t)wide_stripes_max(U, n) * (size_t)k * sizeof(unsigned long long) + 255) & ~(size_t)255;
}

// The lists of one block of columns: written to vals / idx, or with `accumulate` merged into the lists they hold.  part: wide_part_bytes.
static int wide_topk_launch(hipStream_t s, const float* scores, int64_t ld, int64_t U, int64_t n, int64_t col_off, int k, const topk_mask& mk,
                            float* vals, int64_t* idx, int accumulate, unsigned long long* part) {
    const int64_t chunks = (n + kRankCols - 1) / kRankCols, st = wide_stripes_max(U, n);
    const int64_t per = (chunks + st - 1) / st, stripes = (chunks + per - 1) / per;
    const int64_t blocks = U * stripes, cap = (int64_t)CDR_NUM_CU * 32;
    wide_stripe_kernel<<<dim3((unsigned)(blocks > cap ? cap : blocks)), dim3(256), 0, s>>>(scores, ld, U, n, col_off, k, mk, stripes, per,
                                                                                        accumulate ? vals : nullptr,
                                                                                        accumulate ? idx : nullptr, part);
    CDR_LAUNCH_CHECK();
    const int64_t mcap = (int64_t)CDR_NUM_CU * 8;
    wide_merge_kernel<<<dim3((unsigned)(U > mcap ? mcap : U)), dim3(256), 0, s>>>(part, U, stripes, k, accumulate, vals, idx);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

}  // namespace
