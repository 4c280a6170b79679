// Sampled-candidate evaluation (eval_args mode uniN / popN): every evaluated user carries a ragged list of candidate columns -- its
// ground-truth positives and the negatives sampled for them, ascending and distinct (a CSR over the users) -- and each positive is ranked
// inside its user's list.  Two launches, neither of which expands (user, item) pairs or forms the [U, N] matrix:
//
//   cdr_candidate_scores_f32   scores[q] for the flat candidate list: a row gather.  A group of LPR = D/4 lanes owns one candidate at a time
//                              and moves its item row as one float4 per lane (D = 128: two rows per wave instruction, D = 64: four); the
//                              group walks the list with a grid stride and has kCandUnroll candidates' rows in flight before it reduces any
//                              of them (memory-level parallelism: the item rows are random 256..512-byte reads over a table far larger than
//                              the caches).  Neighbouring groups hold neighbouring candidates, which share their user row: those reads hit
//                              L2.  Flat over candidates, so ragged users need no balancing.
//   cdr_candidate_rank_f32     the contract of cdr_rank_rows_f32 over the ragged rows: thresholds by binary search in the user's ascending
//                              range, counts by the walk of cdr_rank.h, one workgroup per (user, block of kRankCols candidates).
#include "cdr_common.h"
#include "cdr_rank.h"

namespace {

constexpr int kCandUnroll = 8;       // candidates in flight per lane group (two row loads each, one of them an L2 hit)

// -DCDR_CAND_NT marks the item-row loads non-temporal, for A/B builds only: the rows are touched once per evaluation, but the hint
// LOSES here -- 1.19-1.46 x slower at five of six shapes of tools/mb_candidate_eval.py, 0.97 at D = 128 x 10 M items
// (profiles/mb_candidate_eval.txt) -- unlike the training step's read-modify-write rows (cdr_common.h)
#ifdef CDR_CAND_NT
constexpr bool kCandNT = true;
#else
constexpr bool kCandNT = false;
#endif

// FORM 0: sum u_d i_d.  FORM 1: -sum (u_d - i_d)^2, the distance as SSCDR's predict forms it.
template <int FORM>
__device__ __forceinline__ float cand_term4(float4 u, float4 i) {
    if (FORM == 0) return dot4(u, i);
    const float4 d = make_float4(u.x - i.x, u.y - i.y, u.z - i.z, u.w - i.w);
    return dot4(d, d);
}

template <int LPR, int FORM>
__global__ __launch_bounds__(kBlock) void cand_scores_kernel(const float* __restrict__ user_e, int D, const float* __restrict__ slab0,
                                                             int64_t n0, const float* __restrict__ slab1,
                                                             const int64_t* __restrict__ cand_row, const int64_t* __restrict__ cand_cols,
                                                             int64_t C, float* __restrict__ scores) {
    constexpr int GPB = kBlock / LPR;
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int D4 = D >> 2;
    if ((D & 3) == 0 && D4 <= LPR) {
        // one float4 per lane per row: the ids of kCandUnroll candidates first, then every row load, then the reductions
        const bool live = sub < D4;
        for (int64_t base = gg; base < C; base += TG * kCandUnroll) {
            int64_t ur[kCandUnroll], ic[kCandUnroll];
#pragma unroll
            for (int r = 0; r < kCandUnroll; ++r) {
                const int64_t q = base + (int64_t)r * TG;
                const int64_t qc = q < C ? q : C - 1;
                ur[r] = cand_row[qc]; ic[r] = cand_cols[qc];
            }
            float4 u[kCandUnroll], it[kCandUnroll];
#pragma unroll
            for (int r = 0; r < kCandUnroll; ++r) {
                const int64_t q = base + (int64_t)r * TG;
                u[r] = it[r] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (q < C && live) {
                    const float* irow = ic[r] < n0 ? slab0 + ic[r] * D : slab1 + (ic[r] - n0) * D;
                    it[r] = ld4n<kCandNT>(irow + 4 * sub);
                    u[r] = ld4(user_e + ur[r] * D + 4 * sub);
                }
            }
#pragma unroll
            for (int r = 0; r < kCandUnroll; ++r) {
                const int64_t q = base + (int64_t)r * TG;
                const float s = group_sum<LPR>(cand_term4<FORM>(u[r], it[r]));
                if (q < C && sub == 0) scores[q] = FORM == 0 ? s : -s;
            }
        }
        return;
    }
    // rows wider than 256 floats in float4 chunks; a D that is no multiple of 4 with 4-byte loads (rows are then not 16-byte aligned)
    for (int64_t q = gg; q < C; q += TG) {
        const int64_t ic = cand_cols[q];
        const float* irow = ic < n0 ? slab0 + ic * D : slab1 + (ic - n0) * D;
        const float* urow = user_e + cand_row[q] * D;
        float s = 0.f;
        if ((D & 3) == 0) {
            for (int c = sub; c < D4; c += LPR) s += cand_term4<FORM>(ld4(urow + 4 * c), ld4n<kCandNT>(irow + 4 * c));
        } else {
            for (int c = sub; c < D; c += LPR) {
                const float a = urow[c], b = irow[c];
                s += FORM == 0 ? a * b : (a - b) * (a - b);
            }
        }
        s = group_sum<LPR>(s);
        if (sub == 0) scores[q] = FORM == 0 ? s : -s;
    }
}

// ---- rank --------------------------------------------------------------------------------------------------------------------------
// The walk's source: the flat score and column lists; [c0, c1) is a block of one user's range.  Nothing is masked: a candidate list holds
// what is ranked and nothing else.
struct rank_src_cand {
    const float* __restrict__ scores;
    const int64_t* __restrict__ cols;
    __device__ __forceinline__ float value(int64_t c) const { return scores[c]; }
    __device__ __forceinline__ int col(int64_t c) const { return (int)cols[c]; }
    __device__ __forceinline__ bool hidden(int64_t, int) const { return false; }
};

// pos_score[p] = the score of the positive's column in its user's range (binary search: the range is ascending), NaN when the column is
// not there; the counters start at 0, at -1 for a positive that is absent or whose score is NaN; n_cand at 0.  One wave per user.
__global__ __launch_bounds__(256) void cand_rank_init_kernel(int64_t U, const int64_t* __restrict__ cand_indptr,
                                                             const int64_t* __restrict__ cand_cols, const float* __restrict__ scores,
                                                             const int64_t* __restrict__ pos_indptr, const int64_t* __restrict__ pos_cols,
                                                             float* __restrict__ pos_score, int* __restrict__ gt, int* __restrict__ eq,
                                                             int* __restrict__ eqb, int* __restrict__ n_cand) {
    const int lane = threadIdx.x & 63;
    const int64_t TW = (int64_t)gridDim.x * 4;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < U; u += TW) {
        const int64_t c0 = cand_indptr[u], c1 = cand_indptr[u + 1], p1 = pos_indptr[u + 1];
        for (int64_t p = pos_indptr[u] + lane; p < p1; p += 64) {
            const int64_t c = pos_cols[p];
            const int64_t at = rank_lower_bound(cand_cols, c0, c1, c);
            float t = __int_as_float(0x7fc00000);
            if (at < c1 && cand_cols[at] == c && c >= 0 && c < ((int64_t)1 << 31)) t = scores[at];
            pos_score[p] = t;
            gt[p] = eq[p] = eqb[p] = t == t ? 0 : -1;
        }
        if (lane == 0) n_cand[u] = 0;
    }
}

// Work unit j -> (user, block) without a host pass over the ragged sizes: user u owns the units [start(u), start(u + 1)) with
// start(u) = cand_indptr[u] / kRankCols + u, which is strictly increasing and leaves every user at least ceil(n_u / kRankCols) units, one
// for an empty user (its walk counts nothing); U + C / kRankCols units in all, the spare ones idle.
__device__ __forceinline__ int64_t cand_unit_start(const int64_t* __restrict__ cand_indptr, int64_t u) { return cand_indptr[u] / kRankCols + u; }

__global__ __launch_bounds__(256) void cand_rank_kernel(int64_t U, int64_t units, const int64_t* __restrict__ cand_indptr,
                                                        const int64_t* __restrict__ cand_cols, const float* __restrict__ scores,
                                                        const int64_t* __restrict__ pos_indptr, const int64_t* __restrict__ pos_cols,
                                                        const float* __restrict__ pos_score, int* __restrict__ gt, int* __restrict__ eq,
                                                        int* __restrict__ eqb, int* __restrict__ n_cand) {
    __shared__ float thr_s[kRankBatch];
    __shared__ int col_s[kRankBatch];
    __shared__ int cnt[3 * kRankBatch + 1];
    for (int64_t j = blockIdx.x; j < units; j += gridDim.x) {
        int64_t lo = 0, hi = U - 1;                                      // the last user whose first unit is <= j
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (cand_unit_start(cand_indptr, mid) <= j) lo = mid; else hi = mid - 1;
        }
        const int64_t u = lo, r0 = cand_indptr[u], r1 = cand_indptr[u + 1];
        const int64_t c0 = r0 + (j - cand_unit_start(cand_indptr, u)) * kRankCols;
        if (c0 < r0 || c0 >= r1) continue;                               // a spare unit, or an empty user (n_cand stays 0); uniform over the workgroup
        const int64_t c1 = c0 + kRankCols < r1 ? c0 + kRankCols : r1;
        rank_walk(rank_src_cand{scores, cand_cols}, u, c0, c1, pos_indptr[u], pos_indptr[u + 1], pos_cols, pos_score, gt, eq, eqb, n_cand, thr_s,
                  col_s, cnt);
    }
}

static int cand_lpr_for(int D) {      // lanes per candidate: one float4 each when D % 4 == 0 (cdr_lpr_for), else one float each, up to a wave
    if ((D & 3) == 0) return cdr_lpr_for(D);
    int l = 1;
    while (l < D && l < 64) l <<= 1;
    return l;
}

}  // namespace

extern "C" int cdr_candidate_scores_f32(void* stream, const float* user_e, int64_t U, int D, const float* slab0, int64_t n0,
                                        const float* slab1, int64_t n1, const int64_t* cand_row, const int64_t* cand_cols, int64_t C,
                                        int form, float* scores) {
    CDR_CHECK_ARG(U >= 0 && C >= 0 && D > 0 && n0 >= 0 && n1 >= 0 && (form == 0 || form == 1));
    if (U == 0 || C == 0) return CDR_OK;
    CDR_CHECK_ARG(user_e && cand_row && cand_cols && scores);
    CDR_CHECK_ARG((slab0 && n0 > 0) || (slab1 && n1 > 0));
    CDR_CHECK_ARG((slab0 || n0 == 0) && (slab1 || n1 == 0) && n0 + n1 < ((int64_t)1 << 31));
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cand_lpr_for(D);
    const bool rows_in_flight = (D & 3) == 0 && (D >> 2) <= lpr;
    DISPATCH_LPR(lpr, {
        const int grid = grid_for(C, (kBlock / L) * (rows_in_flight ? kCandUnroll : 1));
        auto kern = form == 0 ? cand_scores_kernel<L, 0> : cand_scores_kernel<L, 1>;
        kern<<<dim3(grid), dim3(kBlock), 0, s>>>(user_e, D, slab0, slab0 ? n0 : 0, slab1, cand_row, cand_cols, C, scores);
    });
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

extern "C" int cdr_candidate_rank_f32(void* stream, int64_t U, const int64_t* cand_indptr, const int64_t* cand_cols, const float* scores,
                                      int64_t C, const int64_t* pos_indptr, const int64_t* pos_cols, int64_t P, float* pos_score, int32_t* gt,
                                      int32_t* eq, int32_t* eq_before, int32_t* n_cand) {
    CDR_CHECK_ARG(U >= 0 && U < ((int64_t)1 << 30) && C >= 0 && P >= 0);
    CDR_CHECK_ARG(pos_score && gt && eq && eq_before && n_cand);
    if (U == 0 || C == 0 || P == 0) return CDR_OK;
    CDR_CHECK_ARG(cand_indptr && cand_cols && scores && pos_indptr && pos_cols);
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = (U + 3) / 4;
    cand_rank_init_kernel<<<dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s>>>(U, cand_indptr, cand_cols, scores, pos_indptr,
                                                                                                 pos_cols, pos_score, gt, eq, eq_before, n_cand);
    CDR_LAUNCH_CHECK();
    const int64_t units = U + C / kRankCols, cap = (int64_t)CDR_NUM_CU * 32;
    cand_rank_kernel<<<dim3((unsigned)(units > cap ? cap : units)), dim3(256), 0, s>>>(U, units, cand_indptr, cand_cols, scores, pos_indptr,
                                                                                        pos_cols, pos_score, gt, eq, eq_before, n_cand);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}
