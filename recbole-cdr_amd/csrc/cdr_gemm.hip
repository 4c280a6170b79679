// fp32 MFMA contraction with fused epilogue (K6/K8/K9 of SURVEY.md 2.2).
//
// C[M,N] = epi(op(A) x op(B)) on v_mfma_f32_32x32x2_f32 (exact fp32, one rounding per product: the same numerics class
// as the reference's sgemm).  Both operand tiles live in LDS K-contiguous, rows padded to 36 dwords: that stride makes
// the 16-B fragment reads (ds_read_b128) bank-conflict-free for every 16-lane service group (36*i mod 64 is a distinct
// multiple of 4 for 16 rows that differ mod 16) and keeps rows 16-B aligned for ds_write_b128.  The contraction index
// is permuted inside each 8-wide K step so that ONE float4 per lane feeds FOUR MFMAs: lane (i = l&31, h = l>>5) reads
// k = 8s+4h..8s+4h+3 of row i, and MFMA c consumes component c of both operands, i.e. the k pair {8s+c, 8s+4+c}.
//
// Block = 256 threads = 4 waves.  Tile configurations:
//   <BM=32 ,BN=128>: 1x4 waves, one 32x32 accumulator each     -- few users per call (full-sort at reference defaults)
//   <BM=128,BN=128>: 2x2 waves, 2x2 accumulators (64 regs) each -- throughput shape (many users, MLP layers)
// A-operand rows = M side (users / batch rows), B-operand rows = N side (items / output features), so a lane's
// accumulator column is an N index and every store instruction writes 32 consecutive floats per half-wave.
#include <stdlib.h>
#include <type_traits>
#include "cdr_common.h"
#include "cdr_mfma.h"
#include "cdr_topk.h"

namespace {


constexpr int BK = 32;
constexpr int LDS_STRIDE = BK + 4;   // 36 dwords

__device__ __forceinline__ float act_apply(int act, float v) {
    switch (act) {
        case CDR_ACT_TANH: return tanhf(v);
        case CDR_ACT_RELU: return v > 0.f ? v : 0.f;
        case CDR_ACT_SIGMOID: return 1.0f / (1.0f + expf(-v));
        default: return v;
    }
}

// Stage a ROWS x BK tile of op(X) into LDS (row-major, K contiguous).
//   !TRANS: X is [rows, K] with leading dimension ld (K contiguous)  -> float4 along K, ds_write_b128
//    TRANS: X is [K, rows] with leading dimension ld (rows contiguous) -> float4 along rows, 4x ds_write_b32
template <int ROWS, bool TRANS>
__device__ __forceinline__ void stage_tile(float* __restrict__ lds, const float* __restrict__ X, int64_t ld,
                                           int64_t row0, int64_t nrows, int64_t k0, int64_t K, bool vec_ok) {
    constexpr int NLOAD = ROWS / 32;   // float4 per thread
    const int t = threadIdx.x;
    if (!TRANS) {
#pragma unroll
        for (int q = 0; q < NLOAD; ++q) {
            const int r = (t >> 3) + 32 * q, kc = t & 7;
            const int64_t gr = row0 + r, gk = k0 + 4 * kc;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gr < nrows) {
                const float* p = X + gr * ld + gk;
                if (vec_ok && gk + 3 < K) v = ld4(p);
                else {
                    if (gk + 0 < K) v.x = p[0];
                    if (gk + 1 < K) v.y = p[1];
                    if (gk + 2 < K) v.z = p[2];
                    if (gk + 3 < K) v.w = p[3];
                }
            }
            st4(lds + r * LDS_STRIDE + 4 * kc, v);
        }
    } else {
        constexpr int RC = ROWS / 4;   // float4 per k-row
#pragma unroll
        for (int q = 0; q < NLOAD; ++q) {
            const int e = t + 256 * q;
            const int k = e / RC, rc = e % RC;
            const int64_t gk = k0 + k, gr = row0 + 4 * rc;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gk < K) {
                const float* p = X + gk * ld + gr;
                if (vec_ok && gr + 3 < nrows) v = ld4(p);
                else {
                    if (gr + 0 < nrows) v.x = p[0];
                    if (gr + 1 < nrows) v.y = p[1];
                    if (gr + 2 < nrows) v.z = p[2];
                    if (gr + 3 < nrows) v.w = p[3];
                }
            }
            float* d = lds + (4 * rc) * LDS_STRIDE + k;
            d[0] = v.x; d[LDS_STRIDE] = v.y; d[2 * LDS_STRIDE] = v.z; d[3 * LDS_STRIDE] = v.w;
        }
    }
}

// EPI_SQDIST: v = -(((-2*acc) + rown[m]) + coln[n])   (sscdr.py:253-259)
template <int BM, int BN, bool TA, bool TB, bool EPI_SQDIST>
__global__ __launch_bounds__(256) void gemm_f32_kernel(int64_t M, int64_t N, int64_t K, const float* __restrict__ A,
                                                       int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                       float* __restrict__ C, int64_t ldc,
                                                       const float* __restrict__ bias, int act, int accumulate,
                                                       const float* __restrict__ rown, const float* __restrict__ coln,
                                                       int vecA, int vecB, const float* __restrict__ rowscale,
                                                       int64_t k_chunk) {
    constexpr int WM = (BM == 128) ? 2 : 1;            // waves along M
    constexpr int WN = 4 / WM;                         // waves along N
    constexpr int TM = BM / (32 * WM);                 // 32x32 tiles per wave along M
    constexpr int TN = BN / (32 * WN);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;
    float* Bs = smem + BM * LDS_STRIDE;

    // N tiles vary fastest across blockIdx.x so that consecutive blocks stream consecutive item rows
    const int64_t n_tiles = (N + BN - 1) / BN;
    const int64_t bm = blockIdx.x / n_tiles, bn = blockIdx.x % n_tiles;
    const int64_t m0 = bm * BM, n0 = bn * BN;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // split-K (blockIdx.y): weight-gradient shapes (tiny MxN, K = batch rows) would otherwise run on a handful of CUs;
    // each K slice adds its partial product into a pre-zeroed C with fp32 atomics
    const int64_t k_begin = (int64_t)blockIdx.y * k_chunk;
    const int64_t k_end = (k_begin + k_chunk < K) ? k_begin + k_chunk : K;
    const bool split = gridDim.y > 1;
    for (int64_t k0 = k_begin; k0 < k_end; k0 += BK) {
        stage_tile<BM, TA>(As, A, lda, m0, M, k0, k_end, vecA != 0);
        stage_tile<BN, !TB>(Bs, B, ldb, n0, N, k0, k_end, vecB != 0);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < BK / 8; ++s) {
            float4 a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = ld4(As + ((wm * TM + i) * 32 + li) * LDS_STRIDE + 8 * s + 4 * lh);
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = ld4(Bs + ((wn * TN + j) * 32 + li) * LDS_STRIDE + 8 * s + 4 * lh);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
                }
        }
        __syncthreads();
    }

    // epilogue: lane column = N index; register r -> row (r&3) + 8*(r>>2) + 4*lh
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t n = n0 + (wn * TN + j) * 32 + li;
            if (n >= N) continue;
            const float bv = bias ? bias[n] : 0.f;
            const float cn = EPI_SQDIST ? coln[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= M) continue;
                float v = acc[i][j][r];
                if (EPI_SQDIST) {
                    v = -(((-2.0f * v) + rown[m]) + cn);
                } else {
                    if (rowscale) v *= rowscale[m];
                    if (split) { atomicAdd(&C[m * ldc + n], v); continue; }
                    if (accumulate == 2) v = act_apply(act, (C[m * ldc + n] + v) + bv);       // pre-activation add
                    else {
                        v = act_apply(act, v + bv);
                        if (accumulate == 1) v += C[m * ldc + n];                             // post-activation add
                    }
                }
                C[m * ldc + n] = v;
            }
        }
}

template <bool TA, bool TB, bool SQ>
int launch(hipStream_t s, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb,
           float* C, int64_t ldc, const float* bias, int act, int accumulate, const float* rown, const float* coln,
           const float* rowscale = nullptr) {
    // float4 global loads need 16-B aligned rows along the contiguous dimension
    const int vecA = ((lda & 3) == 0) && (((uintptr_t)A & 15) == 0);
    const int vecB = ((ldb & 3) == 0) && (((uintptr_t)B & 15) == 0);
    // few 128x128 tiles (the MLP layers: M = batch rows, N <= 64) leave most CUs idle: use the 32-row tile there too
    const bool small_m = M <= 64 || ((M + 127) / 128) * ((N + 127) / 128) < 192;
    const int64_t tiles = (small_m ? (M + 31) / 32 : (M + 127) / 128) * ((N + 127) / 128);
    // split K when the output has too few tiles to fill the chip and the epilogue is a plain (or post-add) product
    unsigned splits = 1;
    int64_t k_chunk = K;
    if (!SQ && tiles < 64 && K >= 1024 && bias == nullptr && act == CDR_ACT_NONE && accumulate != 2) {
        k_chunk = 256;
        splits = (unsigned)((K + k_chunk - 1) / k_chunk);
        if (accumulate == 0) {
            hipError_t e0 = hipMemset2DAsync(C, (size_t)ldc * sizeof(float), 0, (size_t)N * sizeof(float), (size_t)M, s);
            if (e0 != hipSuccess) { cdr_set_error("cdr_gemm_f32: memset failed: %s", hipGetErrorString(e0)); return (int)e0; }
        }
    }
    if (small_m) {
        constexpr int BM = 32, BN = 128;
        const int64_t grid = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
        const size_t lds = (size_t)(BM + BN) * LDS_STRIDE * sizeof(float);
        gemm_f32_kernel<BM, BN, TA, TB, SQ><<<dim3((unsigned)grid, splits), dim3(256), lds, s>>>(
            M, N, K, A, lda, B, ldb, C, ldc, bias, act, accumulate, rown, coln, vecA, vecB, rowscale, k_chunk);
    } else {
        constexpr int BM = 128, BN = 128;
        const int64_t grid = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
        const size_t lds = (size_t)(BM + BN) * LDS_STRIDE * sizeof(float);
        gemm_f32_kernel<BM, BN, TA, TB, SQ><<<dim3((unsigned)grid, splits), dim3(256), lds, s>>>(
            M, N, K, A, lda, B, ldb, C, ldc, bias, act, accumulate, rown, coln, vecA, vecB, rowscale, k_chunk);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cdr_set_error("cdr_gemm_f32: launch failed: %s", hipGetErrorString(e)); return (int)e; }
    return CDR_OK;
}

// ---- few-users scoring (U <= 8): HBM-streaming GEMV ----------------------------------------------------------------
// The reference's full-sort batch is U = max(eval_batch_size // N, 1) users (recbole FullSortEvalDataLoader): 1..8 for
// every catalogue above 512 items.  There the contraction is a pure stream over the item slab: a lane group of
// LPR = D/4 lanes owns 32 CONSECUTIVE item rows per chunk (16 KB contiguous at D = 128), keeps 4 of them in flight,
// holds the U user vectors in registers, reduces each dot product inside the group, and parks the result in LDS so the
// block writes every score row as whole 1 KiB lines.  Bytes per item = 4D + 4U; no MFMA (padding U to a 32-row tile
// would make the matrix pipe, not HBM, the limiter).
template <int LPR, int UMAX>
__global__ __launch_bounds__(256) void fullsort_gemv_kernel(const float* __restrict__ users, int U, int D,
                                                            const float* __restrict__ items, int64_t N,
                                                            float* __restrict__ scores, int64_t ldc) {
    constexpr int GPB = 256 / LPR;              // groups per block
    constexpr int RPG = 256 / GPB;              // rows per group per chunk (= LPR)
    __shared__ float sm[UMAX][256];
    const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    const int D4 = D >> 2;
    const bool live = sub < D4;
    float4 uv[UMAX];
#pragma unroll
    for (int u = 0; u < UMAX; ++u)
        uv[u] = (u < U && live) ? ld4(users + (int64_t)u * D + 4 * sub) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t n_chunks = (N + 255) / 256;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t row0 = chunk * 256 + (int64_t)grp * RPG;
#pragma unroll 1
        for (int it = 0; it < RPG; it += 4) {
            float4 x[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = row0 + it + r;
                x[r] = (row < N && live) ? ld4n<true>(items + row * D + 4 * sub) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int u = 0; u < UMAX; ++u) {
                    const float d = group_sum<LPR>(dot4(uv[u], x[r]));
                    if (sub == 0) sm[u][grp * RPG + it + r] = d;
                }
            }
        }
        __syncthreads();
        const int64_t n = chunk * 256 + threadIdx.x;
        if (n < N) {
#pragma unroll
            for (int u = 0; u < UMAX; ++u)
                if (u < U) scores[(int64_t)u * ldc + n] = sm[u][threadIdx.x];
        }
        __syncthreads();
    }
}

template <int LPR>
static int launch_gemv(hipStream_t s, const float* users, int U, int D, const float* items, int64_t N, float* scores, int64_t ldc) {
    int64_t chunks = (N + 255) / 256;
    const unsigned grid = (unsigned)(chunks < 4096 ? chunks : 4096);
    if (U <= 1) fullsort_gemv_kernel<LPR, 1><<<dim3(grid), dim3(256), 0, s>>>(users, U, D, items, N, scores, ldc);
    else if (U <= 2) fullsort_gemv_kernel<LPR, 2><<<dim3(grid), dim3(256), 0, s>>>(users, U, D, items, N, scores, ldc);
    else if (U <= 4) fullsort_gemv_kernel<LPR, 4><<<dim3(grid), dim3(256), 0, s>>>(users, U, D, items, N, scores, ldc);
    else fullsort_gemv_kernel<LPR, 8><<<dim3(grid), dim3(256), 0, s>>>(users, U, D, items, N, scores, ldc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cdr_set_error("fullsort gemv: launch failed: %s", hipGetErrorString(e)); return (int)e; }
    return CDR_OK;
}

static bool gemv_ok(int64_t U, int D, const float* users, const float* items) {
    return U <= 8 && (D & 3) == 0 && D >= 16 && D <= 256 && (((uintptr_t)users | (uintptr_t)items) & 15) == 0;
}

static int gemv_dispatch(hipStream_t s, const float* users, int U, int D, const float* items, int64_t N, float* scores, int64_t ldc) {
    switch (cdr_lpr_for(D)) {
        case 4: return launch_gemv<4>(s, users, U, D, items, N, scores, ldc);
        case 8: return launch_gemv<8>(s, users, U, D, items, N, scores, ldc);
        case 16: return launch_gemv<16>(s, users, U, D, items, N, scores, ldc);
        case 32: return launch_gemv<32>(s, users, U, D, items, N, scores, ldc);
        default: return launch_gemv<64>(s, users, U, D, items, N, scores, ldc);
    }
}

// (the evaluation mask, the wave-held running list topk_offer, topk_flush and the merge of partial lists: cdr_topk.h)

// ---- many-users scoring (U >= 64, D <= 128): persistent fp32-MFMA kernel ----------------------------------------------
// One 256-thread workgroup per CU, resident for the whole call.  Waves are 2 (M) x 2 (N); each wave keeps its users'
// A fragments for the WHOLE contraction (D <= 128) in registers -- 32*MT rows x D, loaded once -- so the only LDS traffic
// is the item tile: [64 items, D] double-buffered (2 x 33 KB), filled through registers (global_load issued before the
// MFMA phase of the previous tile, written to the other buffer after it: one barrier per tile).  Work mapping is
// XCD-aware: workgroup b runs on XCD b % 8 (observed placement; speed only), and the workgroups of one XCD that share
// an item stripe walk it together for different user blocks, so an item tile is fetched from HBM once and re-used
// from that XCD's L2 by the other user blocks instead of being re-read U/BM times.
// ---- few users (U <= 8): the streaming GEMV with the mask + top-k behind it ------------------------------------------------
// Same stream over the item slab as fullsort_gemv_kernel (a lane group owns 32 consecutive item rows per chunk, users in
// registers, the chunk's 256 scores per user parked in LDS) -- but instead of writing them out, wave w offers the scores of users
// w and w + 4 to their running lists (registers: lane j = entry j).  Survivors of the k-th-value test wait in a per-user LDS queue
// and are mask-tested 64 at a time (one history search per lane), so the dependent global loads of the search are paid once per
// 64 survivors, not once each.  A block ends with one partial list per user; the reference's U = 1 evaluation never writes the
// 40 MB score vector.
constexpr int kGemvQueue = 128;

template <int LPR, int UMAX>
__global__ __launch_bounds__(256) void fullsort_gemv_topk_kernel(const float* __restrict__ users, int U, int D,
                                                                 const float* __restrict__ items, int64_t N, int col_off, int k,
                                                                 topk_mask mk, float* __restrict__ pv, int* __restrict__ pc,
                                                                 int64_t prod0) {
    constexpr int GPB = 256 / LPR;
    constexpr int RPG = 256 / GPB;
    constexpr int SLOTS = (UMAX + 3) / 4;                     // users per wave
    __shared__ float sm[UMAX][256];
    __shared__ float qv[UMAX][kGemvQueue];
    __shared__ int qc[UMAX][kGemvQueue];
    const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D4 = D >> 2;
    const bool live = sub < D4;
    float4 uv[UMAX];
#pragma unroll
    for (int u = 0; u < UMAX; ++u)
        uv[u] = (u < U && live) ? ld4(users + (int64_t)u * D + 4 * sub) : make_float4(0.f, 0.f, 0.f, 0.f);
    float e[SLOTS], thr[SLOTS];
    int ec[SLOTS], qn[SLOTS];
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) { e[sl] = thr[sl] = -INFINITY; ec[sl] = -1; qn[sl] = 0; }
    const int64_t n_chunks = (N + 255) / 256;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t row0 = chunk * 256 + (int64_t)grp * RPG;
#pragma unroll 1
        for (int it = 0; it < RPG; it += 4) {
            float4 x[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = row0 + it + r;
                x[r] = (row < N && live) ? ld4n<true>(items + row * D + 4 * sub) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int u = 0; u < UMAX; ++u) {
                    const float d = group_sum<LPR>(dot4(uv[u], x[r]));
                    if (sub == 0) sm[u][grp * RPG + it + r] = d;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            const int u = wave + 4 * sl;
            if (u >= U || u >= UMAX) continue;                 // wave-uniform
            volatile float* myv = qv[u];
            volatile int* myc = qc[u];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t nrow = chunk * 256 + 64 * j + lane;
                const float v = sm[u][64 * j + lane];
                const bool pass = nrow < N && v > thr[sl];
                const unsigned long long m = __ballot(pass);
                if (m == 0) continue;
                if (pass) {
                    const int at = qn[sl] + __popcll(m & ((1ull << lane) - 1));
                    myv[at] = v; myc[at] = col_off + (int)nrow;
                }
                qn[sl] += __popcll(m);
                if (qn[sl] > kGemvQueue - 64) {
                    for (int b = 0; b < qn[sl]; b += 64) {
                        const int i = b + lane;
                        thr[sl] = topk_offer(i < qn[sl] ? myv[i] : -INFINITY, i < qn[sl] ? myc[i] : 0, thr[sl], e[sl], ec[sl], k, mk, u);
                    }
                    qn[sl] = 0;
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        const int u = wave + 4 * sl;
        if (u >= U || u >= UMAX) continue;
        volatile float* myv = qv[u];
        volatile int* myc = qc[u];
        for (int b = 0; b < qn[sl]; b += 64) {
            const int i = b + lane;
            thr[sl] = topk_offer(i < qn[sl] ? myv[i] : -INFINITY, i < qn[sl] ? myc[i] : 0, thr[sl], e[sl], ec[sl], k, mk, u);
        }
        if (lane < k) {
            const int64_t o = ((prod0 + blockIdx.x) * U + u) * k + lane;
            pv[o] = e[sl];
            pc[o] = ec[sl];
        }
    }
}

constexpr int kGemvTopkBlocks = 1024;

template <int LPR>
static int launch_gemv_topk(hipStream_t s, const float* users, int U, int D, const float* items, int64_t N, int col_off, int k,
                            const topk_mask& mk, float* pv, int* pc, int64_t prod0, unsigned grid) {
    if (U <= 1) fullsort_gemv_topk_kernel<LPR, 1><<<dim3(grid), dim3(256), 0, s>>>(users, U, D, items, N, col_off, k, mk, pv, pc, prod0);
    else if (U <= 2) fullsort_gemv_topk_kernel<LPR, 2><<<dim3(grid), dim3(256), 0, s>>>(users, U, D, items, N, col_off, k, mk, pv, pc, prod0);
    else if (U <= 4) fullsort_gemv_topk_kernel<LPR, 4><<<dim3(grid), dim3(256), 0, s>>>(users, U, D, items, N, col_off, k, mk, pv, pc, prod0);
    else fullsort_gemv_topk_kernel<LPR, 8><<<dim3(grid), dim3(256), 0, s>>>(users, U, D, items, N, col_off, k, mk, pv, pc, prod0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cdr_set_error("fullsort gemv top-k: launch failed: %s", hipGetErrorString(e)); return (int)e; }
    return CDR_OK;
}

static int gemv_topk_dispatch(hipStream_t s, const float* users, int U, int D, const float* items, int64_t N, int col_off, int k,
                              const topk_mask& mk, float* pv, int* pc, int64_t prod0, unsigned grid) {
    switch (cdr_lpr_for(D)) {
        case 4: return launch_gemv_topk<4>(s, users, U, D, items, N, col_off, k, mk, pv, pc, prod0, grid);
        case 8: return launch_gemv_topk<8>(s, users, U, D, items, N, col_off, k, mk, pv, pc, prod0, grid);
        case 16: return launch_gemv_topk<16>(s, users, U, D, items, N, col_off, k, mk, pv, pc, prod0, grid);
        case 32: return launch_gemv_topk<32>(s, users, U, D, items, N, col_off, k, mk, pv, pc, prod0, grid);
        default: return launch_gemv_topk<64>(s, users, U, D, items, N, col_off, k, mk, pv, pc, prod0, grid);
    }
}

constexpr int kTopkQueue = 256;
#ifndef TOPK_TEST_FIRST_STEP
#define TOPK_TEST_FIRST_STEP 0
#endif

// SQDIST (with TOPK): the scores are SSCDR's distances -(((-2 <u,i>) + |u|^2) + |i|^2) (gemm_f32_kernel's EPI_SQDIST, same expression
// and association), formed once behind the MFMA phase so that thresholds, queues and the LDS score tile only ever see distances.  The
// two norm vectors ride behind the lists' arguments in these instantiations only: the others keep their argument block and their code.
struct topk_out_sq : topk_out {
    const float* rown;          // [M] squared norms of the user rows
    const float* coln;          // squared norms of this slab's item rows (index 0 = the slab's first row)
};

template <int MT, int K, bool TOPK, bool SQDIST = false>
__global__ __launch_bounds__(256, 1) void score_persistent_kernel(const float* __restrict__ A, int M,
                                                                  const float* __restrict__ B, int NT,
                                                                  float* __restrict__ C, int64_t ldc,
                                                                  std::conditional_t<SQDIST, topk_out_sq, topk_out> tk) {
    static_assert(TOPK || !SQDIST, "the distance epilogue exists in the top-k form only");
    constexpr int BM = 64 * MT;            // 2 waves along M, MT 32-row tiles each
    constexpr int BN = 64;                 // 2 waves along N, one 32-col tile each
    constexpr int KS = K / 8;              // K steps of 8 (one float4 per lane per step feeds 4 MFMAs)
    constexpr int LDB = K + 4;             // padded LDS row (dwords): 16-B aligned rows, conflict-free ds_read_b128
    constexpr int BUF = BN * LDB;          // floats per item-tile buffer
    constexpr int F4R = K / 4;             // float4 per item row
    constexpr int NQ = BN * F4R / 256;     // float4 each thread stages per tile (K = 128: 8)
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;

    // ---- work mapping (block b runs on XCD b % 8: speed only) -----------------------------------------------------
    const int MB = (M + BM - 1) / BM;
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;
    const int MBc = MB < per_xcd ? MB : per_xcd;
    const int S = per_xcd / MBc;
    const int mslot = j % MBc, sidx = j / MBc;
    if (sidx >= S) return;
    const int stripe = xcd * S + sidx, n_stripes = 8 * S;
    // a stripe is a CONTIGUOUS range of item tiles (round 5; it was every n_stripes-th tile): a workgroup's successive tiles then read
    // adjacent item rows and write adjacent 256-byte pieces of each of its users' score rows -- same sharing of a tile between the user
    // blocks of a stripe, DRAM pages that stay open
    const int tiles_per_stripe = (NT + n_stripes - 1) / n_stripes;
    const int tile_begin = stripe * tiles_per_stripe;
    const int tile_end = tile_begin + tiles_per_stripe < NT ? tile_begin + tiles_per_stripe : NT;

    // per-thread staging geometry (compile-time divisors)
    int st_lds[NQ];
    int64_t st_gl[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int e = tid + 256 * q;
        const int r = e / F4R, c = e % F4R;
        st_lds[q] = r * LDB + 4 * c;
        st_gl[q] = (int64_t)r * K + 4 * c;
    }
    const int frag_off = (wn * 32 + li) * LDB + 4 * lh;
    // TOPK: LDS behind the two item buffers = score tile [BM][65] | k-th values [BM] | list values [BM][k] | list columns
    constexpr int SCS = 65;
    float* sc = smem + 2 * BUF;
    volatile float* thr_l = sc + BM * SCS;
    volatile float* lv = thr_l + BM;
    volatile int* lc = reinterpret_cast<volatile int*>(lv + BM * (TOPK ? tk.k : 0));
    constexpr int RPW = BM / 4;            // user rows each wave scans
    constexpr int QC = kTopkQueue;         // per-wave queue of candidates waiting for the mask test
    volatile float* q0 = reinterpret_cast<volatile float*>(lc + BM * (TOPK ? tk.k : 0));     // four queues: values | columns | rows
    volatile float* qv = q0 + wave * QC * 3;
    volatile int* qc = reinterpret_cast<volatile int*>(qv + QC);
    volatile int* qu = qc + QC;
    int* qcnt = reinterpret_cast<int*>(const_cast<float*>(q0) + 4 * QC * 3);                  // [4] queue fills, [4] = overflow flag, [5] = attention flag (a queue half full / overflowed)
    // SQDIST: the user block's BM row norms behind everything else (16-byte aligned: every region in front is a multiple of four words).
    // Not in registers: the wave's 16 MT of them across the phase would cost what the 4 MT thresholds did (see below)
    [[maybe_unused]] float* rn_l = reinterpret_cast<float*>(qcnt + 8);

    for (int mb = mslot; mb < MB; mb += MBc) {
        const int m0 = mb * BM + wm * 32 * MT;
        const bool full_rows = (int64_t)(mb + 1) * BM <= M;          // (workgroup-uniform) every user row of this block exists
        int tiles_done = 0;
        if (TOPK) {
            for (int i = tid; i < BM; i += 256) thr_l[i] = topk_seed_thr(tk, (int64_t)mb * BM + i, M);
            for (int i = tid; i < BM * tk.k; i += 256) { lv[i] = -INFINITY; lc[i] = -1; }
            if (tid < 6) qcnt[tid] = 0;
            if constexpr (SQDIST) {            // rows past M: 0 (never read from memory; validmask / the scans drop them anyway)
                for (int i = tid; i < BM; i += 256) {
                    const int64_t u = (int64_t)mb * BM + i;
                    rn_l[i] = u < M ? tk.rown[u] : 0.f;
                }
            }
        }
        // this wave's user rows, whole K, in registers (loaded once per user block)
        float4 a[MT][KS];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int r = m0 + 32 * t + li;
            const float* ap = A + (int64_t)(r < M ? r : 0) * K + 4 * lh;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                a[t][s] = ld4(ap + 8 * s);
                if (r >= M) a[t][s] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        int tile = tile_begin;
        int buf = 0;
        if (tile < tile_end) {
            const float* bp = B + (int64_t)tile * BN * K;
#pragma unroll
            for (int q = 0; q < NQ; ++q) st4(smem + st_lds[q], ld4(bp + st_gl[q]));
        }
        // SQDIST: the norm of this lane's column of the tile in the phase, and of the prefetched tile (loaded with its rows)
        [[maybe_unused]] float cn_cur = 0.f, cn_next = 0.f;
        if constexpr (SQDIST) { if (tile < tile_end) cn_cur = tk.coln[(int64_t)tile * BN + wn * 32 + li]; }
        __syncthreads();
        // PIPE (score output, two accumulator tiles per wave): the scores of tile i are written while tile i+1's MFMAs run
        // (they wait in `prev`), not between two MFMA phases.  Same-box A/B: +4 % (D = 128) / +17 % (D = 64) at U = 1,024; with
        // one tile per wave (U <= 64) +14 % at D = 64 and -3 % at D = 128, hence the condition
        constexpr bool PIPE = !TOPK && (MT == 2 || K == 64);
        // D = 128, two tiles per wave: also the LDS park of the prefetched tile moves into the phase (+8 % at U = 1,024; it lost
        // 5..20 % at D = 64, where the phase is half as long)
        // (round 5: the top-k form parks there as well -- it has no stores to hide, but its park sat exposed between the phase and the
        //  threshold compare)
        constexpr bool PARK_IN = (PIPE || TOPK) && MT == 2 && K == 128;
        f32x16 prev[MT];
        int prev_tile = -1;
        // the slow path of one tile (accumulators x): through LDS, the owner waves scan their rows; queued candidates first, then the tile's
        auto slow_scan = [&](const f32x16 (&x)[MT], int tl) {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    sc[(wm * 32 * MT + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh) * SCS + wn * 32 + li] = x[t][r];
            __syncthreads();
            if (tid == 0) qcnt[4] = 0;
            int qn = qcnt[wave];               // the owner wave scans its rows: private appends, flushes as it goes
            if (qn > QC) qn = QC;
            const int col = tk.col_off + tl * BN + lane;
            const float tl_ = thr_l[wave * RPW + (lane % RPW)];
#pragma unroll 1
            for (int r0 = 0; r0 < RPW; r0 += 8) {                         // eight rows' scores at a time (independent reads)
                float vr[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) vr[j] = sc[(wave * RPW + r0 + j) * SCS + lane];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int ul = wave * RPW + r0 + j;
                    const float thr = __shfl(tl_, r0 + j);
                    const bool pass = vr[j] > thr && (int64_t)mb * BM + ul < M;
                    const unsigned long long m = __ballot(pass);
                    if (m == 0) continue;
                    if (qn + 64 > QC) { topk_flush(qv, qc, qu, qn, thr_l, lv, lc, tk, (int64_t)mb * BM); qn = 0; }
                    if (pass) {
                        const int at = qn + __popcll(m & ((1ull << lane) - 1));
                        qv[at] = vr[j]; qc[at] = col; qu[at] = ul;
                    }
                    qn += __popcll(m);
                }
            }
            if (qn) { topk_flush(qv, qc, qu, qn, thr_l, lv, lc, tk, (int64_t)mb * BM); qn = 0; }
            if (lane == 0) qcnt[wave] = 0;
        };
        for (; tile < tile_end; ++tile) {
            const int next = tile + 1;
            const bool has_next = next < tile_end;
            // issue the next tile's global loads now; they land while the MFMAs below run
            float4 stage[NQ];
            {
                const float* bp = B + (int64_t)(has_next ? next : tile) * BN * K;
#pragma unroll
                for (int q = 0; q < NQ; ++q) stage[q] = ld4(bp + st_gl[q]);
                if constexpr (SQDIST) cn_next = tk.coln[(int64_t)(has_next ? next : tile) * BN + wn * 32 + li];
            }
            // hipcc otherwise SINKS these loads below the MFMA phase (register pressure heuristic) and serialises
            // load -> wait -> ds_write after it: 1.7x slower end to end.  Pin the issue point.
            __builtin_amdgcn_sched_barrier(0);
            f32x16 acc[MT];
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
            const float* bs = smem + buf * BUF + frag_off;
            const bool pend = TOPK && prev_tile >= 0;             // a tile's accumulators wait in `prev` for their threshold test
            // The waiting tile against its users' k-th values, branch-free inside the phase: the thresholds of the wave's 32 MT user rows
            // come as 4 MT 16-byte LDS reads issued in front of the first MFMA (they only change in the drain phases, which sit between
            // barriers; rows past M get +inf), each K step then tests four rows with plain compares into a per-lane bit mask -- a few VALU
            // instructions per MFMA, no waitcnt, no branch (the first shadowed form tested and appended inside the phase: a stalled LDS
            // read or a branch there keeps the wave from issuing its next MFMA, and the compare cost 6 ms of 28 exactly as it had behind
            // the phase).  Survivors (bits set) are appended to the owners' queues behind the phase: about half of the tiles have none.
            // (Register pressure decides here: holding all 4 MT threshold float4 through the phase pushed the kernel's arrays out of the 256
            //  architectural VGPRs -- 247 AGPRs of moves -- and the test cost 5 ms of 28: thresholds are read one group AHEAD of their test,
            //  four registers at a time.  Tried: the compares as wave masks OR-ed on the scalar unit with the exact per-lane tests redone
            //  behind the phase for the tiles that have a candidate -- 24.0 -> 24.7 ms at k = 1, 26.7 -> 29.6 at k = 10.)
            unsigned passmask = 0u, validmask = 0xFFFFFFFFu;
            const float* thr_base = const_cast<const float*>(thr_l) + wm * 32 * MT + 4 * lh;
            constexpr int TG0 = TOPK_TEST_FIRST_STEP;                // first K step that tests a group
            float4 th_next = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pend && (int64_t)(mb + 1) * BM > M) {               // the last user block: rows past M never survive
#pragma unroll
                for (int g = 0; g < MT * 4; ++g)
#pragma unroll
                    for (int rl = 0; rl < 4; ++rl) {
                        const int ul = wm * 32 * MT + 32 * (g >> 2) + 8 * (g & 3) + 4 * lh + rl;
                        if ((int64_t)mb * BM + ul >= M) validmask &= ~(1u << (4 * g + rl));
                    }
            }
            auto test_group = [&](int g) {
                if (g == 0) th_next = *reinterpret_cast<const float4*>(thr_base);
                const float4 th = th_next;
                if (g + 1 < MT * 4) th_next = *reinterpret_cast<const float4*>(thr_base + 32 * ((g + 1) >> 2) + 8 * ((g + 1) & 3));
                const int t = g >> 2, r4 = g & 3;
                passmask |= (prev[t][4 * r4] > th.x ? 1u : 0u) << (4 * g);
                passmask |= (prev[t][4 * r4 + 1] > th.y ? 1u : 0u) << (4 * g + 1);
                passmask |= (prev[t][4 * r4 + 2] > th.z ? 1u : 0u) << (4 * g + 2);
                passmask |= (prev[t][4 * r4 + 3] > th.w ? 1u : 0u) << (4 * g + 3);
            };
            // bit 4 g + rl of a lane's mask: accumulator 4 (g & 3) + rl of tile row block g >> 2 survived -> one slot in the queue of the wave
            // that owns its row
            auto append_survivors = [&]() {
                passmask &= validmask;
                if (__ballot(passmask != 0u) == 0) return;
#pragma unroll
                for (int g = 0; g < MT * 4; ++g) {
                    if (__ballot((passmask >> (4 * g)) & 0xFu) == 0) continue;
#pragma unroll
                    for (int rl = 0; rl < 4; ++rl) {
                        const int t = g >> 2, r = 4 * (g & 3) + rl;
                        if (!((passmask >> (4 * g + rl)) & 1u)) continue;
                        const int ul = wm * 32 * MT + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        const int owner = ul / RPW;
                        const int slot = atomicAdd(&qcnt[owner], 1);
                        if (slot < QC) {
                            volatile float* ov = q0 + owner * QC * 3;
                            ov[slot] = prev[t][r];
                            reinterpret_cast<volatile int*>(ov + QC)[slot] = tk.col_off + prev_tile * BN + wn * 32 + li;
                            reinterpret_cast<volatile int*>(ov + 2 * QC)[slot] = ul;
                            if (slot >= QC / 2 - 1) qcnt[5] = 1;          // half full: every wave drains behind the next barrier
                        } else {
                            qcnt[4] = 1; qcnt[5] = 1;
                        }
                    }
                }
            };
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const float4 b = ld4(bs + 8 * s);
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][s].x, b.x, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][s].y, b.y, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][s].z, b.z, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][s].w, b.w, acc[t], 0, 0, 0);
                }
                // TOPK: the tile that waits in `prev` is compared with its users' k-th values HERE, one group of four user rows per K step,
                // in the shadow of this tile's MFMAs (round 5: behind the phase the same work cost 2,400 of a tile's 13,900 cycles)
                if (TOPK && pend && s >= TG0 && s < TG0 + MT * 4) test_group(s - TG0);
                if (PARK_IN && s == KS / 4) {   // the prefetched tile is parked inside the phase too (its loads landed a while ago)
                    float* dst = smem + (buf ^ 1) * BUF;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) st4(dst + st_lds[q], stage[q]);
                }
                // the previous tile's stores ride in one half of this MFMA phase: the second half when the park sits in the first
                if (PIPE && (PARK_IN ? s >= KS / 2 : s < KS / 2)) {
                    constexpr int PER = (MT * 16 + KS / 2 - 1) / (KS / 2);
                    if (prev_tile >= 0) {
                        float* cpp = C + (int64_t)prev_tile * BN + wn * 32 + li;
                        // a user block that lies wholly inside M (all but the last) stores without a per-lane row test: as written
                        // first, every store sat behind its own exec-mask save / branch (28 of them inside the MFMA phase), each one a
                        // scheduling fence between two MFMAs
                        if (full_rows) {
#pragma unroll
                            for (int j = 0; j < PER; ++j) {
                                const int i = (PARK_IN ? s - KS / 2 : s) * PER + j;
                                if (i < MT * 16) {
                                    const int t = i / 16, r = i % 16;
                                    const int m = m0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
                                    cpp[(int64_t)m * ldc] = prev[t][r];
                                }
                            }
                        } else {
#pragma unroll
                            for (int j = 0; j < PER; ++j) {
                                const int i = (PARK_IN ? s - KS / 2 : s) * PER + j;
                                if (i < MT * 16) {
                                    const int t = i / 16, r = i % 16;
                                    const int m = m0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
                                    if (m < M) cpp[(int64_t)m * ldc] = prev[t][r];
                                }
                            }
                        }
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            // park the prefetched tile in the other buffer FIRST (last read two iterations ago): the vmcnt wait in front
            // of these LDS writes covers the loads issued before the MFMA phase, not the epilogue's stores below
            if (!PARK_IN) {
                float* dst = smem + (buf ^ 1) * BUF;
#pragma unroll
                for (int q = 0; q < NQ; ++q) st4(dst + st_lds[q], stage[q]);
            }
            if constexpr (SQDIST) {
                // dot products -> distances, once: the hand-over to `prev`, slow_scan and the tail group all read them from `acc` / `prev`.
                // Register r is user row (r & 3) + 8 (r >> 2) + 4 lh of its 32-row tile: four consecutive rows per 16-byte LDS read, the
                // addressing test_group uses for the thresholds.  (A NaN score fails every `>` below: it never enters a queue, a list or a threshold.)
                const float* rn_base = rn_l + wm * 32 * MT + 4 * lh;
#pragma unroll
                for (int t = 0; t < MT; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 rn = *reinterpret_cast<const float4*>(rn_base + 32 * t + 8 * g);
                        acc[t][4 * g] = -(((-2.0f * acc[t][4 * g]) + rn.x) + cn_cur);
                        acc[t][4 * g + 1] = -(((-2.0f * acc[t][4 * g + 1]) + rn.y) + cn_cur);
                        acc[t][4 * g + 2] = -(((-2.0f * acc[t][4 * g + 2]) + rn.z) + cn_cur);
                        acc[t][4 * g + 3] = -(((-2.0f * acc[t][4 * g + 3]) + rn.w) + cn_cur);
                    }
                cn_cur = cn_next;
            }
            // epilogue: lane column = item ; register r -> user row (r&3) + 8*(r>>2) + 4*lh
            if (!TOPK) {
                if (PIPE) {
#pragma unroll
                    for (int t = 0; t < MT; ++t) prev[t] = acc[t];
                    prev_tile = tile;
                } else {
                    float* cp = C + (int64_t)tile * BN + wn * 32 + li;
#pragma unroll
                    for (int t = 0; t < MT; ++t)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int m = m0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
                            if (full_rows || m < M) cp[(int64_t)m * ldc] = acc[t][r];
                        }
                }
                __syncthreads();
            } else {
                // Fast path: every accumulator is compared IN REGISTERS with the k-th value of its user row (offer_group, in the shadow of
                // the NEXT tile's MFMA phase); the rare survivor (expected k ln(n/k) per user over the whole stream) reserves a slot in
                // the queue of the wave that owns the row's list (LDS atomic) -- no LDS round trip of the score tile.  Queues are drained
                // between two barriers when one is half full.  The first tiles of a user block (thresholds still -inf) and any tile whose
                // survivors do not fit take the slow path: the whole tile goes through LDS and the owner waves scan it (a candidate that
                // had entered a list through the queues already is dropped there: topk_offer<DEDUP>).
                if (pend) {
                    if constexpr (KS - TG0 < MT * 4) { for (int g = KS - TG0; g < MT * 4; ++g) test_group(g); }
                    append_survivors();
                }
                __syncthreads();                   // parked tile + the waiting tile's queue appends visible
                const int att = qcnt[5];           // ONE LDS read per tile: some queue is half full or overflowed (set by the appender)
                bool refresh = false;
                if (att && qcnt[4]) {              // some queue overflowed: the waiting tile goes the slow way
                    if (lane == 0 && qcnt[wave] > QC) qcnt[wave] = QC;
                    slow_scan(prev, prev_tile);
                    refresh = true;
                }
                const bool slow_now = tiles_done < 2;
                if (slow_now) {
                    if (refresh) __syncthreads();
                    slow_scan(acc, tile);
                    refresh = true;
                    prev_tile = -1;
                } else {
                    if (att && !refresh && (qcnt[0] >= QC / 2 || qcnt[1] >= QC / 2 || qcnt[2] >= QC / 2 || qcnt[3] >= QC / 2)) {   // uniform
                        const int qn = qcnt[wave];
                        if (qn) topk_flush(qv, qc, qu, qn, thr_l, lv, lc, tk, (int64_t)mb * BM);
                        if (lane == 0) qcnt[wave] = 0;
                        refresh = true;
                    }
#pragma unroll
                    for (int t = 0; t < MT; ++t) prev[t] = acc[t];
                    prev_tile = tile;
                }
                if (refresh) {                     // lists, k-th values and empty queues visible before anyone appends again
                    __syncthreads();
                    if (att) {                     // (uniform) everyone has read the flag: clear it between two barriers
                        if (tid == 0) qcnt[5] = 0;
                        __syncthreads();
                    }
                }
                ++tiles_done;
            }
            buf ^= 1;
        }
        if (PIPE && prev_tile >= 0) {          // the last tile of this user block
            float* cpp = C + (int64_t)prev_tile * BN + wn * 32 + li;
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (m < M) cpp[(int64_t)m * ldc] = prev[t][r];
                }
        }
        if (TOPK) {
            if (prev_tile >= 0) {              // the last tile of this user block still waits for its threshold test
                const auto tail_group = [&](int t, int r4) {
                    const float4 th4 = *reinterpret_cast<const float4*>(const_cast<const float*>(thr_l) + wm * 32 * MT + 32 * t + 8 * r4 + 4 * lh);
                    const float th[4] = {th4.x, th4.y, th4.z, th4.w};
#pragma unroll
                    for (int rl = 0; rl < 4; ++rl) {
                        const int r = 4 * r4 + rl;
                        const int ul = wm * 32 * MT + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        if (prev[t][r] > th[rl] && (int64_t)mb * BM + ul < M) {
                            const int owner = ul / RPW;
                            const int slot = atomicAdd(&qcnt[owner], 1);
                            if (slot < QC) {
                                volatile float* ov = q0 + owner * QC * 3;
                                ov[slot] = prev[t][r];
                                reinterpret_cast<volatile int*>(ov + QC)[slot] = tk.col_off + prev_tile * BN + wn * 32 + li;
                                reinterpret_cast<volatile int*>(ov + 2 * QC)[slot] = ul;
                            } else {
                                qcnt[4] = 1;
                            }
                        }
                    }
                };
#pragma unroll
                for (int g = 0; g < MT * 4; ++g) tail_group(g >> 2, g & 3);
                __syncthreads();
                if (qcnt[4]) {
                    if (lane == 0 && qcnt[wave] > QC) qcnt[wave] = QC;
                    slow_scan(prev, prev_tile);
                    __syncthreads();
                }
            }
            // drain what the fast path left in the queues
            const int qn = qcnt[wave];
            if (qn) topk_flush(qv, qc, qu, qn, thr_l, lv, lc, tk, (int64_t)mb * BM);
        }
        __syncthreads();
        if (TOPK) {
            // this stripe's candidates for its user block: partial list [stripe][user][k]
            for (int i = tid; i < BM * tk.k; i += 256) {
                const int64_t ug = (int64_t)mb * BM + i / tk.k;
                if (ug < M) {
                    const int64_t o = ((int64_t)stripe * M + ug) * tk.k + i % tk.k;
                    tk.pv[o] = lv[i];
                    tk.pc[o] = lc[i];
                }
            }
            __syncthreads();
        }
    }
}

// Scores already in memory ([U, n] with leading dimension ld): one wave per (user, chunk of columns), list in registers.
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ scores, int64_t ld, int64_t U, int64_t n,
                                                        int64_t chunk, int col_off, int k, topk_mask mk,
                                                        float* __restrict__ pv, int* __restrict__ pc, int64_t prod0) {
    const int lane = threadIdx.x & 63;
    const int64_t n_chunks = (n + chunk - 1) / chunk;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= U * n_chunks) return;
    const int64_t u = w / n_chunks, ch = w % n_chunks;
    const int64_t c0 = ch * chunk, c1 = c0 + chunk < n ? c0 + chunk : n;
    float e = -INFINITY, thr = -INFINITY;
    int ec = -1;
    const float* row = scores + u * ld;
    for (int64_t c = c0; c < c1; c += 64 * 8) {                     // 8 independent loads in flight, offered in column order
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t cc = c + 64 * j + lane;
            v[j] = cc < c1 ? row[cc] : -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) thr = topk_offer(v[j], col_off + (int)(c + 64 * j + lane), thr, e, ec, k, mk, u);
    }
    if (lane < k) {
        const int64_t o = ((prod0 + ch) * U + u) * k + lane;
        pv[o] = e;
        pc[o] = ec;
    }
}

static bool score_persistent_ok(int64_t U, int D, int64_t N, const float* users, const float* items) {
    return U > 32 && U < ((int64_t)1 << 30) && (D == 64 || D == 128) && N >= 64 && N < ((int64_t)1 << 36) &&
           (((uintptr_t)users | (uintptr_t)items) & 15) == 0;
}

// full 64-item tiles on the persistent kernel; the (< 64)-item tail on the generic tile kernel
static int launch_score_persistent(hipStream_t s, const float* users, int64_t U, int D, const float* items, int64_t N,
                                   float* scores, int64_t ldc) {
    const unsigned grid = CDR_NUM_CU;      // one resident workgroup per CU, 32 per XCD
    const int NT = (int)(N / 64);
    const bool small = U <= 64;            // one 32-row tile per wave (BM = 64) instead of two (BM = 128)
    if (D == 64) {
        const size_t lds = 2 * (size_t)64 * (64 + 4) * sizeof(float);
        if (small) score_persistent_kernel<1, 64, false><<<dim3(grid), dim3(256), lds, s>>>(users, (int)U, items, NT, scores, ldc, topk_out{});
        else score_persistent_kernel<2, 64, false><<<dim3(grid), dim3(256), lds, s>>>(users, (int)U, items, NT, scores, ldc, topk_out{});
    } else {
        const size_t lds = 2 * (size_t)64 * (128 + 4) * sizeof(float);
        if (small) score_persistent_kernel<1, 128, false><<<dim3(grid), dim3(256), lds, s>>>(users, (int)U, items, NT, scores, ldc, topk_out{});
        else score_persistent_kernel<2, 128, false><<<dim3(grid), dim3(256), lds, s>>>(users, (int)U, items, NT, scores, ldc, topk_out{});
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cdr_set_error("score_persistent: launch failed: %s", hipGetErrorString(e)); return (int)e; }
    const int64_t done = (int64_t)NT * 64;
    if (done < N)
        return launch<false, true, false>(s, U, N - done, D, users, D, items + done * D, D, scores + done, ldc, nullptr,
                                          CDR_ACT_NONE, 0, nullptr, nullptr);
    return CDR_OK;
}

// row squared norms: out[r] = sum_d X[r,d]^2  (one wave per row)
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* __restrict__ X, int64_t rows, int D, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), TW = (int64_t)gridDim.x * 4;
    for (int64_t r = w; r < rows; r += TW) {
        float s = 0.f;
        for (int c = lane; c < D; c += 64) { const float v = X[r * D + c]; s += v * v; }
        s = group_sum<64>(s);
        if (lane == 0) out[r] = s;
    }
}

}  // namespace

extern "C" int cdr_gemm_f32_ex(void* stream, int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A,
                               int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias,
                               const float* rowscale, int act, int accumulate) {
    CDR_CHECK_ARG(A && B && C);
    CDR_CHECK_ARG(M > 0 && N > 0 && K > 0);
    CDR_CHECK_ARG(act >= CDR_ACT_NONE && act <= CDR_ACT_SIGMOID);
    CDR_CHECK_ARG(accumulate >= 0 && accumulate <= 2);
    CDR_CHECK_ARG(((M + 127) / 128) * ((N + 127) / 128) < (int64_t)1 << 31);
    hipStream_t s = (hipStream_t)stream;
    if (!transA && transB) return launch<false, true, false>(s, M, N, K, A, lda, B, ldb, C, ldc, bias, act, accumulate, nullptr, nullptr, rowscale);
    if (!transA && !transB) return launch<false, false, false>(s, M, N, K, A, lda, B, ldb, C, ldc, bias, act, accumulate, nullptr, nullptr, rowscale);
    if (transA && !transB) return launch<true, false, false>(s, M, N, K, A, lda, B, ldb, C, ldc, bias, act, accumulate, nullptr, nullptr, rowscale);
    return launch<true, true, false>(s, M, N, K, A, lda, B, ldb, C, ldc, bias, act, accumulate, nullptr, nullptr, rowscale);
}

extern "C" int cdr_gemm_f32(void* stream, int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A,
                            int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias, int act,
                            int accumulate) {
    return cdr_gemm_f32_ex(stream, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, nullptr, act, accumulate);
}

extern "C" int cdr_fullsort_scores_f32(void* stream, const float* user_e, int64_t U, int D, const float* slab0, int64_t n0,
                                       const float* slab1, int64_t n1, float* scores) {
    CDR_CHECK_ARG(user_e && scores && U > 0 && D > 0);
    CDR_CHECK_ARG((slab0 && n0 > 0) || (slab1 && n1 > 0));
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = (slab0 ? n0 : 0) + (slab1 ? n1 : 0);
    int rc = CDR_OK;
    int64_t off = 0;
    if (slab0 && n0 > 0) {
        rc = gemv_ok(U, D, user_e, slab0) ? gemv_dispatch(s, user_e, (int)U, D, slab0, n0, scores, N)
             : score_persistent_ok(U, D, n0, user_e, slab0) ? launch_score_persistent(s, user_e, U, D, slab0, n0, scores, N)
             : launch<false, true, false>(s, U, n0, D, user_e, D, slab0, D, scores, N, nullptr, CDR_ACT_NONE, 0, nullptr, nullptr);
        if (rc) return rc;
        off = n0;
    }
    if (slab1 && n1 > 0)
        rc = gemv_ok(U, D, user_e, slab1) ? gemv_dispatch(s, user_e, (int)U, D, slab1, n1, scores + off, N)
             : score_persistent_ok(U, D, n1, user_e, slab1) ? launch_score_persistent(s, user_e, U, D, slab1, n1, scores + off, N)
             : launch<false, true, false>(s, U, n1, D, user_e, D, slab1, D, scores + off, N, nullptr, CDR_ACT_NONE, 0, nullptr, nullptr);
    return rc;
}

// ---- mask + top-k fused after scoring ---------------------------------------------------------------------
namespace {

constexpr int64_t kTopkSubMax = 16384;              // columns per wave in topk_rows_kernel (fewer when U is small)
constexpr size_t kTopkScoreBytes = (size_t)256 << 20;   // score staging for the unfused passes

struct topk_plan {
    int64_t sub;                                    // columns per wave of topk_rows_kernel
    bool gemv[2];                                   // U <= 8: streaming GEMV with the top-k behind it (no score staging)
    int64_t gemv_blocks[2];
    bool fused[2];
    int64_t stripes[2], fused_cols[2];              // fused: producers and the columns they cover (multiple of 64)
    int64_t pass_cols;                              // unfused: columns scored per pass
    int64_t producers, score_floats;
};

// users up to which the fused mask + top-k runs one 32-row tile per wave (BM = 64: twice the row blocks, half the column stripes, so half
// the insertions -- round 6, U = 128 / 256 / 512 at D = 128: 5.62 -> 4.86, 8.78 -> 8.21, 14.96 -> 14.75 ms; 64 before); the rest of the comment:
// the lists that have to fill up from -inf); CDR_TOPK_SMALL_U overrides for A/B runs
static int64_t topk_small_u() {
    static const int64_t v = [] { const char* e = getenv("CDR_TOPK_SMALL_U"); return e ? (int64_t)atoll(e) : (int64_t)512; }();
    return v;
}

// `sqdist`: BM more floats, the user block's row norms.  (They never decide whether a slab is planned fused -- the limit below is passed
// at k = 49 with MT = 2, D = 128 in either form, 49 x 1,024 B being the step -- so one plan, and one workspace layout, serves both scores.)
static size_t fused_lds_bytes(int D, int MT, int k, bool sqdist = false) {
    const int BM = 64 * MT;
    return sizeof(float) * ((size_t)2 * 64 * (D + 4) + (size_t)BM * 65 + BM + (size_t)BM * k * 2 + (size_t)4 * kTopkQueue * 3 + 8 +
                            (sqdist ? BM : 0));
}

static topk_plan make_topk_plan(int64_t U, int D, const int64_t n[2], int k, const float* users, const float* const slab[2]) {
    topk_plan p{};
    // a wave walks its columns with 8 loads in flight: few users = few waves, so give each a shorter walk (U = 1, N = 10 M:
    // 2,442 waves of 8 iterations instead of 611 of 32)
    p.sub = U >= 16 ? kTopkSubMax : U >= 4 ? 8192 : 4096;
    const int64_t kTopkSub = p.sub;
    int64_t pass = (int64_t)(kTopkScoreBytes / sizeof(float)) / U;
    pass = pass / kTopkSub * kTopkSub;
    if (pass < kTopkSub) pass = kTopkSub;
    p.pass_cols = pass;
    int64_t max_unfused = 0;
    for (int i = 0; i < 2; ++i) {
        if (n[i] <= 0) continue;
        const int MT = U <= topk_small_u() ? 1 : 2;
        p.fused[i] = U > 32 && (D == 64 || D == 128) && n[i] >= 64 && U < ((int64_t)1 << 30) &&
                     (slab[i] == nullptr || ((((uintptr_t)users | (uintptr_t)slab[i]) & 15) == 0)) &&
                     fused_lds_bytes(D, MT, k) <= (size_t)160 * 1024;
        p.gemv[i] = !p.fused[i] && U <= 8 && (D & 3) == 0 && D >= 16 && D <= 256;
        if (p.gemv[i]) {
            const int64_t chunks = (n[i] + 255) / 256;
            p.gemv_blocks[i] = chunks < kGemvTopkBlocks ? chunks : kGemvTopkBlocks;
            p.producers += p.gemv_blocks[i];
        } else if (p.fused[i]) {
            const int BM = 64 * MT;
            const int64_t MB = (U + BM - 1) / BM, per_xcd = CDR_NUM_CU / 8;
            const int64_t MBc = MB < per_xcd ? MB : per_xcd;
            p.stripes[i] = 8 * (per_xcd / MBc);
            p.fused_cols[i] = n[i] / 64 * 64;
            p.producers += p.stripes[i];
            const int64_t tail = n[i] - p.fused_cols[i];
            if (tail > 0) { p.producers += 1; if (tail > max_unfused) max_unfused = tail; }
        } else {
            for (int64_t c = 0; c < n[i]; c += pass) {
                const int64_t cn = n[i] - c < pass ? n[i] - c : pass;
                p.producers += (cn + kTopkSub - 1) / kTopkSub;
                if (cn > max_unfused) max_unfused = cn;
            }
        }
    }
    p.score_floats = U * max_unfused;
    return p;
}

// level-0 lists (values + columns) | level-1 lists (one per kTopkMergeGroup level-0 lists) | score staging
static size_t topk_ws_bytes(const topk_plan& p, int64_t U, int k) {
    const int64_t l1 = (p.producers + kTopkMergeGroup - 1) / kTopkMergeGroup;
    return 2 * topk_part_bytes(p.producers, U, k) + 2 * topk_part_bytes(l1, U, k) + (((size_t)p.score_floats * 4 + 255) & ~(size_t)255);
}

// The score behind the top-k.  rown == nullptr: dot products.  Else SSCDR's distances from the squared row norms of the users and of the
// concatenated slabs (coln[global column]).
struct topk_epi { const float* rown; const float* coln; };

// one block of columns into the staging buffer, dot products or distances (`coln`: the block's first column)
static int score_block(hipStream_t s, const float* user_e, int64_t U, int D, const float* items, int64_t n, float* scores, int64_t ld,
                       const float* rown = nullptr, const float* coln = nullptr) {
    if (rown) return launch<false, true, true>(s, U, n, D, user_e, D, items, D, scores, ld, nullptr, CDR_ACT_NONE, 0, rown, coln);
    return gemv_ok(U, D, user_e, items) ? gemv_dispatch(s, user_e, (int)U, D, items, n, scores, ld)
           : score_persistent_ok(U, D, n, user_e, items) ? launch_score_persistent(s, user_e, U, D, items, n, scores, ld)
           : launch<false, true, false>(s, U, n, D, user_e, D, items, D, scores, ld, nullptr, CDR_ACT_NONE, 0, nullptr, nullptr);
}

}  // namespace

extern "C" int cdr_fullsort_topk_workspace_bytes(int64_t U, int D, int64_t n0, int64_t n1, int k, size_t* bytes) {
    CDR_CHECK_ARG(bytes && U > 0 && D > 0 && k >= 1 && k <= 64 && n0 >= 0 && n1 >= 0 && n0 + n1 > 0);
    const int64_t n[2] = {n0, n1};
    const float* const slab[2] = {nullptr, nullptr};
    *bytes = topk_ws_bytes(make_topk_plan(U, D, n, k, nullptr, slab), U, k);
    return CDR_OK;
}

// One top-k call over the slabs (`fn`: the entry it serves, for the error texts).  With `epi.rown` the score is the distance: the fused
// kernel's SQDIST instantiations, and the distance GEMM in front of topk_rows_kernel wherever the dot-product form stages scores.  The
// streaming GEMV has no distance form (its sums run in another order than the MFMA's: not the bits of cdr_fullsort_neg_sqdist_f32), and
// the plan gives its shapes no score staging: the distance entry refuses them before it comes here.
static int fullsort_topk_impl(const char* fn, const topk_epi& epi, void* stream, const float* user_e, int64_t U, int D, const float* slab0,
                              int64_t n0, const float* slab1, int64_t n1, int k, const int64_t* hist_indptr,
                              const int64_t* hist_cols, int exclude_first_col, float* out_vals, int64_t* out_idx,
                              void* workspace, size_t workspace_bytes, const float* seed, int64_t seed_stride) {
#define TOPK_CHECK_ARG(cond) do { if (!(cond)) { cdr_set_error("%s: invalid argument: %s", fn, #cond); return CDR_EINVAL; } } while (0)
    TOPK_CHECK_ARG(user_e && out_vals && out_idx && workspace && U > 0 && D > 0 && k >= 1 && k <= 64);
    TOPK_CHECK_ARG((slab0 && n0 > 0) || (slab1 && n1 > 0));
    TOPK_CHECK_ARG((hist_indptr == nullptr) == (hist_cols == nullptr));
    hipStream_t s = (hipStream_t)stream;
    const int64_t n[2] = {slab0 ? n0 : 0, slab1 ? n1 : 0};
    const float* const slab[2] = {slab0, slab1};
    TOPK_CHECK_ARG(n[0] + n[1] < ((int64_t)1 << 31) && n[0] + n[1] >= k);
#undef TOPK_CHECK_ARG
    // the workspace was sized without the pointers (alignment unknown): plan the same way, then demote unaligned slabs
    const float* const none[2] = {nullptr, nullptr};
    topk_plan p = make_topk_plan(U, D, n, k, nullptr, none);
    for (int i = 0; i < 2; ++i)
        if (p.fused[i] && ((((uintptr_t)user_e | (uintptr_t)slab[i]) & 15) != 0)) {
            cdr_set_error("%s: operands must be 16-byte aligned", fn);
            return CDR_EINVAL;
        }
    const size_t need = topk_ws_bytes(p, U, k);
    if (workspace_bytes < need) { cdr_set_error("%s: workspace %zu < %zu bytes", fn, workspace_bytes, need); return CDR_EINVAL; }
    const size_t part = topk_part_bytes(p.producers, U, k);
    const int64_t l1 = (p.producers + kTopkMergeGroup - 1) / kTopkMergeGroup;
    const size_t part1 = topk_part_bytes(l1, U, k);
    float* pv = (float*)workspace;
    int* pc = (int*)((char*)workspace + part);
    float* pv1 = (float*)((char*)workspace + 2 * part);
    int* pc1 = (int*)((char*)workspace + 2 * part + part1);
    float* sbuf = (float*)((char*)workspace + 2 * part + 2 * part1);
    const int64_t kTopkSub = p.sub;
    const topk_mask mk{hist_indptr, hist_cols, exclude_first_col};
    int64_t prod = 0, col_off = 0;
    for (int i = 0; i < 2; ++i) {
        if (n[i] <= 0) continue;
        if (p.gemv[i] && ((((uintptr_t)user_e | (uintptr_t)slab[i]) & 15) == 0)) {
            int rc = gemv_topk_dispatch(s, user_e, (int)U, D, slab[i], n[i], (int)col_off, k, mk, pv, pc, prod, (unsigned)p.gemv_blocks[i]);
            if (rc) return rc;
            prod += p.gemv_blocks[i];
        } else if (p.gemv[i]) {
            cdr_set_error("%s: operands must be 16-byte aligned", fn);
            return CDR_EINVAL;
        } else if (p.fused[i]) {
            topk_out_sq tk{};
            tk.k = k; tk.col_off = (int)col_off; tk.pv = pv + prod * U * k; tk.pc = pc + prod * U * k; tk.mk = mk;
            tk.seed = seed; tk.seed_stride = seed_stride;
            tk.rown = epi.rown; tk.coln = epi.rown ? epi.coln + col_off : nullptr;
            const int NT = (int)(n[i] / 64);
            const unsigned grid = CDR_NUM_CU;
            const bool small = U <= topk_small_u();
            const size_t lds = fused_lds_bytes(D, small ? 1 : 2, k, epi.rown != nullptr);
            if (epi.rown) {
                if (D == 64) {
                    if (small) score_persistent_kernel<1, 64, true, true><<<dim3(grid), dim3(256), lds, s>>>(user_e, (int)U, slab[i], NT, nullptr, 0, tk);
                    else score_persistent_kernel<2, 64, true, true><<<dim3(grid), dim3(256), lds, s>>>(user_e, (int)U, slab[i], NT, nullptr, 0, tk);
                } else {
                    if (small) score_persistent_kernel<1, 128, true, true><<<dim3(grid), dim3(256), lds, s>>>(user_e, (int)U, slab[i], NT, nullptr, 0, tk);
                    else score_persistent_kernel<2, 128, true, true><<<dim3(grid), dim3(256), lds, s>>>(user_e, (int)U, slab[i], NT, nullptr, 0, tk);
                }
            } else if (D == 64) {
                if (small) score_persistent_kernel<1, 64, true><<<dim3(grid), dim3(256), lds, s>>>(user_e, (int)U, slab[i], NT, nullptr, 0, tk);
                else score_persistent_kernel<2, 64, true><<<dim3(grid), dim3(256), lds, s>>>(user_e, (int)U, slab[i], NT, nullptr, 0, tk);
            } else {
                if (small) score_persistent_kernel<1, 128, true><<<dim3(grid), dim3(256), lds, s>>>(user_e, (int)U, slab[i], NT, nullptr, 0, tk);
                else score_persistent_kernel<2, 128, true><<<dim3(grid), dim3(256), lds, s>>>(user_e, (int)U, slab[i], NT, nullptr, 0, tk);
            }
            CDR_LAUNCH_CHECK();
            prod += p.stripes[i];
            const int64_t tail = n[i] - p.fused_cols[i];
            if (tail > 0) {
                const int64_t c = p.fused_cols[i];
                int rc = epi.rown ? score_block(s, user_e, U, D, slab[i] + c * D, tail, sbuf, tail, epi.rown, epi.coln + col_off + c)
                                  : launch<false, true, false>(s, U, tail, D, user_e, D, slab[i] + c * D, D, sbuf, tail, nullptr,
                                                               CDR_ACT_NONE, 0, nullptr, nullptr);
                if (rc) return rc;
                topk_rows_kernel<<<dim3((unsigned)((U + 3) / 4)), dim3(256), 0, s>>>(sbuf, tail, U, tail, tail, (int)(col_off + p.fused_cols[i]),
                                                                                    k, mk, pv, pc, prod);
                CDR_LAUNCH_CHECK();
                prod += 1;
            }
        } else {
            for (int64_t c = 0; c < n[i]; c += p.pass_cols) {
                const int64_t cn = n[i] - c < p.pass_cols ? n[i] - c : p.pass_cols;
                int rc = score_block(s, user_e, U, D, slab[i] + c * D, cn, sbuf, cn, epi.rown, epi.rown ? epi.coln + col_off + c : nullptr);
                if (rc) return rc;
                const int64_t chunks = (cn + kTopkSub - 1) / kTopkSub;
                topk_rows_kernel<<<dim3((unsigned)((U * chunks + 3) / 4)), dim3(256), 0, s>>>(sbuf, cn, U, cn, kTopkSub, (int)(col_off + c), k,
                                                                                             mk, pv, pc, prod);
                CDR_LAUNCH_CHECK();
                prod += chunks;
            }
        }
        col_off += n[i];
    }
    return topk_merge_launch(s, pv, pc, prod, U, k, pv1, pc1, out_vals, out_idx);
}

// Round 6: SEEDED thresholds.  Every column stripe of the fused kernel used to fill its k-entry lists from -inf: k ln(n_stripe / k)
// insertions per user and stripe (queue, mask test, LDS list update), 128 stripes at U = 256 -- the +31 % of the masked top-10 over plain
// scoring there.  A first call over a SAMPLE of the columns (the first 65,536 of the first slab, same mask) leaves each user's k-th value
// over the sample in out_vals[:, k - 1]: a lower bound of the final k-th value (the sample is a subset of the columns), handed to the real
// call as the starting threshold of every stripe (one float below it, so that ties with it still enter).  Results are unchanged -- every
// entry of the final top-k is >= its user's seed and passes in its own stripe; a stripe's list may end up shorter than k, which the
// merges already handle (-inf / -1 fillers never enter).
constexpr int64_t kTopkSeedCols = 65536;
// The sample is a subset of the columns whatever the score is, so the distance entry shares the driver.
static int fullsort_topk_seeded(const char* fn, const topk_epi& epi, void* stream, const float* user_e, int64_t U, int D, const float* slab0,
                                int64_t n0, const float* slab1, int64_t n1, int k, const int64_t* hist_indptr,
                                const int64_t* hist_cols, int exclude_first_col, float* out_vals, int64_t* out_idx,
                                void* workspace, size_t workspace_bytes) {
    static const bool seeding = [] { const char* e = getenv("CDR_TOPK_SEED"); return !(e && e[0] == '0'); }();
    const bool first0 = slab0 && n0 > 0;
    const float* fs = first0 ? slab0 : slab1;
    const int64_t fn_cols = first0 ? n0 : n1;
    if (seeding && fs && U > 32 && (D == 64 || D == 128) && fn_cols >= 16 * kTopkSeedCols && k <= kTopkSeedCols / 64 &&
        ((((uintptr_t)user_e | (uintptr_t)fs) & 15) == 0)) {
        // the sample call: same users, same mask, the first columns of the first slab (global columns [0, kTopkSeedCols))
        int rc = fullsort_topk_impl(fn, epi, stream, user_e, U, D, fs, kTopkSeedCols, nullptr, 0, k, hist_indptr, hist_cols, exclude_first_col, out_vals,
                                    out_idx, workspace, workspace_bytes, nullptr, 0);
        if (rc) return rc;
        return fullsort_topk_impl(fn, epi, stream, user_e, U, D, slab0, n0, slab1, n1, k, hist_indptr, hist_cols, exclude_first_col, out_vals, out_idx,
                                  workspace, workspace_bytes, out_vals + (k - 1), k);
    }
    return fullsort_topk_impl(fn, epi, stream, user_e, U, D, slab0, n0, slab1, n1, k, hist_indptr, hist_cols, exclude_first_col, out_vals, out_idx,
                              workspace, workspace_bytes, nullptr, 0);
}

extern "C" int cdr_fullsort_topk_f32(void* stream, const float* user_e, int64_t U, int D, const float* slab0, int64_t n0,
                                     const float* slab1, int64_t n1, int k, const int64_t* hist_indptr,
                                     const int64_t* hist_cols, int exclude_first_col, float* out_vals, int64_t* out_idx,
                                     void* workspace, size_t workspace_bytes) {
    return fullsort_topk_seeded(__func__, topk_epi{nullptr, nullptr}, stream, user_e, U, D, slab0, n0, slab1, n1, k, hist_indptr, hist_cols,
                                exclude_first_col, out_vals, out_idx, workspace, workspace_bytes);
}

static int row_sqnorm_launch(hipStream_t s, const float* X, int64_t rows, int D, float* out) {
    row_sqnorm_kernel<<<dim3((unsigned)((rows + 3) / 4 > 2048 ? 2048 : (rows + 3) / 4)), dim3(256), 0, s>>>(X, rows, D, out);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

extern "C" int cdr_row_sqnorm_f32(void* stream, const float* X, int64_t rows, int D, float* out) {
    CDR_CHECK_ARG(X && out && rows > 0 && D > 0);
    return row_sqnorm_launch((hipStream_t)stream, X, rows, D, out);
}

extern "C" int cdr_fullsort_neg_sqdist_f32(void* stream, const float* user_e, int64_t U, int D, const float* items,
                                           int64_t N, float* norm_scratch, float* scores) {
    CDR_CHECK_ARG(user_e && items && scores && norm_scratch && U > 0 && N > 0 && D > 0);
    hipStream_t s = (hipStream_t)stream;
    float* rown = norm_scratch;
    float* coln = norm_scratch + U;
    if (int rc = row_sqnorm_launch(s, user_e, U, D, rown)) return rc;
    if (int rc = row_sqnorm_launch(s, items, N, D, coln)) return rc;
    return launch<false, true, true>(s, U, N, D, user_e, D, items, D, scores, N, nullptr, CDR_ACT_NONE, 0, rown, coln);
}

// ---- SSCDR's distances under the fused mask + top-k --------------------------------------------------------------------------------
// workspace = the dot-product entry's (same plan, same lists) | user row norms [U] | column norms [n0 + n1]
static size_t sqdist_norm_bytes(int64_t U, int64_t N) { return ((size_t)4 * (size_t)(U + N) + 255) & ~(size_t)255; }

extern "C" int cdr_fullsort_neg_sqdist_topk_workspace_bytes(int64_t U, int D, int64_t n0, int64_t n1, int k, size_t* bytes) {
    CDR_CHECK_ARG(bytes && U > 0 && D > 0 && k >= 1 && k <= 64 && n0 >= 0 && n1 >= 0 && n0 + n1 > 0);
    const int64_t n[2] = {n0, n1};
    const float* const slab[2] = {nullptr, nullptr};
    *bytes = topk_ws_bytes(make_topk_plan(U, D, n, k, nullptr, slab), U, k) + sqdist_norm_bytes(U, n0 + n1);
    return CDR_OK;
}

extern "C" int cdr_fullsort_neg_sqdist_topk_f32(void* stream, const float* user_e, int64_t U, int D, const float* slab0, int64_t n0,
                                                const float* slab1, int64_t n1, const float* col_sqnorm, int k,
                                                const int64_t* hist_indptr, const int64_t* hist_cols, int exclude_first_col,
                                                float* out_vals, int64_t* out_idx, void* workspace, size_t workspace_bytes) {
    CDR_CHECK_ARG(user_e && out_vals && out_idx && workspace && U > 0 && D > 0 && k >= 1 && k <= 64);
    CDR_CHECK_ARG((slab0 && n0 > 0) || (slab1 && n1 > 0));
    hipStream_t s = (hipStream_t)stream;
    const int64_t n[2] = {slab0 ? n0 : 0, slab1 ? n1 : 0};
    CDR_CHECK_ARG(n[0] >= 0 && n[1] >= 0 && n[0] + n[1] < ((int64_t)1 << 31));
    const float* const none[2] = {nullptr, nullptr};
    const topk_plan p = make_topk_plan(U, D, n, k, nullptr, none);
    const size_t lists = topk_ws_bytes(p, U, k), need = lists + sqdist_norm_bytes(U, n[0] + n[1]);
    if (workspace_bytes < need) { cdr_set_error("%s: workspace %zu < %zu bytes", __func__, workspace_bytes, need); return CDR_EINVAL; }
    CDR_CHECK_ARG((hist_indptr == nullptr) == (hist_cols == nullptr));
    CDR_CHECK_ARG(n[0] + n[1] >= k);
    for (int i = 0; i < 2; ++i)
        if (p.fused[i] && ((((uintptr_t)user_e | (uintptr_t)(i ? slab1 : slab0)) & 15) != 0)) {
            cdr_set_error("%s: operands must be 16-byte aligned", __func__);
            return CDR_EINVAL;
        }
    if (p.gemv[0] || p.gemv[1]) {          // (fullsort_topk_impl says why)
        cdr_set_error("%s: U = %lld <= 8 users has no top-k form for distances (score them with cdr_fullsort_neg_sqdist_f32)", __func__, (long long)U);
        return CDR_EINVAL;
    }
    float* rown = (float*)((char*)workspace + lists);
    float* coln = rown + U;
    if (int rc = row_sqnorm_launch(s, user_e, U, D, rown)) return rc;
    if (!col_sqnorm) {
        if (n[0] > 0) { if (int rc = row_sqnorm_launch(s, slab0, n[0], D, coln)) return rc; }
        if (n[1] > 0) { if (int rc = row_sqnorm_launch(s, slab1, n[1], D, coln + n[0])) return rc; }
    }
    return fullsort_topk_seeded(__func__, topk_epi{rown, col_sqnorm ? col_sqnorm : coln}, stream, user_e, U, D, slab0, n0, slab1, n1, k, hist_indptr,
                                hist_cols, exclude_first_col, out_vals, out_idx, workspace, lists);
}

// ---- rank of the ground-truth positives over the masked catalogue ------------------------------------------------------------------
// What the evaluation metrics beyond a top-k list of <= 64 entries need (any k, MAP, GAUC) without the [U, N] matrix: the scores are formed
// in column passes into the workspace staging by score_block -- the launches cdr_fullsort_scores_f32 (respectively
// cdr_fullsort_neg_sqdist_f32) makes for the same columns: passes start at a multiple of 64 columns of their slab, so whole tiles and
// the slab's tail fall to the same kernels, and the counted scores are the bits of S -- and counted by rank_rows_kernel (cdr_rank.h).  The
// thresholds come from a first walk over the same passes (rank_gather_kernel picks pos_score out of the staging); a catalogue that fits
// one pass is scored once.
#include "cdr_rank.h"

namespace {

static int64_t rank_pass_cols(int64_t U) {
    int64_t pass = (int64_t)(kTopkScoreBytes / sizeof(float)) / U / 64 * 64;
    return pass < 64 ? 64 : pass;
}

static size_t rank_ws_bytes(int64_t U, const int64_t n[2]) {
    const int64_t pass = rank_pass_cols(U);
    int64_t cols = 0;
    for (int i = 0; i < 2; ++i) {
        const int64_t c = n[i] < pass ? n[i] : pass;
        if (c > cols) cols = c;
    }
    return ((size_t)U * (size_t)cols * sizeof(float) + 255) & ~(size_t)255;
}

static int fullsort_rank_impl(const char* fn, const topk_epi& epi, hipStream_t s, const float* user_e, int64_t U, int D,
                              const float* const slab[2], const int64_t n[2], const int64_t* pos_indptr, const int64_t* pos_cols,
                              const topk_mask& mk, float* pos_score, int32_t* gt, int32_t* eq, int32_t* eq_before, int32_t* n_unmasked,
                              float* sbuf) {
    const int64_t pass = rank_pass_cols(U);
    int64_t passes = 0;
    for (int i = 0; i < 2; ++i) passes += (n[i] + pass - 1) / pass;
    if (int rc = rank_init_launch(s, 0, U, pos_indptr, pos_cols, mk, pos_score, gt, eq, eq_before, n_unmasked)) return rc;
    for (int walk = 0; walk < 2; ++walk) {              // walk 0: the thresholds; walk 1: the counts
        if (walk == 1)
            if (int rc = rank_init_launch(s, 1, U, pos_indptr, pos_cols, mk, pos_score, gt, eq, eq_before, n_unmasked)) return rc;
        int64_t col_off = 0;
        for (int i = 0; i < 2; ++i) {
            for (int64_t c = 0; c < n[i]; c += pass) {
                const int64_t cn = n[i] - c < pass ? n[i] - c : pass;
                if (walk == 0 || passes > 1) {
                    int rc = score_block(s, user_e, U, D, slab[i] + c * D, cn, sbuf, cn, epi.rown, epi.rown ? epi.coln + col_off + c : nullptr);
                    if (rc) return rc;
                }
                int rc = walk == 0 ? rank_gather_launch(s, sbuf, cn, U, cn, col_off + c, pos_indptr, pos_cols, pos_score)
                                   : rank_rows_launch(s, sbuf, cn, U, cn, col_off + c, pos_indptr, pos_cols, mk, pos_score, gt, eq, eq_before,
                                                      n_unmasked);
                if (rc) return rc;
            }
            col_off += n[i];
        }
    }
    (void)fn;
    return CDR_OK;
}

}  // namespace

#define CDR_RANK_CHECK_COMMON()                                                                                         \
    CDR_CHECK_ARG(user_e && workspace && U > 0 && U < ((int64_t)1 << 30) && D > 0);                                     \
    CDR_CHECK_ARG((slab0 && n0 > 0) || (slab1 && n1 > 0));                                                              \
    CDR_CHECK_ARG(pos_indptr && pos_cols && pos_score && gt && eq && eq_before && n_unmasked);                          \
    CDR_CHECK_ARG((hist_indptr == nullptr) == (hist_cols == nullptr));                                                  \
    const int64_t n[2] = {slab0 ? (n0 > 0 ? n0 : 0) : 0, slab1 ? (n1 > 0 ? n1 : 0) : 0};                                \
    const float* const slab[2] = {slab0, slab1};                                                                        \
    CDR_CHECK_ARG(n[0] + n[1] < ((int64_t)1 << 31))

extern "C" int cdr_fullsort_rank_workspace_bytes(int64_t U, int D, int64_t n0, int64_t n1, int64_t P, size_t* bytes) {
    CDR_CHECK_ARG(bytes && U > 0 && U < ((int64_t)1 << 30) && D > 0 && n0 >= 0 && n1 >= 0 && n0 + n1 > 0 && P >= 0);
    const int64_t n[2] = {n0, n1};
    *bytes = rank_ws_bytes(U, n);
    return CDR_OK;
}

extern "C" int cdr_fullsort_rank_f32(void* stream, const float* user_e, int64_t U, int D, const float* slab0, int64_t n0,
                                     const float* slab1, int64_t n1, const int64_t* pos_indptr, const int64_t* pos_cols,
                                     const int64_t* hist_indptr, const int64_t* hist_cols, int exclude_first_col, float* pos_score,
                                     int32_t* gt, int32_t* eq, int32_t* eq_before, int32_t* n_unmasked, void* workspace,
                                     size_t workspace_bytes) {
    CDR_RANK_CHECK_COMMON();
    const size_t need = rank_ws_bytes(U, n);
    if (workspace_bytes < need) { cdr_set_error("%s: workspace %zu < %zu bytes", __func__, workspace_bytes, need); return CDR_EINVAL; }
    return fullsort_rank_impl(__func__, topk_epi{nullptr, nullptr}, (hipStream_t)stream, user_e, U, D, slab, n, pos_indptr, pos_cols,
                              topk_mask{hist_indptr, hist_cols, exclude_first_col}, pos_score, gt, eq, eq_before, n_unmasked, (float*)workspace);
}

extern "C" int cdr_fullsort_neg_sqdist_rank_workspace_bytes(int64_t U, int D, int64_t n0, int64_t n1, int64_t P, size_t* bytes) {
    CDR_CHECK_ARG(bytes && U > 0 && U < ((int64_t)1 << 30) && D > 0 && n0 >= 0 && n1 >= 0 && n0 + n1 > 0 && P >= 0);
    const int64_t n[2] = {n0, n1};
    *bytes = rank_ws_bytes(U, n) + sqdist_norm_bytes(U, n0 + n1);
    return CDR_OK;
}

extern "C" int cdr_fullsort_neg_sqdist_rank_f32(void* stream, const float* user_e, int64_t U, int D, const float* slab0, int64_t n0,
                                                const float* slab1, int64_t n1, const float* col_sqnorm, const int64_t* pos_indptr,
                                                const int64_t* pos_cols, const int64_t* hist_indptr, const int64_t* hist_cols,
                                                int exclude_first_col, float* pos_score, int32_t* gt, int32_t* eq, int32_t* eq_before,
                                                int32_t* n_unmasked, void* workspace, size_t workspace_bytes) {
    CDR_RANK_CHECK_COMMON();
    const size_t staging = rank_ws_bytes(U, n), need = staging + sqdist_norm_bytes(U, n[0] + n[1]);
    if (workspace_bytes < need) { cdr_set_error("%s: workspace %zu < %zu bytes", __func__, workspace_bytes, need); return CDR_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    float* rown = (float*)((char*)workspace + staging);
    float* coln = rown + U;
    if (int rc = row_sqnorm_launch(s, user_e, U, D, rown)) return rc;
    if (!col_sqnorm) {
        if (n[0] > 0) { if (int rc = row_sqnorm_launch(s, slab0, n[0], D, coln)) return rc; }
        if (n[1] > 0) { if (int rc = row_sqnorm_launch(s, slab1, n[1], D, coln + n[0])) return rc; }
    }
    return fullsort_rank_impl(__func__, topk_epi{rown, col_sqnorm ? col_sqnorm : coln}, s, user_e, U, D, slab, n, pos_indptr, pos_cols,
                              topk_mask{hist_indptr, hist_cols, exclude_first_col}, pos_score, gt, eq, eq_before, n_unmasked, (float*)workspace);
}
#undef CDR_RANK_CHECK_COMMON

extern "C" int cdr_rank_rows_f32(void* stream, const float* scores, int64_t ld, int64_t U, int64_t N, int64_t col_off,
                                 const int64_t* pos_indptr, const int64_t* pos_cols, const int64_t* hist_indptr, const int64_t* hist_cols,
                                 int exclude_first_col, const float* pos_score, int32_t* gt, int32_t* eq, int32_t* eq_before,
                                 int32_t* n_unmasked, int accumulate) {
    CDR_CHECK_ARG(scores && U > 0 && N > 0 && ld >= N && col_off >= 0 && col_off + N < ((int64_t)1 << 31));
    CDR_CHECK_ARG(pos_indptr && pos_cols && pos_score && gt && eq && eq_before && n_unmasked);
    CDR_CHECK_ARG((hist_indptr == nullptr) == (hist_cols == nullptr));
    hipStream_t s = (hipStream_t)stream;
    const topk_mask mk{hist_indptr, hist_cols, exclude_first_col};
    if (!accumulate)
        if (int rc = rank_init_launch(s, 1, U, pos_indptr, pos_cols, mk, const_cast<float*>(pos_score), gt, eq, eq_before, n_unmasked)) return rc;
    return rank_rows_launch(s, scores, ld, U, N, col_off, pos_indptr, pos_cols, mk, pos_score, gt, eq, eq_before, n_unmasked);
}

// ---- mask + top-k lists beyond one wave (k <= 1024) over the masked catalogue -------------------------------------------------------
// The rank route's walk with a selection in place of the count: the same column passes through score_block into the same staging (so the
// listed values are the bits of S), each pass selected by wide_topk_launch (cdr_topk_wide.h) and merged into the running lists in
// out_vals / out_idx, whose last entry is the next pass's starting threshold.  One walk: nothing has to be known before it.
#include "cdr_topk_wide.h"

namespace {

// the columns of the longest pass (what rank_ws_bytes sizes the staging for)
static int64_t wide_pass_max(int64_t U, const int64_t n[2]) {
    const int64_t pass = rank_pass_cols(U);
    int64_t cols = 0;
    for (int i = 0; i < 2; ++i) {
        const int64_t c = n[i] < pass ? n[i] : pass;
        if (c > cols) cols = c;
    }
    return cols;
}

static int fullsort_topk_wide_impl(const topk_epi& epi, hipStream_t s, const float* user_e, int64_t U, int D, const float* const slab[2],
                                   const int64_t n[2], int k, const topk_mask& mk, float* out_vals, int64_t* out_idx, float* sbuf,
                                   unsigned long long* part) {
    const int64_t pass = rank_pass_cols(U);
    int64_t col_off = 0;
    int accumulate = 0;
    for (int i = 0; i < 2; ++i) {
        for (int64_t c = 0; c < n[i]; c += pass) {
            const int64_t cn = n[i] - c < pass ? n[i] - c : pass;
            if (int rc = score_block(s, user_e, U, D, slab[i] + c * D, cn, sbuf, cn, epi.rown, epi.rown ? epi.coln + col_off + c : nullptr)) return rc;
            if (int rc = wide_topk_launch(s, sbuf, cn, U, cn, col_off + c, k, mk, out_vals, out_idx, accumulate, part)) return rc;
            accumulate = 1;
        }
        col_off += n[i];
    }
    return CDR_OK;
}

}  // namespace

#define CDR_WIDE_CHECK_SIZES()                                                                                          \
    CDR_CHECK_ARG(bytes && U > 0 && U < ((int64_t)1 << 30) && D > 0 && k >= 1 && k <= kWideMaxK);                       \
    CDR_CHECK_ARG(n0 >= 0 && n1 >= 0 && n0 + n1 > 0 && n0 + n1 < ((int64_t)1 << 31));                                   \
    const int64_t n[2] = {n0, n1}

#define CDR_WIDE_CHECK_COMMON()                                                                                         \
    CDR_CHECK_ARG(user_e && out_vals && out_idx && workspace && U > 0 && U < ((int64_t)1 << 30) && D > 0);              \
    CDR_CHECK_ARG(k >= 1 && k <= kWideMaxK);                                                                            \
    CDR_CHECK_ARG((slab0 && n0 > 0) || (slab1 && n1 > 0));                                                              \
    CDR_CHECK_ARG((hist_indptr == nullptr) == (hist_cols == nullptr));                                                  \
    const int64_t n[2] = {slab0 ? (n0 > 0 ? n0 : 0) : 0, slab1 ? (n1 > 0 ? n1 : 0) : 0};                                \
    const float* const slab[2] = {slab0, slab1};                                                                        \
    CDR_CHECK_ARG(n[0] + n[1] < ((int64_t)1 << 31))

extern "C" int cdr_fullsort_topk_wide_workspace_bytes(int64_t U, int D, int64_t n0, int64_t n1, int k, size_t* bytes) {
    CDR_WIDE_CHECK_SIZES();
    *bytes = rank_ws_bytes(U, n) + wide_part_bytes(U, wide_pass_max(U, n), k);
    return CDR_OK;
}

extern "C" int cdr_fullsort_topk_wide_f32(void* stream, const float* user_e, int64_t U, int D, const float* slab0, int64_t n0,
                                          const float* slab1, int64_t n1, int k, const int64_t* hist_indptr, const int64_t* hist_cols,
                                          int exclude_first_col, float* out_vals, int64_t* out_idx, void* workspace,
                                          size_t workspace_bytes) {
    CDR_WIDE_CHECK_COMMON();
    const size_t staging = rank_ws_bytes(U, n), need = staging + wide_part_bytes(U, wide_pass_max(U, n), k);
    if (workspace_bytes < need) { cdr_set_error("%s: workspace %zu < %zu bytes", __func__, workspace_bytes, need); return CDR_EINVAL; }
    return fullsort_topk_wide_impl(topk_epi{nullptr, nullptr}, (hipStream_t)stream, user_e, U, D, slab, n, k,
                                   topk_mask{hist_indptr, hist_cols, exclude_first_col}, out_vals, out_idx, (float*)workspace,
                                   (unsigned long long*)((char*)workspace + staging));
}

extern "C" int cdr_fullsort_neg_sqdist_topk_wide_workspace_bytes(int64_t U, int D, int64_t n0, int64_t n1, int k, size_t* bytes) {
    CDR_WIDE_CHECK_SIZES();
    *bytes = rank_ws_bytes(U, n) + wide_part_bytes(U, wide_pass_max(U, n), k) + sqdist_norm_bytes(U, n0 + n1);
    return CDR_OK;
}

extern "C" int cdr_fullsort_neg_sqdist_topk_wide_f32(void* stream, const float* user_e, int64_t U, int D, const float* slab0, int64_t n0,
                                                     const float* slab1, int64_t n1, const float* col_sqnorm, int k,
                                                     const int64_t* hist_indptr, const int64_t* hist_cols, int exclude_first_col,
                                                     float* out_vals, int64_t* out_idx, void* workspace, size_t workspace_bytes) {
    CDR_WIDE_CHECK_COMMON();
    const size_t staging = rank_ws_bytes(U, n), lists = wide_part_bytes(U, wide_pass_max(U, n), k);
    const size_t need = staging + lists + sqdist_norm_bytes(U, n[0] + n[1]);
    if (workspace_bytes < need) { cdr_set_error("%s: workspace %zu < %zu bytes", __func__, workspace_bytes, need); return CDR_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    float* rown = (float*)((char*)workspace + staging + lists);
    float* coln = rown + U;
    if (int rc = row_sqnorm_launch(s, user_e, U, D, rown)) return rc;
    if (!col_sqnorm) {
        if (n[0] > 0) { if (int rc = row_sqnorm_launch(s, slab0, n[0], D, coln)) return rc; }
        if (n[1] > 0) { if (int rc = row_sqnorm_launch(s, slab1, n[1], D, coln + n[0])) return rc; }
    }
    return fullsort_topk_wide_impl(topk_epi{rown, col_sqnorm ? col_sqnorm : coln}, s, user_e, U, D, slab, n, k,
                                   topk_mask{hist_indptr, hist_cols, exclude_first_col}, out_vals, out_idx, (float*)workspace,
                                   (unsigned long long*)((char*)workspace + staging));
}
#undef CDR_WIDE_CHECK_SIZES
#undef CDR_WIDE_CHECK_COMMON

extern "C" int cdr_topk_rows_workspace_bytes(int64_t U, int64_t N, int k, size_t* bytes) {
    CDR_CHECK_ARG(bytes && U > 0 && U < ((int64_t)1 << 30) && N > 0 && N < ((int64_t)1 << 31) && k >= 1 && k <= kWideMaxK);
    *bytes = wide_part_bytes(U, N, k);
    return CDR_OK;
}

extern "C" int cdr_topk_rows_f32(void* stream, const float* scores, int64_t ld, int64_t U, int64_t N, int64_t col_off, int k,
                                 const int64_t* hist_indptr, const int64_t* hist_cols, int exclude_first_col, float* vals, int64_t* idx,
                                 int accumulate, void* workspace, size_t workspace_bytes) {
    CDR_CHECK_ARG(scores && vals && idx && workspace && U > 0 && U < ((int64_t)1 << 30) && N > 0 && ld >= N);
    CDR_CHECK_ARG(k >= 1 && k <= kWideMaxK && col_off >= 0 && col_off + N < ((int64_t)1 << 31));
    CDR_CHECK_ARG((hist_indptr == nullptr) == (hist_cols == nullptr));
    const size_t need = wide_part_bytes(U, N, k);
    if (workspace_bytes < need) { cdr_set_error("%s: workspace %zu < %zu bytes", __func__, workspace_bytes, need); return CDR_EINVAL; }
    return wide_topk_launch((hipStream_t)stream, scores, ld, U, N, col_off, k, topk_mask{hist_indptr, hist_cols, exclude_first_col}, vals,
                            idx, accumulate ? 1 : 0, (unsigned long long*)workspace);
}
