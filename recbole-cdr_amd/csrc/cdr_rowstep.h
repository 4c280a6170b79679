// What the row-wise forward kernels with dense weights share (cdr_clfm.hip, cdr_dtcdr.hip, cdr_deepapf.hip, cdr_dcdcsr.hip): a workgroup
// of four waves walks row tiles of 32 batch rows under a persistent grid, keeps its parameter gradients in MFMA accumulators across its
// tiles and writes them once, as the workgroup's partial [grid][n_elem]; one finishing launch adds the partials in workgroup order (no
// float atomics: a rerun is bit-equal) and turns the fp64 block partials of the loss sums into out8.
#pragma once
#include "cdr_common.h"
#include "cdr_loss_math.h"
#include "cdr_mfma.h"

namespace {

constexpr int kRows = 32;                    // batch rows of a tile = M of the MFMA
constexpr int kLdsPad = 4;                   // floats: a row stride of 4 (mod 32) keeps the float4 reads of 32 consecutive rows apart
constexpr int kSub = kBlock / kRows;         // lanes per row in the staging and epilogue phases (8)
constexpr size_t kLdsPerCu = 160 * 1024;

__host__ __device__ inline int pad32(int d) { return (d + 31) & ~31; }

// STORE_TILE32(dst, off, ld, ti, tj, out, in, acc, li, lh): a wave's 32x32 accumulator tile (ti, tj) into the packed [out][in] matrix
// with row stride ld at dst + off.  A macro, not a function: as a force-inlined function (arguments by value or by reference) the
// compiler reads off / ld once instead of per store and the forward kernels' code changes; textual substitution keeps it as it was.
#define STORE_TILE32(dst, off, ld, ti, tj, out, in, acc, li, lh)                                                    \
    do {                                                                                                            \
        const int cin_ = (tj) * 32 + (li);                                                                          \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                         \
            const int ro_ = (ti) * 32 + (r_ & 3) + 8 * (r_ >> 2) + 4 * (lh);                                        \
            if (ro_ < (out) && cin_ < (in)) (dst)[(off) + ro_ * (ld) + cin_] = (acc)[r_];                           \
        }                                                                                                           \
    } while (0)

// out8 = {w bce, bce, 0, ...}
struct rowstep_bce {
    static constexpr int N = 1;
    int64_t B;
    float weight;
    __device__ void write(const double* acc, float* out8) const {
        const float bce = (float)(acc[0] / (double)B);
        out8[0] = weight * bce;
        out8[1] = bce;
        for (int i = 2; i < 8; ++i) out8[i] = 0.f;
    }
};

// out8 = {w (bce + reg (nU + nI) / B), bce, (nU + nI) / B, nU, nI, c_u, c_i, 0} with c = w reg / (B norm) (0 for a zero norm, as
// step_finish_kernel)
struct rowstep_bce_emb {
    static constexpr int N = 3;
    int64_t B;
    float weight, reg_weight;
    __device__ void write(const double* acc, float* out8) const {
        const float bce = (float)(acc[0] / (double)B);
        const float nu = (float)sqrt(acc[1]), ni = (float)sqrt(acc[2]);
        const float emb = (nu + ni) / (float)B;
        out8[0] = weight * (bce + reg_weight * emb);
        out8[1] = bce; out8[2] = emb; out8[3] = nu; out8[4] = ni;
        out8[5] = weight * embloss_coef(reg_weight, B, nu);
        out8[6] = weight * embloss_coef(reg_weight, B, ni);
        out8[7] = 0.f;
    }
};

// out8 = {sum / count, 0, ...}
struct rowstep_mean {
    static constexpr int N = 1;
    double count;
    __device__ void write(const double* acc, float* out8) const {
        out8[0] = (float)(acc[0] / count);
        for (int i = 1; i < 8; ++i) out8[i] = 0.f;
    }
};

// Block 0: out8 from the fp64 block partials.  Blocks 1..: one thread per parameter adds the workgroups' partials in workgroup order.
template <class Epilogue>
__global__ __launch_bounds__(kBlock) void rowstep_finish_kernel(const double* __restrict__ partials, int nblocks, const Epilogue ep,
                                                                float* __restrict__ out8, const float* __restrict__ part, int n_elem,
                                                                float* __restrict__ dparams) {
    if (blockIdx.x == 0) {
        __shared__ double smem[Epilogue::N * (kBlock / 64)];
        double acc[Epilogue::N] = {};
        sum_partials<Epilogue::N, kBlock>(partials, nblocks, acc, smem);
        if (threadIdx.x == 0) ep.write(acc, out8);
        return;
    }
    const int e = (blockIdx.x - 1) * kBlock + threadIdx.x;
    if (e < n_elem) {
        float s = 0.f;
        for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * n_elem + e];
        dparams[e] = s;
    }
}

// workgroups of the persistent grid: as many as the LDS lets a CU hold (at most max_per_cu: the accumulators bound the waves per SIMD)
inline int rowstep_grid(int64_t tiles, size_t lds, int max_per_cu) {
    int64_t per_cu = (int64_t)(kLdsPerCu / (lds + 512));
    per_cu = per_cu < 1 ? 1 : (per_cu > max_per_cu ? max_per_cu : per_cu);
    const int64_t cap = CDR_NUM_CU * per_cu;
    return (int)(tiles < cap ? tiles : cap);
}

inline int rowstep_optin_lds(const void* kern, size_t lds, const char* entry) {
    if (lds <= 64 * 1024) return CDR_OK;
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { cdr_set_error("%s: %zu B of LDS refused: %s", entry, lds, hipGetErrorString(e)); return (int)e; }
    return CDR_OK;
}

// the tail of an entry point: ``forward()`` launches the forward kernel (timed under ``tag``), then the finishing launch
template <class Forward, class Epilogue>
inline int rowstep_run(cdr_ctx* ctx, hipStream_t s, int tag, const char* entry, Forward&& forward, int grid, const Epilogue& ep, float* out8,
                       const void* workspace, int n_elem, float* dparams) {
    auto launched = [entry] {                // CDR_LAUNCH_CHECK under the entry point's name
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) cdr_set_error("%s: launch failed: %s", entry, hipGetErrorString(e));
        return (int)e;
    };
    {
        cdr_time_scope ts(ctx, tag, s);
        forward();
    }
    if (int e = launched()) return e;
    rowstep_finish_kernel<Epilogue><<<dim3(1 + (n_elem + kBlock - 1) / kBlock), dim3(kBlock), 0, s>>>(ctx->partials, grid, ep, out8,
                                                                                                      (const float*)workspace, n_elem, dparams);
    return launched();
}

}  // namespace
