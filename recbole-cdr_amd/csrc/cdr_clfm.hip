// CLFM's row-wise forward (clfm.py:74-124): one domain's batch through the small dense map W = [shared_linear ; <domain>_only_linear]
// that sits between the user row and the dot product -- the one step of the row-wise family that is not "gather two rows and dot them".
//
//   u_b = U[uid_b]  i_b = I[iid_b]  f_b = W u_b  x_b = <f_b, i_b>  p_b = sigmoid(x_b)  g_b = w (p_b - y_b) / B
//   GU[b] = g_b W^T i_b     GI[b] = g_b f_b     dW = sum_b g_b i_b u_b^T     + the BCE sum and the squared norms of the gathered rows
//
// A workgroup of four waves stages W once in LDS (zero-padded to the 32-wide MFMA tile) and walks row tiles of 32 batch rows under a
// persistent grid.  Per tile the rows of U and I are read once into LDS and feed the three contractions on v_mfma_f32_32x32x2_f32:
//   A  F = U W^T [32, Di] and T = I W [32, Du]: one 32x32 output tile per job, the nI + nU jobs dealt round-robin to the waves
//   B  eight lanes per row: x_b from F and the row's I chunks still in registers, the loss term, g_b; GI[b] = g_b F[b], GU[b] = g_b T[b]
//   C  dW += (g (.) I)^T U: the nI x nU output tiles dealt round-robin to the waves, accumulated in registers ACROSS the workgroup's tiles
// and written once, as the workgroup's partial, when its tiles are done; rowstep_finish_kernel (cdr_rowstep.h) adds the partials in workgroup order (no
// float atomics: a rerun is bit-equal) and turns the fp64 block partials of the loss and norm sums into out8.
// At Du = Di = 64 a row is ~25 kFLOP against ~1 KB of HBM traffic: near the balance of the fp32 matrix pipe and HBM, which is why the
// contractions are on the matrix pipe and not a per-lane matvec with wave reductions.
#include "cdr_rowstep.h"

namespace {

constexpr int kChunks = CDR_CLFM_MAX_DIM / 4 / kSub;     // float4 chunks of a row one of the kSub lanes holds (4)

struct clfm_plan {
    int grid;
    int nq;                                  // dW output tiles per wave
    size_t lds;
    int64_t tiles;
};

inline clfm_plan clfm_plan_for(int64_t B, int Du, int Di) {
    const int DuP = pad32(Du), DiP = pad32(Di), SU = DuP + kLdsPad, SI = DiP + kLdsPad;
    clfm_plan p;
    p.lds = ((size_t)DiP * SU + 2 * (size_t)kRows * SU + 2 * (size_t)kRows * SI + kRows) * sizeof(float);
    p.tiles = (B + kRows - 1) / kRows;
    p.grid = rowstep_grid(p.tiles, p.lds, 4);
    p.nq = ((DuP >> 5) * (DiP >> 5) + 3) / 4;
    return p;
}

template <int NQ, bool NT_U, bool NT_I>
__global__ __launch_bounds__(kBlock) void clfm_fwd_grad_kernel(const float* __restrict__ U, const float* __restrict__ I,
                                                               const float* __restrict__ W, int Du, int Di,
                                                               const int64_t* __restrict__ uid, const int64_t* __restrict__ iid,
                                                               const float* __restrict__ label, int64_t B, float scale,
                                                               float* __restrict__ GU, float* __restrict__ GI,
                                                               float* __restrict__ dWpart, double* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double red[3 * (kBlock / 64)];
    const int DuP = pad32(Du), DiP = pad32(Di), SU = DuP + kLdsPad, SI = DiP + kLdsPad;
    const int Du4 = Du >> 2, Di4 = Di >> 2, nU = DuP >> 5, nI = DiP >> 5;
    float* Ws = smem;                        // [DiP][SU]   W, zero-padded
    float* Us = Ws + DiP * SU;               // [32][SU]    the tile's user rows
    float* Ts = Us + kRows * SU;             // [32][SU]    T = I W
    float* Is = Ts + kRows * SU;             // [32][SI]    the tile's item rows
    float* Fs = Is + kRows * SI;             // [32][SI]    F = U W^T
    float* gs = Fs + kRows * SI;             // [32]        g_b
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 31, lh = lane >> 5;
    const int row = t / kSub, sub = t % kSub;

    // W once per workgroup; the row buffers start as zeros (their columns past Du / Di are never written again)
    const int SU4 = SU >> 2;
    for (int e = t; e < DiP * SU4; e += kBlock) {
        const int r = e / SU4, c = e - r * SU4;
        st4(Ws + r * SU + 4 * c, (r < Di && c < Du4) ? ld4(W + (int64_t)r * Du + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f));
    }
    for (int e = t; e < kRows * SU; e += kBlock) Us[e] = 0.f;
    for (int e = t; e < kRows * SI; e += kBlock) Is[e] = 0.f;

    f32x16 wacc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) wacc[q] = zero16();
    double acc[3] = {0.0, 0.0, 0.0};
    const int KU = (Du + 7) >> 3, KI = (Di + 7) >> 3;      // K steps of eight: the columns up to the next multiple of 8 are zeros

    for (int64_t tile = blockIdx.x; tile < (B + kRows - 1) / kRows; tile += gridDim.x) {
        // ---- stage: ids first, then every row load (vmcnt is in-order); rows past the batch are zeros with g = 0
        const int64_t b = tile * kRows + row;
        const bool valid = b < B;
        const int64_t bc = valid ? b : B - 1;
        const int64_t iu = uid[bc], ii = iid[bc];
        const float y = label[bc];
        float4 u[kChunks], v[kChunks];
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const int c = sub + kSub * j;
            u[j] = v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid && c < Du4) u[j] = ld4n<NT_U>(U + iu * Du + 4 * c);
            if (valid && c < Di4) v[j] = ld4n<NT_I>(I + ii * Di + 4 * c);
        }
        __syncthreads();                     // the previous tile's dW pass (and the set-up) is done with Us / Is / gs
        float su = 0.f, si = 0.f;
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const int c = sub + kSub * j;
            if (c < Du4) { st4(Us + row * SU + 4 * c, u[j]); su += dot4(u[j], u[j]); }
            if (c < Di4) { st4(Is + row * SI + 4 * c, v[j]); si += dot4(v[j], v[j]); }
        }
        acc[1] += (double)su;
        acc[2] += (double)si;
        __syncthreads();

        // ---- A: F = U W^T (jobs 0 .. nI-1) and T = I W (jobs nI .. nI+nU-1), one 32x32 output tile each
        for (int job = wave; job < nI + nU; job += kBlock / 64) {
            f32x16 a16 = zero16();
            if (job < nI) {
                const float* ap = Us + li * SU + 4 * lh;
                const float* bp = Ws + (job * 32 + li) * SU + 4 * lh;
                for (int c = 0; c < KU; ++c) {
                    const float4 av = ld4(ap + 8 * c), bv = ld4(bp + 8 * c);
                    MFMA4(a16, av, bv);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) Fs[((r & 3) + 8 * (r >> 2) + 4 * lh) * SI + job * 32 + li] = a16[r];
            } else {
                const int tu = job - nI;
                const float* ap = Is + li * SI + 4 * lh;
                const float* bp = Ws + (4 * lh) * SU + tu * 32 + li;
                for (int c = 0; c < KI; ++c) {
                    const float4 av = ld4(ap + 8 * c);
                    const float* bq = bp + 8 * c * SU;
                    const float4 bv = make_float4(bq[0], bq[SU], bq[2 * SU], bq[3 * SU]);
                    MFMA4(a16, av, bv);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) Ts[((r & 3) + 8 * (r >> 2) + 4 * lh) * SU + tu * 32 + li] = a16[r];
            }
        }
        __syncthreads();

        // ---- B: the row's score, loss term and coefficient; its two gradient rows
        {
            float4 f[kChunks];
            float x = 0.f;
#pragma unroll
            for (int j = 0; j < kChunks; ++j) {
                const int c = sub + kSub * j;
                f[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c < Di4) { f[j] = ld4(Fs + row * SI + 4 * c); x += dot4(f[j], v[j]); }
            }
            x = group_sum<kSub>(x);
            float l, g;
            point_term(CDR_LOSS_BCE, x, y, scale, l, g);
            if (!valid) { l = 0.f; g = 0.f; }
            if (sub == 0) { gs[row] = g; acc[0] += (double)l; }
            if (valid) {
#pragma unroll
                for (int j = 0; j < kChunks; ++j) {
                    const int c = sub + kSub * j;
                    if (c < Di4) st4n<NT_I>(GI + b * Di + 4 * c, scale4(g, f[j]));
                    if (c < Du4) st4n<NT_U>(GU + b * Du + 4 * c, scale4(g, ld4(Ts + row * SU + 4 * c)));
                }
            }
        }
        __syncthreads();

        // ---- C: dW += (g (.) I)^T U over the tile's 32 rows, tile (ti, tu) = wave + 4 q
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int ot = wave + (kBlock / 64) * q;
            if (ot < nI * nU) {
                const int ti = ot / nU, tu = ot - ti * nU;
                const float* ap = Is + lh * SI + ti * 32 + li;
                const float* bp = Us + lh * SU + tu * 32 + li;
#pragma unroll 4
                for (int s = 0; s < kRows / 2; ++s) {
                    const float a = ap[2 * s * SI] * gs[2 * s + lh];
                    MF1(wacc[q], a, bp[2 * s * SU]);
                }
            }
        }
    }

    // the workgroup's weight-gradient partial, [Di][Du]
    float* part = dWpart + (size_t)blockIdx.x * Di * Du;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int ot = wave + (kBlock / 64) * q;
        if (ot < nI * nU) {
            const int ti = ot / nU, tu = ot - ti * nU;
            STORE_TILE32(part, 0, Du, ti, tu, Di, Du, wacc[q], li, lh);
        }
    }
    block_sum_d<3>(acc, red);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

inline bool clfm_dims_ok(int Du, int Di) {
    return Du >= 4 && Di >= 4 && Du <= CDR_CLFM_MAX_DIM && Di <= CDR_CLFM_MAX_DIM && (Du & 3) == 0 && (Di & 3) == 0;
}

}  // namespace

extern "C" int cdr_clfm_fwd_grad_workspace_bytes(int64_t B, int Du, int Di, size_t* bytes) {
    CDR_CHECK_ARG(bytes && B > 0 && clfm_dims_ok(Du, Di));
    *bytes = (size_t)clfm_plan_for(B, Du, Di).grid * Di * Du * sizeof(float);
    return CDR_OK;
}

extern "C" int cdr_clfm_fwd_grad(cdr_ctx* ctx, void* stream, const float* user_tab, const float* item_tab, int Du, int Di, const float* W,
                                 const int64_t* uid, const int64_t* iid, const float* label, int64_t B, float weight, float reg_weight,
                                 float* out8, float* GU, float* GI, float* dW, void* workspace, size_t workspace_bytes) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && W && uid && iid && label && out8 && GU && GI && dW && workspace);
    CDR_CHECK_ARG(B > 0 && clfm_dims_ok(Du, Di));
    CDR_CHECK_ARG((((uintptr_t)user_tab | (uintptr_t)item_tab | (uintptr_t)W | (uintptr_t)GU | (uintptr_t)GI) & 15) == 0);
    const clfm_plan p = clfm_plan_for(B, Du, Di);
    CDR_CHECK_ARG(workspace_bytes >= (size_t)p.grid * Di * Du * sizeof(float));
    static_assert(CDR_CLFM_MAX_DIM == 128 && kChunks * kSub * 4 == CDR_CLFM_MAX_DIM, "a lane holds four float4 chunks of a row; NQ covers 1..4");
    static_assert(CDR_NUM_CU * 4 <= CDR_MAX_PARTIAL_BLOCKS, "one partial slot per workgroup");
    using kern_fn = void (*)(const float*, const float*, const float*, int, int, const int64_t*, const int64_t*, const float*, int64_t, float,
                             float*, float*, float*, double*);
    const bool ntu = Du * 4 >= 512, nti = Di * 4 >= 512;       // non-temporal row traffic from 512-byte rows up (cdr_common.h)
    kern_fn kern = nullptr;
#define CLFM_PICK(NQ)                                                                                       \
    kern = ntu ? (nti ? clfm_fwd_grad_kernel<NQ, true, true> : clfm_fwd_grad_kernel<NQ, true, false>)       \
               : (nti ? clfm_fwd_grad_kernel<NQ, false, true> : clfm_fwd_grad_kernel<NQ, false, false>)
    switch (p.nq) {
        case 1: CLFM_PICK(1); break;
        case 2: CLFM_PICK(2); break;
        case 3: CLFM_PICK(3); break;
        default: CLFM_PICK(4); break;
    }
#undef CLFM_PICK
    if (int e = rowstep_optin_lds((const void*)kern, p.lds, __func__)) return e;
    hipStream_t s = (hipStream_t)stream;
    return rowstep_run(ctx, s, CDR_TAG_CLFM_FWD_GRAD, __func__, [&] {
        kern<<<dim3(p.grid), dim3(kBlock), p.lds, s>>>(user_tab, item_tab, W, Du, Di, uid, iid, label, B, weight * (1.0f / (float)B), GU, GI,
                                                       (float*)workspace, ctx->partials);
    }, p.grid, rowstep_bce_emb{B, weight, reg_weight}, out8, workspace, Di * Du, dW);
}
