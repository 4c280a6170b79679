// DeepAPF's row-wise forward (deepapf.py:69-152 the two domain forwards, 163-175 the loss): one domain's batch through the two-candidate
// attention -- the share row and the domain-only row of the key id, each multiplied with the other side's row and scored by the small
// ReLU MLP -- the masked pair softmax, the merge and the predict layer.
//
//   s = share[key_b]  o = only[key_b]  t = other[oid_b]   xs = s (.) t   xo = o (.) t
//   hs = relu(W1 xs + b1)  ho = relu(W1 xo + b1)   a_s = w2 . hs (-1e31 where key_b > n_overlap, STRICTLY)   a_o = w2 . ho
//   (al_s, al_o) = softmax(a_s, a_o)   e = al_s s + al_o o   z = wp . (e (.) t)   p = sigmoid(z)   g_b = w (p_b - y_b) / B
//   ge = g wp (.) t   d_s = <ge, s>  d_o = <ge, o>  dot = al_s d_s + al_o d_o   ga_s = al_s (d_s - dot)   ga_o = al_o (d_o - dot)
//   gh_s = ga_s w2 (.) [hs > 0]   gx_s = W1^T gh_s   (the same for o)
//   GS[b] = al_s ge + gx_s (.) t   GO[b] = al_o ge + gx_o (.) t   GT[b] = g wp (.) e + gx_s (.) s + gx_o (.) o
//   dW1 = sum_b gh_s xs^T + gh_o xo^T   db1 = sum_b gh_s + gh_o   dw2 = sum_b ga_s hs + ga_o ho   dwp = sum_b g e (.) t
//
// A workgroup of four waves stages W1 once in LDS (zero-padded to the 32-wide MFMA tile) and walks row tiles of 32 batch rows under a
// persistent grid.  The tile's operand has 64 rows: the 32 share candidates, then the 32 only candidates.  Per tile:
//   stage  eight lanes per row read the three table rows (a masked occurrence does not read its share row: zeros), keep them in
//          registers and write xs, xo to LDS
//   fwd    H = relu(X W1^T + b1) on v_mfma_f32_32x32x2_f32, one 32x32 output tile per wave job
//   score  eight lanes per row: a_s, a_o, the softmax, z, the loss term and g_b, ga_s and ga_o; dwp in per-lane accumulators
//   mask   one thread per (column, row slice): dw2 += ga H, gH = ga w2 [H > 0] written over H in place, db1 += gH
//   dW1    dW1 += gH^T X into register accumulators that live ACROSS the workgroup's tiles
//   gX     gX = gH W1 written over X
//   route  eight lanes per row: the three compact gradient rows of the occurrence (a masked share row is +0.0)
// H, gH and X never leave the CU.  The parameter gradients are written once, as the workgroup's partial, when its tiles are done;
// rowstep_finish_kernel (cdr_rowstep.h) adds the partials in workgroup order (no float atomics: a rerun is bit-equal) and turns the fp64 block partials
// of the loss into out8.
// At D = 64 a row is ~50 kFLOP (three contractions over two candidates) against ~1.5 KB of HBM traffic: past the balance of the fp32
// matrix pipe and HBM, which is why the contractions are on the matrix pipe.
// LDS at the widest accepted shape (D = 128): W1 67,584 + X 33,792 + H 33,792 + b1, w2, wp 1,536 + ga 256 = 136,960 B of the CU's
// 163,840: one workgroup per CU there, nothing spills.
#include "cdr_rowstep.h"

namespace {

constexpr int kChunks = CDR_DEEPAPF_MAX_DIM / 4 / kSub;      // float4 chunks of a row one of the kSub lanes holds (4)

struct deepapf_plan {
    int grid;
    int nq;                                  // dW1 output tiles per wave
    int total;                               // D D + 3 D: the packed parameter vector [W1, b1, w2, wp]
    size_t lds;
    int64_t tiles;
};

inline bool deepapf_dim_ok(int D) { return D >= 4 && D <= CDR_DEEPAPF_MAX_DIM && (D & 3) == 0; }

inline deepapf_plan deepapf_plan_for(int64_t B, int D) {
    const int DP = pad32(D), S = DP + kLdsPad;
    deepapf_plan p;
    p.total = D * D + 3 * D;
    p.lds = ((size_t)DP * S + 4 * (size_t)kRows * S + 3 * (size_t)DP + 2 * kRows) * sizeof(float);
    p.tiles = (B + kRows - 1) / kRows;
    p.grid = rowstep_grid(p.tiles, p.lds, 2);               // (190..216 VGPRs + 32..80 AGPRs: two waves per SIMD at most)
    p.nq = ((DP >> 5) * (DP >> 5) + 3) / 4;
    return p;
}

struct deepapf_args {
    const float *share, *only, *other;
    int D;
    const float* params;
    const int64_t *key, *oid;
    const float* label;
    int64_t B, n_overlap;
    float scale;                             // weight / B
    float *GS, *GO, *GT;                     // GS at this domain's first row of the joint buffer
    float* part;
    double* partials;
};

template <int NQ, bool NT>
__global__ __launch_bounds__(kBlock) void deepapf_fwd_grad_kernel(const deepapf_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double red[kBlock / 64];
    const int D = a.D, D4 = D >> 2, DP = pad32(D), S = DP + kLdsPad, nD = DP >> 5;
    float* Ws = smem;                        // [DP][S]   W1, zero-padded
    float* Xs = Ws + DP * S;                 // [64][S]   xs rows, then xo rows; later gX
    float* Hs = Xs + 2 * kRows * S;          // [64][S]   H, later gH
    float* b1s = Hs + 2 * kRows * S;         // [DP] each, zero-padded
    float* w2s = b1s + DP;
    float* wps = w2s + DP;
    float* gas = wps + DP;                   // [64]      ga_s of the 32 rows, then ga_o
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 31, lh = lane >> 5;
    const int row = t / kSub, sub = t % kSub;
    // the mask phase: thread (column mc, row slice mp) walks rows [mp mrows, (mp + 1) mrows) of the 64-row operand
    const int nsplit = DP == 32 ? 8 : (DP == 64 ? 4 : 2), mrows = 2 * kRows / nsplit;
    const int mc = t % DP, mp = t / DP;
    const bool mact = mp < nsplit;

    // the parameters once per workgroup; the row buffers start as zeros (their columns past D are never written with anything else)
    for (int e = t; e < DP * S; e += kBlock) {
        const int r = e / S, c = e - r * S;
        Ws[e] = (r < D && c < D) ? a.params[r * D + c] : 0.f;
    }
    for (int e = t; e < DP; e += kBlock) {
        b1s[e] = e < D ? a.params[D * D + e] : 0.f;
        w2s[e] = e < D ? a.params[D * D + D + e] : 0.f;
        wps[e] = e < D ? a.params[D * D + 2 * D + e] : 0.f;
    }
    for (int e = t; e < 4 * kRows * S; e += kBlock) Xs[e] = 0.f;

    f32x16 wacc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) wacc[q] = zero16();
    float4 dwp[kChunks];
#pragma unroll
    for (int j = 0; j < kChunks; ++j) dwp[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    float db1acc = 0.f, dw2acc = 0.f;
    double acc[1] = {0.0};
    const int K = (D + 7) >> 3;              // K steps of eight: the columns up to the next multiple of 8 are zeros

    for (int64_t tile = blockIdx.x; tile < (a.B + kRows - 1) / kRows; tile += gridDim.x) {
        // ---- stage: ids first, then every row load; rows past the batch are zeros with g = 0
        const int64_t b = tile * kRows + row;
        const bool valid = b < a.B;
        const int64_t bc = valid ? b : a.B - 1;
        const int64_t ik = a.key[bc], io = a.oid[bc];
        const float y = a.label[bc];
        const bool masked = ik > a.n_overlap;
        float4 sv[kChunks], ov[kChunks], tv[kChunks];
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const int c = sub + kSub * j;
            sv[j] = ov[j] = tv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid && c < D4) {
                if (!masked) sv[j] = ld4n<NT>(a.share + ik * D + 4 * c);
                ov[j] = ld4n<NT>(a.only + ik * D + 4 * c);
                tv[j] = ld4n<NT>(a.other + io * D + 4 * c);
            }
        }
        __syncthreads();                     // the previous tile's routing (and the set-up) is done with Xs
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const int c = sub + kSub * j;
            if (c < D4) {
                st4(Xs + row * S + 4 * c, make_float4(sv[j].x * tv[j].x, sv[j].y * tv[j].y, sv[j].z * tv[j].z, sv[j].w * tv[j].w));
                st4(Xs + (kRows + row) * S + 4 * c, make_float4(ov[j].x * tv[j].x, ov[j].y * tv[j].y, ov[j].z * tv[j].z, ov[j].w * tv[j].w));
            }
        }
        __syncthreads();

        // ---- fwd: H = relu(X W1^T + b1), 2 x nD output tiles of 32 x 32
        for (int job = wave; job < 2 * nD; job += kBlock / 64) {
            const int rt = job / nD, ct = job - rt * nD;
            f32x16 a16 = zero16();
            const float* ap = Xs + (rt * kRows + li) * S + 4 * lh;
            const float* bp = Ws + (ct * 32 + li) * S + 4 * lh;
            for (int c = 0; c < K; ++c) {
                const float4 av = ld4(ap + 8 * c), bv = ld4(bp + 8 * c);
                MFMA4(a16, av, bv);
            }
            const int col = ct * 32 + li;
            const float bias = b1s[col];
#pragma unroll
            for (int r = 0; r < 16; ++r) Hs[(rt * kRows + (r & 3) + 8 * (r >> 2) + 4 * lh) * S + col] = fmaxf(a16[r] + bias, 0.f);
        }
        __syncthreads();

        // ---- score: the two scores, the pair softmax, the merged row's logit, the loss term and the coefficients
        float al_s, al_o, g;
        {
            float as = 0.f, ao = 0.f;
#pragma unroll
            for (int j = 0; j < kChunks; ++j) {
                const int c = sub + kSub * j;
                if (c < D4) {
                    const float4 w = ld4(w2s + 4 * c);
                    as += dot4(w, ld4(Hs + row * S + 4 * c));
                    ao += dot4(w, ld4(Hs + (kRows + row) * S + 4 * c));
                }
            }
            as = group_sum<kSub>(as);
            ao = group_sum<kSub>(ao);
            if (masked) as = -1e31f;
            const float m = fmaxf(as, ao);
            const float es = expf(as - m), eo = expf(ao - m);
            al_s = es / (es + eo); al_o = eo / (es + eo);
            float z = 0.f;
#pragma unroll
            for (int j = 0; j < kChunks; ++j) {
                const int c = sub + kSub * j;
                if (c < D4) {
                    const float4 w = ld4(wps + 4 * c);
                    z += w.x * ((al_s * sv[j].x + al_o * ov[j].x) * tv[j].x) + w.y * ((al_s * sv[j].y + al_o * ov[j].y) * tv[j].y) +
                         w.z * ((al_s * sv[j].z + al_o * ov[j].z) * tv[j].z) + w.w * ((al_s * sv[j].w + al_o * ov[j].w) * tv[j].w);
                }
            }
            z = group_sum<kSub>(z);
            float l;
            point_term(CDR_LOSS_BCE, z, y, a.scale, l, g);
            if (!valid) { l = 0.f; g = 0.f; }
            if (sub == 0) acc[0] += (double)l;
            float d_s = 0.f, d_o = 0.f;
#pragma unroll
            for (int j = 0; j < kChunks; ++j) {
                const int c = sub + kSub * j;
                if (c < D4) {
                    const float4 w = ld4(wps + 4 * c);
                    const float4 ge = make_float4(g * w.x * tv[j].x, g * w.y * tv[j].y, g * w.z * tv[j].z, g * w.w * tv[j].w);
                    d_s += dot4(ge, sv[j]);
                    d_o += dot4(ge, ov[j]);
                    dwp[j].x += g * (al_s * sv[j].x + al_o * ov[j].x) * tv[j].x;
                    dwp[j].y += g * (al_s * sv[j].y + al_o * ov[j].y) * tv[j].y;
                    dwp[j].z += g * (al_s * sv[j].z + al_o * ov[j].z) * tv[j].z;
                    dwp[j].w += g * (al_s * sv[j].w + al_o * ov[j].w) * tv[j].w;
                }
            }
            d_s = group_sum<kSub>(d_s);
            d_o = group_sum<kSub>(d_o);
            const float dot = al_s * d_s + al_o * d_o;
            if (sub == 0) {
                gas[row] = masked ? 0.f : al_s * (d_s - dot);        // (exactly 0 there anyway: al_s == 0)
                gas[kRows + row] = al_o * (d_o - dot);
            }
        }
        __syncthreads();

        // ---- mask: dw2 += ga H, gH = ga w2 [H > 0] over H in place, db1 += gH; one thread per (column, row slice), rows in order
        if (mact) {
            const float w2c = w2s[mc];
            for (int r = mp * mrows; r < (mp + 1) * mrows; ++r) {
                const float h = Hs[r * S + mc], ga = gas[r];
                dw2acc += ga * h;
                const float gh = h > 0.f ? ga * w2c : 0.f;
                db1acc += gh;
                Hs[r * S + mc] = gh;
            }
        }
        __syncthreads();

        // ---- dW1 += gH^T X over the operand's 64 rows, tile (ti, tj) = wave + 4 q
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int ot = wave + (kBlock / 64) * q;
            if (ot < nD * nD) {
                const int ti = ot / nD, tj = ot - ti * nD;
                const float* ap = Hs + lh * S + ti * 32 + li;
                const float* bp = Xs + lh * S + tj * 32 + li;
#pragma unroll 4
                for (int s = 0; s < kRows; ++s) MF1(wacc[q], ap[2 * s * S], bp[2 * s * S]);
            }
        }
        __syncthreads();

        // ---- gX = gH W1 written over X
        for (int job = wave; job < 2 * nD; job += kBlock / 64) {
            const int rt = job / nD, ct = job - rt * nD;
            f32x16 a16 = zero16();
            const float* ap = Hs + (rt * kRows + li) * S + 4 * lh;
            const float* bp = Ws + (4 * lh) * S + ct * 32 + li;
            for (int c = 0; c < K; ++c) {
                const float4 av = ld4(ap + 8 * c);
                const float* bq = bp + 8 * c * S;
                const float4 bv = make_float4(bq[0], bq[S], bq[2 * S], bq[3 * S]);
                MFMA4(a16, av, bv);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) Xs[(rt * kRows + (r & 3) + 8 * (r >> 2) + 4 * lh) * S + ct * 32 + li] = a16[r];
        }
        __syncthreads();

        // ---- route: the occurrence's three gradient rows
        if (valid) {
#pragma unroll
            for (int j = 0; j < kChunks; ++j) {
                const int c = sub + kSub * j;
                if (c < D4) {
                    const float4 w = ld4(wps + 4 * c);
                    const float4 xs = ld4(Xs + row * S + 4 * c), xo = ld4(Xs + (kRows + row) * S + 4 * c);
                    const float4 s4 = sv[j], o4 = ov[j], t4 = tv[j];
                    const float4 ge = make_float4(g * w.x * t4.x, g * w.y * t4.y, g * w.z * t4.z, g * w.w * t4.w);
                    float4 gs = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (!masked) gs = make_float4(al_s * ge.x + xs.x * t4.x, al_s * ge.y + xs.y * t4.y, al_s * ge.z + xs.z * t4.z, al_s * ge.w + xs.w * t4.w);
                    const float4 go = make_float4(al_o * ge.x + xo.x * t4.x, al_o * ge.y + xo.y * t4.y, al_o * ge.z + xo.z * t4.z, al_o * ge.w + xo.w * t4.w);
                    const float4 gt = make_float4(g * w.x * (al_s * s4.x + al_o * o4.x) + xs.x * s4.x + xo.x * o4.x,
                                                  g * w.y * (al_s * s4.y + al_o * o4.y) + xs.y * s4.y + xo.y * o4.y,
                                                  g * w.z * (al_s * s4.z + al_o * o4.z) + xs.z * s4.z + xo.z * o4.z,
                                                  g * w.w * (al_s * s4.w + al_o * o4.w) + xs.w * s4.w + xo.w * o4.w);
                    st4n<NT>(a.GS + b * D + 4 * c, gs);
                    st4n<NT>(a.GO + b * D + 4 * c, go);
                    st4n<NT>(a.GT + b * D + 4 * c, gt);
                }
            }
        }
    }

    // the workgroup's partial of every parameter gradient, in the packed layout
    float* part = a.part + (size_t)blockIdx.x * (D * D + 3 * D);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int ot = wave + (kBlock / 64) * q;
        if (ot < nD * nD) {
            const int ti = ot / nD, tj = ot - ti * nD;
            STORE_TILE32(part, 0, D, ti, tj, D, D, wacc[q], li, lh);
        }
    }
    // db1, dw2: the row slices' sums in slice order; dwp: the 32 row groups' sums in row order -- through the row buffers
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kChunks; ++j) {
        const int c = sub + kSub * j;
        if (c < D4) st4(Xs + row * S + 4 * c, dwp[j]);
    }
    if (mact) {
        Hs[mp * S + mc] = db1acc;
        Hs[(8 + mp) * S + mc] = dw2acc;
    }
    __syncthreads();
    if (t < D) {
        float s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int p = 0; p < nsplit; ++p) { s1 += Hs[p * S + t]; s2 += Hs[(8 + p) * S + t]; }
        for (int r = 0; r < kRows; ++r) s3 += Xs[r * S + t];
        part[D * D + t] = s1;
        part[D * D + D + t] = s2;
        part[D * D + 2 * D + t] = s3;
    }
    block_sum_d<1>(acc, red);
    if (threadIdx.x == 0) store_partials(a.partials, acc);
}

}  // namespace

extern "C" int cdr_deepapf_fwd_grad_workspace_bytes(int64_t B, int D, size_t* bytes) {
    CDR_CHECK_ARG(bytes && B > 0 && deepapf_dim_ok(D));
    const deepapf_plan p = deepapf_plan_for(B, D);
    *bytes = (size_t)p.grid * p.total * sizeof(float);
    return CDR_OK;
}

extern "C" int cdr_deepapf_fwd_grad(cdr_ctx* ctx, void* stream, const float* share_tab, const float* only_tab, const float* other_tab, int D,
                                    const float* params, const int64_t* key, const int64_t* oid, const float* label, int64_t B,
                                    int64_t n_overlap, float weight, int64_t row0, float* out8, float* GS, float* GO, float* GT,
                                    float* dparams, void* workspace, size_t workspace_bytes) {
    CDR_CHECK_ARG(B > 0 && row0 >= 0 && deepapf_dim_ok(D));
    CDR_CHECK_ARG(ctx && share_tab && only_tab && other_tab && params && key && oid && label && out8 && GS && GO && GT && dparams && workspace);
    CDR_CHECK_ARG((((uintptr_t)share_tab | (uintptr_t)only_tab | (uintptr_t)other_tab | (uintptr_t)GS | (uintptr_t)GO | (uintptr_t)GT) & 15) == 0);
    const deepapf_plan p = deepapf_plan_for(B, D);
    CDR_CHECK_ARG(workspace_bytes >= (size_t)p.grid * p.total * sizeof(float));
    static_assert(CDR_DEEPAPF_MAX_DIM == 128 && kChunks * kSub * 4 == CDR_DEEPAPF_MAX_DIM, "a lane holds four float4 chunks of a row; NQ covers 1..4");
    static_assert(kBlock == 2 * CDR_DEEPAPF_MAX_DIM && 2 * kRows == 64, "the mask phase: at least two row slices per column, at most eight");
    static_assert(CDR_NUM_CU * 4 <= CDR_MAX_PARTIAL_BLOCKS, "one partial slot per workgroup");
    if (p.lds > kLdsPerCu) { cdr_set_error("cdr_deepapf_fwd_grad: %zu B of LDS for this shape", p.lds); return CDR_EINVAL; }
    using kern_fn = void (*)(const deepapf_args);
    const bool nt = D * 4 >= 512;                              // non-temporal row traffic from 512-byte rows up (cdr_common.h)
    kern_fn kern = nullptr;
#define DEEPAPF_PICK(NQ) kern = nt ? deepapf_fwd_grad_kernel<NQ, true> : deepapf_fwd_grad_kernel<NQ, false>
    switch (p.nq) {
        case 1: DEEPAPF_PICK(1); break;
        case 2: DEEPAPF_PICK(2); break;
        case 3: DEEPAPF_PICK(3); break;
        default: DEEPAPF_PICK(4); break;
    }
#undef DEEPAPF_PICK
    if (int e = rowstep_optin_lds((const void*)kern, p.lds, __func__)) return e;
    deepapf_args a;
    a.share = share_tab; a.only = only_tab; a.other = other_tab; a.D = D;
    a.params = params;
    a.key = key; a.oid = oid; a.label = label; a.B = B; a.n_overlap = n_overlap;
    a.scale = weight * (1.0f / (float)B);
    a.GS = GS + row0 * D; a.GO = GO; a.GT = GT;
    a.part = (float*)workspace; a.partials = ctx->partials;
    hipStream_t s = (hipStream_t)stream;
    return rowstep_run(ctx, s, CDR_TAG_DEEPAPF_FWD_GRAD, __func__, [&] { kern<<<dim3(p.grid), dim3(kBlock), p.lds, s>>>(a); }, p.grid,
                       rowstep_bce{B, weight}, out8, workspace, p.total, dparams);
}
