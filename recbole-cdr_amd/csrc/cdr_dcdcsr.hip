// DCDCSR's BOTH-phase map step (dcdcsr.py:172-187 the sampled rows, the max-min normalisation, the tanh MLP and the MSE; 167-172 the
// normalisation itself): forward, backward and every parameter gradient of one batch of sampled unit ids in one pass.
//
//   x = table[id_i]   mx = max x  mn = min x  mean = (mx + mn) / 2  h = mx - mean   e = (x - mean) / h     (the same for bench -> b, no gradient)
//   a_0 = e   a_l = tanh(a_{l-1} W_l^T + b_l)  l = 1..L (tanh after EVERY layer, the last included)   m = a_L
//   loss = sum_i sum_d (m - b)^2 / (n D)     g = 2 (m - b) / (n D)
//   gpre_L = g (1 - a_L^2)   dW_l = gpre_l^T a_{l-1}   db_l = sum_i gpre_l   gpre_{l-1} = (gpre_l W_l) (1 - a_{l-1}^2)   gy = gpre_1 W_1
//   G_i = gy / h - [x == mx] (Sg + Sy) / (2 h n_max) - [x == mn] (Sg - Sy) / (2 h n_min),   Sg = sum gy, Sy = sum gy e
//   (amax / amin split their gradient evenly over ties, as torch does: n_max and n_min count them; cdr_rowmodels.hip's maxmin_bwd_kernel)
//
// A workgroup of four waves walks row tiles of 32 occurrences under a persistent grid.  Every layer's activation of the tile stays in LDS
// (zero-padded to the 32-wide MFMA tile); where the padded weights fit beside them they are staged in LDS once per workgroup, wider
// shapes (128-[128]-128 is one) read the weight operand through L2 instead -- the activations alone are 50 KB there and both weight
// matrices 135 KB.  Per tile:
//   stage  eight lanes per row read the table row and the bench row, normalise both, keep x, e, b and the row's max, min, tie counts in
//          registers and write e to LDS
//   fwd    a_l = tanh(a_{l-1} W_l^T + b_l) on v_mfma_f32_32x32x2_f32, one 32x32 output tile per wave job, layer by layer
//   loss   eight lanes per row: (m - b)^2 into the fp64 loss sum, gpre_L over a_L in place
//   bwd    per layer, last first: db_l += column sums (one thread per column, rows in order), dW_l += gpre_l^T a_{l-1} into register
//          accumulators that live ACROSS the workgroup's tiles, then gpre_l W_l (1 - a_{l-1}^2) over a_{l-1} in place
//   route  eight lanes per row: the max-min backward and the occurrence's gradient row G_i
// Nothing but G leaves the CU per row.  The parameter gradients are written once, as the workgroup's partial, when its tiles are done;
// rowstep_finish_kernel (cdr_rowstep.h) adds the partials in workgroup order (no float atomics: a rerun is bit-equal) and turns the fp64 block partials
// of the loss into out8.  Duplicate ids get one gradient row per occurrence; the apply adds them in occurrence order.
// A constant row (max == min) divides by zero exactly as the reference does.
// LDS at the default 64-[128]-64: W 68,608 + activations 34,304 + biases and their gradients 1,536 = 104,448 B of the CU's 163,840.
#include "cdr_rowstep.h"

namespace {

constexpr int kChunks = CDR_DCDCSR_MAX_DIM / 4 / kSub;       // float4 chunks of a row one of the kSub lanes holds (4)
constexpr int kMaxL = CDR_DCDCSR_MAX_LAYERS;

struct dcdcsr_args {
    const float *table, *bench, *params;
    const int64_t* ids;
    int64_t n;
    int L;
    int d[kMaxL + 1];                        // widths, d[0] == d[L] == D
    int pw[kMaxL];                           // W_l in the packed parameter vector (b_l follows it)
    int ws[kMaxL];                           // LDS offsets in floats: W_l (weights in LDS only), b_l, db_l, a_l
    int bs[kMaxL];
    int dbs[kMaxL];
    int as[kMaxL + 1];
    int tb[kMaxL + 1];                       // dW_l's 32x32 output tiles are [tb[l-1], tb[l]) of the workgroup's tile list
    int act0, act1;                          // the activation area [act0, act1)
    int total;
    float scale;                             // 2 / (n D)
    float* G;
    float* part;
    double* partials;
};

struct dcdcsr_plan {
    int grid, nq, total;
    bool wlds;
    size_t lds;
    dcdcsr_args a;                           // the layout fields filled in
};

inline bool dcdcsr_shape_ok(int L, const int* dims) {
    if (!dims || L < 1 || L > kMaxL) return false;
    for (int l = 0; l <= L; ++l)
        if (dims[l] < 4 || dims[l] > CDR_DCDCSR_MAX_DIM || (dims[l] & 3)) return false;
    return dims[0] == dims[L];
}

inline dcdcsr_plan dcdcsr_plan_for(int64_t n, int L, const int* dims) {
    dcdcsr_plan p;
    dcdcsr_args& a = p.a;
    a.L = L;
    for (int l = 0; l <= kMaxL; ++l) a.d[l] = l <= L ? dims[l] : 0;
    size_t wfl = 0, rest = 0;
    int total = 0, tiles = 0;
    a.tb[0] = 0;
    for (int l = 1; l <= L; ++l) {
        a.pw[l - 1] = total;
        total += dims[l] * dims[l - 1] + dims[l];
        wfl += (size_t)pad32(dims[l]) * (pad32(dims[l - 1]) + kLdsPad);
        tiles += (pad32(dims[l]) >> 5) * (pad32(dims[l - 1]) >> 5);
        a.tb[l] = tiles;
        rest += 2 * (size_t)pad32(dims[l]);
    }
    for (int l = L + 1; l <= kMaxL; ++l) { a.pw[l - 1] = 0; a.tb[l] = tiles; }
    for (int l = 0; l <= L; ++l) rest += (size_t)kRows * (pad32(dims[l]) + kLdsPad);
    p.wlds = (wfl + rest) * sizeof(float) + 1024 <= kLdsPerCu;
    int off = 0;
    for (int l = 1; l <= kMaxL; ++l) {
        a.ws[l - 1] = off;
        if (p.wlds && l <= L) off += pad32(dims[l]) * (pad32(dims[l - 1]) + kLdsPad);
    }
    for (int l = 1; l <= kMaxL; ++l) {
        a.bs[l - 1] = off;
        if (l <= L) off += pad32(dims[l]);
        a.dbs[l - 1] = off;
        if (l <= L) off += pad32(dims[l]);
    }
    a.act0 = off;
    for (int l = 0; l <= kMaxL; ++l) {
        a.as[l] = off;
        if (l <= L) off += kRows * (pad32(dims[l]) + kLdsPad);
    }
    a.act1 = off;
    p.lds = (size_t)off * sizeof(float);
    p.total = a.total = total;
    p.nq = (tiles + 3) / 4;
    const int64_t ntile = (n + kRows - 1) / kRows;
    p.grid = rowstep_grid(ntile, p.lds, 2);                 // (the dW accumulators: two waves per SIMD at most)
    return p;
}

__device__ __forceinline__ float group8_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1, CDR_WAVE));
    v = fmaxf(v, __shfl_xor(v, 2, CDR_WAVE));
    return fmaxf(v, __shfl_xor(v, 4, CDR_WAVE));
}

template <int NQ, bool WLDS>
__global__ __launch_bounds__(kBlock) void dcdcsr_map_kernel(const dcdcsr_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double red[kBlock / 64];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 31, lh = lane >> 5;
    const int row = t / kSub, sub = t % kSub;
    const int L = a.L, D = a.d[0], D4 = D >> 2;

    // the parameters once per workgroup; the bias gradients and the activation buffers start as zeros (an activation column past its
    // layer's width is never written with anything else)
    for (int l = 1; l <= L; ++l) {
        const int in = a.d[l - 1], out = a.d[l], S = pad32(in) + kLdsPad, OP = pad32(out);
        const float* W = a.params + a.pw[l - 1];
        if constexpr (WLDS) {
            float* Ws = smem + a.ws[l - 1];
            for (int e = t; e < OP * S; e += kBlock) {
                const int r = e / S, c = e - r * S;
                Ws[e] = (r < out && c < in) ? W[r * in + c] : 0.f;
            }
        }
        for (int e = t; e < OP; e += kBlock) {
            smem[a.bs[l - 1] + e] = e < out ? W[out * in + e] : 0.f;
            smem[a.dbs[l - 1] + e] = 0.f;
        }
    }
    for (int e = a.act0 + t; e < a.act1; e += kBlock) smem[e] = 0.f;

    f32x16 wacc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) wacc[q] = zero16();
    double acc[1] = {0.0};
    const int S0 = pad32(D) + kLdsPad;
    float* A0 = smem + a.as[0];
    float* AL = smem + a.as[L];

    for (int64_t tile = blockIdx.x; tile < (a.n + kRows - 1) / kRows; tile += gridDim.x) {
        // ---- stage: the id first, then both row loads; a row past the batch is zeros with g = 0
        const int64_t b = tile * kRows + row;
        const bool valid = b < a.n;
        const int64_t id = a.ids[valid ? b : a.n - 1];
        float4 xv[kChunks], ev[kChunks], bn[kChunks];
        float mx = -INFINITY, mn = INFINITY, bmx = -INFINITY, bmn = INFINITY;
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const int c = sub + kSub * j;
            xv[j] = ev[j] = bn[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid && c < D4) {
                xv[j] = ld4(a.table + id * D + 4 * c);
                bn[j] = ld4(a.bench + id * D + 4 * c);
                mx = fmaxf(mx, fmaxf(fmaxf(xv[j].x, xv[j].y), fmaxf(xv[j].z, xv[j].w)));
                mn = fminf(mn, fminf(fminf(xv[j].x, xv[j].y), fminf(xv[j].z, xv[j].w)));
                bmx = fmaxf(bmx, fmaxf(fmaxf(bn[j].x, bn[j].y), fmaxf(bn[j].z, bn[j].w)));
                bmn = fminf(bmn, fminf(fminf(bn[j].x, bn[j].y), fminf(bn[j].z, bn[j].w)));
            }
        }
        mx = group8_max(mx); mn = -group8_max(-mn);
        bmx = group8_max(bmx); bmn = -group8_max(-bmn);
        const float mean = (mx + mn) / 2.0f, h = mx - mean;
        const float bmean = (bmx + bmn) / 2.0f, bh = bmx - bmean;
        float nmax = 0.f, nmin = 0.f;
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const int c = sub + kSub * j;
            if (valid && c < D4) {
                const float4 x = xv[j], y = bn[j];
                nmax += (x.x == mx ? 1.f : 0.f) + (x.y == mx ? 1.f : 0.f) + (x.z == mx ? 1.f : 0.f) + (x.w == mx ? 1.f : 0.f);
                nmin += (x.x == mn ? 1.f : 0.f) + (x.y == mn ? 1.f : 0.f) + (x.z == mn ? 1.f : 0.f) + (x.w == mn ? 1.f : 0.f);
                ev[j] = make_float4((x.x - mean) / h, (x.y - mean) / h, (x.z - mean) / h, (x.w - mean) / h);
                bn[j] = make_float4((y.x - bmean) / bh, (y.y - bmean) / bh, (y.z - bmean) / bh, (y.w - bmean) / bh);
            }
        }
        nmax = group_sum<kSub>(nmax);
        nmin = group_sum<kSub>(nmin);
        __syncthreads();                     // the previous tile's routing (and the set-up) is done with a_0
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const int c = sub + kSub * j;
            if (c < D4) st4(A0 + row * S0 + 4 * c, ev[j]);
        }
        __syncthreads();

        // ---- fwd: a_l = tanh(a_{l-1} W_l^T + b_l), pad32(out) / 32 output tiles of 32 x 32 per layer
        for (int l = 1; l <= L; ++l) {
            const int in = a.d[l - 1], out = a.d[l], Sa = pad32(in) + kLdsPad, So = pad32(out) + kLdsPad;
            const float* Ain = smem + a.as[l - 1];
            float* Aout = smem + a.as[l];
            const float* Ws = smem + a.ws[l - 1];
            const float* Wg = a.params + a.pw[l - 1];
            const float* bsl = smem + a.bs[l - 1];
            const int K = (in + 7) >> 3;     // K steps of eight: the columns up to the next multiple of 8 are zeros
            for (int job = wave; job < (pad32(out) >> 5); job += kBlock / 64) {
                f32x16 a16 = zero16();
                const int col = job * 32 + li;
                const float* ap = Ain + li * Sa + 4 * lh;
                for (int c = 0; c < K; ++c) {
                    const float4 av = ld4(ap + 8 * c);
                    float4 bv;
                    if constexpr (WLDS) {
                        bv = ld4(Ws + col * Sa + 4 * lh + 8 * c);
                    } else {
                        bv = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (col < out && 8 * c + 4 * lh < in) bv = ld4(Wg + col * in + 8 * c + 4 * lh);
                    }
                    MFMA4(a16, av, bv);
                }
                const float bias = bsl[col];
#pragma unroll
                for (int r = 0; r < 16; ++r) Aout[((r & 3) + 8 * (r >> 2) + 4 * lh) * So + col] = col < out ? tanhf(a16[r] + bias) : 0.f;
            }
            __syncthreads();
        }

        // ---- loss: (m - b)^2 into the fp64 sum, gpre_L = g (1 - m^2) over a_L in place
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const int c = sub + kSub * j;
            if (c < D4) {
                const float4 m = ld4(AL + row * S0 + 4 * c);
                const float4 df = make_float4(m.x - bn[j].x, m.y - bn[j].y, m.z - bn[j].z, m.w - bn[j].w);
                float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
                if (valid) {
                    acc[0] += (double)(df.x * df.x) + (double)(df.y * df.y) + (double)(df.z * df.z) + (double)(df.w * df.w);
                    g = make_float4(a.scale * df.x * (1.0f - m.x * m.x), a.scale * df.y * (1.0f - m.y * m.y),
                                    a.scale * df.z * (1.0f - m.z * m.z), a.scale * df.w * (1.0f - m.w * m.w));
                }
                st4(AL + row * S0 + 4 * c, g);
            }
        }
        __syncthreads();

        // ---- bwd, last layer first
        for (int l = L; l >= 1; --l) {
            const int in = a.d[l - 1], out = a.d[l], Sa = pad32(in) + kLdsPad, So = pad32(out) + kLdsPad, nI = pad32(in) >> 5;
            float* X = smem + a.as[l - 1];                     // a_{l-1}, then gpre_{l-1} (l = 1: gy)
            const float* gH = smem + a.as[l];                  // gpre_l
            const float* Ws = smem + a.ws[l - 1];
            const float* Wg = a.params + a.pw[l - 1];
            // db_l: one thread per column, the tile's rows in order, the tiles in order
            if (t < out) {
                float s = 0.f;
                for (int r = 0; r < kRows; ++r) s += gH[r * So + t];
                smem[a.dbs[l - 1] + t] += s;
            }
            // dW_l += gpre_l^T a_{l-1} over the tile's 32 rows, tile (ti, tj) = wave + 4 q - tb[l-1] of this layer
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int ot = wave + (kBlock / 64) * q;
                if (ot >= a.tb[l - 1] && ot < a.tb[l]) {
                    const int loc = ot - a.tb[l - 1], ti = loc / nI, tj = loc - ti * nI;
                    const float* ap = gH + lh * So + ti * 32 + li;
                    const float* bp = X + lh * Sa + tj * 32 + li;
#pragma unroll 4
                    for (int s = 0; s < kRows / 2; ++s) MF1(wacc[q], ap[2 * s * So], bp[2 * s * Sa]);
                }
            }
            __syncthreads();
            // gpre_{l-1} = (gpre_l W_l) (1 - a_{l-1}^2) written over a_{l-1}; l = 1: gy = gpre_1 W_1 over e
            const int K = (out + 7) >> 3;
            for (int job = wave; job < nI; job += kBlock / 64) {
                f32x16 a16 = zero16();
                const int col = job * 32 + li;
                const float* ap = gH + li * So + 4 * lh;
                for (int c = 0; c < K; ++c) {
                    const float4 av = ld4(ap + 8 * c);
                    const int k0 = 8 * c + 4 * lh;
                    float4 bv;
                    if constexpr (WLDS) {
                        const float* bq = Ws + k0 * Sa + col;
                        bv = make_float4(bq[0], bq[Sa], bq[2 * Sa], bq[3 * Sa]);
                    } else {
                        bv = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (col < in && k0 < out) {                // (out % 4 == 0: the four rows are inside together)
                            const float* bq = Wg + k0 * in + col;
                            bv = make_float4(bq[0], bq[in], bq[2 * in], bq[3 * in]);
                        }
                    }
                    MFMA4(a16, av, bv);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = ((r & 3) + 8 * (r >> 2) + 4 * lh) * Sa + col;
                    float v = a16[r];
                    if (l > 1) { const float x = X[o]; v *= 1.0f - x * x; }
                    X[o] = v;
                }
            }
            __syncthreads();
        }

        // ---- route: back through the max-min normalisation, one gradient row per occurrence
        {
            float Sg = 0.f, Sy = 0.f;
            float4 gy[kChunks];
#pragma unroll
            for (int j = 0; j < kChunks; ++j) {
                const int c = sub + kSub * j;
                gy[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c < D4) {
                    gy[j] = ld4(A0 + row * S0 + 4 * c);
                    Sg += (gy[j].x + gy[j].y) + (gy[j].z + gy[j].w);
                    Sy += dot4(gy[j], ev[j]);
                }
            }
            Sg = group_sum<kSub>(Sg);
            Sy = group_sum<kSub>(Sy);
            const float cmax = (Sg + Sy) / (2.0f * h * nmax), cmin = (Sg - Sy) / (2.0f * h * nmin);
            if (valid) {
#pragma unroll
                for (int j = 0; j < kChunks; ++j) {
                    const int c = sub + kSub * j;
                    if (c < D4) {
                        const float4 x = xv[j];
                        float4 g = make_float4(gy[j].x / h, gy[j].y / h, gy[j].z / h, gy[j].w / h);
                        if (x.x == mx) g.x -= cmax;
                        if (x.y == mx) g.y -= cmax;
                        if (x.z == mx) g.z -= cmax;
                        if (x.w == mx) g.w -= cmax;
                        if (x.x == mn) g.x -= cmin;
                        if (x.y == mn) g.y -= cmin;
                        if (x.z == mn) g.z -= cmin;
                        if (x.w == mn) g.w -= cmin;
                        st4(a.G + b * D + 4 * c, g);
                    }
                }
            }
        }
    }

    // the workgroup's partial of every parameter gradient, in the packed layout
    float* part = a.part + (size_t)blockIdx.x * a.total;
    for (int l = 1; l <= L; ++l) {
        const int in = a.d[l - 1], out = a.d[l], nI = pad32(in) >> 5;
        float* pl = part + a.pw[l - 1];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int ot = wave + (kBlock / 64) * q;
            if (ot >= a.tb[l - 1] && ot < a.tb[l]) {
                const int loc = ot - a.tb[l - 1], ti = loc / nI, tj = loc - ti * nI;
                STORE_TILE32(pl, 0, in, ti, tj, out, in, wacc[q], li, lh);
            }
        }
        if (t < out) pl[out * in + t] = smem[a.dbs[l - 1] + t];     // (the thread that summed the column)
    }
    block_sum_d<1>(acc, red);
    if (threadIdx.x == 0) store_partials(a.partials, acc);
}

}  // namespace

extern "C" int cdr_dcdcsr_map_fwd_grad_workspace_bytes(int64_t n, int L, const int* dims, size_t* bytes) {
    CDR_CHECK_ARG(bytes && n > 0 && dcdcsr_shape_ok(L, dims));
    const dcdcsr_plan p = dcdcsr_plan_for(n, L, dims);
    *bytes = (size_t)p.grid * p.total * sizeof(float);
    return CDR_OK;
}

extern "C" int cdr_dcdcsr_map_fwd_grad(cdr_ctx* ctx, void* stream, const float* table, const float* bench, const int64_t* ids, int64_t n,
                                       int L, const int* dims, const float* params, float* out8, float* G, float* dparams,
                                       void* workspace, size_t workspace_bytes) {
    CDR_CHECK_ARG(n > 0 && dcdcsr_shape_ok(L, dims));
    CDR_CHECK_ARG(ctx && table && bench && ids && params && out8 && G && dparams && workspace);
    CDR_CHECK_ARG((((uintptr_t)table | (uintptr_t)bench | (uintptr_t)params | (uintptr_t)G) & 15) == 0);
    dcdcsr_plan p = dcdcsr_plan_for(n, L, dims);
    CDR_CHECK_ARG(workspace_bytes >= (size_t)p.grid * p.total * sizeof(float));
    static_assert(CDR_DCDCSR_MAX_DIM == 128 && kChunks * kSub * 4 == CDR_DCDCSR_MAX_DIM, "a lane holds four float4 chunks of a row");
    static_assert(CDR_DCDCSR_MAX_LAYERS * 16 <= 12 * 4, "NQ covers every accepted shape: at most 16 dW tiles per layer, four waves");
    static_assert(kBlock >= CDR_DCDCSR_MAX_DIM, "db_l: one thread per column");
    static_assert(CDR_NUM_CU * 2 <= CDR_MAX_PARTIAL_BLOCKS, "one partial slot per workgroup");
    if (p.lds > kLdsPerCu) { cdr_set_error("cdr_dcdcsr_map_fwd_grad: %zu B of LDS for this shape", p.lds); return CDR_EINVAL; }
    using kern_fn = void (*)(const dcdcsr_args);
    kern_fn kern = nullptr;
#define DCDCSR_PICK(NQ) kern = p.wlds ? dcdcsr_map_kernel<NQ, true> : dcdcsr_map_kernel<NQ, false>
    if (p.nq <= 1) DCDCSR_PICK(1);
    else if (p.nq <= 2) DCDCSR_PICK(2);
    else if (p.nq <= 4) DCDCSR_PICK(4);
    else if (p.nq <= 6) DCDCSR_PICK(6);
    else if (p.nq <= 8) DCDCSR_PICK(8);
    else DCDCSR_PICK(12);
#undef DCDCSR_PICK
    if (int e = rowstep_optin_lds((const void*)kern, p.lds, __func__)) return e;
    dcdcsr_args& a = p.a;
    a.table = table; a.bench = bench; a.params = params; a.ids = ids; a.n = n;
    a.scale = (float)(2.0 / ((double)n * (double)dims[0]));
    a.G = G; a.part = (float*)workspace; a.partials = ctx->partials;
    hipStream_t s = (hipStream_t)stream;
    return rowstep_run(ctx, s, CDR_TAG_DCDCSR_MAP_FWD_GRAD, __func__, [&] { kern<<<dim3(p.grid), dim3(kBlock), p.lds, s>>>(a); }, p.grid,
                       rowstep_mean{(double)n * (double)dims[0]}, out8, workspace, p.total, dparams);
}
