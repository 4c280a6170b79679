// DTCDR's row-wise forward (dtcdr.py:112-126 the NeuMF tower, 182-199 the loss): one domain's batch through the element-wise maximum
// of the two domains' rows and the small ReLU MLP with dropout that sits between the rows and the loss.
//
//   x_b = [max(Us[u], Ut[u]) | max(Is[i], It[i])]   h_0 = x   h_{l+1} = relu(W_l drop_l(h_l) + b_l)   z = w_out . h_L + b_out
//   p = sigmoid(z)   g_b = w (p_b - y_b) / B   gz_{L-1} = g w_out (.) [h_L > 0]   gz_{l-1} = drop_l'(gz_l W_l) (.) [h_l > 0]
//   gx = drop_0'(gz_0 W_0), routed element by element to the table that won the maximum (1/2 : 1/2 on an exact tie, +0.0 to the loser)
//   dW_l = sum_b gz_l,b drop_l(h_l,b)^T   db_l = sum_b gz_l,b   dw_out = sum_b g_b h_L,b   db_out = sum_b g_b
//
// A workgroup of four waves stages the domain's weights once in LDS (zero-padded to the 32-wide MFMA tile) and walks row tiles of 32
// batch rows under a persistent grid.  Per tile:
//   stage  eight lanes per row read the four table rows, keep max, the routing bits and the keep bits of drop_0 in registers, write
//          drop_0(x) to LDS
//   fwd    per layer H_{l+1} = relu(drop_l(H_l) W_l^T + b_l) on v_mfma_f32_32x32x2_f32, one 32x32 output tile per wave job, drop_{l+1}
//          applied in the epilogue (a dropped unit is stored as 0: [drop(h) > 0] is the ReLU mask AND the keep mask of the backward)
//   out    z, the loss term and g_b (cdr_loss_math.h); dw_out / db_out on wave 3; gz_{L-1} written over H_L in place
//   bwd    per layer, last first: dW_l += gz_l^T drop_l(H_l) into register accumulators that live ACROSS the workgroup's tiles, db_l on
//          wave l, then gz_l W_l written over H_l in place (through the masks), for layer 0 over x
//   route  eight lanes per row: gx through the keep bits to the four compact gradient rows of the occurrence
// The weight gradients are written once, as the workgroup's partial, when its tiles are done; rowstep_finish_kernel (cdr_rowstep.h) adds the partials
// in workgroup order (no float atomics: a rerun is bit-equal) and turns the fp64 block partials of the loss into out8.
// At D = 64, hidden [32, 16] a row is ~28 kFLOP against ~2 KB of HBM traffic: near the balance of the fp32 matrix pipe and HBM, as in
// cdr_clfm.hip, which is why the contractions are on the matrix pipe.
// LDS at the widest accepted shape (D = 128, hidden [64, 64, 64]): W 101,376 + x 33,280 + H 26,112 + biases and g 1,152 = 161,920 B of
// the CU's 163,840: one workgroup per CU there, nothing spills.
#include "cdr_rowstep.h"
#include "cdr_dropout.h"

namespace {

constexpr int kML = CDR_DTCDR_MAX_LAYERS;
constexpr int kMH = CDR_DTCDR_MAX_HIDDEN;
constexpr int kChunks = 2 * CDR_DTCDR_MAX_DIM / 4 / kSub;      // float4 chunks of x one lane holds (8)
constexpr int SH = kMH + kLdsPad;            // row stride of the hidden buffers

// the tower of one domain: widths, offsets into the packed parameter vector [W_0, b_0, ..., W_{L-1}, b_{L-1}, w_out, b_out] (the
// layout of dparams and of a workgroup's partial too) and the LDS offsets of the staged weights
struct dtcdr_net {
    int L;
    int n[kML + 1];                          // n[0] = 2 D, n[l + 1] = hidden[l]
    int woff[kML], boff[kML];
    int ooff;                                // w_out; b_out at ooff + n[L]
    int total;
    int lw[kML];                             // floats: W_l in LDS, [pad32(n[l+1])][pad32(n[l]) + kLdsPad]
    int lb;                                  // floats: the biases in LDS (behind the last W_l)
    int lds_floats;
};

struct dtcdr_args {
    const float *Us, *Ut, *Is, *It;
    int D;
    const float* params;
    dtcdr_net net;
    const int64_t *uid, *iid;
    const float* label;
    int64_t B;
    float scale;                             // weight / B
    float p;
    const int64_t* seed_dev;
    uint64_t salt0;
    float *GUs, *GUt, *GIs, *GIt;            // at this domain's first row
    float* part;
    double* partials;
};

struct dtcdr_plan {
    dtcdr_net net;
    int grid, nq0;
    size_t lds;
    int64_t tiles;
};

inline bool dtcdr_shape_ok(int D, int n_hidden, const int* hidden) {
    if (!(D >= 4 && D <= CDR_DTCDR_MAX_DIM && (D & 3) == 0 && n_hidden >= 1 && n_hidden <= kML && hidden)) return false;
    for (int l = 0; l < n_hidden; ++l)
        if (hidden[l] < 1 || hidden[l] > kMH) return false;
    return true;
}

inline dtcdr_plan dtcdr_plan_for(int64_t B, int D, int n_hidden, const int* hidden) {
    dtcdr_plan p;
    dtcdr_net& N = p.net;
    N.L = n_hidden;
    N.n[0] = 2 * D;
    for (int l = 0; l < kML; ++l) N.n[l + 1] = l < n_hidden ? hidden[l] : 0;
    int off = 0, lds = 0;
    for (int l = 0; l < kML; ++l) {
        N.woff[l] = off; N.boff[l] = off; N.lw[l] = lds;
        if (l < n_hidden) {
            off += N.n[l + 1] * N.n[l];
            N.boff[l] = off;
            off += N.n[l + 1];
            lds += pad32(N.n[l + 1]) * (pad32(N.n[l]) + kLdsPad);
        }
    }
    N.ooff = off;
    N.total = off + N.n[n_hidden] + 1;
    N.lb = lds;
    lds += kML * kMH + kMH;                                           // biases, w_out
    lds += kRows * (pad32(2 * D) + kLdsPad) + n_hidden * kRows * SH + kRows;      // x, H_1 .. H_L, g
    N.lds_floats = lds;
    p.lds = (size_t)lds * sizeof(float);
    p.tiles = (B + kRows - 1) / kRows;
    p.grid = rowstep_grid(p.tiles, p.lds, 4);
    p.nq0 = ((pad32(N.n[1]) >> 5) * (pad32(2 * D) >> 5) + 3) / 4;
    return p;
}

// one element through a dropout mask: kept -> v * scale, dropped -> +0.0
__device__ __forceinline__ float drop1(float v, uint64_t seed, int64_t e, float p, float scale) {
    return cdr_drop_uniform(seed, e) >= p ? v * scale : 0.0f;
}

template <int NQ0, bool NT>
__global__ __launch_bounds__(kBlock) void dtcdr_fwd_grad_kernel(const dtcdr_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double red[kBlock / 64];
    const dtcdr_net& N = a.net;
    const int D = a.D, D4 = D >> 2, X4 = 2 * D4, L = N.L;
    const int S0 = pad32(2 * D) + kLdsPad;
    float* bs = smem + N.lb;                 // [kML][kMH]  biases, zero-padded
    float* wo = bs + kML * kMH;              // [kMH]       w_out, zero-padded
    float* Xs = wo + kMH;                    // [32][S0]    drop_0(x), later gx
    float* Hs = Xs + kRows * S0;             // [L][32][SH] drop_{l+1}(h_{l+1}), later gz_l
    float* gs = Hs + L * kRows * SH;         // [32]        g_b
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 31, lh = lane >> 5;
    const int row = t / kSub, sub = t % kSub;
    const bool drop = a.p > 0.f;
    const float dscale = drop ? 1.0f / (1.0f - a.p) : 1.0f;

    // the weights once per workgroup; the row buffers start as zeros (their columns past the widths are never written with anything else)
#pragma unroll
    for (int l = 0; l < kML; ++l) {
        if (l < L) {
            const int nin = N.n[l], nout = N.n[l + 1], S = pad32(nin) + kLdsPad, R = pad32(nout);
            float* Ws = smem + N.lw[l];
            const float* Wg = a.params + N.woff[l];
            for (int e = t; e < R * S; e += kBlock) {
                const int r = e / S, c = e - r * S;
                Ws[e] = (r < nout && c < nin) ? Wg[r * nin + c] : 0.f;
            }
            if (t < kMH) bs[l * kMH + t] = t < nout ? a.params[N.boff[l] + t] : 0.f;
        }
    }
    if (t < kMH) wo[t] = t < N.n[L] ? a.params[N.ooff + t] : 0.f;
    const float bout = a.params[N.ooff + N.n[L]];
    for (int e = t; e < kRows * S0 + L * kRows * SH; e += kBlock) Xs[e] = 0.f;

    uint64_t seed[kML];
#pragma unroll
    for (int l = 0; l < kML; ++l) seed[l] = drop ? cdr_drop_seed_dev(a.seed_dev, a.salt0 + (uint64_t)l) : 0ull;

    f32x16 w0[NQ0], w12[kML - 1];
#pragma unroll
    for (int q = 0; q < NQ0; ++q) w0[q] = zero16();
#pragma unroll
    for (int q = 0; q < kML - 1; ++q) w12[q] = zero16();
    float dbacc = 0.f, dboacc = 0.f;         // wave l < L: db_l[lane]; wave 3: dw_out[lane] and db_out
    double acc[1] = {0.0};

    for (int64_t tile = blockIdx.x; tile < (a.B + kRows - 1) / kRows; tile += gridDim.x) {
        // ---- stage: ids first, then every row load; rows past the batch are zeros with g = 0
        const int64_t b = tile * kRows + row;
        const bool valid = b < a.B;
        const int64_t bc = valid ? b : a.B - 1;
        const int64_t iu = a.uid[bc], ii = a.iid[bc];
        const float y = a.label[bc];
        float4 mx[kChunks];
        uint32_t gt = 0u, eq = 0u, keep = 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const int c = sub + kSub * j;
            mx[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < X4) {
                const bool isu = c < D4;
                const int64_t o = isu ? iu * D + 4 * c : ii * D + 4 * (c - D4);
                float4 s = mx[j], v = mx[j];
                if (valid) { s = ld4n<NT>((isu ? a.Us : a.Is) + o); v = ld4n<NT>((isu ? a.Ut : a.It) + o); }
                mx[j] = make_float4(fmaxf(s.x, v.x), fmaxf(s.y, v.y), fmaxf(s.z, v.z), fmaxf(s.w, v.w));
                // the routing of the backward, on the exact table values: source wins / target wins / neither (a tie: half each)
                gt |= (uint32_t)(s.x > v.x) << (4 * j) | (uint32_t)(s.y > v.y) << (4 * j + 1) | (uint32_t)(s.z > v.z) << (4 * j + 2) |
                      (uint32_t)(s.w > v.w) << (4 * j + 3);
                eq |= (uint32_t)(!(s.x > v.x) && !(v.x > s.x)) << (4 * j) | (uint32_t)(!(s.y > v.y) && !(v.y > s.y)) << (4 * j + 1) |
                      (uint32_t)(!(s.z > v.z) && !(v.z > s.z)) << (4 * j + 2) | (uint32_t)(!(s.w > v.w) && !(v.w > s.w)) << (4 * j + 3);
            }
        }
        if (drop) {
#pragma unroll
            for (int j = 0; j < kChunks; ++j) {
                const int c = sub + kSub * j;
                if (c < X4) {
                    const int64_t e = b * (2 * D) + 4 * c;
                    const bool k0 = cdr_drop_uniform(seed[0], e) >= a.p, k1 = cdr_drop_uniform(seed[0], e + 1) >= a.p;
                    const bool k2 = cdr_drop_uniform(seed[0], e + 2) >= a.p, k3 = cdr_drop_uniform(seed[0], e + 3) >= a.p;
                    mx[j] = make_float4(k0 ? mx[j].x * dscale : 0.f, k1 ? mx[j].y * dscale : 0.f, k2 ? mx[j].z * dscale : 0.f,
                                        k3 ? mx[j].w * dscale : 0.f);
                    keep &= ~((uint32_t)(!k0) << (4 * j) | (uint32_t)(!k1) << (4 * j + 1) | (uint32_t)(!k2) << (4 * j + 2) |
                              (uint32_t)(!k3) << (4 * j + 3));
                }
            }
        }
        __syncthreads();                     // the previous tile's routing (and the set-up) is done with Xs
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const int c = sub + kSub * j;
            if (c < X4) st4(Xs + row * S0 + 4 * c, mx[j]);
        }
        __syncthreads();

        // ---- fwd: H_{l+1} = relu(drop_l(H_l) W_l^T + b_l), then drop_{l+1}
#pragma unroll
        for (int l = 0; l < kML; ++l) {
            if (l < L) {
                const float* in = l == 0 ? Xs : Hs + (l - 1) * kRows * SH;
                const int Sin = l == 0 ? S0 : SH;
                float* out = Hs + l * kRows * SH;
                const int nin = N.n[l], nout = N.n[l + 1], SW = pad32(nin) + kLdsPad, K = (nin + 7) >> 3;
                const float* Ws = smem + N.lw[l];
                const bool dnext = drop && l + 1 < L;
                for (int job = wave; job < (pad32(nout) >> 5); job += kBlock / 64) {
                    f32x16 a16 = zero16();
                    const float* ap = in + li * Sin + 4 * lh;
                    const float* bp = Ws + (job * 32 + li) * SW + 4 * lh;
                    for (int c = 0; c < K; ++c) {
                        const float4 av = ld4(ap + 8 * c), bv = ld4(bp + 8 * c);
                        MFMA4(a16, av, bv);
                    }
                    const int col = job * 32 + li;
                    const float bias = bs[l * kMH + col];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int rr = (r & 3) + 8 * (r >> 2) + 4 * lh;
                        float h = fmaxf(a16[r] + bias, 0.f);
                        if (dnext) h = drop1(h, seed[l + 1 < kML ? l + 1 : 0], (tile * kRows + rr) * nout + col, a.p, dscale);
                        out[rr * SH + col] = h;
                    }
                }
                __syncthreads();
            }
        }

        // ---- out: the row's logit, loss term and coefficient
        float* hL = Hs + (L - 1) * kRows * SH;
        float g;
        {
            float z = 0.f;
#pragma unroll
            for (int j = 0; j < kMH / kSub; ++j) {
                const int c = sub + kSub * j;
                z += hL[row * SH + c] * wo[c];
            }
            z = group_sum<kSub>(z) + bout;
            float l;
            point_term(CDR_LOSS_BCE, z, y, a.scale, l, g);
            if (!valid) { l = 0.f; g = 0.f; }
            if (sub == 0) { gs[row] = g; acc[0] += (double)l; }
        }
        __syncthreads();
        if (wave == 3) {                     // dw_out[lane] += sum_b g_b h_L[b][lane], db_out += sum_b g_b, in row order
            for (int r = 0; r < kRows; ++r) { dbacc += gs[r] * hL[r * SH + lane]; dboacc += gs[r]; }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kMH / kSub; ++j) {           // gz_{L-1} over h_L, in place
            const int c = sub + kSub * j;
            const float h = hL[row * SH + c];
            hL[row * SH + c] = h > 0.f ? g * wo[c] : 0.f;
        }
        __syncthreads();

        // ---- bwd, last layer first
#pragma unroll
        for (int lr = 0; lr < kML; ++lr) {
            const int l = kML - 1 - lr;
            if (l < L) {
                const float* Gz = Hs + l * kRows * SH;
                float* dh = l == 0 ? Xs : Hs + (l - 1) * kRows * SH;
                const int Sd = l == 0 ? S0 : SH;
                const int nin = N.n[l], nout = N.n[l + 1], SW = pad32(nin) + kLdsPad;
                const int tI = pad32(nin) >> 5, tO = pad32(nout) >> 5;
                // dW_l += gz_l^T drop_l(H_l) over the tile's 32 rows
                if (l == 0) {
#pragma unroll
                    for (int q = 0; q < NQ0; ++q) {
                        const int ot = wave + (kBlock / 64) * q;
                        if (ot < tO * tI) {
                            const int ti = ot / tI, tj = ot - ti * tI;
                            const float* ap = Gz + lh * SH + ti * 32 + li;
                            const float* bp = dh + lh * Sd + tj * 32 + li;
#pragma unroll 4
                            for (int s = 0; s < kRows / 2; ++s) MF1(w0[q], ap[2 * s * SH], bp[2 * s * Sd]);
                        }
                    }
                } else if (wave < tO * tI) {
                    const int ti = wave / tI, tj = wave - ti * tI;
                    const float* ap = Gz + lh * SH + ti * 32 + li;
                    const float* bp = dh + lh * Sd + tj * 32 + li;
#pragma unroll 4
                    for (int s = 0; s < kRows / 2; ++s) MF1(w12[l > 0 ? l - 1 : 0], ap[2 * s * SH], bp[2 * s * Sd]);
                }
                if (wave == l) {             // db_l[lane] += sum_b gz_l[b][lane], in row order
                    for (int r = 0; r < kRows; ++r) dbacc += Gz[r * SH + lane];
                }
                __syncthreads();
                // gz_l W_l over drop_l(H_l) in place, through [drop_l(h_l) > 0] (ReLU and keep mask in one); layer 0: gx over x
                const float* Ws = smem + N.lw[l];
                const int K = (nout + 7) >> 3;
                for (int job = wave; job < tI; job += kBlock / 64) {
                    f32x16 a16 = zero16();
                    const float* ap = Gz + li * SH + 4 * lh;
                    const float* bp = Ws + (4 * lh) * SW + job * 32 + li;
                    for (int c = 0; c < K; ++c) {
                        const float4 av = ld4(ap + 8 * c);
                        const float* bq = bp + 8 * c * SW;
                        const float4 bv = make_float4(bq[0], bq[SW], bq[2 * SW], bq[3 * SW]);
                        MFMA4(a16, av, bv);
                    }
                    const int col = job * 32 + li;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int rr = (r & 3) + 8 * (r >> 2) + 4 * lh;
                        if (l == 0) dh[rr * Sd + col] = a16[r];
                        else dh[rr * Sd + col] = dh[rr * Sd + col] > 0.f ? a16[r] * dscale : 0.f;
                    }
                }
                __syncthreads();
            }
        }

        // ---- route: gx through drop_0's keep bits to the table that won each element
        if (valid) {
#pragma unroll
            for (int j = 0; j < kChunks; ++j) {
                const int c = sub + kSub * j;
                if (c < X4) {
                    const float4 gx = ld4(Xs + row * S0 + 4 * c);
                    const float e4[4] = {gx.x, gx.y, gx.z, gx.w};
                    float s4[4], t4[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t bit = 1u << (4 * j + k);
                        const float v = (keep & bit) ? e4[k] * dscale : 0.f;
                        const bool isgt = gt & bit, iseq = eq & bit;
                        s4[k] = isgt ? v : (iseq ? 0.5f * v : 0.f);
                        t4[k] = isgt ? 0.f : (iseq ? 0.5f * v : v);
                    }
                    const bool isu = c < D4;
                    const int64_t o = b * D + 4 * (isu ? c : c - D4);
                    st4n<NT>((isu ? a.GUs : a.GIs) + o, make_float4(s4[0], s4[1], s4[2], s4[3]));
                    st4n<NT>((isu ? a.GUt : a.GIt) + o, make_float4(t4[0], t4[1], t4[2], t4[3]));
                }
            }
        }
    }

    // the workgroup's partial of every parameter gradient, in the packed layout
    float* part = a.part + (size_t)blockIdx.x * N.total;
    {
        const int nin = N.n[0], nout = N.n[1], tI = pad32(nin) >> 5, tO = pad32(nout) >> 5;
#pragma unroll
        for (int q = 0; q < NQ0; ++q) {
            const int ot = wave + (kBlock / 64) * q;
            if (ot < tO * tI) {
                const int ti = ot / tI, tj = ot - ti * tI;
                STORE_TILE32(part, N.woff[0], nin, ti, tj, nout, nin, w0[q], li, lh);
            }
        }
    }
#pragma unroll
    for (int l = 1; l < kML; ++l) {
        if (l < L) {
            const int nin = N.n[l], nout = N.n[l + 1], tI = pad32(nin) >> 5, tO = pad32(nout) >> 5;
            if (wave < tO * tI) {
                const int ti = wave / tI, tj = wave - ti * tI;
                STORE_TILE32(part, N.woff[l], nin, ti, tj, nout, nin, w12[l - 1], li, lh);
            }
        }
    }
#pragma unroll
    for (int l = 0; l < kML; ++l)
        if (l < L && wave == l && lane < N.n[l + 1]) part[N.boff[l] + lane] = dbacc;
    if (wave == 3) {
        if (lane < N.n[L]) part[N.ooff + lane] = dbacc;
        if (lane == 0) part[N.ooff + N.n[L]] = dboacc;
    }
    block_sum_d<1>(acc, red);
    if (threadIdx.x == 0) store_partials(a.partials, acc);
}

}  // namespace

extern "C" int cdr_dtcdr_fwd_grad_workspace_bytes(int64_t B, int D, int n_hidden, const int* hidden, size_t* bytes) {
    CDR_CHECK_ARG(bytes && B > 0 && dtcdr_shape_ok(D, n_hidden, hidden));
    const dtcdr_plan p = dtcdr_plan_for(B, D, n_hidden, hidden);
    *bytes = (size_t)p.grid * p.net.total * sizeof(float);
    return CDR_OK;
}

extern "C" int cdr_dtcdr_fwd_grad(cdr_ctx* ctx, void* stream, const float* src_user, const float* tgt_user, const float* src_item,
                                  const float* tgt_item, int D, int n_hidden, const int* hidden, const float* params, const int64_t* uid,
                                  const int64_t* iid, const float* label, int64_t B, float weight, float p_drop, const int64_t* seed_dev,
                                  uint64_t salt0, int64_t row0, float* out8, float* GUs, float* GUt, float* GIs, float* GIt, float* dparams,
                                  void* workspace, size_t workspace_bytes) {
    CDR_CHECK_ARG(ctx && src_user && tgt_user && src_item && tgt_item && params && uid && iid && label && out8 && GUs && GUt && GIs && GIt &&
                  dparams && workspace);
    CDR_CHECK_ARG(B > 0 && row0 >= 0 && dtcdr_shape_ok(D, n_hidden, hidden));
    CDR_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f && (p_drop == 0.f || seed_dev));
    CDR_CHECK_ARG((((uintptr_t)src_user | (uintptr_t)tgt_user | (uintptr_t)src_item | (uintptr_t)tgt_item | (uintptr_t)GUs | (uintptr_t)GUt |
                    (uintptr_t)GIs | (uintptr_t)GIt) & 15) == 0);
    const dtcdr_plan p = dtcdr_plan_for(B, D, n_hidden, hidden);
    CDR_CHECK_ARG(workspace_bytes >= (size_t)p.grid * p.net.total * sizeof(float));
    static_assert(CDR_DTCDR_MAX_DIM == 128 && kChunks * kSub * 4 == 2 * CDR_DTCDR_MAX_DIM && kChunks * 4 == 32,
                  "a lane holds eight float4 chunks of x and one routing bit per element in a 32-bit word; NQ0 covers 1..4");
    static_assert(CDR_DTCDR_MAX_HIDDEN == 64 && CDR_DTCDR_MAX_LAYERS == 3 && kBlock / 64 == 4,
                  "a hidden layer is one lane per unit of a wave; waves 0..2 keep db_l, wave 3 dw_out; dW_1 and dW_2 are at most four tiles");
    static_assert(CDR_NUM_CU * 4 <= CDR_MAX_PARTIAL_BLOCKS, "one partial slot per workgroup");
    if (p.lds > kLdsPerCu) { cdr_set_error("cdr_dtcdr_fwd_grad: %zu B of LDS for this shape", p.lds); return CDR_EINVAL; }
    using kern_fn = void (*)(const dtcdr_args);
    const bool nt = D * 4 >= 512;                              // non-temporal row traffic from 512-byte rows up (cdr_common.h)
    kern_fn kern = nullptr;
#define DTCDR_PICK(NQ) kern = nt ? dtcdr_fwd_grad_kernel<NQ, true> : dtcdr_fwd_grad_kernel<NQ, false>
    switch (p.nq0) {
        case 1: DTCDR_PICK(1); break;
        case 2: DTCDR_PICK(2); break;
        case 3: DTCDR_PICK(3); break;
        default: DTCDR_PICK(4); break;
    }
#undef DTCDR_PICK
    if (int e = rowstep_optin_lds((const void*)kern, p.lds, __func__)) return e;
    dtcdr_args a;
    a.Us = src_user; a.Ut = tgt_user; a.Is = src_item; a.It = tgt_item; a.D = D;
    a.params = params; a.net = p.net;
    a.uid = uid; a.iid = iid; a.label = label; a.B = B;
    a.scale = weight * (1.0f / (float)B);
    a.p = p_drop; a.seed_dev = seed_dev; a.salt0 = salt0;
    a.GUs = GUs + row0 * D; a.GUt = GUt + row0 * D; a.GIs = GIs + row0 * D; a.GIt = GIt + row0 * D;
    a.part = (float*)workspace; a.partials = ctx->partials;
    hipStream_t s = (hipStream_t)stream;
    return rowstep_run(ctx, s, CDR_TAG_DTCDR_FWD_GRAD, __func__, [&] { kern<<<dim3(p.grid), dim3(kBlock), p.lds, s>>>(a); }, p.grid,
                       rowstep_bce{B, weight}, out8, workspace, p.net.total, dparams);
}
