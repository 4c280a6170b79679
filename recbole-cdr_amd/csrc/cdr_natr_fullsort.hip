// NATR full-sort scoring of phase 2 in ONE launch (natr.py:112-156 over every (evaluated user, target item) pair; predict :178-191).
// The reference -- and this project's fallback -- repeats every user row N times and calls predict in chunks; per pair that gathers
// max_inter_length source rows, runs the transfer layer and a softmax again.  None of that depends on the pair: the history, the transfer
// layer, the unit attention and the weighted sum su depend on the KEY alone (the user in overlap_items mode, the item in overlap_users
// mode) and are computed once per key by functional.natr_history_summary.  What is left per pair, with a = su of the key, p = the key's
// own target row, q = the other side's target row, w = domain_attention_layer.weight:
//      b_s = w . relu(a (.) q) + b_d    b_p = w . relu(p (.) q) + b_d    beta = e^b_s / (e^b_s + e^b_p)
//      score = sigmoid((beta a + (1 - beta) p) . q)
// beta = sigmoid(b_s - b_p) (b_d cancels), relu(x) = (x + |x|) / 2 with |a_d q_d| = |a_d| |q_d|, and
// (beta a + (1 - beta) p) . q = p . q + beta ((a - p) . q).  With D_ = a - p and M = |a| - |p| (elementwise):
//      g = (w/2 (.) D_) . q + (w/2 (.) M) . |q|   (= b_s - b_p)            score = sigmoid(p . q + sigmoid(g) (D_ . q))
// -- three accumulators per pair over a total K of 4 Dt, every term a plain fp32 dot product: all of it runs on v_mfma_f32_32x32x2_f32 and
// the VALU does the two sigmoids.  No ReLU is evaluated, so no unit has an ambiguous branch.  The kernel forms sigmoid(g), not
// e^b_s / (e^b_s + e^b_p): the same number wherever the reference's form is finite; the reference's is NaN once a gate logit passes ~88.
//
// Layout.  An MFMA tile is 32 users (rows, the A operand) x 32 items (columns, the B operand); a wave owns a tile of 32 items and keeps
// their rows in registers for all the users it serves (lane (c, h): features h S .. h S + S - 1 of item c, S = DP / 2, so K step s of the
// chain contracts features s and S + s), the workgroup's chunk of 32 users sits in LDS as Ul[operand][f / 4][user][f % 4]: a lane's four
// K steps are one 16-byte read, the 32 users of a group one 512-byte run (conflict-free).
//   overlap_items (key = user): the chunk holds the user's four stacked operands p, D_, w/2 (.) D_, w/2 (.) M, formed while it is staged
//     (64 KB at Dt = 128); the item registers hold q, and |q| is one VALU operation per K step next to four MFMAs.
//   overlap_users (key = item): the item registers hold a and p (2 S = 128 registers at Dt = 128; the four stacked operands would be 256 and
//     are never held: D_, M and their products with w/2 -- w/2 sits in LDS -- are formed per K step, four VALU operations next to four MFMAs);
//     the chunk holds the users' q.
// Both modes feed the MFMAs the same operand values, rounded the same way.  Nothing but rows and the scores touches memory.
//
// Two epilogues, one scoring body (template parameter TOPK), as in cdr_conet_fullsort.hip / cdr_deepapf_fullsort.hip: out[u][item], or
// per-user running top-k lists behind the evaluation mask (cdr_topk.h) written as partial lists for topk_merge_launch.  The score is the
// same instruction sequence in both, so listed values are bit-equal to stored ones.
#include "cdr_common.h"
#include "cdr_mfma.h"
#include "cdr_topk.h"
#include "cdr_fullsort_tile.h"

namespace {

constexpr int kNfWaves = 8;                      // item tiles per workgroup pass (two waves per SIMD)
constexpr int kNfBlock = 64 * kNfWaves;
constexpr int kNfUsers = 32;                     // users per LDS chunk: the rows of one MFMA tile
// TOPK launch geometry (cdr_topk.h): the 64 KB of lists and queues lie next to at most 64 KB of chunk -- 64 users per workgroup at k = 10
// (a multiple of the 32-user chunk where that many fit), 12 at k = 64.  One workgroup per CU, eight stripes each (at most 8 x 256); the
// sample call runs 4 x 8 = 32 stripes.
constexpr topk_stripe_geom kNfTopkGeom{kNfWaves, 0, CDR_NUM_CU, 4, kNfUsers};

struct nf_args {
    const float* su;                             // [keys, D]: the key side's history summary, by POSITION (user u / item i)
    const float* ptab;                           // the key side's own target table
    const float* qtab;                           // the other side's target table
    int64_t ld_su, ld_p, ld_q;
    const int64_t* uid;                          // [U] evaluated users (rows of the user-side table)
    int64_t U, N;
    int D;
    const float* w;                              // [D] domain_attention_layer.weight
    float* out; int64_t ldo;                     // [U, N]
    int users_per_block;
};
struct nf_args_topk : nf_args { topk_out tk; };
template <bool TOPK> using nf_kargs = std::conditional_t<TOPK, nf_args_topk, nf_args>;

// floats of the fixed LDS part: the user chunk (four stacked operands, or q alone) | w / 2
__host__ __device__ constexpr size_t nf_fixed_words(int DP, bool itemkey) {
    return (size_t)kNfUsers * (itemkey ? 1 : 4) * DP + DP;
}

__device__ __forceinline__ float nf_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// users [u0, u0 + nu) into LDS as Ul[operand][f / 4][user][f % 4], zero beyond nu and beyond D.  A thread takes (feature group, user)
// with the user running fastest: its 16-byte LDS writes are conflict-free.
template <int NB, bool ITEMKEY>
__device__ __forceinline__ void nf_stage_users(const nf_args& a, float* __restrict__ Ul, int64_t u0, int nu) {
    constexpr int DP = 32 * NB, Q = DP / 4;
    for (int e = threadIdx.x; e < kNfUsers * Q; e += kNfBlock) {
        const int g = e >> 5, uu = e & 31, f = 4 * g;
        const bool ok = uu < nu && f < a.D;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        float* const dst = Ul + ((size_t)g * kNfUsers + uu) * 4;
        if constexpr (ITEMKEY) {
            const float4 q = ok ? ld4(a.qtab + a.uid[u0 + uu] * a.ld_q + f) : zero;
            st4(dst, q);
        } else {
            float4 s = zero, p = zero, wh = zero;
            if (ok) {
                s = ld4(a.su + (u0 + uu) * a.ld_su + f);
                p = ld4(a.ptab + a.uid[u0 + uu] * a.ld_p + f);
                wh = make_float4(0.5f * a.w[f], 0.5f * a.w[f + 1], 0.5f * a.w[f + 2], 0.5f * a.w[f + 3]);
            }
            const float4 d = make_float4(s.x - p.x, s.y - p.y, s.z - p.z, s.w - p.w);
            const float4 m = make_float4(fabsf(s.x) - fabsf(p.x), fabsf(s.y) - fabsf(p.y), fabsf(s.z) - fabsf(p.z), fabsf(s.w) - fabsf(p.w));
            constexpr size_t OP = (size_t)Q * kNfUsers * 4;
            st4(dst, p);
            st4(dst + OP, d);
            st4(dst + 2 * OP, make_float4(wh.x * d.x, wh.y * d.y, wh.z * d.z, wh.w * d.w));
            st4(dst + 3 * OP, make_float4(wh.x * m.x, wh.y * m.y, wh.z * m.z, wh.w * m.w));
        }
    }
}

template <int NB, bool ITEMKEY, bool TOPK>
__global__ __launch_bounds__(kNfBlock) void natr_fullsort_kernel(nf_kargs<TOPK> a) {
    constexpr int DP = 32 * NB, S = 16 * NB, Q = DP / 4, S1 = ITEMKEY ? S : 1;
    constexpr size_t OP = (size_t)Q * kNfUsers * 4;                       // floats of one stacked operand of the chunk
    extern __shared__ __attribute__((aligned(16))) float nf_lds[];
    float* const Ul = nf_lds;
    float* const wl = Ul + (size_t)kNfUsers * (ITEMKEY ? 1 : 4) * DP;
    float* const dyn = wl + DP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const int D = a.D;
    const int64_t u_lo = (int64_t)blockIdx.y * a.users_per_block;
    const int64_t u_hi = u_lo + a.users_per_block < a.U ? u_lo + a.users_per_block : a.U;
    const bool one_chunk = u_hi - u_lo <= kNfUsers;           // staged once, not once per tile round
    if (one_chunk) nf_stage_users<NB, ITEMKEY>(a, Ul, u_lo, (int)(u_hi - u_lo));
    for (int t = threadIdx.x; t < DP; t += kNfBlock) wl[t] = t < D ? 0.5f * a.w[t] : 0.f;
    topk_wave_lists lists;                                    // TOPK: this wave's lists of the workgroup's users, all empty
    if constexpr (TOPK) lists.init(dyn, wave, a.users_per_block, a.tk.k, a.tk, u_lo, a.U);
    // this lane's view of the chunk: user row c, K groups h S / 4 ..
    const float* const ua = Ul + ((size_t)(h * (S / 4)) * kNfUsers + c) * 4;
    const float* const wh = wl + h * S;

    const int64_t n_tiles = (a.N + 31) >> 5;
    const int64_t tile_stride = (int64_t)gridDim.x * kNfWaves;
    const int64_t rounds = (n_tiles + tile_stride - 1) / tile_stride;        // the same for every wave: the chunk is staged behind barriers
    __syncthreads();
    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t tile = ((int64_t)rd * gridDim.x + blockIdx.x) * kNfWaves + wave;
        const bool live = tile < n_tiles;
        const int64_t item = tile * 32 + c;
        const bool iv = live && item < a.N;
        // the tile's rows.  overlap_items: r0 = q.  overlap_users: r0 = a (su of the item), r1 = p
        float r0[S], r1[S1];
        if constexpr (ITEMKEY) {
            tile_load_row<S>(r0, a.su + (iv ? item : 0) * a.ld_su, iv, h, D);
            tile_load_row<S>(r1, a.ptab + (iv ? item : 0) * a.ld_p, iv, h, D);
        } else {
            tile_load_row<S>(r0, a.qtab + (iv ? item : 0) * a.ld_q, iv, h, D);
        }
        for (int64_t u0 = u_lo; u0 < u_hi; u0 += kNfUsers) {
            const int nu = (int)(u_hi - u0 < kNfUsers ? u_hi - u0 : kNfUsers);
            if (!one_chunk) {
                __syncthreads();                                           // the previous chunk has been consumed by every wave
                nf_stage_users<NB, ITEMKEY>(a, Ul, u0, nu);
                __syncthreads();
            }
            if (!live) continue;
            if constexpr (ITEMKEY) {
                // (the differences below do not change from chunk to chunk; hoisted out of this loop they would be 2 S more live registers)
#pragma unroll
                for (int s = 0; s < S; ++s) asm volatile("" : "+v"(r0[s]), "+v"(r1[s]));
            }
            f32x16 cp = zero16(), cd = zero16(), cg = zero16();            // p . q | D_ . q | g
            float4 v0 = ld4(ua), v1 = v0, v2 = v0, v3 = v0, nw = ld4(wh);
            if constexpr (!ITEMKEY) { v1 = ld4(ua + OP); v2 = ld4(ua + 2 * OP); v3 = ld4(ua + 3 * OP); }
#pragma unroll
            for (int s = 0; s < S; s += 4) {
                float4 n0 = v0, n1 = v1, n2 = v2, n3 = v3, nnw = nw;
                if (s + 4 < S) {                                           // the operands of K group s + 4 are read while group s runs
                    const float* const nx = ua + (size_t)(s / 4 + 1) * kNfUsers * 4;
                    n0 = ld4(nx);
                    if constexpr (!ITEMKEY) { n1 = ld4(nx + OP); n2 = ld4(nx + 2 * OP); n3 = ld4(nx + 3 * OP); }
                    else nnw = ld4(wh + s + 4);
                }
                const float x0[4] = {v0.x, v0.y, v0.z, v0.w};
                if constexpr (!ITEMKEY) {
                    const float x1[4] = {v1.x, v1.y, v1.z, v1.w}, x2[4] = {v2.x, v2.y, v2.z, v2.w}, x3[4] = {v3.x, v3.y, v3.z, v3.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float q = r0[s + j];
                        MF1(cp, x0[j], q); MF1(cd, x1[j], q); MF1(cg, x2[j], q); MF1(cg, x3[j], fabsf(q));
                    }
                } else {
                    const float xw[4] = {nw.x, nw.y, nw.z, nw.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float sa = r0[s + j], p = r1[s + j], q = x0[j];
                        const float d = sa - p, m = fabsf(sa) - fabsf(p);
                        MF1(cp, q, p); MF1(cd, q, d); MF1(cg, q, xw[j] * d); MF1(cg, fabsf(q), xw[j] * m);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                v0 = n0; v1 = n1; v2 = n2; v3 = n3; nw = nnw;
            }
            // register i = 4 g + j of half h holds user row 8 g + 4 h + j of the chunk, item c
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = 8 * (i >> 2) + 4 * h + (i & 3);
                const float sg = nf_sigmoid(cg[i]);
                const float sc = nf_sigmoid(fmaf(sg, cd[i], cp[i]));
                const bool ok = iv && row < nu;
                if constexpr (!TOPK) {
                    if (ok) a.out[(u0 + row) * a.ldo + item] = sc;
                } else {
                    const int ul = (int)(u0 - u_lo) + row;                  // (every lane may carry a candidate: at most 64 per call)
                    lists.template offer<64>(ok && sc > lists.thr(ok ? ul : 0), sc, (int)item, ul, a.tk, u_lo);
                }
            }
        }
    }
    if constexpr (TOPK) lists.finish(a.tk, kNfWaves, u_lo, u_hi, a.U);
}

template <bool TOPK>
int nf_dispatch(const nf_kargs<TOPK>& a, bool itemkey, dim3 grid, size_t list_bytes, hipStream_t s) {
    const size_t lds = sizeof(float) * nf_fixed_words(32 * ((a.D + 31) / 32), itemkey) + list_bytes;
    const int rc = tile_dispatch(a.D, itemkey, [&](auto nb, auto ik) {
        return tile_launch_one("cdr_natr_fullsort", natr_fullsort_kernel<nb(), ik(), TOPK>, a, grid, kNfBlock, lds, s);
    });
    if (rc < 0) { cdr_set_error("cdr_natr_fullsort: Dt = %d outside the kernel's range", a.D); return CDR_EINVAL; }
    return rc;
}

// score epilogue: a few workgroups per CU (cdr_fullsort_tile.h)
int nf_launch_scores(const nf_args& a, bool itemkey, hipStream_t s) {
    nf_args b = a;
    dim3 grid;
    if (const int rc = tile_score_grid("cdr_natr_fullsort", a.U, a.N, kNfWaves, kNfUsers, &grid, &b.users_per_block)) return rc;
    return nf_dispatch<false>(b, itemkey, grid, 0, s);
}

// the arguments both entries share; nothing is launched for a refused call
int nf_check(const char* fn, const float* su, int64_t ld_su, const float* key_tab, int64_t ld_key, const float* other_tab, int64_t ld_other,
             const int64_t* uid, int64_t U, int64_t N, int Dt, const float* w) {
    if (!cdr_natr_fullsort_supported(Dt)) {
        cdr_set_error("%s: Dt = %d outside the kernel's range (4..128, a multiple of 4)", fn, Dt);
        return CDR_EINVAL;
    }
    if (U < 1 || N < 1 || N >= ((int64_t)1 << 31) || U >= ((int64_t)1 << 31)) {
        cdr_set_error("%s: U = %lld, N = %lld outside 1 <= U, N < 2^31", fn, (long long)U, (long long)N);
        return CDR_EINVAL;
    }
    if (!su || !key_tab || !other_tab || !uid || !w) { cdr_set_error("%s: null argument", fn); return CDR_EINVAL; }
    if (ld_su < Dt || ld_key < Dt || ld_other < Dt || ((ld_su | ld_key | ld_other) & 3) ||
        (((uintptr_t)su | (uintptr_t)key_tab | (uintptr_t)other_tab) & 15)) {
        cdr_set_error("%s: su and the tables must be 16-byte aligned with row strides >= Dt that are multiples of 4", fn);
        return CDR_EINVAL;
    }
    return CDR_OK;
}

nf_args nf_fill(const float* su, int64_t ld_su, const float* key_tab, int64_t ld_key, const float* other_tab, int64_t ld_other,
                const int64_t* uid, int64_t U, int64_t N, int Dt, const float* w) {
    nf_args a{};
    a.su = su; a.ld_su = ld_su; a.ptab = key_tab; a.ld_p = ld_key; a.qtab = other_tab; a.ld_q = ld_other;
    a.uid = uid; a.U = U; a.N = N; a.D = Dt; a.w = w;
    return a;
}

}  // namespace

extern "C" int cdr_natr_fullsort_supported(int Dt) { return Dt >= 4 && Dt <= 128 && (Dt & 3) == 0 ? 1 : 0; }

extern "C" int cdr_natr_fullsort(void* stream, int key_is_item, const float* su, int64_t ld_su, const float* key_tab, int64_t ld_key,
                                 const float* other_tab, int64_t ld_other, const int64_t* uid, int64_t U, int64_t N, int Dt, const float* w,
                                 float* out, int64_t ldo) {
    const int rc = nf_check("cdr_natr_fullsort", su, ld_su, key_tab, ld_key, other_tab, ld_other, uid, U, N, Dt, w);
    if (rc) return rc;
    CDR_CHECK_ARG(out && ldo >= N);
    nf_args a = nf_fill(su, ld_su, key_tab, ld_key, other_tab, ld_other, uid, U, N, Dt, w);
    a.out = out; a.ldo = ldo;
    return nf_launch_scores(a, key_is_item != 0, (hipStream_t)stream);
}

extern "C" int cdr_natr_fullsort_topk_workspace_bytes(int64_t U, int64_t N, int k, size_t* bytes) {
    return topk_stripe_ws_query("cdr_natr_fullsort_topk_workspace_bytes", kNfTopkGeom, U, N, k, bytes);
}

extern "C" int cdr_natr_fullsort_topk(void* stream, int key_is_item, const float* su, int64_t ld_su, const float* key_tab, int64_t ld_key,
                                      const float* other_tab, int64_t ld_other, const int64_t* uid, int64_t U, int64_t N, int Dt,
                                      const float* w, int k, const int64_t* hist_indptr, const int64_t* hist_cols, int exclude_first_col,
                                      float* out_vals, int64_t* out_idx, void* workspace, size_t workspace_bytes) {
    if (const int rc = topk_check_k("cdr_natr_fullsort_topk", k)) return rc;
    const int rc0 = nf_check("cdr_natr_fullsort_topk", su, ld_su, key_tab, ld_key, other_tab, ld_other, uid, U, N, Dt, w);
    if (rc0) return rc0;
    CDR_CHECK_ARG(out_vals && out_idx && workspace);
    CDR_CHECK_ARG((hist_indptr == nullptr) == (hist_cols == nullptr));
    nf_args_topk a{};
    static_cast<nf_args&>(a) = nf_fill(su, ld_su, key_tab, ld_key, other_tab, ld_other, uid, U, N, Dt, w);
    hipStream_t s = (hipStream_t)stream;
    return topk_seeded_run("cdr_natr_fullsort_topk", kNfTopkGeom, s, U, N, k, topk_mask{hist_indptr, hist_cols, exclude_first_col}, out_vals,
                           out_idx, workspace, workspace_bytes, [&](int64_t n_cols, const topk_stripe_plan& p, const topk_out& tk) {
                               nf_args_topk b = a;
                               b.N = n_cols; b.users_per_block = p.upb; b.tk = tk;
                               return nf_dispatch<true>(b, key_is_item != 0, dim3((unsigned)p.gx, (unsigned)p.gy), p.lds, s);
                           });
}
