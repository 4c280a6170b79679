// Fused row-wise training step for tables too large for dense gradients / dense Adam (BASELINE config C5).
//
// Every fused entry point is one call of five stages on one stream (host helpers: "what the host entry points share" and
// "the fused step's skeleton" below):
//   1 EmbLoss head       embloss_head: norms of the batch's rows -> coefficients (+ head counters cleared, device update counts)
//   2 sort and flags     sort_ids_with (stable rocPRIM radix sort of both tables' ids, one key space) + occ_flags: every row's
//                        occurrences become one segment; flags = "only occurrence", heads of the duplicate segments (heads_view)
//   3 forward set-up     make_tables: table pointers + optimizer scalars of both sides
//   4 forward-and-apply  the variant's own kernel: rows occurring once updated in place, duplicates leave gradient rows
//   5 tail               finish_and_apply_dups: dups_plan_make -> the variant's one-block finishing kernel -> apply_dups_pair
//                        (segment sums in occurrence order: deterministic, no float atomics; EmbLoss term count * c * W[r])
// What varies: cdr_bpr_step_fused[_dev] stage 1-2 (count path: ids without a sort) and 4; cdr_point_step_fused 4;
// cdr_*_step_fused_kmajor 1 (point), 4 and the item side's limits; cdr_*_step_presort + cdr_bpr_step_from_diff /
// cdr_point_step_from_dot split 2 from 1, 4, 5 around an all-reduce; cdr_bpr_shard_local_step sorts users only;
// cdr_bpr_shard_plan + cdr_bpr_shard_step own key-making kernel in 2, the shard kernels in 5; cdr_point_step_fused_pair_dev own
// kernels in 1, 2 (key making), 4 and the finish.  cdr_bpr_fwd_grad / cdr_sort_ids / cdr_rowwise_apply are the unfused calls.
//
// Semantics: exactly "sum of the batch's gradients evaluated at the pre-step weights", as autograd + a dense optimizer
// would compute for the touched rows.  Rows not in the batch are not touched (for Adam this is the usual lazy/sparse
// variant: untouched rows keep their moments and do not move) -- documented in DESIGN.md as the one deliberate
// difference from the reference's dense torch.optim.Adam, which is O(table) per step.
#include <cstdlib>
#include <cstring>
#include <string.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include "cdr_common.h"
#include "cdr_adam_math.h"
#include "cdr_opt_math.h"
#include "cdr_loss_math.h"

namespace {

constexpr int kUnroll = 4;

// EmbLoss norms from a per-row cache ("EmbLoss norms from a per-row cache" below): floats per record.  Slot 0 = ||W[r]||^2, the rest is
// padding, so that a record is one whole 64-byte burst at the memory (the first cache's 4-byte records were partial-line
// read-modify-writes: 0.26-0.30 ms per forward launch).  -DCDR_NORM_REC_FLOATS=32 builds the 128-byte form for the A/B.
#ifndef CDR_NORM_REC_FLOATS
#define CDR_NORM_REC_FLOATS 16
#endif
constexpr int kNormRecFloats = CDR_NORM_REC_FLOATS;
static_assert(kNormRecFloats == 16 || kNormRecFloats == 32, "a record is one 64-byte or one 128-byte burst");

// A lane's share of a row's squared norm for the records, in the very operations batch_norms_kernel's dot4(w, w) compiles to -- the
// writers must produce the float the gather would, and left to itself hipcc contracts their copy of dot4 differently (that was the first
// cache's "1 ulp off").  Read off batch_norms_kernel's ISA: rows of 512 bytes and more (LPR >= 32, non-temporal loads) take one multiply
// and three fused multiply-adds, y first; narrower rows take packed multiplies and three plain additions.  tests/test_gpu_norm_cache.py
// holds every lane width to it (cache against gather, bit for bit).
template <int LPR>
__device__ __forceinline__ float sqnorm4(float4 a) {
    if constexpr (LPR >= 32) {
        return __builtin_fmaf(a.w, a.w, __builtin_fmaf(a.z, a.z, __builtin_fmaf(a.x, a.x, a.y * a.y)));
    } else {
#pragma clang fp contract(off)
        const float xx = a.x * a.x, yy = a.y * a.y, zz = a.z * a.z, ww = a.w * a.w;
        return ((xx + yy) + zz) + ww;
    }
}

// The lane group of a row writes the row's record whole (lane `sub` its float4 chunks), past the caches: s = the row's squared norm, in
// every lane of the group (group_sum).
template <int LPR>
__device__ __forceinline__ void norm_rec_store(float* __restrict__ rec, float s, int sub) {
#pragma unroll
    for (int c = 0; c < kNormRecFloats / 4; c += LPR) {
        if (c + sub < kNormRecFloats / 4) st4n<true>(rec + 4 * (c + sub), make_float4(c + sub == 0 ? s : 0.f, 0.f, 0.f, 0.f));
    }
}

// ------------------------------------------------------------------------------------------------ forward + compact grads
// SCATTER (row-sharded step): the item operand is the buffer of received rows, one entry per occurrence, and the item
// gradients are written straight into the send buffer at the same positions: GP[pid[t]] = g u, GP[nid[t]] = -g u.
template <int LPR, bool SCATTER>
__global__ __launch_bounds__(kBlock) void bpr_fwd_grad_kernel(const float* __restrict__ U, const float* __restrict__ I,
                                                              int D, const int64_t* __restrict__ uid,
                                                              const int64_t* __restrict__ pid,
                                                              const int64_t* __restrict__ nid, int64_t B, float gamma,
                                                              float invB, float* __restrict__ GU,
                                                              float* __restrict__ GP, double* __restrict__ partials) {
    constexpr int GPB = kBlock / LPR;
    __shared__ double smem[3 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int D4 = D >> 2;
    double acc[3] = {0.0, 0.0, 0.0};
    const bool live = sub < D4;

    for (int64_t base = gg; base < B; base += TG * kUnroll) {
        float4 u[kUnroll], p[kUnroll], n[kUnroll];
        // ids of all kUnroll triples first, THEN all row loads: vmcnt is an in-order counter, so interleaving
        // "ids(r) -> rows(r)" makes the wait for ids(r+1) also wait for rows(r) and serialises the gathers
        int64_t iu[kUnroll], ip[kUnroll], in[kUnroll];
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const int64_t tc = t < B ? t : B - 1;
            iu[r] = uid[tc]; ip[r] = pid[tc]; in[r] = nid[tc];
        }
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            u[r] = p[r] = n[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < B && live) {
                u[r] = ld4n<(LPR >= 32)>(U + iu[r] * D + 4 * sub);
                p[r] = ld4n<(LPR >= 32)>(I + ip[r] * D + 4 * sub);
                n[r] = ld4n<(LPR >= 32)>(I + in[r] * D + 4 * sub);
            }
        }
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const float dp = group_sum<LPR>(dot4(u[r], p[r]));
            const float dn = group_sum<LPR>(dot4(u[r], n[r]));
            const float su = group_sum<LPR>(dot4(u[r], u[r]));
            const float sp = group_sum<LPR>(dot4(p[r], p[r]));
            if (t < B) {
                const float s = sigmoidf_(dp - dn);
                const float g = bpr_grad(s, gamma, invB);
                if (live) {
                    st4n<(LPR >= 32)>(GU + t * D + 4 * sub, scale_diff4(g, p[r], n[r]));
                    if (SCATTER) {
                        st4n<(LPR >= 32)>(GP + ip[r] * D + 4 * sub, scale4(g, u[r]));
                        st4n<(LPR >= 32)>(GP + in[r] * D + 4 * sub, scale4(-g, u[r]));
                    } else {
                        st4n<(LPR >= 32)>(GP + t * D + 4 * sub, scale4(g, u[r]));
                    }
                }
                if (sub == 0) {
                    acc[0] += (double)bpr_loss(s, gamma);
                    acc[1] += (double)su;
                    acc[2] += (double)sp;
                }
            }
        }
    }
    block_sum_d<3>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// Pointwise counterpart (EMCDR's default MF latent factor model: emcdr.py:111-122, MSE on the raw dot; BCE on sigmoid(dot) as in
// cmf.py:75-99): one pass over the batch's (user, item, label) rows; compact gradient rows GU[b] = g_b i_b, GI[b] = g_b u_b.
template <int LPR>
__global__ __launch_bounds__(kBlock) void point_fwd_grad_kernel(int loss_kind, const float* __restrict__ U, const float* __restrict__ I,
                                                                int D, const int64_t* __restrict__ uid, const int64_t* __restrict__ iid,
                                                                const float* __restrict__ label, int64_t B, float invB,
                                                                float* __restrict__ GU, float* __restrict__ GI,
                                                                double* __restrict__ partials) {
    constexpr int GPB = kBlock / LPR;
    __shared__ double smem[3 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int D4 = D >> 2;
    double acc[3] = {0.0, 0.0, 0.0};
    const bool live = sub < D4;
    for (int64_t base = gg; base < B; base += TG * kUnroll) {
        float4 u[kUnroll], v[kUnroll];
        int64_t iu[kUnroll], ii[kUnroll];
        float yl[kUnroll];
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {                  // ids and labels first, then every row load (vmcnt is in-order)
            const int64_t t = base + (int64_t)r * TG;
            const int64_t tc = t < B ? t : B - 1;
            iu[r] = uid[tc]; ii[r] = iid[tc]; yl[r] = label[tc];
        }
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            u[r] = v[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < B && live) {
                u[r] = ld4n<(LPR >= 32)>(U + iu[r] * D + 4 * sub);
                v[r] = ld4n<(LPR >= 32)>(I + ii[r] * D + 4 * sub);
            }
        }
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const float dx = group_sum<LPR>(dot4(u[r], v[r]));
            const float su = group_sum<LPR>(dot4(u[r], u[r]));
            const float si = group_sum<LPR>(dot4(v[r], v[r]));
            if (t < B) {
                const float y = yl[r];
                float l, g;                                    // point_term (cdr_loss_math.h), in place: the helper changed this kernel's code
                if (loss_kind == CDR_LOSS_MSE) {
                    const float d = dx - y;
                    l = d * d; g = 2.0f * d * invB;
                } else {
                    const float p = sigmoidf_(dx);
                    l = (y - 1.0f) * fmaxf(logf(1.0f - p), -100.0f) - y * fmaxf(logf(p), -100.0f);
                    const float pq = (1.0f - p) * p;
                    g = (p - y) / fmaxf(pq, 1e-12f) * invB * pq;
                }
                if (live) {
                    st4n<(LPR >= 32)>(GU + t * D + 4 * sub, make_float4(g * v[r].x, g * v[r].y, g * v[r].z, g * v[r].w));
                    st4n<(LPR >= 32)>(GI + t * D + 4 * sub, make_float4(g * u[r].x, g * u[r].y, g * u[r].z, g * u[r].w));
                }
                if (sub == 0) { acc[0] += (double)l; acc[1] += (double)su; acc[2] += (double)si; }
            }
        }
    }
    block_sum_d<3>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// SSCDR's domain loss (sscdr.py:120-128, 133-159): TripletMarginLoss on the squared-norm "normalised" rows of a (user, positive,
// negative) triple, and its gradient taken back through the normalisation to the three gathered rows -- one compact gradient row per
// OCCURRENCE: GU[t] (user), GI[t] (positive), GI[B + t] (negative), so that the segmented applies add and never negate.  A lane keeps
// its float4 of the three rows and makes the three gradient float4s from them; eight group reductions per triple (three squared
// norms, two distances, three <row, gradient> dots).  Lanes past the row's width hold zeros and are kept out of the distances (their
// difference would be eps, not 0).  partials: [0] sum of the hinge terms, [1] triples with an open hinge.
template <int LPR>
__device__ __forceinline__ float4 sqnorm_bwd4(float4 x, float4 g, float L) {
    const float d = group_sum<LPR>(dot4(x, g));
    return make_float4(sqnorm_bwd_elem(x.x, g.x, L, d), sqnorm_bwd_elem(x.y, g.y, L, d), sqnorm_bwd_elem(x.z, g.z, L, d),
                       sqnorm_bwd_elem(x.w, g.w, L, d));
}

template <int LPR>
__global__ __launch_bounds__(kBlock) void triplet_fwd_grad_kernel(const float* __restrict__ U, const float* __restrict__ I, int D,
                                                                  const int64_t* __restrict__ uid, const int64_t* __restrict__ pid,
                                                                  const int64_t* __restrict__ nid, int64_t B, float margin, float eps,
                                                                  float invB, float* __restrict__ GU, float* __restrict__ GI,
                                                                  double* __restrict__ partials) {
    constexpr int GPB = kBlock / LPR;
    __shared__ double smem[2 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int D4 = D >> 2;
    double acc[2] = {0.0, 0.0};
    const bool live = sub < D4;
    const float e = live ? eps : 0.f;

    for (int64_t base = gg; base < B; base += TG * kUnroll) {
        float4 u[kUnroll], p[kUnroll], n[kUnroll];
        int64_t iu[kUnroll], ip[kUnroll], in[kUnroll];
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {                  // ids of every triple first, then every row load (vmcnt is in-order)
            const int64_t t = base + (int64_t)r * TG;
            const int64_t tc = t < B ? t : B - 1;
            iu[r] = uid[tc]; ip[r] = pid[tc]; in[r] = nid[tc];
        }
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            u[r] = p[r] = n[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < B && live) {
                u[r] = ld4n<(LPR >= 32)>(U + iu[r] * D + 4 * sub);
                p[r] = ld4n<(LPR >= 32)>(I + ip[r] * D + 4 * sub);
                n[r] = ld4n<(LPR >= 32)>(I + in[r] * D + 4 * sub);
            }
        }
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const float Lu = group_sum<LPR>(dot4(u[r], u[r]));
            const float Lp = group_sum<LPR>(dot4(p[r], p[r]));
            const float Ln = group_sum<LPR>(dot4(n[r], n[r]));
            const float su = sqnorm_scale(Lu), sp = sqnorm_scale(Lp), sn = sqnorm_scale(Ln);
            const float4 yu = make_float4(u[r].x / su, u[r].y / su, u[r].z / su, u[r].w / su);
            const float4 dp = make_float4(yu.x - p[r].x / sp + e, yu.y - p[r].y / sp + e, yu.z - p[r].z / sp + e, yu.w - p[r].w / sp + e);
            const float4 dn = make_float4(yu.x - n[r].x / sn + e, yu.y - n[r].y / sn + e, yu.z - n[r].z / sn + e, yu.w - n[r].w / sn + e);
            const float d1 = sqrtf(group_sum<LPR>(dot4(dp, dp)));
            const float d2 = sqrtf(group_sum<LPR>(dot4(dn, dn)));
            bool on;
            const float hinge = triplet_hinge(d1, d2, margin, on);
            const float4 u1 = make_float4(unit_dir(on, dp.x, d1), unit_dir(on, dp.y, d1), unit_dir(on, dp.z, d1), unit_dir(on, dp.w, d1));
            const float4 u2 = make_float4(unit_dir(on, dn.x, d2), unit_dir(on, dn.y, d2), unit_dir(on, dn.z, d2), unit_dir(on, dn.w, d2));
            // (the three reductions run for every triple, open hinge or not: a lane group is a whole wave at LPR = 64)
            const float4 gu = sqnorm_bwd4<LPR>(u[r], scale_diff4(invB, u1, u2), Lu);
            const float4 gp = sqnorm_bwd4<LPR>(p[r], neg_scale4(invB, u1), Lp);
            const float4 gn = sqnorm_bwd4<LPR>(n[r], scale4(invB, u2), Ln);
            if (t < B) {
                if (live) {
                    st4n<(LPR >= 32)>(GU + t * D + 4 * sub, gu);
                    st4n<(LPR >= 32)>(GI + t * D + 4 * sub, gp);
                    st4n<(LPR >= 32)>(GI + (B + t) * D + 4 * sub, gn);
                }
                if (sub == 0) {
                    acc[0] += (double)hinge;
                    acc[1] += on ? 1.0 : 0.0;
                }
            }
        }
    }
    block_sum_d<2>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// out3 = {mean hinge loss, triples with an open hinge, 0}
__global__ __launch_bounds__(kBlock) void triplet_finish_kernel(const double* __restrict__ partials, int nblocks, int64_t B,
                                                                float* __restrict__ out3) {
    __shared__ double smem[2 * (kBlock / 64)];
    double acc[2] = {0.0, 0.0};
    sum_partials<2, kBlock>(partials, nblocks, acc, smem);
    if (threadIdx.x == 0) {
        out3[0] = (float)(acc[0] / (double)B);
        out3[1] = (float)acc[1];
        out3[2] = 0.f;
    }
}

// out9 = {total, main, ||U_b||, ||I_b||, c_u, c_i, sum loss, sum u^2, sum p^2} with c = reg_weight / (B * norm)
// (0 when the norm is 0).  B is the batch size the mean and the EmbLoss are taken over (the GLOBAL batch when the
// step is sharded: then out9[0..5] are provisional and cdr_loss_finish_sums recomputes them from all-reduced sums).
__global__ __launch_bounds__(kBlock) void step_finish_kernel(const double* __restrict__ partials, int nblocks, int64_t B,
                                                             float reg_weight, float* __restrict__ out6) {
    __shared__ double smem[3 * (kBlock / 64)];
    double acc[3] = {0.0, 0.0, 0.0};
    sum_partials<3, kBlock>(partials, nblocks, acc, smem);
    if (threadIdx.x == 0) {
        const float main_loss = (float)(acc[0] / (double)B);
        const float nu = (float)sqrt(acc[1]), ni = (float)sqrt(acc[2]);
        out6[1] = main_loss; out6[2] = nu; out6[3] = ni;
        out6[0] = main_loss + reg_weight * ((nu + ni) / (float)B);
        out6[4] = embloss_coef(reg_weight, B, nu);
        out6[5] = embloss_coef(reg_weight, B, ni);
        out6[6] = (float)acc[0]; out6[7] = (float)acc[1]; out6[8] = (float)acc[2];
    }
}

__global__ void finish_sums_kernel(const float* __restrict__ sums3, int64_t B, float reg_weight, float* __restrict__ out6) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float main_loss = sums3[0] / (float)B;
        const float nu = sqrtf(sums3[1]), ni = sqrtf(sums3[2]);
        out6[1] = main_loss; out6[2] = nu; out6[3] = ni;
        out6[0] = main_loss + reg_weight * ((nu + ni) / (float)B);
        out6[4] = embloss_coef(reg_weight, B, nu);
        out6[5] = embloss_coef(reg_weight, B, ni);
    }
}

// ------------------------------------------------------------------------------------------------ keys for the sort
// Every key-making kernel also clears, grid-stride, the `zwords` words at `zspan`: the zero-initialised state of the sort's own launch
// list ("the id sort's own launch list" below), which no launch of its own clears.  zspan = nullptr: the kernel only makes keys.
__device__ __forceinline__ void sort_state_clear(uint32_t* __restrict__ zspan, int64_t zwords) {
    if (!zspan) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < zwords; i += (int64_t)gridDim.x * blockDim.x) zspan[i] = 0u;
}

__global__ __launch_bounds__(kBlock) void make_keys_kernel(const int64_t* __restrict__ ids0, int64_t n0,
                                                           const int64_t* __restrict__ ids1, int64_t n1,
                                                           uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                           uint32_t* __restrict__ zspan, int64_t zwords) {
    sort_state_clear(zspan, zwords);
    const int64_t n = n0 + n1, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
        keys[e] = (uint32_t)(e < n0 ? ids0[e] : ids1[e - n0]);
        vals[e] = (uint32_t)e;
    }
}

// ------------------------------------------------------------------------------------------------ segmented apply
// OPT 0: SGD  w -= lr * grad            OPT 1: Adam on the touched rows (torch.optim.Adam arithmetic per element)
//
// Segments up to kLongSeg occurrences are summed by their head's lane group (the common case: a batch of 1-2 M ids over
// 10-50 M rows has segments of 1-5).  Skewed id streams (Zipf item popularity, SURVEY 8d synthetic inputs (ii)) put tens
// of thousands of occurrences into one segment; walking those with one lane group took 52 ms per step.  A head that
// sees a long segment therefore only registers it: the segment is cut into pieces of kPiece occurrences, every piece is
// summed by its own lane group (seg_piece_sum_kernel), and a finishing kernel adds the piece sums in piece order and
// applies the optimizer.  All three levels add in a fixed order: results stay bit-reproducible.
constexpr int kLongSeg = 32;
constexpr int kPiece = 256;

struct seg_long { int64_t head, len, base; };           // sorted position of the head, occurrences, first piece index
struct seg_piece { int64_t start; int64_t len; };

// dev (optional): {step_size, bc2_sqrt} in DEVICE memory, written earlier on the stream from device-resident update counts
// (coef_finish_kernel) -- the capturable form of the step: a hipGraph replay must not bake the update number into its launches.
struct apply_hp { float lr, b1, b2, eps, wd, step_size, bc2_sqrt; const float* dev; };
#define HP_FROM_DEV(h) do { if ((h).dev) { (h).step_size = (h).dev[0]; (h).bc2_sqrt = (h).dev[1]; } } while (0)

template <int LPR, int OPT>
__device__ __forceinline__ float4 apply_update(float* __restrict__ wp, float* __restrict__ mp, float* __restrict__ vp, float4 w,
                                               float4 acc, float rc, const apply_hp& h) {
    float4 gr = make_float4(acc.x + rc * w.x, acc.y + rc * w.y, acc.z + rc * w.z, acc.w + rc * w.w);
    float4 wn;
    if constexpr (OPT == 2) {                  // Adagrad: vp is the row's sum, mp is not read (cdr_opt_math.h: the dense sweep's function)
        float4 sm = ld4n<(LPR >= 32)>(vp);
        if (h.wd != 0.f) { gr.x += h.wd * w.x; gr.y += h.wd * w.y; gr.z += h.wd * w.z; gr.w += h.wd * w.w; }
        wn = make_float4(cdr_adagrad_elem(w.x, gr.x, sm.x, h.lr, h.eps, 0.f), cdr_adagrad_elem(w.y, gr.y, sm.y, h.lr, h.eps, 0.f),
                         cdr_adagrad_elem(w.z, gr.z, sm.z, h.lr, h.eps, 0.f), cdr_adagrad_elem(w.w, gr.w, sm.w, h.lr, h.eps, 0.f));
        st4n<(LPR >= 32)>(vp, sm);
    } else if (OPT == 0) {
        if (h.wd != 0.f) { gr.x += h.wd * w.x; gr.y += h.wd * w.y; gr.z += h.wd * w.z; gr.w += h.wd * w.w; }
        wn = make_float4(w.x - h.lr * gr.x, w.y - h.lr * gr.y, w.z - h.lr * gr.z, w.w - h.lr * gr.w);
    } else {
        float4 m = ld4n<(LPR >= 32)>(mp), v = ld4n<(LPR >= 32)>(vp);
        if (h.wd != 0.f) { gr.x += h.wd * w.x; gr.y += h.wd * w.y; gr.z += h.wd * w.z; gr.w += h.wd * w.w; }
        m.x += (gr.x - m.x) * (1.0f - h.b1); m.y += (gr.y - m.y) * (1.0f - h.b1);
        m.z += (gr.z - m.z) * (1.0f - h.b1); m.w += (gr.w - m.w) * (1.0f - h.b1);
        v.x = h.b2 * v.x + (1.0f - h.b2) * gr.x * gr.x; v.y = h.b2 * v.y + (1.0f - h.b2) * gr.y * gr.y;
        v.z = h.b2 * v.z + (1.0f - h.b2) * gr.z * gr.z; v.w = h.b2 * v.w + (1.0f - h.b2) * gr.w * gr.w;
        st4n<(LPR >= 32)>(mp, m); st4n<(LPR >= 32)>(vp, v);
        wn = make_float4(w.x - cdr_adam_term(m.x, v.x, h.step_size, h.bc2_sqrt, h.eps), w.y - cdr_adam_term(m.y, v.y, h.step_size, h.bc2_sqrt, h.eps),
                         w.z - cdr_adam_term(m.z, v.z, h.step_size, h.bc2_sqrt, h.eps), w.w - cdr_adam_term(m.w, v.w, h.step_size, h.bc2_sqrt, h.eps));
    }
    st4n<(LPR >= 32)>(wp, wn);
    return wn;
}

template <int LPR, int OPT, bool SIGNED>
__global__ __launch_bounds__(kBlock) void rowwise_apply_kernel(float* __restrict__ W, float* __restrict__ Mo,
                                                               float* __restrict__ Vo, int D,
                                                               const uint32_t* __restrict__ keys,
                                                               const uint32_t* __restrict__ perm, int64_t n,
                                                               const float* __restrict__ G, int64_t neg_start,
                                                               int64_t reg_limit, const float* __restrict__ reg_coef,
                                                               apply_hp hp, const int64_t* __restrict__ occ_ids,
                                                               unsigned* __restrict__ counters, seg_long* __restrict__ longs,
                                                               seg_piece* __restrict__ pieces) {
    HP_FROM_DEV(hp);
    constexpr int GPB = kBlock / LPR;
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int D4 = D >> 2;
    const float c = reg_coef ? reg_coef[0] : 0.f;
    for (int64_t q = gg; q < n; q += TG) {
        // three independent probes, issued together (prefetching them one iteration ahead was measured slower: the copies
        // of the prefetched registers at the loop's back edge wait for this iteration's row stores)
        const uint32_t row = keys[q];
        const uint32_t before = keys[q > 0 ? q - 1 : 0];
        const uint32_t far = keys[q + kLongSeg < n ? q + kLongSeg : n - 1];
        const bool head = !(q > 0 && before == row);         // uniform inside the lane group
        const bool is_long = q + kLongSeg < n && far == row;  // registered below, summed by the piece kernels
        if (head && !is_long) {
            for (int ch = sub; ch < D4; ch += LPR) {
                float* wp = W + (int64_t)row * D + 4 * ch;
                const float4 w = ld4n<(LPR >= 32)>(wp);
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                int cnt = 0;
                for (int64_t e = q; e < n && keys[e] == row; ++e) {
                    const int64_t o = perm[e];
                    const bool neg = SIGNED && o >= neg_start;
                    const float4 g = ld4n<(LPR >= 32)>(G + (neg ? o - neg_start : o) * D + 4 * ch);
                    if (neg) { acc.x -= g.x; acc.y -= g.y; acc.z -= g.z; acc.w -= g.w; }
                    else { acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w; }
                    cnt += occ_ids ? (int)((occ_ids[o] >> 62) & 1) : ((o < reg_limit) ? 1 : 0);
                }
                apply_update<LPR, OPT>(wp, OPT == 1 ? Mo + (int64_t)row * D + 4 * ch : nullptr, OPT ? Vo + (int64_t)row * D + 4 * ch : nullptr,
                                  w, acc, c * (float)cnt, hp);
            }
        }
    }
    // ---- registration of the long segments, one THREAD per sorted position.  Kept out of the loop above on purpose: with
    // the atomics inside it hipcc put an s_waitcnt vmcnt(0) on the loop's back edge (every iteration then waited for its
    // own row stores before issuing the next key loads: +25 % on the whole kernel).
    if (counters == nullptr) return;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q + kLongSeg < n; q += (int64_t)gridDim.x * kBlock) {
        const uint32_t row = keys[q];
        const uint32_t before = keys[q > 0 ? q - 1 : 0];
        const uint32_t far = keys[q + kLongSeg];
        if ((q > 0 && before == row) || far != row) continue;
        int64_t lo = q + kLongSeg, hi = n;                   // keys[lo] == row, keys[hi] != row (or hi == n): keys are sorted
        while (lo + 1 < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] == row) lo = mid; else hi = mid;
        }
        const int64_t len = hi - q;
        const unsigned np = (unsigned)((len + kPiece - 1) / kPiece);
        const unsigned base = atomicAdd(&counters[0], np);
        const unsigned li = atomicAdd(&counters[1], 1u);
        longs[li] = seg_long{q, len, (int64_t)base};
        for (unsigned k = 0; k < np; ++k) {
            const int64_t st = q + (int64_t)k * kPiece;
            pieces[base + k] = seg_piece{st, (hi - st) < kPiece ? (hi - st) : (int64_t)kPiece};
        }
    }
}

// One WORKGROUP per piece of a long segment (round 6; one lane group per piece before): the piece's kPiece = 256 occurrences are cut into
// eight sub-pieces of kSubPiece = 32; the workgroup's lane groups sum one sub-piece each in occurrence order (sixteen row loads in flight: two
// rounds), park the eight sub-sums in LDS, and the first lane group adds them in sub-piece order: partial[pi] = ((s0 + s1) + ...) + s7, a fixed
// association that does not depend on the launch shape.  This is north_star's "LDS staging of the hot rows" where it pays: a hot item's
// segment (4,068 occurrences at Zipf(1.05), B = 65,536) was 16 pieces of 16 dependent rounds each -- 44.8 us of the step's 300
// (profiles/r06_zipf65k_kernel_stats_before.csv); the staged sub-sums make it two rounds and one pass through LDS.  pcnt[pi] = the piece's
// EmbLoss occurrences.  Every long-segment path of this file (two-pass apply, fused duplicate apply, row-shard owner and requester) runs this
// body, so they keep agreeing bit for bit with each other.
constexpr int kSubPiece = 32, kSubs = kPiece / kSubPiece;
template <int LPR, bool SIGNED>
__device__ __forceinline__ void seg_piece_sum_body(int D, const uint32_t* __restrict__ perm,
                                                   const float* __restrict__ G, int64_t neg_start, int64_t reg_limit,
                                                   const int64_t* __restrict__ occ_ids,
                                                   const unsigned* __restrict__ counters,
                                                   const seg_piece* __restrict__ pieces, float* __restrict__ partial,
                                                   int* __restrict__ pcnt) {
    constexpr int GPB = kBlock / LPR;
    constexpr int UN = 16;
    __shared__ float4 sub_sum[kSubs][64];                     // one row of <= 256 floats per sub-piece (wider rows: chunk by chunk)
    __shared__ int sub_cnt[kSubs];
    const int sub = threadIdx.x % LPR, gid = threadIdx.x / LPR;
    const int D4 = D >> 2;
    const int64_t np = counters[0];
    for (int64_t pi = blockIdx.x; pi < np; pi += gridDim.x) {
        const seg_piece pc = pieces[pi];
        for (int ch0 = 0; ch0 < D4; ch0 += 64) {              // 64 float4 chunks of the row at a time (one trip for D <= 256)
            for (int sp = gid; sp < kSubs; sp += GPB) {
                const int64_t s0 = (int64_t)sp * kSubPiece, slen = pc.len - s0 < kSubPiece ? pc.len - s0 : (int64_t)kSubPiece;
                int cnt = 0;
                for (int ch = ch0 + sub; ch < D4 && ch < ch0 + 64; ch += LPR) {
                    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                    cnt = 0;
                    for (int64_t e0 = 0; e0 < slen; e0 += UN) {
                        int64_t o[UN]; float4 g[UN]; bool neg[UN];
#pragma unroll
                        for (int j = 0; j < UN; ++j) o[j] = (e0 + j < slen) ? (int64_t)perm[pc.start + s0 + e0 + j] : -1;
#pragma unroll
                        for (int j = 0; j < UN; ++j) {
                            neg[j] = SIGNED && o[j] >= neg_start;
                            g[j] = o[j] >= 0 ? ld4n<(LPR >= 32)>(G + (neg[j] ? o[j] - neg_start : o[j]) * D + 4 * ch) : make_float4(0.f, 0.f, 0.f, 0.f);
                        }
#pragma unroll
                        for (int j = 0; j < UN; ++j) {
                            if (o[j] < 0) continue;
                            if (neg[j]) { acc.x -= g[j].x; acc.y -= g[j].y; acc.z -= g[j].z; acc.w -= g[j].w; }
                            else { acc.x += g[j].x; acc.y += g[j].y; acc.z += g[j].z; acc.w += g[j].w; }
                            cnt += occ_ids ? (int)((occ_ids[o[j]] >> 62) & 1) : ((o[j] < reg_limit) ? 1 : 0);
                        }
                    }
                    sub_sum[sp][ch - ch0] = acc;
                }
                if (sub == 0 && ch0 == 0) sub_cnt[sp] = slen > 0 ? cnt : 0;
            }
            __syncthreads();
            const int nsub = (int)((pc.len + kSubPiece - 1) / kSubPiece);
            for (int c = threadIdx.x; c < 64 && ch0 + c < D4; c += kBlock) {        // sub-piece order: the piece's sum
                float4 acc = sub_sum[0][c];
                for (int sp = 1; sp < nsub; ++sp) { const float4 x = sub_sum[sp][c]; acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w; }
                st4n<(LPR >= 32)>(partial + pi * D + 4 * (ch0 + c), acc);
            }
            if (threadIdx.x == 0 && ch0 == 0) {
                int cn = 0;
                for (int sp = 0; sp < nsub; ++sp) cn += sub_cnt[sp];
                pcnt[pi] = cn;
            }
            __syncthreads();
        }
    }
}
template <int LPR, bool SIGNED>
__global__ __launch_bounds__(kBlock) void seg_piece_sum_kernel(int D, const uint32_t* __restrict__ perm,
                                                               const float* __restrict__ G, int64_t neg_start, int64_t reg_limit,
                                                               const int64_t* __restrict__ occ_ids,
                                                               const unsigned* __restrict__ counters,
                                                               const seg_piece* __restrict__ pieces, float* __restrict__ partial,
                                                               int* __restrict__ pcnt) {
    seg_piece_sum_body<LPR, SIGNED>(D, perm, G, neg_start, reg_limit, occ_ids, counters, pieces, partial, pcnt);
}

// One lane group per long segment: piece sums added in piece order, then the same update as the head-only path.
// NC (whole rows per lane group only, D <= 4 LPR): the updated row's squared-norm record goes to n2 (the fused BPR step's norm cache).
template <int LPR, int OPT, bool NC = false>
__device__ __forceinline__ void seg_long_finish_body(float* __restrict__ W, float* __restrict__ Mo, float* __restrict__ Vo,
                                                     int D, const uint32_t* __restrict__ keys,
                                                     const float* __restrict__ reg_coef, apply_hp hp,
                                                     const unsigned* __restrict__ counters,
                                                     const seg_long* __restrict__ longs,
                                                     const float* __restrict__ partial, const int* __restrict__ pcnt,
                                                     float* __restrict__ n2 = nullptr) {
    HP_FROM_DEV(hp);
    constexpr int GPB = kBlock / LPR;
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int D4 = D >> 2;
    const float c = reg_coef ? reg_coef[0] : 0.f;
    const int64_t nl = counters[1];
    for (int64_t li = gg; li < nl; li += TG) {
        const seg_long sg = longs[li];
        const uint32_t row = keys[sg.head];
        const int64_t np = (sg.len + kPiece - 1) / kPiece;
        float4 wnew = make_float4(0.f, 0.f, 0.f, 0.f);               // (NC: this lane's chunk of the updated row; a dead lane keeps 0)
        for (int ch = sub; ch < D4; ch += LPR) {
            float* wp = W + (int64_t)row * D + 4 * ch;
            const float4 w = ld4n<(LPR >= 32)>(wp);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int cnt = 0;
            for (int64_t k0 = 0; k0 < np; k0 += 8) {                  // eight piece sums in flight, added in piece order
                float4 g[8]; int c[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool in = k0 + j < np;
                    g[j] = in ? ld4n<(LPR >= 32)>(partial + (sg.base + k0 + j) * D + 4 * ch) : make_float4(0.f, 0.f, 0.f, 0.f);
                    c[j] = in ? pcnt[sg.base + k0 + j] : 0;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (k0 + j < np) { acc.x += g[j].x; acc.y += g[j].y; acc.z += g[j].z; acc.w += g[j].w; cnt += c[j]; }
                }
            }
            wnew = apply_update<LPR, OPT>(wp, OPT == 1 ? Mo + (int64_t)row * D + 4 * ch : nullptr, OPT ? Vo + (int64_t)row * D + 4 * ch : nullptr,
                                          w, acc, c * (float)cnt, hp);
        }
        if (NC) norm_rec_store<LPR>(n2 + (int64_t)row * kNormRecFloats, group_sum<LPR>(sqnorm4<LPR>(wnew)), sub);
    }
}
template <int LPR, int OPT>
__global__ __launch_bounds__(kBlock) void seg_long_finish_kernel(float* __restrict__ W, float* __restrict__ Mo, float* __restrict__ Vo,
                                                                 int D, const uint32_t* __restrict__ keys,
                                                                 const float* __restrict__ reg_coef, apply_hp hp,
                                                                 const unsigned* __restrict__ counters,
                                                                 const seg_long* __restrict__ longs,
                                                                 const float* __restrict__ partial, const int* __restrict__ pcnt) {
    seg_long_finish_body<LPR, OPT>(W, Mo, Vo, D, keys, reg_coef, hp, counters, longs, partial, pcnt);
}

// Two tables in ONE sort: rocPRIM's radix sort costs ~0.16 ms whether it sorts 1 M or 3 M pairs (a chain of small launches),
// so the user ids and the item ids of a step are sorted together; the item keys carry one extra high bit (key_base), which
// puts them behind every user key and is subtracted again by the apply kernel.
__global__ __launch_bounds__(kBlock) void make_keys2_kernel(const int64_t* __restrict__ a, int64_t na, const int64_t* __restrict__ b0,
                                                            int64_t nb0, const int64_t* __restrict__ b1, int64_t nb1, uint32_t key_base,
                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                            uint32_t* __restrict__ zspan, int64_t zwords) {
    sort_state_clear(zspan, zwords);
    const int64_t n = na + nb0 + nb1, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
        if (e < na) { keys[e] = (uint32_t)a[e]; vals[e] = (uint32_t)e; }
        else {
            const int64_t o = e - na;
            keys[e] = key_base + (uint32_t)(o < nb0 ? b0[o] : b1[o - nb0]);
            vals[e] = (uint32_t)o;                               // occurrence index inside table b's own list
        }
    }
}

// The big sort's shape (big_sort_config below): 1,024-thread blocks of 8 items, 9-bit digits, so 512 bins per digit place.
constexpr unsigned kSortBlock = 1024, kSortItems = 8, kSortRadixBits = 9, kSortRadix = 1u << kSortRadixBits;
constexpr unsigned kSortMaxPlaces = (32 + kSortRadixBits - 1) / kSortRadixBits;
using sort_offs_t = size_t;                     // rocPRIM's offset type for a size_t item count, the one the library call instantiates

// make_keys2_kernel, the digit histogram and its scan in ONE launch (the fused BPR step's sorted path): every key's digits are counted
// in LDS as the key is made ([place][digit][4 stripes], rocPRIM's layout against same-address conflicts), a block adds its non-zero
// bins to counts[place][512] with global atomics -- integer counts, the order does not matter -- and the block that signs in last
// (cdr_sign_in_last: the atomics are acknowledged by memory before the ticket is taken, the finisher reads past its L2) turns every
// place's counts into exclusive offsets, what rocPRIM's histogram and scan launches leave for its Onesweep passes.
// counts and ticket must be zero at the start (the caller's earlier launch: coef_finish_kernel); zspan is cleared as in every key kernel.
__global__ __launch_bounds__(kSortBlock) void make_keys2_offsets_kernel(const int64_t* __restrict__ a, int64_t na, const int64_t* __restrict__ b0,
                                                                        int64_t nb0, const int64_t* __restrict__ b1, int64_t nb1,
                                                                        uint32_t key_base, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                        uint32_t* __restrict__ zspan, int64_t zwords,
                                                                        sort_offs_t* __restrict__ counts, unsigned* __restrict__ ticket, unsigned places) {
    constexpr unsigned kStripes = 4;
    __shared__ unsigned hist[kSortMaxPlaces * kSortRadix * kStripes];
    sort_state_clear(zspan, zwords);
    const unsigned tid = threadIdx.x, bins = places * kSortRadix;
    for (unsigned i = tid; i < bins * kStripes; i += kSortBlock) hist[i] = 0u;
    __syncthreads();
    const unsigned stripe = tid % kStripes;
    const int64_t n = na + nb0 + nb1, stride = (int64_t)gridDim.x * kSortBlock;
    for (int64_t e = (int64_t)blockIdx.x * kSortBlock + tid; e < n; e += stride) {
        uint32_t k, v;
        if (e < na) { k = (uint32_t)a[e]; v = (uint32_t)e; }
        else {
            const int64_t o = e - na;
            k = key_base + (uint32_t)(o < nb0 ? b0[o] : b1[o - nb0]);
            v = (uint32_t)o;
        }
        keys[e] = k; vals[e] = v;
        for (unsigned p = 0; p < places; ++p) {
            const unsigned digit = (k >> (p * kSortRadixBits)) & (kSortRadix - 1u);
            atomicAdd(&hist[(p * kSortRadix + digit) * kStripes + stripe], 1u);
        }
    }
    __syncthreads();
    for (unsigned i = tid; i < bins; i += kSortBlock) {
        unsigned t = 0;
#pragma unroll
        for (unsigned j = 0; j < kStripes; ++j) t += hist[i * kStripes + j];
        if (t) atomicAdd(reinterpret_cast<unsigned long long*>(counts + i), (unsigned long long)t);
    }
    if (!cdr_sign_in_last(ticket, gridDim.x)) return;
    unsigned* sc = hist;                                         // (every thread is past its reads of hist: cdr_sign_in_last's barriers)
    for (unsigned p = 0; p < places; ++p) {
        unsigned c = 0;
        if (tid < kSortRadix) {
            c = (unsigned)__hip_atomic_load(reinterpret_cast<unsigned long long*>(counts + p * kSortRadix + tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sc[tid] = c;
        }
        __syncthreads();
        for (unsigned d = 1; d < kSortRadix; d <<= 1) {          // inclusive scan of the 512 counts
            const unsigned t = (tid < kSortRadix && tid >= d) ? sc[tid - d] : 0u;
            __syncthreads();
            if (tid < kSortRadix) sc[tid] += t;
            __syncthreads();
        }
        if (tid < kSortRadix) counts[p * kSortRadix + tid] = (sort_offs_t)(sc[tid] - c);
        __syncthreads();
    }
}


// ================================================================================================ single-occurrence rows in the forward
// Round 3.  At C5 a batch of 1 M triples names ~0.98 M users that occur ONCE and ~1.6 M of its 2 M item occurrences are the only
// occurrence of their row.  For such a row the "segment sum" is one gradient row that the forward kernel has in registers, so the
// forward kernel applies the optimizer itself: it reads the row's two moments next to the row, writes all three back, and the
// compact gradient row (GU[b] / GP[b]) is neither written nor read again, nor is the row re-read by an apply kernel:
//
//   cdr_sort_ids_two_tables   as before, but FIRST (it needs only the ids)
//   occ_flags_kernel          one pass over the sorted keys: flags[occurrence] = "only occurrence of its row" and the heads of the
//                             remaining (duplicate) segments compacted into two lists
//   batch_norms_kernel        the EmbLoss norms ||U[uid]||, ||I[pid]|| of the batch (its gradient coefficient is a global scalar the
//                             optimizer needs BEFORE the first row is updated): a gather of 2 rows per triple.  (First version: a
//                             per-row squared-norm cache kept current by every writer -- its 2.6 M scattered 4-byte stores per
//                             step, partial-line read-modify-writes at the HBM, cost 0.35 ms per domain step against 0.18 ms for
//                             this gather, measured A/B.  The cache came back with 64-byte records written whole: "EmbLoss norms
//                             from a per-row cache" below; this gather remains the path of every step that cannot use it.)
//   bpr_fwd_apply_kernel      gather 3 rows (+ 2 moments per single row) -> loss -> single rows: optimizer in place;
//                             duplicate rows: GU[b] / GP[b] as before
//   rowwise_apply_dups_kernel the segmented apply over the duplicate segments only (same sums, same order as rowwise_apply_kernel)
//
// Same arithmetic per row as cdr_bpr_fwd_grad + cdr_rowwise_apply (one occurrence: 0 + g, then the same update), fixed order
// everywhere: bit-reproducible.  Bytes per triple at D = 128, uniform ids: ~9.5 KB against 12.9 KB before (SURVEY 8d floor 9.2 KB).
struct tab_ptrs { float* W; float* M; float* V; };

template <int OPT>
__device__ __forceinline__ float4 upd_math(float4 w, float4& m, float4& v, float4 acc, float rc, const apply_hp& h) {
    float4 gr = make_float4(acc.x + rc * w.x, acc.y + rc * w.y, acc.z + rc * w.z, acc.w + rc * w.w);
    if (h.wd != 0.f) { gr.x += h.wd * w.x; gr.y += h.wd * w.y; gr.z += h.wd * w.z; gr.w += h.wd * w.w; }
    if (OPT == 0) return make_float4(w.x - h.lr * gr.x, w.y - h.lr * gr.y, w.z - h.lr * gr.z, w.w - h.lr * gr.w);
    if constexpr (OPT == 2)                    // Adagrad: v is the row's sum, m is not touched (cdr_opt_math.h: the dense sweep's function)
        return make_float4(cdr_adagrad_elem(w.x, gr.x, v.x, h.lr, h.eps, 0.f), cdr_adagrad_elem(w.y, gr.y, v.y, h.lr, h.eps, 0.f),
                           cdr_adagrad_elem(w.z, gr.z, v.z, h.lr, h.eps, 0.f), cdr_adagrad_elem(w.w, gr.w, v.w, h.lr, h.eps, 0.f));
    m.x += (gr.x - m.x) * (1.0f - h.b1); m.y += (gr.y - m.y) * (1.0f - h.b1);
    m.z += (gr.z - m.z) * (1.0f - h.b1); m.w += (gr.w - m.w) * (1.0f - h.b1);
    v.x = h.b2 * v.x + (1.0f - h.b2) * gr.x * gr.x; v.y = h.b2 * v.y + (1.0f - h.b2) * gr.y * gr.y;
    v.z = h.b2 * v.z + (1.0f - h.b2) * gr.z * gr.z; v.w = h.b2 * v.w + (1.0f - h.b2) * gr.w * gr.w;
    return make_float4(w.x - cdr_adam_term(m.x, v.x, h.step_size, h.bc2_sqrt, h.eps), w.y - cdr_adam_term(m.y, v.y, h.step_size, h.bc2_sqrt, h.eps),
                       w.z - cdr_adam_term(m.z, v.z, h.step_size, h.bc2_sqrt, h.eps), w.w - cdr_adam_term(m.w, v.w, h.step_size, h.bc2_sqrt, h.eps));
}

// A lane's chunk, at float offset `off`, of a row of table T.  row_moments: the two Adam moments (SGD: nothing is read, m and v keep what
// they hold); the caller's `if` says for which rows.  row_store: moments and weights back in place.  `if constexpr` and references to m
// and v, so that an SGD kernel's code never names them: passed by value they cost the k-major SGD kernels registers and split their
// 16-byte stores.  The step around them stays written out in the kernels -- `if (single) { upd_math; row_store } else spill the gradient
// row`: as one function it changed the code of every kernel that used it (tools/kernel_diff.py).
template <int LPR, int OPT>
__device__ __forceinline__ void row_moments(const tab_ptrs& T, int64_t off, float4& m, float4& v) {
    if constexpr (OPT == 1) { m = ld4n<(LPR >= 32)>(T.M + off); v = ld4n<(LPR >= 32)>(T.V + off); }
    if constexpr (OPT == 2) v = ld4n<(LPR >= 32)>(T.V + off);          // Adagrad: the sum alone (T.M is NULL)
}
template <int LPR, int OPT>
__device__ __forceinline__ void row_store(const tab_ptrs& T, int64_t off, float4 w, const float4& m, const float4& v) {
    if constexpr (OPT == 1) { st4n<(LPR >= 32)>(T.M + off, m); st4n<(LPR >= 32)>(T.V + off, v); }
    if constexpr (OPT == 2) st4n<(LPR >= 32)>(T.V + off, v);
    st4n<(LPR >= 32)>(T.W + off, w);
}

// partials[block] = {sum_b ||U[uid[b]]||^2, sum_b ||I[pid[b]]||^2}: the EmbLoss norms of the batch (emcdr.py:129-131: reg_loss(user_e, pos_e))
template <int LPR>
__global__ __launch_bounds__(kBlock) void batch_norms_kernel(const float* __restrict__ U, const float* __restrict__ I, int D,
                                                             const int64_t* __restrict__ uid, const int64_t* __restrict__ pid, int64_t B,
                                                             double* __restrict__ partials) {
    constexpr int GPB = kBlock / LPR;
    constexpr int UNR = 8;
    __shared__ double smem[2 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const bool live = sub < (D >> 2);
    double acc[2] = {0.0, 0.0};
    for (int64_t base = gg; base < B; base += TG * UNR) {
        int64_t iu[UNR], ip[UNR];
        float4 u[UNR], p[UNR];
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const int64_t tc = t < B ? t : B - 1;
            iu[r] = uid[tc]; ip[r] = pid[tc];
        }
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            u[r] = p[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < B && live) { u[r] = ld4n<(LPR >= 32)>(U + iu[r] * D + 4 * sub); p[r] = ld4n<(LPR >= 32)>(I + ip[r] * D + 4 * sub); }
        }
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const float su = group_sum<LPR>(dot4(u[r], u[r])), sp = group_sum<LPR>(dot4(p[r], p[r]));
            if (sub == 0) { acc[0] += (double)su; acc[1] += (double)sp; }
        }
    }
    block_sum_d<2>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// ------------------------------------------------------------------------------------------------ EmbLoss norms from a per-row cache
// batch_norms_kernel re-gathers two whole rows per triple (1.09 GB per domain step at C5) for two scalars.  The cache keeps the scalar:
// NU / NI [rows, kNormRecFloats], slot 0 = ||W[r]||^2 formed as batch_norms_kernel forms it -- group_sum<LPR>(dot4(w, w)) over the same
// lanes -- by cdr_row_norms_build and, for every row the sorted path of cdr_bpr_step_fused updates, by the kernel that has the new row
// in registers (bpr_fwd_apply_kernel<.., NC>, rowwise_apply_dups2_kernel<.., NC>, seg_long_finish2_kernel<.., NC>).
//
// The reader below keeps batch_norms_kernel's grid, unroll, triple -> lane group assignment and accumulation order: the same floats enter
// the same fp64 sums in the same order, so the partials -- and the coefficient coef_finish_kernel makes of them -- are bit-equal to the
// gather's.  (Which is why it is a launch of its own and not part of make_keys2_kernel: another summation order may move the last bit.)
template <int LPR>
__global__ __launch_bounds__(kBlock) void batch_norms_cached_kernel(const float* __restrict__ NU, const float* __restrict__ NI,
                                                                    const int64_t* __restrict__ uid, const int64_t* __restrict__ pid, int64_t B,
                                                                    double* __restrict__ partials) {
    constexpr int GPB = kBlock / LPR;
    constexpr int UNR = 8;
    __shared__ double smem[2 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    double acc[2] = {0.0, 0.0};
    for (int64_t base = gg; base < B; base += TG * UNR) {
        int64_t iu[UNR], ip[UNR];
        float su[UNR], sp[UNR];
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const int64_t tc = t < B ? t : B - 1;
            iu[r] = uid[tc]; ip[r] = pid[tc];
        }
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            su[r] = sp[r] = 0.f;
            if (t < B && sub == 0) { su[r] = NU[iu[r] * kNormRecFloats]; sp[r] = NI[ip[r] * kNormRecFloats]; }
        }
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            if (sub == 0) { acc[0] += (double)su[r]; acc[1] += (double)sp[r]; }
        }
    }
    block_sum_d<2>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// The records of a whole table in one streaming pass: one lane group per row, four rows in flight.
template <int LPR>
__global__ __launch_bounds__(kBlock) void row_norms_build_kernel(const float* __restrict__ W, int64_t rows, int D, float* __restrict__ n2) {
    constexpr int GPB = kBlock / LPR;
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const bool live = sub < (D >> 2);
    for (int64_t base = gg; base < rows; base += TG * kUnroll) {
        float4 w[kUnroll];
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const int64_t row = base + (int64_t)r * TG;
            w[r] = (row < rows && live) ? ld4n<(LPR >= 32)>(W + row * D + 4 * sub) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const int64_t row = base + (int64_t)r * TG;
            const float s = group_sum<LPR>(sqnorm4<LPR>(w[r]));
            if (row < rows) norm_rec_store<LPR>(n2 + row * kNormRecFloats, s, sub);
        }
    }
}

// keys / perm: the two-table sort's output (section A = positions [0, nA): user keys; section B = [nA, n): item keys + key_base).
// flags: fstride bytes per positive j = {its user occurrence (A occurrence j), its positive (B occurrence j), its negatives (B
// occurrence nA + j + m nA for m = 0 .. k - 1: recbole's k-major layout), padding}; the per-triple step is the case k = 1 of it
// (fstride = 4: one 32-bit load per triple in the forward kernel).  cnt[0] / cnt[1]: lengths of headsA / headsB (sorted
// positions, relative to their section, of the first occurrence of every row that occurs more than once; list order is
// irrelevant -- every segment is summed in occurrence order by whoever takes it).
// A thread takes kFlagIT consecutive positions and a block reserves its share of each list with ONE atomic: with an atomic per
// 256 positions the 24 k same-address atomics of a 3 M-position launch were most of its 0.157 ms.
constexpr int kFlagIT = 8;
__global__ __launch_bounds__(kBlock) void occ_flags_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                           int64_t nA, int64_t n, int fstride, uint8_t* __restrict__ flags,
                                                           uint32_t* __restrict__ headsA, uint32_t* __restrict__ headsB,
                                                           unsigned* __restrict__ cnt, bool stat = false) {
    constexpr int NW = kBlock / 64;
    __shared__ unsigned wcnt[3][NW], wbase[2][NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t base = (int64_t)blockIdx.x * kBlock * kFlagIT; base < n; base += (int64_t)gridDim.x * kBlock * kFlagIT) {
        const int64_t q0 = base + (int64_t)threadIdx.x * kFlagIT;
        uint32_t k[kFlagIT + 2], o[kFlagIT];
#pragma unroll
        for (int j = 0; j < kFlagIT + 2; ++j) {
            const int64_t q = q0 - 1 + j;
            k[j] = (q >= 0 && q < n) ? keys[q] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kFlagIT; ++j) o[j] = q0 + j < n ? perm[q0 + j] : 0u;
        unsigned hA = 0, hB = 0, nd = 0;                   // bit j: position q0 + j heads a duplicate segment; nd: positions that are not alone
#pragma unroll
        for (int j = 0; j < kFlagIT; ++j) {
            const int64_t q = q0 + j;
            if (q < n) {
                const uint32_t row = k[j + 1];
                const bool first = q == 0 || k[j] != row, last = q + 1 >= n || k[j + 2] != row;
                nd += (first && last) ? 0u : 1u;
                if (q < nA) {
                    flags[(int64_t)fstride * o[j]] = (uint8_t)(first && last);
                    hA |= (unsigned)(first && !last) << j;
                } else {
                    const int64_t ob = o[j];
                    int64_t fi;
                    if (ob < nA) fi = fstride * ob + 1;
                    else { const int64_t r_ = ob - nA, m_ = r_ / nA; fi = fstride * (r_ - m_ * nA) + 2 + m_; }
                    flags[fi] = (uint8_t)(first && last);
                    hB |= (unsigned)(first && !last) << j;
                }
            }
        }
        // exclusive prefix of the per-thread head counts: inside the wave by shuffles, across waves through LDS, one atomic per list
        unsigned cA = (unsigned)__popc(hA), cB = (unsigned)__popc(hB), pA = cA, pB = cB;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned a = __shfl_up(pA, d, 64), b = __shfl_up(pB, d, 64);
            if (lane >= d) { pA += a; pB += b; }
        }
        if (stat) {                                            // (medium batches only: the statistic that picks their id path)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) nd += __shfl_xor(nd, d, 64);
        }
        if (lane == 63) { wcnt[0][wave] = pA; wcnt[1][wave] = pB; wcnt[2][wave] = nd; }
        __syncthreads();
        if (stat && threadIdx.x == 2) {                        // cnt[2] += duplicate occurrences: the host binding's statistic (which id path serves this stream)
            unsigned tot = 0;
            for (int w = 0; w < NW; ++w) tot += wcnt[2][w];
            if (tot) atomicAdd(&cnt[2], tot);
        }
        if (threadIdx.x < 2) {
            const int t = threadIdx.x;
            unsigned tot = 0;
            for (int w = 0; w < NW; ++w) { wbase[t][w] = tot; tot += wcnt[t][w]; }
            const unsigned b = tot ? atomicAdd(&cnt[t], tot) : 0u;
            for (int w = 0; w < NW; ++w) wbase[t][w] += b;
        }
        __syncthreads();
        unsigned sA = wbase[0][wave] + pA - cA, sB = wbase[1][wave] + pB - cB;
#pragma unroll
        for (int j = 0; j < kFlagIT; ++j) {
            if ((hA >> j) & 1u) headsA[sA++] = (uint32_t)(q0 + j);
            if ((hB >> j) & 1u) headsB[sB++] = (uint32_t)(q0 + j - nA);
        }
        __syncthreads();
    }
}

// out9[4], out9[5] = reg_weight / (B * ||rows||) from batch_norms_kernel's partial sums (0 when there is no EmbLoss or the norm is 0)
// (k-major batches: the partials are sums over the S positives, every one of which stands for k rows of the batch -- the norm is taken
// over B = S k rows and the coefficient is handed out pre-multiplied by k, per S-list occurrence)
// step_dev (optional; the capturable step): {user table's, item table's} update counts in device memory -- advanced here, and the Adam
// scalars of the new counts left in hp_dev[0..3] = {step_size_u, bc2_sqrt_u, step_size_i, bc2_sqrt_i} for the kernels behind (apply_hp::dev)
// norms2 (optional): {sum ||u||^2, sum ||p||^2} GIVEN (all-reduced over ranks) instead of summed from `partials`
__global__ __launch_bounds__(kBlock) void coef_finish_kernel(const double* __restrict__ partials, int nblocks, int64_t B,
                                                             float reg_weight, float* __restrict__ out9, int kmul = 1,
                                                             int64_t* __restrict__ step_u_dev = nullptr, int64_t* __restrict__ step_i_dev = nullptr,
                                                             float* __restrict__ hp_dev = nullptr, float lr = 0.f, float b1 = 0.f, float b2 = 0.f,
                                                             unsigned* __restrict__ zero4 = nullptr, const float* __restrict__ norms2 = nullptr,
                                                             uint32_t* __restrict__ zspan = nullptr, int zwords = 0) {
    __shared__ double smem[2 * (kBlock / 64)];
    if (zero4 && threadIdx.x >= 64 && threadIdx.x < 68) zero4[threadIdx.x - 64] = 0u;       // the head lists' counters (occ_flags_kernel): no launch of their own
    if (zspan) {                                 // the id sort's digit counts and ticket (make_keys2_offsets_kernel, the next launch)
        for (int i = threadIdx.x; i < zwords; i += kBlock) zspan[i] = 0u;
    }
    if (hp_dev && threadIdx.x < 2) {
        int64_t* c = threadIdx.x == 0 ? step_u_dev : step_i_dev;
        const int64_t st = c[0] + 1;
        c[0] = st;
        cdr_adam_hp((double)st, lr, b1, b2, hp_dev[2 * threadIdx.x], hp_dev[2 * threadIdx.x + 1]);
    }
    double acc[2] = {0.0, 0.0};
    sum_partials<2, kBlock>(partials, nblocks, acc, smem);
    if (threadIdx.x == 0) {
        if (norms2) { acc[0] = (double)norms2[0]; acc[1] = (double)norms2[1]; }
        const float nu = (float)sqrt((double)kmul * acc[0]), ni = (float)sqrt((double)kmul * acc[1]);
        // embloss_coef (cdr_loss_math.h) with k = kmul, in place: the helper changed this kernel's code
        out9[4] = (reg_weight != 0.f && nu > 0.f) ? (float)kmul * (reg_weight / ((float)B * nu)) : 0.f;
        out9[5] = (reg_weight != 0.f && ni > 0.f) ? (float)kmul * (reg_weight / ((float)B * ni)) : 0.f;
    }
}

// loss scalars of the fused step: as step_finish_kernel, but out9[4..5] (the EmbLoss coefficients the kernels used) stay
__global__ __launch_bounds__(kBlock) void step_finish_keep_kernel(const double* __restrict__ partials, int nblocks, int64_t B,
                                                                  float reg_weight, float* __restrict__ out9,
                                                                  unsigned* __restrict__ zero_a = nullptr, unsigned* __restrict__ zero_b = nullptr,
                                                                  const float* __restrict__ norms2 = nullptr) {
    __shared__ double smem[3 * (kBlock / 64)];
    // the long-segment counters of the two duplicate-row applies behind this launch (apply_dups_pair): no launches of their own
    if (zero_a && threadIdx.x >= 64 && threadIdx.x < 68) zero_a[threadIdx.x - 64] = 0u;
    if (zero_b && threadIdx.x >= 128 && threadIdx.x < 132) zero_b[threadIdx.x - 128] = 0u;
    double acc[3] = {0.0, 0.0, 0.0};
    sum_partials<3, kBlock>(partials, nblocks, acc, smem);
    if (threadIdx.x == 0) {
        if (norms2) { acc[1] = (double)norms2[0]; acc[2] = (double)norms2[1]; }
        const float main_loss = (float)(acc[0] / (double)B);
        const float nu = (float)sqrt(acc[1]), ni = (float)sqrt(acc[2]);
        out9[1] = main_loss; out9[2] = nu; out9[3] = ni;
        out9[0] = main_loss + reg_weight * ((nu + ni) / (float)B);
        out9[6] = (float)acc[0]; out9[7] = (float)acc[1]; out9[8] = (float)acc[2];
    }
}

// {0, sum u^2, sum p^2} of batch_norms_kernel's partials as three floats (the row shard all-reduces them before the update)
__global__ __launch_bounds__(kBlock) void norm_sums_kernel(const double* __restrict__ partials, int nblocks, float* __restrict__ sums3) {
    __shared__ double smem[2 * (kBlock / 64)];
    double acc[2] = {0.0, 0.0};
    sum_partials<2, kBlock>(partials, nblocks, acc, smem);
    if (threadIdx.x == 0) { sums3[0] = 0.f; sums3[1] = (float)acc[0]; sums3[2] = (float)acc[1]; }
}

// out9[6..8] = this rank's {loss sum, sum u^2, sum p^2} from the forward's partials; nothing else of out9 moves (row shard: the caller
// all-reduces the three and finishes the loss with cdr_loss_finish_sums)
__global__ __launch_bounds__(kBlock) void shard_sums_kernel(const double* __restrict__ partials, int nblocks, float* __restrict__ out9,
                                                            unsigned* __restrict__ zero_a) {
    __shared__ double smem[3 * (kBlock / 64)];
    if (zero_a && threadIdx.x >= 64 && threadIdx.x < 68) zero_a[threadIdx.x - 64] = 0u;
    double acc[3] = {0.0, 0.0, 0.0};
    sum_partials<3, kBlock>(partials, nblocks, acc, smem);
    if (threadIdx.x == 0) { out9[6] = (float)acc[0]; out9[7] = (float)acc[1]; out9[8] = (float)acc[2]; }
}

// XD (round 5, the dimension-sharded step): the triple's score x_t = <u,p> - <u,n> is GIVEN (xdiff[t]: the all-reduced sum of every
// rank's column-slice partials, cdr_dimshard.hip) instead of being formed from the rows held here; the norm partials are not produced.
// SH (round 6, the row-sharded step): the item "table" TI.W is the buffer of RECEIVED rows (one per distinct item this rank asked for,
// read-only) and an item occurrence flagged "only occurrence of its row" is not updated -- its finished gradient row (g u + c_i p for the
// positive, -g u for the negative) is written straight into the send slot of its row, GS[ip] / GS[in]; GP[t] = g u only when one of the
// triple's two item rows is a duplicate (the segmented sum over the duplicates reads it).
// NC (the plain step with a norm cache): the squared norm of every row updated here goes to its record in NU / NI, written whole.
template <int LPR, int OPT, int UN, bool XD = false, bool SH = false, bool NC = false>
__global__ __launch_bounds__(kBlock) void bpr_fwd_apply_kernel(tab_ptrs TU, tab_ptrs TI, int D, const int64_t* __restrict__ uid,
                                                               const int64_t* __restrict__ pid, const int64_t* __restrict__ nid,
                                                               const uint32_t* __restrict__ flags4, int64_t B, float gamma, float invB,
                                                               const float* __restrict__ coef, apply_hp hu, apply_hp hi,
                                                               float* __restrict__ GU, float* __restrict__ GP,
                                                               double* __restrict__ partials, const float* __restrict__ xdiff = nullptr,
                                                               float* __restrict__ GS = nullptr, float* __restrict__ NU = nullptr,
                                                               float* __restrict__ NI = nullptr) {
    static_assert(!NC || (!XD && !SH), "the norm cache belongs to the plain step");
    HP_FROM_DEV(hu); HP_FROM_DEV(hi);
    constexpr int GPB = kBlock / LPR;
    __shared__ double smem[3 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int D4 = D >> 2;
    const bool live = sub < D4;
    const float cu = coef[0], ci = coef[1];
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    double acc[3] = {0.0, 0.0, 0.0};

    // The ids + flags of the NEXT iteration are requested right behind this iteration's row loads and are waited for together
    // with them, BEFORE this iteration's stores are issued: vmcnt retires in order, so a wait for anything requested after the
    // stores also waits for every store's acknowledgement (the first version of this loop had s_waitcnt vmcnt(0) at its head).
    uint32_t iu[UN], ip[UN], in[UN], fl[UN];
    float xd[UN];
#pragma unroll
    for (int r = 0; r < UN; ++r) {
        const int64_t t = gg + (int64_t)r * TG;
        const int64_t tc = t < B ? t : B - 1;
        iu[r] = (uint32_t)uid[tc]; ip[r] = (uint32_t)pid[tc]; in[r] = (uint32_t)nid[tc];
        fl[r] = flags4[tc];
        xd[r] = XD ? xdiff[tc] : 0.f;
    }
    // (waited for HERE: a wait that the loop header inherits from this prologue is a static s_waitcnt vmcnt(0) on every iteration)
#pragma unroll
    for (int r = 0; r < UN; ++r) asm volatile("" : "+v"(iu[r]), "+v"(ip[r]), "+v"(in[r]), "+v"(fl[r]), "+v"(xd[r]));
    for (int64_t base = gg; base < B; base += TG * UN) {
        float4 u[UN], p[UN], n[UN], um[UN], uv[UN], pm[UN], pv[UN], nm[UN], nv[UN];
        int64_t ou[UN], op[UN], on[UN];
        bool fu[UN], fp[UN], fn[UN];
#pragma unroll
        for (int r = 0; r < UN; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const bool ok = t < B && live;
            fu[r] = (fl[r] & 0xFFu) != 0 && t < B; fp[r] = (fl[r] & 0xFF00u) != 0 && t < B; fn[r] = (fl[r] & 0xFF0000u) != 0 && t < B;
            ou[r] = (int64_t)iu[r] * D + 4 * sub; op[r] = (int64_t)ip[r] * D + 4 * sub; on[r] = (int64_t)in[r] * D + 4 * sub;
            u[r] = ok ? ld4n<(LPR >= 32)>(TU.W + ou[r]) : z4;
            p[r] = ok ? ld4n<(LPR >= 32)>(TI.W + op[r]) : z4;
            n[r] = ok ? ld4n<(LPR >= 32)>(TI.W + on[r]) : z4;
            um[r] = uv[r] = pm[r] = pv[r] = nm[r] = nv[r] = z4;
            if (ok && fu[r]) row_moments<LPR, OPT>(TU, ou[r], um[r], uv[r]);
            if (!SH && ok && fp[r]) row_moments<LPR, OPT>(TI, op[r], pm[r], pv[r]);
            if (!SH && ok && fn[r]) row_moments<LPR, OPT>(TI, on[r], nm[r], nv[r]);
        }
        uint32_t ju[UN], jp[UN], jn[UN], gl[UN];
        float yd[UN];
#pragma unroll
        for (int r = 0; r < UN; ++r) {
            const int64_t t = base + (int64_t)(UN + r) * TG;
            const int64_t tc = t < B ? t : B - 1;
            ju[r] = (uint32_t)uid[tc]; jp[r] = (uint32_t)pid[tc]; jn[r] = (uint32_t)nid[tc];
            gl[r] = flags4[tc];
            yd[r] = XD ? xdiff[tc] : 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);                  // keep the requests above the arithmetic (the scheduler sinks them otherwise)
        float gco[UN], sus[UN], sps[UN], lss[UN];
#pragma unroll
        for (int r = 0; r < UN; ++r) {
            float x;
            if (XD) { x = xd[r]; sus[r] = sps[r] = 0.f; }
            else {
                const float dp = group_sum<LPR>(dot4(u[r], p[r]));
                const float dn = group_sum<LPR>(dot4(u[r], n[r]));
                sus[r] = group_sum<LPR>(dot4(u[r], u[r]));
                sps[r] = group_sum<LPR>(dot4(p[r], p[r]));
                x = dp - dn;
            }
            bpr_term(x, gamma, invB, lss[r], gco[r]);
        }
        // every request of this iteration -- rows AND the next ids -- has returned here; nothing below waits on vmcnt again
#pragma unroll
        for (int r = 0; r < UN; ++r) asm volatile("" : "+v"(ju[r]), "+v"(jp[r]), "+v"(jn[r]), "+v"(gl[r]), "+v"(yd[r]));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < UN; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const float g = gco[r];
            const float4 gu = make_float4(g * (p[r].x - n[r].x), g * (p[r].y - n[r].y), g * (p[r].z - n[r].z), g * (p[r].w - n[r].w));
            const float4 gi = make_float4(g * u[r].x, g * u[r].y, g * u[r].z, g * u[r].w);
            const bool ok = t < B && live;
            // ---- user row
            if (fu[r]) {
                const float4 wu = upd_math<OPT>(u[r], um[r], uv[r], gu, cu, hu);
                // row_store, in place: the helper changed the code of the SH kernel at 64 lanes per row (Adam)
                if (live) { if (OPT == 1) { st4n<(LPR >= 32)>(TU.M + ou[r], um[r]); st4n<(LPR >= 32)>(TU.V + ou[r], uv[r]); }
                            if constexpr (OPT == 2) st4n<(LPR >= 32)>(TU.V + ou[r], uv[r]);
                            st4n<(LPR >= 32)>(TU.W + ou[r], wu); }
                if (NC) norm_rec_store<LPR>(NU + (int64_t)iu[r] * kNormRecFloats, group_sum<LPR>(sqnorm4<LPR>(wu)), sub);
            } else if (ok) st4n<(LPR >= 32)>(GU + t * D + 4 * sub, gu);
            // ---- positive item row (EmbLoss occurrence), negative item row (gradient -g u, no EmbLoss)
            if (SH) {
                if (fp[r] && live) st4n<(LPR >= 32)>(GS + op[r], make_float4(__builtin_fmaf(ci, p[r].x, gi.x), __builtin_fmaf(ci, p[r].y, gi.y),
                                                               __builtin_fmaf(ci, p[r].z, gi.z), __builtin_fmaf(ci, p[r].w, gi.w)));
                if (fn[r] && live) st4n<(LPR >= 32)>(GS + on[r], make_float4(0.f - gi.x, 0.f - gi.y, 0.f - gi.z, 0.f - gi.w));
            } else {
            if (fp[r]) {
                const float4 wp = upd_math<OPT>(p[r], pm[r], pv[r], gi, ci, hi);
                if (live) row_store<LPR, OPT>(TI, op[r], wp, pm[r], pv[r]);
                if (NC) norm_rec_store<LPR>(NI + (int64_t)ip[r] * kNormRecFloats, group_sum<LPR>(sqnorm4<LPR>(wp)), sub);
            }
            if (fn[r]) {
                const float4 wn = upd_math<OPT>(n[r], nm[r], nv[r], make_float4(0.f - gi.x, 0.f - gi.y, 0.f - gi.z, 0.f - gi.w), 0.f, hi);
                if (live) row_store<LPR, OPT>(TI, on[r], wn, nm[r], nv[r]);
                if (NC) norm_rec_store<LPR>(NI + (int64_t)in[r] * kNormRecFloats, group_sum<LPR>(sqnorm4<LPR>(wn)), sub);
            }
            }
            if (ok && !(fp[r] && fn[r])) st4n<(LPR >= 32)>(GP + t * D + 4 * sub, gi);
            if (t < B && sub == 0) {
                acc[0] += (double)lss[r];
                acc[1] += (double)sus[r];
                acc[2] += (double)sps[r];
            }
        }
#pragma unroll
        for (int r = 0; r < UN; ++r) { iu[r] = ju[r]; ip[r] = jp[r]; in[r] = jn[r]; fl[r] = gl[r]; xd[r] = yd[r]; }
    }
    block_sum_d<3>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// The pointwise rows (user, item, label) -- EMCDR's default MF latent factor model (emcdr.py:111-122: MSE on the raw dot) and CMF's BCE
// (cmf.py:75-99) -- through the same forward-and-update pass (round 5): flags4[t] byte 0 / byte 1 = the row's user / item occurs once in the
// batch; such a row is updated in place from registers (gradient g v resp. g u plus its EmbLoss term), a duplicate row's gradient row goes
// to GU[t] / GI[t] for the segmented apply.  Same prefetch discipline as bpr_fwd_apply_kernel (ids, labels and flags of the next iteration
// requested behind this iteration's row loads and waited for before its stores).
// XD: the row's dot <u, i> is GIVEN (xdot[t]: the all-reduced sum of every rank's column-slice partials, the dimension-sharded step).
template <int LPR, int OPT, bool XD = false>
__global__ __launch_bounds__(kBlock) void point_fwd_apply_kernel(int loss_kind, tab_ptrs TU, tab_ptrs TI, int D, const int64_t* __restrict__ uid,
                                                                 const int64_t* __restrict__ iid, const float* __restrict__ label,
                                                                 const uint32_t* __restrict__ flags4, int64_t B, float invB,
                                                                 const float* __restrict__ coef, apply_hp hu, apply_hp hi,
                                                                 float* __restrict__ GU, float* __restrict__ GI, double* __restrict__ partials,
                                                                 const float* __restrict__ xdot = nullptr) {
    HP_FROM_DEV(hu); HP_FROM_DEV(hi);
    constexpr int GPB = kBlock / LPR;
    __shared__ double smem[3 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const bool live = sub < (D >> 2);
    const float cu = coef[0], ci = coef[1];
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    double acc[3] = {0.0, 0.0, 0.0};
    uint32_t iu, ii, fl; float yl, xd = 0.f;
    {
        const int64_t tc = gg < B ? gg : B - 1;
        iu = (uint32_t)uid[tc]; ii = (uint32_t)iid[tc]; fl = flags4[tc]; yl = label[tc];
        if (XD) xd = xdot[tc];
    }
    asm volatile("" : "+v"(iu), "+v"(ii), "+v"(fl), "+v"(yl), "+v"(xd));
    for (int64_t t = gg; t < B; t += TG) {
        const bool fu = (fl & 0xFFu) != 0, fi = (fl & 0xFF00u) != 0;
        const int64_t ou = (int64_t)iu * D + 4 * sub, oi = (int64_t)ii * D + 4 * sub;
        float4 u = live ? ld4n<(LPR >= 32)>(TU.W + ou) : z4, v = live ? ld4n<(LPR >= 32)>(TI.W + oi) : z4;
        float4 um = z4, uv = z4, im = z4, iv = z4;
        if (live && fu) row_moments<LPR, OPT>(TU, ou, um, uv);
        if (live && fi) row_moments<LPR, OPT>(TI, oi, im, iv);
        uint32_t ju, ji, gl; float yn, xn = 0.f;
        {
            const int64_t tn = t + TG, tc = tn < B ? tn : B - 1;
            ju = (uint32_t)uid[tc]; ji = (uint32_t)iid[tc]; gl = flags4[tc]; yn = label[tc];
            if (XD) xn = xdot[tc];
        }
        __builtin_amdgcn_sched_barrier(0);
        const float dx = XD ? xd : group_sum<LPR>(dot4(u, v));
        const float su = XD ? 0.f : group_sum<LPR>(dot4(u, u));
        const float si = XD ? 0.f : group_sum<LPR>(dot4(v, v));
        float l, g;
        point_term(loss_kind, dx, yl, invB, l, g);
        asm volatile("" : "+v"(ju), "+v"(ji), "+v"(gl), "+v"(yn), "+v"(xn));        // every request of this iteration has returned: stores below wait on nothing older
        __builtin_amdgcn_sched_barrier(0);
        const float4 gu = make_float4(g * v.x, g * v.y, g * v.z, g * v.w);
        const float4 gi = make_float4(g * u.x, g * u.y, g * u.z, g * u.w);
        if (fu) {
            const float4 wu = upd_math<OPT>(u, um, uv, gu, cu, hu);
            if (live) row_store<LPR, OPT>(TU, ou, wu, um, uv);
        } else if (live) st4n<(LPR >= 32)>(GU + t * D + 4 * sub, gu);
        if (fi) {
            const float4 wi = upd_math<OPT>(v, im, iv, gi, ci, hi);
            if (live) row_store<LPR, OPT>(TI, oi, wi, im, iv);
        } else if (live) st4n<(LPR >= 32)>(GI + t * D + 4 * sub, gi);
        if (sub == 0) { acc[0] += (double)l; acc[1] += (double)su; acc[2] += (double)si; }
        iu = ju; ii = ji; fl = gl; yl = yn; xd = xn;
    }
    block_sum_d<3>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// The same idea on recbole's pairwise batch layout (S positives tiled k times, negatives k-major: crossdomain_sampler.py:148-152;
// csrc/cdr_kstep.hip): one lane group per POSITIVE gathers u and p once and its k negatives; every row among them that occurs once
// in the step's lists (users [S]; items [pid | nid]) is updated in place from registers -- user: sum_m g_m (p - n_m) + k c_u u,
// positive: (sum_m g_m) u + k c_i p, negative m: -g_m u -- and a duplicate row's gradient row goes to GU[j] / GI[occurrence] for
// the segmented apply (no {user row, coefficient} records here: the user row an item gradient is made of is updated by this very
// kernel).  flags: fstride bytes per positive {user, positive, negative 0 .. k - 1} from occ_flags_kernel.
template <int LPR, int OPT, int KC>
__global__ __launch_bounds__(kBlock) void bpr_fwd_apply_kmajor_kernel(tab_ptrs TU, tab_ptrs TI, int D, const int64_t* __restrict__ uid,
                                                                      const int64_t* __restrict__ pid, const int64_t* __restrict__ nid,
                                                                      const uint8_t* __restrict__ flags, int fstride, int64_t S, int k,
                                                                      float gamma, float invB, const float* __restrict__ coef,
                                                                      apply_hp hu, apply_hp hi, float* __restrict__ GU,
                                                                      float* __restrict__ GI, double* __restrict__ partials) {
    HP_FROM_DEV(hu); HP_FROM_DEV(hi);
    constexpr int GPB = kBlock / LPR;
    __shared__ double smem[3 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int D4 = D >> 2;
    const bool live = sub < D4;
    const float cu = coef[0], ci = coef[1];                 // pre-multiplied by k (coef_finish_kernel)
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t j = gg; j < S; j += TG) {
        const uint8_t* fl = flags + j * fstride;
        const int64_t iu = uid[j], ip = pid[j];
        const bool fu = fl[0] != 0, fp = fl[1] != 0;
        int64_t in0[KC]; bool fn0[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) { const int m = c < k ? c : k - 1; in0[c] = nid[j + (int64_t)m * S]; fn0[c] = fl[2 + m] != 0; }
        const int64_t ou = iu * D + 4 * sub, op = ip * D + 4 * sub;
        float4 u = z4, p = z4, um = z4, uv = z4, pm = z4, pv = z4;
        if (live) {
            u = ld4n<(LPR >= 32)>(TU.W + ou); p = ld4n<(LPR >= 32)>(TI.W + op);
            if (fu) row_moments<LPR, OPT>(TU, ou, um, uv);
            if (fp) row_moments<LPR, OPT>(TI, op, pm, pv);
        }
        float4 gu = z4;
        float gs = 0.f, dp = 0.f;
        for (int m0 = 0; m0 < k; m0 += KC) {
            int64_t in[KC], on[KC]; bool fn[KC];
            float4 n[KC], nm[KC], nv[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                if (m0 == 0) { in[c] = in0[c]; fn[c] = fn0[c]; }
                else { const int m = m0 + c < k ? m0 + c : k - 1; in[c] = nid[j + (int64_t)m * S]; fn[c] = fl[2 + m] != 0; }
                fn[c] = fn[c] && m0 + c < k;
                on[c] = in[c] * D + 4 * sub;
            }
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                n[c] = live ? ld4n<(LPR >= 32)>(TI.W + on[c]) : z4;
                nm[c] = nv[c] = z4;
                if (live && fn[c]) row_moments<LPR, OPT>(TI, on[c], nm[c], nv[c]);
            }
            if (m0 == 0) {
                dp = group_sum<LPR>(dot4(u, p));
                const float su = group_sum<LPR>(dot4(u, u)), sp = group_sum<LPR>(dot4(p, p));
                if (sub == 0) { acc[1] += (double)k * (double)su; acc[2] += (double)k * (double)sp; }      // EmbLoss sees k copies
            }
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const float dn = group_sum<LPR>(dot4(u, n[c]));
                if (m0 + c < k) {
                    const float sg = sigmoidf_(dp - dn);
                    const float g = bpr_grad(sg, gamma, invB);
                    gu.x += g * (p.x - n[c].x); gu.y += g * (p.y - n[c].y); gu.z += g * (p.z - n[c].z); gu.w += g * (p.w - n[c].w);
                    gs += g;
                    if (sub == 0) acc[0] += (double)bpr_loss(sg, gamma);
                    const float4 gn = make_float4(0.f - g * u.x, 0.f - g * u.y, 0.f - g * u.z, 0.f - g * u.w);
                    if (fn[c]) {
                        const float4 wn = upd_math<OPT>(n[c], nm[c], nv[c], gn, 0.f, hi);
                        if (live) row_store<LPR, OPT>(TI, on[c], wn, nm[c], nv[c]);
                    } else if (live) st4n<(LPR >= 32)>(GI + (S + j + (int64_t)(m0 + c) * S) * D + 4 * sub, gn);
                }
            }
        }
        if (fu) {
            const float4 wu = upd_math<OPT>(u, um, uv, gu, cu, hu);
            if (live) row_store<LPR, OPT>(TU, ou, wu, um, uv);
        } else if (live) st4n<(LPR >= 32)>(GU + j * D + 4 * sub, gu);
        const float4 gp = make_float4(gs * u.x, gs * u.y, gs * u.z, gs * u.w);
        if (fp) {
            const float4 wp = upd_math<OPT>(p, pm, pv, gp, ci, hi);
            if (live) row_store<LPR, OPT>(TI, op, wp, pm, pv);
        } else if (live) st4n<(LPR >= 32)>(GI + j * D + 4 * sub, gp);
    }
    block_sum_d<3>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// ---- pointwise rows per POSITIVE (round 5) ---------------------------------------------------------------------------------------------
// recbole's pointwise batch (TrainDataLoader._neg_sampling, driven by data/dataloader.py:114-162): S positives, the user column tiled 1 + k
// times, items = [positives | k-major negatives], labels = [1] * S + [0] * S k.  In that layout EVERY user row occurs 1 + k times, so the
// per-row kernel above never finds a user that occurs once; here one lane group takes a positive with its k negatives: the user row is
// gathered once, its gradient sum_r g_r i_r accumulated in registers, and a user that occurs in ONE positive is updated in place (EmbLoss
// count 1 + k); every item row among the 1 + k that occurs once in [pid | nid] is updated in place (g_r u, EmbLoss count 1).  Lists, flags
// and gradient buffers exactly as bpr_fwd_apply_kmajor_kernel's: users [S] -> GU [S, D]; items [pid | nid] -> GI [S + S k, D].
template <int LPR>
__global__ __launch_bounds__(kBlock) void point_norms_kmajor_kernel(const float* __restrict__ U, const float* __restrict__ I, int D,
                                                                    const int64_t* __restrict__ uid, const int64_t* __restrict__ iid, int64_t S,
                                                                    int k, double* __restrict__ partials) {
    constexpr int GPB = kBlock / LPR;
    __shared__ double smem[2 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const bool live = sub < (D >> 2);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    double acc[2] = {0.0, 0.0};
    for (int64_t j = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR; j < S; j += (int64_t)gridDim.x * GPB) {
        const float4 u = live ? ld4n<(LPR >= 32)>(U + uid[j] * D + 4 * sub) : z4;
        float si = 0.f;
        for (int r0 = 0; r0 <= k; r0 += 4) {                       // four item rows in flight
            float4 v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = (live && r0 + c <= k) ? ld4n<(LPR >= 32)>(I + iid[j + (int64_t)(r0 + c) * S] * D + 4 * sub) : z4;
#pragma unroll
            for (int c = 0; c < 4; ++c) si += dot4(v[c], v[c]);
        }
        const float su = group_sum<LPR>(dot4(u, u)), st = group_sum<LPR>(si);
        if (sub == 0) { acc[0] += (double)(1 + k) * (double)su; acc[1] += (double)st; }
    }
    block_sum_d<2>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// out9[4], out9[5] = reg_weight / (B ||rows||) as coef_finish_kernel; out9[9] = (1 + k) out9[4]: the user coefficient per LIST occurrence
__global__ __launch_bounds__(kBlock) void point_coef_kmajor_kernel(const double* __restrict__ partials, int nblocks, int64_t B, int k,
                                                                   float reg_weight, float* __restrict__ out9, unsigned* __restrict__ zero4) {
    __shared__ double smem[2 * (kBlock / 64)];
    if (zero4 && threadIdx.x >= 64 && threadIdx.x < 68) zero4[threadIdx.x - 64] = 0u;
    double acc[2] = {0.0, 0.0};
    sum_partials<2, kBlock>(partials, nblocks, acc, smem);
    if (threadIdx.x == 0) {
        const float nu = (float)sqrt(acc[0]), ni = (float)sqrt(acc[1]);
        out9[4] = embloss_coef(reg_weight, B, nu);
        out9[5] = embloss_coef(reg_weight, B, ni);
        out9[9] = (float)(1 + k) * out9[4];
    }
}

template <int LPR, int OPT, int KC>
__global__ __launch_bounds__(kBlock) void point_fwd_apply_kmajor_kernel(int loss_kind, tab_ptrs TU, tab_ptrs TI, int D, const int64_t* __restrict__ uid,
                                                                        const int64_t* __restrict__ iid, const float* __restrict__ label,
                                                                        const uint8_t* __restrict__ flags, int fstride, int64_t S, int k,
                                                                        float invB, const float* __restrict__ coef, apply_hp hu, apply_hp hi,
                                                                        float* __restrict__ GU, float* __restrict__ GI,
                                                                        double* __restrict__ partials) {
    HP_FROM_DEV(hu); HP_FROM_DEV(hi);
    constexpr int GPB = kBlock / LPR;
    __shared__ double smem[3 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const bool live = sub < (D >> 2);
    const float cu = coef[5], ci = coef[1];                 // coef = out9 + 4: {c_u, c_i, ..., (1 + k) c_u at out9[9]}
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t j = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR; j < S; j += (int64_t)gridDim.x * GPB) {
        const uint8_t* fl = flags + j * fstride;
        const int64_t iu = uid[j];
        const bool fu = fl[0] != 0;
        const int64_t ou = iu * D + 4 * sub;
        float4 u = z4, um = z4, uv = z4;
        if (live) {
            u = ld4n<(LPR >= 32)>(TU.W + ou);
            if (fu) row_moments<LPR, OPT>(TU, ou, um, uv);
        }
        float4 gu = z4;
        float su = 0.f;
        for (int r0 = 0; r0 <= k; r0 += KC) {                   // item rows r = 0 (the positive), 1 .. k (negatives), KC at a time
            int64_t oi[KC]; bool fi[KC]; float yl[KC];
            float4 v[KC], vm[KC], vv[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int r = r0 + c <= k ? r0 + c : k;
                oi[c] = iid[j + (int64_t)r * S] * D + 4 * sub;
                fi[c] = fl[1 + r] != 0 && r0 + c <= k;
                yl[c] = label[j + (int64_t)r * S];
            }
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                v[c] = live ? ld4n<(LPR >= 32)>(TI.W + oi[c]) : z4;
                vm[c] = vv[c] = z4;
                if (live && fi[c]) row_moments<LPR, OPT>(TI, oi[c], vm[c], vv[c]);
            }
            if (r0 == 0) su = group_sum<LPR>(dot4(u, u));
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const float dx = group_sum<LPR>(dot4(u, v[c]));
                const float si = group_sum<LPR>(dot4(v[c], v[c]));
                if (r0 + c <= k) {
                    const float y = yl[c];
                    float l, g;
                    point_term(loss_kind, dx, y, invB, l, g);
                    gu.x += g * v[c].x; gu.y += g * v[c].y; gu.z += g * v[c].z; gu.w += g * v[c].w;
                    if (sub == 0) { acc[0] += (double)l; acc[2] += (double)si; }
                    const float4 gi = make_float4(g * u.x, g * u.y, g * u.z, g * u.w);
                    if (fi[c]) {
                        const float4 wi = upd_math<OPT>(v[c], vm[c], vv[c], gi, ci, hi);
                        if (live) row_store<LPR, OPT>(TI, oi[c], wi, vm[c], vv[c]);
                    } else if (live) st4n<(LPR >= 32)>(GI + (j + (int64_t)(r0 + c) * S) * D + 4 * sub, gi);
                }
            }
        }
        if (sub == 0) acc[1] += (double)(1 + k) * (double)su;
        if (fu) {
            const float4 wu = upd_math<OPT>(u, um, uv, gu, cu, hu);
            if (live) row_store<LPR, OPT>(TU, ou, wu, um, uv);
        } else if (live) st4n<(LPR >= 32)>(GU + j * D + 4 * sub, gu);
    }
    block_sum_d<3>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// End of a MEDIUM segment (3 .. kLongSeg occurrences) headed at sorted position q: the first position past q + 2 whose key differs.
// One probe per lane and a ballot instead of a walk (round 6): the walk was a chain of up to 30 dependent key loads per segment -- most of
// the 60 us the duplicate apply took on a Zipf(1.05) batch of 65,536 triples, whose items of rank 100 .. 3,000 have such segments.
template <int LPR>
__device__ __forceinline__ int64_t seg_end_probe(const uint32_t* __restrict__ keys, int64_t q, int64_t n, uint32_t row) {
    if constexpr (LPR >= 32) {
        const int lane = threadIdx.x & 63, l = lane & 31;
        const int64_t p = q + 3 + l;
        const bool same = (LPR == 32 || lane < 32) && p < n && p <= q + kLongSeg && keys[p] == row;
        const unsigned long long m = __ballot(!same);
        const uint32_t mg = LPR == 32 ? (uint32_t)(m >> (lane & 32)) : (uint32_t)m;
        return q + 3 + (mg ? (int64_t)(__ffs((int)mg) - 1) : 32);
    } else {
        int64_t end = q + 3;
        while (end < n && end <= q + kLongSeg && keys[end] == row) ++end;
        return end;
    }
}

// The occurrence numbers of a medium segment's third and later entries, one per lane (lane l of the group: sorted position q + 2 + l),
// fetched together behind the end probe: the rounds below hand them round with lane shuffles instead of loading perm[] ahead of every
// round's row loads (one dependent hop per round less).
template <int LPR>
__device__ __forceinline__ uint32_t seg_occ_fetch(const uint32_t* __restrict__ perm, int64_t q, int64_t end) {
    if constexpr (LPR >= 32) {
        const int l = threadIdx.x & 31;
        return ((LPR == 32 || (threadIdx.x & 63) < 32) && q + 2 + l < end) ? perm[q + 2 + l] : 0u;
    } else {
        return 0u;
    }
}
template <int LPR>
__device__ __forceinline__ int64_t seg_occ_at(const uint32_t* __restrict__ perm, uint32_t mine, int64_t q, int64_t e) {
    if constexpr (LPR >= 32) return (int64_t)__shfl(mine, (int)(e - (q + 2)), LPR);      // (LPR = 64: the values sit in the wave's lower half)
    else return (int64_t)perm[e];
}

// The segmented apply over the DUPLICATE segments only: heads[0 .. *nheads) are the sorted positions of their first occurrences
// (any order: every segment is summed by one lane group in occurrence order, whoever takes it).  Long segments as in
// rowwise_apply_kernel.  NC (whole rows per lane group only): the updated row's squared-norm record goes to n2.
template <int LPR, int OPT, bool SIGNED, bool NC = false>
__device__ __forceinline__ void rowwise_apply_dups_body(float* __restrict__ W, float* __restrict__ Mo, float* __restrict__ Vo,
                                                        int D, const uint32_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ perm, int64_t n,
                                                        const uint32_t* __restrict__ heads, const unsigned* __restrict__ nheads,
                                                        const float* __restrict__ G, int64_t neg_start, int64_t reg_limit,
                                                        const float* __restrict__ reg_coef, apply_hp hp,
                                                        unsigned* __restrict__ counters, seg_long* __restrict__ longs,
                                                        seg_piece* __restrict__ pieces, float* __restrict__ n2 = nullptr) {
    HP_FROM_DEV(hp);
    const tab_ptrs T{W, Mo, Vo};
    constexpr int GPB = kBlock / LPR;
    constexpr int SU = 4;                                 // segments in flight per lane group
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int D4 = D >> 2;
    const float c = reg_coef ? reg_coef[0] : 0.f;
    const int64_t nh = (int64_t)nheads[0];
    if (D4 <= LPR) {
        // Whole rows per lane (D <= 256).  A segment is a chain of dependent random accesses (head -> keys -> perm -> gradient rows,
        // next to w, m, v): one segment at a time per lane group left the kernel latency-bound (0.197 ms for 0.8 GB at C5).  SU
        // segments go through the chain together: SU heads, then SU x 3 keys, then their rows, moments and the first two
        // occurrences' gradient rows (most duplicate rows have two or three occurrences) are all requested before anything is used.
        const bool live = sub < D4;
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t h0 = gg * SU; h0 < nh; h0 += TG * SU) {
            int64_t q[SU]; uint32_t row[SU], k1[SU], k2[SU]; bool ok[SU];
#pragma unroll
            for (int j = 0; j < SU; ++j) { ok[j] = h0 + j < nh; q[j] = ok[j] ? (int64_t)heads[h0 + j] : 0; }
#pragma unroll
            for (int j = 0; j < SU; ++j) {
                row[j] = keys[q[j]];
                k1[j] = q[j] + 1 < n ? keys[q[j] + 1] : ~0u;               // (a head of a duplicate segment: keys[q + 1] == row)
                k2[j] = q[j] + 2 < n ? keys[q[j] + 2] : ~0u;
            }
            uint32_t far[SU], o0[SU], o1[SU];
#pragma unroll
            for (int j = 0; j < SU; ++j) {
                far[j] = q[j] + kLongSeg < n ? keys[q[j] + kLongSeg] : ~0u;
                o0[j] = perm[q[j]]; o1[j] = q[j] + 1 < n ? perm[q[j] + 1] : 0u;
            }
            float4 w[SU], m[SU], v[SU], g0[SU], g1[SU];
            int64_t off[SU];
#pragma unroll
            for (int j = 0; j < SU; ++j) {
                ok[j] = ok[j] && !(far[j] == row[j] && row[j] != ~0u && q[j] + kLongSeg < n);      // long segments: registered below
                off[j] = (int64_t)row[j] * D + 4 * sub;
                w[j] = m[j] = v[j] = g0[j] = g1[j] = z4;
                if (ok[j] && live) {
                    w[j] = ld4n<(LPR >= 32)>(W + off[j]);
                    row_moments<LPR, OPT>(T, off[j], m[j], v[j]);
                    const bool n0 = SIGNED && (int64_t)o0[j] >= neg_start, n1 = SIGNED && (int64_t)o1[j] >= neg_start;
                    g0[j] = ld4n<(LPR >= 32)>(G + (n0 ? (int64_t)o0[j] - neg_start : (int64_t)o0[j]) * D + 4 * sub);
                    g1[j] = ld4n<(LPR >= 32)>(G + (n1 ? (int64_t)o1[j] - neg_start : (int64_t)o1[j]) * D + 4 * sub);
                }
            }
#pragma unroll
            for (int j = 0; j < SU; ++j) {
                if (!ok[j]) continue;
                float4 acc = z4;
                int cnt = 0;
                {   // occurrences 0 and 1 (always present), in occurrence order, exactly as the one-at-a-time loop adds them
                    const bool n0 = SIGNED && (int64_t)o0[j] >= neg_start, n1 = SIGNED && (int64_t)o1[j] >= neg_start;
                    if (n0) { acc.x -= g0[j].x; acc.y -= g0[j].y; acc.z -= g0[j].z; acc.w -= g0[j].w; }
                    else { acc.x += g0[j].x; acc.y += g0[j].y; acc.z += g0[j].z; acc.w += g0[j].w; }
                    cnt += ((int64_t)o0[j] < reg_limit) ? 1 : 0;
                    if (n1) { acc.x -= g1[j].x; acc.y -= g1[j].y; acc.z -= g1[j].z; acc.w -= g1[j].w; }
                    else { acc.x += g1[j].x; acc.y += g1[j].y; acc.z += g1[j].z; acc.w += g1[j].w; }
                    cnt += ((int64_t)o1[j] < reg_limit) ? 1 : 0;
                }
                if (k2[j] == row[j]) {                                     // third and later occurrences (at most kLongSeg - 2 of them)
                    // the segment's end first (its keys are neighbours in memory), then the gradient rows eight at a time: one at a time
                    // this walk was a chain of up to 30 dependent ~1.5 us loads per segment, which is what a Zipf batch's step waited for
                    const int64_t end = seg_end_probe<LPR>(keys, q[j], n, row[j]);
                    const uint32_t occ_l = seg_occ_fetch<LPR>(perm, q[j], end);
                    for (int64_t e0 = q[j] + 2; e0 < end; e0 += 8) {
                        int64_t o[8]; float4 g[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) { const int64_t ov = seg_occ_at<LPR>(perm, occ_l, q[j], e0 + u < end ? e0 + u : q[j] + 2); o[u] = e0 + u < end ? ov : -1; }
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const bool neg = SIGNED && o[u] >= neg_start;
                            g[u] = (o[u] >= 0 && live) ? ld4n<(LPR >= 32)>(G + (neg ? o[u] - neg_start : o[u]) * D + 4 * sub) : z4;
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            if (o[u] < 0) continue;
                            if (SIGNED && o[u] >= neg_start) { acc.x -= g[u].x; acc.y -= g[u].y; acc.z -= g[u].z; acc.w -= g[u].w; }
                            else { acc.x += g[u].x; acc.y += g[u].y; acc.z += g[u].z; acc.w += g[u].w; }
                            cnt += (o[u] < reg_limit) ? 1 : 0;
                        }
                    }
                }
                const float4 wn = upd_math<OPT>(w[j], m[j], v[j], acc, c * (float)cnt, hp);
                if (live) row_store<LPR, OPT>(T, off[j], wn, m[j], v[j]);
                if (NC) norm_rec_store<LPR>(n2 + (int64_t)row[j] * kNormRecFloats, group_sum<LPR>(sqnorm4<LPR>(wn)), sub);
            }
        }
    } else {
        for (int64_t h = gg; h < nh; h += TG) {
            const int64_t q = heads[h];
            const uint32_t row = keys[q];
            const bool is_long = q + kLongSeg < n && keys[q + kLongSeg] == row;
            if (is_long) continue;
            for (int ch = sub; ch < D4; ch += LPR) {
                const int64_t off = (int64_t)row * D + 4 * ch;
                const float4 w = ld4n<(LPR >= 32)>(W + off);
                float4 m = make_float4(0.f, 0.f, 0.f, 0.f), v = m;
                row_moments<LPR, OPT>(T, off, m, v);
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                int cnt = 0;
                for (int64_t e = q; e < n && keys[e] == row; ++e) {
                    const int64_t o = perm[e];
                    const bool neg = SIGNED && o >= neg_start;
                    const float4 g = ld4n<(LPR >= 32)>(G + (neg ? o - neg_start : o) * D + 4 * ch);
                    if (neg) { acc.x -= g.x; acc.y -= g.y; acc.z -= g.z; acc.w -= g.w; }
                    else { acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w; }
                    cnt += (o < reg_limit) ? 1 : 0;
                }
                const float4 wn = upd_math<OPT>(w, m, v, acc, c * (float)cnt, hp);
                row_store<LPR, OPT>(T, off, wn, m, v);
            }
        }
    }
    if (counters == nullptr) return;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q + kLongSeg < n; q += (int64_t)gridDim.x * kBlock) {
        const uint32_t row = keys[q];
        const uint32_t before = keys[q > 0 ? q - 1 : 0];
        const uint32_t far = keys[q + kLongSeg];
        if ((q > 0 && before == row) || far != row || row == ~0u) continue;       // (~0: the count path's filler behind the duplicate entries)
        int64_t lo = q + kLongSeg, hi = n;
        while (lo + 1 < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] == row) lo = mid; else hi = mid;
        }
        const int64_t len = hi - q;
        const unsigned np = (unsigned)((len + kPiece - 1) / kPiece);
        const unsigned base = atomicAdd(&counters[0], np);
        const unsigned li = atomicAdd(&counters[1], 1u);
        longs[li] = seg_long{q, len, (int64_t)base};
        for (unsigned k = 0; k < np; ++k) {
            const int64_t st = q + (int64_t)k * kPiece;
            pieces[base + k] = seg_piece{st, (hi - st) < kPiece ? (hi - st) : (int64_t)kPiece};
        }
    }
}
// The two tables of a fused step in ONE launch each (round 4): blockIdx.y = 0 the user table's duplicate segments, 1 the item table's.
// The device functions are the ones above with SIGNED = true for both sides -- the user side passes neg_start = n, so no occurrence is
// ever negated: the same sums in the same order as the two launches of round 3.  (Not the same BITS as the round-3 build on rows whose
// moments are non-zero: hipcc fuses the Adam update's multiply-adds differently in this instantiation -- 1 ulp on such rows, found by
// running both builds on one batch, tools/ab_step_builds.py; reruns of one build are bit-equal as before.)  At 65,536 triples the step's six
// small apply launches and three counter clears were ~45 us of its 230; the two sides also share the chip instead of queueing.
struct dup_side {
    float* W; float* M; float* V; const uint32_t* keys; const uint32_t* perm; int64_t n; const uint32_t* heads; const unsigned* nheads;
    const float* G; int64_t neg_start, reg_limit; const float* reg_coef; apply_hp hp;
    unsigned* counters; seg_long* longs; seg_piece* pieces; int* pcnt; float* partial;
    float* out = nullptr; const uint32_t* uidx = nullptr;     // row shard, item side: W = the received rows (read-only), out[uidx[position]] = the segment's sum
    float* n2 = nullptr;                                      // NC kernels: the table's squared-norm records (moved back by key_base rows like W)
};
template <int LPR, int OPT, bool NC = false>
__global__ __launch_bounds__(kBlock) void rowwise_apply_dups2_kernel(int D, dup_side a, dup_side b) {
    const dup_side& t = blockIdx.y ? b : a;
    rowwise_apply_dups_body<LPR, OPT, true, NC>(t.W, t.M, t.V, D, t.keys, t.perm, t.n, t.heads, t.nheads, t.G, t.neg_start, t.reg_limit, t.reg_coef, t.hp,
                                                t.counters, t.longs, t.pieces, t.n2);
}
template <int LPR>
__global__ __launch_bounds__(kBlock) void seg_piece_sum2_kernel(int D, dup_side a, dup_side b) {
    const dup_side& t = blockIdx.y ? b : a;
    if (t.counters == nullptr) return;
    seg_piece_sum_body<LPR, true>(D, t.perm, t.G, t.neg_start, t.reg_limit, nullptr, t.counters, t.pieces, t.partial, t.pcnt);
}
template <int LPR, int OPT, bool NC = false>
__global__ __launch_bounds__(kBlock) void seg_long_finish2_kernel(int D, dup_side a, dup_side b) {
    const dup_side& t = blockIdx.y ? b : a;
    if (t.counters == nullptr) return;
    seg_long_finish_body<LPR, OPT, NC>(t.W, t.M, t.V, D, t.keys, t.reg_coef, t.hp, t.counters, t.longs, t.partial, t.pcnt, t.n2);
}

// ================================================================================================ round 6: the row-sharded step's own passes
// Keys of one requester-side sort for BOTH lists of a rank's routed triples (recv3 [Bl, 3] = {local user row, positive item, negative
// item}, item ids global): section A [0, Bl) = the user rows; section B [Bl, 3 Bl) = key_base + ((owner << lb) | local row) of [p | n],
// so that the distinct item rows come out grouped by owner, ascending inside an owner -- the order in which they are requested.
// Also unpacks the user column and clears the two head-list counters (cnt) of occ_flags_kernel.
__global__ __launch_bounds__(kBlock) void shard_keys_kernel(const int64_t* __restrict__ recv3, int64_t Bl, uint32_t G, unsigned lb,
                                                            uint32_t key_base, int64_t* __restrict__ u_loc, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ vals, unsigned* __restrict__ cnt,
                                                            uint32_t* __restrict__ zspan, int64_t zwords) {
    sort_state_clear(zspan, zwords);
    if (blockIdx.x == 0 && threadIdx.x < 4) cnt[threadIdx.x] = 0u;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < Bl; t += (int64_t)gridDim.x * kBlock) {
        const int64_t u = recv3[3 * t];
        const uint32_t p = (uint32_t)recv3[3 * t + 1], n = (uint32_t)recv3[3 * t + 2];
        u_loc[t] = u;
        keys[t] = (uint32_t)u; vals[t] = (uint32_t)t;
        keys[Bl + t] = key_base + (((p % G) << lb) | (p / G)); vals[Bl + t] = (uint32_t)t;
        keys[2 * Bl + t] = key_base + (((n % G) << lb) | (n / G)); vals[2 * Bl + t] = (uint32_t)(Bl + t);
    }
}

struct head_flag_op {                          // 1 where a sorted position starts a new key (the scan's input, never materialised)
    const uint32_t* keys;
    __device__ uint32_t operator()(uint32_t q) const { return (q == 0u || keys[q] != keys[q - 1]) ? 1u : 0u; }
};

// Section B after the scan of its head flags: uidx[q] = dense index of q's segment (= the distinct item's slot in the request list and in
// both row buffers), umap[occurrence] = the same per occurrence ([0, Bl) positives, [Bl, 2 Bl) negatives), uniq_local[j] = the local row
// asked of the owner, starts[k] = first slot of owner k (no atomics), n_uniq.
__global__ __launch_bounds__(kBlock) void shard_emit_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                            const uint32_t* __restrict__ excl, int64_t n, int world, unsigned lb,
                                                            uint32_t key_base, uint32_t* __restrict__ uidx, int64_t* __restrict__ uniq_local,
                                                            int64_t* __restrict__ umap, int64_t* __restrict__ starts,
                                                            int64_t* __restrict__ n_uniq) {
    const uint32_t lmask = (1u << lb) - 1u;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (int64_t)gridDim.x * kBlock) {
        const uint32_t key = keys[q] - key_base;
        const uint32_t prev = q > 0 ? keys[q - 1] - key_base : 0u;
        const bool head = q == 0 || prev != key;
        const uint32_t j = excl[q] + (head ? 1u : 0u) - 1u;
        uidx[q] = j;
        umap[perm[q]] = (int64_t)j;
        if (head) {
            uniq_local[j] = (int64_t)(key & lmask);
            const int owner = (int)(key >> lb), before = q > 0 ? (int)(prev >> lb) : -1;
            for (int k = before + 1; k <= owner; ++k) starts[k] = (int64_t)j;
        }
        if (q == n - 1) {
            n_uniq[0] = (int64_t)j + 1;
            for (int k = (int)(key >> lb) + 1; k <= world; ++k) starts[k] = (int64_t)j + 1;
        }
    }
}
__global__ void shard_counts_kernel(int64_t* __restrict__ starts_counts, int world) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        for (int k = 0; k < world; ++k) starts_counts[k] = starts_counts[k + 1] - starts_counts[k];
}

// partials[block] = {sum_t ||U[u_loc[t]]||^2, sum_t nrm2[ip[t]]}: the EmbLoss norms of a rank's routed triples.  The item rows' squared
// norms were formed by their OWNERS while they gathered the rows (cdr_gather_rows_norms) and travelled beside them: 4 bytes per distinct
// row instead of a second pass over the received rows.
template <int LPR>
__global__ __launch_bounds__(kBlock) void shard_norms_kernel(const float* __restrict__ U, int D, const int64_t* __restrict__ uid,
                                                             const float* __restrict__ nrm2, const int64_t* __restrict__ ip, int64_t B,
                                                             double* __restrict__ partials) {
    constexpr int GPB = kBlock / LPR;
    constexpr int UNR = 8;
    __shared__ double smem[2 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const bool live = sub < (D >> 2);
    double acc[2] = {0.0, 0.0};
    for (int64_t base = gg; base < B; base += TG * UNR) {
        int64_t iu[UNR], ii[UNR];
        float4 u[UNR];
        float pn[UNR];
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const int64_t tc = t < B ? t : B - 1;
            iu[r] = uid[tc]; ii[r] = ip[tc];
        }
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            u[r] = (t < B && live) ? ld4n<(LPR >= 32)>(U + iu[r] * D + 4 * sub) : make_float4(0.f, 0.f, 0.f, 0.f);
            pn[r] = (t < B && sub == 0) ? nrm2[ii[r]] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const float su = group_sum<LPR>(dot4(u[r], u[r]));
            if (sub == 0) { acc[0] += (double)su; acc[1] += (double)pn[r]; }
        }
    }
    block_sum_d<2>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// The duplicate ITEM segments of a rank's routed triples: out[uidx[head]] = signed sum of GP over the segment's occurrences, in
// occurrence order (+ for positives, - for negatives) + c_i * #positives * (the received row) -- the one gradient row that goes home for
// that item.  Structure and summation order of rowwise_apply_dups_body (SU segments in flight; third and later occurrences eight at a
// time; long segments registered for the piece kernels); nothing is updated here.
template <int LPR>
__device__ __forceinline__ void segsum_dups_body(int D, const dup_side& t) {
    constexpr int GPB = kBlock / LPR;
    constexpr int SU = 4;
    const uint32_t* __restrict__ keys = t.keys; const uint32_t* __restrict__ perm = t.perm; const uint32_t* __restrict__ heads = t.heads;
    const float* __restrict__ G = t.G; const float* __restrict__ rows = t.W; float* __restrict__ out = t.out;
    const uint32_t* __restrict__ uidx = t.uidx;
    const int64_t n = t.n, neg_start = t.neg_start, reg_limit = t.reg_limit;
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int D4 = D >> 2;
    const float c = t.reg_coef ? t.reg_coef[0] : 0.f;
    const int64_t nh = (int64_t)t.nheads[0];
    const bool live = sub < D4;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t h0 = gg * SU; h0 < nh; h0 += TG * SU) {
        int64_t q[SU]; uint32_t row[SU], k2[SU]; bool ok[SU];
#pragma unroll
        for (int j = 0; j < SU; ++j) { ok[j] = h0 + j < nh; q[j] = ok[j] ? (int64_t)heads[h0 + j] : 0; }
        uint32_t far[SU], o0[SU], o1[SU], ju[SU];
#pragma unroll
        for (int j = 0; j < SU; ++j) {
            row[j] = keys[q[j]];
            k2[j] = q[j] + 2 < n ? keys[q[j] + 2] : ~0u;
            far[j] = q[j] + kLongSeg < n ? keys[q[j] + kLongSeg] : ~0u;
            o0[j] = perm[q[j]]; o1[j] = q[j] + 1 < n ? perm[q[j] + 1] : 0u;
            ju[j] = uidx[q[j]];
        }
        float4 w[SU], g0[SU], g1[SU];
#pragma unroll
        for (int j = 0; j < SU; ++j) {
            ok[j] = ok[j] && !(far[j] == row[j] && row[j] != ~0u && q[j] + kLongSeg < n);
            w[j] = g0[j] = g1[j] = z4;
            if (ok[j] && live) {
                if (c != 0.f) w[j] = ld4n<(LPR >= 32)>(rows + (int64_t)ju[j] * D + 4 * sub);
                const bool n0 = (int64_t)o0[j] >= neg_start, n1 = (int64_t)o1[j] >= neg_start;
                g0[j] = ld4n<(LPR >= 32)>(G + (n0 ? (int64_t)o0[j] - neg_start : (int64_t)o0[j]) * D + 4 * sub);
                g1[j] = ld4n<(LPR >= 32)>(G + (n1 ? (int64_t)o1[j] - neg_start : (int64_t)o1[j]) * D + 4 * sub);
            }
        }
#pragma unroll
        for (int j = 0; j < SU; ++j) {
            if (!ok[j]) continue;
            float4 acc = z4;
            int cnt = 0;
            {
                const bool n0 = (int64_t)o0[j] >= neg_start, n1 = (int64_t)o1[j] >= neg_start;
                if (n0) { acc.x -= g0[j].x; acc.y -= g0[j].y; acc.z -= g0[j].z; acc.w -= g0[j].w; }
                else { acc.x += g0[j].x; acc.y += g0[j].y; acc.z += g0[j].z; acc.w += g0[j].w; }
                cnt += ((int64_t)o0[j] < reg_limit) ? 1 : 0;
                if (n1) { acc.x -= g1[j].x; acc.y -= g1[j].y; acc.z -= g1[j].z; acc.w -= g1[j].w; }
                else { acc.x += g1[j].x; acc.y += g1[j].y; acc.z += g1[j].z; acc.w += g1[j].w; }
                cnt += ((int64_t)o1[j] < reg_limit) ? 1 : 0;
            }
            if (k2[j] == row[j]) {
                const int64_t end = seg_end_probe<LPR>(keys, q[j], n, row[j]);
                const uint32_t occ_l = seg_occ_fetch<LPR>(perm, q[j], end);
                for (int64_t e0 = q[j] + 2; e0 < end; e0 += 8) {
                    int64_t o[8]; float4 g[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { const int64_t ov = seg_occ_at<LPR>(perm, occ_l, q[j], e0 + u < end ? e0 + u : q[j] + 2); o[u] = e0 + u < end ? ov : -1; }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        g[u] = (o[u] >= 0 && live) ? ld4n<(LPR >= 32)>(G + (o[u] >= neg_start ? o[u] - neg_start : o[u]) * D + 4 * sub) : z4;
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        if (o[u] < 0) continue;
                        if (o[u] >= neg_start) { acc.x -= g[u].x; acc.y -= g[u].y; acc.z -= g[u].z; acc.w -= g[u].w; }
                        else { acc.x += g[u].x; acc.y += g[u].y; acc.z += g[u].z; acc.w += g[u].w; }
                        cnt += (o[u] < reg_limit) ? 1 : 0;
                    }
                }
            }
            const float rc = c * (float)cnt;
            if (live) st4n<(LPR >= 32)>(out + (int64_t)ju[j] * D + 4 * sub, make_float4(__builtin_fmaf(rc, w[j].x, acc.x), __builtin_fmaf(rc, w[j].y, acc.y),
                                                                          __builtin_fmaf(rc, w[j].z, acc.z), __builtin_fmaf(rc, w[j].w, acc.w)));
        }
    }
    if (t.counters == nullptr) return;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q + kLongSeg < n; q += (int64_t)gridDim.x * kBlock) {
        const uint32_t row = keys[q];
        const uint32_t before = keys[q > 0 ? q - 1 : 0];
        const uint32_t far = keys[q + kLongSeg];
        if ((q > 0 && before == row) || far != row) continue;
        int64_t lo = q + kLongSeg, hi = n;
        while (lo + 1 < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] == row) lo = mid; else hi = mid;
        }
        const int64_t len = hi - q;
        const unsigned np = (unsigned)((len + kPiece - 1) / kPiece);
        const unsigned base = atomicAdd(&t.counters[0], np);
        const unsigned li = atomicAdd(&t.counters[1], 1u);
        t.longs[li] = seg_long{q, len, (int64_t)base};
        for (unsigned k = 0; k < np; ++k) {
            const int64_t st = q + (int64_t)k * kPiece;
            t.pieces[base + k] = seg_piece{st, (hi - st) < kPiece ? (hi - st) : (int64_t)kPiece};
        }
    }
}
template <int LPR>
__device__ __forceinline__ void segsum_long_finish_body(int D, const dup_side& t) {
    constexpr int GPB = kBlock / LPR;
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int D4 = D >> 2;
    const float c = t.reg_coef ? t.reg_coef[0] : 0.f;
    const int64_t nl = t.counters[1];
    for (int64_t li = gg; li < nl; li += TG) {
        const seg_long sg = t.longs[li];
        const int64_t j = t.uidx[sg.head];
        const int64_t np = (sg.len + kPiece - 1) / kPiece;
        for (int ch = sub; ch < D4; ch += LPR) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int cnt = 0;
            for (int64_t k0 = 0; k0 < np; k0 += 8) {
                float4 g[8]; int cc[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const bool in = k0 + u < np;
                    g[u] = in ? ld4n<(LPR >= 32)>(t.partial + (sg.base + k0 + u) * D + 4 * ch) : make_float4(0.f, 0.f, 0.f, 0.f);
                    cc[u] = in ? t.pcnt[sg.base + k0 + u] : 0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (k0 + u < np) { acc.x += g[u].x; acc.y += g[u].y; acc.z += g[u].z; acc.w += g[u].w; cnt += cc[u]; }
            }
            const float rc = c * (float)cnt;
            float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c != 0.f) w = ld4n<(LPR >= 32)>(t.W + j * D + 4 * ch);
            st4n<(LPR >= 32)>(t.out + j * D + 4 * ch, make_float4(__builtin_fmaf(rc, w.x, acc.x), __builtin_fmaf(rc, w.y, acc.y),
                                                    __builtin_fmaf(rc, w.z, acc.z), __builtin_fmaf(rc, w.w, acc.w)));
        }
    }
}
// blockIdx.y = 0: the duplicate USER rows (updated in place, as in the one-GPU step); 1: the duplicate ITEM segments (summed for the way home)
template <int LPR, int OPT>
__global__ __launch_bounds__(kBlock) void shard_dups_kernel(int D, dup_side a, dup_side b) {
    if (blockIdx.y == 0)
        rowwise_apply_dups_body<LPR, OPT, true>(a.W, a.M, a.V, D, a.keys, a.perm, a.n, a.heads, a.nheads, a.G, a.neg_start, a.reg_limit, a.reg_coef, a.hp,
                                                a.counters, a.longs, a.pieces);
    else segsum_dups_body<LPR>(D, b);
}
template <int LPR, int OPT>
__global__ __launch_bounds__(kBlock) void shard_long_finish_kernel(int D, dup_side a, dup_side b) {
    if (blockIdx.y == 0) {
        if (a.counters) seg_long_finish_body<LPR, OPT>(a.W, a.M, a.V, D, a.keys, a.reg_coef, a.hp, a.counters, a.longs, a.partial, a.pcnt);
    } else if (b.counters) segsum_long_finish_body<LPR>(D, b);
}
// out9[6] = this rank's loss sum (out9[7..8] keep the all-reduced norm sums the caller put there) + both sides' long-segment counters cleared
__global__ __launch_bounds__(kBlock) void shard_sums2_kernel(const double* __restrict__ partials, int nblocks, float* __restrict__ out9,
                                                             unsigned* __restrict__ zero_a, unsigned* __restrict__ zero_b) {
    __shared__ double smem[3 * (kBlock / 64)];
    if (zero_a && threadIdx.x >= 64 && threadIdx.x < 68) zero_a[threadIdx.x - 64] = 0u;
    if (zero_b && threadIdx.x >= 128 && threadIdx.x < 132) zero_b[threadIdx.x - 128] = 0u;
    double acc[3] = {0.0, 0.0, 0.0};
    sum_partials<3, kBlock>(partials, nblocks, acc, smem);
    if (threadIdx.x == 0) out9[6] = (float)acc[0];
}
// The owner's apply of ONE ascending duplicate-free run (what a single requester sends): position q updates row ids[q] with gradient row
// G[q] -- no keys, no permutation, no segments.  Two rows per lane group in flight, all four streams of a row (w, m, v, g) requested together.
template <int LPR, int OPT>
__global__ __launch_bounds__(kBlock) void apply_run_kernel(float* __restrict__ W, float* __restrict__ Mo, float* __restrict__ Vo, int D,
                                                           const int64_t* __restrict__ ids, int64_t n, const float* __restrict__ G, apply_hp hp) {
    HP_FROM_DEV(hp);
    const tab_ptrs T{W, Mo, Vo};
    constexpr int GPB = kBlock / LPR, UN = 2;
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const bool live = sub < (D >> 2);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t base = gg; base < n; base += TG * UN) {
        int64_t off[UN]; float4 w[UN], m[UN], v[UN], g[UN]; bool ok[UN];
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            const int64_t q = base + j * TG;
            ok[j] = q < n && live;
            off[j] = ids[q < n ? q : n - 1] * D + 4 * sub;
        }
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            const int64_t q = base + j * TG;
            w[j] = m[j] = v[j] = g[j] = z4;
            if (ok[j]) {
                w[j] = ld4n<(LPR >= 32)>(W + off[j]); g[j] = ld4n<(LPR >= 32)>(G + q * D + 4 * sub);
                row_moments<LPR, OPT>(T, off[j], m[j], v[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            if (!ok[j]) continue;
            // (0 + g first: the segmented apply's accumulator starts at zero -- same bits, also for g = -0)
            const float4 acc = make_float4(0.f + g[j].x, 0.f + g[j].y, 0.f + g[j].z, 0.f + g[j].w);
            const float4 wn = upd_math<OPT>(w[j], m[j], v[j], acc, 0.f, hp);
            row_store<LPR, OPT>(T, off[j], wn, m[j], v[j]);
        }
    }
}

// keys / perm of a list that is ALREADY one ascending duplicate-free run (what one requester sends an owner): nothing to sort
__global__ __launch_bounds__(kBlock) void sorted_run_keys_kernel(const int64_t* __restrict__ ids, int64_t n, uint32_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ perm) {
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (int64_t)gridDim.x * kBlock) {
        keys[q] = (uint32_t)ids[q]; perm[q] = (uint32_t)q;
    }
}

// ================================================================================================ round 6: ids without a sort (medium batches)
// At 65,536 triples the step's id work -- make_keys + nine rocPRIM launches + occurrence flags, 72 us -- was a third of the step, to find
// the few hundred duplicate occurrences of a uniform batch.  With one uint32 counter per table row (all zero between steps):
//   batch_norms_count_kernel   the EmbLoss norms pass also counts every occurrence (atomicAdd, integer: order-independent) and fills the
//                              duplicate arrays with the sentinel key
//   count_flags_kernel         per triple: a row whose counter reads 1 occurs once (the same flag byte occ_flags_kernel derives from the
//                              sorted keys); every other occurrence is appended to a list as {key, occurrence}
//   count_sort_kernel          block 0 sorts that list by (key, occurrence) -- in LDS up to 16,384 entries, in global memory beyond (slow,
//                              correct: the host binding moves a stream with that many duplicates back to the sorted path) -- and writes
//                              it out in the sorted path's layout (users at keys[0..), items at keys[B..), heads of every run); the other
//                              blocks put the counters back to zero.
// Same flags, same segments in the same occurrence order as the sorted path: the forward-and-update kernel and the segmented applies
// behind it run unchanged, on identical operands -- bit-equal tables.  (Hashing the ids into a small table instead of one counter per row
// was measured first, tools/r06/mb_atomics.hip / profiles/r06_mb_atomics.txt: 33.9 us for the insert of 196,608 keys alone.)
constexpr int64_t kCountMinB = 16448, kCountMaxB = 131072;    // (profiles/r06_mb_idpath.json: -29 % / -22 % / -9 % of the step at 32,768 / 65,536 / 131,072 uniform triples)
constexpr int kCountLds = 16384;                      // duplicate occurrences block 0 sorts in LDS (128 KB of {key, occurrence} words)

template <int LPR, bool NORMS>
__global__ __launch_bounds__(kBlock) void batch_norms_count_kernel(const float* __restrict__ U, const float* __restrict__ I, int D,
                                                                   const int64_t* __restrict__ uid, const int64_t* __restrict__ pid,
                                                                   const int64_t* __restrict__ nid, int64_t B, uint32_t* __restrict__ cu,
                                                                   uint32_t* __restrict__ ci, uint32_t* __restrict__ keysD,
                                                                   uint64_t* __restrict__ list_hdr, double* __restrict__ partials) {
    constexpr int GPB = kBlock / LPR;
    constexpr int UNR = 8;
    __shared__ double smem[2 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const bool live = sub < (D >> 2);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < 3 * B; i += (int64_t)gridDim.x * kBlock) keysD[i] = ~0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) list_hdr[0] = 0ull;          // the users' share of the duplicate list (count_flags_kernel)
    double acc[2] = {0.0, 0.0};
    for (int64_t base = gg; base < B; base += TG * UNR) {
        int64_t iu[UNR], ip[UNR], in[UNR];
        float4 u[UNR], p[UNR];
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const int64_t tc = t < B ? t : B - 1;
            iu[r] = uid[tc]; ip[r] = pid[tc]; in[r] = nid[tc];
        }
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            u[r] = p[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (NORMS && t < B && live) { u[r] = ld4(U + iu[r] * D + 4 * sub); p[r] = ld4(I + ip[r] * D + 4 * sub); }
            if (t < B && sub == 0) { atomicAdd(cu + iu[r], 1u); atomicAdd(ci + ip[r], 1u); atomicAdd(ci + in[r], 1u); }
        }
        if (NORMS) {
#pragma unroll
            for (int r = 0; r < UNR; ++r) {
                const float su = group_sum<LPR>(dot4(u[r], u[r])), sp = group_sum<LPR>(dot4(p[r], p[r]));
                if (sub == 0) { acc[0] += (double)su; acc[1] += (double)sp; }
            }
        }
    }
    if (NORMS) {
        block_sum_d<2>(acc, smem);
        if (threadIdx.x == 0) store_partials(partials, acc);
    }
}

// cnt[2] += duplicate occurrences (the list's length), cnt[3] = max(the largest counter seen): the host binding's statistics.
// list = {header: hdr[0] = the users' share of the list | 7 spare words | entries {key << 32 | occurrence}}
constexpr int kListHdr = 8;
__global__ __launch_bounds__(kBlock) void count_flags_kernel(const int64_t* __restrict__ uid, const int64_t* __restrict__ pid,
                                                             const int64_t* __restrict__ nid, int64_t B, const uint32_t* __restrict__ cu,
                                                             const uint32_t* __restrict__ ci, uint32_t key_base, uint32_t* __restrict__ flags4,
                                                             uint64_t* __restrict__ list_hdr, unsigned* __restrict__ cnt) {
    constexpr int NW = kBlock / 64;
    __shared__ unsigned wtot[NW], wbase[NW], wmax[NW], wusr[NW];
    uint64_t* __restrict__ list = list_hdr + kListHdr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < B; t0 += (int64_t)gridDim.x * kBlock) {
        const int64_t t = t0 + threadIdx.x;
        uint32_t u = 0, p = 0, n = 0, c0 = 1, c1 = 1, c2 = 1;
        if (t < B) {
            u = (uint32_t)uid[t]; p = (uint32_t)pid[t]; n = (uint32_t)nid[t];
            c0 = cu[u]; c1 = ci[p]; c2 = ci[n];
            flags4[t] = (c0 == 1u ? 1u : 0u) | (c1 == 1u ? 0x100u : 0u) | (c2 == 1u ? 0x10000u : 0u);
        }
        const unsigned mine = (c0 != 1u) + (c1 != 1u) + (c2 != 1u);
        unsigned incl = mine, mx = c0 > c1 ? (c0 > c2 ? c0 : c2) : (c1 > c2 ? c1 : c2), usr = c0 != 1u ? 1u : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned a = __shfl_up(incl, d, 64), b = __shfl_xor(mx, d, 64), c = __shfl_xor(usr, d, 64);
            if (lane >= d) incl += a;
            mx = mx > b ? mx : b;
            usr += c;
        }
        if (lane == 63) { wtot[wave] = incl; wmax[wave] = mx; wusr[wave] = usr; }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned tot = 0, m = 0, ut = 0;
            for (int w = 0; w < NW; ++w) { wbase[w] = tot; tot += wtot[w]; m = m > wmax[w] ? m : wmax[w]; ut += wusr[w]; }
            const unsigned b = tot ? atomicAdd(&cnt[2], tot) : 0u;
            for (int w = 0; w < NW; ++w) wbase[w] += b;
            if (m > 1u) atomicMax(&cnt[3], m);
            if (ut) atomicAdd((unsigned long long*)&list_hdr[0], (unsigned long long)ut);
        }
        __syncthreads();
        unsigned at = wbase[wave] + incl - mine;
        if (c0 != 1u) list[at++] = ((uint64_t)u << 32) | (uint32_t)t;
        if (c1 != 1u) list[at++] = ((uint64_t)(key_base + p) << 32) | (uint32_t)t;
        if (c2 != 1u) list[at++] = ((uint64_t)(key_base + n) << 32) | (uint32_t)(B + t);
        __syncthreads();
    }
}

// blocks [0, kRankBlocks): the duplicate list into sorted order.  Up to kCountLds entries by RANK: a block owns 64 entries, one WAVE per
// sixteenth of the list each, and counts for every entry the entries below it ((key, occurrence) words are distinct) while the whole list
// passes through LDS in tiles -- the n^2 compares spread over the chip (first cut: 256 entries per block, 1,741 entries on SEVEN CUs, 25 us;
// a one-workgroup bitonic network before that: 35 us at 2,048 entries, 250 us at 8,192); an entry with no smaller occurrence of its key
// heads its segment.  Beyond kCountLds entries block 0 alone sorts in global memory (slow, correct).
// blocks [kRankBlocks, ...): every counter this batch touched back to zero (the flags have been taken).
constexpr int kRankEPB = 64, kRankParts = 1024 / kRankEPB, kRankBlocks = kCountLds / kRankEPB, kRankTile = 2048;
__global__ __launch_bounds__(1024) void count_sort_kernel(const int64_t* __restrict__ uid, const int64_t* __restrict__ pid,
                                                          const int64_t* __restrict__ nid, int64_t B, uint32_t* __restrict__ cu,
                                                          uint32_t* __restrict__ ci, uint32_t key_base, uint64_t* __restrict__ list_hdr,
                                                          uint32_t* __restrict__ keysD, uint32_t* __restrict__ permD,
                                                          uint32_t* __restrict__ headsA, uint32_t* __restrict__ headsB,
                                                          unsigned* __restrict__ cnt) {
    if ((int)blockIdx.x >= kRankBlocks) {
        const int64_t nth = (int64_t)(gridDim.x - kRankBlocks) * 1024;
        for (int64_t t = (int64_t)(blockIdx.x - kRankBlocks) * 1024 + threadIdx.x; t < B; t += nth) { cu[uid[t]] = 0u; ci[pid[t]] = 0u; ci[nid[t]] = 0u; }
        return;
    }
    __shared__ uint64_t tile[kRankTile];
    __shared__ unsigned part_rank[kRankParts][kRankEPB], part_dup[kRankParts][kRankEPB];
    __shared__ unsigned nA_s, hA_s, hB_s;
    uint64_t* __restrict__ list = list_hdr + kListHdr;
    const unsigned nd = cnt[2];
    if (nd == 0u) return;                             // cnt[0] = cnt[1] = 0 already (coef_finish_kernel)
    if (nd <= (unsigned)kCountLds) {
        const unsigned e0 = blockIdx.x * (unsigned)kRankEPB;
        if (e0 >= nd) return;
        const unsigned le = threadIdx.x % kRankEPB, part = threadIdx.x / kRankEPB;
        const bool have = e0 + le < nd;
        const uint64_t my = have ? list[e0 + le] : ~0ull;
        const uint32_t mykey = (uint32_t)(my >> 32);
        unsigned rank = 0, dup = 0;
        for (unsigned t0 = 0; t0 < nd; t0 += kRankTile) {
            for (unsigned i = threadIdx.x; i < (unsigned)kRankTile; i += 1024) tile[i] = t0 + i < nd ? list[t0 + i] : ~0ull;
            __syncthreads();
            const unsigned jb = part * (kRankTile / kRankParts);
#pragma unroll 8
            for (unsigned j = 0; j < (unsigned)(kRankTile / kRankParts); ++j) {
                const uint64_t x = tile[jb + j];
                const bool below = x < my;
                rank += below ? 1u : 0u;
                dup |= (below && (uint32_t)(x >> 32) == mykey) ? 1u : 0u;
            }
            __syncthreads();
        }
        part_rank[part][le] = rank; part_dup[part][le] = dup;
        if (threadIdx.x == 0) { hA_s = 0u; hB_s = 0u; }
        __syncthreads();
        // heads are numbered inside the workgroup first (LDS), one reservation per list and workgroup on the global counters: a returning
        // atomic per head on ONE word serialises at ~12 ns each (870 heads: 10 us of this launch's first 27)
        unsigned r = 0, nA = 0, slot = 0;
        bool head = false, isA = false;
        if (part == 0 && have) {
            unsigned dd = 0;
#pragma unroll
            for (int q = 0; q < kRankParts; ++q) { r += part_rank[q][le]; dd |= part_dup[q][le]; }
            head = dd == 0u;
            nA = (unsigned)list_hdr[0];
            isA = r < nA;
            if (isA) { keysD[r] = mykey; permD[r] = (uint32_t)my; }
            else { keysD[B + (r - nA)] = mykey; permD[B + (r - nA)] = (uint32_t)my; }
            if (head) slot = atomicAdd(isA ? &hA_s : &hB_s, 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) { nA_s = hA_s ? atomicAdd(&cnt[0], hA_s) : 0u; part_rank[0][0] = hB_s ? atomicAdd(&cnt[1], hB_s) : 0u; }
        __syncthreads();
        if (head) {
            if (isA) headsA[nA_s + slot] = r;
            else headsB[part_rank[0][0] + slot] = r - nA;
        }
        return;
    }
    if (blockIdx.x != 0) return;
    // ---- a long list (a skewed stream the host binding has not yet moved to the sorted path): bitonic network in global memory
    unsigned P = 1024;
    while (P < nd) P <<= 1;
    uint64_t* A = list;
    for (unsigned i = nd + threadIdx.x; i < P; i += 1024) list[i] = ~0ull;
    if (threadIdx.x == 0) { hA_s = 0u; hB_s = 0u; }
    __syncthreads();
    for (unsigned k = 2; k <= P; k <<= 1) {
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned i = threadIdx.x; i < P; i += 1024) {
                const unsigned l = i ^ j;
                if (l > i) {
                    const uint64_t a = A[i], b = A[l];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { A[i] = b; A[l] = a; }
                }
            }
            __threadfence_block();
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) nA_s = (unsigned)list_hdr[0];
    __syncthreads();
    const unsigned nA = nA_s;
    for (unsigned i = threadIdx.x; i < nd; i += 1024) {
        const uint64_t e = A[i];
        const uint32_t key = (uint32_t)(e >> 32), occ = (uint32_t)e;
        const bool head = i == 0u || (uint32_t)(A[i - 1] >> 32) != key;
        if (i < nA) {
            keysD[i] = key; permD[i] = occ;
            if (head) headsA[atomicAdd(&hA_s, 1u)] = i;
        } else {
            keysD[B + (i - nA)] = key; permD[B + (i - nA)] = occ;
            if (head) headsB[atomicAdd(&hB_s, 1u)] = i - nA;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) { cnt[0] = hA_s; cnt[1] = hB_s; }
}

}  // namespace

extern "C" int cdr_bpr_fwd_grad(cdr_ctx* ctx, void* stream, const float* user_tab, const float* item_tab, int D,
                                const int64_t* uid, const int64_t* pid, const int64_t* nid, int64_t B, int64_t B_mean,
                                float gamma, float reg_weight, float* out6, float* GU, float* GP, int scatter) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && uid && pid && nid && out6 && GU && GP);
    CDR_CHECK_ARG(D > 0 && (D & 3) == 0 && D <= 256 && B > 0);
    hipStream_t s = (hipStream_t)stream;
    if (B_mean <= 0) B_mean = B;
    const float invB = 1.0f / (float)B_mean;
    const int lpr = cdr_lpr_for(D);
    const int grid = grid_for((B + kUnroll - 1) / kUnroll, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_BPR_FWD_GRAD, s);
        DISPATCH_LPR(lpr, {
            auto kern = scatter ? bpr_fwd_grad_kernel<L, true> : bpr_fwd_grad_kernel<L, false>;
            kern<<<dim3(grid), dim3(kBlock), 0, s>>>(user_tab, item_tab, D, uid, pid, nid, B, gamma, invB, GU, GP, ctx->partials);
        });
    }
    CDR_LAUNCH_CHECK();
    step_finish_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, B_mean, reg_weight, out6);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

extern "C" int cdr_point_fwd_grad(cdr_ctx* ctx, void* stream, int loss_kind, const float* user_tab, const float* item_tab, int D,
                                 const int64_t* uid, const int64_t* iid, const float* label, int64_t B, float reg_weight,
                                 float* out9, float* GU, float* GI) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && uid && iid && label && out9 && GU && GI);
    CDR_CHECK_ARG((loss_kind == CDR_LOSS_MSE || loss_kind == CDR_LOSS_BCE) && D > 0 && (D & 3) == 0 && D <= 256 && B > 0);
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(D);
    const int grid = grid_for((B + kUnroll - 1) / kUnroll, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_POINT_FWD_GRAD, s);
        DISPATCH_LPR(lpr, point_fwd_grad_kernel<L><<<dim3(grid), dim3(kBlock), 0, s>>>(loss_kind, user_tab, item_tab, D, uid, iid, label, B,
                                                                                        1.0f / (float)B, GU, GI, ctx->partials));
    }
    CDR_LAUNCH_CHECK();
    step_finish_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, B, reg_weight, out9);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

extern "C" int cdr_triplet_fwd_grad(cdr_ctx* ctx, void* stream, const float* user_tab, const float* item_tab, int D,
                                    const int64_t* uid, const int64_t* pid, const int64_t* nid, int64_t B, float margin, float eps,
                                    float* out3, float* GU, float* GI) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && uid && pid && nid && out3 && GU && GI);
    CDR_CHECK_ARG(D > 0 && (D & 3) == 0 && D <= 256 && B > 0);
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(D);
    const int grid = grid_for((B + kUnroll - 1) / kUnroll, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_TRIPLET_FWD_GRAD, s);
        DISPATCH_LPR(lpr, triplet_fwd_grad_kernel<L><<<dim3(grid), dim3(kBlock), 0, s>>>(user_tab, item_tab, D, uid, pid, nid, B, margin, eps,
                                                                                          1.0f / (float)B, GU, GI, ctx->partials));
    }
    CDR_LAUNCH_CHECK();
    triplet_finish_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, B, out3);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

extern "C" int cdr_loss_finish_sums(void* stream, const float* sums3, int64_t B_mean, float reg_weight, float* out6) {
    CDR_CHECK_ARG(sums3 && out6 && B_mean > 0);
    finish_sums_kernel<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(sums3, B_mean, reg_weight, out6);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

// rocPRIM's Onesweep with a configuration measured for this step's shape (tools/sort_tune.hip: 3,145,728 (key, index) pairs,
// 27 significant bits): 1,024-thread blocks x 8 items, 9-bit digits (27 bits = 3 passes instead of 4), wave-match ranking --
// 117 us against 161 us for the library's gfx950 default.  Used from 2^18 pairs up; smaller sorts keep the default.
using big_sort_config = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<kSortBlock, kSortItems>, rocprim::kernel_config<kSortBlock, kSortItems>, kSortRadixBits,
                                        rocprim::block_radix_rank_algorithm::match>,
    (size_t)1 << 17>;          // (the library merge-sorts up to 2^20 items: 0.167 ms for 1,048,576 pairs against 0.06 with Onesweep)
constexpr int64_t kBigSort = 1 << 18;

static inline hipError_t sort_pairs(void* tmp, size_t& tmp_bytes, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout,
                                    size_t n, unsigned bits, hipStream_t s) {
    if ((int64_t)n >= kBigSort) return rocprim::radix_sort_pairs<big_sort_config>(tmp, tmp_bytes, kin, kout, vin, vout, n, 0u, bits, s);
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, kin, kout, vin, vout, n, 0u, bits, s);
}

static inline unsigned bits_for(int64_t num_rows) {
    unsigned b = 1;
    while (b < 32 && ((int64_t)1 << b) < num_rows) ++b;
    return b;
}

// ------------------------------------------------------------------------------------------------ the id sort's own launch list
// rocprim::radix_sort_pairs at this size is 14 dependent launches of which 4 move keys: the histogram, its scan, one Onesweep pass per
// digit place -- and 7 memsets (1 for the digit counts, per pass 1 for the look-back states and 1 for the ordered block-id counter).
// From kBigSort pairs up the same device code (rocprim::detail::onesweep_histograms / onesweep_scan_histograms / onesweep_iteration with
// big_sort_config's constants, in thin kernels of ours) is launched by a host loop that is the library's radix_sort_onesweep_impl
// without the memsets: every pass has its own look-back region and its own block-id word, and everything that must start at zero is ONE
// span of the workspace that the caller's key-making kernel clears (sort_state_clear) -- stream-ordered before the first pass on every
// path, which matters: a pass spins on look-back states, so a stale state could hang it.  The result is the library's, bit for bit (a
// stable sort's output is a function of the keys alone).  This leans on rocprim::detail, so it is tied to the one rocPRIM version it was
// written against; any other version, a smaller sort, and CDR_OWN_SORT=0 (the A/B switch: tools/ab_id_sort.sh) take the public call.
#if ROCPRIM_VERSION == 400200
#define CDR_HAVE_OWN_SORT 1
namespace {

namespace rpd = rocprim::detail;
using sort_bid_t = rpd::block_id_wrapper<unsigned int, true>;    // ordered block ids (the library's choice on gfx950): what makes the look-back safe

__global__ __launch_bounds__(kSortBlock) void sort_hist_kernel(const uint32_t* keys, sort_offs_t* counts, sort_offs_t size, sort_offs_t full_blocks,
                                                               unsigned end_bit) {
    rpd::onesweep_histograms<kSortBlock, kSortItems, kSortRadixBits, false>(keys, counts, size, full_blocks, rocprim::identity_decomposer{}, 0u, end_bit);
}
__global__ __launch_bounds__(kSortBlock) void sort_scan_kernel(sort_offs_t* counts) {
    rpd::onesweep_scan_histograms<kSortBlock, kSortRadixBits>(counts);
}
__global__ __launch_bounds__(kSortBlock) void sort_pass_kernel(const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                                                               unsigned size, sort_offs_t* offs_in, sort_offs_t* offs_out,
                                                               rpd::onesweep_lookback_state* lookback, unsigned bit, unsigned cur_bits,
                                                               unsigned full_blocks, sort_bid_t bid) {
    rpd::onesweep_iteration<kSortBlock, kSortItems, kSortRadixBits, false, rocprim::block_radix_rank_algorithm::match>(
        keys_in, keys_out, vals_in, vals_out, size, offs_in, offs_out, lookback, rocprim::identity_decomposer{}, bit, cur_bits, full_blocks, bid);
}

// The own list's part of the sort workspace, behind {keys_in | vals_in}:
//   zero span A   counts[places][512] (sort_offs_t) | ticket line (32 words; word 0 = make_keys2_offsets_kernel's sign-in ticket)
//   zero span B   block-id words, one 128-byte line per pass | look-back states [places][blocks][512]
//   offs_tmp[512] | keys_tmp[n] | vals_tmp[n]                        (written before they are read: not cleared)
// A and B are contiguous.  `blocks` is the grid of every pass and sizes the look-back regions -- one place, this constructor.
struct own_sort_plan {
    unsigned blocks = 0, full_blocks = 0, places = 0;
    int64_t wordsA = 0, wordsB = 0;
    size_t o_ids = 0, o_lookback = 0, o_offs_tmp = 0, o_keys_tmp = 0, o_vals_tmp = 0, bytes = 0;
    own_sort_plan(size_t n, unsigned bits) {
        constexpr size_t per_block = (size_t)kSortBlock * kSortItems;
        blocks = (unsigned)((n + per_block - 1) / per_block);
        full_blocks = n % per_block == 0 ? blocks : blocks - 1;
        places = (bits + kSortRadixBits - 1) / kSortRadixBits;
        const size_t arr = ((n * sizeof(uint32_t)) + 255) & ~(size_t)255;
        wordsA = (int64_t)(places * kSortRadix * (sizeof(sort_offs_t) / 4) + 32);
        o_ids = (size_t)wordsA * 4;
        o_lookback = o_ids + (size_t)kSortMaxPlaces * 128;
        const size_t lb_bytes = (size_t)places * blocks * kSortRadix * sizeof(rpd::onesweep_lookback_state);
        wordsB = (int64_t)((o_lookback + lb_bytes - o_ids) / 4);
        o_offs_tmp = (o_lookback + lb_bytes + 255) & ~(size_t)255;
        o_keys_tmp = o_offs_tmp + kSortRadix * sizeof(sort_offs_t);
        o_vals_tmp = o_keys_tmp + arr;
        bytes = o_vals_tmp + arr;
    }
    sort_offs_t* counts(char* tmp) const { return (sort_offs_t*)tmp; }
    unsigned* ticket(char* tmp) const { return (unsigned*)(tmp + (size_t)wordsA * 4 - 128); }
};
static_assert(sizeof(rpd::onesweep_lookback_state) == 4 && sizeof(sort_offs_t) % 4 == 0, "the zero span is counted in 32-bit words");

// one batch of the library's loop (it cuts a sort into batches of 2^30 items; larger sorts keep the library call)
constexpr int64_t kOwnSortMax = (int64_t)1 << 30;

inline bool own_sort_on(int64_t n) {
    static const bool on = [] { const char* e = getenv("CDR_OWN_SORT"); return !(e && e[0] == '0'); }();       // A/B switch (tools/)
    return on && n >= kBigSort && n <= kOwnSortMax;
}

// histogram + scan of keys_in -> exclusive digit offsets in counts (what make_keys2_offsets_kernel does inside the key-making launch)
inline hipError_t own_sort_offsets(const own_sort_plan& P, char* tmp, const uint32_t* keys_in, size_t n, unsigned bits, hipStream_t s) {
    sort_hist_kernel<<<dim3(P.blocks), dim3(kSortBlock), 0, s>>>(keys_in, P.counts(tmp), (sort_offs_t)n, (sort_offs_t)P.full_blocks, bits);
    sort_scan_kernel<<<dim3(P.places), dim3(kSortBlock), 0, s>>>(P.counts(tmp));
    return hipGetLastError();
}

// radix_sort_onesweep_impl's pass loop: the first pass reads the input, the passes alternate between the temporaries and the output
// so that the last one lands in the output.  Needs the offsets in counts and zero span B cleared.
inline hipError_t own_sort_passes(const own_sort_plan& P, char* tmp, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in,
                                  uint32_t* vals_out, size_t n, unsigned bits, hipStream_t s) {
    uint32_t* keys_tmp = (uint32_t*)(tmp + P.o_keys_tmp);
    uint32_t* vals_tmp = (uint32_t*)(tmp + P.o_vals_tmp);
    auto* lookback = (rpd::onesweep_lookback_state*)(tmp + P.o_lookback);
    bool to_output = (P.places - 1) % 2 == 0, from_input = true;
    unsigned place = 0;
    for (unsigned bit = 0; bit < bits; bit += kSortRadixBits, ++place) {
        const uint32_t* ki = from_input ? keys_in : (to_output ? keys_tmp : keys_out);
        const uint32_t* vi = from_input ? vals_in : (to_output ? vals_tmp : vals_out);
        const unsigned cur_bits = bits - bit < kSortRadixBits ? bits - bit : kSortRadixBits;
        sort_pass_kernel<<<dim3(P.blocks), dim3(kSortBlock), 0, s>>>(
            ki, to_output ? keys_out : keys_tmp, vi, to_output ? vals_out : vals_tmp, (unsigned)n, P.counts(tmp) + (size_t)place * kSortRadix,
            (sort_offs_t*)(tmp + P.o_offs_tmp), lookback + (size_t)place * P.blocks * kSortRadix, bit, cur_bits, P.full_blocks,
            sort_bid_t::create(tmp + P.o_ids + (size_t)place * 128));
        from_input = false;
        to_output = !to_output;
    }
    return hipGetLastError();
}

}  // namespace
#else
#define CDR_HAVE_OWN_SORT 0
#endif

// ------------------------------------------------------------------------------------------------ what the host entry points share
namespace {

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// A step's index buffer `heads` = {cnt[4] | headsA[n_a / 2 + 1] | headsB[n_b / 2 + 1]}: the two duplicate-segment head lists of
// occ_flags_kernel (a list of n occurrences has at most n / 2 segments of two and more) behind their lengths cnt[0], cnt[1].
struct heads_view {
    unsigned* cnt; uint32_t* headsA; uint32_t* headsB;
    heads_view(uint32_t* heads, int64_t n_a) : cnt((unsigned*)heads), headsA(heads + 4), headsB(headsA + (n_a / 2 + 1)) {}
    static int64_t words(int64_t n_a, int64_t n_b) { return 4 + (n_a / 2 + 1) + (n_b / 2 + 1); }
};

// The count path's duplicate list (cdr_ctx_set_id_counters): kListHdr header words + the 3 B occurrences rounded up to a power of two.
inline size_t count_list_bytes(int64_t B) {
    int64_t P = 1024;
    while (P < 3 * B) P <<= 1;
    return (size_t)(P + kListHdr) * sizeof(uint64_t);
}

// Keys of a two-table sort: table A's rows as they are, table B's rows with bit hb set (key_base = 1 << hb; hb + 1 key bits in all).
inline unsigned two_table_bits(int64_t rows_a, int64_t rows_b) {
    const unsigned a = bits_for(rows_a), b = bits_for(rows_b);
    return a > b ? a : b;
}

apply_hp make_hp(int opt, float lr, float beta1, float beta2, float eps, float wd, int64_t step) {
    float step_size = lr, bc2_sqrt = 1.f;
    if (opt == 1) {
        cdr_adam_hp((double)step, lr, beta1, beta2, step_size, bc2_sqrt);       // (bc2_sqrt carries cdr_adam_hp's bc2: cdr_adam_math.h)
    }
    return apply_hp{lr, beta1, beta2, eps, wd, step_size, bc2_sqrt};
}

// Long-segment scratch of one segmented apply over n occurrences (empty when no segment can be longer than kLongSeg):
//   counters[4] (256 bytes) | seg_long[long_cap] | seg_piece[piece_cap] | int pcnt[piece_cap] | float partial[piece_cap][D]
struct long_scratch {
    int64_t long_cap = 0, piece_cap = 0;
    size_t o_long = 0, o_piece = 0, o_cnt = 0, o_part = 0, bytes = 0;          // bytes: up to the end of partial, not rounded up
    long_scratch() = default;
    long_scratch(int64_t n, int D) {
        if (n <= kLongSeg) return;
        long_cap = n / (kLongSeg + 1) + 1;
        piece_cap = n / kPiece + long_cap + 1;
        o_long = 256; o_piece = o_long + up256(sizeof(seg_long) * long_cap); o_cnt = o_piece + up256(sizeof(seg_piece) * piece_cap);
        o_part = o_cnt + up256(sizeof(int) * piece_cap); bytes = o_part + sizeof(float) * (size_t)piece_cap * D;
    }
    void bind(char* base, dup_side& t) const {
        t.counters = (unsigned*)base; t.longs = (seg_long*)(base + o_long); t.pieces = (seg_piece*)(base + o_piece);
        t.pcnt = (int*)(base + o_cnt); t.partial = (float*)(base + o_part);
    }
};

}  // namespace

extern "C" int cdr_sort_workspace_bytes(int64_t n, int64_t num_rows, size_t* bytes) {
    CDR_CHECK_ARG(bytes && n > 0 && num_rows > 0 && num_rows <= (int64_t)0xFFFFFFFFu && n <= (int64_t)0x7FFFFFFF);
    size_t tmp = 0;
    hipError_t e = sort_pairs(nullptr, tmp, nullptr, nullptr, nullptr, nullptr, (size_t)n, bits_for(num_rows), (hipStream_t)0);
    if (e != hipSuccess) { cdr_set_error("cdr_sort_workspace_bytes: %s", hipGetErrorString(e)); return (int)e; }
#if CDR_HAVE_OWN_SORT
    if (n >= kBigSort && n <= kOwnSortMax) {             // either list works on the same region (whatever CDR_OWN_SORT says: one size per shape)
        const size_t own = own_sort_plan((size_t)n, bits_for(num_rows)).bytes;
        if (own > tmp) tmp = own;
    }
#endif
    *bytes = up256(tmp) + 2 * up256((size_t)n * sizeof(uint32_t));
    return CDR_OK;
}

// What a key-making launch clears beside making keys (sort_state_clear; p = nullptr: nothing).
struct sort_clear { uint32_t* p; int64_t words; };

// What every id sort shares: the workspace {keys_in[n] | vals_in[n] | the sort's temporary} (cdr_sort_workspace_bytes), the caller's
// key-making launch -- make_keys(keys_in, vals_in, z), which also clears z -- and the radix sort over the bits of `key_space`, in one
// CDR_TAG_SORT bracket: the own launch list from kBigSort pairs up, else the library call.
// keys_make_offsets: the caller's key-making launch leaves the digit offsets too whenever it is handed a span to clear (z.p != nullptr:
// zero span B; the caller has cleared span A on the stream before, see own_sort_span_a) -- no histogram and scan launches then.
template <class MakeKeys>
static int sort_ids_with(cdr_ctx* ctx, hipStream_t s, int64_t n, int64_t key_space, uint32_t* keys_sorted, uint32_t* perm, void* ws,
                         size_t ws_bytes, MakeKeys&& make_keys, bool keys_make_offsets = false) {
    size_t need = 0;
    int rc = cdr_sort_workspace_bytes(n, key_space, &need);
    if (rc) return rc;
    CDR_CHECK_ARG(ws_bytes >= need);
    const size_t arr = up256((size_t)n * sizeof(uint32_t));
    uint32_t* keys_in = (uint32_t*)ws;
    uint32_t* vals_in = (uint32_t*)((char*)ws + arr);
    char* tmp = (char*)ws + 2 * arr;
    size_t tmp_bytes = ws_bytes - 2 * arr;
    const unsigned bits = bits_for(key_space);
    cdr_time_scope ts(ctx, CDR_TAG_SORT, s);
#if CDR_HAVE_OWN_SORT
    if (own_sort_on(n)) {
        CDR_CHECK_ARG(((uintptr_t)tmp & 127) == 0);
        const own_sort_plan P((size_t)n, bits);
        if (keys_make_offsets) {
            make_keys(keys_in, vals_in, sort_clear{(uint32_t*)(tmp + P.o_ids), P.wordsB});
            CDR_LAUNCH_CHECK();
        } else {
            make_keys(keys_in, vals_in, sort_clear{(uint32_t*)tmp, P.wordsA + P.wordsB});
            CDR_LAUNCH_CHECK();
            CDR_HIP(own_sort_offsets(P, tmp, keys_in, (size_t)n, bits, s));
        }
        CDR_HIP(own_sort_passes(P, tmp, keys_in, keys_sorted, vals_in, perm, (size_t)n, bits, s));
        return CDR_OK;
    }
#endif
    make_keys(keys_in, vals_in, sort_clear{nullptr, 0});
    CDR_LAUNCH_CHECK();
    CDR_HIP(sort_pairs(tmp, tmp_bytes, keys_in, keys_sorted, vals_in, perm, (size_t)n, bits, s));
    return CDR_OK;
}

#if CDR_HAVE_OWN_SORT
// Zero span A (digit counts + ticket) of the sort that sort_ids_with will run on this workspace with keys_make_offsets, for the caller's
// earlier launch to clear; words = 0 when that sort takes the library call or the workspace is too small (sort_ids_with refuses it).
static sort_clear own_sort_span_a(int64_t n, int64_t key_space, void* ws, size_t ws_bytes) {
    size_t need = 0;
    if (!own_sort_on(n) || cdr_sort_workspace_bytes(n, key_space, &need) != CDR_OK || ws_bytes < need) return {nullptr, 0};
    return {(uint32_t*)((char*)ws + 2 * up256((size_t)n * sizeof(uint32_t))), own_sort_plan((size_t)n, bits_for(key_space)).wordsA};
}
#else
static sort_clear own_sort_span_a(int64_t, int64_t, void*, size_t) { return {nullptr, 0}; }
#endif

extern "C" int cdr_sort_ids(cdr_ctx* ctx, void* stream, const int64_t* ids0, int64_t n0, const int64_t* ids1, int64_t n1,
                            int64_t num_rows, uint32_t* keys_sorted, uint32_t* perm, void* workspace,
                            size_t workspace_bytes) {
    const int64_t n = n0 + n1;
    CDR_CHECK_ARG(ids0 && n0 > 0 && (n1 == 0 || ids1) && keys_sorted && perm && workspace);
    hipStream_t s = (hipStream_t)stream;
    return sort_ids_with(ctx, s, n, num_rows, keys_sorted, perm, workspace, workspace_bytes, [&](uint32_t* keys_in, uint32_t* vals_in, sort_clear z) {
        make_keys_kernel<<<dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s>>>(ids0, n0, ids1, n1, keys_in, vals_in, z.p, z.words);
    });
}

// key_base of a two-table sort (two_table_bits); 0: the key space does not fit
static inline uint32_t two_table_key_base(int64_t rows_a, int64_t rows_b) {
    const unsigned hb = two_table_bits(rows_a, rows_b);
    return hb < 31 ? 1u << hb : 0u;
}

// span_a: zero span A of this very sort (own_sort_span_a with the same n, key space and workspace), ALREADY CLEARED by an earlier launch
// on the stream -- the key-making launch then leaves the digit offsets itself (make_keys2_offsets_kernel); {nullptr, 0}: it does not.
static int sort_two_tables(cdr_ctx* ctx, void* stream, const int64_t* ids_a, int64_t n_a, int64_t rows_a, const int64_t* ids_b0,
                           int64_t n_b0, const int64_t* ids_b1, int64_t n_b1, int64_t rows_b, uint32_t* keys_sorted, uint32_t* perm,
                           uint32_t* key_base_out, void* workspace, size_t workspace_bytes, sort_clear span_a) {
    const int64_t n = n_a + n_b0 + n_b1;
    CDR_CHECK_ARG(ids_a && n_a > 0 && ids_b0 && n_b0 > 0 && (n_b1 == 0 || ids_b1) && keys_sorted && perm && key_base_out && workspace);
    CDR_CHECK_ARG(rows_a > 0 && rows_b > 0);
    const uint32_t key_base = two_table_key_base(rows_a, rows_b);
    CDR_CHECK_ARG(key_base != 0u);
    hipStream_t s = (hipStream_t)stream;
    int rc = sort_ids_with(ctx, s, n, (int64_t)key_base * 2, keys_sorted, perm, workspace, workspace_bytes, [&](uint32_t* keys_in, uint32_t* vals_in, sort_clear z) {
        if (span_a.p && z.p) {
            const unsigned places = (bits_for((int64_t)key_base * 2) + kSortRadixBits - 1) / kSortRadixBits;
            // (8 keys per thread as rocPRIM's histogram launch: a few hundred blocks keep the global atomics of the flush few)
            const unsigned kgrid = (unsigned)((n + (int64_t)kSortBlock * kSortItems - 1) / ((int64_t)kSortBlock * kSortItems));
            make_keys2_offsets_kernel<<<dim3(kgrid), dim3(kSortBlock), 0, s>>>(ids_a, n_a, ids_b0, n_b0, ids_b1, n_b1, key_base, keys_in, vals_in, z.p, z.words,
                                                                               (sort_offs_t*)span_a.p, (unsigned*)span_a.p + span_a.words - 32, places);
        } else {
            make_keys2_kernel<<<dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s>>>(ids_a, n_a, ids_b0, n_b0, ids_b1, n_b1, key_base, keys_in, vals_in, z.p, z.words);
        }
    }, span_a.p != nullptr);
    if (rc) return rc;
    *key_base_out = key_base;
    return CDR_OK;
}

extern "C" int cdr_sort_ids_two_tables(cdr_ctx* ctx, void* stream, const int64_t* ids_a, int64_t n_a, int64_t rows_a,
                                       const int64_t* ids_b0, int64_t n_b0, const int64_t* ids_b1, int64_t n_b1, int64_t rows_b,
                                       uint32_t* keys_sorted, uint32_t* perm, uint32_t* key_base_out, void* workspace,
                                       size_t workspace_bytes) {
    return sort_two_tables(ctx, stream, ids_a, n_a, rows_a, ids_b0, n_b0, ids_b1, n_b1, rows_b, keys_sorted, perm, key_base_out, workspace,
                           workspace_bytes, sort_clear{nullptr, 0});
}

extern "C" int cdr_rowwise_apply(cdr_ctx* ctx, void* stream, int opt, float* table, float* exp_avg, float* exp_avg_sq, int D,
                                 const uint32_t* keys_sorted, const uint32_t* perm, int64_t n, const float* G,
                                 int64_t neg_start, int64_t reg_limit, const float* reg_coef, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int64_t step, const int64_t* occ_ids, uint32_t key_base) {
    CDR_CHECK_ARG(table && keys_sorted && perm && G && n > 0);
    CDR_CHECK_ARG(D > 0 && (D & 3) == 0);
    CDR_CHECK_ARG(opt == 0 || (opt == 1 && exp_avg && exp_avg_sq && step > 0) || (opt == CDR_OPT_ADAGRAD && !exp_avg && exp_avg_sq));
    hipStream_t s = (hipStream_t)stream;
    // keys of a two-table sort carry the table bit: instead of subtracting it per row in the kernels, the three table
    // pointers are moved back by key_base rows here (row r of the table is then addressed as key = key_base + r)
    if (key_base) {
        table -= (int64_t)key_base * D;
        if (exp_avg) exp_avg -= (int64_t)key_base * D;
        if (exp_avg_sq) exp_avg_sq -= (int64_t)key_base * D;
    }
    const int lpr = cdr_lpr_for(D);
    const int grid = grid_for(n, kBlock / lpr);
    const bool is_signed = neg_start < n;
    const apply_hp hp = make_hp(opt, lr, beta1, beta2, eps, weight_decay, step);
    const long_scratch ls(n, D);
    dup_side sc{};                                          // (only its five scratch members are used here)
    if (ls.bytes) {
        CDR_CHECK_ARG(ctx != nullptr);
        void* base = nullptr;
        int rc = cdr_ctx_scratch(ctx, ls.bytes, &base);
        if (rc != CDR_OK) return rc;
        ls.bind((char*)base, sc);
        CDR_HIP(cdr_zero_u32(sc.counters, 4, s));
    }
    cdr_time_scope ts(ctx, is_signed ? CDR_TAG_APPLY_SIGNED : CDR_TAG_APPLY_UNSIGNED, s);
    DISPATCH_LPR_OPT3(lpr, opt, {
        auto kern = is_signed ? rowwise_apply_kernel<L, O, true> : rowwise_apply_kernel<L, O, false>;
        kern<<<dim3(grid), dim3(kBlock), 0, s>>>(table, exp_avg, exp_avg_sq, D, keys_sorted, perm, n, G, neg_start, reg_limit, reg_coef, hp, occ_ids,
                                                 sc.counters, sc.longs, sc.pieces);
    });
    CDR_LAUNCH_CHECK();
    if (ls.bytes) {
        // sized for the worst case, but a launch whose counters read 0 retires in a few microseconds
        const int gp = (int)(ls.piece_cap < 2048 ? ls.piece_cap : 2048);          // one workgroup per piece (looping past 2,048)
        DISPATCH_LPR(lpr, {
            auto kern = is_signed ? seg_piece_sum_kernel<L, true> : seg_piece_sum_kernel<L, false>;
            kern<<<dim3(gp), dim3(kBlock), 0, s>>>(D, perm, G, neg_start, reg_limit, occ_ids, sc.counters, sc.pieces, sc.partial, sc.pcnt);
        });
        CDR_LAUNCH_CHECK();
        const int gl = grid_for(ls.long_cap < 4096 ? ls.long_cap : 4096, kBlock / lpr);
        DISPATCH_LPR_OPT3(lpr, opt, seg_long_finish_kernel<L, O><<<dim3(gl), dim3(kBlock), 0, s>>>(table, exp_avg, exp_avg_sq, D, keys_sorted, reg_coef, hp, sc.counters,
                                                                                                 sc.longs, sc.partial, sc.pcnt));
        CDR_LAUNCH_CHECK();
    }
    return CDR_OK;
}

// ------------------------------------------------------------------------------------------------ the fused step's skeleton
namespace {

// The two tables of a step with the optimizer scalars of their updates (a table that is only read: opt_item = 0, no moments).
struct step_tables { tab_ptrs TU, TI; apply_hp hu, hi; };
step_tables make_tables(int opt_user, float* user_tab, float* user_m, float* user_v, int64_t step_user, int opt_item, float* item_tab,
                        float* item_m, float* item_v, int64_t step_item, float lr, float beta1, float beta2, float eps, float wd) {
    return {{user_tab, user_m, user_v}, {item_tab, item_m, item_v}, make_hp(opt_user, lr, beta1, beta2, eps, wd, step_user),
            make_hp(opt_item, lr, beta1, beta2, eps, wd, step_item)};
}

// Stage 1, EmbLoss head: the squared norms of the n_rows gathered (user, item) rows -> coefficients in out9[4], out9[5].  Without
// regularisation the norms launch is skipped (ngrid = 0 says so to coef_finish_kernel).  The finishing block also clears the head
// lists' counters `cnt` and `zspan` (zero span A of the id sort behind it: own_sort_span_a) and, when given, advances the
// device-resident update counts (their Adam scalars -> hp_dev).
int embloss_head(cdr_ctx* ctx, hipStream_t s, const float* user_tab, const float* item_tab, int D, const int64_t* uid, const int64_t* pid,
                 int64_t n_rows, int64_t B, int kmul, float reg_weight, float* out9, unsigned* cnt, int64_t* step_user_dev = nullptr,
                 int64_t* step_item_dev = nullptr, float* hp_dev = nullptr, float lr = 0.f, float beta1 = 0.f, float beta2 = 0.f,
                 const float* user_n2 = nullptr, const float* item_n2 = nullptr, sort_clear zspan = {nullptr, 0}) {
    int ngrid = 0;
    if (reg_weight != 0.f) {
        const int lpr = cdr_lpr_for(D);
        ngrid = grid_for((n_rows + 7) / 8, kBlock / lpr);
        cdr_time_scope ts(ctx, CDR_TAG_BATCH_NORMS, s);
        if (user_n2 && item_n2) {                   // the tables' squared-norm records: one float per row instead of the row
            DISPATCH_LPR(lpr, batch_norms_cached_kernel<L><<<dim3(ngrid), dim3(kBlock), 0, s>>>(user_n2, item_n2, uid, pid, n_rows, ctx->partials));
        } else {
            DISPATCH_LPR(lpr, batch_norms_kernel<L><<<dim3(ngrid), dim3(kBlock), 0, s>>>(user_tab, item_tab, D, uid, pid, n_rows, ctx->partials));
        }
        CDR_LAUNCH_CHECK();
    }
    coef_finish_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, ngrid, B, ngrid ? reg_weight : 0.f, out9, kmul, step_user_dev, step_item_dev, hp_dev,
                                                        lr, beta1, beta2, cnt, nullptr, zspan.p, (int)zspan.words);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

// Stage 2 behind the sort: per-occurrence "only occurrence of its row" flags and the duplicate segments' heads of the sorted list
// [n_a keys of table A | n - n_a keys of table B].
int occ_flags(cdr_ctx* ctx, hipStream_t s, const uint32_t* keys, const uint32_t* perm, int64_t n_a, int64_t n, int fstride, uint8_t* flags,
              const heads_view& hv, bool stat = false) {
    cdr_time_scope ts(ctx, CDR_TAG_OCC_FLAGS, s);
    occ_flags_kernel<<<dim3(grid_for(n, kBlock * kFlagIT)), dim3(kBlock), 0, s>>>(keys, perm, n_a, n, fstride, flags, hv.headsA, hv.headsB, hv.cnt, stat);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

// Stage 5, both tables' duplicate-row applies: one scratch request carved for the two sides, three launches with blockIdx.y = side
// instead of six (+ two counter clears, which the step's one-block finishing kernel does: finish_and_apply_dups).
struct dup_host { tab_ptrs T; const uint32_t* keys; const uint32_t* perm; int64_t n; const uint32_t* heads; const unsigned* nheads;
                  const float* G; int64_t neg_start, reg_limit; const float* reg_coef; apply_hp hp; uint32_t key_base;
                  float* out = nullptr; const uint32_t* uidx = nullptr; float* n2 = nullptr; };
struct dups_plan { dup_side side[2]; long_scratch ls[2]; };

// The sides of a step on the sorted list [n_user user keys | n_item item keys]: users over GU with every occurrence positive and
// regularised, items over GI with occurrences from neg_start_item on subtracted and those below reg_limit_item regularised.
void make_sides(dup_host (&sides)[2], const step_tables& T, const uint32_t* keys, const uint32_t* perm, const heads_view& hv, const float* GU,
                const float* GI, int64_t n_user, int64_t n_item, int64_t neg_start_item, int64_t reg_limit_item, const float* coef_user,
                const float* coef_item, uint32_t key_base) {
    sides[0] = {T.TU, keys, perm, n_user, hv.headsA, hv.cnt, GU, n_user, n_user, coef_user, T.hu, 0};
    sides[1] = {T.TI, keys + n_user, perm + n_user, n_item, hv.headsB, hv.cnt + 1, GI, neg_start_item, reg_limit_item, coef_item, T.hi, key_base};
}

int dups_plan_make(cdr_ctx* ctx, int D, const dup_host (&h)[2], dups_plan& pl) {
    size_t off[2], total = 0;
    for (int i = 0; i < 2; ++i) {
        pl.ls[i] = long_scratch(h[i].n, D);
        off[i] = total;
        total += up256(pl.ls[i].bytes);
    }
    char* base = nullptr;
    if (total) {
        void* b = nullptr;
        int rc = cdr_ctx_scratch(ctx, total, &b);
        if (rc != CDR_OK) return rc;
        base = (char*)b;
    }
    for (int i = 0; i < 2; ++i) {
        dup_side& t = pl.side[i];
        const int64_t kb = (int64_t)h[i].key_base * D;
        t.W = h[i].T.W - kb; t.M = h[i].T.M ? h[i].T.M - kb : nullptr; t.V = h[i].T.V ? h[i].T.V - kb : nullptr;
        t.keys = h[i].keys; t.perm = h[i].perm; t.n = h[i].n; t.heads = h[i].heads; t.nheads = h[i].nheads; t.G = h[i].G;
        t.neg_start = h[i].neg_start; t.reg_limit = h[i].reg_limit; t.reg_coef = h[i].reg_coef; t.hp = h[i].hp;
        t.counters = nullptr; t.longs = nullptr; t.pieces = nullptr; t.pcnt = nullptr; t.partial = nullptr;
        t.out = h[i].out; t.uidx = h[i].uidx;
        t.n2 = h[i].n2 ? h[i].n2 - (int64_t)h[i].key_base * kNormRecFloats : nullptr;
        if (pl.ls[i].bytes) pl.ls[i].bind(base + off[i], t);
    }
    return CDR_OK;
}

// The two kernel pairs of apply_dups_pair: both sides update their table (every one-GPU step), or side 1 sums its segments into the
// send buffer dup_side::out (the row-sharded step).
// (adagrad: the pair also exists for OPT = 2 -- the one-GPU steps whose entries accept CDR_OPT_ADAGRAD)
struct table_dups {
    static constexpr bool adagrad = true;
    template <int L, int OPT> static constexpr auto dups = rowwise_apply_dups2_kernel<L, OPT>;
    template <int L, int OPT> static constexpr auto long_finish = seg_long_finish2_kernel<L, OPT>;
};
struct table_dups_nc {                          // ... and keep the tables' squared-norm records current (dup_side::n2)
    static constexpr bool adagrad = true;
    template <int L, int OPT> static constexpr auto dups = rowwise_apply_dups2_kernel<L, OPT, true>;
    template <int L, int OPT> static constexpr auto long_finish = seg_long_finish2_kernel<L, OPT, true>;
};
struct shard_dups {
    static constexpr bool adagrad = false;
    template <int L, int OPT> static constexpr auto dups = shard_dups_kernel<L, OPT>;
    template <int L, int OPT> static constexpr auto long_finish = shard_long_finish_kernel<L, OPT>;
};

template <class K>
int apply_dups_pair(cdr_ctx* ctx, hipStream_t s, int opt, int D, const dups_plan& pl) {
    const int lpr = cdr_lpr_for(D);
    const int64_t nmax = pl.side[0].n > pl.side[1].n ? pl.side[0].n : pl.side[1].n;     // (row shard: the item side's 2 Bl)
    const int grid = grid_for(nmax / 16 + 1, kBlock / lpr);          // four segments per lane group and round (apply_dups)
    {
        cdr_time_scope ts(ctx, CDR_TAG_APPLY_SIGNED, s);
        if constexpr (K::adagrad) DISPATCH_LPR_OPT3(lpr, opt, K::template dups<L, O><<<dim3(grid, 2), dim3(kBlock), 0, s>>>(D, pl.side[0], pl.side[1]));
        else DISPATCH_LPR_OPT(lpr, opt, K::template dups<L, O><<<dim3(grid, 2), dim3(kBlock), 0, s>>>(D, pl.side[0], pl.side[1]));
    }
    CDR_LAUNCH_CHECK();
    if (pl.ls[0].long_cap || pl.ls[1].long_cap) {
        const int64_t pc = pl.ls[0].piece_cap > pl.ls[1].piece_cap ? pl.ls[0].piece_cap : pl.ls[1].piece_cap;
        const int64_t lc = pl.ls[0].long_cap > pl.ls[1].long_cap ? pl.ls[0].long_cap : pl.ls[1].long_cap;
        const int gp = (int)(pc < 2048 ? pc : 2048);                        // one workgroup per piece (looping past 2,048)
        DISPATCH_LPR(lpr, seg_piece_sum2_kernel<L><<<dim3(gp, 2), dim3(kBlock), 0, s>>>(D, pl.side[0], pl.side[1]));
        CDR_LAUNCH_CHECK();
        const int gl = grid_for(lc < 4096 ? lc : 4096, kBlock / lpr);
        if constexpr (K::adagrad) DISPATCH_LPR_OPT3(lpr, opt, K::template long_finish<L, O><<<dim3(gl, 2), dim3(kBlock), 0, s>>>(D, pl.side[0], pl.side[1]));
        else DISPATCH_LPR_OPT(lpr, opt, K::template long_finish<L, O><<<dim3(gl, 2), dim3(kBlock), 0, s>>>(D, pl.side[0], pl.side[1]));
        CDR_LAUNCH_CHECK();
    }
    return CDR_OK;
}

// The tail of every step: plan the two sides' scratch, let the step's one-block finishing kernel run -- finish(counters of side 0,
// counters of side 1) launches it; it writes the loss vector and clears the long-segment counters given -- then the applies.
template <class K = table_dups, class Finish>
int finish_and_apply_dups(cdr_ctx* ctx, hipStream_t s, int opt, int D, const dup_host (&sides)[2], Finish&& finish) {
    dups_plan pl;
    int rc = dups_plan_make(ctx, D, sides, pl);
    if (rc) return rc;
    finish(pl.side[0].counters, pl.side[1].counters);
    CDR_LAUNCH_CHECK();
    return apply_dups_pair<K>(ctx, s, opt, D, pl);
}

}  // namespace

extern "C" int cdr_bpr_step_fused_heads_words(int64_t B, int64_t* words) {
    CDR_CHECK_ARG(words && B > 0);
    *words = heads_view::words(B, 2 * B);          // heads of the user list | heads of the item list [pid | nid]
    return CDR_OK;
}

static int bpr_step_fused_impl(cdr_ctx* ctx, void* stream, int opt, float* user_tab, float* user_m, float* user_v, int64_t user_rows,
                               float* item_tab, float* item_m, float* item_v, int64_t item_rows, int D, const int64_t* uid,
                               const int64_t* pid, const int64_t* nid, int64_t B, float gamma, float reg_weight, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int64_t step_user, int64_t step_item,
                               int64_t* step_user_dev, int64_t* step_item_dev, float* hp_dev,
                               float* out9, float* GU, float* GP, uint32_t* keys, uint32_t* perm, uint8_t* flags, uint32_t* heads,
                               void* sort_ws, size_t sort_ws_bytes) {
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(D);
    const heads_view hv(heads, B);                     // (cnt[0..3] are cleared by coef_finish_kernel)
    uint32_t key_base = 0;
    int rc;
    // ---- ids without a sort (medium batches, counters handed over by cdr_ctx_set_id_counters): see "round 6: ids without a sort"
    const bool count_path = ctx->idc_user && ctx->idc_item && ctx->idc_user_rows == user_rows && ctx->idc_item_rows == item_rows &&
                            B >= kCountMinB && B <= kCountMaxB && ctx->idc_list_bytes >= count_list_bytes(B);
    // ---- the tables' squared-norm records (cdr_ctx_set_norm_cache), sorted path only: read by the EmbLoss head, kept current by the writers
    const bool cached = !count_path && ctx->n2_user && ctx->n2_item && ctx->n2_user_rows == user_rows && ctx->n2_item_rows == item_rows;
    float* NU = cached ? ctx->n2_user : nullptr;
    float* NI = cached ? ctx->n2_item : nullptr;
    if (count_path) {
        const unsigned hb = two_table_bits(user_rows, item_rows);
        CDR_CHECK_ARG(hb < 31);
        key_base = 1u << hb;
        const int ngrid = grid_for((B + 7) / 8, kBlock / lpr);
        {
            cdr_time_scope ts(ctx, CDR_TAG_BATCH_NORMS, s);
            DISPATCH_LPR(lpr, {
                auto kern = reg_weight != 0.f ? batch_norms_count_kernel<L, true> : batch_norms_count_kernel<L, false>;
                kern<<<dim3(ngrid), dim3(kBlock), 0, s>>>(user_tab, item_tab, D, uid, pid, nid, B, ctx->idc_user, ctx->idc_item, keys, (uint64_t*)ctx->idc_list, ctx->partials);
            });
        }
        CDR_LAUNCH_CHECK();
        coef_finish_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, reg_weight != 0.f ? ngrid : 0, B, reg_weight, out9, 1, step_user_dev, step_item_dev, hp_dev,
                                                            lr, beta1, beta2, hv.cnt);
        CDR_LAUNCH_CHECK();
        {
            cdr_time_scope ts(ctx, CDR_TAG_OCC_FLAGS, s);
            count_flags_kernel<<<dim3(grid_for(B, kBlock)), dim3(kBlock), 0, s>>>(uid, pid, nid, B, ctx->idc_user, ctx->idc_item, key_base, (uint32_t*)flags,
                                                                                 (uint64_t*)ctx->idc_list, hv.cnt);
            CDR_LAUNCH_CHECK();
            count_sort_kernel<<<dim3(kRankBlocks + 128), dim3(1024), 0, s>>>(uid, pid, nid, B, ctx->idc_user, ctx->idc_item, key_base,
                                                                                            (uint64_t*)ctx->idc_list, keys, perm, hv.headsA, hv.headsB, hv.cnt);
        }
        CDR_LAUNCH_CHECK();
    } else {
        // ---- EmbLoss coefficients first (they do not need the sort): out9[4], out9[5]  (+ the device-resident update counts, when given)
        // (its finishing block also clears the digit counts and the ticket of the sort behind it, whose key-making launch then leaves
        // the digit offsets itself: one id sort = key making + one launch per digit place.  CDR_OWN_SORT=1: the A/B arm without this.)
        static const bool keys_make_offsets = [] { const char* e = getenv("CDR_OWN_SORT"); return !(e && e[0] == '1'); }();
        const uint32_t kb = two_table_key_base(user_rows, item_rows);
        const sort_clear span_a = keys_make_offsets && kb ? own_sort_span_a(3 * B, (int64_t)kb * 2, sort_ws, sort_ws_bytes) : sort_clear{nullptr, 0};
        rc = embloss_head(ctx, s, user_tab, item_tab, D, uid, pid, B, B, 1, reg_weight, out9, hv.cnt, step_user_dev, step_item_dev, hp_dev, lr, beta1, beta2,
                          NU, NI, span_a);
        if (rc) return rc;
        rc = sort_two_tables(ctx, stream, uid, B, user_rows, pid, B, nid, B, item_rows, keys, perm, &key_base, sort_ws, sort_ws_bytes, span_a);
        if (rc) return rc;
        rc = occ_flags(ctx, s, keys, perm, B, 3 * B, 4, flags, hv, B <= kCountMaxB);
        if (rc) return rc;
    }
    step_tables T = make_tables(opt, user_tab, user_m, user_v, step_user, opt, item_tab, item_m, item_v, step_item, lr, beta1, beta2, eps, weight_decay);
    if (hp_dev && opt == 1) { T.hu.dev = hp_dev; T.hi.dev = hp_dev + 2; }          // the scalars coef_finish_kernel left on the device
    static const int un = [] { const char* e = getenv("CDR_FWD_APPLY_UN"); return (e && e[0] == '2') ? 2 : 1; }();   // A/B switch (tools/)
    const int grid = grid_for((B + un - 1) / un, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_BPR_FWD_APPLY, s);
        DISPATCH_LPR_OPT3(lpr, opt, {
            constexpr int U2 = O == 1 ? 2 : 1;              // (the two-triple form exists for Adam only)
            auto kern = cached ? (un == 2 ? bpr_fwd_apply_kernel<L, O, U2, false, false, true> : bpr_fwd_apply_kernel<L, O, 1, false, false, true>)
                               : (un == 2 ? bpr_fwd_apply_kernel<L, O, U2> : bpr_fwd_apply_kernel<L, O, 1>);
            kern<<<dim3(grid), dim3(kBlock), 0, s>>>(T.TU, T.TI, D, uid, pid, nid, (const uint32_t*)flags, B, gamma, 1.0f / (float)B, out9 + 4, T.hu, T.hi, GU, GP,
                                                     ctx->partials, nullptr, nullptr, NU, NI);
        });
    }
    CDR_LAUNCH_CHECK();
    dup_host sides[2];
    make_sides(sides, T, keys, perm, hv, GU, GP, B, 2 * B, B, B, out9 + 4, out9 + 5, key_base);
    sides[0].n2 = NU; sides[1].n2 = NI;
    auto finish = [&](unsigned* za, unsigned* zb) {
        step_finish_keep_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, B, reg_weight, out9, za, zb);
    };
    return cached ? finish_and_apply_dups<table_dups_nc>(ctx, s, opt, D, sides, finish) : finish_and_apply_dups(ctx, s, opt, D, sides, finish);
}

extern "C" int cdr_norm_rec_floats(void) { return kNormRecFloats; }

// One streaming pass over a table: n2[r * cdr_norm_rec_floats()] = ||table[r]||^2 (the rest of the record 0), formed exactly as the fused
// BPR step's norm gather forms it.  n2: [rows, cdr_norm_rec_floats()] floats, aligned to the record size.
extern "C" int cdr_row_norms_build(void* stream, const float* table, int64_t rows, int D, float* n2) {
    CDR_CHECK_ARG(table && n2 && rows > 0 && D > 0 && (D & 3) == 0 && D <= 256);
    CDR_CHECK_ARG((uintptr_t)n2 % (kNormRecFloats * sizeof(float)) == 0);
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(D);
    const int grid = grid_for((rows + kUnroll - 1) / kUnroll, kBlock / lpr);
    DISPATCH_LPR(lpr, row_norms_build_kernel<L><<<dim3(grid), dim3(kBlock), 0, s>>>(table, rows, D, n2));
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

extern "C" int cdr_id_count_workspace_bytes(int64_t B, size_t* bytes) {
    CDR_CHECK_ARG(bytes && B > 0 && 3 * B <= (int64_t)0x7FFFFFFF);
    *bytes = count_list_bytes(B);
    return CDR_OK;
}

extern "C" int cdr_bpr_step_fused(cdr_ctx* ctx, void* stream, int opt, float* user_tab, float* user_m, float* user_v, int64_t user_rows,
                                  float* item_tab, float* item_m, float* item_v, int64_t item_rows, int D, const int64_t* uid,
                                  const int64_t* pid, const int64_t* nid, int64_t B, float gamma, float reg_weight, float lr,
                                  float beta1, float beta2, float eps, float weight_decay, int64_t step_user, int64_t step_item,
                                  float* out9, float* GU, float* GP, uint32_t* keys, uint32_t* perm, uint8_t* flags, uint32_t* heads,
                                  void* sort_ws, size_t sort_ws_bytes) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && uid && pid && nid && out9 && GU && GP && keys && perm && flags && heads && sort_ws);
    CDR_CHECK_ARG(D > 0 && (D & 3) == 0 && D <= 256 && B > 0 && 3 * B <= (int64_t)0x7FFFFFFF);
    CDR_CHECK_ARG(opt == 0 || (opt == 1 && user_m && user_v && item_m && item_v && step_user > 0 && step_item > 0) ||
                  (opt == CDR_OPT_ADAGRAD && !user_m && user_v && !item_m && item_v));       // Adagrad: the sums in user_v / item_v, no steps
    CDR_CHECK_ARG(((uintptr_t)flags & 3) == 0);
    return bpr_step_fused_impl(ctx, stream, opt, user_tab, user_m, user_v, user_rows, item_tab, item_m, item_v, item_rows, D, uid, pid, nid, B, gamma,
                               reg_weight, lr, beta1, beta2, eps, weight_decay, step_user, step_item, nullptr, nullptr, nullptr, out9, GU, GP,
                               keys, perm, flags, heads, sort_ws, sort_ws_bytes);
}

// The same step with the tables' update counts in DEVICE memory (int64 each, advanced by the call's first finishing block) and the Adam
// scalars derived from them on the device (hp_dev: 4 floats of scratch owned by the caller): nothing about the update number is baked
// into the launches, so the call can be captured in a hipGraph and replayed.
extern "C" int cdr_bpr_step_fused_dev(cdr_ctx* ctx, void* stream, int opt, float* user_tab, float* user_m, float* user_v, int64_t user_rows,
                                      float* item_tab, float* item_m, float* item_v, int64_t item_rows, int D, const int64_t* uid,
                                      const int64_t* pid, const int64_t* nid, int64_t B, float gamma, float reg_weight, float lr,
                                      float beta1, float beta2, float eps, float weight_decay, int64_t* step_user_dev, int64_t* step_item_dev,
                                      float* hp_dev, float* out9, float* GU, float* GP, uint32_t* keys, uint32_t* perm, uint8_t* flags,
                                      uint32_t* heads, void* sort_ws, size_t sort_ws_bytes) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && uid && pid && nid && out9 && GU && GP && keys && perm && flags && heads && sort_ws);
    CDR_CHECK_ARG(D > 0 && (D & 3) == 0 && D <= 256 && B > 0 && 3 * B <= (int64_t)0x7FFFFFFF);
    CDR_CHECK_ARG(opt == 1 && user_m && user_v && item_m && item_v && step_user_dev && step_item_dev && hp_dev);
    CDR_CHECK_ARG(((uintptr_t)flags & 3) == 0);
    return bpr_step_fused_impl(ctx, stream, opt, user_tab, user_m, user_v, user_rows, item_tab, item_m, item_v, item_rows, D, uid, pid, nid, B, gamma,
                               reg_weight, lr, beta1, beta2, eps, weight_decay, 1, 1, step_user_dev, step_item_dev, hp_dev, out9, GU, GP,
                               keys, perm, flags, heads, sort_ws, sort_ws_bytes);
}


// ---- round 5: the pointwise step (EMCDR-MF / CMF rows: emcdr.py:111-122, cmf.py:75-99) as ONE call on the forward-and-update pass ---------
// Same structure as cdr_bpr_step_fused with two rows per batch row: EmbLoss norms of (U[uid], I[iid]) -> coefficients, ONE sort of both
// id lists + occurrence flags, point_fwd_apply_kernel (rows occurring once updated in place), segmented applies over the duplicate rows.
// Buffers as cdr_bpr_step_fused's with B = the number of (user, item, label) rows: keys / perm [2 B], flags [4 B], heads
// cdr_bpr_step_fused_heads_words(B) words, GU / GI [B, D], sort workspace cdr_sort_workspace_bytes(2 B, ...).
extern "C" int cdr_point_step_fused(cdr_ctx* ctx, void* stream, int loss_kind, int opt, float* user_tab, float* user_m, float* user_v,
                                    int64_t user_rows, float* item_tab, float* item_m, float* item_v, int64_t item_rows, int D,
                                    const int64_t* uid, const int64_t* iid, const float* label, int64_t B, float reg_weight, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, int64_t step_user, int64_t step_item,
                                    float* out9, float* GU, float* GI, uint32_t* keys, uint32_t* perm, uint8_t* flags, uint32_t* heads,
                                    void* sort_ws, size_t sort_ws_bytes) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && uid && iid && label && out9 && GU && GI && keys && perm && flags && heads && sort_ws);
    CDR_CHECK_ARG((loss_kind == CDR_LOSS_MSE || loss_kind == CDR_LOSS_BCE) && D > 0 && (D & 3) == 0 && D <= 256 && B > 0 && 2 * B <= (int64_t)0x7FFFFFFF);
    CDR_CHECK_ARG(opt == 0 || (opt == 1 && user_m && user_v && item_m && item_v && step_user > 0 && step_item > 0) ||
                  (opt == CDR_OPT_ADAGRAD && !user_m && user_v && !item_m && item_v));       // Adagrad: the sums in user_v / item_v, no steps
    CDR_CHECK_ARG(((uintptr_t)flags & 3) == 0);
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(D);
    const heads_view hv(heads, B);
    int rc = embloss_head(ctx, s, user_tab, item_tab, D, uid, iid, B, B, 1, reg_weight, out9, hv.cnt);
    if (rc) return rc;
    uint32_t key_base = 0;
    rc = cdr_sort_ids_two_tables(ctx, stream, uid, B, user_rows, iid, B, nullptr, 0, item_rows, keys, perm, &key_base, sort_ws, sort_ws_bytes);
    if (rc) return rc;
    rc = occ_flags(ctx, s, keys, perm, B, 2 * B, 4, flags, hv);
    if (rc) return rc;
    const step_tables T = make_tables(opt, user_tab, user_m, user_v, step_user, opt, item_tab, item_m, item_v, step_item, lr, beta1, beta2, eps, weight_decay);
    const int grid = grid_for(B, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_POINT_FWD_GRAD, s);
        DISPATCH_LPR_OPT3(lpr, opt, point_fwd_apply_kernel<L, O><<<dim3(grid), dim3(kBlock), 0, s>>>(loss_kind, T.TU, T.TI, D, uid, iid, label, (const uint32_t*)flags, B,
                                                                                                   1.0f / (float)B, out9 + 4, T.hu, T.hi, GU, GI, ctx->partials));
    }
    CDR_LAUNCH_CHECK();
    dup_host sides[2];
    make_sides(sides, T, keys, perm, hv, GU, GI, B, B, B, B, out9 + 4, out9 + 5, key_base);
    return finish_and_apply_dups(ctx, s, opt, D, sides, [&](unsigned* za, unsigned* zb) {
        step_finish_keep_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, B, reg_weight, out9, za, zb);
    });
}

// The pointwise step per POSITIVE: uid [S] (the first S entries of recbole's tiled user column), iid [S + S k] = [positives | k-major
// negatives], label [S + S k].  Sizes from cdr_bpr_step_fused_kmajor_sizes(S, k); GU [S, D], GI [S + S k, D]; keys / perm [2 S + S k].
extern "C" int cdr_point_step_fused_kmajor(cdr_ctx* ctx, void* stream, int loss_kind, int opt, float* user_tab, float* user_m, float* user_v,
                                           int64_t user_rows, float* item_tab, float* item_m, float* item_v, int64_t item_rows, int D,
                                           const int64_t* uid, const int64_t* iid, const float* label, int64_t S, int k, float reg_weight,
                                           float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step_user,
                                           int64_t step_item, float* out12, float* GU, float* GI, uint32_t* keys, uint32_t* perm,
                                           uint8_t* flags, uint32_t* heads, void* sort_ws, size_t sort_ws_bytes) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && uid && iid && label && out12 && GU && GI && keys && perm && flags && heads && sort_ws);
    CDR_CHECK_ARG((loss_kind == CDR_LOSS_MSE || loss_kind == CDR_LOSS_BCE) && D > 0 && (D & 3) == 0 && D <= 256 && S > 0 && k >= 1 && k <= 64);
    const int64_t nI = S + S * (int64_t)k, B = nI;
    CDR_CHECK_ARG(S + nI <= (int64_t)0x7FFFFFFF);
    CDR_CHECK_ARG(opt == 0 || (opt == 1 && user_m && user_v && item_m && item_v && step_user > 0 && step_item > 0));
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(D);
    const int fstride = (2 + k + 3) & ~3;
    const heads_view hv(heads, S);
    const int ngrid = reg_weight != 0.f ? grid_for(S, kBlock / lpr) : 0;
    if (reg_weight != 0.f) {
        cdr_time_scope ts(ctx, CDR_TAG_BATCH_NORMS, s);
        DISPATCH_LPR(lpr, point_norms_kmajor_kernel<L><<<dim3(ngrid), dim3(kBlock), 0, s>>>(user_tab, item_tab, D, uid, iid, S, k, ctx->partials));
        CDR_LAUNCH_CHECK();
    }
    point_coef_kmajor_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, ngrid, B, k, reg_weight, out12, hv.cnt);
    CDR_LAUNCH_CHECK();
    uint32_t key_base = 0;
    int rc = cdr_sort_ids_two_tables(ctx, stream, uid, S, user_rows, iid, S, iid + S, S * (int64_t)k, item_rows, keys, perm, &key_base, sort_ws, sort_ws_bytes);
    if (rc) return rc;
    rc = occ_flags(ctx, s, keys, perm, S, S + nI, fstride, flags, hv);
    if (rc) return rc;
    const step_tables T = make_tables(opt, user_tab, user_m, user_v, step_user, opt, item_tab, item_m, item_v, step_item, lr, beta1, beta2, eps, weight_decay);
    const int grid = grid_for(S, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_POINT_FWD_GRAD, s);
        DISPATCH_LPR_OPT(lpr, opt, {
            constexpr int KW = O == 1 ? 3 : 2;              // item rows per round: 2; 3 for Adam when there is more than one negative
            auto kern = k <= 1 ? point_fwd_apply_kmajor_kernel<L, O, 2> : point_fwd_apply_kmajor_kernel<L, O, KW>;
            kern<<<dim3(grid), dim3(kBlock), 0, s>>>(loss_kind, T.TU, T.TI, D, uid, iid, label, flags, fstride, S, k, 1.0f / (float)B, out12 + 4, T.hu, T.hi, GU, GI,
                                                     ctx->partials);
        });
    }
    CDR_LAUNCH_CHECK();
    // duplicate rows: users over GU [S, D] with (1 + k) c_u per list occurrence (out12[9]); items over GI [S + S k, D], every occurrence
    // with c_i (reg_limit = the whole list)
    dup_host sides[2];
    make_sides(sides, T, keys, perm, hv, GU, GI, S, nI, nI, nI, out12 + 9, out12 + 5, key_base);
    return finish_and_apply_dups(ctx, s, opt, D, sides, [&](unsigned* za, unsigned* zb) {
        step_finish_keep_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, B, reg_weight, out12, za, zb);
    });
}

// ---- round 5: the fused single-occurrence update inside the two multi-GPU layouts -----------------------------------
// DIMENSION shard (cdr_dimshard.hip): the step is cut in two around the all-reduce of the partial scores.
//   cdr_bpr_step_presort    needs only the ids -> runs under the all-reduce: two-table sort + occurrence flags + duplicate-segment heads
//   cdr_bpr_step_from_diff  behind the all-reduce: EmbLoss coefficients from the all-reduced norms (diff[B], diff[B+1]), then ONE pass that
//                           re-gathers the column slices, forms g_t from the GIVEN score diff[t], updates every row that occurs once in
//                           place and writes gradient rows only for duplicate rows; the duplicate segments are applied as in the one-GPU step.
extern "C" int cdr_bpr_step_presort(cdr_ctx* ctx, void* stream, const int64_t* uid, const int64_t* pid, const int64_t* nid, int64_t B,
                                    int64_t user_rows, int64_t item_rows, uint32_t* keys, uint32_t* perm, uint8_t* flags, uint32_t* heads,
                                    void* sort_ws, size_t sort_ws_bytes, uint32_t* key_base_out) {
    CDR_CHECK_ARG(ctx && uid && pid && nid && keys && perm && flags && heads && sort_ws && key_base_out && B > 0 && 3 * B <= (int64_t)0x7FFFFFFF);
    CDR_CHECK_ARG(((uintptr_t)flags & 3) == 0);
    hipStream_t s = (hipStream_t)stream;
    int rc = cdr_sort_ids_two_tables(ctx, stream, uid, B, user_rows, pid, B, nid, B, item_rows, keys, perm, key_base_out, sort_ws, sort_ws_bytes);
    if (rc) return rc;
    CDR_HIP(cdr_zero_u32(heads, 4, s));                     // the two head lists' counters
    return occ_flags(ctx, s, keys, perm, B, 3 * B, 4, flags, heads_view(heads, B));
}

extern "C" int cdr_bpr_step_from_diff(cdr_ctx* ctx, void* stream, int opt, float* user_tab, float* user_m, float* user_v, float* item_tab,
                                      float* item_m, float* item_v, int Ds, const int64_t* uid, const int64_t* pid, const int64_t* nid,
                                      int64_t B, float gamma, float reg_weight, float lr, float beta1, float beta2, float eps,
                                      float weight_decay, int64_t step_user, int64_t step_item, const float* diff, uint32_t key_base,
                                      float* out9, float* GU, float* GP, const uint32_t* keys, const uint32_t* perm, const uint8_t* flags,
                                      uint32_t* heads) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && uid && pid && nid && diff && out9 && GU && GP && keys && perm && flags && heads);
    CDR_CHECK_ARG(Ds > 0 && (Ds & 3) == 0 && Ds <= 256 && B > 0 && 3 * B <= (int64_t)0x7FFFFFFF);
    CDR_CHECK_ARG(opt == 0 || (opt == 1 && user_m && user_v && item_m && item_v && step_user > 0 && step_item > 0));
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(Ds);
    coef_finish_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, 0, B, reg_weight, out9, 1, nullptr, nullptr, nullptr, 0.f, 0.f, 0.f, nullptr, diff + B);
    CDR_LAUNCH_CHECK();
    const step_tables T = make_tables(opt, user_tab, user_m, user_v, step_user, opt, item_tab, item_m, item_v, step_item, lr, beta1, beta2, eps, weight_decay);
    const int grid = grid_for(B, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_BPR_FWD_APPLY, s);
        DISPATCH_LPR_OPT(lpr, opt, bpr_fwd_apply_kernel<L, O, 1, true><<<dim3(grid), dim3(kBlock), 0, s>>>(T.TU, T.TI, Ds, uid, pid, nid, (const uint32_t*)flags, B, gamma,
                                                                                                          1.0f / (float)B, out9 + 4, T.hu, T.hi, GU, GP, ctx->partials, diff));
    }
    CDR_LAUNCH_CHECK();
    dup_host sides[2];
    make_sides(sides, T, keys, perm, heads_view(heads, B), GU, GP, B, 2 * B, B, B, out9 + 4, out9 + 5, key_base);
    return finish_and_apply_dups(ctx, s, opt, Ds, sides, [&](unsigned* za, unsigned* zb) {
        step_finish_keep_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, B, reg_weight, out9, za, zb, diff + B);
    });
}

// The pointwise rows of the dimension layout (cdr_point_partial_dot -> all-reduce -> here), same cut as the BPR pair above:
//   cdr_point_step_presort   ids only (under the all-reduce): two-table sort of uid / iid + occurrence flags + duplicate-segment heads
//   cdr_point_step_from_dot  dot [B + 2] = all-reduced {<u, i> ..., sum u^2, sum i^2}
extern "C" int cdr_point_step_presort(cdr_ctx* ctx, void* stream, const int64_t* uid, const int64_t* iid, int64_t B, int64_t user_rows,
                                      int64_t item_rows, uint32_t* keys, uint32_t* perm, uint8_t* flags, uint32_t* heads, void* sort_ws,
                                      size_t sort_ws_bytes, uint32_t* key_base_out) {
    CDR_CHECK_ARG(ctx && uid && iid && keys && perm && flags && heads && sort_ws && key_base_out && B > 0 && 2 * B <= (int64_t)0x7FFFFFFF);
    CDR_CHECK_ARG(((uintptr_t)flags & 3) == 0);
    hipStream_t s = (hipStream_t)stream;
    int rc = cdr_sort_ids_two_tables(ctx, stream, uid, B, user_rows, iid, B, nullptr, 0, item_rows, keys, perm, key_base_out, sort_ws, sort_ws_bytes);
    if (rc) return rc;
    CDR_HIP(cdr_zero_u32(heads, 4, s));
    return occ_flags(ctx, s, keys, perm, B, 2 * B, 4, flags, heads_view(heads, B));
}

extern "C" int cdr_point_step_from_dot(cdr_ctx* ctx, void* stream, int loss_kind, int opt, float* user_tab, float* user_m, float* user_v,
                                       float* item_tab, float* item_m, float* item_v, int Ds, const int64_t* uid, const int64_t* iid,
                                       const float* label, int64_t B, float reg_weight, float lr, float beta1, float beta2, float eps,
                                       float weight_decay, int64_t step_user, int64_t step_item, const float* dot, uint32_t key_base,
                                       float* out9, float* GU, float* GI, const uint32_t* keys, const uint32_t* perm, const uint8_t* flags,
                                       uint32_t* heads) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && uid && iid && label && dot && out9 && GU && GI && keys && perm && flags && heads);
    CDR_CHECK_ARG((loss_kind == CDR_LOSS_MSE || loss_kind == CDR_LOSS_BCE) && Ds > 0 && (Ds & 3) == 0 && Ds <= 256 && B > 0);
    CDR_CHECK_ARG(opt == 0 || (opt == 1 && user_m && user_v && item_m && item_v && step_user > 0 && step_item > 0));
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(Ds);
    coef_finish_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, 0, B, reg_weight, out9, 1, nullptr, nullptr, nullptr, 0.f, 0.f, 0.f, nullptr, dot + B);
    CDR_LAUNCH_CHECK();
    const step_tables T = make_tables(opt, user_tab, user_m, user_v, step_user, opt, item_tab, item_m, item_v, step_item, lr, beta1, beta2, eps, weight_decay);
    const int grid = grid_for(B, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_POINT_FWD_GRAD, s);
        DISPATCH_LPR_OPT(lpr, opt, point_fwd_apply_kernel<L, O, true><<<dim3(grid), dim3(kBlock), 0, s>>>(loss_kind, T.TU, T.TI, Ds, uid, iid, label, (const uint32_t*)flags, B,
                                                                                                         1.0f / (float)B, out9 + 4, T.hu, T.hi, GU, GI, ctx->partials, dot));
    }
    CDR_LAUNCH_CHECK();
    dup_host sides[2];
    make_sides(sides, T, keys, perm, heads_view(heads, B), GU, GI, B, B, B, B, out9 + 4, out9 + 5, key_base);
    return finish_and_apply_dups(ctx, s, opt, Ds, sides, [&](unsigned* za, unsigned* zb) {
        step_finish_keep_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, B, reg_weight, out9, za, zb, dot + B);
    });
}

// ROW shard (shard.ShardedBPRStep): after user-aligned routing the user rows of a rank's triples are its own, the item rows arrive in a
// compact buffer (`irows`, one row per distinct item, indexed by ip / in).
//   cdr_batch_norm_sums       sums3 = {0, sum ||U[u]||^2, sum ||irows[ip]||^2} of the rank's triples -> all-reduced by the caller (the EmbLoss
//                             coefficients need the GLOBAL norms before any row is updated) -> cdr_loss_finish_sums leaves them in out9[4..5]
//   cdr_bpr_shard_local_step  sort of the local user rows + flags, then the one-GPU forward-and-update kernel with the item "table" = irows
//                             and no item row ever flagged: user rows that occur once are updated in place, duplicate user rows go through
//                             GU and the segmented apply, GP[t] = g_t u_t for EVERY triple (summed per distinct item and sent home by the
//                             caller: cdr_segsum_rows).  out9[6..8] = this rank's {loss sum, sum u^2, sum p^2}; out9[4..5] untouched.
extern "C" int cdr_batch_norm_sums(cdr_ctx* ctx, void* stream, const float* user_tab, const float* item_rows, int D, const int64_t* uid,
                                   const int64_t* pid, int64_t B, float* sums3) {
    CDR_CHECK_ARG(ctx && user_tab && item_rows && uid && pid && sums3 && D > 0 && (D & 3) == 0 && D <= 256 && B > 0);
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(D);
    const int ngrid = grid_for((B + 7) / 8, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_BATCH_NORMS, s);
        DISPATCH_LPR(lpr, batch_norms_kernel<L><<<dim3(ngrid), dim3(kBlock), 0, s>>>(user_tab, item_rows, D, uid, pid, B, ctx->partials));
    }
    CDR_LAUNCH_CHECK();
    norm_sums_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, ngrid, sums3);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

extern "C" int cdr_bpr_shard_local_step(cdr_ctx* ctx, void* stream, int opt, float* user_tab, float* user_m, float* user_v, int64_t user_rows,
                                        const float* irows, int D, const int64_t* u_loc, const int64_t* ip, const int64_t* in, int64_t Bl,
                                        int64_t B_global, float gamma, float reg_weight, float lr, float beta1, float beta2, float eps,
                                        float weight_decay, int64_t step_user, float* out9, float* GU, float* GP, uint32_t* keys,
                                        uint32_t* perm, uint8_t* flags, uint32_t* heads, void* sort_ws, size_t sort_ws_bytes) {
    CDR_CHECK_ARG(ctx && user_tab && irows && u_loc && ip && in && out9 && GU && GP && keys && perm && flags && heads && sort_ws);
    CDR_CHECK_ARG(D > 0 && (D & 3) == 0 && D <= 256 && Bl > 0 && Bl <= (int64_t)0x7FFFFFFF && B_global >= Bl);
    CDR_CHECK_ARG(opt == 0 || (opt == 1 && user_m && user_v && step_user > 0));
    CDR_CHECK_ARG(((uintptr_t)flags & 3) == 0);
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(D);
    int rc = cdr_sort_ids(ctx, stream, u_loc, Bl, nullptr, 0, user_rows, keys, perm, sort_ws, sort_ws_bytes);
    if (rc) return rc;
    CDR_HIP(cdr_zero_u32(heads, 4, s));
    const heads_view hv(heads, Bl);                                 // (headsB stays empty: no item row is ever updated here)
    rc = occ_flags(ctx, s, keys, perm, Bl, Bl, 4, flags, hv);
    if (rc) return rc;
    // (the item side's scalars are never used: the p / n flag bytes stay 0)
    const step_tables T = make_tables(opt, user_tab, user_m, user_v, step_user, 0, const_cast<float*>(irows), nullptr, nullptr, 1, lr, beta1, beta2, eps, weight_decay);
    const int grid = grid_for(Bl, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_BPR_FWD_APPLY, s);
        DISPATCH_LPR_OPT(lpr, opt, bpr_fwd_apply_kernel<L, O, 1><<<dim3(grid), dim3(kBlock), 0, s>>>(T.TU, T.TI, D, u_loc, ip, in, (const uint32_t*)flags, Bl, gamma,
                                                                                                    1.0f / (float)B_global, out9 + 4, T.hu, T.hi, GU, GP, ctx->partials));
    }
    CDR_LAUNCH_CHECK();
    dup_host sides[2];
    make_sides(sides, T, keys, perm, hv, GU, GP, Bl, 0, 0, 0, out9 + 4, out9 + 5, 0);
    sides[1].keys = keys; sides[1].perm = perm;                     // an empty item side: it names the start of the (user-only) list
    return finish_and_apply_dups(ctx, s, opt, D, sides, [&](unsigned* za, unsigned*) {
        shard_sums_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, out9, za);
    });
}

// ---- round 6: the row-sharded step on its own passes --------------------------------------------------------------
//   cdr_bpr_shard_plan   ONE sort for both lists of a rank's routed triples (user rows | item keys grouped by owner) -> occurrence flags of
//                        both (user occurs once -> updated in place; item occurs once -> its gradient row goes straight into its send
//                        slot), the duplicate segments' heads, and the request list: distinct item rows per owner, occurrence -> slot map.
//   cdr_shard_norm_sums  EmbLoss norm sums from the local user rows and the owners' per-row squared norms.
//   cdr_bpr_shard_step   the forward-and-update pass (SH): user rows as in the one-GPU step; gradient rows of single item occurrences written
//                        once, into GS; GP only where a duplicate needs it; then ONE launch for the duplicate user rows (update) and the
//                        duplicate item segments (sum -> GS).
namespace {
struct shard_bits { unsigned lb, hb; uint32_t key_base; };
static int shard_key_bits(int64_t user_rows, int64_t item_local_rows, int world, shard_bits& kb) {
    if (user_rows <= 0 || item_local_rows <= 0 || world < 1 || world > 1024) return CDR_EINVAL;
    kb.lb = bits_for(item_local_rows);
    const unsigned ob = world > 1 ? bits_for(world) : 0u;
    const unsigned ub = bits_for(user_rows);
    kb.hb = ub > kb.lb + ob ? ub : kb.lb + ob;
    if (kb.hb >= 31) return CDR_EINVAL;
    kb.key_base = 1u << kb.hb;
    return CDR_OK;
}
}  // namespace

// the request list's scan reuses the sort's workspace: {excl[2 Bl] | rocPRIM's temporary}
static int shard_scan_bytes(int64_t Bl, size_t* bytes) {
    size_t tmp = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, tmp, rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint32_t>(0u), head_flag_op{nullptr}),
                                           (uint32_t*)nullptr, 0u, (size_t)(2 * Bl), rocprim::plus<uint32_t>());
    if (e != hipSuccess) { cdr_set_error("cdr_bpr_shard_plan_sizes: %s", hipGetErrorString(e)); return (int)e; }
    *bytes = up256((size_t)(2 * Bl) * sizeof(uint32_t)) + up256(tmp);
    return CDR_OK;
}

extern "C" int cdr_bpr_shard_plan_sizes(int64_t Bl, int64_t user_rows, int64_t item_local_rows, int world, int64_t* heads_words,
                                        size_t* ws_bytes) {
    CDR_CHECK_ARG(heads_words && ws_bytes && Bl > 0 && 3 * Bl <= (int64_t)0x7FFFFFFF);
    shard_bits kb;
    CDR_CHECK_ARG(shard_key_bits(user_rows, item_local_rows, world, kb) == CDR_OK);
    *heads_words = heads_view::words(Bl, 2 * Bl);
    size_t sort_need = 0, scan_need = 0;
    int rc = cdr_sort_workspace_bytes(3 * Bl, (int64_t)kb.key_base * 2, &sort_need);
    if (rc) return rc;
    rc = shard_scan_bytes(Bl, &scan_need);
    if (rc) return rc;
    *ws_bytes = sort_need > scan_need ? sort_need : scan_need;
    return CDR_OK;
}

extern "C" int cdr_bpr_shard_plan(cdr_ctx* ctx, void* stream, const int64_t* recv3, int64_t Bl, int64_t user_rows, int64_t item_local_rows,
                                  int world, int64_t* u_loc, uint32_t* keys, uint32_t* perm, uint8_t* flags, uint32_t* heads,
                                  uint32_t* uidx, int64_t* uniq_local, int64_t* umap, int64_t* counts, int64_t* n_uniq, void* ws,
                                  size_t ws_bytes) {
    CDR_CHECK_ARG(ctx && recv3 && u_loc && keys && perm && flags && heads && uidx && uniq_local && umap && counts && n_uniq && ws);
    CDR_CHECK_ARG(Bl > 0 && 3 * Bl <= (int64_t)0x7FFFFFFF && ((uintptr_t)flags & 3) == 0);
    shard_bits kb;
    CDR_CHECK_ARG(shard_key_bits(user_rows, item_local_rows, world, kb) == CDR_OK);
    size_t scan_need = 0;
    int rc = shard_scan_bytes(Bl, &scan_need);
    if (rc) return rc;
    CDR_CHECK_ARG(ws_bytes >= scan_need);                   // (sort_ids_with checks the sort's own need)
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = 3 * Bl;
    const heads_view hv(heads, Bl);
    rc = sort_ids_with(ctx, s, n, (int64_t)kb.key_base * 2, keys, perm, ws, ws_bytes, [&](uint32_t* keys_in, uint32_t* vals_in, sort_clear z) {
        shard_keys_kernel<<<dim3(grid_for(Bl, kBlock)), dim3(kBlock), 0, s>>>(recv3, Bl, (uint32_t)world, kb.lb, kb.key_base, u_loc, keys_in, vals_in, hv.cnt,
                                                                             z.p, z.words);
    });
    if (rc) return rc;
    rc = occ_flags(ctx, s, keys, perm, Bl, n, 4, flags, hv);
    if (rc) return rc;
    // the request list from section B (the sort's inputs are dead: the scan reuses the workspace)
    const int64_t nB = 2 * Bl;
    const uint32_t* keysB = keys + Bl;
    const size_t arrB = up256((size_t)nB * sizeof(uint32_t));
    uint32_t* excl = (uint32_t*)ws;
    void* stmp = (char*)ws + arrB;
    size_t stmp_bytes = ws_bytes - arrB;
    CDR_HIP(rocprim::exclusive_scan(stmp, stmp_bytes, rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint32_t>(0u), head_flag_op{keysB}),
                                    excl, 0u, (size_t)nB, rocprim::plus<uint32_t>(), s));
    shard_emit_kernel<<<dim3(grid_for(nB, kBlock)), dim3(kBlock), 0, s>>>(keysB, perm + Bl, excl, nB, world, kb.lb, kb.key_base, uidx, uniq_local, umap,
                                                                          counts, n_uniq);
    CDR_LAUNCH_CHECK();
    shard_counts_kernel<<<dim3(1), dim3(64), 0, s>>>(counts, world);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

extern "C" int cdr_shard_norm_sums(cdr_ctx* ctx, void* stream, const float* user_tab, int D, const int64_t* u_loc, const float* nrm2,
                                   const int64_t* ip, int64_t Bl, float* sums3) {
    CDR_CHECK_ARG(ctx && user_tab && u_loc && nrm2 && ip && sums3 && D > 0 && (D & 3) == 0 && D <= 256 && Bl > 0);
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(D);
    const int ngrid = grid_for((Bl + 7) / 8, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_BATCH_NORMS, s);
        DISPATCH_LPR(lpr, shard_norms_kernel<L><<<dim3(ngrid), dim3(kBlock), 0, s>>>(user_tab, D, u_loc, nrm2, ip, Bl, ctx->partials));
    }
    CDR_LAUNCH_CHECK();
    norm_sums_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, ngrid, sums3);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

extern "C" int cdr_bpr_shard_step(cdr_ctx* ctx, void* stream, int opt, float* user_tab, float* user_m, float* user_v, const float* irows, int D,
                                  const int64_t* u_loc, const int64_t* umap, int64_t Bl, int64_t B_global, float gamma, float reg_weight,
                                  float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step_user, float* out9, float* GU,
                                  float* GP, float* GS, const uint32_t* keys, const uint32_t* perm, const uint8_t* flags, uint32_t* heads,
                                  const uint32_t* uidx) {
    CDR_CHECK_ARG(ctx && user_tab && irows && u_loc && umap && out9 && GU && GP && GS && keys && perm && flags && heads && uidx);
    CDR_CHECK_ARG(D > 0 && (D & 3) == 0 && D <= 256 && Bl > 0 && 3 * Bl <= (int64_t)0x7FFFFFFF && B_global >= Bl);
    CDR_CHECK_ARG(opt == 0 || (opt == 1 && user_m && user_v && step_user > 0));
    CDR_CHECK_ARG(((uintptr_t)flags & 3) == 0);
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(D);
    // (no item row is updated on this side)
    const step_tables T = make_tables(opt, user_tab, user_m, user_v, step_user, 0, const_cast<float*>(irows), nullptr, nullptr, 1, lr, beta1, beta2, eps, weight_decay);
    const int grid = grid_for(Bl, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_BPR_FWD_APPLY, s);
        DISPATCH_LPR_OPT(lpr, opt, bpr_fwd_apply_kernel<L, O, 1, false, true><<<dim3(grid), dim3(kBlock), 0, s>>>(
                                       T.TU, T.TI, D, u_loc, umap, umap + Bl, (const uint32_t*)flags, Bl, gamma, 1.0f / (float)B_global, out9 + 4, T.hu, T.hi, GU, GP,
                                       ctx->partials, nullptr, GS));
    }
    CDR_LAUNCH_CHECK();
    dup_host sides[2];
    make_sides(sides, T, keys, perm, heads_view(heads, Bl), GU, GP, Bl, 2 * Bl, Bl, Bl, out9 + 4, out9 + 5, 0);
    sides[1].out = GS; sides[1].uidx = uidx;
    return finish_and_apply_dups<shard_dups>(ctx, s, opt, D, sides, [&](unsigned* za, unsigned* zb) {
        shard_sums2_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, out9, za, zb);
    });
}

// The owner's side: ids = `runs` ascending duplicate-free runs of local rows (one per requesting rank, in rank order), grads one summed
// gradient row per id (EmbLoss term inside).  One run needs no sort: the list IS the sorted segment list; several runs are radix-sorted
// as everywhere (stable: rows asked for by several ranks are summed in rank order).
extern "C" int cdr_shard_owner_apply(cdr_ctx* ctx, void* stream, int opt, float* table, float* exp_avg, float* exp_avg_sq, int64_t table_rows,
                                     int D, const int64_t* ids, int64_t n, int runs, const float* grads, float lr, float beta1, float beta2,
                                     float eps, float weight_decay, int64_t step, uint32_t* keys, uint32_t* perm, void* ws, size_t ws_bytes) {
    CDR_CHECK_ARG(ctx && table && ids && grads && keys && perm && n > 0 && runs >= 1 && table_rows > 0);
    hipStream_t s = (hipStream_t)stream;
    if (runs == 1 && D <= 256 && getenv("CDR_OWNER_RUN_GENERIC") == nullptr) {
        CDR_CHECK_ARG(D > 0 && (D & 3) == 0 && (opt == 0 || (opt == 1 && exp_avg && exp_avg_sq && step > 0)));
        const apply_hp hp = make_hp(opt, lr, beta1, beta2, eps, weight_decay, step);
        const int lpr = cdr_lpr_for(D);
        cdr_time_scope ts(ctx, CDR_TAG_APPLY_UNSIGNED, s);
        DISPATCH_LPR_OPT(lpr, opt, apply_run_kernel<L, O><<<dim3(grid_for((n + 1) / 2, kBlock / lpr)), dim3(kBlock), 0, s>>>(table, exp_avg, exp_avg_sq, D, ids, n, grads, hp));
        CDR_LAUNCH_CHECK();
        return CDR_OK;
    }
    if (runs == 1) {
        sorted_run_keys_kernel<<<dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s>>>(ids, n, keys, perm);
        CDR_LAUNCH_CHECK();
    } else {
        int rc = cdr_sort_ids(ctx, stream, ids, n, nullptr, 0, table_rows, keys, perm, ws, ws_bytes);
        if (rc) return rc;
    }
    return cdr_rowwise_apply(ctx, stream, opt, table, exp_avg, exp_avg_sq, D, keys, perm, n, grads, n, 0, nullptr, lr, beta1, beta2, eps,
                             weight_decay, step, nullptr, 0);
}

// ---- the per-positive (k-major) form: uid / pid [S] (the first S entries of recbole's tiled [S k] columns), nid [S k] k-major
extern "C" int cdr_bpr_step_fused_kmajor_sizes(int64_t S, int k, int64_t* flag_bytes, int64_t* heads_words) {
    CDR_CHECK_ARG(flag_bytes && heads_words && S > 0 && k >= 1 && k <= 64);
    const int fstride = (2 + k + 3) & ~3;
    *flag_bytes = S * (int64_t)fstride;
    *heads_words = heads_view::words(S, S + S * (int64_t)k);
    return CDR_OK;
}

extern "C" int cdr_bpr_step_fused_kmajor(cdr_ctx* ctx, void* stream, int opt, float* user_tab, float* user_m, float* user_v,
                                         int64_t user_rows, float* item_tab, float* item_m, float* item_v, int64_t item_rows, int D,
                                         const int64_t* uid, const int64_t* pid, const int64_t* nid, int64_t S, int k, float gamma,
                                         float reg_weight, float lr, float beta1, float beta2, float eps, float weight_decay,
                                         int64_t step_user, int64_t step_item, float* out9, float* GU, float* GI, uint32_t* keys,
                                         uint32_t* perm, uint8_t* flags, uint32_t* heads, void* sort_ws, size_t sort_ws_bytes) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && uid && pid && nid && out9 && GU && GI && keys && perm && flags && heads && sort_ws);
    CDR_CHECK_ARG(D > 0 && (D & 3) == 0 && D <= 256 && S > 0 && k >= 1 && k <= 64);
    const int64_t B = S * (int64_t)k, nI = S + B;
    CDR_CHECK_ARG(S + nI <= (int64_t)0x7FFFFFFF);
    CDR_CHECK_ARG(opt == 0 || (opt == 1 && user_m && user_v && item_m && item_v && step_user > 0 && step_item > 0));
    hipStream_t s = (hipStream_t)stream;
    const int lpr = cdr_lpr_for(D);
    const int fstride = (2 + k + 3) & ~3;
    const heads_view hv(heads, S);                     // (cnt[0..3] are cleared by coef_finish_kernel)
    int rc = embloss_head(ctx, s, user_tab, item_tab, D, uid, pid, S, B, k, reg_weight, out9, hv.cnt);
    if (rc) return rc;
    uint32_t key_base = 0;
    rc = cdr_sort_ids_two_tables(ctx, stream, uid, S, user_rows, pid, S, nid, B, item_rows, keys, perm, &key_base, sort_ws, sort_ws_bytes);
    if (rc) return rc;
    rc = occ_flags(ctx, s, keys, perm, S, S + nI, fstride, flags, hv);
    if (rc) return rc;
    const step_tables T = make_tables(opt, user_tab, user_m, user_v, step_user, opt, item_tab, item_m, item_v, step_item, lr, beta1, beta2, eps, weight_decay);
    const int grid = grid_for(S, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_BPR_FWD_APPLY, s);
        DISPATCH_LPR_OPT(lpr, opt, {
            constexpr int KS = O == 1 ? 2 : 4;              // negatives per round: 4; 2 for Adam at k <= 2
            auto kern = k <= 2 ? bpr_fwd_apply_kmajor_kernel<L, O, KS> : bpr_fwd_apply_kmajor_kernel<L, O, 4>;
            kern<<<dim3(grid), dim3(kBlock), 0, s>>>(T.TU, T.TI, D, uid, pid, nid, flags, fstride, S, k, gamma, 1.0f / (float)B, out9 + 4, T.hu, T.hi, GU, GI, ctx->partials);
        });
    }
    CDR_LAUNCH_CHECK();
    // duplicate rows: users over GU [S, D]; items over GI [S + B, D] (one row per occurrence of [pid | nid], signs folded in)
    dup_host sides[2];
    make_sides(sides, T, keys, perm, hv, GU, GI, S, nI, nI, S, out9 + 4, out9 + 5, key_base);
    return finish_and_apply_dups(ctx, s, opt, D, sides, [&](unsigned* za, unsigned* zb) {
        step_finish_keep_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, B, reg_weight, out9, za, zb);
    });
}

// ================================================================================================ CMF's two-domain step on shared tables
// cmf.py:75-99: both domains' batches train ONE user and ONE item table, and the reference takes one torch.optim.Adam step on the summed
// loss  alpha (BCE_s + lambda EmbLoss_s) + (1 - alpha) (BCE_t + gamma EmbLoss_t).  A row named by both domains' batches (an overlapped user,
// an item in both lists) gets ONE update from the sum of its contributions, so the step is cdr_point_step_fused over the JOINT occurrence
// list [source rows | target rows] -- occurrence o < B_s is source row o, o >= B_s target row o - B_s -- with per-domain weights:
//   pair_norms_kernel        the four EmbLoss sums ||U_s||^2, ||I_s||^2, ||U_t||^2, ||I_t||^2 (skipped when lambda = gamma = 0)
//   pair_coef_kernel         -> the per-domain coefficients c = w_d reg_d / (B_d ||.||); the update counts bumped on the device
//   one two-table sort       user keys [su | tu], item keys [si | ti] (make_keys_pair_kernel reads the four lists in place)
//   occ_flags_kernel         "only occurrence of its row across BOTH domains" per joint occurrence
//   point_pair_fwd_apply     single rows updated in place with their own domain's gradient and EmbLoss coefficient; every other occurrence
//                            writes its FULL gradient row (loss term + its domain's EmbLoss term), so the duplicate apply sums rows with no
//                            coefficient of its own (reg_coef = nullptr)
//   pair_finish_kernel       the loss vector; the duplicate applies (apply_dups_pair) give every other row exactly one update.
namespace {

__global__ __launch_bounds__(kBlock) void make_keys_pair_kernel(const int64_t* __restrict__ a0, int64_t na0, const int64_t* __restrict__ a1,
                                                                int64_t na1, const int64_t* __restrict__ b0, int64_t nb0,
                                                                const int64_t* __restrict__ b1, int64_t nb1, uint32_t key_base,
                                                                uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                uint32_t* __restrict__ zspan, int64_t zwords) {
    sort_state_clear(zspan, zwords);
    const int64_t na = na0 + na1, n = na + nb0 + nb1, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
        if (e < na) { keys[e] = (uint32_t)(e < na0 ? a0[e] : a1[e - na0]); vals[e] = (uint32_t)e; }
        else {
            const int64_t o = e - na;
            keys[e] = key_base + (uint32_t)(o < nb0 ? b0[o] : b1[o - nb0]);
            vals[e] = (uint32_t)o;                               // joint occurrence index inside the item lists
        }
    }
}

// partials[block] = {sum ||U[su]||^2, sum ||I[si]||^2, sum ||U[tu]||^2, sum ||I[ti]||^2} over the joint occurrence list
template <int LPR>
__global__ __launch_bounds__(kBlock) void pair_norms_kernel(const float* __restrict__ U, const float* __restrict__ I, int D,
                                                            const int64_t* __restrict__ su, const int64_t* __restrict__ si, int64_t Bs,
                                                            const int64_t* __restrict__ tu, const int64_t* __restrict__ ti, int64_t Bt,
                                                            double* __restrict__ partials) {
    constexpr int GPB = kBlock / LPR;
    constexpr int UNR = 8;
    __shared__ double smem[4 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int64_t N = Bs + Bt;
    const bool live = sub < (D >> 2);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t base = gg; base < N; base += TG * UNR) {
        int64_t iu[UNR], ii[UNR];
        float4 u[UNR], v[UNR];
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const int64_t tc = t < N ? t : N - 1;
            iu[r] = tc < Bs ? su[tc] : tu[tc - Bs]; ii[r] = tc < Bs ? si[tc] : ti[tc - Bs];
        }
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            u[r] = v[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < N && live) { u[r] = ld4n<(LPR >= 32)>(U + iu[r] * D + 4 * sub); v[r] = ld4n<(LPR >= 32)>(I + ii[r] * D + 4 * sub); }
        }
#pragma unroll
        for (int r = 0; r < UNR; ++r) {
            const int64_t t = base + (int64_t)r * TG;
            const float s_u = group_sum<LPR>(dot4(u[r], u[r])), s_i = group_sum<LPR>(dot4(v[r], v[r]));
            if (sub == 0) {
                if (t < Bs) { acc[0] += (double)s_u; acc[1] += (double)s_i; }
                else { acc[2] += (double)s_u; acc[3] += (double)s_i; }          // (t >= N: zero rows)
            }
        }
    }
    block_sum_d<4>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// out[9..12] = {c_u_s, c_i_s, c_u_t, c_i_t}: c = w_d reg_d / (B_d ||rows||) (0 without EmbLoss or for a zero norm), w_s = alpha, w_t = 1 - alpha.
// As coef_finish_kernel: the update counts (when given) advanced here with the Adam scalars of the new counts in hp_dev[0..3]; zero4 = the
// head lists' counters of occ_flags_kernel.
__global__ __launch_bounds__(kBlock) void pair_coef_kernel(const double* __restrict__ partials, int nblocks, int64_t Bs, int64_t Bt,
                                                           float wreg_s, float wreg_t, float* __restrict__ out, int64_t* __restrict__ step_u_dev,
                                                           int64_t* __restrict__ step_i_dev, float* __restrict__ hp_dev, float lr, float b1,
                                                           float b2, unsigned* __restrict__ zero4) {
    __shared__ double smem[4 * (kBlock / 64)];
    if (threadIdx.x >= 64 && threadIdx.x < 68) zero4[threadIdx.x - 64] = 0u;
    if (step_u_dev && threadIdx.x < 2) {
        int64_t* c = threadIdx.x == 0 ? step_u_dev : step_i_dev;
        const int64_t st = c[0] + 1;
        c[0] = st;
        if (hp_dev) cdr_adam_hp((double)st, lr, b1, b2, hp_dev[2 * threadIdx.x], hp_dev[2 * threadIdx.x + 1]);
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    sum_partials<4, kBlock>(partials, nblocks, acc, smem);
    if (threadIdx.x == 0) {
        const float n[4] = {(float)sqrt(acc[0]), (float)sqrt(acc[1]), (float)sqrt(acc[2]), (float)sqrt(acc[3])};
        for (int j = 0; j < 4; ++j) {
            const float wr = j < 2 ? wreg_s : wreg_t;
            const float B = (float)(j < 2 ? Bs : Bt);
            out[9 + j] = (wr != 0.f && n[j] > 0.f) ? wr / (B * n[j]) : 0.f;      // embloss_coef (cdr_loss_math.h), in place: the helper changed this kernel's code
        }
    }
}

// point_fwd_apply_kernel over the joint occurrence list: row t < Bs is source row t (weight invB_s = alpha / B_s, coefficients coef[0..1]),
// row t >= Bs target row t - Bs (invB_t = (1 - alpha) / B_t, coef[2..3]).  flags4[t] byte 0 / 1: its user / item occurs once in BOTH lists.
// partials[block] = {BCE sum_s, BCE sum_t, sum u_s^2, sum i_s^2, sum u_t^2, sum i_t^2} (pre-step rows).
template <int LPR, int OPT>
__global__ __launch_bounds__(kBlock) void point_pair_fwd_apply_kernel(int loss_kind, tab_ptrs TU, tab_ptrs TI, int D,
                                                                      const int64_t* __restrict__ su, const int64_t* __restrict__ si,
                                                                      const float* __restrict__ ys, int64_t Bs, const int64_t* __restrict__ tu,
                                                                      const int64_t* __restrict__ ti, const float* __restrict__ yt, int64_t Bt,
                                                                      const uint32_t* __restrict__ flags4, float invB_s, float invB_t,
                                                                      const float* __restrict__ coef, apply_hp hu, apply_hp hi,
                                                                      float* __restrict__ GU, float* __restrict__ GI, double* __restrict__ partials) {
    HP_FROM_DEV(hu); HP_FROM_DEV(hi);
    constexpr int GPB = kBlock / LPR;
    __shared__ double smem[6 * (kBlock / 64)];
    const int sub = threadIdx.x % LPR;
    const int64_t gg = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const int64_t TG = (int64_t)gridDim.x * GPB;
    const int64_t N = Bs + Bt;
    const bool live = sub < (D >> 2);
    const float cus = coef[0], cis = coef[1], cut = coef[2], cit = coef[3];
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t iu, ii, fl; float yl;
    {
        const int64_t tc = gg < N ? gg : N - 1;
        const bool src = tc < Bs;
        iu = (uint32_t)(src ? su[tc] : tu[tc - Bs]); ii = (uint32_t)(src ? si[tc] : ti[tc - Bs]); yl = src ? ys[tc] : yt[tc - Bs];
        fl = flags4[tc];
    }
    asm volatile("" : "+v"(iu), "+v"(ii), "+v"(fl), "+v"(yl));
    for (int64_t t = gg; t < N; t += TG) {
        const bool src = t < Bs;
        const bool fu = (fl & 0xFFu) != 0, fi = (fl & 0xFF00u) != 0;
        const int64_t ou = (int64_t)iu * D + 4 * sub, oi = (int64_t)ii * D + 4 * sub;
        float4 u = live ? ld4n<(LPR >= 32)>(TU.W + ou) : z4, v = live ? ld4n<(LPR >= 32)>(TI.W + oi) : z4;
        float4 um = z4, uv = z4, im = z4, iv = z4;
        if (live && fu) row_moments<LPR, OPT>(TU, ou, um, uv);
        if (live && fi) row_moments<LPR, OPT>(TI, oi, im, iv);
        uint32_t ju, ji, gl; float yn;
        {
            const int64_t tn = t + TG, tc = tn < N ? tn : N - 1;
            const bool sn = tc < Bs;
            ju = (uint32_t)(sn ? su[tc] : tu[tc - Bs]); ji = (uint32_t)(sn ? si[tc] : ti[tc - Bs]); yn = sn ? ys[tc] : yt[tc - Bs];
            gl = flags4[tc];
        }
        __builtin_amdgcn_sched_barrier(0);
        const float dx = group_sum<LPR>(dot4(u, v));
        const float s_u = group_sum<LPR>(dot4(u, u));
        const float s_i = group_sum<LPR>(dot4(v, v));
        const float invB = src ? invB_s : invB_t;
        float l, g;
        point_term(loss_kind, dx, yl, invB, l, g);
        asm volatile("" : "+v"(ju), "+v"(ji), "+v"(gl), "+v"(yn));        // every request of this iteration has returned
        __builtin_amdgcn_sched_barrier(0);
        const float cu = src ? cus : cut, ci = src ? cis : cit;
        const float4 gu = make_float4(g * v.x, g * v.y, g * v.z, g * v.w);
        const float4 gi = make_float4(g * u.x, g * u.y, g * u.z, g * u.w);
        if (fu) {
            const float4 wu = upd_math<OPT>(u, um, uv, gu, cu, hu);
            if (live) row_store<LPR, OPT>(TU, ou, wu, um, uv);
        } else if (live) {
            st4n<(LPR >= 32)>(GU + t * D + 4 * sub, make_float4(gu.x + cu * u.x, gu.y + cu * u.y, gu.z + cu * u.z, gu.w + cu * u.w));
        }
        if (fi) {
            const float4 wi = upd_math<OPT>(v, im, iv, gi, ci, hi);
            if (live) row_store<LPR, OPT>(TI, oi, wi, im, iv);
        } else if (live) {
            st4n<(LPR >= 32)>(GI + t * D + 4 * sub, make_float4(gi.x + ci * v.x, gi.y + ci * v.y, gi.z + ci * v.z, gi.w + ci * v.w));
        }
        if (sub == 0) {
            if (src) { acc[0] += (double)l; acc[2] += (double)s_u; acc[3] += (double)s_i; }
            else { acc[1] += (double)l; acc[4] += (double)s_u; acc[5] += (double)s_i; }
        }
        iu = ju; ii = ji; fl = gl; yl = yn;
    }
    block_sum_d<6>(acc, smem);
    if (threadIdx.x == 0) store_partials(partials, acc);
}

// out[0..8] = {total, BCE_s, BCE_t, EmbLoss_s, EmbLoss_t, ||U_s||, ||I_s||, ||U_t||, ||I_t||} from the forward's partials (BCE: the mean over
// the domain's rows; EmbLoss = (||U_d|| + ||I_d||) / B_d, recbole's EmbLoss over the gathered rows); out[9..12] (the coefficients) stay.
// zero_a / zero_b: the long-segment counters of the duplicate applies behind this launch.
__global__ __launch_bounds__(kBlock) void pair_finish_kernel(const double* __restrict__ partials, int nblocks, int64_t Bs, int64_t Bt,
                                                             float alpha, float reg_s, float reg_t, float* __restrict__ out,
                                                             unsigned* __restrict__ zero_a, unsigned* __restrict__ zero_b) {
    __shared__ double smem[6 * (kBlock / 64)];
    if (zero_a && threadIdx.x >= 64 && threadIdx.x < 68) zero_a[threadIdx.x - 64] = 0u;
    if (zero_b && threadIdx.x >= 128 && threadIdx.x < 132) zero_b[threadIdx.x - 128] = 0u;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nblocks; b += kBlock) {           // sum_partials (cdr_loss_math.h), in place: the helper changed this kernel's code
        const double* o = partials + (size_t)b * CDR_PARTIAL_STRIDE;
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[j] += o[j];
    }
    block_sum_d<6>(acc, smem);
    if (threadIdx.x == 0) {
        const float bce_s = (float)(acc[0] / (double)Bs), bce_t = (float)(acc[1] / (double)Bt);
        const float nus = (float)sqrt(acc[2]), nis = (float)sqrt(acc[3]), nut = (float)sqrt(acc[4]), nit = (float)sqrt(acc[5]);
        const float emb_s = (nus + nis) / (float)Bs, emb_t = (nut + nit) / (float)Bt;
        out[0] = alpha * (bce_s + reg_s * emb_s) + (1.0f - alpha) * (bce_t + reg_t * emb_t);
        out[1] = bce_s; out[2] = bce_t; out[3] = emb_s; out[4] = emb_t;
        out[5] = nus; out[6] = nis; out[7] = nut; out[8] = nit;
    }
}

}  // namespace

// What the two entries of CMF's pair step share.  THREE: the launch also exists for CDR_OPT_ADAGRAD (cdr_point_step_fused_pair).
template <bool THREE>
static int point_pair_step_impl(cdr_ctx* ctx, void* stream, int loss_kind, int opt, float* user_tab, float* user_m, float* user_v,
                                int64_t user_rows, float* item_tab, float* item_m, float* item_v, int64_t item_rows, int D,
                                const int64_t* su, const int64_t* si, const float* ys, int64_t B_s, const int64_t* tu,
                                const int64_t* ti, const float* yt, int64_t B_t, float alpha, float reg_s, float reg_t, float lr,
                                float beta1, float beta2, float eps, float weight_decay, int64_t* step_user_dev,
                                int64_t* step_item_dev, float* hp_dev, float* out16, float* GU, float* GI, uint32_t* keys,
                                uint32_t* perm, uint8_t* flags, uint32_t* heads, void* sort_ws, size_t sort_ws_bytes) {
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = B_s + B_t;
    const int lpr = cdr_lpr_for(D);
    const float wreg_s = alpha * reg_s, wreg_t = (1.0f - alpha) * reg_t;
    const heads_view hv(heads, N);                     // (cnt[0..3] are cleared by pair_coef_kernel)
    // ---- EmbLoss coefficients first (they do not need the sort) + the device-resident update counts
    int ngrid = 0;
    if (wreg_s != 0.f || wreg_t != 0.f) {
        ngrid = grid_for((N + 7) / 8, kBlock / lpr);
        cdr_time_scope ts(ctx, CDR_TAG_BATCH_NORMS, s);
        DISPATCH_LPR(lpr, pair_norms_kernel<L><<<dim3(ngrid), dim3(kBlock), 0, s>>>(user_tab, item_tab, D, su, si, B_s, tu, ti, B_t, ctx->partials));
        CDR_LAUNCH_CHECK();
    }
    pair_coef_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, ngrid, B_s, B_t, wreg_s, wreg_t, out16, step_user_dev, step_item_dev,
                                                      opt == 1 ? hp_dev : nullptr, lr, beta1, beta2, hv.cnt);
    CDR_LAUNCH_CHECK();
    // ---- one sort of both tables' keys: [su | tu] and key_base + [si | ti]
    const unsigned hb = two_table_bits(user_rows, item_rows);
    CDR_CHECK_ARG(hb < 31);
    const uint32_t key_base = 1u << hb;
    int rc = sort_ids_with(ctx, s, 2 * N, (int64_t)key_base * 2, keys, perm, sort_ws, sort_ws_bytes, [&](uint32_t* keys_in, uint32_t* vals_in, sort_clear z) {
        make_keys_pair_kernel<<<dim3(grid_for(2 * N, kBlock)), dim3(kBlock), 0, s>>>(su, B_s, tu, B_t, si, B_s, ti, B_t, key_base, keys_in, vals_in, z.p, z.words);
    });
    if (rc) return rc;
    rc = occ_flags(ctx, s, keys, perm, N, 2 * N, 4, flags, hv);
    if (rc) return rc;
    // ---- forward + single rows in place; the Adam scalars of the new counts come from hp_dev (apply_hp::dev)
    step_tables T = make_tables(opt, user_tab, user_m, user_v, 1, opt, item_tab, item_m, item_v, 1, lr, beta1, beta2, eps, weight_decay);
    if (opt == 1) { T.hu.dev = hp_dev; T.hi.dev = hp_dev + 2; }
    const int grid = grid_for(N, kBlock / lpr);
    {
        cdr_time_scope ts(ctx, CDR_TAG_POINT_FWD_GRAD, s);
        if constexpr (THREE) DISPATCH_LPR_OPT3(lpr, opt, point_pair_fwd_apply_kernel<L, O><<<dim3(grid), dim3(kBlock), 0, s>>>(
                                       loss_kind, T.TU, T.TI, D, su, si, ys, B_s, tu, ti, yt, B_t, (const uint32_t*)flags, alpha / (float)B_s, (1.0f - alpha) / (float)B_t,
                                       out16 + 9, T.hu, T.hi, GU, GI, ctx->partials));
        else DISPATCH_LPR_OPT(lpr, opt, point_pair_fwd_apply_kernel<L, O><<<dim3(grid), dim3(kBlock), 0, s>>>(
                                       loss_kind, T.TU, T.TI, D, su, si, ys, B_s, tu, ti, yt, B_t, (const uint32_t*)flags, alpha / (float)B_s, (1.0f - alpha) / (float)B_t,
                                       out16 + 9, T.hu, T.hi, GU, GI, ctx->partials));
    }
    CDR_LAUNCH_CHECK();
    // ---- every row with more than one occurrence: one update from the sum of its (complete) gradient rows
    dup_host sides[2];
    make_sides(sides, T, keys, perm, hv, GU, GI, N, N, N, N, nullptr, nullptr, key_base);
    return finish_and_apply_dups(ctx, s, opt, D, sides, [&](unsigned* za, unsigned* zb) {
        pair_finish_kernel<<<dim3(1), dim3(kBlock), 0, s>>>(ctx->partials, grid, B_s, B_t, alpha, reg_s, reg_t, out16, za, zb);
    });
}

extern "C" int cdr_point_step_fused_pair_dev(cdr_ctx* ctx, void* stream, int loss_kind, int opt, float* user_tab, float* user_m, float* user_v,
                                             int64_t user_rows, float* item_tab, float* item_m, float* item_v, int64_t item_rows, int D,
                                             const int64_t* su, const int64_t* si, const float* ys, int64_t B_s, const int64_t* tu,
                                             const int64_t* ti, const float* yt, int64_t B_t, float alpha, float reg_s, float reg_t, float lr,
                                             float beta1, float beta2, float eps, float weight_decay, int64_t* step_user_dev,
                                             int64_t* step_item_dev, float* hp_dev, float* out16, float* GU, float* GI, uint32_t* keys,
                                             uint32_t* perm, uint8_t* flags, uint32_t* heads, void* sort_ws, size_t sort_ws_bytes) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && su && si && ys && tu && ti && yt && out16 && GU && GI && keys && perm && flags && heads && sort_ws);
    CDR_CHECK_ARG((loss_kind == CDR_LOSS_MSE || loss_kind == CDR_LOSS_BCE) && D > 0 && (D & 3) == 0 && D <= 256 && B_s >= 1 && B_t >= 1);
    CDR_CHECK_ARG(2 * (B_s + B_t) <= (int64_t)0x7FFFFFFF && user_rows > 0 && item_rows > 0);
    CDR_CHECK_ARG((step_user_dev == nullptr) == (step_item_dev == nullptr));
    CDR_CHECK_ARG(opt == 0 || (opt == 1 && user_m && user_v && item_m && item_v && step_user_dev && hp_dev));
    CDR_CHECK_ARG(((uintptr_t)flags & 3) == 0);
    return point_pair_step_impl<false>(ctx, stream, loss_kind, opt, user_tab, user_m, user_v, user_rows, item_tab, item_m, item_v, item_rows, D, su, si, ys, B_s,
                                       tu, ti, yt, B_t, alpha, reg_s, reg_t, lr, beta1, beta2, eps, weight_decay, step_user_dev, step_item_dev, hp_dev,
                                       out16, GU, GI, keys, perm, flags, heads, sort_ws, sort_ws_bytes);
}

// The same step under CDR_OPT_ADAGRAD, which reads no update count (user_m = item_m = NULL, the tables' sums of squared gradients in
// user_v / item_v; eps = torch's 1e-10).  Buffers as cdr_point_step_fused_pair_dev's.  CDR_OPT_SGD and CDR_OPT_ADAM are refused here:
// their entry is the _dev form.
extern "C" int cdr_point_step_fused_pair(cdr_ctx* ctx, void* stream, int loss_kind, int opt, float* user_tab, float* user_m, float* user_v,
                                         int64_t user_rows, float* item_tab, float* item_m, float* item_v, int64_t item_rows, int D,
                                         const int64_t* su, const int64_t* si, const float* ys, int64_t B_s, const int64_t* tu,
                                         const int64_t* ti, const float* yt, int64_t B_t, float alpha, float reg_s, float reg_t, float lr,
                                         float eps, float weight_decay, float* out16, float* GU, float* GI, uint32_t* keys,
                                         uint32_t* perm, uint8_t* flags, uint32_t* heads, void* sort_ws, size_t sort_ws_bytes) {
    CDR_CHECK_ARG(ctx && user_tab && item_tab && su && si && ys && tu && ti && yt && out16 && GU && GI && keys && perm && flags && heads && sort_ws);
    CDR_CHECK_ARG((loss_kind == CDR_LOSS_MSE || loss_kind == CDR_LOSS_BCE) && D > 0 && (D & 3) == 0 && D <= 256 && B_s >= 1 && B_t >= 1);
    CDR_CHECK_ARG(2 * (B_s + B_t) <= (int64_t)0x7FFFFFFF && user_rows > 0 && item_rows > 0);
    CDR_CHECK_ARG(opt == CDR_OPT_ADAGRAD && !user_m && user_v && !item_m && item_v);
    CDR_CHECK_ARG(((uintptr_t)flags & 3) == 0);
    return point_pair_step_impl<true>(ctx, stream, loss_kind, opt, user_tab, user_m, user_v, user_rows, item_tab, item_m, item_v, item_rows, D, su, si, ys, B_s,
                                      tu, ti, yt, B_t, alpha, reg_s, reg_t, lr, 0.f, 0.f, eps, weight_decay, nullptr, nullptr, nullptr,
                                      out16, GU, GI, keys, perm, flags, heads, sort_ws, sort_ws_bytes);
}
