// DeepAPF full-sort scoring in ONE launch (deepapf.py:111-161: target_forward over every (evaluated user, target item) pair).  The
// reference -- and this project's fallback -- repeats every user row N times and calls predict in chunks; per pair that gathers three table
// rows again and pushes two [2B, D] intermediates through memory.  Per pair (u, i), with S / O the key side's share / target-only rows and
// T the other side's row:
//      x_c = c (.) T   a_c = w2 . relu(W1 x_c + b1)   (c = S, O)     a_S = -1e31 where key > n_overlap (strictly)
//      (al_S, al_O) = softmax(a_S, a_O)     p = sigmoid(wp . ((al_S S + al_O O) (.) T)) = sigmoid(al_S z_S + al_O z_O),   z_c = wp . x_c
// -- two D x D contractions (4 D^2 FLOP) and a handful of row dots; nothing but table rows is read.
//
// Layout (the one of cdr_conet_fullsort.hip).  A wave owns a tile of 32 items and keeps their rows in registers for all the users it
// serves: T in overlap_users mode (the user carries S and O), S and O in overlap_items mode (the user carries T).  The workgroup's user
// chunk sits in LDS; lane (item c, half h) reads the chunk rows as wave-half broadcasts and forms the B operand of
// v_mfma_f32_32x32x2_f32 on the fly, x[f][c] = (item register) * (user value): W1 (s (.) t) = (W1 diag(s)) t needs no operand in memory.
// A = W1 (rows = output features), read from LDS: W1 is D x D -- 64 fragment registers per lane at D = 64 and 256 at D = 128 -- so it is
// staged once per workgroup as Wl[f / 4][j][f % 4]: a lane's four K steps are one 16-byte read, 32 consecutive rows j one 512-byte run
// (conflict-free).  Half h contracts features h S + s at K step s (S = DP / 2), 32 output features per pass (`blk`); the two candidates
// run as two independent accumulator chains that share the A read.  relu(+ b1) and the w2 dot happen on the accumulator registers
// (feature of register r, half h: cdr_conet_fullsort's fs_feat); z_c is a per-lane chain over the lane's features against a second copy
// of the chunk rows that was multiplied by wp while it was staged; both end in one exchange with the other half.  Nothing but table rows
// and the scores touches memory.
// Registers: the compiler hoists, sinks and re-uses LDS reads across the 32-feature passes as far as it is allowed to, which cost up to 700 B
// of scratch at D = 128; ap_opaque, the pinned z sums and a scheduling barrier per K group keep the live set at the item rows, two
// accumulators and one group of operands read ahead (DESIGN 4.4.2 has the counts: no scratch, two waves per SIMD at every width).
// A masked key has al_S = 0 and al_O = 1 exactly (exp(-1e31 - a_O) = 0 in fp32), so p = sigmoid(z_O): a masked USER (wave-uniform)
// and a tile whose items are ALL masked skip the share contraction; its operands are never read.
//
// Two epilogues, one scoring body (template parameter TOPK), as in conet_fullsort_kernel: out[u][item], or per-user running top-k lists
// behind the evaluation mask (cdr_topk.h) written as partial lists for topk_merge_launch.  The score is the same instruction sequence in
// both, so listed values are bit-equal to stored ones.
#include "cdr_common.h"
#include "cdr_mfma.h"
#include "cdr_topk.h"
#include "cdr_fullsort_tile.h"

namespace {

constexpr int kApWaves = 8;                      // item tiles per workgroup pass: W1 is staged once for eight waves (two per SIMD)
constexpr int kApBlock = 64 * kApWaves;
constexpr int kApUsers = 8;                      // users per LDS chunk (four rows of 128 floats each at most: 16 KB)
// TOPK launch geometry (cdr_topk.h): the 64 KB of lists and queues lie next to at most 81 KB of W1, vectors and chunk -- 79 users per
// workgroup at k = 10, 12 at k = 64.  One workgroup per CU, eight stripes each (at most 8 x 256); the sample call runs 4 x 8 = 32 stripes.
constexpr topk_stripe_geom kApTopkGeom{kApWaves, 0, CDR_NUM_CU, 4, 0};

struct ap_args {
    const float* key_s; const float* key_o;      // the key side's share / target-only tables
    const float* oth;                            // the other side's target table
    int64_t ld_s, ld_o, ld_t;
    const int64_t* uid;                          // [U] evaluated users (rows of the user-side tables)
    int64_t U, N, n_overlap;
    int D;
    const float* W1; const float* b1; const float* w2; const float* wp;      // [D, D] row-major, [D], [D], [D]
    float* out; int64_t ldo;                     // [U, N]
    int users_per_block;
};
struct ap_args_topk : ap_args { topk_out tk; };
template <bool TOPK> using ap_kargs = std::conditional_t<TOPK, ap_args_topk, ap_args>;

// floats of the fixed LDS part: W1 | b1 | w2 | the user chunk | the chunk's mask flags
__host__ __device__ constexpr size_t ap_fixed_words(int DP, bool itemkey) {
    return (size_t)DP * DP + 2 * DP + (size_t)kApUsers * (itemkey ? 2 : 4) * DP + kApUsers;
}

// the user rows of [u0, u0 + nu) into LDS, zero-padded to DP, each followed by the same rows multiplied by wp (the z dots' operands);
// overlap_users: a masked user's share row is not read
template <int NB, bool ITEMKEY>
__device__ __forceinline__ void ap_stage_users(const ap_args& a, float* __restrict__ Ul, int* __restrict__ mflag, int64_t u0, int nu) {
    constexpr int DP = 32 * NB, RU = ITEMKEY ? 1 : 2, Q = DP / 4;
    for (int e = threadIdx.x; e < nu * RU * Q; e += kApBlock) {
        const int uu = e / (RU * Q), rem = e - uu * RU * Q, r = rem / Q, f = 4 * (rem - r * Q);
        const int64_t id = a.uid[u0 + uu];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (f < a.D) {
            if (ITEMKEY) v = ld4(a.oth + id * a.ld_t + f);
            else if (r == 1) v = ld4(a.key_o + id * a.ld_o + f);
            else if (id <= a.n_overlap) v = ld4(a.key_s + id * a.ld_s + f);
        }
        *reinterpret_cast<float4*>(Ul + (uu * 2 * RU + r) * DP + f) = v;
        const float4 w = f < a.D ? ld4(a.wp + f) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(Ul + (uu * 2 * RU + RU + r) * DP + f) = make_float4(w.x * v.x, w.y * v.y, w.z * v.z, w.w * v.w);
    }
    if (!ITEMKEY)
        for (int e = threadIdx.x; e < nu; e += kApBlock) mflag[e] = a.uid[u0 + e] > a.n_overlap ? 1 : 0;
}

// an offset the optimiser cannot see through: the chunk rows are re-read in every 32-feature pass instead of being kept (hoisted out of the
// pass loop they are 2 x 64 more live registers at D = 128)
__device__ __forceinline__ int ap_opaque(int v) {
    asm volatile("" : "+s"(v));
    return v;
}

template <bool ITEMKEY, int S, int S1>
__device__ __forceinline__ const float (&ap_pick(const float (&r0)[S], const float (&r1)[S1]))[S] {
    if constexpr (ITEMKEY) return r1; else return r0;
}

// z_c = wp . (c (.) T) for both candidates: the chunk holds every user row a second time multiplied by wp (`w0` / `wo`), so this is a
// per-lane chain over the lane's features with the item registers.  Operands of group s + 4 are read while group s runs.
template <int NB, bool BOTH>
__device__ __forceinline__ void ap_zdots(const float* w0, const float* wo, const float (&r0)[16 * NB], const float (&ro)[16 * NB], float& zs,
                                         float& zo) {
    constexpr int S = 16 * NB;
    const auto ld = [](const float* p) { return *reinterpret_cast<const float4*>(p); };
    float4 vo = ld(wo), vs = BOTH ? ld(w0) : vo;
#pragma unroll
    for (int s = 0; s < S; s += 4) {
        float4 nvo = vo, nvs = vs;
        if (s + 4 < S) {
            nvo = ld(wo + s + 4);
            if (BOTH) nvs = ld(w0 + s + 4);
        }
        if (BOTH) { zs = fmaf(r0[s], vs.x, zs); zs = fmaf(r0[s + 1], vs.y, zs); zs = fmaf(r0[s + 2], vs.z, zs); zs = fmaf(r0[s + 3], vs.w, zs); }
        zo = fmaf(ro[s], vo.x, zo); zo = fmaf(ro[s + 1], vo.y, zo); zo = fmaf(ro[s + 2], vo.z, zo); zo = fmaf(ro[s + 3], vo.w, zo);
        // (the sums are pinned here: left free, the chain sinks behind the MFMA passes and every operand read above stays live across them)
        asm volatile("" : "+v"(zs), "+v"(zo));
        __builtin_amdgcn_sched_barrier(0);
        vo = nvo; vs = nvs;
    }
}

// One pass of 32 output features for one (tile, user): the K loop of both candidates (BOTH) or of the only candidate alone on
// v_mfma_f32_32x32x2_f32, then relu(+ b1) and the w2 dot on the accumulator registers.  wa: this lane's A fragments of the pass; l0 / lo: the
// chunk rows the share / only candidate multiplies (this half's features); r0 / ro: the item rows likewise; b1b / w2b: the pass's vectors.
// The operands of K group s + 4 are read while group s runs (the scheduling barrier keeps the compiler from reading the whole pass ahead).
template <int NB, bool BOTH>
__device__ __forceinline__ void ap_block(const float* wa, const float* l0, const float* lo, const float* b1b, const float* w2b,
                                         const float (&r0)[16 * NB], const float (&ro)[16 * NB], float& as, float& ao) {
    constexpr int DP = 32 * NB, S = 16 * NB;
    const auto ld = [](const float* p) { return *reinterpret_cast<const float4*>(p); };
    f32x16 cs = zero16(), co = zero16();
    float4 av = ld(wa), vo = ld(lo), vs = BOTH ? ld(l0) : vo;
#pragma unroll
    for (int s = 0; s < S; s += 4) {
        float4 nav = av, nvo = vo, nvs = vs;
        if (s + 4 < S) {
            nav = ld(wa + (size_t)(s / 4 + 1) * DP * 4);
            nvo = ld(lo + s + 4);
            if (BOTH) nvs = ld(l0 + s + 4);
        }
        if (BOTH) {
            MF1(cs, av.x, r0[s] * vs.x); MF1(co, av.x, ro[s] * vo.x);
            MF1(cs, av.y, r0[s + 1] * vs.y); MF1(co, av.y, ro[s + 1] * vo.y);
            MF1(cs, av.z, r0[s + 2] * vs.z); MF1(co, av.z, ro[s + 2] * vo.z);
            MF1(cs, av.w, r0[s + 3] * vs.w); MF1(co, av.w, ro[s + 3] * vo.w);
        } else {
            MF1(co, av.x, ro[s] * vo.x); MF1(co, av.y, ro[s + 1] * vo.y); MF1(co, av.z, ro[s + 2] * vo.z); MF1(co, av.w, ro[s + 3] * vo.w);
        }
        __builtin_amdgcn_sched_barrier(0);
        av = nav; vo = nvo; vs = nvs;
    }
    // register r = 4 g + q of half h holds output feature 8 g + 4 h + q of the pass
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 bv = ld(b1b + 8 * g), wv = ld(w2b + 8 * g);
        if (BOTH) {
            as = fmaf(wv.x, fmaxf(cs[4 * g] + bv.x, 0.f), as); as = fmaf(wv.y, fmaxf(cs[4 * g + 1] + bv.y, 0.f), as);
            as = fmaf(wv.z, fmaxf(cs[4 * g + 2] + bv.z, 0.f), as); as = fmaf(wv.w, fmaxf(cs[4 * g + 3] + bv.w, 0.f), as);
        }
        ao = fmaf(wv.x, fmaxf(co[4 * g] + bv.x, 0.f), ao); ao = fmaf(wv.y, fmaxf(co[4 * g + 1] + bv.y, 0.f), ao);
        ao = fmaf(wv.z, fmaxf(co[4 * g + 2] + bv.z, 0.f), ao); ao = fmaf(wv.w, fmaxf(co[4 * g + 3] + bv.w, 0.f), ao);
    }
    __builtin_amdgcn_sched_barrier(0);
}

template <int NB, bool ITEMKEY, bool TOPK>
__global__ __launch_bounds__(kApBlock) void deepapf_fullsort_kernel(ap_kargs<TOPK> a) {
    constexpr int DP = 32 * NB, S = 16 * NB, RU = ITEMKEY ? 1 : 2, S1 = ITEMKEY ? S : 1;
    extern __shared__ __attribute__((aligned(16))) float ap_lds[];
    float* const Wl = ap_lds;
    float* const b1l = Wl + DP * DP;
    float* const w2l = b1l + DP;
    float* const Ul = w2l + DP;
    int* const mflag = reinterpret_cast<int*>(Ul + kApUsers * 2 * RU * DP);
    float* const dyn = reinterpret_cast<float*>(mflag + kApUsers);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const int D = a.D;
    const int64_t u_lo = (int64_t)blockIdx.y * a.users_per_block;
    const int64_t u_hi = u_lo + a.users_per_block < a.U ? u_lo + a.users_per_block : a.U;
    const bool one_chunk = u_hi - u_lo <= kApUsers;           // staged once, not once per tile round
    if (one_chunk) ap_stage_users<NB, ITEMKEY>(a, Ul, mflag, u_lo, (int)(u_hi - u_lo));
    // W1 as Wl[f / 4][j][f % 4] (D % 4 == 0: a group of four K features is wholly inside or outside), the three vectors, zero-padded
    for (int t = threadIdx.x; t < DP * (DP / 4); t += kApBlock) {
        const int g = t / DP, j = t - g * DP;
        const bool ok = j < D && 4 * g < D;
        const float4 v = ld4(a.W1 + (ok ? (int64_t)j * D + 4 * g : 0));
        *reinterpret_cast<float4*>(Wl + 4 * t) = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int t = threadIdx.x; t < DP; t += kApBlock) {
        const bool ok = t < D;
        const float vb = a.b1[ok ? t : 0], v2 = a.w2[ok ? t : 0];
        b1l[t] = ok ? vb : 0.f; w2l[t] = ok ? v2 : 0.f;
    }
    topk_wave_lists lists;                                    // TOPK: this wave's lists of the workgroup's users, all empty
    if constexpr (TOPK) lists.init(dyn, wave, a.users_per_block, a.tk.k, a.tk, u_lo, a.U);
    // this lane's views: A fragments of row c (K features h S ..), the vectors' and the chunk rows' half
    const float* const wa0 = Wl + ((size_t)(h * (S / 4)) * DP + c) * 4;
    const float* const b1h = b1l + 4 * h;
    const float* const w2h = w2l + 4 * h;

    const int64_t n_tiles = (a.N + 31) >> 5;
    const int64_t tile_stride = (int64_t)gridDim.x * kApWaves;
    const int64_t rounds = (n_tiles + tile_stride - 1) / tile_stride;        // the same for every wave: the chunk is staged behind barriers
    __syncthreads();
    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t tile = ((int64_t)rd * gridDim.x + blockIdx.x) * kApWaves + wave;
        const bool live = tile < n_tiles;
        const int64_t item = tile * 32 + c;
        const bool iv = live && item < a.N;
        // the tile's rows.  overlap_users: r0 = T.  overlap_items: r0 = S (not read for a masked item), r1 = O
        float r0[S], r1[S1];
        const float (&ro)[S] = ap_pick<ITEMKEY>(r0, r1);                    // the item row of the only candidate: O / T
        const bool imask = ITEMKEY && item > a.n_overlap;                   // this lane's item takes al_S = 0
        const bool tile_masked = ITEMKEY && tile * 32 > a.n_overlap;        // ... and so does every item of the tile
        if constexpr (ITEMKEY) {
            tile_load_row<S>(r0, a.key_s + (iv ? item : 0) * a.ld_s, iv && !imask, h, D);
            tile_load_row<S>(r1, a.key_o + (iv ? item : 0) * a.ld_o, iv, h, D);
        } else {
            tile_load_row<S>(r0, a.oth + (iv ? item : 0) * a.ld_t, iv, h, D);
        }
        for (int64_t u0 = u_lo; u0 < u_hi; u0 += kApUsers) {
            const int nu = (int)(u_hi - u0 < kApUsers ? u_hi - u0 : kApUsers);
            if (!one_chunk) {
                __syncthreads();                                           // the previous chunk has been consumed by every wave
                ap_stage_users<NB, ITEMKEY>(a, Ul, mflag, u0, nu);
                __syncthreads();
            }
            if (!live) continue;
            for (int uu = 0; uu < nu; ++uu) {
                const float* const l0 = Ul + uu * 2 * RU * DP + h * S;          // overlap_users: S_u (zeros when masked); overlap_items: T_u
                const float* const lo = l0 + (ITEMKEY ? 0 : DP);            // the row the only candidate multiplies: O_u / T_u
                const bool skip_s = ITEMKEY ? tile_masked : mflag[uu] != 0;  // wave-uniform
                float thr_u = 0.f;
                if constexpr (TOPK) thr_u = lists.thr((int)(u0 - u_lo) + uu);
                // z_c = wp . x_c, then a_c = w2 . relu(W1 x_c + b1), 32 output features per pass
                float as = 0.f, ao = 0.f, zs = 0.f, zo = 0.f;
                if (!skip_s) {
                    ap_zdots<NB, true>(l0 + RU * DP, lo + RU * DP, r0, ro, zs, zo);
#pragma unroll 1
                    for (int blk = 0; blk < NB; ++blk) {
                        const int ofs = ap_opaque(blk * 32), zr = ap_opaque(0);
                        ap_block<NB, true>(wa0 + ofs * 4, l0 + zr, lo + zr, b1h + ofs, w2h + ofs, r0, ro, as, ao);
                    }
                } else {
                    ap_zdots<NB, false>(l0 + RU * DP, lo + RU * DP, r0, ro, zs, zo);
#pragma unroll 1
                    for (int blk = 0; blk < NB; ++blk) {
                        const int ofs = ap_opaque(blk * 32), zr = ap_opaque(0);
                        ap_block<NB, false>(wa0 + ofs * 4, l0 + zr, lo + zr, b1h + ofs, w2h + ofs, r0, ro, as, ao);
                    }
                }
                as += __shfl_xor(as, 32, 64); ao += __shfl_xor(ao, 32, 64);
                zs += __shfl_xor(zs, 32, 64); zo += __shfl_xor(zo, 32, 64);
                // masked: al_S = 0, al_O = 1 exactly; else the two-way softmax about the larger score
                const float m = fmaxf(as, ao);
                const float es = expf(as - m), eo = expf(ao - m);
                const float den = es + eo;
                const float zz = (es / den) * zs + (eo / den) * zo;
                const float z = (skip_s || imask) ? zo : zz;
                const float sc = 1.0f / (1.0f + expf(-z));
                if constexpr (!TOPK) {
                    if (h == 0 && iv) a.out[(u0 + uu) * a.ldo + item] = sc;
                } else {
                    // (only the h == 0 half carries candidates: at most 32 per call)
                    lists.template offer<32>(h == 0 && iv && sc > thr_u, sc, (int)item, (int)(u0 - u_lo) + uu, a.tk, u_lo);
                }
            }
        }
    }
    if constexpr (TOPK) lists.finish(a.tk, kApWaves, u_lo, u_hi, a.U);
}

template <bool TOPK>
int ap_dispatch(const ap_kargs<TOPK>& a, bool itemkey, dim3 grid, size_t list_bytes, hipStream_t s) {
    const size_t lds = sizeof(float) * ap_fixed_words(32 * ((a.D + 31) / 32), itemkey) + list_bytes;
    const int rc = tile_dispatch(a.D, itemkey, [&](auto nb, auto ik) {
        return tile_launch_one("cdr_deepapf_fullsort", deepapf_fullsort_kernel<nb(), ik(), TOPK>, a, grid, kApBlock, lds, s);
    });
    if (rc < 0) { cdr_set_error("cdr_deepapf_fullsort: D = %d outside the kernel's range", a.D); return CDR_EINVAL; }
    return rc;
}

// score epilogue: every workgroup stages W1 once, so the grid is a few workgroups per CU (cdr_fullsort_tile.h)
int ap_launch_scores(const ap_args& a, bool itemkey, hipStream_t s) {
    ap_args b = a;
    dim3 grid;
    if (const int rc = tile_score_grid("cdr_deepapf_fullsort", a.U, a.N, kApWaves, kApUsers, &grid, &b.users_per_block)) return rc;
    return ap_dispatch<false>(b, itemkey, grid, 0, s);
}

// the arguments both entries share; nothing is launched for a refused call
int ap_check(const char* fn, const float* share_tab, int64_t ld_share, const float* only_tab, int64_t ld_only, const float* other_tab,
             int64_t ld_other, const int64_t* uid, int64_t U, int64_t N, int D, const float* W1, const float* b1, const float* w2,
             const float* wp) {
    if (!cdr_deepapf_fullsort_supported(D)) {
        cdr_set_error("%s: D = %d outside the kernel's range (4..128, a multiple of 4)", fn, D);
        return CDR_EINVAL;
    }
    if (U < 1 || N < 1 || N >= ((int64_t)1 << 31) || U >= ((int64_t)1 << 31)) {
        cdr_set_error("%s: U = %lld, N = %lld outside 1 <= U, N < 2^31", fn, (long long)U, (long long)N);
        return CDR_EINVAL;
    }
    if (!share_tab || !only_tab || !other_tab || !uid || !W1 || !b1 || !w2 || !wp) { cdr_set_error("%s: null argument", fn); return CDR_EINVAL; }
    if (ld_share < D || ld_only < D || ld_other < D || ((ld_share | ld_only | ld_other) & 3) ||
        (((uintptr_t)share_tab | (uintptr_t)only_tab | (uintptr_t)other_tab | (uintptr_t)W1) & 15)) {
        cdr_set_error("%s: tables and W1 must be 16-byte aligned with row strides >= D that are multiples of 4", fn);
        return CDR_EINVAL;
    }
    return CDR_OK;
}

ap_args ap_fill(int key_is_item, const float* share_tab, int64_t ld_share, const float* only_tab, int64_t ld_only, const float* other_tab,
                int64_t ld_other, const int64_t* uid, int64_t U, int64_t N, int D, int64_t n_overlap, const float* W1, const float* b1,
                const float* w2, const float* wp) {
    ap_args a{};
    (void)key_is_item;
    a.key_s = share_tab; a.ld_s = ld_share; a.key_o = only_tab; a.ld_o = ld_only; a.oth = other_tab; a.ld_t = ld_other;
    a.uid = uid; a.U = U; a.N = N; a.D = D; a.n_overlap = n_overlap; a.W1 = W1; a.b1 = b1; a.w2 = w2; a.wp = wp;
    return a;
}

}  // namespace

extern "C" int cdr_deepapf_fullsort_supported(int D) { return D >= 4 && D <= 128 && (D & 3) == 0 ? 1 : 0; }

extern "C" int cdr_deepapf_fullsort(void* stream, int key_is_item, const float* share_tab, int64_t ld_share, const float* only_tab,
                                    int64_t ld_only, const float* other_tab, int64_t ld_other, const int64_t* uid, int64_t U, int64_t N,
                                    int D, int64_t n_overlap, const float* W1, const float* b1, const float* w2, const float* wp,
                                    float* out, int64_t ldo) {
    const int rc = ap_check("cdr_deepapf_fullsort", share_tab, ld_share, only_tab, ld_only, other_tab, ld_other, uid, U, N, D, W1, b1, w2, wp);
    if (rc) return rc;
    CDR_CHECK_ARG(out && ldo >= N);
    ap_args a = ap_fill(key_is_item, share_tab, ld_share, only_tab, ld_only, other_tab, ld_other, uid, U, N, D, n_overlap, W1, b1, w2, wp);
    a.out = out; a.ldo = ldo;
    return ap_launch_scores(a, key_is_item != 0, (hipStream_t)stream);
}

extern "C" int cdr_deepapf_fullsort_topk_workspace_bytes(int64_t U, int64_t N, int k, size_t* bytes) {
    return topk_stripe_ws_query("cdr_deepapf_fullsort_topk_workspace_bytes", kApTopkGeom, U, N, k, bytes);
}

extern "C" int cdr_deepapf_fullsort_topk(void* stream, int key_is_item, const float* share_tab, int64_t ld_share, const float* only_tab,
                                         int64_t ld_only, const float* other_tab, int64_t ld_other, const int64_t* uid, int64_t U,
                                         int64_t N, int D, int64_t n_overlap, const float* W1, const float* b1, const float* w2,
                                         const float* wp, int k, const int64_t* hist_indptr, const int64_t* hist_cols,
                                         int exclude_first_col, float* out_vals, int64_t* out_idx, void* workspace, size_t workspace_bytes) {
    if (const int rc = topk_check_k("cdr_deepapf_fullsort_topk", k)) return rc;
    const int rc0 = ap_check("cdr_deepapf_fullsort_topk", share_tab, ld_share, only_tab, ld_only, other_tab, ld_other, uid, U, N, D, W1, b1,
                             w2, wp);
    if (rc0) return rc0;
    CDR_CHECK_ARG(out_vals && out_idx && workspace);
    CDR_CHECK_ARG((hist_indptr == nullptr) == (hist_cols == nullptr));
    ap_args_topk a{};
    static_cast<ap_args&>(a) = ap_fill(key_is_item, share_tab, ld_share, only_tab, ld_only, other_tab, ld_other, uid, U, N, D, n_overlap, W1,
                                       b1, w2, wp);
    hipStream_t s = (hipStream_t)stream;
    return topk_seeded_run("cdr_deepapf_fullsort_topk", kApTopkGeom, s, U, N, k, topk_mask{hist_indptr, hist_cols, exclude_first_col},
                           out_vals, out_idx, workspace, workspace_bytes, [&](int64_t n_cols, const topk_stripe_plan& p, const topk_out& tk) {
                               ap_args_topk b = a;
                               b.N = n_cols; b.users_per_block = p.upb; b.tk = tk;
                               return ap_dispatch<true>(b, key_is_item != 0, dim3((unsigned)p.gx, (unsigned)p.gy), p.lds, s);
                           });
}
