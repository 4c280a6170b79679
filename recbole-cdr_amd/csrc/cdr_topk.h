// The mask + top-k pieces shared by the scoring kernels that end in a top-k instead of a score matrix: the evaluation mask, the wave-held
// running list, the LDS-list flush of queued candidates and the merge of partial lists (cdr_gemm.hip: the dot-product full-sort, with lists
// per workgroup and a queue size of its own).  The three one-launch scoring kernels whose waves each own an item stripe --
// cdr_conet_fullsort.hip (the MLP tower), cdr_deepapf_fullsort.hip, cdr_natr_fullsort.hip -- also share everything around those
// primitives: a wave's lists in LDS (topk_wave_lists), the launch geometry and workspace layout (topk_stripe_geom / topk_make_stripe_plan /
// topk_stripe_ws_bytes) and the host tail that seeds the thresholds from a sample call (topk_seeded_run).  One copy, internal linkage per
// translation unit.
#pragma once
#include "cdr_common.h"

namespace {

// ---- running top-k of one user, kept by a whole wave (mask + top-k fused after scoring) -------------------
// Lane j holds entry j of the list (values descending; k <= 64).  A wave "offers" 64 candidate scores at once: a ballot
// against the current k-th value rejects almost all of them after the first few tiles (expected survivors per user over
// N items: k ln(N/k)), the survivors are inserted one at a time with a shuffle (no LDS, no sort).  Masked columns -- the
// PAD item and the user's history, given as a CSR with ascending columns (the reference sets those scores to -inf before
// torch.topk: recbole Trainer._full_sort_batch_eval) -- are tested only for survivors.
struct topk_mask {
    const int64_t* indptr;      // [U + 1] or nullptr
    const int64_t* cols;        // ascending inside each user's range
    int exclude_col0;
};

__device__ __forceinline__ bool topk_masked(const topk_mask& mk, int64_t u, int col) {
    if (mk.exclude_col0 && col == 0) return true;
    if (!mk.indptr) return false;
    int64_t lo = mk.indptr[u], hi = mk.indptr[u + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t c = mk.cols[mid];
        if (c == col) return true;
        if (c < col) lo = mid + 1; else hi = mid;
    }
    return false;
}

// e / ec: this lane's list entry (lanes >= k carry -inf / -1 and never change).  Returns the new k-th value.
// DEDUP: a candidate whose column already sits in the list is dropped (the persistent kernel's overflow recovery re-offers a whole tile,
// part of which may have entered the list through the queues already).
template <bool DEDUP = false>
__device__ __forceinline__ float topk_offer(float v, int col, float thr, float& e, int& ec, int k, const topk_mask& mk, int64_t u) {
    const int lane = threadIdx.x & 63;
    bool pass = v > thr;
    if (__ballot(pass) == 0) return thr;
    // every surviving lane tests ITS column against the mask at the same time (64 binary searches in flight): testing them one
    // after the other inside the insertion loop put ~2.5 us of dependent loads on each of the k ln(n/k) survivors of a wave
    if (pass && (mk.indptr || mk.exclude_col0)) pass = !topk_masked(mk, u, col);
    unsigned long long m = __ballot(pass);
    while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float cv = __shfl(v, l);
        const int cc = __shfl(col, l);
        if (!(cv > thr)) continue;                                             // wave-uniform: the k-th value rose meanwhile
        if (DEDUP && __ballot(lane < k && ec == cc)) continue;
        const int pos = __popcll(__ballot(lane < k && e >= cv));                // entries that stay in front (ties: first seen)
        const float up = __shfl_up(e, 1);
        const int upc = __shfl_up(ec, 1);
        if (lane < k) {
            if (lane == pos) { e = cv; ec = cc; }
            else if (lane > pos) { e = up; ec = upc; }
        }
        thr = __shfl(e, k - 1);
    }
    return thr;
}

struct topk_out {
    int k;
    int col_off;                // column index of this slab's first item
    float* pv;                  // partial lists [producer][M][k]
    int* pc;
    topk_mask mk;
    const float* seed = nullptr;    // optional: seed[u * seed_stride] = a LOWER BOUND of user u's final k-th value (the k-th value over a sample
    int64_t seed_stride = 0;        // of the columns): every stripe's threshold starts just below it instead of at -inf (round 6)
};
// the threshold a seed stands for: the largest float below it, so that a score EQUAL to the sample's k-th value still enters its list
__device__ __forceinline__ float topk_seed_thr(const topk_out& tk, int64_t u, int64_t M) {
    if (!tk.seed || u >= M) return -INFINITY;
    const float s = tk.seed[u * tk.seed_stride];
    return s == -INFINITY ? s : nextafterf(s, -INFINITY);
}

// Mask test for the queued candidates, one per lane (64 binary searches in flight), then the survivors enter their
// user's list one at a time (LDS only).  Thresholds may have risen since a candidate was queued: re-tested on insert.
// (Tried in round 5: row-parallel insertion -- lane l owns row l's list and walks the compacted queue itself: every step of such a
//  per-lane loop is a dependent LDS round trip, 26.7 -> 32.3 ms at U = 1,024, k = 10.)
__device__ __forceinline__ void topk_flush(volatile float* qv, volatile int* qc, volatile int* qu, int qn, volatile float* thr_l,
                                           volatile float* lv, volatile int* lc, const topk_out& tk, int64_t u0) {
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < qn; base += 64) {
        const int i = base + lane;
        const bool valid = i < qn;
        const float v = valid ? qv[i] : -INFINITY;
        const int c = valid ? qc[i] : 0;
        const int ul = valid ? qu[i] : 0;
        const bool ok = valid && v > thr_l[ul] && !topk_masked(tk.mk, u0 + ul, c);
        unsigned long long m = __ballot(ok);
        const topk_mask none{nullptr, nullptr, 0};
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            const float cv = __shfl(v, l);
            const int cc = __shfl(c, l);
            const int cu = __shfl(ul, l);
            const float thr = thr_l[cu];
            if (!(cv > thr)) continue;
            float e = lane < tk.k ? lv[cu * tk.k + lane] : -INFINITY;
            int ec = lane < tk.k ? lc[cu * tk.k + lane] : -1;
            const float nthr = topk_offer<true>(lane == 0 ? cv : -INFINITY, cc, thr, e, ec, tk.k, none, 0);
            if (lane < tk.k) { lv[cu * tk.k + lane] = e; lc[cu * tk.k + lane] = ec; }
            // (a seeded list is not full for a while: its k-th value is -inf, the seed stays the threshold until the list's own passes it)
            if (lane == 0) thr_l[cu] = tk.seed ? fmaxf(nthr, topk_seed_thr(tk, u0 + cu, u0 + cu + 1)) : nthr;
        }
    }
}

// ---- a wave's running lists of its workgroup's users, in LDS (the stripe kernels: every wave owns an item stripe) ---------------------
// Private to the wave: no other wave reads or writes them, so they need no barrier.  Layout of a wave's region of the dynamic LDS, in
// floats: the k-th values thr[upb] | list values [upb][k] | list columns [upb][k] | queue [3][kTopkStripeQueue] of (score, column, user)
// candidates parked for their mask test (topk_flush: 64 history searches in flight).
constexpr int kTopkStripeQueue = 128;
__host__ __device__ constexpr size_t topk_wave_words(int upb, int k) { return (size_t)upb * (1 + 2 * k) + 3 * kTopkStripeQueue; }

struct topk_wave_lists {
    volatile float* thr_l = nullptr; volatile float* lv = nullptr; volatile int* lc = nullptr;
    volatile float* qv = nullptr; volatile int* qc = nullptr; volatile int* qu = nullptr;
    int qn = 0;

    // all lists empty: entries (-inf, -1), the k-th value -inf or just below the user's seed
    __device__ __forceinline__ void init(float* base, int wave, int upb, int k, const topk_out& tk, int64_t u_lo, int64_t U) {
        const int lane = threadIdx.x & 63;
        thr_l = base + (size_t)wave * topk_wave_words(upb, k);
        lv = thr_l + upb;
        lc = reinterpret_cast<volatile int*>(lv + (size_t)upb * k);
        qv = reinterpret_cast<volatile float*>(lc + (size_t)upb * k);
        qc = reinterpret_cast<volatile int*>(qv + kTopkStripeQueue);
        qu = qc + kTopkStripeQueue;
        for (int i = lane; i < upb; i += 64) thr_l[i] = topk_seed_thr(tk, u_lo + i, U);      // (-inf without a seed)
        for (int i = lane; i < upb * k; i += 64) { lv[i] = -INFINITY; lc[i] = -1; }
    }
    // user ul's current k-th value (the kernels may read it ahead of their MFMA chain)
    __device__ __forceinline__ float thr(int ul) const { return thr_l[ul]; }
    // `pass`: this lane's score beats its user's k-th value (formed by the kernel).  Almost every tile fails as a whole; the survivors wait
    // in the queue, which is flushed first when it cannot take MAXADD more (what one call adds at most).
    template <int MAXADD>
    __device__ __forceinline__ void offer(bool pass, float score, int item, int ul, const topk_out& tk, int64_t u_lo) {
        const unsigned long long m = __ballot(pass);
        if (m) {
            if (qn + MAXADD > kTopkStripeQueue) { topk_flush(qv, qc, qu, qn, thr_l, lv, lc, tk, u_lo); qn = 0; }
            if (pass) {
                const int at = qn + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1));
                qv[at] = score; qc[at] = item; qu[at] = ul;
            }
            qn += __popcll(m);
        }
    }
    // one partial list per (this wave, user of the workgroup): pv / pc [blockIdx.x * waves + wave][U][k]; a wave that met no tile writes its
    // empty lists.  (The producer index is formed here, behind the flush: handed in by the kernel it cost the default tower's 68 B of scratch.)
    __device__ __forceinline__ void finish(const topk_out& tk, int waves, int64_t u_lo, int64_t u_hi, int64_t U) {
        if (qn) topk_flush(qv, qc, qu, qn, thr_l, lv, lc, tk, u_lo);
        const int64_t prod = (int64_t)blockIdx.x * waves + (threadIdx.x >> 6);
        const int k = tk.k, n = (int)(u_hi - u_lo) * k;
        for (int i = (int)(threadIdx.x & 63); i < n; i += 64) {
            const int64_t o = (prod * U + u_lo) * k + i;
            tk.pv[o] = lv[i];
            tk.pc[o] = lc[i];
        }
    }
};

// Merge of partial lists (already masked): one wave per (user, group of `gsz` producers).  With `out_pv` set the group's list
// goes to partial list `group` of the next level; the last level (one group) writes the final [U, k] output.
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ pv, const int* __restrict__ pc, int64_t P,
                                                         int64_t U, int k, int64_t gsz, float* __restrict__ out_pv,
                                                         int* __restrict__ out_pc, float* __restrict__ out_v,
                                                         int64_t* __restrict__ out_c) {
    const int lane = threadIdx.x & 63;
    const int64_t groups = (P + gsz - 1) / gsz;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= U * groups) return;
    const int64_t u = w % U, grp = w / U;
    const int64_t p0 = grp * gsz, p1 = p0 + gsz < P ? p0 + gsz : P;
    float e = -INFINITY, thr = -INFINITY;
    int ec = -1;
    const topk_mask none{nullptr, nullptr, 0};
    const int64_t total = (p1 - p0) * k;                             // candidate i = entry i % k of producer p0 + i / k
    for (int64_t i0 = 0; i0 < total; i0 += 64 * 8) {
        float v[8];
        int c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t i = i0 + 64 * j + lane;
            const int64_t o = ((p0 + i / k) * U + u) * k + i % k;
            v[j] = i < total ? pv[o] : -INFINITY;
            c[j] = i < total ? pc[o] : -1;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) thr = topk_offer(v[j], c[j], thr, e, ec, k, none, u);
    }
    if (lane < k) {
        if (out_pv) {
            out_pv[(grp * U + u) * k + lane] = e;
            out_pc[(grp * U + u) * k + lane] = ec;
        } else {
            out_v[u * k + lane] = e;
            out_c[u * k + lane] = ec;
        }
    }
}

constexpr int64_t kTopkMergeGroup = 64;             // partial lists merged per wave and level

// bytes of `producers` partial lists' values (or columns), rounded to 256
inline size_t topk_part_bytes(int64_t producers, int64_t U, int k) {
    return ((size_t)producers * U * k * 4 + 255) & ~(size_t)255;
}

// `prod` partial lists (pv, pc: [prod][U][k]) -> out_vals / out_idx [U, k].  pv1 / pc1: room for ceil(prod / kTopkMergeGroup) lists,
// used when two levels are run (groups of 64 lists, then the group lists).
inline int topk_merge_launch(hipStream_t s, const float* pv, const int* pc, int64_t prod, int64_t U, int k, float* pv1, int* pc1,
                             float* out_vals, int64_t* out_idx) {
    const int64_t l1 = (prod + kTopkMergeGroup - 1) / kTopkMergeGroup;
    if (prod > 2 * kTopkMergeGroup) {                                // two levels: groups of 64 lists, then the l1 group lists
        topk_merge_kernel<<<dim3((unsigned)((U * l1 + 3) / 4)), dim3(256), 0, s>>>(pv, pc, prod, U, k, kTopkMergeGroup, pv1, pc1, nullptr, nullptr);
        CDR_LAUNCH_CHECK();
        topk_merge_kernel<<<dim3((unsigned)((U + 3) / 4)), dim3(256), 0, s>>>(pv1, pc1, l1, U, k, l1, nullptr, nullptr, out_vals, out_idx);
    } else {
        topk_merge_kernel<<<dim3((unsigned)((U + 3) / 4)), dim3(256), 0, s>>>(pv, pc, prod, U, k, prod, nullptr, nullptr, out_vals, out_idx);
    }
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

// ---- launch geometry and workspace of the stripe kernels, from U, N and k alone (the workspace is sized without the model) ------------
// A workgroup's lists live across all of its item tiles, so its users are bounded by LDS: waves x (4 + 8 k) B per user inside
// kTopkStripeLds, next to the queues and whatever else the kernel keeps there.  The workgroups are equally long (the same users x tile
// rounds each), so the grid is what is resident at once and never a partial round more (one workgroup beyond what fits trails as long as
// a whole round).  That also caps the item stripes (one per wave) and with them the partial lists [stripes][U][k].
// `sample`: the call that seeds the thresholds.  Its lists fill from -inf -- k (1 + ln(n_stripe / k)) insertions per user and stripe -- so
// it runs FEW stripes (sample_gx workgroups along x) and spreads the users over the rest of the grid instead (the first form -- 32,768
// columns, as many stripes as the real call -- made the tower's whole call 3.4 ms longer at 1,024 users x 1 M items and 1.0 ms at 64).
constexpr size_t kTopkStripeLds = (size_t)64 * 1024;
struct topk_stripe_geom {
    int waves;                  // per workgroup: one item stripe each
    size_t reserved_lds;        // bytes of the budget taken by something else than lists and queues
    int64_t grid;               // workgroups per launch: what is resident at once
    int64_t sample_gx;          // workgroups along x of the sample call
    int round_to;               // users per workgroup: 0 = the groups evened out; n = a multiple of n where more than n fit
};
struct topk_stripe_plan { int upb; int64_t gx, gy, stripes; size_t lds; };

// columns of the sample that seeds the thresholds (catalogues of >= 8 x this): the real call then inserts ~k N / sample entries per user
constexpr int64_t topk_seed_cols(int k) { return (int64_t)1024 * (k < 8 ? 8 : k); }

inline topk_stripe_plan topk_make_stripe_plan(const topk_stripe_geom& g, int64_t U, int64_t N, int k, bool sample = false) {
    topk_stripe_plan p{};
    const size_t fixed = g.reserved_lds + sizeof(float) * (size_t)g.waves * 3 * kTopkStripeQueue;
    int64_t upb = (int64_t)((kTopkStripeLds - fixed) / (g.waves * sizeof(float) * (1 + 2 * (size_t)k)));
    if (g.round_to && upb > g.round_to) upb -= upb % g.round_to;
    if (upb > U) upb = U;
    if (sample) {
        const int64_t spread = (U + g.grid / g.sample_gx - 1) / (g.grid / g.sample_gx);
        if (upb > spread) upb = spread;
    }
    p.gy = (U + upb - 1) / upb;
    if (!g.round_to) {
        upb = (U + p.gy - 1) / p.gy;
        p.gy = (U + upb - 1) / upb;
    }
    p.upb = (int)upb;
    const int64_t wg_tiles = (((N + 31) >> 5) + g.waves - 1) / g.waves;
    int64_t gx = g.grid / p.gy;
    if (gx < 1) gx = 1;
    if (sample && gx > g.sample_gx) gx = g.sample_gx;
    if (gx > wg_tiles) gx = wg_tiles;
    p.gx = gx;
    p.stripes = g.waves * gx;
    p.lds = g.waves * sizeof(float) * topk_wave_words(p.upb, k);
    return p;
}

// stripes the workspace is laid out for: those of the real call, or of the sample call in front of it when that has more
inline int64_t topk_stripe_ws_stripes(const topk_stripe_geom& g, int64_t U, int64_t N, int k) {
    const int64_t s = topk_make_stripe_plan(g, U, N, k).stripes;
    const int64_t ss = N >= 8 * topk_seed_cols(k) ? topk_make_stripe_plan(g, U, topk_seed_cols(k), k, true).stripes : 0;
    return s > ss ? s : ss;
}

// level-0 lists (values | columns) | level-1 lists (one per kTopkMergeGroup level-0 lists)
inline size_t topk_stripe_ws_bytes(const topk_stripe_geom& g, int64_t U, int64_t N, int k) {
    const int64_t stripes = topk_stripe_ws_stripes(g, U, N, k);
    return 2 * topk_part_bytes(stripes, U, k) + 2 * topk_part_bytes((stripes + kTopkMergeGroup - 1) / kTopkMergeGroup, U, k);
}

// the *_topk_workspace_bytes entries
inline int topk_stripe_ws_query(const char* fn, const topk_stripe_geom& g, int64_t U, int64_t N, int k, size_t* bytes) {
    if (!(bytes && U > 0 && N > 0 && N < ((int64_t)1 << 31) && U < ((int64_t)1 << 31) && k >= 1 && k <= 64)) {
        cdr_set_error("%s: invalid argument: bytes && 0 < U, N < 2^31 && 1 <= k <= 64", fn);
        return CDR_EINVAL;
    }
    *bytes = topk_stripe_ws_bytes(g, U, N, k);
    return CDR_OK;
}

inline int topk_check_k(const char* fn, int k) {
    if (k < 1 || k > 64) { cdr_set_error("%s: k = %d outside 1..64", fn, k); return CDR_EINVAL; }
    return CDR_OK;
}

// The host tail of a *_fullsort_topk entry, behind its own argument checks: the remaining refusals, the workspace carve, the launches.
// launch(n_cols, plan, tk) -> int runs the entry's kernel over columns [0, n_cols) with plan's geometry and the lists of `tk`.
// SEEDED thresholds, as in cdr_fullsort_topk_f32: every stripe that fills its lists from -inf pays k (1 + ln(n_stripe / k)) insertions per
// user -- with ~1,000 items per stripe that was ~2 insertions per (tile, user), +45 % (CoNet's tower) to +160 % (DTCDR's) on the launch.
// A first call over a SAMPLE (the first topk_seed_cols(k) columns, same mask) leaves each user's k-th value over the sample in
// out_vals[:, k - 1]: a lower bound of the final one, the starting threshold (one float below: ties still enter) of every stripe of the
// real call.  Results are unchanged: every entry of the final top-k is >= its user's seed; short lists are padded with (-inf, -1), which
// the merge never takes.
template <class Launch>
int topk_seeded_run(const char* fn, const topk_stripe_geom& g, hipStream_t s, int64_t U, int64_t N, int k, const topk_mask& mask,
                    float* out_vals, int64_t* out_idx, void* workspace, size_t workspace_bytes, Launch&& launch) {
    if (const int rc = topk_check_k(fn, k)) return rc;
    const topk_stripe_plan p = topk_make_stripe_plan(g, U, N, k);
    if (p.gy > 65535 || topk_make_stripe_plan(g, U, topk_seed_cols(k), k, true).gy > 65535) {
        cdr_set_error("%s: %lld users at k = %d need more than 65,535 user groups; evaluate them in batches", fn, (long long)U, k);
        return CDR_EINVAL;
    }
    const size_t need = topk_stripe_ws_bytes(g, U, N, k);
    if (workspace_bytes < need) { cdr_set_error("%s: workspace %zu < %zu bytes", fn, workspace_bytes, need); return CDR_EINVAL; }
    const int64_t ws_stripes = topk_stripe_ws_stripes(g, U, N, k);
    const size_t part = topk_part_bytes(ws_stripes, U, k);
    const size_t part1 = topk_part_bytes((ws_stripes + kTopkMergeGroup - 1) / kTopkMergeGroup, U, k);
    float* pv = (float*)workspace;
    int* pc = (int*)((char*)workspace + part);
    float* pv1 = (float*)((char*)workspace + 2 * part);
    int* pc1 = (int*)((char*)workspace + 2 * part + part1);
    topk_out tk{k, 0, pv, pc, mask};
    if (N >= 8 * topk_seed_cols(k)) {
        const topk_stripe_plan sp = topk_make_stripe_plan(g, U, topk_seed_cols(k), k, true);    // (the workspace holds the larger of the two calls)
        int rc = launch(topk_seed_cols(k), sp, tk);
        if (rc) return rc;
        rc = topk_merge_launch(s, pv, pc, sp.stripes, U, k, pv1, pc1, out_vals, out_idx);
        if (rc) return rc;
        tk.seed = out_vals + (k - 1);
        tk.seed_stride = k;
    }
    const int rc = launch(N, p, tk);
    if (rc) return rc;
    return topk_merge_launch(s, pv, pc, p.stripes, U, k, pv1, pc1, out_vals, out_idx);
}

}  // namespace
