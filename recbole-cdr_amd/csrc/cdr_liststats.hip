// Non-accuracy metrics from the top-k lists (recbole's ItemCoverage / AveragePopularity / ShannonEntropy / GiniIndex / TailPercentage):
// the one accumulation they share.  A batch's lists idx [U, kmax] are folded into
//
//   rec_count [n_bucket, N]   how often item i was recommended at a position of bucket b (the distinct values of topk cut the positions into
//                             buckets; the count inside the first k positions is a prefix sum over buckets, taken by the caller)
//   col_pop / col_tail [kmax] the training-set counts / the tail flags of the items recommended at position j, summed over the users
//   n_bad [1]                 entries that could not be counted: an id >= N (or a position whose bucket is outside [0, n_bucket))
//
// by one launch, across batches, with integer atomics only: the buffers are bit-reproducible whatever the launch geometry or the batch cut.
//
// A workgroup walks tiles of whole rows (kListTile / kmax rows, at most kListTile entries), grid-stride; neighbouring lanes hold
// neighbouring positions of a row, so the id loads are contiguous 8-byte reads.  A lane has its tile entries' ids in flight before the
// first dependent gather (item_count, tail).  The histogram add is one 4-byte integer atomic per entry, spread over the catalogue by the ids themselves; the column totals -- every
// user adds to the same kmax addresses -- are summed in LDS first (two int64 arrays, 16 KB at kmax = 1024) and leave the workgroup as one
// 64-bit global add per column (guide G12).
#include "cdr_common.h"

namespace {

constexpr int kListMaxK = 1024;
constexpr int kListPerLane = 4;                       // entries a lane has in flight
constexpr int kListTile = kBlock * kListPerLane;      // entries per tile
static_assert(kListMaxK <= kListTile, "a tile holds at least one whole row");

__global__ __launch_bounds__(kBlock) void list_stats_kernel(const int64_t* __restrict__ idx, int64_t ld, int64_t U, int kmax,
                                                            const int32_t* __restrict__ pos_bucket, int n_bucket, int64_t N,
                                                            const int64_t* __restrict__ item_count, const uint8_t* __restrict__ tail,
                                                            int32_t* __restrict__ rec_count, int64_t* __restrict__ col_pop,
                                                            int64_t* __restrict__ col_tail, int64_t* __restrict__ n_bad,
                                                            int rows_per_tile, int64_t tiles) {
    __shared__ unsigned long long pop_s[kListMaxK];
    __shared__ unsigned long long tail_s[kListMaxK];
    __shared__ int bucket_s[kListMaxK];
    __shared__ unsigned bad_s;
    for (int j = threadIdx.x; j < kmax; j += kBlock) {
        pop_s[j] = 0; tail_s[j] = 0;
        bucket_s[j] = pos_bucket[j];
    }
    if (threadIdx.x == 0) bad_s = 0;
    __syncthreads();
    unsigned bad = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t row0 = t * rows_per_tile;                          // tile t: rows [row0, row0 + rows_per_tile) below U
        const int span = rows_per_tile * kmax;                           // <= kListTile
        int64_t id[kListPerLane];
        int pos[kListPerLane];
#pragma unroll
        for (int i = 0; i < kListPerLane; ++i) {
            const int e = threadIdx.x + i * kBlock;                      // entry of the tile
            const int r = e / kmax, j = e - r * kmax;
            const bool live = e < span && row0 + r < U;                  // then 0 <= j < kmax <= ld
            pos[i] = j;
            id[i] = live ? idx[(row0 + r) * ld + j] : -1;               // a pad
        }
        int64_t cnt[kListPerLane];
        unsigned tl[kListPerLane];
#pragma unroll
        for (int i = 0; i < kListPerLane; ++i) {
            const bool ok = id[i] >= 0 && id[i] < N;                     // the only ids anything is indexed with
            cnt[i] = ok ? item_count[id[i]] : 0;
            tl[i] = ok && tail ? tail[id[i]] : 0;
        }
#pragma unroll
        for (int i = 0; i < kListPerLane; ++i) {
            if (id[i] < 0) continue;
            const int b = bucket_s[pos[i]];
            if (id[i] >= N || b < 0 || b >= n_bucket) { ++bad; continue; }
            atomicAdd(rec_count + (int64_t)b * N + id[i], 1);
            if (cnt[i]) atomicAdd(pop_s + pos[i], (unsigned long long)cnt[i]);
            if (tl[i]) atomicAdd(tail_s + pos[i], (unsigned long long)tl[i]);
        }
    }
    if (bad) atomicAdd(&bad_s, bad);
    __syncthreads();
    for (int j = threadIdx.x; j < kmax; j += kBlock) {
        if (pop_s[j]) atomicAdd((unsigned long long*)col_pop + j, pop_s[j]);
        if (col_tail && tail_s[j]) atomicAdd((unsigned long long*)col_tail + j, tail_s[j]);
    }
    if (threadIdx.x == 0 && bad_s) atomicAdd((unsigned long long*)n_bad, (unsigned long long)bad_s);
}

}  // namespace

extern "C" int cdr_list_stats_accumulate(void* stream, const int64_t* idx, int64_t ld, int64_t U, int kmax, const int32_t* pos_bucket,
                                         int n_bucket, int64_t N, const int64_t* item_count, const uint8_t* tail, int32_t* rec_count,
                                         int64_t* col_pop, int64_t* col_tail, int64_t* n_bad) {
    CDR_CHECK_ARG(kmax >= 1 && kmax <= kListMaxK && U >= 0 && U < ((int64_t)1 << 30) && ld >= kmax);
    CDR_CHECK_ARG(N >= 1 && N < ((int64_t)1 << 31) && n_bucket >= 1 && n_bucket <= kmax);
    CDR_CHECK_ARG(pos_bucket && item_count && rec_count && col_pop && n_bad);
    CDR_CHECK_ARG((tail == nullptr) == (col_tail == nullptr));
    if (U == 0) return CDR_OK;
    CDR_CHECK_ARG(idx);
    const int rows_per_tile = kListTile / kmax;                          // >= 1
    const int64_t tiles = (U + rows_per_tile - 1) / rows_per_tile;
    list_stats_kernel<<<dim3((unsigned)grid_for(tiles, 1)), dim3(kBlock), 0, (hipStream_t)stream>>>(
        idx, ld, U, kmax, pos_bucket, n_bucket, N, item_count, tail, rec_count, col_pop, col_tail, n_bad, rows_per_tile, tiles);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}
