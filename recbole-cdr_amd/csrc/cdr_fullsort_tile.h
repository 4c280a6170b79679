// Host and device pieces the one-launch full-sort files share.  All three (cdr_conet_fullsort.hip, cdr_deepapf_fullsort.hip,
// cdr_natr_fullsort.hip) launch through tile_launch_one; DeepAPF and NATR, whose kernels are templated over <NB = padded width / 32,
// ITEMKEY, TOPK> and score 32-item tiles held in registers against user chunks in LDS, also share the row load, the instantiation switch
// and the score epilogue's grid.  One copy, internal linkage per translation unit.
#pragma once
#include "cdr_common.h"
#include <type_traits>

namespace {

// one item row's features h S .. h S + S - 1 (zero beyond D, or for a lane without an item)
template <int S>
__device__ __forceinline__ void tile_load_row(float (&p)[S], const float* __restrict__ row, bool iv, int h, int D) {
#pragma unroll
    for (int s = 0; s < S; s += 4) {
        const int f = h * S + s;
        const bool ok = iv && f < D;
        const float4 v = ld4(row + (ok ? f : 0));
        p[s] = ok ? v.x : 0.f; p[s + 1] = ok ? v.y : 0.f; p[s + 2] = ok ? v.z : 0.f; p[s + 3] = ok ? v.w : 0.f;
    }
}

// one launch; dynamic LDS above 48 KB has to be asked for per kernel
template <class Kern, class Args>
int tile_launch_one(const char* fn, Kern kern, const Args& a, dim3 grid, int block, size_t lds, hipStream_t s) {
    if (lds > (size_t)48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { cdr_set_error("%s: %zu B of LDS refused: %s", fn, lds, hipGetErrorString(e)); return CDR_EINVAL; }
    }
    kern<<<grid, dim3(block), lds, s>>>(a);
    CDR_LAUNCH_CHECK();
    return CDR_OK;
}

// the NB x ITEMKEY instantiation for width D: f(integral_constant<int, NB>, bool_constant<ITEMKEY>) -> int; -1 when D is out of range
template <class F>
int tile_dispatch(int D, bool itemkey, F&& f) {
    using std::integral_constant;
    switch ((D + 31) / 32 * 2 + (itemkey ? 1 : 0)) {
        case 2: return f(integral_constant<int, 1>{}, std::false_type{});
        case 3: return f(integral_constant<int, 1>{}, std::true_type{});
        case 4: return f(integral_constant<int, 2>{}, std::false_type{});
        case 5: return f(integral_constant<int, 2>{}, std::true_type{});
        case 6: return f(integral_constant<int, 3>{}, std::false_type{});
        case 7: return f(integral_constant<int, 3>{}, std::true_type{});
        case 8: return f(integral_constant<int, 4>{}, std::false_type{});
        case 9: return f(integral_constant<int, 4>{}, std::true_type{});
    }
    return -1;
}

// score epilogue: a few workgroups per CU, the waves walk the remaining tiles; the users (in whole LDS chunks of `chunk`) are split over
// blockIdx.y only while the item tiles alone do not fill the chip
inline int tile_score_grid(const char* fn, int64_t U, int64_t N, int waves, int chunk, dim3* grid, int* users_per_block) {
    const int64_t n_tiles = (N + 31) >> 5;
    int64_t gx = (n_tiles + waves - 1) / waves;
    const int64_t groups = (U + chunk - 1) / chunk;
    int64_t gy = 1;
    while (gx * gy < 2 * CDR_NUM_CU && gy < groups) gy *= 2;
    if (gy > groups) gy = groups;
    const int64_t per = (groups + gy - 1) / gy;
    gy = (groups + per - 1) / per;
    if (gy > 65535) { cdr_set_error("%s: %lld users need more than 65,535 user groups", fn, (long long)U); return CDR_EINVAL; }
    *users_per_block = (int)(per * chunk);
    if (gx > 4 * CDR_NUM_CU) gx = 4 * CDR_NUM_CU;
    *grid = dim3((unsigned)gx, (unsigned)gy);
    return CDR_OK;
}

}  // namespace
