// v_mfma_f32_32x32x2_f32 helpers shared by the kernels that contract out of LDS (cdr_mapstep.hip, cdr_conet.hip) and the
// accumulator type of every MFMA kernel of the library.
#pragma once
#include "cdr_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}
// four weights of one row: one 16-byte load where the matrix is 16-byte aligned
__device__ __forceinline__ float4 ldw4(const float* p, bool vec) {
    return vec ? ld4(p) : make_float4(p[0], p[1], p[2], p[3]);
}
#define MFMA4(acc, a, b)                                                          \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32((a).x, (b).x, acc, 0, 0, 0);       \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32((a).y, (b).y, acc, 0, 0, 0);       \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32((a).z, (b).z, acc, 0, 0, 0);       \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32((a).w, (b).w, acc, 0, 0, 0)
#define MF1(acc, a, b) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0)

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt, i.e. waits for every global STORE of
// the phase (rows that nothing in the kernel reads back: ~1.5 us per CoNet layer, more than the small layers' MFMA time) and for
// every LDS DMA in flight (cdr_mapstep.hip's row waves).  Register results of global LOADS are still waited for by their consumers.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
