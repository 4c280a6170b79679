// The counter-based dropout mask of the library (cdr_graph.hip: dropout_kernel / dropout_dev_kernel / the transfer kernels with the
// dropout folded in; cdr_dtcdr.hip: the NeuMF tower's layers): element e of a call keeps iff splitmix64(seed + (e + 1) * golden) maps to
// a uniform >= p.  One copy of the hash, so that every kernel that regenerates a mask draws the same (seed, salt, element) -> keep mapping.
#pragma once
#include <stdint.h>

// the seed of one mask of a step whose counter lives in DEVICE memory: consecutive counters -> unrelated seeds; `salt` separates the
// masks of one step (layer, domain)
__device__ __forceinline__ uint64_t cdr_drop_seed_dev(const int64_t* seed_dev, uint64_t salt) {
    uint64_t s0 = (uint64_t)seed_dev[0] * 0xD1342543DE82EF95ull + 0x9E3779B97F4A7C15ull;
    s0 = (s0 ^ (s0 >> 30)) * 0xBF58476D1CE4E5B9ull;
    s0 = (s0 ^ (s0 >> 27)) * 0x94D049BB133111EBull;
    return (s0 ^ (s0 >> 31)) + salt * 0xA24BAED4963EE407ull;
}

// 24 uniform bits in [0,1) for element e of the mask `seed`
__device__ __forceinline__ float cdr_drop_uniform(uint64_t seed, int64_t e) {
    uint64_t z = seed + (uint64_t)(e + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (float)(z >> 40) * (1.0f / 16777216.0f);
}
