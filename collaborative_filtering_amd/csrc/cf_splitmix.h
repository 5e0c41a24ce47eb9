// cf_splitmix.h -- the one splitmix64 of the device library (the host's is host/cf_mf_cli.hpp): the
// negative sampler of cf_bpr.hip and the random order keys of cf_split.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

__host__ __device__ inline uint64_t splitmix64(uint64_t x) {   // host/cf_mf_cli.hpp
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
