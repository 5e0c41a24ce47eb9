// cf_sort.h -- the device sorts cf_prep.hip and cf_bpr.hip share.  Everything has internal linkage.
#pragma once

#include <cstring>   // rocprim's texture iterator calls memset without including it

#include <rocprim/rocprim.hpp>

namespace {

// Sorts run rocprim's stable merge-sort path at every size (radix_sort_config with an unbounded
// merge-sort limit).  Inside a PyTorch process this library is served by torch's bundled HIP
// runtime, under which rocprim's onesweep radix path fails to launch (hipErrorInvalidValue, in
// both its gfx950-tuned and generic configurations), while the merge path runs; standalone on
// the ROCm 7.2 runtime all of them run (tools/probe_sort.hip, 10.7M u64 keys + u32 values,
// 47 bits: onesweep 0.94 ms, merge sort 0.86 ms).
using SortCfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config,
                                           (size_t)1 << 40>;

template <class K, class V>
hipError_t sort_pairs(void* tmp, size_t& bytes, const K* ki, K* ko, const V* vi, V* vo, uint64_t n, int bits,
                      hipStream_t st) {
    return rocprim::radix_sort_pairs<SortCfg>(tmp, bytes, ki, ko, vi, vo, (unsigned int)n, 0u, (unsigned int)bits, st);
}
template <class K>
hipError_t sort_keys(void* tmp, size_t& bytes, const K* ki, K* ko, uint64_t n, int bits, hipStream_t st) {
    return rocprim::radix_sort_keys<SortCfg>(tmp, bytes, ki, ko, (unsigned int)n, 0u, (unsigned int)bits, st);
}

inline int bits_for(uint64_t n) {   // bits to represent 0 .. n-1 (>= 1)
    int b = 1;
    while (b < 64 && (1ull << b) < n) ++b;
    return b;
}

}  // namespace
