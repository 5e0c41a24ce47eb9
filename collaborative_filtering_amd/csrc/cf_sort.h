// cf_sort.h -- the device sorts of cf_prep.hip, cf_bpr.hip and cf_ease.hip, and the by-key lists (a
// device transpose) that the last two build from them.  Everything has internal linkage.
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

// ---- the lists of n entries by key, on the device ---------------------------------------------

constexpr int kSortT = 256;
inline unsigned sort_blocks(uint64_t n) { return (unsigned)((n + kSortT - 1) / kSortT); }

template <class T>
__global__ __launch_bounds__(kSortT) void iota_kernel(T* out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kSortT + threadIdx.x;
    if (i < n) out[i] = (T)i;
}

// off[i] = the first position of the sorted keys that holds a key >= i, i = 0 .. n_lists (keys
// above every list, such as the mark of a skipped entry, lie past off[n_lists]).
template <class K>
__global__ __launch_bounds__(kSortT) void key_offsets_kernel(const K* __restrict__ key, uint64_t n, uint32_t n_lists,
                                                            uint64_t* __restrict__ off) {
    const uint64_t i = (uint64_t)blockIdx.x * kSortT + threadIdx.x;
    if (i > n_lists) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)key[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    off[i] = lo;
}

// The entries 0 .. n-1 as a CSR by key[]: pos = the entries in a stable order of their keys (the
// entries of one list ascend), skey = the keys in that order, off = the n_lists + 1 offsets.
// tmp == nullptr asks for the bytes of tmp only, as sort_pairs does.  iota is n entries of scratch:
// filled here, or by the caller once for many calls (fill_iota = false).
inline hipError_t lists_by_key(void* tmp, size_t& bytes, const uint32_t* key, uint32_t* skey, uint32_t* iota,
                               bool fill_iota, uint32_t* pos, uint64_t n, uint32_t n_lists, uint64_t* off, int bits,
                               hipStream_t st) {
    if (!tmp) return sort_pairs(nullptr, bytes, key, skey, (const uint32_t*)iota, pos, n, bits, st);
    if (fill_iota) hipLaunchKernelGGL(iota_kernel<uint32_t>, dim3(sort_blocks(n)), dim3(kSortT), 0, st, iota, n);
    const hipError_t e = sort_pairs(tmp, bytes, key, skey, (const uint32_t*)iota, pos, n, bits, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(key_offsets_kernel<uint32_t>, dim3(sort_blocks((uint64_t)n_lists + 1)), dim3(kSortT), 0, st,
                       (const uint32_t*)skey, n, n_lists, off);
    return hipSuccess;
}

}  // namespace
