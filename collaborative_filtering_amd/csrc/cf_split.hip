// cf_split.hip -- per-user hold-out split and k-core filter on the GPU (cf_kcore, cf_holdout_split;
// the semantics are stated in cf_abi.h).  Integers only: no floating point anywhere in this file.
//
// Over the edges in read order (compact ids):
//   1. key = user << 32 | item, stable sort of (key, index): equal keys keep read order, so the
//      last edge of a run is the one that stays (alive[j] = 1, j = the position in this order).
//      The users' lists are the runs of this order (offsets by binary search); the items' lists
//      come from lists_by_key over the kept positions (a dropped edge carries the mark n_items).
//   2. a core round: the degree of every vertex is the alive entries of its list, one wave per
//      list, both sides the same kernel; a list above kLongList entries is left to a second kernel
//      that spreads it over many workgroups (integer atomics).  The kill pass clears alive[j]
//      where an end is below its limit and sets the word that the host reads back.
//   3. order within a user, the LSD way: the positions are in (user, item) order already; a stable
//      sort by the 64-bit order key, then a stable sort by user (dead edges under the mark
//      n_users) leaves every user's alive edges together, by (key, item).
//   4. part from the position in the user's run and its length; the counts of the stats are sums
//      of per-user and per-item terms, reduced per workgroup and then by one workgroup in index
//      order.
// Bytes: about 12 B per edge in and out of each of the four sorts, plus 5 B per alive edge and
// round; at the sizes of data prep (10^7 edges) everything but the sorts is launch-bound.

#include <hipcub/hipcub.hpp>

#include "cf_internal.h"
#include "cf_prep_scratch.h"
#include "cf_sort.h"
#include "cf_splitmix.h"

namespace {

constexpr uint32_t kLongList = 2048;   // entries above which a list is counted by degree_long_kernel
constexpr int kLongBlocks = 64;        // workgroups that share one long list
constexpr uint32_t kLongRows = 64;     // long lists per pass of degree_long_kernel's grid
constexpr int kT = 256;
constexpr unsigned kListBlocks = 65536;   // cap of the wave-per-list grid (4 lists per workgroup and pass)
constexpr unsigned kStatBlocks = 256;
constexpr int kStatTerms = 5;

struct SplitRule {
    int mode;
    uint32_t a, b, min_train;
};

// word[0] = 1 when an id is out of range (such an edge gets key 0: nothing is indexed by it before
// the call fails)
__global__ void split_keys_kernel(uint64_t n, const uint32_t* __restrict__ user, const uint32_t* __restrict__ item,
                                  uint32_t n_users, uint32_t n_items, uint64_t* __restrict__ key,
                                  uint32_t* __restrict__ idx, uint32_t* word) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t u = user[i], m = item[i];
        const bool bad = u >= n_users || m >= n_items;
        if (bad) word[0] = 1u;
        key[i] = bad ? 0ull : ((uint64_t)u << 32 | m);
        idx[i] = (uint32_t)i;
    }
}

// position j of the sorted keys: alive = the last of its run; its user; its item, or the mark
// n_items for a dropped edge (the key of lists_by_key)
__global__ void split_runs_kernel(uint64_t n, const uint64_t* __restrict__ key, uint32_t n_items,
                                  uint8_t* __restrict__ alive, uint32_t* __restrict__ suser,
                                  uint32_t* __restrict__ ikey) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = key[j];
        const bool last = j + 1 == n || key[j + 1] != k;
        alive[j] = last ? 1 : 0;
        suser[j] = (uint32_t)(k >> 32);
        ikey[j] = last ? (uint32_t)k : n_items;
    }
}

// the lists above kLongList entries: longv[0 .. *n_long) in no particular order (their counts are
// integer sums)
__global__ void long_lists_kernel(uint32_t n_lists, const uint64_t* __restrict__ off, uint32_t* __restrict__ longv,
                                  uint32_t* n_long) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_lists; v += (uint64_t)gridDim.x * blockDim.x)
        if (off[v + 1] - off[v] > kLongList) longv[atomicAdd(n_long, 1u)] = (uint32_t)v;
}

// deg[v] = the alive entries of list v, one wave per list; pos == nullptr: the entries are the
// positions off[v] .. off[v + 1) themselves (the users' lists).  A long list gets 0 here.
__global__ __launch_bounds__(kT) void degree_kernel(uint32_t n_lists, const uint64_t* __restrict__ off,
                                                    const uint32_t* __restrict__ pos,
                                                    const uint8_t* __restrict__ alive, uint32_t* __restrict__ deg) {
    const int lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (kT / 64);
    for (uint64_t v = (uint64_t)blockIdx.x * (kT / 64) + (threadIdx.x >> 6); v < n_lists; v += waves) {
        const uint64_t b = off[v], e = off[v + 1];
        uint32_t c = 0;
        if (e - b <= kLongList)
            for (uint64_t p = b + lane; p < e; p += 64) c += alive[pos ? pos[p] : p];
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0) deg[v] = c;
    }
}

// the long lists: kLongBlocks workgroups (blockIdx.x) share list longv[blockIdx.y]
__global__ __launch_bounds__(kT) void degree_long_kernel(uint32_t n_long, const uint32_t* __restrict__ longv,
                                                         const uint64_t* __restrict__ off,
                                                         const uint32_t* __restrict__ pos,
                                                         const uint8_t* __restrict__ alive, uint32_t* deg) {
    using Reduce = hipcub::BlockReduce<uint32_t, kT>;
    __shared__ typename Reduce::TempStorage tmp;
    for (uint32_t lv = blockIdx.y; lv < n_long; lv += gridDim.y) {
        const uint32_t v = longv[lv];
        const uint64_t b = off[v], e = off[v + 1];
        uint32_t c = 0;
        for (uint64_t p = b + (uint64_t)blockIdx.x * kT + threadIdx.x; p < e; p += (uint64_t)gridDim.x * kT)
            c += alive[pos ? pos[p] : p];
        const uint32_t sum = Reduce(tmp).Sum(c);
        if (threadIdx.x == 0 && sum) atomicAdd(&deg[v], sum);
        __syncthreads();
    }
}

__global__ void kill_kernel(uint64_t n, const uint64_t* __restrict__ key, const uint32_t* __restrict__ udeg,
                            const uint32_t* __restrict__ ideg, uint32_t min_user, uint32_t min_item,
                            uint8_t* __restrict__ alive, uint32_t* died) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        if (!alive[j]) continue;
        const uint64_t k = key[j];
        if (udeg[k >> 32] < min_user || ideg[(uint32_t)k] < min_item) {
            alive[j] = 0;
            *died = 1u;
        }
    }
}

__global__ void keep_scatter_kernel(uint64_t n, const uint32_t* __restrict__ idx, const uint8_t* __restrict__ alive,
                                    uint8_t* __restrict__ keep) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
        keep[idx[j]] = alive[j];
}

// the order key of position j: the caller's, of the edge that stayed, or the hash of its ids
// (seed_m = splitmix64(seed))
__global__ void order_keys_kernel(uint64_t n, const uint64_t* __restrict__ key, const uint32_t* __restrict__ idx,
                                  const uint64_t* __restrict__ order_key, uint64_t seed_m, uint64_t* __restrict__ okey) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = key[j];
        okey[j] = order_key ? order_key[idx[j]] : splitmix64(splitmix64(seed_m ^ (k >> 32)) ^ (uint64_t)(uint32_t)k);
    }
}

// the key of the second sort: the user of the position at rank q of the first, n_users when dead
__global__ void order_users_kernel(uint64_t n, const uint32_t* __restrict__ v, const uint64_t* __restrict__ key,
                                   const uint8_t* __restrict__ alive, uint32_t n_users, uint32_t* __restrict__ ukey) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t j = v[q];
        ukey[q] = alive[j] ? (uint32_t)(key[j] >> 32) : n_users;
    }
}

__device__ __forceinline__ uint64_t held_of(uint64_t nu, const SplitRule& r) {   // h_u of the hold-out modes
    const uint64_t t = nu > r.min_train ? nu - r.min_train : 0;
    const uint64_t h = r.mode == CF_SPLIT_LEAVE_K ? (uint64_t)r.a : nu * (uint64_t)r.a / (uint64_t)r.b;
    return h < t ? h : t;
}

// rank r of the final order -> the part of its edge, stored at the edge's read index; the items
// seen alive and seen in TRAIN are marked (every writer of a mark stores the same 1)
__global__ void parts_kernel(uint64_t n, const uint32_t* __restrict__ skey, const uint32_t* __restrict__ v,
                             const uint32_t* __restrict__ idx, const uint64_t* __restrict__ key,
                             const uint64_t* __restrict__ uoff, uint32_t n_users, SplitRule rule,
                             uint8_t* __restrict__ part, uint32_t* ialive, uint32_t* itrain) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t u = skey[r], j = v[r], i = idx[j];
        if (u >= n_users) {
            part[i] = CF_SPLIT_DROPPED;
            continue;
        }
        const uint64_t b = uoff[u], p = r - b, nu = uoff[u + 1] - b;
        const uint32_t pt = rule.mode == CF_SPLIT_FOLDS ? (uint32_t)(p % rule.a) : (p < held_of(nu, rule) ? 1u : 0u);
        part[i] = (uint8_t)pt;
        const uint32_t m = (uint32_t)key[j];
        ialive[m] = 1u;
        if (rule.mode != CF_SPLIT_FOLDS && pt == 0) itrain[m] = 1u;
    }
}

// the terms of the stats by vertex: users alive, edges of part 0, of part 1 (closed forms of n_u),
// items alive, alive items without a TRAIN edge; partial[blockIdx.x * kStatTerms + t]
__global__ __launch_bounds__(kT) void stats_partial_kernel(uint32_t n_users, uint32_t n_items,
                                                           const uint64_t* __restrict__ uoff, SplitRule rule,
                                                           const uint32_t* __restrict__ ialive,
                                                           const uint32_t* __restrict__ itrain,
                                                           uint64_t* __restrict__ partial) {
    using Reduce = hipcub::BlockReduce<uint64_t, kT>;
    __shared__ typename Reduce::TempStorage tmp;
    uint64_t s[kStatTerms] = {0, 0, 0, 0, 0};
    const uint64_t stride = (uint64_t)gridDim.x * kT, t0 = (uint64_t)blockIdx.x * kT + threadIdx.x;
    for (uint64_t u = t0; u < n_users; u += stride) {
        const uint64_t nu = uoff[u + 1] - uoff[u];
        if (!nu) continue;
        s[0] += 1;
        if (rule.mode == CF_SPLIT_FOLDS) {   // positions p < n_u with p mod F == 0, == 1
            s[1] += (nu + rule.a - 1) / rule.a;
            s[2] += (nu + rule.a - 2) / rule.a;
        } else {
            const uint64_t h = held_of(nu, rule);
            s[1] += nu - h;
            s[2] += h;
        }
    }
    for (uint64_t m = t0; m < n_items; m += stride) {
        if (!ialive[m]) continue;
        s[3] += 1;
        if (rule.mode != CF_SPLIT_FOLDS && !itrain[m]) s[4] += 1;
    }
    for (int t = 0; t < kStatTerms; ++t) {
        const uint64_t sum = Reduce(tmp).Sum(s[t]);
        if (threadIdx.x == 0) partial[(uint64_t)blockIdx.x * kStatTerms + t] = sum;
        __syncthreads();
    }
}

// one workgroup: the partial sums in index order; kept = the end of the items' lists, alive = the
// end of the users' runs
__global__ void stats_final_kernel(unsigned n_blocks, const uint64_t* __restrict__ partial,
                                   const uint64_t* __restrict__ ioff, uint32_t n_items,
                                   const uint64_t* __restrict__ uoff, uint32_t n_users, uint32_t rounds,
                                   uint64_t* __restrict__ stats) {
    const unsigned t = threadIdx.x;
    if (t < (unsigned)kStatTerms) {
        uint64_t s = 0;
        for (unsigned b = 0; b < n_blocks; ++b) s += partial[(uint64_t)b * kStatTerms + t];
        stats[t == 0 ? 2 : t == 1 ? 4 : t == 2 ? 5 : t == 3 ? 3 : 6] = s;
    } else if (t == (unsigned)kStatTerms) {
        stats[0] = ioff[n_items];
        stats[1] = uoff[n_users];
        stats[7] = rounds;
    }
}

unsigned list_grid(uint64_t n_lists) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_lists + kT / 64 - 1) / (kT / 64), kListBlocks));
}

// What both calls share: the scratch layout and steps 1-2.
struct SplitWork {
    uint64_t *key_a, *key_b, *key_c, *uoff, *ioff, *uoff2, *partial;
    uint32_t *idx_a, *idx_b, *suser, *ikey, *iskey, *ipos, *v2, *v3, *udeg, *ideg, *ulong, *ilong, *ialive, *itrain,
        *words;   // words: [0] bad id, [1] long user lists, [2] long item lists, [3] died
    uint8_t* alive;
    void* tmp;
    size_t tmp_bytes;
};

size_t split_tmp_bytes(uint64_t n, int bits_key, int bits_item, int bits_user, hipStream_t st) {
    size_t a = 0, b = 0, c = 0, d = 0;
    (void)sort_pairs(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                     (uint32_t*)nullptr, n, bits_key, st);
    (void)sort_pairs(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                     (uint32_t*)nullptr, n, bits_item, st);
    (void)sort_pairs(nullptr, c, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                     (uint32_t*)nullptr, n, 64, st);
    (void)sort_pairs(nullptr, d, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                     (uint32_t*)nullptr, n, bits_user, st);
    return std::max({a, b, c, d}) + 4096;
}

int split_events(cf_ctx* ctx) {
    CF_TRY(prep_events(ctx));
    for (hipEvent_t& e : ctx->split_ev)
        if (!e) CF_HIP_CHECK(ctx, hipEventCreate(&e));
    return CF_OK;
}

int split_args(cf_ctx* ctx, const char* fn, uint64_t n) {
    if (n >= (1ull << 31)) return cf_set_error(ctx, CF_ERANGE, std::string(fn) + ": more than 2^31 edges");
    return CF_OK;
}

int split_rule_check(cf_ctx* ctx, const char* fn, const SplitRule& r) {
    if (r.mode == CF_SPLIT_LEAVE_K) return CF_OK;
    if (r.mode == CF_SPLIT_RATIO) {
        if (r.a == 0 || r.a >= r.b) return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": the ratio a / b needs 0 < a < b");
        return CF_OK;
    }
    if (r.mode == CF_SPLIT_FOLDS) {
        if (r.a < 2 || r.a > 254) return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": folds outside 2 .. 254");
        return CF_OK;
    }
    return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": unknown mode");
}

// Steps 1-2 on the stream: W carved and filled, alive[] final, *rounds set; n > 0.  Records
// split_ev[0 .. 2] and prep_ev[0].
int split_core(cf_ctx* ctx, const char* fn, uint64_t n, uint32_t n_users, uint32_t n_items, const uint32_t* d_user,
               const uint32_t* d_item, uint32_t min_user, uint32_t min_item, SplitWork& W, uint32_t* rounds,
               hipStream_t st) {
    const int bits_key = 32 + bits_for(n_users), bits_item = bits_for((uint64_t)n_items + 1),
              bits_user = bits_for((uint64_t)n_users + 1);
    const size_t cub = split_tmp_bytes(n, bits_key, bits_item, bits_user, st);
    const uint64_t n_long_cap = n / kLongList + 1;
    const auto carve = [&](char* base, SplitWork& L) {
        Carve cv{base};
        L.key_a = cv.take<uint64_t>(n);
        L.key_b = cv.take<uint64_t>(n);
        L.key_c = cv.take<uint64_t>(n);
        L.idx_a = cv.take<uint32_t>(n);
        L.idx_b = cv.take<uint32_t>(n);
        L.suser = cv.take<uint32_t>(n);
        L.ikey = cv.take<uint32_t>(n);
        L.iskey = cv.take<uint32_t>(n);
        L.ipos = cv.take<uint32_t>(n);
        L.v2 = cv.take<uint32_t>(n);
        L.v3 = cv.take<uint32_t>(n);
        L.alive = cv.take<uint8_t>(n);
        L.uoff = cv.take<uint64_t>((uint64_t)n_users + 1);
        L.uoff2 = cv.take<uint64_t>((uint64_t)n_users + 1);
        L.ioff = cv.take<uint64_t>((uint64_t)n_items + 1);
        L.udeg = cv.take<uint32_t>(n_users);
        L.ideg = cv.take<uint32_t>(n_items);
        L.ulong = cv.take<uint32_t>(n_long_cap);
        L.ilong = cv.take<uint32_t>(n_long_cap);
        L.ialive = cv.take<uint32_t>(n_items);
        L.itrain = cv.take<uint32_t>(n_items);
        L.partial = cv.take<uint64_t>((size_t)kStatBlocks * kStatTerms);
        L.words = cv.take<uint32_t>(4);
        L.tmp = cv.take<char>(cub);
        L.tmp_bytes = cub;
        return cv.used;
    };
    CF_TRY(prep_reserve(ctx, carve(nullptr, W)));
    if (carve(static_cast<char*>(ctx->d_prep), W) > ctx->prep_bytes)
        return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": scratch layout exceeds the reservation");
    const dim3 G = grid_for(n), B(kT);
    size_t tb = W.tmp_bytes;
    CF_HIP_CHECK(ctx, hipEventRecord(ctx->prep_ev[0], st));
    CF_HIP_CHECK(ctx, hipEventRecord(ctx->split_ev[0], st));
    // ---- 1. the last of every (user, item), the lists of both sides ------------------------
    CF_HIP_CHECK(ctx, hipMemsetAsync(W.words, 0, 4 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(split_keys_kernel, G, B, 0, st, n, d_user, d_item, n_users, n_items, W.key_a, W.idx_a, W.words);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, sort_pairs(W.tmp, tb, W.key_a, W.key_b, W.idx_a, W.idx_b, n, bits_key, st));
    hipLaunchKernelGGL(split_runs_kernel, G, B, 0, st, n, W.key_b, n_items, W.alive, W.suser, W.ikey);
    hipLaunchKernelGGL(key_offsets_kernel<uint32_t>, dim3(sort_blocks((uint64_t)n_users + 1)), dim3(kSortT), 0, st,
                       (const uint32_t*)W.suser, n, n_users, W.uoff);
    // idx_a is the identity already: the entries of the items' lists are positions of the sorted order
    CF_HIP_CHECK(ctx, lists_by_key(W.tmp, tb, W.ikey, W.iskey, W.idx_a, false, W.ipos, n, n_items, W.ioff, bits_item, st));
    const bool core_u = min_user > 1, core_i = min_item > 1;
    if (core_u)
        hipLaunchKernelGGL(long_lists_kernel, grid_for(n_users), B, 0, st, n_users, W.uoff, W.ulong, W.words + 1);
    if (core_i)
        hipLaunchKernelGGL(long_lists_kernel, grid_for(n_items), B, 0, st, n_items, W.ioff, W.ilong, W.words + 2);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipEventRecord(ctx->split_ev[1], st));
    uint32_t h_words[4] = {0, 0, 0, 0};
    CF_HIP_CHECK(ctx, hipMemcpyAsync(h_words, W.words, sizeof(h_words), hipMemcpyDeviceToHost, st));
    CF_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (h_words[0]) {
        CF_HIP_CHECK(ctx, hipEventRecord(ctx->prep_ev[1], st));   // cf_prep_timing stays a pair of one call
        return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": user or item id out of range");
    }
    // ---- 2. the core ---------------------------------------------------------------------
    *rounds = 0;
    if (core_u || core_i) {
        // a side without a limit is never counted: its degrees stay 0 against a limit of 0
        if (!core_u) CF_HIP_CHECK(ctx, hipMemsetAsync(W.udeg, 0, sizeof(uint32_t) * (size_t)n_users, st));
        if (!core_i) CF_HIP_CHECK(ctx, hipMemsetAsync(W.ideg, 0, sizeof(uint32_t) * (size_t)n_items, st));
        const uint32_t lim_u = core_u ? min_user : 0, lim_i = core_i ? min_item : 0;
        const uint32_t n_ulong = h_words[1], n_ilong = h_words[2];
        for (;;) {
            CF_HIP_CHECK(ctx, hipMemsetAsync(W.words + 3, 0, sizeof(uint32_t), st));
            if (core_u) {
                hipLaunchKernelGGL(degree_kernel, dim3(list_grid(n_users)), B, 0, st, n_users, W.uoff,
                                   (const uint32_t*)nullptr, W.alive, W.udeg);
                if (n_ulong)
                    hipLaunchKernelGGL(degree_long_kernel, dim3(kLongBlocks, std::min(n_ulong, kLongRows)), B, 0, st,
                                       n_ulong, W.ulong, W.uoff, (const uint32_t*)nullptr, W.alive, W.udeg);
            }
            if (core_i) {
                hipLaunchKernelGGL(degree_kernel, dim3(list_grid(n_items)), B, 0, st, n_items, W.ioff, W.ipos, W.alive,
                                   W.ideg);
                if (n_ilong)
                    hipLaunchKernelGGL(degree_long_kernel, dim3(kLongBlocks, std::min(n_ilong, kLongRows)), B, 0, st,
                                       n_ilong, W.ilong, W.ioff, W.ipos, W.alive, W.ideg);
            }
            hipLaunchKernelGGL(kill_kernel, G, B, 0, st, n, W.key_b, W.udeg, W.ideg, lim_u, lim_i, W.alive, W.words + 3);
            CF_HIP_CHECK(ctx, hipGetLastError());
            uint32_t died = 0;
            CF_HIP_CHECK(ctx, hipMemcpyAsync(&died, W.words + 3, sizeof(died), hipMemcpyDeviceToHost, st));
            CF_HIP_CHECK(ctx, hipStreamSynchronize(st));
            if (!died) break;
            ++*rounds;
        }
    }
    CF_HIP_CHECK(ctx, hipEventRecord(ctx->split_ev[2], st));
    return CF_OK;
}

}  // namespace

int cf_kcore_run(cf_ctx* ctx, uint64_t n, uint32_t n_users, uint32_t n_items, const uint32_t* d_user,
                 const uint32_t* d_item, uint32_t min_user, uint32_t min_item, uint8_t* d_keep, uint32_t* rounds,
                 void* stream_) {
    if (!ctx) return CF_EINVAL;
    CF_TRY(split_args(ctx, "cf_kcore_run", n));
    if (!rounds || (n && (!d_user || !d_item || !d_keep))) return cf_set_error(ctx, CF_EINVAL, "cf_kcore_run: null argument");
    CF_TRY(set_device(ctx));
    CF_TRY(split_events(ctx));
    hipStream_t st = (hipStream_t)stream_;
    *rounds = 0;
    ctx->split_steps = 0;
    if (n == 0) {
        CF_HIP_CHECK(ctx, hipEventRecord(ctx->prep_ev[0], st));
        CF_HIP_CHECK(ctx, hipEventRecord(ctx->prep_ev[1], st));
        return CF_OK;
    }
    SplitWork W{};
    CF_TRY(split_core(ctx, "cf_kcore_run", n, n_users, n_items, d_user, d_item, min_user, min_item, W, rounds, st));
    hipLaunchKernelGGL(keep_scatter_kernel, grid_for(n), dim3(kT), 0, st, n, W.idx_b, W.alive, d_keep);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipEventRecord(ctx->prep_ev[1], st));
    CF_HIP_CHECK(ctx, hipStreamSynchronize(st));
    ctx->split_steps = 2;
    return CF_OK;
}

int cf_holdout_split_run(cf_ctx* ctx, uint64_t n, uint32_t n_users, uint32_t n_items, const uint32_t* d_user,
                         const uint32_t* d_item, const uint64_t* d_order_key, uint64_t seed, uint32_t min_user,
                         uint32_t min_item, int mode, uint32_t a, uint32_t b, uint32_t min_train, uint8_t* d_part,
                         uint64_t* d_stats, void* stream_) {
    if (!ctx) return CF_EINVAL;
    CF_TRY(split_args(ctx, "cf_holdout_split_run", n));
    const SplitRule rule{mode, a, b, min_train};
    CF_TRY(split_rule_check(ctx, "cf_holdout_split_run", rule));
    if (n && (!d_user || !d_item || !d_part)) return cf_set_error(ctx, CF_EINVAL, "cf_holdout_split_run: null argument");
    CF_TRY(set_device(ctx));
    CF_TRY(split_events(ctx));
    hipStream_t st = (hipStream_t)stream_;
    ctx->split_steps = 0;
    if (n == 0) {
        CF_HIP_CHECK(ctx, hipEventRecord(ctx->prep_ev[0], st));
        if (d_stats) CF_HIP_CHECK(ctx, hipMemsetAsync(d_stats, 0, sizeof(uint64_t) * CF_SPLIT_STATS, st));
        CF_HIP_CHECK(ctx, hipEventRecord(ctx->prep_ev[1], st));
        CF_HIP_CHECK(ctx, hipStreamSynchronize(st));
        return CF_OK;
    }
    SplitWork W{};
    uint32_t rounds = 0;
    CF_TRY(split_core(ctx, "cf_holdout_split_run", n, n_users, n_items, d_user, d_item, min_user, min_item, W, &rounds, st));
    const dim3 G = grid_for(n), B(kT);
    size_t tb = W.tmp_bytes;
    // ---- 3. (user, key, item) order: stable by key over the (user, item) order, then by user ----
    hipLaunchKernelGGL(order_keys_kernel, G, B, 0, st, n, W.key_b, W.idx_b, d_order_key, splitmix64(seed), W.key_a);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, sort_pairs(W.tmp, tb, W.key_a, W.key_c, W.idx_a, W.v2, n, 64, st));
    hipLaunchKernelGGL(order_users_kernel, G, B, 0, st, n, W.v2, W.key_b, W.alive, n_users, W.ikey);
    CF_HIP_CHECK(ctx, sort_pairs(W.tmp, tb, W.ikey, W.iskey, W.v2, W.v3, n, bits_for((uint64_t)n_users + 1), st));
    hipLaunchKernelGGL(key_offsets_kernel<uint32_t>, dim3(sort_blocks((uint64_t)n_users + 1)), dim3(kSortT), 0, st,
                       (const uint32_t*)W.iskey, n, n_users, W.uoff2);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipEventRecord(ctx->split_ev[3], st));
    // ---- 4. parts and stats ------------------------------------------------------------------
    CF_HIP_CHECK(ctx, hipMemsetAsync(W.ialive, 0, sizeof(uint32_t) * (size_t)n_items, st));
    CF_HIP_CHECK(ctx, hipMemsetAsync(W.itrain, 0, sizeof(uint32_t) * (size_t)n_items, st));
    hipLaunchKernelGGL(parts_kernel, G, B, 0, st, n, W.iskey, W.v3, W.idx_b, W.key_b, W.uoff2, n_users, rule, d_part,
                       W.ialive, W.itrain);
    if (d_stats) {
        const unsigned blocks = (unsigned)std::max<uint64_t>(
            1, std::min<uint64_t>(((uint64_t)std::max(n_users, n_items) + kT - 1) / kT, kStatBlocks));
        hipLaunchKernelGGL(stats_partial_kernel, dim3(blocks), B, 0, st, n_users, n_items, W.uoff2, rule, W.ialive,
                           W.itrain, W.partial);
        hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(64), 0, st, blocks, W.partial, W.ioff, n_items, W.uoff2,
                           n_users, rounds, d_stats);
    }
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipEventRecord(ctx->split_ev[4], st));
    CF_HIP_CHECK(ctx, hipEventRecord(ctx->prep_ev[1], st));
    CF_HIP_CHECK(ctx, hipStreamSynchronize(st));
    ctx->split_steps = 4;
    return CF_OK;
}

namespace {

int split_host_check(cf_ctx* ctx, const char* fn, uint64_t n, uint32_t n_users, uint32_t n_items, const uint32_t* user,
                     const uint32_t* item, const void* out) {
    if (n && (!user || !item || !out)) return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": null argument");
    for (uint64_t i = 0; i < n; ++i)
        if (user[i] >= n_users || item[i] >= n_items)
            return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": user or item id out of range");
    return CF_OK;
}

}  // namespace

int cf_kcore(cf_ctx* ctx, uint64_t n, uint32_t n_users, uint32_t n_items, const uint32_t* user, const uint32_t* item,
             uint32_t min_user, uint32_t min_item, uint8_t* keep, uint32_t* rounds) {
    if (!ctx) return CF_EINVAL;
    CF_TRY(split_args(ctx, "cf_kcore", n));
    if (!rounds) return cf_set_error(ctx, CF_EINVAL, "cf_kcore: null argument");
    CF_TRY(split_host_check(ctx, "cf_kcore", n, n_users, n_items, user, item, keep));
    CF_TRY(set_device(ctx));
    DevBuf du, dm, dk;
    int rc = dev_alloc(ctx, du, 4 * n);
    if (rc == CF_OK) rc = dev_alloc(ctx, dm, 4 * n);
    if (rc == CF_OK) rc = dev_alloc(ctx, dk, n);
    if (rc != CF_OK) return rc;
    if (n) {
        CF_HIP_CHECK(ctx, hipMemcpy(du.p, user, 4 * n, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy(dm.p, item, 4 * n, hipMemcpyHostToDevice));
    }
    CF_TRY(cf_kcore_run(ctx, n, n_users, n_items, (const uint32_t*)du.p, (const uint32_t*)dm.p, min_user, min_item,
                        (uint8_t*)dk.p, rounds, nullptr));
    CF_HIP_CHECK(ctx, hipDeviceSynchronize());
    if (n) CF_HIP_CHECK(ctx, hipMemcpy(keep, dk.p, n, hipMemcpyDeviceToHost));
    return CF_OK;
}

int cf_holdout_split(cf_ctx* ctx, uint64_t n, uint32_t n_users, uint32_t n_items, const uint32_t* user,
                     const uint32_t* item, const uint64_t* order_key, uint64_t seed, uint32_t min_user,
                     uint32_t min_item, int mode, uint32_t a, uint32_t b, uint32_t min_train, uint8_t* part,
                     uint64_t* stats) {
    if (!ctx) return CF_EINVAL;
    CF_TRY(split_args(ctx, "cf_holdout_split", n));
    CF_TRY(split_rule_check(ctx, "cf_holdout_split", SplitRule{mode, a, b, min_train}));
    CF_TRY(split_host_check(ctx, "cf_holdout_split", n, n_users, n_items, user, item, part));
    CF_TRY(set_device(ctx));
    DevBuf du, dm, dk, dp, ds;
    int rc = dev_alloc(ctx, du, 4 * n);
    if (rc == CF_OK) rc = dev_alloc(ctx, dm, 4 * n);
    if (rc == CF_OK && order_key) rc = dev_alloc(ctx, dk, 8 * n);
    if (rc == CF_OK) rc = dev_alloc(ctx, dp, n);
    if (rc == CF_OK) rc = dev_alloc(ctx, ds, sizeof(uint64_t) * CF_SPLIT_STATS);
    if (rc != CF_OK) return rc;
    if (n) {
        CF_HIP_CHECK(ctx, hipMemcpy(du.p, user, 4 * n, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy(dm.p, item, 4 * n, hipMemcpyHostToDevice));
        if (order_key) CF_HIP_CHECK(ctx, hipMemcpy(dk.p, order_key, 8 * n, hipMemcpyHostToDevice));
    }
    CF_TRY(cf_holdout_split_run(ctx, n, n_users, n_items, (const uint32_t*)du.p, (const uint32_t*)dm.p,
                                (const uint64_t*)dk.p, seed, min_user, min_item, mode, a, b, min_train, (uint8_t*)dp.p,
                                (uint64_t*)ds.p, nullptr));
    CF_HIP_CHECK(ctx, hipDeviceSynchronize());
    if (n) CF_HIP_CHECK(ctx, hipMemcpy(part, dp.p, n, hipMemcpyDeviceToHost));
    if (stats) CF_HIP_CHECK(ctx, hipMemcpy(stats, ds.p, sizeof(uint64_t) * CF_SPLIT_STATS, hipMemcpyDeviceToHost));
    return CF_OK;
}

int cf_split_timing(cf_ctx* ctx, float ms[4]) {
    if (!ctx) return CF_EINVAL;
    if (!ms) return cf_set_error(ctx, CF_EINVAL, "cf_split_timing: null argument");
    if (!ctx->split_steps) return cf_set_error(ctx, CF_ESTATE, "cf_split_timing: no split call with edges yet");
    CF_TRY(set_device(ctx));
    CF_HIP_CHECK(ctx, hipEventSynchronize(ctx->split_ev[ctx->split_steps]));
    for (int s = 0; s < 4; ++s) {
        ms[s] = 0.0f;
        if (s < ctx->split_steps) CF_HIP_CHECK(ctx, hipEventElapsedTime(&ms[s], ctx->split_ev[s], ctx->split_ev[s + 1]));
    }
    return CF_OK;
}
