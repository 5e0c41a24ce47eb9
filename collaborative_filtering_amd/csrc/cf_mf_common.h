// cf_mf_common.h -- what the matrix-factorization files (cf_als.hip, cf_sgd.hip, cf_svdpp.hip)
// share: the degree cuts, the scan compaction of one side's flags into per-class active lists,
// the dot-product group, the fixed block reduction, and the host helpers of the fits: argument
// checks, the context-owned workspace (one allocation, ctx->d_als, carved per call) and the
// uploads of a side and of the validation edges.  The vertex reduction of SGD and SVD++ is in
// cf_mf_reduce.h.  Everything has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "cf_internal.h"

namespace {

constexpr int kAT = 256;               // threads per workgroup
constexpr int kWaves = kAT / 64;
constexpr int kLowMax = 64;            // low / mid cut (TRAIN degree)
constexpr int kSeg = 2048;             // mid / high cut and the segment length
constexpr int kG = 8;                  // lanes per edge of the dot-product kernels
constexpr int kVPT = 4;                // vertices per thread of the compaction kernels
constexpr int kCompBlock = kAT * kVPT;
constexpr int kErrPerBlock = (kAT / kG) * 8;   // edges per block of the error kernels

// The compacted active lists of the side being updated (ascending vertex order).
struct AlsLists {
    uint32_t* low;
    uint32_t* mid;
    uint32_t* high;
    uint32_t* high_base;   // first workspace slot (= index into seg_*) of each high vertex
    uint32_t* seg_vertex;  // one entry per (high vertex, segment)
    uint32_t* seg_index;
    uint32_t* block_cnt;   // 4 counters per compaction block, then their exclusive scan
    uint32_t* record;      // {low, mid, high, segments} of the last compaction
};

// ---- compaction of one side's flags into the class lists (deterministic scan) ------------

__device__ __forceinline__ int als_class(uint64_t deg) { return deg <= (uint64_t)kLowMax ? 0 : (deg <= (uint64_t)kSeg ? 1 : 2); }

// Exclusive scan of one value per thread over the block (kAT threads); *total = the block sum.
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t* s_wave /* kWaves + 1 */, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();   // s_wave may still be read from the previous call
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t c = s_wave[w];
        if (w < wave) before += c;
        all += c;
    }
    *total = all;
    return before + inc - v;
}

// FILL = false: per-block counters {low, mid, high, segments}.  FILL = true: with their exclusive
// scan in block_cnt, writes the lists, sets active[] and clears flag[].  Side has n, off, flag
// and active.
template <bool FILL, class Side>
__global__ __launch_bounds__(kAT) void als_compact_kernel(Side s, AlsLists L) {
    __shared__ uint32_t s_wave[kWaves + 1];
    const uint32_t v0 = (blockIdx.x * (uint32_t)kAT + threadIdx.x) * kVPT;
    uint32_t cnt[4] = {0, 0, 0, 0};
    int cls[kVPT];
    uint32_t nseg[kVPT];
#pragma unroll
    for (int i = 0; i < kVPT; ++i) {
        cls[i] = -1;
        nseg[i] = 0;
        const uint64_t v = (uint64_t)v0 + i;
        if (v < s.n && s.flag[v]) {
            const uint64_t deg = s.off[v + 1] - s.off[v];
            cls[i] = als_class(deg);
            cnt[cls[i]]++;
            if (cls[i] == 2) {
                nseg[i] = (uint32_t)((deg + kSeg - 1) / kSeg);
                cnt[3] += nseg[i];
            }
        }
    }
    uint32_t pre[4], tot[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) pre[c] = block_excl_scan(cnt[c], s_wave, &tot[c]);
    if (!FILL) {
        if (threadIdx.x == 0)
            for (int c = 0; c < 4; ++c) L.block_cnt[(size_t)blockIdx.x * 4 + c] = tot[c];
        return;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) pre[c] += L.block_cnt[(size_t)blockIdx.x * 4 + c];
#pragma unroll
    for (int i = 0; i < kVPT; ++i) {
        const uint64_t v = (uint64_t)v0 + i;
        if (v >= s.n) continue;
        s.active[v] = cls[i] >= 0;
        s.flag[v] = 0;
        if (cls[i] == 0) L.low[pre[0]++] = (uint32_t)v;
        else if (cls[i] == 1) L.mid[pre[1]++] = (uint32_t)v;
        else if (cls[i] == 2) {
            L.high[pre[2]] = (uint32_t)v;
            L.high_base[pre[2]++] = pre[3];
            for (uint32_t q = 0; q < nseg[i]; ++q) {
                L.seg_vertex[pre[3]] = (uint32_t)v;
                L.seg_index[pre[3]++] = q;
            }
        }
    }
}

// Exclusive scan of the per-block counters in block order (one workgroup; counter c by thread c);
// the totals go to the record.
__global__ void als_scan_kernel(AlsLists L, uint32_t n_blocks) {
    const int c = threadIdx.x;
    if (c >= 4) return;
    uint32_t run = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint32_t t = L.block_cnt[(size_t)b * 4 + c];
        L.block_cnt[(size_t)b * 4 + c] = run;
        run += t;
    }
    L.record[c] = run;
}

template <class Side>
void launch_compact(const Side& s, const AlsLists& lists, hipStream_t st) {
    const uint32_t blocks = (uint32_t)(((uint64_t)s.n + kCompBlock - 1) / kCompBlock);
    if (blocks) {
        hipLaunchKernelGGL((als_compact_kernel<false, Side>), dim3(blocks), dim3(kAT), 0, st, s, lists);
        hipLaunchKernelGGL(als_scan_kernel, dim3(1), dim3(64), 0, st, lists, blocks);
        hipLaunchKernelGGL((als_compact_kernel<true, Side>), dim3(blocks), dim3(kAT), 0, st, s, lists);
    } else {
        hipLaunchKernelGGL(als_scan_kernel, dim3(1), dim3(64), 0, st, lists, 0u);
    }
}

// ---- dot product: kG lanes per edge --------------------------------------------------------

__device__ __forceinline__ double group_dot(const double* __restrict__ a, const double* __restrict__ b, int D, int sl) {
    double s = 0.0;
    for (int d = sl; d < D; d += kG) s = fma(a[d], b[d], s);
#pragma unroll
    for (int o = kG / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o, kG);
    return s;
}

// Fixed tree over the block's kAT values in LDS; the result is in v[0].
__device__ inline void block_tree_sum(double* v) {
    for (int o = kAT / 2; o >= 1; o >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < o) v[threadIdx.x] += v[threadIdx.x + o];
    }
    __syncthreads();
}

// The prediction of one edge from its dot product.  bu == NULL (ALS, plain SGD): the dot itself.
// Otherwise biassgd.cpp:400-403, in its order: ((mean + bu) + bi) + dot.
__device__ __forceinline__ double mf_predict(double dot, double mean, const double* __restrict__ bu,
                                             const double* __restrict__ bi, uint32_t u, uint32_t i) {
    return bu ? mean + bu[u] + bi[i] + dot : dot;
}

__device__ __forceinline__ double mf_clamp(double p, double minval, double maxval) {
    p = fmin(maxval, p);
    return fmax(minval, p);
}

// pred[e] of the pairs (user[e], item[e]); clamped iff clamp != 0.  (Not every file that includes
// this header predicts: cf_ials.hip leaves it unused.)
__attribute__((unused)) __global__ __launch_bounds__(kAT) void mf_predict_kernel(uint64_t n, const uint32_t* __restrict__ user,
                                                        const uint32_t* __restrict__ item, const double* __restrict__ U,
                                                        const double* __restrict__ V, int D, const double* __restrict__ bu,
                                                        const double* __restrict__ bi, double mean, int clamp,
                                                        double minval, double maxval, double* pred) {
    const uint64_t e = ((uint64_t)blockIdx.x * kAT + threadIdx.x) / kG;
    const int sl = threadIdx.x & (kG - 1);
    if (e >= n) return;
    const uint32_t u = user[e], i = item[e];
    double p = mf_predict(group_dot(U + (size_t)u * D, V + (size_t)i * D, D, sl), mean, bu, bi, u, i);
    if (clamp) p = mf_clamp(p, minval, maxval);
    if (sl == 0) pred[e] = p;
}

// error aggregate (als.cpp:424-430), level 1: block b sums the clamped squared errors of edges
// [b kErrPerBlock, (b + 1) kErrPerBlock): group g takes edges g, g + 32, .. in order, then a tree.
__global__ __launch_bounds__(kAT) void mf_error_kernel(uint64_t n, const uint32_t* __restrict__ user,
                                                      const uint32_t* __restrict__ item, const float* __restrict__ obs,
                                                      const double* __restrict__ U, const double* __restrict__ V, int D,
                                                      const double* __restrict__ bu, const double* __restrict__ bi,
                                                      double mean, double minval, double maxval, double* partial) {
    __shared__ double s_v[kAT];
    const int grp = threadIdx.x / kG, sl = threadIdx.x & (kG - 1);
    const uint64_t e0 = (uint64_t)blockIdx.x * kErrPerBlock;
    double acc = 0.0;
    for (int r = 0; r < kErrPerBlock / (kAT / kG); ++r) {
        const uint64_t e = e0 + (uint64_t)r * (kAT / kG) + grp;
        if (e >= n) break;   // per group
        const uint32_t u = user[e], i = item[e];
        double p = mf_predict(group_dot(U + (size_t)u * D, V + (size_t)i * D, D, sl), mean, bu, bi, u, i);
        p = mf_clamp(p, minval, maxval);
        const double d = (double)obs[e] - p;
        acc = fma(d, d, acc);
    }
    s_v[threadIdx.x] = sl == 0 ? acc : 0.0;
    block_tree_sum(s_v);
    if (threadIdx.x == 0) partial[blockIdx.x] = s_v[0];
}

// Level 2 of the error reduction: one workgroup; thread t sums partials t, t + kAT, .. in order,
// then the same tree.
__global__ __launch_bounds__(kAT) void als_error_final_kernel(const double* __restrict__ partial, uint64_t n_partial,
                                                             double* out) {
    __shared__ double s_v[kAT];
    double acc = 0.0;
    for (uint64_t i = threadIdx.x; i < n_partial; i += kAT) acc += partial[i];
    s_v[threadIdx.x] = acc;
    block_tree_sum(s_v);
    if (threadIdx.x == 0) *out = s_v[0];
}

// ---- host ---------------------------------------------------------------------------------

inline uint64_t error_blocks(uint64_t n_edges) { return (n_edges + kErrPerBlock - 1) / kErrPerBlock; }

// Both levels of the error reduction over device arrays: partial holds error_blocks(n) doubles,
// *out receives the sum (n > 0).
inline void launch_error(hipStream_t st, uint64_t n, const uint32_t* user, const uint32_t* item, const float* obs,
                         const double* U, const double* V, int D, const double* bu, const double* bi, double mean,
                         double minval, double maxval, double* partial, double* out) {
    const uint64_t blocks = error_blocks(n);
    hipLaunchKernelGGL(mf_error_kernel, dim3((unsigned)blocks), dim3(kAT), 0, st, n, user, item, obs, U, V, D, bu, bi,
                       mean, minval, maxval, partial);
    hipLaunchKernelGGL(als_error_final_kernel, dim3(1), dim3(kAT), 0, st, (const double*)partial, blocks, out);
}

// Carves one device allocation (the context's ALS workspace) into aligned arrays.
struct Carver {
    size_t pos = 0;
    char* base = nullptr;
    template <class T>
    T* take(size_t count) {
        const size_t at = pos;
        pos = (pos + sizeof(T) * std::max<size_t>(count, 1) + 255) & ~(size_t)255;
        return base ? reinterpret_cast<T*>(base + at) : nullptr;
    }
};

// The context's ALS workspace with at least `bytes` bytes; grown before any launch of the call.
inline int als_reserve(cf_ctx* ctx, size_t bytes) {
    if (ctx->als_bytes >= bytes && ctx->d_als) return CF_OK;
    if (ctx->d_als) {
        CF_HIP_CHECK(ctx, hipDeviceSynchronize());
        (void)hipFree(ctx->d_als);
        ctx->d_als = nullptr;
        ctx->als_bytes = 0;
    }
    CF_TRY(cf_malloc_evict(ctx, &ctx->d_als, bytes, "ALS workspace"));
    ctx->als_bytes = bytes;
    return CF_OK;
}

// Runs carve twice: the size pass, then, with the workspace reserved, over ctx->d_als.
template <class F>
int carve_workspace(cf_ctx* ctx, F carve) {
    Carver size;
    carve(size);
    CF_TRY(als_reserve(ctx, size.pos));
    Carver c;
    c.base = static_cast<char*>(ctx->d_als);
    carve(c);
    return CF_OK;
}

// The part of one side that every fit keeps (AlsSide, SgdSide, PpSide): its CSR with the owner
// of each edge, the update counts and the flags.
template <class Side>
void carve_side(Carver& c, Side& s, uint32_t n, uint64_t nnz) {
    s.n = n;
    s.off = c.take<uint64_t>((size_t)n + 1);
    s.nbr = c.take<uint32_t>(nnz);
    s.obs = c.take<float>(nnz);
    s.src = c.take<uint32_t>(nnz);
    s.nupd = c.take<uint32_t>(n);
    s.flag = c.take<uint8_t>(n);
    s.active = c.take<uint8_t>(n);
}

// d_src[e] = the vertex that owns edge e of the CSR `off` (n vertices, nnz > 0 edges).
inline int upload_edge_owners(cf_ctx* ctx, uint32_t* d_src, uint32_t n, const uint64_t* off, uint64_t nnz) {
    std::vector<uint32_t> src(nnz);
    for (uint32_t v = 0; v < n; ++v)
        for (uint64_t e = off[v]; e < off[v + 1]; ++e) src[e] = v;
    CF_HIP_CHECK(ctx, hipMemcpy(d_src, src.data(), sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
    return CF_OK;
}

// Uploads that part of a side with n > 0 vertices.  flag = activate, or flag_fill everywhere
// where activate is NULL.
template <class Side>
int upload_side(cf_ctx* ctx, const Side& s, uint64_t nnz, const uint64_t* off, const uint32_t* nbr, const float* obs,
                const uint32_t* nupd, const uint8_t* activate, int flag_fill) {
    CF_HIP_CHECK(ctx, hipMemcpy((void*)s.off, off, sizeof(uint64_t) * ((size_t)s.n + 1), hipMemcpyHostToDevice));
    if (nnz) {
        CF_HIP_CHECK(ctx, hipMemcpy((void*)s.nbr, nbr, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy((void*)s.obs, obs, sizeof(float) * nnz, hipMemcpyHostToDevice));
        CF_TRY(upload_edge_owners(ctx, (uint32_t*)s.src, s.n, off, nnz));
    }
    CF_HIP_CHECK(ctx, hipMemcpy(s.nupd, nupd, sizeof(uint32_t) * s.n, hipMemcpyHostToDevice));
    if (activate) CF_HIP_CHECK(ctx, hipMemcpy(s.flag, activate, s.n, hipMemcpyHostToDevice));
    else CF_HIP_CHECK(ctx, hipMemset(s.flag, flag_fill, s.n));
    CF_HIP_CHECK(ctx, hipMemset(s.active, 0, s.n));
    return CF_OK;
}

// The VALIDATE edges of a traced fit on the device.
struct MfVal {
    uint32_t* user;
    uint32_t* item;
    float* obs;
};

inline void carve_val(Carver& c, MfVal& v, uint64_t n) {
    v.user = c.take<uint32_t>(n);
    v.item = c.take<uint32_t>(n);
    v.obs = c.take<float>(n);
}

inline int upload_val(cf_ctx* ctx, const MfVal& v, uint64_t n, const uint32_t* user, const uint32_t* item,
                      const float* obs) {
    if (n == 0) return CF_OK;
    CF_HIP_CHECK(ctx, hipMemcpy(v.user, user, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    CF_HIP_CHECK(ctx, hipMemcpy(v.item, item, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    CF_HIP_CHECK(ctx, hipMemcpy(v.obs, obs, sizeof(float) * n, hipMemcpyHostToDevice));
    return CF_OK;
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + kAT - 1) / kAT); }

inline float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}

inline uint64_t total_segments(uint32_t n, const uint64_t* off) {
    uint64_t segs = 0;
    for (uint32_t v = 0; v < n; ++v) {
        const uint64_t deg = off[v + 1] - off[v];
        if (deg > (uint64_t)kSeg) segs += (deg + kSeg - 1) / kSeg;
    }
    return segs;
}

inline void carve_lists(Carver& c, AlsLists& L, size_t nmax, uint64_t seg_cap) {
    L.low = c.take<uint32_t>(nmax);
    L.mid = c.take<uint32_t>(nmax);
    L.high = c.take<uint32_t>(nmax);
    L.high_base = c.take<uint32_t>(nmax);
    L.seg_vertex = c.take<uint32_t>(seg_cap);
    L.seg_index = c.take<uint32_t>(seg_cap);
    L.block_cnt = c.take<uint32_t>(((nmax + kCompBlock - 1) / kCompBlock) * 4);
    L.record = c.take<uint32_t>(4);
}

template <int N>
struct MfEvents {   // destroyed on every return path
    hipEvent_t e[N] = {};
    ~MfEvents() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

// Per-vertex degree counts of one CSR against the other's neighbour lists (the transpose check).
inline bool transpose_counts_agree(uint32_t n_a, const uint64_t* off_a, const uint32_t* nbr_a, uint32_t n_b,
                                   const uint64_t* off_b) {
    std::vector<uint64_t> cnt(n_b, 0);
    for (uint64_t e = 0; e < off_a[n_a]; ++e) cnt[nbr_a[e]]++;
    for (uint32_t v = 0; v < n_b; ++v)
        if (cnt[v] != off_b[v + 1] - off_b[v]) return false;
    return true;
}

// The CSR check of every entry point, in two halves so that a caller's own limits can stand
// between them (cf_bpr.hip).  The shape: offsets present, from 0 and not decreasing, and the edge
// arrays present where there are edges (`val` counts only with has_val: a CSR without values
// passes neither).
inline int check_csr_shape(cf_ctx* ctx, const char* fn, const char* what, uint32_t n, const uint64_t* off,
                           const uint32_t* nbr, bool has_val = false, const void* val = nullptr) {
    const std::string head = std::string(fn) + ": " + what;
    if (!off) return cf_set_error(ctx, CF_EINVAL, head + " offsets are null");
    if (off[0] != 0) return cf_set_error(ctx, CF_EINVAL, head + " offsets do not start at 0");
    for (uint32_t v = 0; v < n; ++v)
        if (off[v + 1] < off[v]) return cf_set_error(ctx, CF_EINVAL, head + " offsets decrease");
    if (off[n] && (!nbr || (has_val && !val))) return cf_set_error(ctx, CF_EINVAL, head + " edge array is null");
    return CF_OK;
}

// The indices of a CSR of good shape: below n_other and, with `ascending`, strictly ascending in
// every list.
inline int check_csr_index(cf_ctx* ctx, const char* fn, const char* what, uint32_t n, const uint64_t* off,
                           const uint32_t* nbr, uint32_t n_other, bool ascending = false) {
    const std::string head = std::string(fn) + ": " + what;
    for (uint64_t e = 0; e < off[n]; ++e)
        if (nbr[e] >= n_other) return cf_set_error(ctx, CF_EINVAL, head + " index out of range");
    if (ascending)
        for (uint32_t v = 0; v < n; ++v)
            for (uint64_t e = off[v] + 1; e < off[v + 1]; ++e)
                if (nbr[e] <= nbr[e - 1])
                    return cf_set_error(ctx, CF_EINVAL, head + " lists are not strictly ascending");
    return CF_OK;
}

inline int check_csr(cf_ctx* ctx, const char* fn, const char* what, uint32_t n, const uint64_t* off,
                     const uint32_t* nbr, uint32_t n_other, bool ascending = false, bool has_val = false,
                     const void* val = nullptr) {
    CF_TRY(check_csr_shape(ctx, fn, what, n, off, nbr, has_val, val));
    return check_csr_index(ctx, fn, what, n, off, nbr, n_other, ascending);
}

// The argument checks cf_als_fit and cf_sgd_fit share: D, the two CSRs and their consistency.
inline int check_two_csr(cf_ctx* ctx, const char* fn, uint32_t n_users, uint32_t n_items, uint32_t D,
                         const uint64_t* user_off, const uint32_t* user_item, const float* user_obs,
                         const uint64_t* item_off, const uint32_t* item_user, const float* item_obs, uint64_t* nnz_out) {
    const std::string f(fn);
    if (D == 0) return cf_set_error(ctx, CF_EINVAL, f + ": D = 0");
    if (D > CF_ALS_MAX_D) return cf_set_error(ctx, CF_ERANGE, f + ": D above CF_ALS_MAX_D");
    if ((n_users && !user_off) || (n_items && !item_off)) return cf_set_error(ctx, CF_EINVAL, f + ": null argument");
    const uint64_t nnz = n_users ? user_off[n_users] : 0;
    const uint64_t nnz_i = n_items ? item_off[n_items] : 0;
    if (nnz != nnz_i) return cf_set_error(ctx, CF_EINVAL, f + ": the two CSRs hold different edge counts");
    if (nnz && (!user_item || !user_obs || !item_user || !item_obs))
        return cf_set_error(ctx, CF_EINVAL, f + ": null edge array");
    if (n_users) CF_TRY(check_csr(ctx, fn, "user", n_users, user_off, user_item, n_items));
    if (n_items) CF_TRY(check_csr(ctx, fn, "item", n_items, item_off, item_user, n_users));
    if (nnz && (!transpose_counts_agree(n_users, user_off, user_item, n_items, item_off) ||
                !transpose_counts_agree(n_items, item_off, item_user, n_users, user_off)))
        return cf_set_error(ctx, CF_EINVAL,
                            f + ": the per-vertex edge counts of the user CSR and the item CSR disagree");
    *nnz_out = nnz;
    return CF_OK;
}

// The two checks cf_sgd_fit and cf_svdpp_fit share beyond check_two_csr(): a cap is set, and the
// VALIDATE edges of a traced fit are in range.
inline int check_caps(cf_ctx* ctx, const char* fn, uint64_t max_updates, uint32_t max_supersteps) {
    if (max_updates == std::numeric_limits<uint64_t>::max() && max_supersteps == 0)
        return cf_set_error(ctx, CF_EINVAL, std::string(fn) +
                                                ": neither max_updates nor max_supersteps is set (the run would never end)");
    return CF_OK;
}

inline int check_validation(cf_ctx* ctx, const char* fn, uint64_t n, const uint32_t* user, const uint32_t* item,
                            const float* obs, uint32_t n_users, uint32_t n_items) {
    if (n == 0) return CF_OK;
    if (!user || !item || !obs) return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": null validation array");
    for (uint64_t e = 0; e < n; ++e)
        if (user[e] >= n_users || item[e] >= n_items)
            return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": validation index out of range");
    return CF_OK;
}

inline int check_pairs(cf_ctx* ctx, const char* fn, uint64_t n, const uint32_t* user, const uint32_t* item,
                       const double* U, const double* V, uint32_t D, uint32_t n_users, uint32_t n_items) {
    if (D == 0) return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": D = 0");
    if (D > CF_ALS_MAX_D) return cf_set_error(ctx, CF_ERANGE, std::string(fn) + ": D above CF_ALS_MAX_D");
    if (n && (!user || !item || !U || !V)) return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": null argument");
    for (uint64_t e = 0; e < n; ++e)
        if (user[e] >= n_users || item[e] >= n_items)
            return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": index out of range");
    return CF_OK;
}

// Uploads the pair list and both factor matrices (and, for bias-SGD, the biases) into the
// context's ALS workspace.
struct PairLayout {
    uint32_t* user;
    uint32_t* item;
    float* obs;
    double* U;
    double* V;
    double* bu;        // NULL without biases
    double* bi;
    double* out;       // predictions, or the block partials followed by the sum
};

inline int upload_pairs(cf_ctx* ctx, PairLayout& p, uint64_t n, const uint32_t* user, const uint32_t* item,
                        const float* obs, uint32_t nu, uint32_t ni, uint32_t D, const double* U, const double* V,
                        size_t n_out, const double* bu = nullptr, const double* bi = nullptr) {
    CF_TRY(carve_workspace(ctx, [&](Carver& c) {
        p.user = c.take<uint32_t>(n);
        p.item = c.take<uint32_t>(n);
        p.obs = c.take<float>(n);
        p.U = c.take<double>((size_t)nu * D);
        p.V = c.take<double>((size_t)ni * D);
        p.out = c.take<double>(n_out);
        p.bu = bu ? c.take<double>(nu) : nullptr;
        p.bi = bi ? c.take<double>(ni) : nullptr;
    }));
    CF_HIP_CHECK(ctx, hipMemcpy(p.user, user, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    CF_HIP_CHECK(ctx, hipMemcpy(p.item, item, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    if (obs) CF_HIP_CHECK(ctx, hipMemcpy(p.obs, obs, sizeof(float) * n, hipMemcpyHostToDevice));
    CF_HIP_CHECK(ctx, hipMemcpy(p.U, U, sizeof(double) * (size_t)nu * D, hipMemcpyHostToDevice));
    CF_HIP_CHECK(ctx, hipMemcpy(p.V, V, sizeof(double) * (size_t)ni * D, hipMemcpyHostToDevice));
    if (bu) CF_HIP_CHECK(ctx, hipMemcpy(p.bu, bu, sizeof(double) * nu, hipMemcpyHostToDevice));
    if (bi) CF_HIP_CHECK(ctx, hipMemcpy(p.bi, bi, sizeof(double) * ni, hipMemcpyHostToDevice));
    return CF_OK;
}

}  // namespace
