// cf_knn_topn.hip -- top-N recommendation and ranking evaluation from the item graph (cf_knn_topn,
// cf_knn_rank_eval): the neighbourhood model's score of every item m for a user's profile,
//   sw = sum_t [w(m, i_t) > w_min] w(m, i_t),  swr = sum_t [w(m, i_t) > w_min] w(m, i_t) r_t,
// over the profile in its order, in fp64 from the graph's fp32 weights (the out-edges of the scored
// item, as knn3_kernel reads them).  knn3 (knn3.cpp:185-227) scores listed pairs only; this fills
// the key panel of cf_topn_panel.h, and the panel drivers of cf_topn.hip / cf_rank.hip do the
// rest.  DESIGN 3.19.
//
// Scatter over in-lists, not a gather per candidate: a profile entry (i, r) touches only the items
// m with an edge m -> i above w_min.
//   knn_in_kernel<false/true>  the in-lists of the resident graph (either layout): per column i the
//                        pairs (m, w(m, i)) with w > w_min as a CSR.  A counting pass (integer
//                        atomics), knn_in_scan_kernel (one workgroup, block_excl_scan per kAT
//                        columns with a carry) and a fill pass with an atomic cursor per column: the
//                        order inside an in-list does not reach a score, each m is in it once.
//                        Cached in the context for the graph and w_min they were built from.
//   knn_score_kernel     one workgroup per user row of the block.  The row of the panel is the swr
//                        accumulator (the bits of doubles), MEAN mode keeps sw in a second plane.  The
//                        profile is walked entry by entry; the lanes stride over in(i_t) with
//                        kKnnUnroll entries in flight each and every entry is a plain read-modify-
//                        write of its own m (all m of one in-list differ: no two lanes collide).
//                        __syncthreads() between entries orders the accesses of two entries to one
//                        m (it fences global memory at workgroup scope).  A last pass turns every
//                        accumulator into score_key(score) in place.  Three workgroups per CU, not
//                        the eight that fit (knn_lds_pad): measured faster.
// The sums of one (user, m) run in profile order from zero whatever the block, the layout or the
// other users are: the same bytes everywhere.  No floating-point atomics.

#include <cmath>
#include <cstdlib>

#include "cf_topn_panel.h"

namespace {

constexpr int kKnnUnroll = 4;   // in-list entries in flight per lane

// Row m of the graph by the workgroup: FILL = false counts the entries above w_min per column,
// FILL = true appends (m, w) to the in-list of each such column at its cursor.
template <bool FILL>
__global__ __launch_bounds__(kAT) void knn_in_kernel(GraphDev g, double w_min, uint32_t* __restrict__ cnt,
                                                    const uint64_t* __restrict__ in_off, uint32_t* __restrict__ in_m,
                                                    float* __restrict__ in_w) {
    for (uint64_t m = blockIdx.x; m < g.n; m += gridDim.x) {
        const GraphRow r = g.row((uint32_t)m);
        const uint64_t len = r.dense ? g.n : r.len;
        for (uint64_t j = threadIdx.x; j < len; j += kAT) {
            const uint32_t i = r.dense ? (uint32_t)j : r.col[j];
            const float w = r.dense ? r.dense[j] : r.w[j];
            if (!((double)w > w_min) || i >= g.n) continue;
            const uint32_t at = atomicAdd(&cnt[i], 1u);
            if (FILL) {
                in_m[in_off[i] + at] = (uint32_t)m;
                in_w[in_off[i] + at] = w;
            }
        }
    }
}

// in_off = exclusive scan of cnt over the n columns, in_off[n] = the total (one workgroup).
__global__ __launch_bounds__(kAT) void knn_in_scan_kernel(const uint32_t* __restrict__ cnt, uint64_t n,
                                                         uint64_t* __restrict__ in_off) {
    __shared__ uint32_t s_scan[kWaves + 1];
    uint64_t carry = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += kAT) {   // the same trips for the whole workgroup
        const uint64_t i = i0 + threadIdx.x;
        const uint32_t v = i < n ? cnt[i] : 0u;
        uint32_t all;
        const uint32_t before = block_excl_scan(v, s_scan, &all);
        if (i < n) in_off[i] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0) in_off[n] = carry;
}

// Row blockIdx.x of the block: user sel[b0 + row] (b0 + row without a selection).  acc = the row of
// the panel, sw = the row of the second plane (MEAN) or null.
__global__ __launch_bounds__(kAT) void knn_score_kernel(const uint64_t* __restrict__ in_off,
                                                       const uint32_t* __restrict__ in_m,
                                                       const float* __restrict__ in_w,
                                                       const uint64_t* __restrict__ prof_off,
                                                       const uint32_t* __restrict__ prof_item,
                                                       const float* __restrict__ prof_rating,
                                                       const uint32_t* __restrict__ sel, uint32_t b0,
                                                       uint32_t n_items, int mean_mode, uint64_t* panel,
                                                       uint64_t* plane) {
    const uint32_t u = sel ? sel[b0 + blockIdx.x] : b0 + blockIdx.x;
    uint64_t* acc = panel + (size_t)blockIdx.x * n_items;
    uint64_t* sw = mean_mode ? plane + (size_t)blockIdx.x * n_items : nullptr;
    for (uint32_t i = threadIdx.x; i < n_items; i += kAT) {
        acc[i] = 0ull;   // +0.0
        if (sw) sw[i] = 0ull;
    }
    __syncthreads();
    const uint64_t p0 = prof_off[u], p1 = prof_off[u + 1];
    for (uint64_t t = p0; t < p1; ++t) {   // the order is the contract; the same trips for the whole workgroup
        const uint32_t it = prof_item[t];
        const double r = (double)prof_rating[t];
        const uint64_t e1 = in_off[it + 1];
        for (uint64_t e0 = in_off[it] + threadIdx.x; e0 < e1; e0 += (uint64_t)kAT * kKnnUnroll) {
            uint32_t m[kKnnUnroll];
            double w[kKnnUnroll], a[kKnnUnroll], s[kKnnUnroll];
#pragma unroll
            for (int j = 0; j < kKnnUnroll; ++j) {
                const uint64_t e = e0 + (uint64_t)j * kAT;
                m[j] = e < e1 ? in_m[e] : 0xffffffffu;
                w[j] = e < e1 ? (double)in_w[e] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < kKnnUnroll; ++j) {
                a[j] = m[j] < n_items ? __longlong_as_double((long long)acc[m[j]]) : 0.0;
                s[j] = (sw && m[j] < n_items) ? __longlong_as_double((long long)sw[m[j]]) : 0.0;
            }
#pragma unroll
            for (int j = 0; j < kKnnUnroll; ++j) {
                if (m[j] >= n_items) continue;
                acc[m[j]] = (uint64_t)__double_as_longlong(a[j] + w[j] * r);   // the product is exact in fp64
                if (sw) sw[m[j]] = (uint64_t)__double_as_longlong(s[j] + w[j]);
            }
        }
        __syncthreads();   // entry t + 1 may touch the same m from another lane
    }
    for (uint32_t i = threadIdx.x; i < n_items; i += kAT) {
        double score = __longlong_as_double((long long)acc[i]);
        if (sw) {
            const double d = __longlong_as_double((long long)sw[i]);
            score = d > 0.0 ? score / d : 0.0;   // knn3.cpp:216: no neighbour -> 0
        }
        acc[i] = score_key(score);
    }
}

// The in-lists of the resident graph above w_min: the cached ones, or built now (their device
// time is added to *ms).
int knn_in_lists(cf_ctx* ctx, double w_min, hipStream_t st, float* ms) {
    if (ctx->d_knn_in_off && ctx->knn_in_gen == ctx->graph_gen && ctx->knn_in_wmin == w_min) return CF_OK;
    cf_knn_in_free(ctx);
    const uint64_t n = ctx->n_items;
    // the scan sums kAT column counts (each <= n) in 32 bits before the 64-bit carry takes them
    if (n > (1ull << 24)) return cf_set_error(ctx, CF_ERANGE, "kNN in-lists: more than 2^24 items");
    const GraphDev g = graph_dev(ctx);
    MfEvents<2> evs;
    for (hipEvent_t& e : evs.e) CF_HIP_CHECK(ctx, hipEventCreate(&e));
    CF_TRY(cf_malloc_evict(ctx, (void**)&ctx->d_knn_in_off, sizeof(uint64_t) * (n + 1), "kNN in-list offsets"));
    CF_TRY(cf_malloc_evict(ctx, (void**)&ctx->d_knn_in_cnt, sizeof(uint32_t) * n, "kNN in-list counts"));
    const unsigned grid = (unsigned)std::min<uint64_t>(n, 65536u);
    CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
    CF_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_knn_in_cnt, 0, sizeof(uint32_t) * n, st));
    hipLaunchKernelGGL(knn_in_kernel<false>, dim3(grid), dim3(kAT), 0, st, g, w_min, ctx->d_knn_in_cnt,
                       (const uint64_t*)nullptr, (uint32_t*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(knn_in_scan_kernel, dim3(1), dim3(kAT), 0, st, (const uint32_t*)ctx->d_knn_in_cnt, n,
                       ctx->d_knn_in_off);
    CF_HIP_CHECK(ctx, hipGetLastError());
    uint64_t total = 0;
    CF_HIP_CHECK(ctx, hipMemcpyAsync(&total, ctx->d_knn_in_off + n, sizeof(total), hipMemcpyDeviceToHost, st));
    CF_HIP_CHECK(ctx, hipStreamSynchronize(st));
    CF_TRY(cf_malloc_evict(ctx, (void**)&ctx->d_knn_in_m, sizeof(uint32_t) * std::max<uint64_t>(total, 1), "kNN in-lists"));
    CF_TRY(cf_malloc_evict(ctx, (void**)&ctx->d_knn_in_w, sizeof(float) * std::max<uint64_t>(total, 1), "kNN in-lists"));
    CF_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_knn_in_cnt, 0, sizeof(uint32_t) * n, st));
    hipLaunchKernelGGL(knn_in_kernel<true>, dim3(grid), dim3(kAT), 0, st, g, w_min, ctx->d_knn_in_cnt,
                       (const uint64_t*)ctx->d_knn_in_off, ctx->d_knn_in_m, ctx->d_knn_in_w);
    CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipStreamSynchronize(st));
    *ms += elapsed(evs.e[0], evs.e[1]);
    ctx->knn_in_gen = ctx->graph_gen;
    ctx->knn_in_wmin = w_min;
    return CF_OK;
}

// Users in flight per CU.  knn_score_kernel uses no LDS; a workgroup that asks for 160 KB / w of it
// all the same leaves room for w workgroups per CU, which bounds the accumulator rows that compete
// for the caches and the memory pipeline.  Measured: 3 against the 8 that fit, 27 % less
// time in SUM mode and 3 % in MEAN mode at 20,000 items, 47 % and 26 % at 5,000 items; 2 is no
// faster than 3 and 4 is slower in MEAN mode.  CF_KNN_TOPN_WGS = 2 .. 8 forces a value (read once per
// context; for A/B runs).  The results do not depend on it.
constexpr int kKnnWgs = 3;
size_t knn_lds_pad(cf_ctx* ctx) {
    if (ctx->knn_topn_wgs < 0) {
        const char* e = std::getenv("CF_KNN_TOPN_WGS");
        const int v = e ? std::atoi(e) : 0;
        ctx->knn_topn_wgs = (v >= 2 && v <= 8) ? v : kKnnWgs;
    }
    const size_t w = (size_t)ctx->knn_topn_wgs;
    if (w >= 8) return 0;
    const size_t kLds = 160 * 1024, kMaxDynamic = 64 * 1024;   // per CU; per workgroup without an attribute
    return std::min(kMaxDynamic, (kLds / w) & ~(size_t)1023);
}

// The graph source of the panel drivers: after the profiles, the sw plane of MEAN mode in the
// workspace; the in-lists in the context, knn_score_kernel over the block's rows.
struct KnnPanelSource final : ProfilePanelSource {
    int mode = CF_KNN_SCORE_SUM;
    double w_min = 0.0;
    uint64_t* d_plane = nullptr;

    uint64_t* carve_plane(Carver& c, uint32_t ub) const {
        return mode == CF_KNN_SCORE_MEAN ? c.take<uint64_t>((size_t)ub * n_items) : nullptr;
    }
    size_t workspace(uint32_t ub) const override {
        Carver c;
        carve(c);
        carve_plane(c, ub);
        return c.pos;
    }
    int upload(cf_ctx* ctx, void* ws, uint32_t ub, hipStream_t st, float* score_ms) override {
        Carver c;
        c.base = static_cast<char*>(ws);
        CF_TRY(upload_profiles(ctx, c));
        d_plane = carve_plane(c, ub);
        return knn_in_lists(ctx, w_min, st, score_ms);
    }
    int fill(cf_ctx* ctx, hipStream_t st, const uint32_t* d_sel, uint32_t b0, uint32_t nb, uint64_t* d_panel) override {
        hipLaunchKernelGGL(knn_score_kernel, dim3(nb), dim3(kAT), knn_lds_pad(ctx), st, (const uint64_t*)ctx->d_knn_in_off,
                           (const uint32_t*)ctx->d_knn_in_m, (const float*)ctx->d_knn_in_w, (const uint64_t*)dev.off,
                           (const uint32_t*)dev.item, (const float*)dev.rating, d_sel, b0, n_items,
                           mode == CF_KNN_SCORE_MEAN ? 1 : 0, d_panel, d_plane);
        return CF_OK;
    }
};

// The checks of the graph source, before the drivers' own.
int cf_knn_check(cf_ctx* ctx, const std::string& fn, uint32_t n_users, const uint64_t* prof_off,
                 const uint32_t* prof_item, const float* prof_rating, int score_mode, double w_min,
                 KnnPanelSource* src) {
    if (!has_graph(ctx)) return cf_set_error(ctx, CF_ESTATE, fn + ": no item graph uploaded");
    if (score_mode != CF_KNN_SCORE_SUM && score_mode != CF_KNN_SCORE_MEAN)
        return cf_set_error(ctx, CF_EINVAL, fn + ": unknown score mode");
    if (!std::isfinite(w_min) || w_min < 0.0) return cf_set_error(ctx, CF_EINVAL, fn + ": w_min is not finite and >= 0");
    CF_TRY(check_csr(ctx, fn.c_str(), "profile", n_users, prof_off, prof_item, ctx->n_items, false, true, prof_rating));
    src->n_users = n_users, src->n_items = ctx->n_items;
    src->prof_off = prof_off, src->prof_item = prof_item, src->prof_rating = prof_rating;
    src->mode = score_mode, src->w_min = w_min;
    return CF_OK;
}

}  // namespace

void cf_knn_in_free(cf_ctx* ctx) {
    if (ctx->d_knn_in_off) (void)hipFree(ctx->d_knn_in_off);
    if (ctx->d_knn_in_m) (void)hipFree(ctx->d_knn_in_m);
    if (ctx->d_knn_in_w) (void)hipFree(ctx->d_knn_in_w);
    if (ctx->d_knn_in_cnt) (void)hipFree(ctx->d_knn_in_cnt);
    ctx->d_knn_in_off = nullptr;
    ctx->d_knn_in_m = nullptr;
    ctx->d_knn_in_w = nullptr;
    ctx->d_knn_in_cnt = nullptr;
    ctx->knn_in_gen = ~0ull;
}

extern "C" int cf_debug_knn_topn_walk(void) { return kAT * kKnnUnroll; }

extern "C" int cf_knn_topn(cf_ctx* ctx, uint32_t n_users, const uint64_t* prof_off, const uint32_t* prof_item,
                           const float* prof_rating, int score_mode, double w_min, const uint64_t* excl_off,
                           const uint32_t* excl_item, uint32_t n_sel, const uint32_t* sel_user, uint32_t N,
                           uint32_t* items, double* scores, uint32_t* count, cf_topn_stats* stats) {
    if (!ctx) return CF_EINVAL;
    KnnPanelSource src;
    CF_TRY(cf_knn_check(ctx, "cf_knn_topn", n_users, prof_off, prof_item, prof_rating, score_mode, w_min, &src));
    return cf_topn_drive(ctx, "cf_knn_topn", src, n_users, ctx->n_items, excl_off, excl_item, n_sel, sel_user, N, items,
                         scores, count, stats);
}

extern "C" int cf_knn_rank_eval(cf_ctx* ctx, uint32_t n_users, const uint64_t* prof_off, const uint32_t* prof_item,
                                const float* prof_rating, int score_mode, double w_min, const uint64_t* excl_off,
                                const uint32_t* excl_item, const uint64_t* held_off, const uint32_t* held_item,
                                const double* held_w, uint32_t N, uint32_t* rank, cf_rank_user* users,
                                cf_rank_summary* summary) {
    if (!ctx) return CF_EINVAL;
    KnnPanelSource src;
    CF_TRY(cf_knn_check(ctx, "cf_knn_rank_eval", n_users, prof_off, prof_item, prof_rating, score_mode, w_min, &src));
    return cf_rank_drive(ctx, "cf_knn_rank_eval", src, n_users, ctx->n_items, excl_off, excl_item, held_off, held_item,
                         held_w, N, rank, users, summary);
}
