// cf_als.hip -- ALS matrix factorization R ~ U V^T on gfx950 (als.cpp:290-371 on the synchronous
// engine), fp64 throughout.
//
// The graph is bipartite (users | items) and only TRAIN edges reach this file.  A superstep
// updates the active vertices of ONE side (signals only cross sides, so the sides alternate):
//   apply   (als.cpp:313-334)  A = sum x_j x_j^T + reg I, b = sum obs_j x_j over the vertex's
//                              edges (x_j = the other end's factor), factor = ldlt(A).solve(b),
//                              residual = (float)(|new - old|_1 / D), nupdates += 1; a vertex
//                              without edges only gets residual = 0, nupdates += 1
//   scatter (als.cpp:343-357)  per edge of an active vertex: error = (float)|obs - u.v|,
//                              priority = (double)(error * residual) (a float product); the other
//                              end is active next superstep iff priority > tol and its
//                              nupdates < max_updates
// The superstep loop is on the host (cf_als_fit): it reads one 16-byte record per superstep.
//
// Layout in HBM: factors row-major n x D fp64; one CSR per side (u64 offsets, u32 neighbour,
// f32 obs, u32 owner per edge for the edge-parallel scatter).  A half-sweep reads about
// nnz (8 D + 8) bytes (one D-long fp64 row, the neighbour id and the rating per edge) and does
// nnz D (D + 1) flops: bound by the row gathers, not by the fp64 units.
//
// Work is shaped by the vertex's TRAIN degree: the three classes (low / mid / high), the
// determinism rule they carry and the update kernels are in cf_als_update.h, shared with
// cf_ials.hip; this file gives them the policy AlsOp.  The Gram of one wave and the one-wave
// unpivoted LDL^T solve (the upper triangle the reference factors, als.cpp:330; an exactly zero
// pivot is skipped as cf_ldlt.hpp documents, pivots <= 0 or NaN are counted in n_not_pd) are in
// cf_als_gram.h.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cf_als_update.h"
#include "cf_internal.h"
#include "cf_mf_common.h"

namespace {

// One side of the graph as the kernels see it.
struct AlsSide {
    uint32_t n;
    const uint64_t* off;
    const uint32_t* nbr;
    const float* obs;
    const uint32_t* src;   // owner of each edge
    double* F;             // n x D factors
    const double* reg;
    uint32_t* nupd;
    float* resid;
    uint8_t* flag;         // signalled for the next superstep of this side
    uint8_t* active;       // active in the current superstep of this side
};

// The policy of cf_als_update.h: the unweighted edge, and apply's tail for vertex v.
struct AlsOp {
    static constexpr bool kWeighted = false;
    AlsSide s;
    __device__ const float* edge_obs() const { return s.obs; }
    __device__ const float* edge_pref() const { return nullptr; }
    // no TRAIN edge (als.cpp:319)
    __device__ void no_edges(uint32_t v, int, int lane) const {
        if (lane == 0) {
            s.resid[v] = 0.0f;
            s.nupd[v] += 1;
        }
    }
    // with the system in S: solve, residual, store
    __device__ void apply(double* S, int D, uint32_t v, unsigned long long* not_pd, int lane) const {
        const int bad = wave_ldlt_solve(S, D, s.reg[v], lane);
        double* Fv = s.F + (size_t)v * D;
        double diff = 0.0;
        for (int d = lane; d < D; d += 64) {
            const double x = S[tri(D, d)];
            diff += fabs(x - Fv[d]);
            Fv[d] = x;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) diff += __shfl_xor(diff, o);
        if (lane == 0) {
            s.resid[v] = (float)(diff / (double)D);
            s.nupd[v] += 1;
            if (bad) atomicAdd(not_pd, (unsigned long long)bad);   // integer counter
        }
    }
};

// scatter (als.cpp:343-357) over every edge of the side just updated; edges of inactive
// vertices leave at once.  The flag stores are plain and all write the same value.
__global__ __launch_bounds__(kAT) void als_scatter_kernel(AlsSide s, uint64_t nnz, const double* __restrict__ Fo,
                                                         const uint32_t* __restrict__ nupd_o, uint8_t* flag_o, int D,
                                                         double tol, uint64_t max_updates) {
    const uint64_t e = ((uint64_t)blockIdx.x * kAT + threadIdx.x) / kG;
    const int sl = threadIdx.x & (kG - 1);
    if (e >= nnz) return;   // whole groups leave together
    const uint32_t v = s.src[e];
    if (!s.active[v]) return;
    const uint32_t o = s.nbr[e];
    const double pred = group_dot(s.F + (size_t)v * D, Fo + (size_t)o * D, D, sl);
    if (sl != 0) return;
    const float error = (float)fabs((double)s.obs[e] - pred);
    const float prod = error * s.resid[v];
    const double priority = (double)prod;
    if (priority > tol && (uint64_t)nupd_o[o] < max_updates) flag_o[o] = 1;
}

// ---- host ---------------------------------------------------------------------------------

struct FitLayout {
    AlsSide side[2];
    AlsLists lists;
    double* ws;
    unsigned long long* not_pd;
    uint32_t seg_cap;
};

void carve_fit(Carver& c, FitLayout& f, uint32_t n_users, uint32_t n_items, uint64_t nnz, int D, uint64_t seg_cap) {
    const uint32_t n[2] = {n_users, n_items};
    for (int k = 0; k < 2; ++k) {
        AlsSide& s = f.side[k];
        carve_side(c, s, n[k], nnz);
        s.F = c.take<double>((size_t)n[k] * D);
        s.reg = c.take<double>(n[k]);
        s.resid = c.take<float>(n[k]);
    }
    const size_t nmax = std::max(n_users, n_items);
    carve_lists(c, f.lists, nmax, seg_cap);
    f.ws = c.take<double>((size_t)seg_cap * sys_len(D));
    f.not_pd = c.take<unsigned long long>(1);
    f.seg_cap = (uint32_t)seg_cap;
}

}  // namespace

extern "C" int cf_debug_als_segment(void) { return kSeg; }
extern "C" int cf_debug_als_low_max(void) { return kLowMax; }

extern "C" int cf_als_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                          const uint32_t* user_item, const float* user_obs, const uint64_t* item_off,
                          const uint32_t* item_user, const float* item_obs, const double* reg_user,
                          const double* reg_item, double tol, uint64_t max_updates, uint32_t max_supersteps, double* U,
                          double* V, uint32_t* nupdates_user, uint32_t* nupdates_item, float* residual_user,
                          float* residual_item, const uint8_t* activate_user, cf_als_stats* stats) {
    if (!ctx) return CF_EINVAL;
    if (stats) *stats = cf_als_stats{};
    if (D == 0) return cf_set_error(ctx, CF_EINVAL, "cf_als_fit: D = 0");
    if (D > CF_ALS_MAX_D) return cf_set_error(ctx, CF_ERANGE, "cf_als_fit: D above CF_ALS_MAX_D");
    if ((n_users && (!user_off || !reg_user || !U || !nupdates_user || !residual_user)) ||
        (n_items && (!item_off || !reg_item || !V || !nupdates_item || !residual_item)))
        return cf_set_error(ctx, CF_EINVAL, "cf_als_fit: null argument");
    uint64_t nnz = 0;
    CF_TRY(check_two_csr(ctx, "cf_als_fit", n_users, n_items, D, user_off, user_item, user_obs, item_off, item_user,
                         item_obs, &nnz));
    if (n_users == 0) return CF_OK;   // nothing can be active
    CF_TRY(set_device(ctx));

    // everything the fit needs exists before its first launch
    const uint64_t seg_cap = std::max(total_segments(n_users, user_off), n_items ? total_segments(n_items, item_off) : 0);
    if (seg_cap > 0xffffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_als_fit: too many segments");
    FitLayout f{};
    CF_TRY(carve_workspace(ctx, [&](Carver& c) { carve_fit(c, f, n_users, n_items, nnz, (int)D, seg_cap); }));
    MfEvents<3> evs;
    for (hipEvent_t& e : evs.e) CF_HIP_CHECK(ctx, hipEventCreate(&e));
    hipStream_t st = nullptr;

    const uint32_t n[2] = {n_users, n_items};
    const uint64_t* h_off[2] = {user_off, item_off};
    const uint32_t* h_nbr[2] = {user_item, item_user};
    const float* h_obs[2] = {user_obs, item_obs};
    const double* h_reg[2] = {reg_user, reg_item};
    double* h_F[2] = {U, V};
    uint32_t* h_nupd[2] = {nupdates_user, nupdates_item};
    float* h_res[2] = {residual_user, residual_item};
    for (int k = 0; k < 2; ++k) {
        if (n[k] == 0) continue;
        const AlsSide& s = f.side[k];
        CF_TRY(upload_side(ctx, s, nnz, h_off[k], h_nbr[k], h_obs[k], h_nupd[k], k == 0 ? activate_user : nullptr, k == 0));
        CF_HIP_CHECK(ctx, hipMemcpy(s.F, h_F[k], sizeof(double) * (size_t)n[k] * D, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy((void*)s.reg, h_reg[k], sizeof(double) * n[k], hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy(s.resid, h_res[k], sizeof(float) * n[k], hipMemcpyHostToDevice));
    }
    CF_HIP_CHECK(ctx, hipMemset(f.not_pd, 0, sizeof(unsigned long long)));

    if ((nnz * kG + kAT - 1) / kAT > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_als_fit: too many edges");
    const unsigned scatter_blocks = (unsigned)((nnz * kG + kAT - 1) / kAT);
    uint32_t supersteps = 0;
    uint64_t updates = 0;
    double update_ms = 0.0, scatter_ms = 0.0;
    int k = 0;   // the side being updated: users first (als.cpp:363-367,662)
    launch_compact(f.side[k], f.lists, st);
    for (;;) {
        // the one small record of the superstep: the active counts per class and the segments
        uint32_t rec[4];
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(rec, f.lists.record, sizeof(rec), hipMemcpyDeviceToHost));   // waits for the stream
        if (supersteps) {
            update_ms += elapsed(evs.e[0], evs.e[1]);
            scatter_ms += elapsed(evs.e[1], evs.e[2]);
        }
        const uint64_t n_active = (uint64_t)rec[0] + rec[1] + rec[2];
        if (n_active == 0) break;                                   // the run ends when no vertex is active
        if (max_supersteps && supersteps >= max_supersteps) break;
        if (rec[3] > f.seg_cap) return cf_set_error(ctx, CF_EHIP, "cf_als_fit: segment list overflow");
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
        launch_update(AlsOp{f.side[k]}, f.side[1 - k].F, (int)D, f.lists, rec, f.ws, f.not_pd, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
        if (nnz && n[1 - k])
            hipLaunchKernelGGL(als_scatter_kernel, dim3(scatter_blocks), dim3(kAT), 0, st, f.side[k], nnz,
                               (const double*)f.side[1 - k].F, (const uint32_t*)f.side[1 - k].nupd, f.side[1 - k].flag,
                               (int)D, tol, max_updates);
        k = 1 - k;
        launch_compact(f.side[k], f.lists, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[2], st));
        ++supersteps;
        updates += n_active;
    }
    CF_HIP_CHECK(ctx, hipDeviceSynchronize());
    for (int q = 0; q < 2; ++q) {
        if (n[q] == 0) continue;
        const AlsSide& s = f.side[q];
        CF_HIP_CHECK(ctx, hipMemcpy(h_F[q], s.F, sizeof(double) * (size_t)n[q] * D, hipMemcpyDeviceToHost));
        CF_HIP_CHECK(ctx, hipMemcpy(h_nupd[q], s.nupd, sizeof(uint32_t) * n[q], hipMemcpyDeviceToHost));
        CF_HIP_CHECK(ctx, hipMemcpy(h_res[q], s.resid, sizeof(float) * n[q], hipMemcpyDeviceToHost));
    }
    unsigned long long bad = 0;
    CF_HIP_CHECK(ctx, hipMemcpy(&bad, f.not_pd, sizeof(bad), hipMemcpyDeviceToHost));
    if (stats) {
        stats->supersteps = supersteps;
        stats->updates = updates;
        stats->n_not_pd = bad;
        stats->update_ms = (float)update_ms;
        stats->scatter_ms = (float)scatter_ms;
    }
    return CF_OK;
}

extern "C" int cf_als_error(cf_ctx* ctx, uint64_t n_edges, const uint32_t* user, const uint32_t* item, const float* obs,
                            uint32_t n_users, uint32_t n_items, uint32_t D, const double* U, const double* V,
                            double minval, double maxval, double* sum_sq) {
    if (!ctx) return CF_EINVAL;
    if (!sum_sq) return cf_set_error(ctx, CF_EINVAL, "cf_als_error: null result");
    *sum_sq = 0.0;
    CF_TRY(check_pairs(ctx, "cf_als_error", n_edges, user, item, U, V, D, n_users, n_items));
    if (n_edges && !obs) return cf_set_error(ctx, CF_EINVAL, "cf_als_error: null ratings");
    if (n_edges == 0) return CF_OK;
    CF_TRY(set_device(ctx));
    const uint64_t blocks = error_blocks(n_edges);
    if (blocks > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_als_error: too many edges");
    PairLayout p{};
    CF_TRY(upload_pairs(ctx, p, n_edges, user, item, obs, n_users, n_items, D, U, V, (size_t)blocks + 1));
    launch_error(nullptr, n_edges, p.user, p.item, p.obs, p.U, p.V, (int)D, nullptr, nullptr, 0.0, minval, maxval, p.out,
                 p.out + blocks);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(sum_sq, p.out + blocks, sizeof(double), hipMemcpyDeviceToHost));
    return CF_OK;
}

extern "C" int cf_als_predict(cf_ctx* ctx, uint64_t n_pairs, const uint32_t* user, const uint32_t* item,
                              uint32_t n_users, uint32_t n_items, uint32_t D, const double* U, const double* V,
                              double* pred) {
    if (!ctx) return CF_EINVAL;
    CF_TRY(check_pairs(ctx, "cf_als_predict", n_pairs, user, item, U, V, D, n_users, n_items));
    if (n_pairs && !pred) return cf_set_error(ctx, CF_EINVAL, "cf_als_predict: null result");
    if (n_pairs == 0) return CF_OK;
    CF_TRY(set_device(ctx));
    const uint64_t blocks = (n_pairs * kG + kAT - 1) / kAT;
    if (blocks > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_als_predict: too many pairs");
    PairLayout p{};
    CF_TRY(upload_pairs(ctx, p, n_pairs, user, item, nullptr, n_users, n_items, D, U, V, n_pairs));
    hipLaunchKernelGGL(mf_predict_kernel, dim3((unsigned)blocks), dim3(kAT), 0, nullptr, n_pairs,
                       (const uint32_t*)p.user, (const uint32_t*)p.item, (const double*)p.U, (const double*)p.V, (int)D,
                       (const double*)nullptr, (const double*)nullptr, 0.0, 0, 0.0, 0.0, p.out);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(pred, p.out, sizeof(double) * n_pairs, hipMemcpyDeviceToHost));
    return CF_OK;
}
