// cf_sgd.hip -- SGD and bias-SGD matrix factorization on gfx950 (sgd.cpp:243-339,344-401 and
// biassgd.cpp:249-347,399-434 on the synchronous engine with --interval 0), fp64 throughout.
//
// The graph is bipartite (users | items) and only TRAIN edges reach this file.  Supersteps
// alternate (cf_abi.h has the full rule):
//   user superstep   every active user u sums, over its edges (u, i), the per-edge error
//                      err = (float)(clamp(mean + bu + bi + U_u.V_i) - obs)
//                    into dU_u = sum -gamma (err V_i + lambda U_u) (gather / apply), signals its
//                    items with nupdates < max_updates (scatter), and sends each of them the
//                    message -gamma (err U_u + lambda V_i) where |err| > tol (gather's signal)
//   item superstep   every signalled item adds the sum of its messages and signals its users
// Both reductions are done from the SAME old U and V by one vertex-reduction kernel:
//   delta[v] = -gamma (sum_{accepted e} err_e X_nbr(e) + cnt lambda own_v),  cnt = accepted edges
// with the predicate "always" on the user side and "active[u] && fabs(err) > tol" on the item
// side (the item's CSR list is walked, so the message is a gather, not a scatter: no
// floating-point atomic).  The deltas go to buffers; U += dU and V += M are separate commit
// launches, so no factor changes before both sides have been reduced.
// lambda and -gamma are applied in closed form, once per vertex (cnt lambda own), not once per
// edge as the reference's per-edge deltas do: one rounding instead of cnt, same value to rounding.
//
// Layout in HBM: as cf_als.hip (row-major n x D fp64 factors, one CSR per side with u64 offsets,
// u32 neighbour, f32 obs, u32 owner per edge), plus fp64 biases and the delta buffers.  A
// reduction of one side reads about nnz (8 D + 8) bytes and does 4 nnz D flops (dot and axpy):
// bound by the row gathers.
//
// The reduction runs on the shared skeleton of cf_mf_reduce.h (lane mapping, the low / mid / high
// classes on the vertex's TRAIN degree, every summation order: the determinism rule of DESIGN
// 3.12); this file supplies SgdOp, what one edge adds and how the sums become deltas.  A row is
// used by exactly one lane group, so it is gathered straight into registers; ALS stages rows in
// LDS because every lane of its wave needs every row, which is not the case here.
// The dot product is edge_err(): the same fma order over d and the same butterfly as
// group_dot(), called with (U row, V row) from both sides, so err_e has the same float bits on
// the user side and the item side and both agree on every threshold.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cf_internal.h"
#include "cf_mf_reduce.h"

namespace {

// One side of the graph as the kernels see it.
struct SgdSide {
    uint32_t n;
    const uint64_t* off;
    const uint32_t* nbr;
    const float* obs;
    const uint32_t* src;   // owner of each edge
    double* F;             // n x D factors
    double* b;             // biases, NULL for plain SGD
    double* dF;            // n x D pending deltas (users: the gather sum; items: the message)
    double* db;
    uint32_t* nupd;
    uint8_t* flag;         // signalled for the next superstep of this side
    uint8_t* active;       // users: updated in this superstep pair; items: signalled by it
};

struct SgdArgs {
    double gamma, lambda, tol, minval, maxval, mean;
    int D;
};

// err of one edge from the register images of its two rows (elements sl, sl + 8, .. per lane,
// zero beyond D).  Same order as group_dot().  A NaN prediction stays NaN through the clamp
// (std::min / std::max of the reference do the same).
template <int NJ>
__device__ __forceinline__ float edge_err(const double (&u)[NJ], const double (&v)[NJ], bool bias, double mean, double bu,
                                          double bi, float obs, double minval, double maxval) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) s = fma(u[j], v[j], s);
#pragma unroll
    for (int o = kG / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o, kG);
    double p = bias ? mean + bu + bi + s : s;
    p = p > maxval ? maxval : p;
    p = p < minval ? minval : p;
    return (float)(p - (double)obs);
}

__device__ __forceinline__ double sgd_delta(double sum, double cnt, double own, const SgdArgs& a) {
    return -a.gamma * (sum + cnt * a.lambda * own);
}

// The policy of the reduction of side s (ITEM: s holds the items and the neighbours are users of
// side o): D sums err x, the scalar sum err (the bias part), and
//   delta[v] = -gamma (sum + cnt lambda own_v)
template <bool ITEM>
struct SgdOp {
    static constexpr int NS = 1;
    static constexpr bool kCountNan = !ITEM;
    SgdSide s, o;
    SgdArgs a;
    template <int NJ>
    struct Own {
        double row[NJ];
        double bias;
    };
    __host__ __device__ int dim() const { return a.D; }
    __device__ __forceinline__ uint64_t begin(uint32_t v) const { return s.off[v]; }
    __device__ __forceinline__ uint64_t end(uint32_t v) const { return s.off[v + 1]; }
    template <int NJ>
    __device__ __forceinline__ void load_own(Own<NJ>& own, uint32_t v, int sl) const {
        load_row<NJ>(own.row, s.F + (size_t)v * a.D, a.D, sl);
        own.bias = s.b ? s.b[v] : 0.0;
    }
    template <int NJ>
    __device__ __forceinline__ void edge(Acc<NJ, NS>& acc, const Own<NJ>& own, uint64_t e, int sl) const {
        const bool bias = s.b != nullptr;
        const uint32_t w = s.nbr[e];
        if (ITEM && !o.active[w]) return;         // the user did not run: no message on this edge
        double x[NJ];
        load_row<NJ>(x, o.F + (size_t)w * a.D, a.D, sl);
        const double ob = bias ? o.b[w] : 0.0;
        const float err = ITEM ? edge_err<NJ>(x, own.row, bias, a.mean, ob, own.bias, s.obs[e], a.minval, a.maxval)
                               : edge_err<NJ>(own.row, x, bias, a.mean, own.bias, ob, s.obs[e], a.minval, a.maxval);
        if (!ITEM && err != err) acc.nan += sl == 0;
        if (ITEM && !(fabs((double)err) > a.tol)) return;
        const double ed = (double)err;
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc.s[j] = fma(ed, x[j], acc.s[j]);
        acc.x[0] += ed;
        acc.cnt += 1;
    }
    __device__ __forceinline__ void scalar(uint32_t v, double own_bias, double e, double cnt,
                                           unsigned long long* counters) const {
        if (s.b) s.db[v] = sgd_delta(e, cnt, own_bias, a);
        if (ITEM && cnt > 0.0) atomicAdd(&counters[1], (unsigned long long)cnt);   // messages
    }
    __device__ __forceinline__ void finish_elem(uint32_t v, int d, double sum, const double*, double cnt) const {
        s.dF[(size_t)v * a.D + d] = sgd_delta(sum, cnt, s.F[(size_t)v * a.D + d], a);
    }
    __device__ __forceinline__ void finish_scalar(uint32_t v, const double* x, double cnt,
                                                  unsigned long long* counters) const {
        scalar(v, s.b ? s.b[v] : 0.0, x[0], cnt, counters);
    }
    template <int NJ>
    __device__ __forceinline__ void finish_elem_own(const Own<NJ>& own, int jj, uint32_t v, int d, double sum,
                                                    const double*, double cnt) const {
        s.dF[(size_t)v * a.D + d] = sgd_delta(sum, cnt, own.row[jj], a);
    }
    template <int NJ>
    __device__ __forceinline__ void finish_scalar_own(const Own<NJ>& own, uint32_t v, const double* x, double cnt,
                                                      unsigned long long* counters) const {
        scalar(v, own.bias, x[0], cnt, counters);
    }
};

// apply: F += dF, b += db, nupdates += 1 for the active vertices of one side.
__global__ __launch_bounds__(kAT) void sgd_commit_kernel(SgdSide s, int D) {
    const uint64_t idx = (uint64_t)blockIdx.x * kAT + threadIdx.x;
    if (idx >= (uint64_t)s.n * D) return;
    const uint32_t v = (uint32_t)(idx / D);
    if (!s.active[v]) return;
    s.F[idx] += s.dF[idx];
    if (idx % D == 0) {
        if (s.b) s.b[v] += s.db[v];
        s.nupd[v] += 1;
    }
}

// ---- host ---------------------------------------------------------------------------------

struct SgdLayout {
    SgdSide side[2];
    AlsLists lists[2];
    double* ws;
    unsigned long long* counters;
    MfVal val;
    double* partial;   // error block partials, then {train, validate} sums
    double* sums;
    uint32_t seg_cap;
};

void carve_sgd(Carver& c, SgdLayout& f, uint32_t n_users, uint32_t n_items, uint64_t nnz, int D, bool bias,
               uint64_t seg_cap, uint64_t n_val, bool trace) {
    const uint32_t n[2] = {n_users, n_items};
    for (int k = 0; k < 2; ++k) {
        SgdSide& s = f.side[k];
        carve_side(c, s, n[k], nnz);
        s.F = c.take<double>((size_t)n[k] * D);
        s.dF = c.take<double>((size_t)n[k] * D);
        s.b = bias ? c.take<double>(n[k]) : nullptr;
        s.db = bias ? c.take<double>(n[k]) : nullptr;
        carve_lists(c, f.lists[k], n[k], seg_cap);
    }
    f.ws = c.take<double>((size_t)seg_cap * (D + 2));   // D sums, the bias sum, the count
    f.counters = c.take<unsigned long long>(2);
    carve_val(c, f.val, n_val);
    f.partial = c.take<double>(trace ? error_blocks(std::max(nnz, n_val)) : 0);
    f.sums = c.take<double>(2);
    f.seg_cap = (uint32_t)seg_cap;
}

template <bool ITEM>
void launch_reduce(const SgdLayout& f, const SgdArgs& a, const uint32_t rec[4], hipStream_t st) {
    const int k = ITEM ? 1 : 0;
    launch_reduce(SgdOp<ITEM>{f.side[k], f.side[1 - k], a}, f.lists[k], rec, f.ws, f.counters, st);
}

void launch_commit(const SgdSide& s, int D, hipStream_t st) {
    const uint64_t total = (uint64_t)s.n * D;
    if (total) hipLaunchKernelGGL(sgd_commit_kernel, dim3(blocks_for(total)), dim3(kAT), 0, st, s, D);
}

// the edges of side `from` signal side `to`, then `to`'s flags are compacted into its lists
void launch_signal(const SgdLayout& f, int from, uint64_t nnz, uint64_t max_updates, hipStream_t st) {
    const SgdSide& s = f.side[from];
    const SgdSide& t = f.side[1 - from];
    if (nnz && t.n)
        hipLaunchKernelGGL(mf_signal_kernel, dim3(blocks_for(nnz)), dim3(kAT), 0, st, s.src, s.nbr, nnz,
                           (const uint8_t*)s.active, (const uint32_t*)t.nupd, t.flag, max_updates, true);
    launch_compact(t, f.lists[1 - from], st);
}

}  // namespace

extern "C" int cf_sgd_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                          const uint32_t* user_item, const float* user_obs, const uint64_t* item_off,
                          const uint32_t* item_user, const float* item_obs, const cf_sgd_params* params, double* U,
                          double* V, double* bias_user, double* bias_item, uint32_t* nupdates_user,
                          uint32_t* nupdates_item, const uint8_t* activate_user, uint64_t n_validate,
                          const uint32_t* val_user, const uint32_t* val_item, const float* val_obs, double* trace,
                          uint32_t trace_rows, cf_sgd_stats* stats) {
    if (!ctx) return CF_EINVAL;
    if (stats) *stats = cf_sgd_stats{};
    if (!params) return cf_set_error(ctx, CF_EINVAL, "cf_sgd_fit: null params");
    if (stats) stats->gamma_next = params->gamma;
    uint64_t nnz = 0;
    CF_TRY(check_two_csr(ctx, "cf_sgd_fit", n_users, n_items, D, user_off, user_item, user_obs, item_off, item_user,
                         item_obs, &nnz));
    CF_TRY(check_caps(ctx, "cf_sgd_fit", params->max_updates, params->max_supersteps));
    if ((bias_user == nullptr) != (bias_item == nullptr))
        return cf_set_error(ctx, CF_EINVAL, "cf_sgd_fit: exactly one bias array is NULL");
    if ((n_users && (!U || !nupdates_user)) || (n_items && (!V || !nupdates_item)))
        return cf_set_error(ctx, CF_EINVAL, "cf_sgd_fit: null argument");
    const bool want_trace = trace != nullptr && trace_rows > 0;
    const uint64_t n_val = want_trace ? n_validate : 0;
    CF_TRY(check_validation(ctx, "cf_sgd_fit", n_val, val_user, val_item, val_obs, n_users, n_items));
    if (n_users == 0) return CF_OK;   // nothing can be active
    CF_TRY(set_device(ctx));
    const bool bias = bias_user != nullptr;
    if ((nnz + kAT - 1) / kAT > 0x7fffffffull || error_blocks(std::max(nnz, n_val)) > 0x7fffffffull)
        return cf_set_error(ctx, CF_ERANGE, "cf_sgd_fit: too many edges");

    // everything the fit needs exists before its first launch
    const uint64_t seg_cap = std::max(total_segments(n_users, user_off), n_items ? total_segments(n_items, item_off) : 0);
    if (seg_cap > 0xffffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_sgd_fit: too many segments");
    SgdLayout f{};
    CF_TRY(carve_workspace(
        ctx, [&](Carver& c) { carve_sgd(c, f, n_users, n_items, nnz, (int)D, bias, seg_cap, n_val, want_trace); }));
    MfEvents<8> evs;
    for (hipEvent_t& e : evs.e) CF_HIP_CHECK(ctx, hipEventCreate(&e));
    hipStream_t st = nullptr;

    const uint32_t n[2] = {n_users, n_items};
    const uint64_t* h_off[2] = {user_off, item_off};
    const uint32_t* h_nbr[2] = {user_item, item_user};
    const float* h_obs[2] = {user_obs, item_obs};
    double* h_F[2] = {U, V};
    double* h_b[2] = {bias_user, bias_item};
    uint32_t* h_nupd[2] = {nupdates_user, nupdates_item};
    for (int k = 0; k < 2; ++k) {
        if (n[k] == 0) continue;
        const SgdSide& s = f.side[k];
        CF_TRY(upload_side(ctx, s, nnz, h_off[k], h_nbr[k], h_obs[k], h_nupd[k], k == 0 ? activate_user : nullptr, k == 0));
        CF_HIP_CHECK(ctx, hipMemcpy(s.F, h_F[k], sizeof(double) * (size_t)n[k] * D, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemset(s.dF, 0, sizeof(double) * (size_t)n[k] * D));
        if (bias) {
            CF_HIP_CHECK(ctx, hipMemcpy(s.b, h_b[k], sizeof(double) * n[k], hipMemcpyHostToDevice));
            CF_HIP_CHECK(ctx, hipMemset(s.db, 0, sizeof(double) * n[k]));
        }
    }
    CF_TRY(upload_val(ctx, f.val, n_val, val_user, val_item, val_obs));
    CF_HIP_CHECK(ctx, hipMemset(f.counters, 0, 2 * sizeof(unsigned long long)));

    SgdArgs a{params->gamma, params->lambda, params->tol, params->minval, params->maxval, params->global_mean, (int)D};
    const uint64_t max_updates = params->max_updates;
    const uint32_t max_supersteps = params->max_supersteps;
    const SgdSide& su = f.side[0];
    const SgdSide& si = f.side[1];
    uint32_t supersteps = 0;
    uint64_t updates = 0;
    unsigned long long counters[2] = {0, 0};
    double reduce_ms[2] = {0.0, 0.0}, apply_ms = 0.0;
    bool item_step_pending = false;   // events 6, 7 recorded and not read yet
    launch_compact(su, f.lists[0], st);
    for (;;) {
        // the small record of the user side: the active counts per class and the segments
        uint32_t rec_u[4], rec_i[4] = {0, 0, 0, 0};
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(rec_u, f.lists[0].record, sizeof(rec_u), hipMemcpyDeviceToHost));   // waits for the stream
        if (item_step_pending) apply_ms += elapsed(evs.e[6], evs.e[7]);
        item_step_pending = false;
        const uint64_t n_active = (uint64_t)rec_u[0] + rec_u[1] + rec_u[2];
        if (n_active == 0) break;                                   // the run ends when nobody is signalled
        if (max_supersteps && supersteps >= max_supersteps) break;
        if (rec_u[3] > f.seg_cap) return cf_set_error(ctx, CF_EHIP, "cf_sgd_fit: segment list overflow");

        // ---- user superstep: gather sum, scatter (signals), the items' messages, apply ----
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
        launch_reduce<false>(f, a, rec_u, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
        launch_signal(f, 0, nnz, max_updates, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[2], st));
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(rec_i, f.lists[1].record, sizeof(rec_i), hipMemcpyDeviceToHost));
        if (rec_i[3] > f.seg_cap) return cf_set_error(ctx, CF_EHIP, "cf_sgd_fit: segment list overflow");
        const uint64_t n_signalled = (uint64_t)rec_i[0] + rec_i[1] + rec_i[2];
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[3], st));
        if (n_signalled) launch_reduce<true>(f, a, rec_i, st);      // from the old U and V
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[4], st));
        launch_commit(su, (int)D, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[5], st));
        a.gamma *= params->step_dec;                                // sgd.cpp:372-387: after every user superstep
        const uint32_t row = supersteps / 2;
        const bool trace_row = want_trace && row < trace_rows;
        if (trace_row) {   // new U, old V
            CF_HIP_CHECK(ctx, hipMemsetAsync(f.sums, 0, 2 * sizeof(double), st));
            if (nnz)
                launch_error(st, nnz, su.src, su.nbr, su.obs, su.F, si.F, (int)D, su.b, si.b, a.mean, a.minval, a.maxval,
                             f.partial, f.sums);
            if (n_val)
                launch_error(st, n_val, f.val.user, f.val.item, f.val.obs, su.F, si.F, (int)D, su.b, si.b, a.mean, a.minval,
                             a.maxval, f.partial, f.sums + 1);
        }
        ++supersteps;
        updates += n_active;
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(counters, f.counters, sizeof(counters), hipMemcpyDeviceToHost));   // waits
        if (trace_row) CF_HIP_CHECK(ctx, hipMemcpy(trace + 2 * (size_t)row, f.sums, 2 * sizeof(double), hipMemcpyDeviceToHost));
        reduce_ms[0] += elapsed(evs.e[0], evs.e[1]);
        reduce_ms[1] += elapsed(evs.e[3], evs.e[4]);
        apply_ms += elapsed(evs.e[1], evs.e[2]) + elapsed(evs.e[4], evs.e[5]);
        if (counters[0]) break;                                     // numeric errors: the caller reports them
        if (n_signalled == 0) break;
        if (max_supersteps && supersteps >= max_supersteps) break;  // the pending messages are dropped

        // ---- item superstep: the signalled items add their messages and signal their users ----
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[6], st));
        launch_commit(si, (int)D, st);
        launch_signal(f, 1, nnz, max_updates, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[7], st));
        item_step_pending = true;
        ++supersteps;
        updates += n_signalled;
    }
    CF_HIP_CHECK(ctx, hipDeviceSynchronize());
    for (int q = 0; q < 2; ++q) {
        if (n[q] == 0) continue;
        const SgdSide& s = f.side[q];
        CF_HIP_CHECK(ctx, hipMemcpy(h_F[q], s.F, sizeof(double) * (size_t)n[q] * D, hipMemcpyDeviceToHost));
        if (bias) CF_HIP_CHECK(ctx, hipMemcpy(h_b[q], s.b, sizeof(double) * n[q], hipMemcpyDeviceToHost));
        CF_HIP_CHECK(ctx, hipMemcpy(h_nupd[q], s.nupd, sizeof(uint32_t) * n[q], hipMemcpyDeviceToHost));
    }
    ctx->sgd_reduce_ms[0] = (float)reduce_ms[0];
    ctx->sgd_reduce_ms[1] = (float)reduce_ms[1];
    if (stats) {
        stats->supersteps = supersteps;
        stats->updates = updates;
        stats->messages = counters[1];
        stats->n_nan = counters[0];
        stats->gamma_next = a.gamma;
        stats->reduce_ms = (float)(reduce_ms[0] + reduce_ms[1]);
        stats->apply_ms = (float)apply_ms;
    }
    return CF_OK;
}

extern "C" int cf_sgd_timing(cf_ctx* ctx, float* user_reduce_ms, float* item_reduce_ms) {
    if (!ctx) return CF_EINVAL;
    if (user_reduce_ms) *user_reduce_ms = ctx->sgd_reduce_ms[0];
    if (item_reduce_ms) *item_reduce_ms = ctx->sgd_reduce_ms[1];
    return CF_OK;
}

extern "C" int cf_sgd_error(cf_ctx* ctx, uint64_t n_edges, const uint32_t* user, const uint32_t* item, const float* obs,
                            uint32_t n_users, uint32_t n_items, uint32_t D, const double* U, const double* V,
                            const double* bias_user, const double* bias_item, double global_mean, double minval,
                            double maxval, double* sum_sq) {
    if (!ctx) return CF_EINVAL;
    if (!sum_sq) return cf_set_error(ctx, CF_EINVAL, "cf_sgd_error: null result");
    *sum_sq = 0.0;
    CF_TRY(check_pairs(ctx, "cf_sgd_error", n_edges, user, item, U, V, D, n_users, n_items));
    if ((bias_user == nullptr) != (bias_item == nullptr))
        return cf_set_error(ctx, CF_EINVAL, "cf_sgd_error: exactly one bias array is NULL");
    if (n_edges && !obs) return cf_set_error(ctx, CF_EINVAL, "cf_sgd_error: null ratings");
    if (n_edges == 0) return CF_OK;
    CF_TRY(set_device(ctx));
    const uint64_t blocks = error_blocks(n_edges);
    if (blocks > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_sgd_error: too many edges");
    PairLayout p{};
    CF_TRY(upload_pairs(ctx, p, n_edges, user, item, obs, n_users, n_items, D, U, V, (size_t)blocks + 1, bias_user,
                        bias_item));
    launch_error(nullptr, n_edges, p.user, p.item, p.obs, p.U, p.V, (int)D, p.bu, p.bi, global_mean, minval, maxval, p.out,
                 p.out + blocks);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(sum_sq, p.out + blocks, sizeof(double), hipMemcpyDeviceToHost));
    return CF_OK;
}

extern "C" int cf_sgd_predict(cf_ctx* ctx, uint64_t n_pairs, const uint32_t* user, const uint32_t* item,
                              uint32_t n_users, uint32_t n_items, uint32_t D, const double* U, const double* V,
                              const double* bias_user, const double* bias_item, double global_mean, int clamp,
                              double minval, double maxval, double* pred) {
    if (!ctx) return CF_EINVAL;
    CF_TRY(check_pairs(ctx, "cf_sgd_predict", n_pairs, user, item, U, V, D, n_users, n_items));
    if ((bias_user == nullptr) != (bias_item == nullptr))
        return cf_set_error(ctx, CF_EINVAL, "cf_sgd_predict: exactly one bias array is NULL");
    if (n_pairs && !pred) return cf_set_error(ctx, CF_EINVAL, "cf_sgd_predict: null result");
    if (n_pairs == 0) return CF_OK;
    CF_TRY(set_device(ctx));
    const uint64_t blocks = (n_pairs * kG + kAT - 1) / kAT;
    if (blocks > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_sgd_predict: too many pairs");
    PairLayout p{};
    CF_TRY(upload_pairs(ctx, p, n_pairs, user, item, nullptr, n_users, n_items, D, U, V, n_pairs, bias_user, bias_item));
    hipLaunchKernelGGL(mf_predict_kernel, dim3((unsigned)blocks), dim3(kAT), 0, nullptr, n_pairs, (const uint32_t*)p.user,
                       (const uint32_t*)p.item, (const double*)p.U, (const double*)p.V, (int)D, (const double*)p.bu,
                       (const double*)p.bi, global_mean, clamp, minval, maxval, p.out);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(pred, p.out, sizeof(double) * n_pairs, hipMemcpyDeviceToHost));
    return CF_OK;
}
