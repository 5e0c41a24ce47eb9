// cf_nmf.hip -- non-negative matrix factorization under the generalised Kullback-Leibler
// divergence on gfx950 (Lee and Seung's multiplicative rules), fp64 throughout.
//
// R ~ U V^T with every component >= CF_NMF_EPS.  For an edge (u, i, r), r >= 0, p = U_u.V_i:
//   OBSERVED  L = sum_edges [r log(r / p) - r + p]                 the rated pairs only
//   GRID      L = sum_edges [r log(r / p) - r] + s_U.s_V           every pair of the grid, unrated = 0
// with s_F[d] the sum of column d over ALL rows of F (Poisson factorization).  The reference
// nmf.cpp sums the numerator below over every edge of the graph into one vector shared by all
// vertices, which is no factorization; its pre_iter column sum is the GRID denominator, and that
// is what this file keeps of it.
//
// A half-sweep updates every vertex v of one side in place from the other side's rows x:
//   F_v[d] <- F_v[d] * (sum_{e in N(v)} x_e[d] r_e / p_e) / den[d]
//   den[d] = sum_{e in N(v)} x_e[d] (OBSERVED),  s_X[d] (GRID);   below CF_NMF_EPS -> CF_NMF_EPS
// A sweep is the user half-sweep, then the item half-sweep.  A vertex reads only its own row and
// the other side's rows, and writes only its own row, so the update needs no second buffer.
// A vertex without edges: OBSERVED leaves its row alone; GRID sets it to CF_NMF_EPS.
//
// The update is a policy (NmfOp) of the three-class vertex reduction of cf_mf_reduce.h: per edge
// one 8-lane dot product (the fma order and butterfly of group_dot()), one division r / p and D
// fma into the numerator; OBSERVED asks the skeleton for its second D sums (TWO) and adds the row
// itself to them.  Every vertex is active in every half-sweep: the class lists are compacted
// once per fit and side.  The finish step divides, floors and counts floor events with an integer
// atomic; no floating-point atomic anywhere.
// Column sum: one workgroup per slice of kSumRows rows; thread (rr, d) adds rows rr, rr + RP, ..
// of the slice (RP = kAT / D rows per trip, contiguous loads), the RP partials are added in rr
// order and the slice partials in slice order.
// Loss: edge-parallel over the user CSR with the two-level fixed reduction of mf_error_kernel /
// als_error_final_kernel; GRID adds the D-term dot s_U.s_V in index order in one thread.
// Determinism: a vertex's new row depends only on its own edge list, the other
// side's rows and, in GRID mode, the bits of s.
//
// A half-sweep reads about nnz (8 D + 8) + n 8 D bytes, like SGD's reduction.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cf_internal.h"
#include "cf_mf_reduce.h"

namespace {

constexpr int kSumRows = 1024;   // rows per slice of the column sum

struct NmfSide {
    uint32_t n;
    const uint64_t* off;
    const uint32_t* nbr;
    const float* obs;
    double* F;             // n x D factors
    uint8_t* flag;         // all ones until the one compaction of the fit
    uint8_t* active;
};

// ---- per-vertex update ----------------------------------------------------------------------

// The policy of the reduction of side s from the rows X of the other side.  GRID: the D sums are
// the numerator and the denominator is den (the other side's column sum).  Otherwise the skeleton
// runs with TWO and acc.t is the denominator.
template <bool GRID>
struct NmfOp {
    static constexpr int NS = 0;
    static constexpr bool kCountNan = false;
    NmfSide s;
    const double* X;
    const double* den;
    int D;
    unsigned long long* floored;   // floor events of the fit
    template <int NJ>
    struct Own {
        double row[NJ];
    };
    __host__ __device__ int dim() const { return D; }
    __device__ __forceinline__ uint64_t begin(uint32_t v) const { return s.off[v]; }
    __device__ __forceinline__ uint64_t end(uint32_t v) const { return s.off[v + 1]; }
    template <int NJ>
    __device__ __forceinline__ void load_own(Own<NJ>& own, uint32_t v, int sl) const {
        load_row<NJ>(own.row, s.F + (size_t)v * D, D, sl);
    }
    template <int NJ>
    __device__ __forceinline__ void edge(Acc<NJ, NS, !GRID>& acc, const Own<NJ>& own, uint64_t e, int sl) const {
        double x[NJ];
        load_row<NJ>(x, X + (size_t)s.nbr[e] * D, D, sl);
        double p = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) p = fma(own.row[j], x[j], p);
#pragma unroll
        for (int o = kG / 2; o >= 1; o >>= 1) p += __shfl_xor(p, o, kG);
        const double q = (double)s.obs[e] / p;   // r = 0 adds +0.0 to every sum
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc.s[j] = fma(q, x[j], acc.s[j]);
        if constexpr (!GRID) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc.t[j] += x[j];
        }
        acc.cnt += 1;
    }
    // the new component from the old one
    __device__ __forceinline__ void put(uint32_t v, int d, double old, double num, double dn, double cnt) const {
        if (cnt == 0.0) {
            if (!GRID) return;   // no edges: the row stays as it is
            num = 0.0;
            dn = 1.0;            // numerator 0 whatever s holds
        }
        double f = old * num / dn;
        if (f < CF_NMF_EPS) {
            f = CF_NMF_EPS;
            atomicAdd(floored, 1ull);
        }
        s.F[(size_t)v * D + d] = f;
    }
    __device__ __forceinline__ void finish_elem(uint32_t v, int d, double sum, const double*, double cnt) const {
        put(v, d, s.F[(size_t)v * D + d], sum, den[d], cnt);
    }
    __device__ __forceinline__ void finish_elem2(uint32_t v, int d, double sum, double sum2, const double*,
                                                 double cnt) const {
        put(v, d, s.F[(size_t)v * D + d], sum, sum2, cnt);
    }
    template <int NJ>
    __device__ __forceinline__ void finish_elem_own(const Own<NJ>& own, int jj, uint32_t v, int d, double sum,
                                                    const double*, double cnt) const {
        put(v, d, own.row[jj], sum, den[d], cnt);
    }
    template <int NJ>
    __device__ __forceinline__ void finish_elem2_own(const Own<NJ>& own, int jj, uint32_t v, int d, double sum,
                                                     double sum2, const double*, double cnt) const {
        put(v, d, own.row[jj], sum, sum2, cnt);
    }
    __device__ __forceinline__ void finish_scalar(uint32_t, const double*, double, unsigned long long*) const {}
    template <int NJ>
    __device__ __forceinline__ void finish_scalar_own(const Own<NJ>&, uint32_t, const double*, double,
                                                      unsigned long long*) const {}
};

// ---- column sum ------------------------------------------------------------------------------

__global__ __launch_bounds__(kAT) void nmf_colsum_slice_kernel(const double* __restrict__ F, uint32_t n, int D,
                                                              double* __restrict__ partial) {
    __shared__ double part[kAT];
    const uint64_t r0 = (uint64_t)blockIdx.x * kSumRows;
    const int len = (int)std::min<uint64_t>((uint64_t)kSumRows, (uint64_t)n - r0);
    const int RP = kAT / D;   // rows per trip; D <= 64, so at least 4
    const int t = threadIdx.x, rr = t / D, d = t - rr * D;
    double acc = 0.0;
    if (rr < RP)
        for (int r = rr; r < len; r += RP) acc += F[(r0 + (uint64_t)r) * D + d];
    part[t] = acc;
    __syncthreads();
    if (t < D) {
        double sum = part[t];
        for (int q = 1; q < RP; ++q) sum += part[q * D + t];
        partial[(size_t)blockIdx.x * D + t] = sum;
    }
}

// s = the slice partials added in slice order (one chain per column; the loads of kAhead slices
// are issued together, as ials_gram_sum_kernel does).
__global__ __launch_bounds__(64) void nmf_colsum_sum_kernel(const double* __restrict__ partial, uint32_t n_slices, int D,
                                                           double* __restrict__ s) {
    const int t = threadIdx.x;
    if (t >= D) return;
    constexpr uint32_t kAhead = 32;
    double acc = 0.0;
    uint32_t q = 0;
    for (; q + kAhead <= n_slices; q += kAhead) {
        double v[kAhead];
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) v[j] = partial[(size_t)(q + j) * D + t];
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) acc += v[j];
    }
    for (; q < n_slices; ++q) acc += partial[(size_t)q * D + t];
    s[t] = acc;
}

// ---- loss ----------------------------------------------------------------------------------

// Level 1: block b sums the terms of edges [b kErrPerBlock, (b + 1) kErrPerBlock) of the user CSR:
// group g takes edges g, g + 32, .. in order, then a tree.
template <bool GRID>
__global__ __launch_bounds__(kAT) void nmf_loss_kernel(uint64_t n, const uint32_t* __restrict__ user,
                                                      const uint32_t* __restrict__ item, const float* __restrict__ obs,
                                                      const double* __restrict__ U, const double* __restrict__ V, int D,
                                                      double* partial) {
    __shared__ double s_v[kAT];
    const int grp = threadIdx.x / kG, sl = threadIdx.x & (kG - 1);
    const uint64_t e0 = (uint64_t)blockIdx.x * kErrPerBlock;
    double acc = 0.0;
    for (int k = 0; k < kErrPerBlock / (kAT / kG); ++k) {
        const uint64_t e = e0 + (uint64_t)k * (kAT / kG) + grp;
        if (e >= n) break;   // per group
        const double p = group_dot(U + (size_t)user[e] * D, V + (size_t)item[e] * D, D, sl);
        const double r = (double)obs[e];
        double term = r > 0.0 ? r * log(r / p) - r : 0.0;
        if (!GRID) term += p;
        acc += term;
    }
    s_v[threadIdx.x] = sl == 0 ? acc : 0.0;
    block_tree_sum(s_v);
    if (threadIdx.x == 0) partial[blockIdx.x] = s_v[0];
}

// GRID: *out = the edge sum + s_U.s_V, the dot one fma chain in index order.
__global__ void nmf_loss_grid_kernel(const double* __restrict__ edges, const double* __restrict__ sU,
                                     const double* __restrict__ sV, int D, double* out) {
    if (threadIdx.x || blockIdx.x) return;
    double dot = 0.0;
    for (int d = 0; d < D; ++d) dot = fma(sU[d], sV[d], dot);
    *out = *edges + dot;
}

// ---- host ---------------------------------------------------------------------------------

inline uint32_t sum_slices(uint32_t n) { return (uint32_t)(((uint64_t)n + kSumRows - 1) / kSumRows); }

// s [D] = the column sums of the n x D device matrix F.
void launch_colsum(const double* F, uint32_t n, int D, double* partial, double* s, hipStream_t st) {
    const uint32_t slices = sum_slices(n);
    if (slices) hipLaunchKernelGGL(nmf_colsum_slice_kernel, dim3(slices), dim3(kAT), 0, st, F, n, D, partial);
    hipLaunchKernelGGL(nmf_colsum_sum_kernel, dim3(1), dim3(64), 0, st, (const double*)partial, slices, D, s);
}

// The graph of one call, host side: index 0 users, 1 items.
struct NmfArgs {
    uint32_t n[2];
    uint32_t D;
    const uint64_t* off[2];
    const uint32_t* nbr[2];
    const float* obs[2];
    int mode;
    uint64_t nnz;
};

struct NmfLayout {
    NmfSide side[2];
    AlsLists lists[2];
    uint32_t* user_of_edge;   // owner of each edge of the user CSR (the loss runs over it)
    double* ws;               // segment partials
    double* spart;            // column-sum slice partials
    double* s[2];             // column sums
    unsigned long long* floored;
    double* pe;               // loss block partials
    double* edge_sum;
    double* trace;
};

void carve_nmf(Carver& c, NmfLayout& f, const NmfArgs& a, const uint64_t segs[2], uint32_t n_trace) {
    const int D = (int)a.D;
    for (int k = 0; k < 2; ++k) {
        NmfSide& s = f.side[k];
        s.n = a.n[k];
        s.off = c.take<uint64_t>((size_t)a.n[k] + 1);
        s.nbr = c.take<uint32_t>(a.nnz);
        s.obs = c.take<float>(a.nnz);
        s.F = c.take<double>((size_t)a.n[k] * D);
        s.flag = c.take<uint8_t>(a.n[k]);
        s.active = c.take<uint8_t>(a.n[k]);
        carve_lists(c, f.lists[k], a.n[k], segs[k]);
        f.s[k] = c.take<double>(D);
    }
    f.user_of_edge = c.take<uint32_t>(a.nnz);
    f.ws = c.take<double>((size_t)std::max(segs[0], segs[1]) * (2 * D + 1));   // 2 D sums and the count
    f.spart = c.take<double>((size_t)sum_slices(std::max(a.n[0], a.n[1])) * D);
    f.floored = c.take<unsigned long long>(1);
    f.pe = c.take<double>(error_blocks(a.nnz));
    f.edge_sum = c.take<double>(1);
    f.trace = c.take<double>(n_trace);
}

// The checks cf_nmf_fit and cf_nmf_loss share.
int check_nmf(cf_ctx* ctx, const char* fn, NmfArgs& a, const double* U, const double* V) {
    const std::string f(fn);
    if (a.mode != CF_NMF_OBSERVED && a.mode != CF_NMF_GRID) return cf_set_error(ctx, CF_EINVAL, f + ": unknown mode");
    CF_TRY(check_two_csr(ctx, fn, a.n[0], a.n[1], a.D, a.off[0], a.nbr[0], a.obs[0], a.off[1], a.nbr[1], a.obs[1],
                         &a.nnz));
    if ((a.n[0] && !U) || (a.n[1] && !V)) return cf_set_error(ctx, CF_EINVAL, f + ": null argument");
    for (int k = 0; k < 2; ++k)
        for (uint64_t e = 0; e < a.nnz; ++e)
            if (!(a.obs[k][e] >= 0.0f) || !std::isfinite(a.obs[k][e]))
                return cf_set_error(ctx, CF_EINVAL, f + ": a rating that is negative or not finite");
    const double* F[2] = {U, V};
    for (int k = 0; k < 2; ++k)
        for (size_t t = 0; t < (size_t)a.n[k] * a.D; ++t)
            if (!(F[k][t] >= CF_NMF_EPS) || !std::isfinite(F[k][t]))
                return cf_set_error(ctx, CF_EINVAL, f + ": a factor component below CF_NMF_EPS or not finite");
    return CF_OK;
}

int upload_nmf(cf_ctx* ctx, const NmfLayout& f, const NmfArgs& a, const double* const F[2]) {
    for (int k = 0; k < 2; ++k) {
        if (a.n[k] == 0) continue;
        const NmfSide& s = f.side[k];
        const size_t n = a.n[k];
        CF_HIP_CHECK(ctx, hipMemcpy((void*)s.off, a.off[k], sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice));
        if (a.nnz) {
            CF_HIP_CHECK(ctx, hipMemcpy((void*)s.nbr, a.nbr[k], sizeof(uint32_t) * a.nnz, hipMemcpyHostToDevice));
            CF_HIP_CHECK(ctx, hipMemcpy((void*)s.obs, a.obs[k], sizeof(float) * a.nnz, hipMemcpyHostToDevice));
        }
        CF_HIP_CHECK(ctx, hipMemcpy(s.F, F[k], sizeof(double) * n * a.D, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemset(s.flag, 1, n));
        CF_HIP_CHECK(ctx, hipMemset(s.active, 0, n));
    }
    if (a.nnz) CF_TRY(upload_edge_owners(ctx, f.user_of_edge, a.n[0], a.off[0], a.nnz));
    CF_HIP_CHECK(ctx, hipMemset(f.floored, 0, sizeof(unsigned long long)));
    return CF_OK;
}

// The loss of the factors on the device into *out (device).  GRID computes both column sums anew.
void launch_loss(const NmfLayout& f, const NmfArgs& a, double* out, hipStream_t st) {
    const int D = (int)a.D;
    const bool grid = a.mode == CF_NMF_GRID;
    const uint64_t be = error_blocks(a.nnz);
    if (be) {
        auto kern = grid ? nmf_loss_kernel<true> : nmf_loss_kernel<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)be), dim3(kAT), 0, st, a.nnz, (const uint32_t*)f.user_of_edge,
                           f.side[0].nbr, f.side[0].obs, (const double*)f.side[0].F, (const double*)f.side[1].F, D, f.pe);
    }
    hipLaunchKernelGGL(als_error_final_kernel, dim3(1), dim3(kAT), 0, st, (const double*)f.pe, be, grid ? f.edge_sum : out);
    if (!grid) return;
    for (int k = 0; k < 2; ++k) launch_colsum(f.side[k].F, a.n[k], D, f.spart, f.s[k], st);
    hipLaunchKernelGGL(nmf_loss_grid_kernel, dim3(1), dim3(64), 0, st, (const double*)f.edge_sum, (const double*)f.s[0],
                       (const double*)f.s[1], D, out);
}

// One half-sweep of side k.
void launch_half_sweep(const NmfLayout& f, const NmfArgs& a, int k, const uint32_t rec[4], hipStream_t st) {
    const int D = (int)a.D;
    if (a.mode == CF_NMF_GRID)
        launch_reduce<false>(NmfOp<true>{f.side[k], f.side[1 - k].F, f.s[1 - k], D, f.floored}, f.lists[k], rec, f.ws,
                             f.floored, st);
    else
        launch_reduce<true>(NmfOp<false>{f.side[k], f.side[1 - k].F, nullptr, D, f.floored}, f.lists[k], rec, f.ws,
                            f.floored, st);
}

}  // namespace

extern "C" int cf_debug_nmf_sum_rows(void) { return kSumRows; }

extern "C" int cf_mf_colsum(cf_ctx* ctx, uint32_t n, uint32_t D, const double* F, double* s) {
    if (!ctx) return CF_EINVAL;
    if (D == 0) return cf_set_error(ctx, CF_EINVAL, "cf_mf_colsum: D = 0");
    if (D > CF_ALS_MAX_D) return cf_set_error(ctx, CF_ERANGE, "cf_mf_colsum: D above CF_ALS_MAX_D");
    if (!s || (n && !F)) return cf_set_error(ctx, CF_EINVAL, "cf_mf_colsum: null argument");
    CF_TRY(set_device(ctx));
    double *dF = nullptr, *part = nullptr, *ds = nullptr;
    CF_TRY(carve_workspace(ctx, [&](Carver& c) {
        dF = c.take<double>((size_t)n * D);
        part = c.take<double>((size_t)sum_slices(n) * D);
        ds = c.take<double>(D);
    }));
    if (n) CF_HIP_CHECK(ctx, hipMemcpy(dF, F, sizeof(double) * (size_t)n * D, hipMemcpyHostToDevice));
    launch_colsum(dF, n, (int)D, part, ds, nullptr);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(s, ds, sizeof(double) * D, hipMemcpyDeviceToHost));
    return CF_OK;
}

extern "C" int cf_nmf_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                          const uint32_t* user_item, const float* user_obs, const uint64_t* item_off,
                          const uint32_t* item_user, const float* item_obs, int mode, uint32_t n_sweeps, double* U,
                          double* V, double* loss_trace, cf_nmf_stats* stats) {
    if (!ctx) return CF_EINVAL;
    if (stats) *stats = cf_nmf_stats{};
    NmfArgs a{{n_users, n_items}, D, {user_off, item_off}, {user_item, item_user}, {user_obs, item_obs}, mode, 0};
    CF_TRY(check_nmf(ctx, "cf_nmf_fit", a, U, V));
    if (n_sweeps == 0 || (n_users == 0 && n_items == 0)) return CF_OK;   // no half-sweep runs: U, V untouched
    if (n_sweeps > (1u << 24)) return cf_set_error(ctx, CF_ERANGE, "cf_nmf_fit: more than 2^24 sweeps");
    CF_TRY(set_device(ctx));

    // everything the fit needs exists before its first launch
    const uint64_t segs[2] = {total_segments(n_users, user_off), n_items ? total_segments(n_items, item_off) : 0};
    if (std::max(segs[0], segs[1]) > 0xffffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_nmf_fit: too many segments");
    if (error_blocks(a.nnz) > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_nmf_fit: too many edges");
    NmfLayout f{};
    CF_TRY(carve_workspace(ctx, [&](Carver& c) { carve_nmf(c, f, a, segs, 2 * n_sweeps); }));
    MfEvents<4> evs;
    for (hipEvent_t& e : evs.e) CF_HIP_CHECK(ctx, hipEventCreate(&e));
    hipStream_t st = nullptr;
    const double* h_in[2] = {U, V};
    double* h_F[2] = {U, V};
    CF_TRY(upload_nmf(ctx, f, a, h_in));

    // every vertex is active in every half-sweep: one compaction per side
    uint32_t rec[2][4];
    for (int k = 0; k < 2; ++k) {
        launch_compact(f.side[k], f.lists[k], st);
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(rec[k], f.lists[k].record, sizeof(rec[k]), hipMemcpyDeviceToHost));
        if (rec[k][3] > segs[k]) return cf_set_error(ctx, CF_EHIP, "cf_nmf_fit: segment list overflow");
    }
    double sum_ms = 0.0, update_ms = 0.0, loss_ms = 0.0;
    for (uint32_t h = 0; h < 2 * n_sweeps; ++h) {
        const int k = (int)(h & 1);   // users, then items
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
        if (mode == CF_NMF_GRID) launch_colsum(f.side[1 - k].F, a.n[1 - k], (int)D, f.spart, f.s[1 - k], st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
        launch_half_sweep(f, a, k, rec[k], st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[2], st));
        if (loss_trace) launch_loss(f, a, f.trace + h, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[3], st));
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipEventSynchronize(evs.e[3]));
        sum_ms += elapsed(evs.e[0], evs.e[1]);
        update_ms += elapsed(evs.e[1], evs.e[2]);
        loss_ms += elapsed(evs.e[2], evs.e[3]);
    }
    CF_HIP_CHECK(ctx, hipDeviceSynchronize());
    for (int k = 0; k < 2; ++k)
        if (a.n[k])
            CF_HIP_CHECK(ctx, hipMemcpy(h_F[k], f.side[k].F, sizeof(double) * (size_t)a.n[k] * D, hipMemcpyDeviceToHost));
    if (loss_trace)
        CF_HIP_CHECK(ctx, hipMemcpy(loss_trace, f.trace, sizeof(double) * 2 * n_sweeps, hipMemcpyDeviceToHost));
    unsigned long long floored = 0;
    CF_HIP_CHECK(ctx, hipMemcpy(&floored, f.floored, sizeof(floored), hipMemcpyDeviceToHost));
    if (stats) {
        stats->sweeps = n_sweeps;
        stats->n_floored = floored;
        stats->sum_ms = (float)sum_ms;
        stats->update_ms = (float)update_ms;
        stats->loss_ms = loss_trace ? (float)loss_ms : 0.0f;
    }
    return CF_OK;
}

extern "C" int cf_nmf_loss(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                           const uint32_t* user_item, const float* user_obs, const uint64_t* item_off,
                           const uint32_t* item_user, const float* item_obs, int mode, const double* U, const double* V,
                           double* loss) {
    if (!ctx) return CF_EINVAL;
    if (!loss) return cf_set_error(ctx, CF_EINVAL, "cf_nmf_loss: null result");
    *loss = 0.0;
    NmfArgs a{{n_users, n_items}, D, {user_off, item_off}, {user_item, item_user}, {user_obs, item_obs}, mode, 0};
    CF_TRY(check_nmf(ctx, "cf_nmf_loss", a, U, V));
    if (n_users == 0 && n_items == 0) return CF_OK;
    if (error_blocks(a.nnz) > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_nmf_loss: too many edges");
    CF_TRY(set_device(ctx));
    const uint64_t segs[2] = {0, 0};   // no update runs: no segment lists
    NmfLayout f{};
    CF_TRY(carve_workspace(ctx, [&](Carver& c) { carve_nmf(c, f, a, segs, 1); }));
    const double* h_in[2] = {U, V};
    CF_TRY(upload_nmf(ctx, f, a, h_in));
    launch_loss(f, a, f.trace, nullptr);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(loss, f.trace, sizeof(double), hipMemcpyDeviceToHost));
    return CF_OK;
}
