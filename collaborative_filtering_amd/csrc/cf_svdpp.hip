// cf_svdpp.hip -- SVD++ matrix factorization on gfx950 (svdpp.cpp:268-397,412-499 on the
// synchronous engine with --interval 0), fp64 throughout.  cf_abi.h has the full update rule.
//
// A vertex's phase is the parity of its own nupdates (even = 1, odd = 2), so one superstep can
// hold vertices of both phases: every kernel below takes the phase per vertex, through the
// per-phase active lists that the compaction of cf_mf_common.h builds.
//   user superstep   phase-1 users: W_u = usrNorm_u sum Y_i over EVERY edge of any role (P1)
//                    phase-2 users: dU_u, dbu from the TRAIN edges with the row V_i + Y_i in the
//                                   dot and V_i in the axpy (U2)
//                    items signalled, in phase 2 and with updates left: their messages, a gather
//                                   over the item's own TRAIN list that accepts an edge iff its
//                                   user is active and in phase 2 (I2); an item in phase 1 gets no
//                                   reduction at all
//   item superstep   phase-2 items add their messages; every signalled item counts an update
// The reductions of one user superstep all read the values of its start; the results go to the
// delta buffers, and commit, signalling and compaction are separate launches.
//
// Layout in HBM: one row of 2 D doubles per vertex, [U_u | W_u] and [V_i | Y_i], so the second
// row of every gather is the same contiguous piece (320 B at D = 20); the ABI keeps four n x D
// arrays and the copies in and out interleave them on the host.  The all-role list of a user is
// its TRAIN items followed by its implicit items (one CSR built on the host).
//
// The three reductions run on the shared skeleton of cf_mf_reduce.h (work shape, lane mapping,
// every summation order: the determinism rule of DESIGN 3.12), with the classes taken on the
// degree of the list that is walked (all-role degree for P1, TRAIN degree for U2 and I2); this
// file supplies PpOp<kP1 | kU2 | kI2>.
// Every kind reduces to D + 3 numbers per vertex: D sums, sum err, sum err c_u, count, with
//   P1  s = sum Y_i
//   U2  s = sum err V_i,            e = sum err                  (reg: user_factor_reg U_u e)
//   I2  s = sum err (U_u + W_u),    e = sum err,  e2 = sum err c_u,  c_u = (float)(step2 usrNorm_u)
// and the regularisers are applied in closed form by PpOp::finish_*(), once per vertex.
// edge_err() is one function called with (U row, V row, Y row) from both sides, so err_e has the
// same float bits in U2 and I2.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cf_internal.h"
#include "cf_mf_reduce.h"

namespace {

enum : int { kP1 = 0, kU2 = 1, kI2 = 2 };

// One side of the graph as the kernels see it (TRAIN CSR).
struct PpSide {
    uint32_t n;
    const uint64_t* off;
    const uint32_t* nbr;
    const float* obs;
    const uint32_t* src;   // owner of each edge
    double* F;             // n x 2D: [U | W] or [V | Y]
    double* b;
    double* dF;            // n x 2D pending: users [dU | new W], items [dV | dY]
    double* db;
    uint32_t* nupd;
    uint8_t* flag;         // signalled for the next superstep of this side
    uint8_t* active;       // items: signalled in this superstep pair, any phase (users: act1 / act2 of PpGraph)
};

// What the compaction needs of one (side, phase) view.
struct PpView {
    uint32_t n;
    const uint64_t* off;   // the degrees that give the class
    uint8_t* flag;
    uint8_t* active;
};

struct PpGraph {
    PpSide u, i;
    const uint64_t* all_off;    // users: every role, TRAIN items first
    const uint32_t* all_item;
    const uint32_t* all_src;
    const float* unorm;         // (float)(1 / sqrt(all-role degree)), 0 without edges
    uint8_t* act1;              // users running phase 1 in this superstep
    uint8_t* act2;              // users running phase 2
    uint8_t* iact2;             // items whose messages are reduced and added
};

struct PpArgs {
    float ubs, ibs, ufs, ifs, if2s;   // the five steps
    float ufr, ifr, if2r;             // the regularisers that have an effect
    double minval, maxval, mean;
    int D;
};

// err of one TRAIN edge from the register images of U_u, V_i and Y_i (svdpp.cpp:287-291).  A NaN
// prediction stays NaN through the clamp, as std::min / std::max of the reference leave it.
template <int NJ>
__device__ __forceinline__ float edge_err(const double (&u)[NJ], const double (&v)[NJ], const double (&y)[NJ], double mean,
                                          double bu, double bi, float obs, double minval, double maxval) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) s = fma(u[j], v[j] + y[j], s);
#pragma unroll
    for (int o = kG / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o, kG);
    double p = mean + bu + bi + s;
    p = p > maxval ? maxval : p;
    p = p < minval ? minval : p;
    return (float)((double)obs - p);
}

// The policy of one kind of reduction.  own.a / own.b: U_u (U2) or V_i, Y_i (I2); the sums x are
// {sum err, sum err c_u}.
template <int MODE>
struct PpOp {
    static constexpr int NS = 2;
    static constexpr bool kCountNan = MODE == kU2;
    PpGraph G;
    PpArgs a;
    template <int NJ>
    struct Own {
        double a[NJ], b[NJ];
        double bias;
    };
    __host__ __device__ int dim() const { return a.D; }
    // P1: the all-role list; U2, I2: the TRAIN list
    __device__ __forceinline__ uint64_t begin(uint32_t v) const {
        return MODE == kP1 ? G.all_off[v] : (MODE == kU2 ? G.u.off[v] : G.i.off[v]);
    }
    __device__ __forceinline__ uint64_t end(uint32_t v) const {
        return MODE == kP1 ? G.all_off[v + 1] : (MODE == kU2 ? G.u.off[v + 1] : G.i.off[v + 1]);
    }
    template <int NJ>
    __device__ __forceinline__ void load_own(Own<NJ>& own, uint32_t v, int sl) const {
        const int D = a.D;
#pragma unroll
        for (int j = 0; j < NJ; ++j) own.a[j] = own.b[j] = 0.0;
        own.bias = 0.0;
        if (MODE == kU2) {
            load_row<NJ>(own.a, G.u.F + (size_t)v * 2 * D, D, sl);
            own.bias = G.u.b[v];
        } else if (MODE == kI2) {
            load_row<NJ>(own.a, G.i.F + (size_t)v * 2 * D, D, sl);
            load_row<NJ>(own.b, G.i.F + (size_t)v * 2 * D + D, D, sl);
            own.bias = G.i.b[v];
        }
    }
    template <int NJ>
    __device__ __forceinline__ void edge(Acc<NJ, NS>& acc, const Own<NJ>& own, uint64_t e, int sl) const {
        const int D = a.D;
        if (MODE == kP1) {
            double y[NJ];
            load_row<NJ>(y, G.i.F + (size_t)G.all_item[e] * 2 * D + D, D, sl);
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc.s[j] += y[j];
            acc.cnt += 1;
        } else if (MODE == kU2) {
            const uint32_t w = G.u.nbr[e];
            const double* row = G.i.F + (size_t)w * 2 * D;
            double v[NJ], y[NJ];
            load_row<NJ>(v, row, D, sl);
            load_row<NJ>(y, row + D, D, sl);
            const float err = edge_err<NJ>(own.a, v, y, a.mean, own.bias, G.i.b[w], G.u.obs[e], a.minval, a.maxval);
            if (err != err) acc.nan += sl == 0;
            const double ed = (double)err;
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc.s[j] = fma(ed, v[j], acc.s[j]);
            acc.x[0] += ed;
            acc.cnt += 1;
        } else {
            const uint32_t w = G.i.nbr[e];
            if (!G.act2[w]) return;   // the user did not run phase 2: no message on this edge
            const double* row = G.u.F + (size_t)w * 2 * D;
            double uu[NJ], ww[NJ];
            load_row<NJ>(uu, row, D, sl);
            load_row<NJ>(ww, row + D, D, sl);
            const float err = edge_err<NJ>(uu, own.a, own.b, a.mean, G.u.b[w], own.bias, G.i.obs[e], a.minval, a.maxval);
            const double ed = (double)err;
            const float c = a.if2s * G.unorm[w];   // float product (svdpp.cpp:307-308)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc.s[j] = fma(ed, uu[j] + ww[j], acc.s[j]);
            acc.x[0] += ed;
            acc.x[1] = fma(ed, (double)c, acc.x[1]);
            acc.cnt += 1;
        }
    }
    // Element d of vertex v's pending values from its sums; the regularisers in closed form.
    __device__ __forceinline__ void finish_elem(uint32_t v, int d, double sum, const double* x, double cnt) const {
        const int D = a.D;
        const size_t at = (size_t)v * 2 * D + d;
        if (MODE == kP1) {
            G.u.dF[at + D] = cnt > 0.0 ? sum * (double)G.unorm[v] : G.u.F[at + D];
        } else if (MODE == kU2) {
            G.u.dF[at] = (double)a.ufs * (sum - (double)a.ufr * G.u.F[at] * x[0]);
        } else {
            const double own_v = G.i.F[at], own_y = G.i.F[at + D];
            const float mult = a.if2s * a.if2r;   // float product, then double (svdpp.cpp:310)
            G.i.dF[at] = (double)a.ifs * (sum - cnt * (double)a.ifr * own_v);
            G.i.dF[at + D] = own_v * x[1] - cnt * (double)mult * own_y;
        }
    }
    // counters[1]: messages (edges the item reduction accepted)
    __device__ __forceinline__ void finish_scalar(uint32_t v, const double* x, double cnt,
                                                  unsigned long long* counters) const {
        if (MODE == kU2) G.u.db[v] = (double)a.ubs * x[0];
        if (MODE == kI2) {
            G.i.db[v] = (double)a.ibs * x[0];
            if (cnt > 0.0) atomicAdd(&counters[1], (unsigned long long)cnt);
        }
    }
    template <int NJ>
    __device__ __forceinline__ void finish_elem_own(const Own<NJ>&, int, uint32_t v, int d, double sum, const double* x,
                                                    double cnt) const {
        finish_elem(v, d, sum, x, cnt);
    }
    template <int NJ>
    __device__ __forceinline__ void finish_scalar_own(const Own<NJ>&, uint32_t v, const double* x, double cnt,
                                                      unsigned long long* counters) const {
        finish_scalar(v, x, cnt, counters);
    }
};

// The flags of one side split by the vertex's own phase.  Users: f1 = phase 1, f2 = phase 2.
// Items: f1 = every signalled item (it counts an update and signals its users), f2 = those in
// phase 2 with updates left (svdpp.cpp:321: only they are sent a message).
template <bool ITEM>
__global__ __launch_bounds__(kAT) void svdpp_split_kernel(uint32_t n, uint8_t* flag, const uint32_t* __restrict__ nupd,
                                                         uint8_t* f1, uint8_t* f2, uint64_t max_updates) {
    const uint32_t v = blockIdx.x * (uint32_t)kAT + threadIdx.x;
    if (v >= n) return;
    const bool on = flag[v] != 0;
    const bool odd = (nupd[v] & 1u) != 0;
    flag[v] = 0;
    if (ITEM) {
        f1[v] = on;
        f2[v] = on && odd && (uint64_t)nupd[v] < max_updates;
    } else {
        f1[v] = on && !odd;
        f2[v] = on && odd;
    }
}

// apply, users: phase 1 stores the new W, phase 2 adds dU and dbu; either counts an update.
__global__ __launch_bounds__(kAT) void svdpp_commit_user_kernel(PpGraph G, int D) {
    const uint64_t idx = (uint64_t)blockIdx.x * kAT + threadIdx.x;
    if (idx >= (uint64_t)G.u.n * D) return;
    const uint32_t v = (uint32_t)(idx / D);
    const int d = (int)(idx % D);
    const bool p1 = G.act1[v], p2 = G.act2[v];
    if (!p1 && !p2) return;
    const size_t at = (size_t)v * 2 * D + d;
    if (p1) G.u.F[at + D] = G.u.dF[at + D];
    else G.u.F[at] += G.u.dF[at];
    if (d == 0) {
        if (p2) G.u.b[v] += G.u.db[v];
        G.u.nupd[v] += 1;
    }
}

// apply, items: a phase-2 item with a reduction adds it; every signalled item counts an update.
__global__ __launch_bounds__(kAT) void svdpp_commit_item_kernel(PpGraph G, int D) {
    const uint64_t idx = (uint64_t)blockIdx.x * kAT + threadIdx.x;
    if (idx >= (uint64_t)G.i.n * D) return;
    const uint32_t v = (uint32_t)(idx / D);
    const int d = (int)(idx % D);
    if (!G.i.active[v]) return;
    const size_t at = (size_t)v * 2 * D + d;
    if (G.iact2[v]) {
        G.i.F[at] += G.i.dF[at];
        G.i.F[at + D] += G.i.dF[at + D];
        if (d == 0) G.i.b[v] += G.i.db[v];
    }
    if (d == 0) G.i.nupd[v] += 1;
}

// The first D of every 2 D-long row (U or V alone) for the error reduction of the trace.
__global__ __launch_bounds__(kAT) void svdpp_front_kernel(const double* __restrict__ F, uint64_t total, int D, double* out) {
    const uint64_t idx = (uint64_t)blockIdx.x * kAT + threadIdx.x;
    if (idx >= total) return;
    out[idx] = F[(idx / D) * 2 * D + idx % D];
}

// ---- host ---------------------------------------------------------------------------------

struct PpLayout {
    PpGraph G;
    PpView view[4];      // users phase 1, users phase 2, items all, items reduced
    AlsLists lists[4];
    uint8_t* iflag2;     // the flag arrays of the views (the master flags are G.u.flag / G.i.flag)
    uint8_t* uflag1;
    uint8_t* uflag2;
    uint8_t* iflag_all;
    double* ws;
    unsigned long long* counters;
    MfVal val;
    double* Uf;          // n_users x D and n_items x D fronts for the trace
    double* Vf;
    double* partial;
    double* sums;
    uint32_t seg_cap;
};

void carve_svdpp(Carver& c, PpLayout& f, uint32_t n_users, uint32_t n_items, uint64_t nnz, uint64_t n_all, int D,
                 uint64_t seg_cap, uint64_t n_val, bool trace) {
    const uint32_t n[2] = {n_users, n_items};
    PpSide* side[2] = {&f.G.u, &f.G.i};
    for (int k = 0; k < 2; ++k) {
        PpSide& s = *side[k];
        carve_side(c, s, n[k], nnz);
        s.F = c.take<double>((size_t)n[k] * 2 * D);
        s.dF = c.take<double>((size_t)n[k] * 2 * D);
        s.b = c.take<double>(n[k]);
        s.db = c.take<double>(n[k]);
    }
    f.G.all_off = c.take<uint64_t>((size_t)n_users + 1);
    f.G.all_item = c.take<uint32_t>(n_all);
    f.G.all_src = c.take<uint32_t>(n_all);
    f.G.unorm = c.take<float>(n_users);
    f.G.act1 = c.take<uint8_t>(n_users);
    f.G.act2 = c.take<uint8_t>(n_users);
    f.G.iact2 = c.take<uint8_t>(n_items);
    f.uflag1 = c.take<uint8_t>(n_users);
    f.uflag2 = c.take<uint8_t>(n_users);
    f.iflag_all = c.take<uint8_t>(n_items);
    f.iflag2 = c.take<uint8_t>(n_items);
    f.view[0] = PpView{n_users, f.G.all_off, f.uflag1, f.G.act1};
    f.view[1] = PpView{n_users, f.G.u.off, f.uflag2, f.G.act2};
    f.view[2] = PpView{n_items, f.G.i.off, f.iflag_all, f.G.i.active};
    f.view[3] = PpView{n_items, f.G.i.off, f.iflag2, f.G.iact2};
    for (int q = 0; q < 4; ++q) carve_lists(c, f.lists[q], q < 2 ? n_users : n_items, seg_cap);
    f.ws = c.take<double>((size_t)seg_cap * (D + 3));   // D sums, sum err, sum err c, the count
    f.counters = c.take<unsigned long long>(2);
    carve_val(c, f.val, n_val);
    f.Uf = c.take<double>(trace ? (size_t)n_users * D : 0);
    f.Vf = c.take<double>(trace ? (size_t)n_items * D : 0);
    f.partial = c.take<double>(trace ? error_blocks(std::max(nnz, n_val)) : 0);
    f.sums = c.take<double>(2);
    f.seg_cap = (uint32_t)seg_cap;
}

template <int MODE>
void launch_reduce(const PpLayout& f, const PpArgs& a, const uint32_t rec[4], hipStream_t st) {
    launch_reduce(PpOp<MODE>{f.G, a}, f.lists[MODE == kP1 ? 0 : (MODE == kU2 ? 1 : 3)], rec, f.ws, f.counters, st);
}

// the master flags of one side -> its two views' flags -> their class lists
void launch_split_compact(const PpLayout& f, bool item, uint64_t max_updates, hipStream_t st) {
    const PpSide& s = item ? f.G.i : f.G.u;
    const int q = item ? 2 : 0;
    if (s.n) {
        if (item)
            hipLaunchKernelGGL(svdpp_split_kernel<true>, dim3(blocks_for(s.n)), dim3(kAT), 0, st, s.n, s.flag,
                               (const uint32_t*)s.nupd, f.view[q].flag, f.view[q + 1].flag, max_updates);
        else
            hipLaunchKernelGGL(svdpp_split_kernel<false>, dim3(blocks_for(s.n)), dim3(kAT), 0, st, s.n, s.flag,
                               (const uint32_t*)s.nupd, f.view[q].flag, f.view[q + 1].flag, max_updates);
    }
    launch_compact(f.view[q], f.lists[q], st);
    launch_compact(f.view[q + 1], f.lists[q + 1], st);
}

uint64_t sum3(const uint32_t rec[4]) { return (uint64_t)rec[0] + rec[1] + rec[2]; }

}  // namespace

extern "C" int cf_svdpp_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                            const uint32_t* user_item, const float* user_obs, const uint64_t* item_off,
                            const uint32_t* item_user, const float* item_obs, const uint64_t* imp_off,
                            const uint32_t* imp_item, const cf_svdpp_params* params, double* U, double* V, double* W,
                            double* Y, double* bias_user, double* bias_item, uint32_t* nupdates_user,
                            uint32_t* nupdates_item, const uint8_t* activate_user, uint64_t n_validate,
                            const uint32_t* val_user, const uint32_t* val_item, const float* val_obs, double* trace,
                            uint32_t trace_rows, cf_svdpp_stats* stats) {
    if (!ctx) return CF_EINVAL;
    if (stats) *stats = cf_svdpp_stats{};
    if (!params) return cf_set_error(ctx, CF_EINVAL, "cf_svdpp_fit: null params");
    PpArgs a{params->user_bias_step,  params->item_bias_step,  params->user_factor_step, params->item_factor_step,
             params->item_factor2_step, params->user_factor_reg, params->item_factor_reg, params->item_factor2_reg,
             params->minval,          params->maxval,          params->global_mean,      (int)D};
    auto put_steps = [&]() {
        if (!stats) return;
        stats->user_bias_step = a.ubs;
        stats->item_bias_step = a.ibs;
        stats->user_factor_step = a.ufs;
        stats->item_factor_step = a.ifs;
        stats->item_factor2_step = a.if2s;
    };
    put_steps();
    uint64_t nnz = 0;
    CF_TRY(check_two_csr(ctx, "cf_svdpp_fit", n_users, n_items, D, user_off, user_item, user_obs, item_off, item_user,
                         item_obs, &nnz));
    CF_TRY(check_caps(ctx, "cf_svdpp_fit", params->max_updates, params->max_supersteps));
    if ((n_users && (!U || !W || !bias_user || !nupdates_user)) || (n_items && (!V || !Y || !bias_item || !nupdates_item)))
        return cf_set_error(ctx, CF_EINVAL, "cf_svdpp_fit: null argument");
    uint64_t n_imp = 0;
    if (imp_off && n_users) {
        n_imp = imp_off[n_users];
        if (n_imp && !imp_item) return cf_set_error(ctx, CF_EINVAL, "cf_svdpp_fit: null implicit item array");
        CF_TRY(check_csr(ctx, "cf_svdpp_fit", "implicit", n_users, imp_off, imp_item, n_items));
    }
    const bool want_trace = trace != nullptr && trace_rows > 0;
    const uint64_t n_val = want_trace ? n_validate : 0;
    CF_TRY(check_validation(ctx, "cf_svdpp_fit", n_val, val_user, val_item, val_obs, n_users, n_items));
    if (n_users == 0) return CF_OK;   // nothing can be active
    CF_TRY(set_device(ctx));
    const uint64_t n_all = nnz + n_imp;
    if ((n_all + kAT - 1) / kAT > 0x7fffffffull || error_blocks(std::max(nnz, n_val)) > 0x7fffffffull ||
        (uint64_t)std::max(n_users, n_items) * D > 0x7fffffffull * (uint64_t)kAT)
        return cf_set_error(ctx, CF_ERANGE, "cf_svdpp_fit: too many edges");

    // the all-role list of every user: its TRAIN items, then its implicit items
    std::vector<uint64_t> all_off((size_t)n_users + 1, 0);
    std::vector<uint32_t> all_item(n_all), all_src(n_all);
    std::vector<float> unorm(n_users, 0.0f);
    for (uint32_t u = 0; u < n_users; ++u) {
        uint64_t at = all_off[u];
        for (uint64_t e = user_off[u]; e < user_off[u + 1]; ++e) all_item[at++] = user_item[e];
        if (n_imp)
            for (uint64_t e = imp_off[u]; e < imp_off[u + 1]; ++e) all_item[at++] = imp_item[e];
        for (uint64_t e = all_off[u]; e < at; ++e) all_src[e] = u;
        all_off[u + 1] = at;
        const uint64_t deg = at - all_off[u];
        if (deg) unorm[u] = (float)(1.0 / std::sqrt((double)deg));   // svdpp.cpp:307,358
    }

    // everything the fit needs exists before its first launch
    const uint64_t seg_cap = std::max({total_segments(n_users, user_off), total_segments(n_users, all_off.data()),
                                       n_items ? total_segments(n_items, item_off) : (uint64_t)0});
    if (seg_cap > 0xffffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_svdpp_fit: too many segments");
    PpLayout f{};
    CF_TRY(carve_workspace(
        ctx, [&](Carver& c) { carve_svdpp(c, f, n_users, n_items, nnz, n_all, (int)D, seg_cap, n_val, want_trace); }));
    MfEvents<9> evs;
    for (hipEvent_t& e : evs.e) CF_HIP_CHECK(ctx, hipEventCreate(&e));
    hipStream_t st = nullptr;
    PpGraph& G = f.G;

    const uint32_t n[2] = {n_users, n_items};
    const uint64_t* h_off[2] = {user_off, item_off};
    const uint32_t* h_nbr[2] = {user_item, item_user};
    const float* h_obs[2] = {user_obs, item_obs};
    double* h_A[2] = {U, V};
    double* h_B[2] = {W, Y};
    double* h_b[2] = {bias_user, bias_item};
    uint32_t* h_nupd[2] = {nupdates_user, nupdates_item};
    PpSide* side[2] = {&G.u, &G.i};
    std::vector<double> rows;
    for (int k = 0; k < 2; ++k) {
        if (n[k] == 0) continue;
        const PpSide& s = *side[k];
        CF_TRY(upload_side(ctx, s, nnz, h_off[k], h_nbr[k], h_obs[k], h_nupd[k], k == 0 ? activate_user : nullptr, k == 0));
        rows.resize((size_t)n[k] * 2 * D);   // interleave [A | B]
        for (uint32_t v = 0; v < n[k]; ++v)
            for (uint32_t d = 0; d < D; ++d) {
                rows[(size_t)v * 2 * D + d] = h_A[k][(size_t)v * D + d];
                rows[(size_t)v * 2 * D + D + d] = h_B[k][(size_t)v * D + d];
            }
        CF_HIP_CHECK(ctx, hipMemcpy(s.F, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemset(s.dF, 0, sizeof(double) * rows.size()));
        CF_HIP_CHECK(ctx, hipMemcpy(s.b, h_b[k], sizeof(double) * n[k], hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemset(s.db, 0, sizeof(double) * n[k]));
    }
    CF_HIP_CHECK(ctx, hipMemcpy((void*)G.all_off, all_off.data(), sizeof(uint64_t) * all_off.size(), hipMemcpyHostToDevice));
    if (n_all) {
        CF_HIP_CHECK(ctx, hipMemcpy((void*)G.all_item, all_item.data(), sizeof(uint32_t) * n_all, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy((void*)G.all_src, all_src.data(), sizeof(uint32_t) * n_all, hipMemcpyHostToDevice));
    }
    CF_HIP_CHECK(ctx, hipMemcpy((void*)G.unorm, unorm.data(), sizeof(float) * n_users, hipMemcpyHostToDevice));
    CF_HIP_CHECK(ctx, hipMemset(G.act1, 0, n_users));
    CF_HIP_CHECK(ctx, hipMemset(G.act2, 0, n_users));
    if (n_items) CF_HIP_CHECK(ctx, hipMemset(G.iact2, 0, n_items));
    CF_TRY(upload_val(ctx, f.val, n_val, val_user, val_item, val_obs));
    CF_HIP_CHECK(ctx, hipMemset(f.counters, 0, 2 * sizeof(unsigned long long)));

    const uint64_t max_updates = params->max_updates;
    const uint32_t max_supersteps = params->max_supersteps;
    uint32_t supersteps = 0;
    uint64_t updates = 0;
    unsigned long long counters[2] = {0, 0};
    double reduce_ms[3] = {0.0, 0.0, 0.0}, apply_ms = 0.0;
    bool item_step_pending = false;   // events 7, 8 recorded and not read yet
    launch_split_compact(f, false, max_updates, st);
    for (;;) {
        uint32_t rec_u1[4], rec_u2[4], rec_ia[4] = {0, 0, 0, 0}, rec_i2[4] = {0, 0, 0, 0};
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(rec_u1, f.lists[0].record, sizeof(rec_u1), hipMemcpyDeviceToHost));   // waits for the stream
        CF_HIP_CHECK(ctx, hipMemcpy(rec_u2, f.lists[1].record, sizeof(rec_u2), hipMemcpyDeviceToHost));
        if (item_step_pending) apply_ms += elapsed(evs.e[7], evs.e[8]);
        item_step_pending = false;
        const uint64_t n_active = sum3(rec_u1) + sum3(rec_u2);
        if (n_active == 0) break;                                   // the run ends when nobody is signalled
        if (max_supersteps && supersteps >= max_supersteps) break;
        if (rec_u1[3] > f.seg_cap || rec_u2[3] > f.seg_cap)
            return cf_set_error(ctx, CF_EHIP, "cf_svdpp_fit: segment list overflow");

        // ---- user superstep: both phases' reductions, signals, the items' messages, apply ----
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
        launch_reduce<kP1>(f, a, rec_u1, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
        launch_reduce<kU2>(f, a, rec_u2, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[2], st));
        if (n_items) {
            if (nnz && sum3(rec_u2))   // the scatter of the phase-2 users (a phase-1 user's is contained in the next)
                hipLaunchKernelGGL(mf_signal_kernel, dim3(blocks_for(nnz)), dim3(kAT), 0, st, G.u.src, G.u.nbr, nnz,
                                   (const uint8_t*)G.act2, (const uint32_t*)G.i.nupd, G.i.flag, max_updates, true);
            if (n_all && sum3(rec_u1))
                hipLaunchKernelGGL(mf_signal_kernel, dim3(blocks_for(n_all)), dim3(kAT), 0, st, G.all_src, G.all_item,
                                   n_all, (const uint8_t*)G.act1, (const uint32_t*)G.i.nupd, G.i.flag, max_updates, false);
        }
        launch_split_compact(f, true, max_updates, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[3], st));
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(rec_ia, f.lists[2].record, sizeof(rec_ia), hipMemcpyDeviceToHost));
        CF_HIP_CHECK(ctx, hipMemcpy(rec_i2, f.lists[3].record, sizeof(rec_i2), hipMemcpyDeviceToHost));
        if (rec_ia[3] > f.seg_cap) return cf_set_error(ctx, CF_EHIP, "cf_svdpp_fit: segment list overflow");
        const uint64_t n_signalled = sum3(rec_ia);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[4], st));
        if (sum3(rec_i2)) launch_reduce<kI2>(f, a, rec_i2, st);     // from the values of the superstep's start
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[5], st));
        hipLaunchKernelGGL(svdpp_commit_user_kernel, dim3(blocks_for((uint64_t)n_users * D)), dim3(kAT), 0, st, G, (int)D);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[6], st));
        const double dec = params->step_dec;                        // svdpp.cpp:454-458: after every user superstep
        a.ubs = (float)((double)a.ubs * dec);
        a.ibs = (float)((double)a.ibs * dec);
        a.ufs = (float)((double)a.ufs * dec);
        a.ifs = (float)((double)a.ifs * dec);
        a.if2s = (float)((double)a.if2s * dec);
        const uint32_t row = supersteps / 2;
        const bool trace_row = want_trace && row < trace_rows;
        if (trace_row) {   // new U, old V, no Y (svdpp.cpp:466-476)
            CF_HIP_CHECK(ctx, hipMemsetAsync(f.sums, 0, 2 * sizeof(double), st));
            const uint64_t tu = (uint64_t)n_users * D, ti = (uint64_t)n_items * D;
            hipLaunchKernelGGL(svdpp_front_kernel, dim3(blocks_for(tu)), dim3(kAT), 0, st, (const double*)G.u.F, tu, (int)D, f.Uf);
            if (ti)
                hipLaunchKernelGGL(svdpp_front_kernel, dim3(blocks_for(ti)), dim3(kAT), 0, st, (const double*)G.i.F, ti, (int)D, f.Vf);
            if (nnz)
                launch_error(st, nnz, G.u.src, G.u.nbr, G.u.obs, f.Uf, f.Vf, (int)D, G.u.b, G.i.b, a.mean, a.minval,
                             a.maxval, f.partial, f.sums);
            if (n_val)
                launch_error(st, n_val, f.val.user, f.val.item, f.val.obs, f.Uf, f.Vf, (int)D, G.u.b, G.i.b, a.mean, a.minval,
                             a.maxval, f.partial, f.sums + 1);
        }
        ++supersteps;
        updates += n_active;
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(counters, f.counters, sizeof(counters), hipMemcpyDeviceToHost));   // waits
        if (trace_row) CF_HIP_CHECK(ctx, hipMemcpy(trace + 2 * (size_t)row, f.sums, 2 * sizeof(double), hipMemcpyDeviceToHost));
        reduce_ms[0] += elapsed(evs.e[0], evs.e[1]);
        reduce_ms[1] += elapsed(evs.e[1], evs.e[2]);
        reduce_ms[2] += elapsed(evs.e[4], evs.e[5]);
        apply_ms += elapsed(evs.e[2], evs.e[3]) + elapsed(evs.e[5], evs.e[6]);
        if (counters[0]) break;                                     // numeric errors: the caller reports them
        if (n_signalled == 0) break;
        if (max_supersteps && supersteps >= max_supersteps) break;  // the pending messages are dropped

        // ---- item superstep: phase-2 items add their messages; every signalled item signals its users ----
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[7], st));
        hipLaunchKernelGGL(svdpp_commit_item_kernel, dim3(blocks_for((uint64_t)n_items * D)), dim3(kAT), 0, st, G, (int)D);
        if (nnz)
            hipLaunchKernelGGL(mf_signal_kernel, dim3(blocks_for(nnz)), dim3(kAT), 0, st, G.i.src, G.i.nbr, nnz,
                               (const uint8_t*)G.i.active, (const uint32_t*)G.u.nupd, G.u.flag, max_updates, true);
        launch_split_compact(f, false, max_updates, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[8], st));
        item_step_pending = true;
        ++supersteps;
        updates += n_signalled;
    }
    CF_HIP_CHECK(ctx, hipDeviceSynchronize());
    for (int k = 0; k < 2; ++k) {
        if (n[k] == 0) continue;
        const PpSide& s = *side[k];
        rows.resize((size_t)n[k] * 2 * D);
        CF_HIP_CHECK(ctx, hipMemcpy(rows.data(), s.F, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
        for (uint32_t v = 0; v < n[k]; ++v)
            for (uint32_t d = 0; d < D; ++d) {
                h_A[k][(size_t)v * D + d] = rows[(size_t)v * 2 * D + d];
                h_B[k][(size_t)v * D + d] = rows[(size_t)v * 2 * D + D + d];
            }
        CF_HIP_CHECK(ctx, hipMemcpy(h_b[k], s.b, sizeof(double) * n[k], hipMemcpyDeviceToHost));
        CF_HIP_CHECK(ctx, hipMemcpy(h_nupd[k], s.nupd, sizeof(uint32_t) * n[k], hipMemcpyDeviceToHost));
    }
    for (int q = 0; q < 3; ++q) ctx->svdpp_reduce_ms[q] = (float)reduce_ms[q];
    if (stats) {
        stats->supersteps = supersteps;
        stats->updates = updates;
        stats->messages = counters[1];
        stats->n_nan = counters[0];
        put_steps();
        stats->reduce_ms = (float)(reduce_ms[0] + reduce_ms[1] + reduce_ms[2]);
        stats->apply_ms = (float)apply_ms;
    }
    return CF_OK;
}

extern "C" int cf_svdpp_timing(cf_ctx* ctx, float* phase1_reduce_ms, float* user_reduce_ms, float* item_reduce_ms) {
    if (!ctx) return CF_EINVAL;
    if (phase1_reduce_ms) *phase1_reduce_ms = ctx->svdpp_reduce_ms[0];
    if (user_reduce_ms) *user_reduce_ms = ctx->svdpp_reduce_ms[1];
    if (item_reduce_ms) *item_reduce_ms = ctx->svdpp_reduce_ms[2];
    return CF_OK;
}

extern "C" int cf_svdpp_predict(cf_ctx* ctx, uint64_t n_pairs, const uint32_t* user, const uint32_t* item,
                                uint32_t n_users, uint32_t n_items, uint32_t D, const double* U, const double* V,
                                const double* Y, const double* bias_user, const double* bias_item, double global_mean,
                                double minval, double maxval, double* pred) {
    if (!ctx) return CF_EINVAL;
    CF_TRY(check_pairs(ctx, "cf_svdpp_predict", n_pairs, user, item, U, V, D, n_users, n_items));
    if (n_pairs && (!Y || !bias_user || !bias_item || !pred))
        return cf_set_error(ctx, CF_EINVAL, "cf_svdpp_predict: null argument");
    if (n_pairs == 0) return CF_OK;
    CF_TRY(set_device(ctx));
    const uint64_t blocks = (n_pairs * kG + kAT - 1) / kAT;
    if (blocks > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_svdpp_predict: too many pairs");
    // the row V_i + Y_i is formed once per item while the factors are staged for the upload, so the
    // pair kernel is the bias-SGD one: fma(U_u[d], V_i[d] + Y_i[d], s) in the same order
    std::vector<double> VY((size_t)n_items * D);
    for (size_t k = 0; k < VY.size(); ++k) VY[k] = V[k] + Y[k];
    PairLayout p{};
    CF_TRY(upload_pairs(ctx, p, n_pairs, user, item, nullptr, n_users, n_items, D, U, VY.data(), n_pairs, bias_user,
                        bias_item));
    hipLaunchKernelGGL(mf_predict_kernel, dim3((unsigned)blocks), dim3(kAT), 0, nullptr, n_pairs, (const uint32_t*)p.user,
                       (const uint32_t*)p.item, (const double*)p.U, (const double*)p.V, (int)D, (const double*)p.bu,
                       (const double*)p.bi, global_mean, 1, minval, maxval, p.out);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(pred, p.out, sizeof(double) * n_pairs, hipMemcpyDeviceToHost));
    return CF_OK;
}
