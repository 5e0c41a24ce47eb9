// cf_ials.hip -- implicit-feedback ALS (Hu, Koren, Volinsky, ICDM 2008) on gfx950, fp64 throughout.
//
// Every pair of the n_users x n_items grid is a training example: an observed edge carries a
// confidence c >= 1 and a preference p, every other pair is p = 0 with c = 1, and
//   L(U, V) = sum_{u,i} c_ui (p_ui - U_u.V_i)^2 + sum_u reg_user[u] |U_u|^2 + sum_i reg_item[i] |V_i|^2.
// A half-sweep sets every vertex of one side to its exact minimiser: with x_j the other side's
// rows and G = sum over ALL of them of x x^T (the global Gram, once per half-sweep), vertex v solves
//   (G + sum_{edges} (c - 1) x x^T + reg[v] I) f = sum_{edges} (c p) x.
// A sweep is the user half-sweep, then the item half-sweep; every vertex is active in each, so the
// class lists of both sides are compacted once per fit.
//
// Global Gram of an n x D row-major matrix: one workgroup per slice of kGramRows rows; wave w
// takes rows [w kGramRows / 4, (w + 1) kGramRows / 4) of the slice in the Gram<DP> register block
// of cf_als_gram.h (rows staged kBatch at a time by flat, coalesced loads), the four partials are
// summed in wave order in LDS and the slice's D x D partial goes to the workspace; a second kernel
// sums the partials in slice order.  Element (i, q) and element (q, i) run the same fma chain
// (fma(a, b, c) = fma(b, a, c)), so G is symmetric bit for bit; the same F gives the same bits in
// every run, and a slice's partial depends on its own rows only.  Reads n 8 D bytes once and does
// n D^2 fma.
//
// Per-vertex update, in the three degree classes of cf_als_update.h (shared with cf_als.hip; this
// file gives its kernels the policy IalsOp).  ORDER OF THE SYSTEM, the same in all three classes:
//   1. the edge sums start from zero: A_e = sum (c - 1) x x^T, b = sum (c p) x, each element one
//      fma chain in CSR order within a wave's edge range (gram_accumulate<DP, true>); the ranges
//      are summed in wave order, then (high) in segment order
//   2. S = A_e + G, the packed lower triangle of G added once by the wave that solves
//   3. S_ii += reg[v], in wave_ldlt_solve
//   4. the unpivoted LDL^T and the back substitution
// G and reg are never added per wave or per segment.  A vertex without edges has b = 0: its factor
// is written as +0.0 without a solve.
// Determinism rule (ALS's, extended): a vertex's new factor depends only on its own edge list, the
// other side's rows and the bits of G; no floating-point atomic anywhere.
//
// Loss without the unobserved pairs:
//   L = <G_U, G_V>_F + sum_obs [c (p - s)^2 - s^2] + sum reg |row|^2,  s = U_u.V_i,
// each term a fixed two-level reduction (the pattern of mf_error_kernel / als_error_final_kernel),
// combined as ((frob + obs) + reg_user) + reg_item.
//
// Layout in HBM: as cf_als.hip, with two f32 per edge (confidence, preference): a half-sweep reads
// about nnz (8 D + 12) + n 8 D bytes.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cf_als_update.h"
#include "cf_internal.h"
#include "cf_mf_common.h"

namespace {

constexpr int kGramRows = 512;   // rows per slice of the global Gram

struct IalsSide {
    uint32_t n;
    const uint64_t* off;
    const uint32_t* nbr;
    const float* conf;
    const float* pref;
    double* F;             // n x D factors
    const double* reg;
    uint8_t* flag;         // all ones until the one compaction of the fit
    uint8_t* active;
};

// ---- global Gram ---------------------------------------------------------------------------

template <int DP>
constexpr int gram_region() {
    return kWaves * kBatch * DP > DP * DP ? kWaves * kBatch * DP : DP * DP;
}

template <int DP>
__global__ __launch_bounds__(kAT) void ials_gram_slice_kernel(const double* __restrict__ F, uint32_t n, int D,
                                                             double* __restrict__ partial) {
    constexpr int TS = DP / 8;
    __shared__ __attribute__((aligned(16))) double lds[gram_region<DP>()];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ti = lane >> 3, tj = lane & 7;
    const uint64_t r0 = (uint64_t)blockIdx.x * kGramRows;
    const int len = (int)std::min<uint64_t>((uint64_t)kGramRows, (uint64_t)n - r0);
    constexpr int chunk = kGramRows / kWaves;
    const int b = std::min(len, wave * chunk), e = std::min(len, (wave + 1) * chunk);
    double* stage = lds + wave * kBatch * DP;
    for (int t = lane; t < kBatch * DP; t += 64) stage[t] = 0.0;   // the padding columns stay zero
    WAVE_SYNC();
    Gram<DP> g;
    g.clear();
    for (int r = b; r < e; r += kBatch) {
        const int nb = std::min(kBatch, e - r);
        const double* __restrict__ src = F + (r0 + (uint64_t)r) * D;   // nb rows = nb D contiguous doubles
        for (int t = lane; t < nb * D; t += 64) stage[(t / D) * DP + t % D] = src[t];
        WAVE_SYNC();
        for (int k = 0; k < nb; ++k) {
            double xi[TS], xj[TS];
#pragma unroll
            for (int x = 0; x < TS; ++x) {
                xi[x] = stage[k * DP + ti * TS + x];
                xj[x] = stage[k * DP + tj * TS + x];
            }
#pragma unroll
            for (int x = 0; x < TS; ++x)
#pragma unroll
                for (int y = 0; y < TS; ++y) g.a[x][y] = fma(xi[x], xj[y], g.a[x][y]);
        }
        WAVE_SYNC();
    }
    __syncthreads();   // the staging rows are dead: the D x D sum takes their place
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {   // partials summed in wave order
        if (wave == w) {
#pragma unroll
            for (int x = 0; x < TS; ++x)
#pragma unroll
                for (int y = 0; y < TS; ++y) {
                    const int i = ti * TS + x, q = tj * TS + y;
                    if (i < D && q < D) lds[i * D + q] = w ? lds[i * D + q] + g.a[x][y] : g.a[x][y];
                }
        }
        __syncthreads();
    }
    double* slot = partial + (size_t)blockIdx.x * D * D;
    for (int t = threadIdx.x; t < D * D; t += kAT) slot[t] = lds[t];
}

// G = the partials summed in slice order; Gp = its packed lower triangle (what the solves add).
__global__ __launch_bounds__(kAT) void ials_gram_sum_kernel(const double* __restrict__ partial, uint32_t n_slices, int D,
                                                           double* __restrict__ G, double* __restrict__ Gp) {
    const int t = blockIdx.x * kAT + threadIdx.x;
    if (t >= D * D) return;
    // The adds are one chain in slice order; the loads of kAhead slices are issued together, or
    // the chain would wait for one HBM round trip per slice.
    constexpr uint32_t kAhead = 32;
    const size_t DD = (size_t)D * D;
    double acc = 0.0;
    uint32_t s = 0;
    for (; s + kAhead <= n_slices; s += kAhead) {
        double v[kAhead];
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) v[j] = partial[(size_t)(s + j) * DD + t];
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) acc += v[j];
    }
    for (; s < n_slices; ++s) acc += partial[(size_t)s * DD + t];
    G[t] = acc;
    const int i = t / D, q = t % D;
    if (Gp && q <= i) Gp[tri(i, q)] = acc;
}

// ---- per-vertex update -----------------------------------------------------------------------

// The policy of cf_als_update.h: the weighted edge, and steps 2-4 of the header as the tail.
struct IalsOp {
    static constexpr bool kWeighted = true;
    IalsSide s;
    const double* Gp;   // packed lower triangle of the other side's Gram
    __device__ const float* edge_obs() const { return s.conf; }
    __device__ const float* edge_pref() const { return s.pref; }
    // b = 0: the minimiser is the zero vector
    __device__ void no_edges(uint32_t v, int D, int lane) const {
        for (int d = lane; d < D; d += 64) s.F[(size_t)v * D + d] = 0.0;
    }
    __device__ void apply(double* S, int D, uint32_t v, unsigned long long* not_pd, int lane) const {
        for (int t = lane; t < D * (D + 1) / 2; t += 64) S[t] += Gp[t];
        WAVE_SYNC();
        const int bad = wave_ldlt_solve(S, D, s.reg[v], lane);
        double* Fv = s.F + (size_t)v * D;
        for (int d = lane; d < D; d += 64) Fv[d] = S[tri(D, d)];
        if (lane == 0 && bad) atomicAdd(not_pd, (unsigned long long)bad);   // integer counter
    }
};

// ---- loss --------------------------------------------------------------------------------

// Level 1 of the observed-edge term: block b sums c (p - s)^2 - s^2 over edges [b kErrPerBlock,
// (b + 1) kErrPerBlock) of the user CSR: group g takes edges g, g + 32, .. in order, then a tree.
__global__ __launch_bounds__(kAT) void ials_obs_kernel(uint64_t n, const uint32_t* __restrict__ user,
                                                      const uint32_t* __restrict__ item, const float* __restrict__ conf,
                                                      const float* __restrict__ pref, const double* __restrict__ U,
                                                      const double* __restrict__ V, int D, double* partial) {
    __shared__ double s_v[kAT];
    const int grp = threadIdx.x / kG, sl = threadIdx.x & (kG - 1);
    const uint64_t e0 = (uint64_t)blockIdx.x * kErrPerBlock;
    double acc = 0.0;
    for (int r = 0; r < kErrPerBlock / (kAT / kG); ++r) {
        const uint64_t e = e0 + (uint64_t)r * (kAT / kG) + grp;
        if (e >= n) break;   // per group
        const double s = group_dot(U + (size_t)user[e] * D, V + (size_t)item[e] * D, D, sl);
        const double d = (double)pref[e] - s;
        acc = fma((double)conf[e] * d, d, acc);
        acc = fma(-s, s, acc);
    }
    s_v[threadIdx.x] = sl == 0 ? acc : 0.0;
    block_tree_sum(s_v);
    if (threadIdx.x == 0) partial[blockIdx.x] = s_v[0];
}

// Level 1 of a regularisation term: block b sums reg[r] |F_r|^2 over rows [b kErrPerBlock, ..).
__global__ __launch_bounds__(kAT) void ials_rownorm_kernel(uint32_t n, const double* __restrict__ F,
                                                          const double* __restrict__ reg, int D, double* partial) {
    __shared__ double s_v[kAT];
    const int grp = threadIdx.x / kG, sl = threadIdx.x & (kG - 1);
    const uint64_t r0 = (uint64_t)blockIdx.x * kErrPerBlock;
    double acc = 0.0;
    for (int r = 0; r < kErrPerBlock / (kAT / kG); ++r) {
        const uint64_t v = r0 + (uint64_t)r * (kAT / kG) + grp;
        if (v >= n) break;   // per group
        const double* Fv = F + (size_t)v * D;
        acc = fma(reg[v], group_dot(Fv, Fv, D, sl), acc);
    }
    s_v[threadIdx.x] = sl == 0 ? acc : 0.0;
    block_tree_sum(s_v);
    if (threadIdx.x == 0) partial[blockIdx.x] = s_v[0];
}

// <G_U, G_V>_F: one workgroup; thread t takes elements t, t + kAT, .. in order, then the tree.
__global__ __launch_bounds__(kAT) void ials_frob_kernel(const double* __restrict__ GU, const double* __restrict__ GV,
                                                       int DD, double* out) {
    __shared__ double s_v[kAT];
    double acc = 0.0;
    for (int t = threadIdx.x; t < DD; t += kAT) acc = fma(GU[t], GV[t], acc);
    s_v[threadIdx.x] = acc;
    block_tree_sum(s_v);
    if (threadIdx.x == 0) *out = s_v[0];
}

// four = {frob, obs, reg_user, reg_item}
__global__ void ials_loss_combine_kernel(const double* __restrict__ four, double* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = ((four[0] + four[1]) + four[2]) + four[3];
}

// ---- host ---------------------------------------------------------------------------------

inline uint32_t gram_slices(uint32_t n) { return (uint32_t)(((uint64_t)n + kGramRows - 1) / kGramRows); }

// G (and, where Gp is not NULL, its packed lower triangle) of the n x D device matrix F.
void launch_gram(const double* F, uint32_t n, int D, double* partial, double* G, double* Gp, hipStream_t st) {
    const uint32_t slices = gram_slices(n);
    if (slices)
        dispatch_dp(D, [&](auto dp) {
            hipLaunchKernelGGL(ials_gram_slice_kernel<decltype(dp)::value>, dim3(slices), dim3(kAT), 0, st, F, n, D,
                               partial);
        });
    hipLaunchKernelGGL(ials_gram_sum_kernel, dim3((D * D + kAT - 1) / kAT), dim3(kAT), 0, st, (const double*)partial,
                       slices, D, G, Gp);
}

// The graph and the factors of one call, host side: index 0 users, 1 items.
struct IalsArgs {
    uint32_t n[2];
    uint32_t D;
    const uint64_t* off[2];
    const uint32_t* nbr[2];
    const float* conf[2];
    const float* pref[2];
    const double* reg[2];
    uint64_t nnz;
};

struct IalsLayout {
    IalsSide side[2];
    AlsLists lists[2];
    uint32_t* user_of_edge;   // owner of each edge of the user CSR (the loss runs over it)
    double* ws;               // segment partials
    double* gpart;            // Gram slice partials
    double* G[2];
    double* Gp[2];
    unsigned long long* not_pd;
    double* pe;               // loss partials: observed edges, user rows, item rows
    double* pr[2];
    double* four;
    double* trace;
};

void carve_ials(Carver& c, IalsLayout& f, const IalsArgs& a, const uint64_t segs[2], uint32_t n_trace) {
    const int D = (int)a.D;
    for (int k = 0; k < 2; ++k) {
        IalsSide& s = f.side[k];
        s.n = a.n[k];
        s.off = c.take<uint64_t>((size_t)a.n[k] + 1);
        s.nbr = c.take<uint32_t>(a.nnz);
        s.conf = c.take<float>(a.nnz);
        s.pref = c.take<float>(a.nnz);
        s.F = c.take<double>((size_t)a.n[k] * D);
        s.reg = c.take<double>(a.n[k]);
        s.flag = c.take<uint8_t>(a.n[k]);
        s.active = c.take<uint8_t>(a.n[k]);
        carve_lists(c, f.lists[k], a.n[k], segs[k]);
        f.G[k] = c.take<double>((size_t)D * D);
        f.Gp[k] = c.take<double>((size_t)D * (D + 1) / 2);
        f.pr[k] = c.take<double>(error_blocks(a.n[k]));
    }
    f.user_of_edge = c.take<uint32_t>(a.nnz);
    f.ws = c.take<double>((size_t)std::max(segs[0], segs[1]) * sys_len(D));
    f.gpart = c.take<double>((size_t)gram_slices(std::max(a.n[0], a.n[1])) * D * D);
    f.not_pd = c.take<unsigned long long>(1);
    f.pe = c.take<double>(error_blocks(a.nnz));
    f.four = c.take<double>(4);
    f.trace = c.take<double>(n_trace);
}

// The checks cf_ials_fit and cf_ials_loss share.
int check_ials(cf_ctx* ctx, const char* fn, IalsArgs& a, const double* U, const double* V) {
    const std::string f(fn);
    if (a.D == 0) return cf_set_error(ctx, CF_EINVAL, f + ": D = 0");
    if (a.D > CF_ALS_MAX_D) return cf_set_error(ctx, CF_ERANGE, f + ": D above CF_ALS_MAX_D");
    if ((a.n[0] && (!a.off[0] || !a.reg[0] || !U)) || (a.n[1] && (!a.off[1] || !a.reg[1] || !V)))
        return cf_set_error(ctx, CF_EINVAL, f + ": null argument");
    CF_TRY(check_two_csr(ctx, fn, a.n[0], a.n[1], a.D, a.off[0], a.nbr[0], a.conf[0], a.off[1], a.nbr[1], a.conf[1],
                         &a.nnz));
    if ((a.pref[0] == nullptr) != (a.pref[1] == nullptr))
        return cf_set_error(ctx, CF_EINVAL, f + ": exactly one of the two preference arrays is NULL");
    for (int k = 0; k < 2; ++k)
        for (uint64_t e = 0; e < a.nnz; ++e) {
            if (!(a.conf[k][e] >= 1.0f) || !std::isfinite(a.conf[k][e]))
                return cf_set_error(ctx, CF_EINVAL, f + ": a confidence below 1 or not finite");
            if (a.pref[k] && !std::isfinite(a.pref[k][e]))
                return cf_set_error(ctx, CF_EINVAL, f + ": a preference that is not finite");
        }
    return CF_OK;
}

int upload_ials(cf_ctx* ctx, const IalsLayout& f, const IalsArgs& a, const double* const F[2]) {
    const std::vector<float> ones(a.pref[0] ? 0 : a.nnz, 1.0f);
    for (int k = 0; k < 2; ++k) {
        if (a.n[k] == 0) continue;
        const IalsSide& s = f.side[k];
        const size_t n = a.n[k];
        CF_HIP_CHECK(ctx, hipMemcpy((void*)s.off, a.off[k], sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice));
        if (a.nnz) {
            CF_HIP_CHECK(ctx, hipMemcpy((void*)s.nbr, a.nbr[k], sizeof(uint32_t) * a.nnz, hipMemcpyHostToDevice));
            CF_HIP_CHECK(ctx, hipMemcpy((void*)s.conf, a.conf[k], sizeof(float) * a.nnz, hipMemcpyHostToDevice));
            CF_HIP_CHECK(ctx, hipMemcpy((void*)s.pref, a.pref[k] ? a.pref[k] : ones.data(), sizeof(float) * a.nnz,
                                        hipMemcpyHostToDevice));
        }
        CF_HIP_CHECK(ctx, hipMemcpy(s.F, F[k], sizeof(double) * n * a.D, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy((void*)s.reg, a.reg[k], sizeof(double) * n, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemset(s.flag, 1, n));
        CF_HIP_CHECK(ctx, hipMemset(s.active, 0, n));
    }
    if (a.nnz) CF_TRY(upload_edge_owners(ctx, f.user_of_edge, a.n[0], a.off[0], a.nnz));
    CF_HIP_CHECK(ctx, hipMemset(f.not_pd, 0, sizeof(unsigned long long)));
    return CF_OK;
}

// The loss of the factors on the device, from G[0] and G[1] as they stand, into *out (device).
void launch_loss(const IalsLayout& f, const IalsArgs& a, double* out, hipStream_t st) {
    const int D = (int)a.D;
    hipLaunchKernelGGL(ials_frob_kernel, dim3(1), dim3(kAT), 0, st, (const double*)f.G[0], (const double*)f.G[1], D * D,
                       f.four);
    const uint64_t be = error_blocks(a.nnz);
    if (be)
        hipLaunchKernelGGL(ials_obs_kernel, dim3((unsigned)be), dim3(kAT), 0, st, a.nnz, (const uint32_t*)f.user_of_edge,
                           f.side[0].nbr, f.side[0].conf, f.side[0].pref, (const double*)f.side[0].F,
                           (const double*)f.side[1].F, D, f.pe);
    hipLaunchKernelGGL(als_error_final_kernel, dim3(1), dim3(kAT), 0, st, (const double*)f.pe, be, f.four + 1);
    for (int k = 0; k < 2; ++k) {
        const uint64_t br = error_blocks(a.n[k]);
        if (br)
            hipLaunchKernelGGL(ials_rownorm_kernel, dim3((unsigned)br), dim3(kAT), 0, st, a.n[k],
                               (const double*)f.side[k].F, f.side[k].reg, D, f.pr[k]);
        hipLaunchKernelGGL(als_error_final_kernel, dim3(1), dim3(kAT), 0, st, (const double*)f.pr[k], br, f.four + 2 + k);
    }
    hipLaunchKernelGGL(ials_loss_combine_kernel, dim3(1), dim3(64), 0, st, (const double*)f.four, out);
}

}  // namespace

extern "C" int cf_debug_ials_gram_rows(void) { return kGramRows; }

extern "C" int cf_mf_gram(cf_ctx* ctx, uint32_t n, uint32_t D, const double* F, double* G) {
    if (!ctx) return CF_EINVAL;
    if (D == 0) return cf_set_error(ctx, CF_EINVAL, "cf_mf_gram: D = 0");
    if (D > CF_ALS_MAX_D) return cf_set_error(ctx, CF_ERANGE, "cf_mf_gram: D above CF_ALS_MAX_D");
    if (!G || (n && !F)) return cf_set_error(ctx, CF_EINVAL, "cf_mf_gram: null argument");
    CF_TRY(set_device(ctx));
    double *dF = nullptr, *part = nullptr, *dG = nullptr;
    CF_TRY(carve_workspace(ctx, [&](Carver& c) {
        dF = c.take<double>((size_t)n * D);
        part = c.take<double>((size_t)gram_slices(n) * D * D);
        dG = c.take<double>((size_t)D * D);
    }));
    if (n) CF_HIP_CHECK(ctx, hipMemcpy(dF, F, sizeof(double) * (size_t)n * D, hipMemcpyHostToDevice));
    launch_gram(dF, n, (int)D, part, dG, nullptr, nullptr);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(G, dG, sizeof(double) * (size_t)D * D, hipMemcpyDeviceToHost));
    return CF_OK;
}

extern "C" int cf_ials_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                           const uint32_t* user_item, const float* user_conf, const float* user_pref,
                           const uint64_t* item_off, const uint32_t* item_user, const float* item_conf,
                           const float* item_pref, const double* reg_user, const double* reg_item, uint32_t n_sweeps,
                           double* U, double* V, double* loss_trace, cf_ials_stats* stats) {
    if (!ctx) return CF_EINVAL;
    if (stats) *stats = cf_ials_stats{};
    IalsArgs a{{n_users, n_items}, D, {user_off, item_off}, {user_item, item_user}, {user_conf, item_conf},
               {user_pref, item_pref}, {reg_user, reg_item}, 0};
    CF_TRY(check_ials(ctx, "cf_ials_fit", a, U, V));
    if (n_sweeps == 0 || (n_users == 0 && n_items == 0)) return CF_OK;   // no half-sweep runs: U, V untouched
    if (n_sweeps > (1u << 24)) return cf_set_error(ctx, CF_ERANGE, "cf_ials_fit: more than 2^24 sweeps");
    CF_TRY(set_device(ctx));

    // everything the fit needs exists before its first launch
    const uint64_t segs[2] = {total_segments(n_users, user_off), n_items ? total_segments(n_items, item_off) : 0};
    if (std::max(segs[0], segs[1]) > 0xffffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_ials_fit: too many segments");
    if (error_blocks(a.nnz) > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_ials_fit: too many edges");
    IalsLayout f{};
    CF_TRY(carve_workspace(ctx, [&](Carver& c) { carve_ials(c, f, a, segs, 2 * n_sweeps); }));
    MfEvents<4> evs;
    for (hipEvent_t& e : evs.e) CF_HIP_CHECK(ctx, hipEventCreate(&e));
    hipStream_t st = nullptr;
    const double* h_in[2] = {U, V};
    double* h_F[2] = {U, V};
    CF_TRY(upload_ials(ctx, f, a, h_in));

    // every vertex is active in every half-sweep: one compaction per side
    uint32_t rec[2][4];
    for (int k = 0; k < 2; ++k) {
        launch_compact(f.side[k], f.lists[k], st);
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(rec[k], f.lists[k].record, sizeof(rec[k]), hipMemcpyDeviceToHost));
        if (rec[k][3] > segs[k]) return cf_set_error(ctx, CF_EHIP, "cf_ials_fit: segment list overflow");
    }
    const int Di = (int)D;
    double gram_ms = 0.0, update_ms = 0.0, loss_ms = 0.0;
    CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
    launch_gram(f.side[1].F, n_items, Di, f.gpart, f.G[1], f.Gp[1], st);
    CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
    CF_HIP_CHECK(ctx, hipEventSynchronize(evs.e[1]));
    gram_ms += elapsed(evs.e[0], evs.e[1]);
    for (uint32_t h = 0; h < 2 * n_sweeps; ++h) {
        const int k = (int)(h & 1);   // users, then items
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
        launch_update(IalsOp{f.side[k], f.Gp[1 - k]}, f.side[1 - k].F, Di, f.lists[k], rec[k], f.ws, f.not_pd, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
        launch_gram(f.side[k].F, a.n[k], Di, f.gpart, f.G[k], f.Gp[k], st);   // for the loss and the next half-sweep
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[2], st));
        if (loss_trace) launch_loss(f, a, f.trace + h, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[3], st));
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipEventSynchronize(evs.e[3]));
        update_ms += elapsed(evs.e[0], evs.e[1]);
        gram_ms += elapsed(evs.e[1], evs.e[2]);
        loss_ms += elapsed(evs.e[2], evs.e[3]);
    }
    CF_HIP_CHECK(ctx, hipDeviceSynchronize());
    for (int k = 0; k < 2; ++k)
        if (a.n[k])
            CF_HIP_CHECK(ctx, hipMemcpy(h_F[k], f.side[k].F, sizeof(double) * (size_t)a.n[k] * D, hipMemcpyDeviceToHost));
    if (loss_trace)
        CF_HIP_CHECK(ctx, hipMemcpy(loss_trace, f.trace, sizeof(double) * 2 * n_sweeps, hipMemcpyDeviceToHost));
    unsigned long long bad = 0;
    CF_HIP_CHECK(ctx, hipMemcpy(&bad, f.not_pd, sizeof(bad), hipMemcpyDeviceToHost));
    if (stats) {
        stats->sweeps = n_sweeps;
        stats->n_not_pd = bad;
        stats->gram_ms = (float)gram_ms;
        stats->update_ms = (float)update_ms;
        stats->loss_ms = (float)loss_ms;
    }
    return CF_OK;
}

extern "C" int cf_ials_loss(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                            const uint32_t* user_item, const float* user_conf, const float* user_pref,
                            const uint64_t* item_off, const uint32_t* item_user, const float* item_conf,
                            const float* item_pref, const double* reg_user, const double* reg_item, const double* U,
                            const double* V, double* loss) {
    if (!ctx) return CF_EINVAL;
    if (!loss) return cf_set_error(ctx, CF_EINVAL, "cf_ials_loss: null result");
    *loss = 0.0;
    IalsArgs a{{n_users, n_items}, D, {user_off, item_off}, {user_item, item_user}, {user_conf, item_conf},
               {user_pref, item_pref}, {reg_user, reg_item}, 0};
    CF_TRY(check_ials(ctx, "cf_ials_loss", a, U, V));
    if (n_users == 0 && n_items == 0) return CF_OK;
    if (error_blocks(a.nnz) > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_ials_loss: too many edges");
    CF_TRY(set_device(ctx));
    const uint64_t segs[2] = {0, 0};   // no update runs: no segment lists
    IalsLayout f{};
    CF_TRY(carve_workspace(ctx, [&](Carver& c) { carve_ials(c, f, a, segs, 1); }));
    const double* h_in[2] = {U, V};
    CF_TRY(upload_ials(ctx, f, a, h_in));
    for (int k = 0; k < 2; ++k) launch_gram(f.side[k].F, a.n[k], (int)D, f.gpart, f.G[k], f.Gp[k], nullptr);
    launch_loss(f, a, f.trace, nullptr);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(loss, f.trace, sizeof(double), hipMemcpyDeviceToHost));
    return CF_OK;
}
