// cf_topn_panel.h -- the score panel that cf_topn.hip (the N best items per user) and cf_rank.hip
// (the rank of held-out items) share: the order-preserving 64-bit key of a score, the kernel that
// scores a block of users into a panel of keys, the kernel that marks the excluded pairs in it, the
// row walk's loads, the order of two (key, item) pairs, the users-per-block rule, the factor source
// of the panel drivers (MfPanelSource), the part of both drivers up to a filled and excluded block
// (panel_check_head, PanelBlocks) and the base of the sources that score from user profiles
// (ProfilePanelSource: the graph source of cf_knn_topn.hip, the EASE one of cf_ease.hip).
//
// The selected users run in blocks of `ub` users whose scores live in a panel of 64-bit keys,
// key[user in block][item] (row stride n_items, carved from the context's ALS workspace):
//   topn_score_kernel    one workgroup per (kTU users x kTI items) tile: both tiles' rows staged in
//                        LDS kKC deep (zero-padded), 16 x 16 fp64 MFMA accumulators, and an
//                        epilogue that adds the bias term and stores the order-preserving key
//   topn_exclude_kernel  one thread per exclusion edge of the block's users: key = kKeyExcluded
//                        (a plain store: repeats and order do not matter)
// Keys: the double's bits with the sign bit set for positives and every bit flipped for
// negatives, -0 taken as +0.  Keys 0 and 1 are images of NaN bit patterns only, so they are free:
// 0 marks an excluded item, 1 a NaN score; both rank below every real score and are never listed.
// A score is one MFMA chain over its own two rows, so its bits do not depend on the tile it
// falls in, the block size or the other users.
// Everything has internal linkage.
#pragma once

// of cf_mf_common.h the panel takes the workspace helpers and the block scan, not its kernels
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "cf_mf_common.h"

namespace {

using d4 = __attribute__((ext_vector_type(4))) double;

constexpr int kTU = 64;                  // users per score tile
constexpr int kTI = 64;                  // items per score tile
constexpr int kKC = 32;                  // depth staged per pass (Dp <= 64: at most two passes)
constexpr int kSt = kKC + 2;             // LDS row stride in doubles: 2 mod 4, so the 32 lanes of a
                                         // half wave (16 rows x 2 depths) read 32 distinct 8-byte banks
constexpr int kMaxN = CF_TOPN_MAX_N;
constexpr uint64_t kKeyExcluded = 0ull;
constexpr uint64_t kKeyNaN = 1ull;
constexpr uint64_t kSign = 0x8000000000000000ull;
constexpr size_t kPanelBudget = (size_t)1 << 30;   // bytes of keys per user block (fixed, never from free HBM)

static_assert(kAT == 256 && kWaves == 4, "the score tile is four waves of 32 x 32");

__device__ __forceinline__ uint64_t score_key(double s) {
    if (s != s) return kKeyNaN;
    if (s == 0.0) s = 0.0;   // -0 ranks (and reads back) as +0
    const uint64_t b = (uint64_t)__double_as_longlong(s);
    return (b & kSign) ? ~b : (b | kSign);
}

__device__ __forceinline__ double key_score(uint64_t k) {
    return __longlong_as_double((long long)((k & kSign) ? (k ^ kSign) : ~k));
}

// Tile (ut, it) of the block: rows r0 .. r0 + kTU of the block's nb users (user of row r:
// sel[b0 + r], or b0 + r without a selection), items i0 .. i0 + kTI.  Wave w owns the 32 x 32
// quadrant (w >> 1, w & 1) as 2 x 2 MFMA tiles: A lane l = U row (l & 15), depth (l >> 4); B lane
// l = V row (l & 15), depth (l >> 4); result q of lane l = user (l >> 4) + 4 q, item l & 15.
__global__ __launch_bounds__(kAT) void topn_score_kernel(const double* __restrict__ U, const double* __restrict__ V,
                                                        int D, uint32_t n_items, uint32_t n_it,
                                                        const uint32_t* __restrict__ sel, uint32_t b0, uint32_t nb,
                                                        const double* __restrict__ bu, const double* __restrict__ bi,
                                                        double mean, uint64_t* __restrict__ panel) {
    __shared__ double s_u[kTU * kSt];
    __shared__ double s_v[kTI * kSt];
    const uint32_t ut = blockIdx.x / n_it, it = blockIdx.x % n_it;
    const uint32_t r0 = ut * kTU, i0 = it * kTI;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wu = (wave >> 1) * 32, wi = (wave & 1) * 32;
    const int Dp = (D + 3) & ~3;
    d4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = d4{0.0, 0.0, 0.0, 0.0};
    for (int d0 = 0; d0 < Dp; d0 += kKC) {
        const int dc = min(kKC, Dp - d0);   // a multiple of 4
        if (d0) __syncthreads();
        for (int idx = threadIdx.x; idx < kTU * dc; idx += kAT) {
            const int r = idx / dc, dd = idx - r * dc, d = d0 + dd;
            double a = 0.0, b = 0.0;
            if (d < D) {
                if (r0 + r < nb) {
                    const uint32_t u = sel ? sel[b0 + r0 + r] : b0 + r0 + r;
                    a = U[(size_t)u * D + d];
                }
                if ((uint64_t)i0 + r < n_items) b = V[((size_t)i0 + r) * D + d];
            }
            s_u[r * kSt + dd] = a;
            s_v[r * kSt + dd] = b;
        }
        __syncthreads();
        for (int kk = 0; kk < dc; kk += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) av[x] = s_u[(wu + x * 16 + (lane & 15)) * kSt + kk + (lane >> 4)];
#pragma unroll
            for (int y = 0; y < 2; ++y) bv[y] = s_v[(wi + y * 16 + (lane & 15)) * kSt + kk + (lane >> 4)];
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
                    acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], bv[y], acc[x][y], 0, 0, 0);
        }
    }
    const bool biased = bu || bi;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t r = r0 + wu + x * 16 + (lane >> 4) + 4 * q;
            if (r >= nb) continue;
            double tu = mean;   // mean + bias_user[u]
            if (bu) tu = mean + bu[sel ? sel[b0 + r] : b0 + r];
            uint64_t* prow = panel + (size_t)r * n_items;
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const uint64_t i = (uint64_t)i0 + wi + y * 16 + (lane & 15);
                if (i >= n_items) continue;
                double s = acc[x][y][q];
                if (biased) s = s + (bi ? bi[i] + tu : tu);
                prow[i] = score_key(s);
            }
        }
}

// Edge e of the block: the (e - first edge of its row)-th exclusion of the row r whose range in
// sel_off (the prefix of the selected users' exclusion counts; excl_off itself without a
// selection) holds sel_off[b0] + e.
__global__ __launch_bounds__(kAT) void topn_exclude_kernel(const uint64_t* __restrict__ excl_off,
                                                          const uint32_t* __restrict__ excl_item,
                                                          const uint64_t* __restrict__ sel_off,
                                                          const uint32_t* __restrict__ sel, uint32_t b0, uint32_t nb,
                                                          uint32_t n_items, uint64_t n_edges,
                                                          uint64_t* __restrict__ panel) {
    const uint64_t e = (uint64_t)blockIdx.x * kAT + threadIdx.x;
    if (e >= n_edges) return;
    const uint64_t target = sel_off[b0] + e;
    uint32_t lo = 0, hi = nb;   // first row whose range starts above target
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sel_off[b0 + mid] <= target) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return;
    const uint32_t r = lo - 1;
    const uint32_t u = sel ? sel[b0 + r] : b0 + r;
    const uint32_t item = excl_item[excl_off[u] + (target - sel_off[b0 + r])];
    if (item < n_items) panel[(size_t)r * n_items + item] = kKeyExcluded;
}

// Keys first, first + STRIDE, .. (kUnroll of them) of a row of n keys, requested together: a walk
// with one load in flight per lane is bound by the load latency, not by L2 or HBM.  Past the end
// of the row: kKeyExcluded, which no pass counts.
constexpr int kUnroll = 8;
template <int STRIDE>
__device__ __forceinline__ void load_keys(const uint64_t* __restrict__ row, uint64_t first, uint64_t n,
                                          uint64_t (&kv)[kUnroll]) {
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
        const uint64_t i = first + (uint64_t)j * STRIDE;
        kv[j] = i < n ? row[i] : kKeyExcluded;
    }
}

__device__ __forceinline__ bool topn_before(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    return ka > kb || (ka == kb && ia < ib);
}

// Users per block: the forced value, or as many rows of n_items keys as fit the budget (whole
// score tiles when at least one fits); at least 1, at most the selection.
uint32_t topn_block_users(const cf_ctx* ctx, uint32_t n_items, uint32_t n_out) {
    uint64_t ub = ctx->topn_block;
    if (!ub) {
        ub = std::max<uint64_t>(1, kPanelBudget / ((uint64_t)n_items * sizeof(uint64_t)));
        if (ub >= (uint64_t)kTU) ub -= ub % kTU;
    }
    return (uint32_t)std::min<uint64_t>(ub, n_out);
}

// The factor source of the panel drivers (cf_mf_topn, cf_mf_rank_eval): U, V and the biases in
// the workspace, topn_score_kernel over the block's tiles.
struct MfPanelSource final : PanelSource {
    uint32_t n_users = 0, n_items = 0, D = 0;
    const double* U = nullptr;
    const double* V = nullptr;
    const double* bias_user = nullptr;
    const double* bias_item = nullptr;
    double mean = 0.0;
    double* dU = nullptr;
    double* dV = nullptr;
    double* dbu = nullptr;
    double* dbi = nullptr;

    void carve(Carver& c) {
        dU = c.take<double>((size_t)n_users * D);
        dV = c.take<double>((size_t)n_items * D);
        dbu = bias_user ? c.take<double>(n_users) : nullptr;
        dbi = bias_item ? c.take<double>(n_items) : nullptr;
    }
    bool valid() const override { return U && V; }
    size_t workspace(uint32_t) const override {
        MfPanelSource s = *this;
        Carver c;
        s.carve(c);
        return c.pos;
    }
    int upload(cf_ctx* ctx, void* ws, uint32_t, hipStream_t, float*) override {
        Carver c;
        c.base = static_cast<char*>(ws);
        carve(c);
        CF_HIP_CHECK(ctx, hipMemcpy(dU, U, sizeof(double) * (size_t)n_users * D, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy(dV, V, sizeof(double) * (size_t)n_items * D, hipMemcpyHostToDevice));
        if (bias_user) CF_HIP_CHECK(ctx, hipMemcpy(dbu, bias_user, sizeof(double) * n_users, hipMemcpyHostToDevice));
        if (bias_item) CF_HIP_CHECK(ctx, hipMemcpy(dbi, bias_item, sizeof(double) * n_items, hipMemcpyHostToDevice));
        return CF_OK;
    }
    int fill(cf_ctx*, hipStream_t st, const uint32_t* d_sel, uint32_t b0, uint32_t nb, uint64_t* d_panel) override {
        const uint32_t n_it = (uint32_t)(((uint64_t)n_items + kTI - 1) / kTI);
        const uint32_t tiles = ((nb + kTU - 1) / kTU) * n_it;
        const double bias_mean = (bias_user || bias_item) ? mean : 0.0;
        hipLaunchKernelGGL(topn_score_kernel, dim3(tiles), dim3(kAT), 0, st, (const double*)dU, (const double*)dV, (int)D,
                           n_items, n_it, d_sel, b0, nb, (const double*)dbu, (const double*)dbi, bias_mean, d_panel);
        return CF_OK;
    }
};

// The first checks of both panel drivers, in their order.
inline int panel_check_head(cf_ctx* ctx, const std::string& fn, uint32_t N, const uint64_t* excl_off,
                            const uint32_t* excl_item) {
    if (N > CF_TOPN_MAX_N) return cf_set_error(ctx, CF_ERANGE, fn + ": N above CF_TOPN_MAX_N");
    if (N == 0) return cf_set_error(ctx, CF_EINVAL, fn + ": N = 0");
    if ((excl_off == nullptr) != (excl_item == nullptr))
        return cf_set_error(ctx, CF_EINVAL, fn + ": exactly one of excl_off / excl_item is null");
    return CF_OK;
}

// The user blocks of both panel drivers (cf_topn_drive, cf_rank_drive), after their checks: the
// n_out users of the selection (sel_user on the host; null = users 0 .. n_out - 1) run in blocks
// of ub, each filled by src and stripped of its exclusions; what is done with a filled block is
// the caller's.  begin() sizes the blocks, carves the workspace (own(Carver&) adds the caller's
// arrays to the same carve, once per pass) and uploads source, exclusions and selection; run()
// is the loop: per block launch(b0, nb) between the events, then collect(b0, nb) -> int with the
// copies back, which wait for the stream.  score_ms: the fills (and what the source's upload
// adds), use_ms: exclusion and launch().
struct PanelBlocks {
    cf_ctx* ctx;
    std::string fn;
    PanelSource& src;
    uint32_t n_users, n_items;
    const uint64_t* excl_off;
    const uint32_t* excl_item;
    uint32_t n_out;
    const uint32_t* sel_user;

    uint32_t ub = 0, blocks = 0;
    uint64_t nnz = 0;
    std::vector<uint64_t> sel_off;   // the selection's own prefix of exclusion counts; without a selection it is excl_off
    uint64_t* d_excl_off = nullptr;
    uint32_t* d_excl_item = nullptr;
    uint64_t* d_sel_off = nullptr;
    uint32_t* d_sel = nullptr;
    uint64_t* d_panel = nullptr;
    hipStream_t st = nullptr;
    float score_ms = 0.0f, use_ms = 0.0f;

    template <class Own>
    int begin(Own own) {
        nnz = excl_off ? excl_off[n_users] : 0;
        if (sel_user && nnz) {
            sel_off.assign((size_t)n_out + 1, 0);
            for (uint32_t j = 0; j < n_out; ++j)
                sel_off[j + 1] = sel_off[j] + (excl_off[sel_user[j] + 1] - excl_off[sel_user[j]]);
        }
        ub = topn_block_users(ctx, n_items, n_out);
        const uint32_t n_it = (uint32_t)(((uint64_t)n_items + kTI - 1) / kTI);
        if ((uint64_t)((ub + kTU - 1) / kTU) * n_it > 0x7fffffffull)
            return cf_set_error(ctx, CF_ERANGE, fn + ": users per block x items exceed the launch grid");
        void* d_src = nullptr;
        const size_t src_bytes = src.workspace(ub);
        CF_TRY(carve_workspace(ctx, [&](Carver& c) {
            d_src = c.take<char>(src_bytes);
            d_excl_off = nnz ? c.take<uint64_t>((size_t)n_users + 1) : nullptr;
            d_excl_item = nnz ? c.take<uint32_t>(nnz) : nullptr;
            d_sel_off = !sel_off.empty() ? c.take<uint64_t>(sel_off.size()) : nullptr;
            d_sel = sel_user ? c.take<uint32_t>(n_out) : nullptr;
            d_panel = c.take<uint64_t>((size_t)ub * n_items);
            own(c);
        }));
        CF_TRY(src.upload(ctx, d_src, ub, st, &score_ms));
        if (nnz) {
            CF_HIP_CHECK(ctx, hipMemcpy(d_excl_off, excl_off, sizeof(uint64_t) * ((size_t)n_users + 1), hipMemcpyHostToDevice));
            CF_HIP_CHECK(ctx, hipMemcpy(d_excl_item, excl_item, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
        }
        if (d_sel_off)
            CF_HIP_CHECK(ctx, hipMemcpy(d_sel_off, sel_off.data(), sizeof(uint64_t) * sel_off.size(), hipMemcpyHostToDevice));
        if (sel_user) CF_HIP_CHECK(ctx, hipMemcpy(d_sel, sel_user, sizeof(uint32_t) * n_out, hipMemcpyHostToDevice));
        return CF_OK;
    }

    template <class Launch, class Collect>
    int run(Launch launch, Collect collect) {
        MfEvents<3> evs;
        for (hipEvent_t& e : evs.e) CF_HIP_CHECK(ctx, hipEventCreate(&e));
        const uint64_t* dev_off = d_sel_off ? d_sel_off : d_excl_off;
        const uint64_t* host_off = !sel_off.empty() ? sel_off.data() : excl_off;
        for (uint32_t b0 = 0; b0 < n_out; b0 += ub) {
            const uint32_t nb = std::min(ub, n_out - b0);
            CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
            CF_TRY(src.fill(ctx, st, (const uint32_t*)d_sel, b0, nb, d_panel));
            CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
            const uint64_t edges = nnz ? host_off[b0 + nb] - host_off[b0] : 0;
            if (edges) {
                if ((edges + kAT - 1) / kAT > 0x7fffffffull)
                    return cf_set_error(ctx, CF_ERANGE, fn + ": exclusions of one user block exceed the launch grid");
                hipLaunchKernelGGL(topn_exclude_kernel, dim3((unsigned)((edges + kAT - 1) / kAT)), dim3(kAT), 0, st,
                                   (const uint64_t*)d_excl_off, (const uint32_t*)d_excl_item, dev_off, (const uint32_t*)d_sel,
                                   b0, nb, n_items, edges, d_panel);
            }
            launch(b0, nb);
            CF_HIP_CHECK(ctx, hipEventRecord(evs.e[2], st));
            CF_HIP_CHECK(ctx, hipGetLastError());
            CF_TRY(collect(b0, nb));
            score_ms += elapsed(evs.e[0], evs.e[1]);
            use_ms += elapsed(evs.e[1], evs.e[2]);
            ++blocks;
        }
        return CF_OK;
    }
};

// What the sources that score from user profiles share (the graph in cf_knn_topn.hip, EASE in
// cf_ease.hip): the profile CSR on the host, checked by the entry point, and its copy at the head
// of the source's workspace.
struct ProfilePanelSource : PanelSource {
    uint32_t n_users = 0, n_items = 0;
    const uint64_t* prof_off = nullptr;
    const uint32_t* prof_item = nullptr;
    const float* prof_rating = nullptr;
    struct Dev {
        uint64_t* off;
        uint32_t* item;
        float* rating;
    } dev{};

    Dev carve(Carver& c) const {
        const uint64_t nnz = prof_off[n_users];
        return Dev{c.take<uint64_t>((size_t)n_users + 1), c.take<uint32_t>(nnz), c.take<float>(nnz)};
    }
    int upload_profiles(cf_ctx* ctx, Carver& c) {
        dev = carve(c);
        const uint64_t nnz = prof_off[n_users];
        CF_HIP_CHECK(ctx, hipMemcpy(dev.off, prof_off, sizeof(uint64_t) * ((size_t)n_users + 1), hipMemcpyHostToDevice));
        if (nnz) {
            CF_HIP_CHECK(ctx, hipMemcpy(dev.item, prof_item, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
            CF_HIP_CHECK(ctx, hipMemcpy(dev.rating, prof_rating, sizeof(float) * nnz, hipMemcpyHostToDevice));
        }
        return CF_OK;
    }
    bool valid() const override { return true; }
    size_t workspace(uint32_t) const override {
        Carver c;
        carve(c);
        return c.pos;
    }
    int upload(cf_ctx* ctx, void* ws, uint32_t, hipStream_t, float*) override {
        Carver c;
        c.base = static_cast<char*>(ws);
        return upload_profiles(ctx, c);
    }
};

}  // namespace
