// cf_topn.hip -- top-N recommendation from fitted factors (cf_mf_topn): for every selected user
// the N best items by score = U_u . V_i (+ biases) among the items the user has not rated.
// The reference stops at the factor files and the PREDICT edges (als.cpp:493-510); this is the
// scorer the five factorizers (als, sgd, biassgd, svdpp, svd) lacked.  DESIGN 3.16.
//
// The selected users run in blocks of `ub` users whose scores live in a panel of 64-bit keys;
// the panel, its keys and the two kernels that fill it (topn_score_kernel, topn_exclude_kernel)
// are cf_topn_panel.h, shared with cf_rank.hip.  On the filled panel:
//   topn_select_kernel   one workgroup per user row: 8 x 8-bit radix select of the K-th largest
//                        key, K = min(N, candidates), compaction of the keys above it and of the
//                        lowest-index ties at it, a bitonic sort of the <= 1024 survivors in LDS by
//                        (key descending, item ascending), and the keys mapped back to doubles
// A score's bits do not depend on the tile it falls in, the block size or the other users; the
// only atomics are integer counts (the LDS histogram, the NaN count).
// The host driver (cf_topn_drive: its checks, the list slots, the selection kernel, the copies back
// and the stats) takes the panel's filler as a PanelSource (cf_internal.h): the factors here, the
// item graph in cf_knn_topn.hip, EASE in cf_ease.hip.  The user blocks, their workspace, the uploads
// and the exclusion launch are PanelBlocks (cf_topn_panel.h), shared with cf_rank_drive.

#include "cf_topn_panel.h"

namespace {

// One histogram increment per active lane, called by whole waves.  The keys of a row share their
// high bytes, so in the first passes most lanes of a wave hit one bin, and 64 LDS atomics on one
// address run one after the other: up to kAggRounds times the lanes that share the first active
// lane's bin add their count once; what is left (spread bins) adds lane by lane.  Integer sums:
// the order does not show.
constexpr int kAggRounds = 4;
__device__ __forceinline__ void hist_add(unsigned int* s_hist, bool active, unsigned int bin, int lane) {
#pragma unroll
    for (int round = 0; round < kAggRounds; ++round) {
        const unsigned long long act = __ballot(active);
        if (!act) return;   // the whole wave
        const int first = __ffsll((long long)act) - 1;
        const unsigned int b = (unsigned int)__shfl((int)bin, first);
        const bool mine = active && bin == b;
        const unsigned long long same = __ballot(mine);
        if (lane == first) atomicAdd(&s_hist[b], (unsigned int)__popcll(same));
        if (mine) active = false;
    }
    if (active) atomicAdd(&s_hist[bin], 1u);
}

__global__ __launch_bounds__(kAT) void topn_select_kernel(const uint64_t* __restrict__ panel, uint32_t n_items,
                                                         uint32_t N, uint32_t* __restrict__ out_items,
                                                         double* __restrict__ out_scores,
                                                         uint32_t* __restrict__ out_count,
                                                         unsigned long long* __restrict__ n_nan) {
    __shared__ unsigned int s_hist[256];
    __shared__ unsigned int s_sel[2];
    __shared__ uint32_t s_scan[kWaves + 1];
    __shared__ unsigned int s_cnt[2][kWaves];
    __shared__ uint64_t s_key[kMaxN];
    __shared__ uint32_t s_item[kMaxN];
    const uint64_t* row = panel + (size_t)blockIdx.x * n_items;
    uint32_t* o_items = out_items + (size_t)blockIdx.x * N;
    double* o_scores = out_scores + (size_t)blockIdx.x * N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // candidates (keys above the two markers) and NaN scores of the row
    unsigned int cv = 0, cn = 0;
    uint64_t kv[kUnroll];
    for (uint64_t i0 = 0; i0 < n_items; i0 += (uint64_t)kAT * kUnroll) {
        load_keys<kAT>(row, i0 + threadIdx.x, n_items, kv);
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) {
            cv += kv[j] > kKeyNaN;
            cn += kv[j] == kKeyNaN;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        cv += __shfl_xor(cv, o);
        cn += __shfl_xor(cn, o);
    }
    if (lane == 0) {
        s_cnt[0][wave] = cv;
        s_cnt[1][wave] = cn;
    }
    __syncthreads();
    unsigned int valid = 0, nans = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        valid += s_cnt[0][w];
        nans += s_cnt[1][w];
    }
    if (threadIdx.x == 0 && nans) atomicAdd(n_nan, (unsigned long long)nans);
    const uint32_t K = min(N, valid);
    if (threadIdx.x == 0) out_count[blockIdx.x] = K;
    for (uint32_t p = K + threadIdx.x; p < N; p += kAT) {
        o_items[p] = 0xffffffffu;
        o_scores[p] = 0.0;
    }
    if (K == 0) return;   // the whole workgroup

    // the K-th largest key T, and rem = how many of the keys equal to T are listed
    uint64_t prefix = 0, mask = 0;
    uint32_t rem = K;
    for (int shift = 56; shift >= 0; shift -= 8) {
        __syncthreads();
        s_hist[threadIdx.x] = 0u;   // kAT == 256 bins
        __syncthreads();
        for (uint64_t i0 = 0; i0 < n_items; i0 += (uint64_t)kAT * kUnroll) {   // whole waves enter hist_add
            load_keys<kAT>(row, i0 + threadIdx.x, n_items, kv);
#pragma unroll
            for (int j = 0; j < kUnroll; ++j)
                hist_add(s_hist, kv[j] > kKeyNaN && (kv[j] & mask) == prefix, (unsigned int)(kv[j] >> shift) & 255u, lane);
        }
        __syncthreads();
        // thread t looks at bin 255 - t: `above` = the keys in higher bins; the bin that holds the
        // rem-th largest is the one with above < rem <= above + its count (bin 0 catches the rest)
        const unsigned int mine = s_hist[255 - threadIdx.x];
        unsigned int all;
        const unsigned int above = block_excl_scan(mine, s_scan, &all);
        if (above < rem && (rem <= above + mine || threadIdx.x == kAT - 1)) {
            s_sel[0] = 255u - threadIdx.x;
            s_sel[1] = above;
        }
        __syncthreads();
        prefix |= (uint64_t)s_sel[0] << shift;
        mask |= 255ull << shift;
        rem -= s_sel[1];
    }
    const uint64_t T = prefix;
    const uint32_t G = K - rem;   // keys above T

    // compaction: wave w walks its contiguous quarter of the row, 64 items at a time, so the ties
    // are numbered in item order; keys above T fill slots [0, G), the first rem ties [G, K)
    const uint64_t per = ((((uint64_t)n_items + kWaves - 1) / kWaves) + 63) & ~63ull;
    const uint64_t beg = min((uint64_t)n_items, per * wave), end = min((uint64_t)n_items, beg + per);
    unsigned int cg = 0, ct = 0;
    for (uint64_t i0 = beg; i0 < end; i0 += 64 * kUnroll) {
        load_keys<64>(row, i0 + lane, end, kv);
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) {
            cg += kv[j] > T;
            ct += kv[j] == T;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        cg += __shfl_xor(cg, o);
        ct += __shfl_xor(ct, o);
    }
    __syncthreads();   // s_cnt was read above
    if (lane == 0) {
        s_cnt[0][wave] = cg;
        s_cnt[1][wave] = ct;
    }
    __syncthreads();
    unsigned int gpos = 0, tpos = 0;
    for (int w = 0; w < wave; ++w) {
        gpos += s_cnt[0][w];
        tpos += s_cnt[1][w];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint64_t i0 = beg; i0 < end; i0 += 64 * kUnroll) {
        load_keys<64>(row, i0 + lane, end, kv);
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) {   // in item order
            const uint64_t i = i0 + (uint64_t)j * 64 + lane;
            const bool gt = kv[j] > T, tie = kv[j] == T;   // T is a real key: the fill value is neither
            const unsigned long long bg = __ballot(gt), bt = __ballot(tie);
            if (gt) {
                const unsigned int p = gpos + (unsigned int)__popcll(bg & below);
                if (p < G) {
                    s_key[p] = kv[j];
                    s_item[p] = (uint32_t)i;
                }
            }
            if (tie) {
                const unsigned int tr = tpos + (unsigned int)__popcll(bt & below);
                if (tr < rem) {
                    s_key[G + tr] = kv[j];
                    s_item[G + tr] = (uint32_t)i;
                }
            }
            gpos += (unsigned int)__popcll(bg);
            tpos += (unsigned int)__popcll(bt);
        }
    }
    uint32_t P = 1;
    while (P < K) P <<= 1;   // <= kMaxN
    for (uint32_t p = K + threadIdx.x; p < P; p += kAT) {
        s_key[p] = kKeyExcluded;
        s_item[p] = 0xffffffffu;
    }
    __syncthreads();

    // bitonic sort of the P slots by (key descending, item ascending); the padding sorts last
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += kAT) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint64_t ka = s_key[i], kb = s_key[l];
                    const uint32_t ia = s_item[i], ib = s_item[l];
                    const bool swap = (i & k) == 0 ? topn_before(kb, ib, ka, ia) : topn_before(ka, ia, kb, ib);
                    if (swap) {
                        s_key[i] = kb;
                        s_item[i] = ib;
                        s_key[l] = ka;
                        s_item[l] = ia;
                    }
                }
            }
            __syncthreads();
        }
    for (uint32_t p = threadIdx.x; p < K; p += kAT) {
        o_items[p] = s_item[p];
        o_scores[p] = key_score(s_key[p]);
    }
}

}  // namespace

extern "C" int cf_debug_topn_tile_users(void) { return kTU; }
extern "C" int cf_debug_topn_tile_items(void) { return kTI; }

extern "C" int cf_set_topn_block(cf_ctx* ctx, uint32_t users_per_block) {
    if (!ctx) return CF_EINVAL;
    ctx->topn_block = users_per_block;
    return CF_OK;
}

extern "C" int cf_mf_topn(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const double* U, const double* V,
                          const double* bias_user, const double* bias_item, double mean, const uint64_t* excl_off,
                          const uint32_t* excl_item, uint32_t n_sel, const uint32_t* sel_user, uint32_t N,
                          uint32_t* items, double* scores, uint32_t* count, cf_topn_stats* stats) {
    if (!ctx) return CF_EINVAL;
    const std::string fn = "cf_mf_topn";
    if (D == 0) return cf_set_error(ctx, CF_ERANGE, fn + ": D = 0");
    if (D > CF_ALS_MAX_D) return cf_set_error(ctx, CF_ERANGE, fn + ": D above CF_ALS_MAX_D");
    MfPanelSource src;
    src.n_users = n_users, src.n_items = n_items, src.D = D;
    src.U = U, src.V = V, src.bias_user = bias_user, src.bias_item = bias_item, src.mean = mean;
    return cf_topn_drive(ctx, "cf_mf_topn", src, n_users, n_items, excl_off, excl_item, n_sel, sel_user, N, items, scores,
                         count, stats);
}

// The N best candidates of every selected user from the panel that `src` fills, block by block.
int cf_topn_drive(cf_ctx* ctx, const char* name, PanelSource& src, uint32_t n_users, uint32_t n_items,
                  const uint64_t* excl_off, const uint32_t* excl_item, uint32_t n_sel, const uint32_t* sel_user,
                  uint32_t N, uint32_t* items, double* scores, uint32_t* count, cf_topn_stats* stats) {
    const std::string fn = name;
    CF_TRY(panel_check_head(ctx, fn, N, excl_off, excl_item));
    const uint32_t n_out = sel_user ? n_sel : n_users;
    if (sel_user)
        for (uint32_t j = 0; j < n_sel; ++j)
            if (sel_user[j] >= n_users) return cf_set_error(ctx, CF_EINVAL, fn + ": selected user out of range");
    if (n_out && !count) return cf_set_error(ctx, CF_EINVAL, fn + ": null argument");
    if (excl_off && n_users) CF_TRY(check_csr(ctx, name, "exclusion", n_users, excl_off, excl_item, n_items));
    if (stats) *stats = cf_topn_stats{};
    for (uint32_t j = 0; j < n_out; ++j) count[j] = 0;
    if (n_out == 0 || n_items == 0) return CF_OK;
    if (!src.valid() || !items || !scores) return cf_set_error(ctx, CF_EINVAL, fn + ": null argument");
    CF_TRY(set_device(ctx));

    PanelBlocks pb{ctx, fn, src, n_users, n_items, excl_off, excl_item, n_out, sel_user};
    uint32_t* d_items = nullptr;   // the lists of one block
    double* d_scores = nullptr;
    uint32_t* d_count = nullptr;
    unsigned long long* d_nan = nullptr;
    CF_TRY(pb.begin([&](Carver& c) {
        d_items = c.take<uint32_t>((size_t)pb.ub * N);
        d_scores = c.take<double>((size_t)pb.ub * N);
        d_count = c.take<uint32_t>(pb.ub);
        d_nan = c.take<unsigned long long>(1);
    }));
    CF_HIP_CHECK(ctx, hipMemset(d_nan, 0, sizeof(unsigned long long)));
    CF_TRY(pb.run(
        [&](uint32_t, uint32_t nb) {
            hipLaunchKernelGGL(topn_select_kernel, dim3(nb), dim3(kAT), 0, pb.st, (const uint64_t*)pb.d_panel, n_items, N,
                               d_items, d_scores, d_count, d_nan);
        },
        [&](uint32_t b0, uint32_t nb) {
            CF_HIP_CHECK(ctx, hipMemcpy(items + (size_t)b0 * N, d_items, sizeof(uint32_t) * (size_t)nb * N, hipMemcpyDeviceToHost));
            CF_HIP_CHECK(ctx, hipMemcpy(scores + (size_t)b0 * N, d_scores, sizeof(double) * (size_t)nb * N, hipMemcpyDeviceToHost));
            CF_HIP_CHECK(ctx, hipMemcpy(count + b0, d_count, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost));
            return (int)CF_OK;
        }));
    unsigned long long n_nan = 0;
    CF_HIP_CHECK(ctx, hipMemcpy(&n_nan, d_nan, sizeof(n_nan), hipMemcpyDeviceToHost));
    if (stats) {
        stats->blocks = pb.blocks;
        stats->n_nan = n_nan;
        stats->score_ms = pb.score_ms;
        stats->select_ms = pb.use_ms;
    }
    return CF_OK;
}
