// cf_rank.hip -- ranking evaluation of fitted factors (cf_mf_rank_eval): the exact rank of every
// held-out edge in its user's full candidate ordering, and precision / recall / NDCG / AP / RR /
// AUC at a cutoff per user with their means and the expected percentile rank of Hu, Koren and
// Volinsky.  No program of the reference ranks anything; this closes the pipeline that ials and
// recommend opened.  DESIGN 3.18.
//
// Only the users with a held-out edge are scored: their ascending list goes through the `sel`
// path of the panel kernels (cf_topn_panel.h), in the user blocks of cf_mf_topn.  On the filled
// panel:
//   rank_count_kernel    one workgroup per user row.  The user's held-out items are taken kRankT
//                        at a time: their keys are fetched from the row (key 0 = excluded, 1 = NaN:
//                        rank UINT32_MAX), then the row is walked once with kUnroll loads in flight
//                        per lane while every lane keeps kRankT counters of the keys that come
//                        before each target (topn_before), then a wave and a block reduction.  The
//                        first walk also counts the candidates (keys above 1).
// The device returns integers only and integer sums take any order, so the ranks do not depend on
// the block size; the metrics are computed on the host from them in fixed orders (rank_metrics).
// The only atomic is the integer count of NaN held-out items.
// The host driver (cf_rank_drive: its checks, the evaluated users, the held-out arrays, the count
// kernel, the copies back and the metrics) takes the panel's filler as a PanelSource and runs the
// user blocks through PanelBlocks (cf_topn_panel.h), as cf_topn_drive does.

#include <algorithm>
#include <cmath>

#include "cf_topn_panel.h"

namespace {

constexpr int kRankT = 16;               // held-out items counted per walk of a row
constexpr uint32_t kRankNone = 0xffffffffu;

__device__ __forceinline__ uint32_t wave_uniform(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// Row blockIdx.x of the block is the user b0 + blockIdx.x of the evaluated list; its held-out edges
// are held_item[held_off[b0 + row] .. held_off[b0 + row + 1]) (held_off: the prefix over the
// evaluated users, whose edges are the held-out CSR's in the same order).  Every held item is below
// n_items (checked by the host).
__global__ __launch_bounds__(kAT) void rank_count_kernel(const uint64_t* __restrict__ panel, uint32_t n_items,
                                                        const uint64_t* __restrict__ held_off,
                                                        const uint32_t* __restrict__ held_item, uint32_t b0,
                                                        uint32_t* __restrict__ out_rank,
                                                        uint32_t* __restrict__ out_ncand,
                                                        unsigned long long* __restrict__ n_nan_held) {
    __shared__ uint64_t s_tkey[kRankT];
    __shared__ uint32_t s_titem[kRankT];
    __shared__ uint32_t s_red[kWaves][kRankT + 1];
    const uint64_t* row = panel + (size_t)blockIdx.x * n_items;
    const uint64_t e0 = held_off[b0 + blockIdx.x], e1 = held_off[b0 + blockIdx.x + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    for (uint64_t g0 = e0; g0 < e1; g0 += kRankT) {   // the same trips for the whole workgroup
        if (threadIdx.x < kRankT) {
            // an empty slot: the largest key at item 0, which nothing comes before
            uint64_t k = ~0ull;
            uint32_t it = 0;
            if (g0 + threadIdx.x < e1) {
                it = held_item[g0 + threadIdx.x];
                k = row[it];
            }
            s_tkey[threadIdx.x] = k;
            s_titem[threadIdx.x] = it;
        }
        __syncthreads();
        // the targets are the same in every lane: kept in scalar registers
        uint32_t tlo[kRankT], thi[kRankT], ti[kRankT];
#pragma unroll
        for (int t = 0; t < kRankT; ++t) {
            const uint64_t k = s_tkey[t];
            tlo[t] = wave_uniform((uint32_t)k);
            thi[t] = wave_uniform((uint32_t)(k >> 32));
            ti[t] = wave_uniform(s_titem[t]);
        }
        uint32_t cnt[kRankT], cand = 0;
#pragma unroll
        for (int t = 0; t < kRankT; ++t) cnt[t] = 0;
        uint64_t kv[kUnroll];
        for (uint64_t i0 = 0; i0 < n_items; i0 += (uint64_t)kAT * kUnroll) {
            load_keys<kAT>(row, i0 + threadIdx.x, n_items, kv);
#pragma unroll
            for (int j = 0; j < kUnroll; ++j) {
                // past the end of the row: kKeyExcluded, which comes before no candidate
                const uint32_t i = (uint32_t)(i0 + (uint64_t)j * kAT + threadIdx.x);
                cand += kv[j] > kKeyNaN;
#pragma unroll
                for (int t = 0; t < kRankT; ++t)
                    cnt[t] += topn_before(kv[j], i, ((uint64_t)thi[t] << 32) | tlo[t], ti[t]);
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            cand += __shfl_xor(cand, o);
#pragma unroll
            for (int t = 0; t < kRankT; ++t) cnt[t] += __shfl_xor(cnt[t], o);
        }
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < kRankT; ++t) s_red[wave][t] = cnt[t];
            s_red[wave][kRankT] = cand;
        }
        __syncthreads();
        if (threadIdx.x <= kRankT) {
            uint32_t sum = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) sum += s_red[w][threadIdx.x];
            if (threadIdx.x == kRankT) {
                if (g0 == e0) out_ncand[blockIdx.x] = sum;
            } else if (g0 + threadIdx.x < e1) {
                const uint64_t k = s_tkey[threadIdx.x];
                out_rank[g0 + threadIdx.x] = k > kKeyNaN ? sum : kRankNone;
                if (k == kKeyNaN) atomicAdd(n_nan_held, 1ull);
            }
        }
        __syncthreads();   // s_tkey and s_red are rewritten by the next group
    }
}

// The record of one user from its C candidates and the ranks of its held-out edges (CSR order,
// kRankNone = skipped), and the user's share of the percentile-rank sums.  `sorted` is scratch.
// Every sum runs in ascending rank order.
void rank_metrics(uint32_t C, const uint32_t* rank, const double* w, uint64_t n_edges, uint32_t N,
                  std::vector<uint32_t>& sorted, cf_rank_user* rec, double* pr_num, double* pr_den) {
    sorted.clear();
    for (uint64_t e = 0; e < n_edges; ++e)
        if (rank[e] != kRankNone) sorted.push_back(rank[e]);
    *rec = cf_rank_user{};
    const uint32_t m = (uint32_t)sorted.size();
    if (m == 0) return;
    std::sort(sorted.begin(), sorted.end());
    const uint32_t cut = std::min(m, N);
    uint32_t hits = 0;
    double dcg = 0.0, idcg = 0.0, ap = 0.0;
    uint64_t auc_num = 0;   // sum of C - m - r_j + j: the non-held candidates ranked after r_j
    for (uint32_t j = 0; j < m; ++j) {
        const uint32_t r = sorted[j];
        if (r < N) {
            ++hits;
            dcg += 1.0 / std::log2((double)r + 2.0);
            ap += (double)(j + 1) / ((double)r + 1.0);
        }
        auc_num += (uint64_t)C - m - r + j;
    }
    for (uint32_t t = 0; t < cut; ++t) idcg += 1.0 / std::log2((double)t + 2.0);
    rec->n_cand = C;
    rec->n_rel = m;
    rec->hits = hits;
    rec->precision = (double)hits / (double)N;
    rec->recall = (double)hits / (double)m;
    rec->ndcg = dcg / idcg;
    rec->ap = ap / (double)cut;
    rec->rr = 1.0 / ((double)sorted[0] + 1.0);
    rec->auc = C > m ? (double)auc_num / ((double)m * (double)(C - m)) : 0.0;
    for (uint64_t e = 0; e < n_edges; ++e) {   // CSR order
        if (rank[e] == kRankNone) continue;
        const double we = w ? w[e] : 1.0;
        const double pr = C > 1 ? (double)rank[e] / (double)(C - 1) : 0.0;
        *pr_num += we * pr;
        *pr_den += we;
    }
}

}  // namespace

extern "C" int cf_debug_rank_targets(void) { return kRankT; }
extern "C" int cf_debug_rank_walk(void) { return kAT * kUnroll; }

extern "C" int cf_mf_rank_eval(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const double* U,
                               const double* V, const double* bias_user, const double* bias_item, double mean,
                               const uint64_t* excl_off, const uint32_t* excl_item, const uint64_t* held_off,
                               const uint32_t* held_item, const double* held_w, uint32_t N, uint32_t* rank,
                               cf_rank_user* users, cf_rank_summary* summary) {
    if (!ctx) return CF_EINVAL;
    const std::string fn = "cf_mf_rank_eval";
    if (D == 0) return cf_set_error(ctx, CF_ERANGE, fn + ": D = 0");
    if (D > CF_ALS_MAX_D) return cf_set_error(ctx, CF_ERANGE, fn + ": D above CF_ALS_MAX_D");
    MfPanelSource src;
    src.n_users = n_users, src.n_items = n_items, src.D = D;
    src.U = U, src.V = V, src.bias_user = bias_user, src.bias_item = bias_item, src.mean = mean;
    return cf_rank_drive(ctx, "cf_mf_rank_eval", src, n_users, n_items, excl_off, excl_item, held_off, held_item, held_w, N,
                         rank, users, summary);
}

// The rank of every held-out edge in the panel that `src` fills, block by block, and the metrics.
int cf_rank_drive(cf_ctx* ctx, const char* name, PanelSource& src, uint32_t n_users, uint32_t n_items,
                  const uint64_t* excl_off, const uint32_t* excl_item, const uint64_t* held_off,
                  const uint32_t* held_item, const double* held_w, uint32_t N, uint32_t* rank, cf_rank_user* users,
                  cf_rank_summary* summary) {
    const std::string fn = name;
    CF_TRY(panel_check_head(ctx, fn, N, excl_off, excl_item));
    if (!held_off) return cf_set_error(ctx, CF_EINVAL, fn + ": held-out offsets are null");
    if (excl_off && n_users) CF_TRY(check_csr(ctx, name, "exclusion", n_users, excl_off, excl_item, n_items));
    CF_TRY(check_csr(ctx, name, "held-out", n_users, held_off, held_item, n_items, true));
    const uint64_t n_held = held_off[n_users];
    if ((n_users && !users) || (n_held && !rank)) return cf_set_error(ctx, CF_EINVAL, fn + ": null argument");
    if (summary) *summary = cf_rank_summary{};
    for (uint32_t u = 0; u < n_users; ++u) users[u] = cf_rank_user{};
    if (n_held == 0) return CF_OK;   // no users and no items are among these: an edge needs both
    if (!src.valid()) return cf_set_error(ctx, CF_EINVAL, fn + ": null argument");
    CF_TRY(set_device(ctx));

    // the evaluated users in ascending index: their held-out edges are the CSR's, in its order
    std::vector<uint32_t> sel;
    for (uint32_t u = 0; u < n_users; ++u)
        if (held_off[u + 1] > held_off[u]) sel.push_back(u);
    const uint32_t n_eval = (uint32_t)sel.size();
    std::vector<uint64_t> hoff((size_t)n_eval + 1, 0);
    for (uint32_t j = 0; j < n_eval; ++j) hoff[j + 1] = held_off[sel[j] + 1];

    PanelBlocks pb{ctx, fn, src, n_users, n_items, excl_off, excl_item, n_eval, sel.data()};
    uint64_t* d_held_off = nullptr;
    uint32_t* d_held_item = nullptr;
    uint32_t* d_rank = nullptr;    // of every held-out edge
    uint32_t* d_ncand = nullptr;   // of one block
    unsigned long long* d_nan_held = nullptr;
    CF_TRY(pb.begin([&](Carver& c) {
        d_held_off = c.take<uint64_t>(hoff.size());
        d_held_item = c.take<uint32_t>(n_held);
        d_rank = c.take<uint32_t>(n_held);
        d_ncand = c.take<uint32_t>(pb.ub);
        d_nan_held = c.take<unsigned long long>(1);
    }));
    CF_HIP_CHECK(ctx, hipMemcpy(d_held_off, hoff.data(), sizeof(uint64_t) * hoff.size(), hipMemcpyHostToDevice));
    CF_HIP_CHECK(ctx, hipMemcpy(d_held_item, held_item, sizeof(uint32_t) * n_held, hipMemcpyHostToDevice));
    CF_HIP_CHECK(ctx, hipMemset(d_nan_held, 0, sizeof(unsigned long long)));
    std::vector<uint32_t> n_cand(n_eval);
    CF_TRY(pb.run(
        [&](uint32_t b0, uint32_t nb) {
            hipLaunchKernelGGL(rank_count_kernel, dim3(nb), dim3(kAT), 0, pb.st, (const uint64_t*)pb.d_panel, n_items,
                               (const uint64_t*)d_held_off, (const uint32_t*)d_held_item, b0, d_rank, d_ncand, d_nan_held);
        },
        [&](uint32_t b0, uint32_t nb) {
            CF_HIP_CHECK(ctx, hipMemcpy(rank + hoff[b0], d_rank + hoff[b0], sizeof(uint32_t) * (hoff[b0 + nb] - hoff[b0]),
                                        hipMemcpyDeviceToHost));
            CF_HIP_CHECK(ctx, hipMemcpy(n_cand.data() + b0, d_ncand, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost));
            return (int)CF_OK;
        }));
    unsigned long long n_nan_held = 0;
    CF_HIP_CHECK(ctx, hipMemcpy(&n_nan_held, d_nan_held, sizeof(n_nan_held), hipMemcpyDeviceToHost));

    // the metrics: a few flops per edge, from the integers alone, in ascending user index
    cf_rank_summary s{};
    double pr_num = 0.0, pr_den = 0.0;
    std::vector<uint32_t> sorted;
    for (uint32_t j = 0; j < n_eval; ++j) {
        const uint32_t u = sel[j];
        const uint64_t e0 = held_off[u], ne = held_off[u + 1] - e0;
        cf_rank_user& rec = users[u];
        rank_metrics(n_cand[j], rank + e0, held_w ? held_w + e0 : nullptr, ne, N, sorted, &rec, &pr_num, &pr_den);
        s.edges_counted += rec.n_rel;
        s.edges_skipped += ne - rec.n_rel;
        if (rec.n_rel == 0) continue;
        ++s.users_evaluated;
        s.precision += rec.precision;
        s.recall += rec.recall;
        s.ndcg += rec.ndcg;
        s.map += rec.ap;
        s.mrr += rec.rr;
        if (rec.n_cand > rec.n_rel) {
            ++s.users_auc;
            s.auc += rec.auc;
        }
    }
    if (s.users_evaluated) {
        const double n = (double)s.users_evaluated;
        s.precision /= n;
        s.recall /= n;
        s.ndcg /= n;
        s.map /= n;
        s.mrr /= n;
    }
    if (s.users_auc) s.auc /= (double)s.users_auc;
    s.mpr = pr_den != 0.0 ? pr_num / pr_den : 0.0;
    s.n_nan_held = n_nan_held;
    s.blocks = pb.blocks;
    s.score_ms = pb.score_ms;
    s.rank_ms = pb.use_ms;
    if (summary) *summary = s;
    return CF_OK;
}
