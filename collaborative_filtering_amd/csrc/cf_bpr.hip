// cf_bpr.hip -- Bayesian Personalized Ranking (Rendle et al., UAI 2009) on gfx950, fp64 throughout:
// matrix factorization trained on  sum ln sigmoid(x_ui - x_uj)  over (user, rated item, unrated
// item) triples.  include/cf_abi.h has the contract; this is how it is computed.
//
// Once per fit (host): the owner of every user-CSR position p, and ipos, the user-CSR position of
// every item-CSR position.  ipos is the counting-sort transposition of the user CSR; that the
// item CSR holds exactly the users this transposition puts there is the check that the two CSRs
// are each other's transpose with ascending lists.
// Per sweep:
//   1. bpr_sample_kernel: eight lanes per edge, as mf_error_kernel.  Lane t of the group draws
//      candidate t and looks it up in the user's ascending list by binary search; the first lane
//      whose candidate is not in the list gives the negative j.  Then x from the start-of-sweep
//      factors, neg[p] and g[p] = 1 / (1 + exp(x)) are written, and softplus(-x) goes into the
//      block's partial (group g takes edges g, g + 32, .. in order, then a tree; the partials are
//      added by als_error_final_kernel).
//   2. The negative lists: lists_by_key (cf_sort.h: a stable sort of (neg[p], p), then a lower-bound
//      pass) gives a CSR of the triples by negative item, p ascending within an item; skipped edges carry
//      UINT32_MAX and sort past the end.  Its class lists are compacted anew every sweep.
//   3. Three policies of the vertex reduction of cf_mf_reduce.h (its degree classes, LDS partials
//      and HBM segment workspace unchanged):
//        user           walks the user's CSR range; an accepted edge gathers V_i and V_j and adds
//                       g (V_i - V_j); a skipped edge is rejected, adds nothing and moves no other
//        item positive  walks the item's CSR range (mapped to p by ipos), adds g U_u and g, and
//                       parks the sums and the count in a staging buffer
//        item negative  walks the item's range of the negative CSR; every item runs, classed by its
//                       negative count; finish combines with the staged sums
//      All three write pending rows; a vertex with count 0 gets its old row.
//   4. Commit: the pending rows become the rows.
// No floating-point atomic (skipped edges and NaN are counted with integer atomics, one per
// block).  Determinism: the class, the split points and every summation order of a
// vertex depend on the length of the list that is summed only.
//
// A sweep reads about nnz (8 + 3 * 8 D) bytes in the sample kernel, nnz (16 + 2 * 8 D) in the user
// reduction and nnz (16 + 8 D) in each item reduction; the rows V_j and, in the negative
// reduction, U_u are gathered at random addresses.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cf_internal.h"
#include "cf_mf_reduce.h"
#include "cf_sort.h"
#include "cf_splitmix.h"   // splitmix64

namespace {

constexpr uint32_t kSkipped = 0xffffffffu;
static_assert(CF_BPR_TRIES == kG, "one lane of an edge's group per try");

inline uint64_t sweep_key(uint64_t seed, uint32_t sweep) { return splitmix64(splitmix64(seed) ^ (uint64_t)sweep); }

__device__ __forceinline__ bool in_list(const uint32_t* __restrict__ list, uint32_t len, uint32_t c) {
    uint32_t lo = 0, hi = len;   // first position with list[pos] >= c
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (list[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < len && list[lo] == c;
}

// The negative of the edge at rank r of user u (list, len: the user's items).  Called by the
// eight lanes of one group together; lane sl makes try sl.
__device__ __forceinline__ uint32_t draw_negative(uint64_t key_s, uint32_t u, uint32_t r, uint32_t n_items,
                                                  const uint32_t* __restrict__ list, uint32_t len, int lane) {
    const int sl = lane & (kG - 1);
    const uint64_t h = splitmix64(splitmix64(key_s ^ (uint64_t)u) ^ ((uint64_t)r * CF_BPR_TRIES + (uint64_t)sl));
    const uint32_t cand = (uint32_t)(((h >> 32) * (uint64_t)n_items) >> 32);
    const bool free = !in_list(list, len, cand);
    const unsigned mask = (unsigned)(__ballot(free) >> (lane & ~(kG - 1))) & 0xffu;
    const uint32_t first = __shfl(cand, mask ? __ffs(mask) - 1 : 0, kG);
    return mask ? first : kSkipped;
}

// What the kernels see of a fit.
struct BprDev {
    uint64_t nnz;
    uint32_t n_users, n_items;
    int D;
    const uint64_t* uoff;       // user CSR
    const uint32_t* uitem;
    const uint32_t* user_of;    // owner of each user-CSR position
    const uint64_t* ioff;       // item CSR
    const uint32_t* iuser;
    const uint32_t* ipos;       // user-CSR position of each item-CSR position
    double *U, *V, *b;          // b NULL: no bias
    double *Unew, *Vnew, *bnew; // pending
    uint32_t* neg;              // per user-CSR position, kSkipped = no triple this sweep
    double* g;
    uint64_t* noff;             // the negative CSR: offsets, then the positions p (ascending per item)
    uint32_t* npos;
    double* stage;              // per item: D positive sums, the positive sum of g, the positive count
};

__device__ __forceinline__ double softplus(double z) { return fmax(z, 0.0) + log1p(exp(-fabs(z))); }

// GRAD = false is the sampler alone (cf_bpr_sample).  counters: [0] skipped edges, [1] NaN x.
template <bool GRAD>
__global__ __launch_bounds__(kAT) void bpr_sample_kernel(BprDev f, uint64_t key_s, double* partial,
                                                        unsigned long long* counters) {
    __shared__ double s_v[GRAD ? kAT : 1];
    __shared__ uint32_t s_c[kWaves][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = threadIdx.x / kG, sl = threadIdx.x & (kG - 1);
    const uint64_t e0 = (uint64_t)blockIdx.x * kErrPerBlock;
    const int D = f.D;
    double acc = 0.0;
    uint32_t skipped = 0, nan = 0;
    for (int k = 0; k < kErrPerBlock / (kAT / kG); ++k) {
        const uint64_t e = e0 + (uint64_t)k * (kAT / kG) + grp;
        if (e >= f.nnz) break;   // per group
        const uint32_t u = f.user_of[e];
        const uint64_t b = f.uoff[u];
        const uint32_t len = (uint32_t)(f.uoff[u + 1] - b);
        const uint32_t j = draw_negative(key_s, u, (uint32_t)(e - b), f.n_items, f.uitem + b, len, lane);
        if (sl == 0) f.neg[e] = j;
        if (j == kSkipped) {
            skipped += sl == 0;
            continue;
        }
        if constexpr (GRAD) {
            const uint32_t i = f.uitem[e];
            const double* __restrict__ pu = f.U + (size_t)u * D;
            const double* __restrict__ vi = f.V + (size_t)i * D;
            const double* __restrict__ vj = f.V + (size_t)j * D;
            double s = 0.0;
            for (int d = sl; d < D; d += kG) s = fma(pu[d], vi[d] - vj[d], s);
#pragma unroll
            for (int o = kG / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o, kG);
            const double x = f.b ? s + (f.b[i] - f.b[j]) : s;
            if (x != x) nan += sl == 0;
            if (sl == 0) f.g[e] = 1.0 / (1.0 + exp(x));
            acc += softplus(-x);
        }
    }
    if constexpr (GRAD) {
        s_v[threadIdx.x] = sl == 0 ? acc : 0.0;
        block_tree_sum(s_v);
        if (threadIdx.x == 0) partial[blockIdx.x] = s_v[0];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        skipped += __shfl_xor(skipped, o);
        nan += __shfl_xor(nan, o);
    }
    if (lane == 0) {
        s_c[wave][0] = skipped;
        s_c[wave][1] = nan;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t t = 0;
        for (int w = 0; w < kWaves; ++w) t += s_c[w][threadIdx.x];
        if (t) atomicAdd(&counters[threadIdx.x], (unsigned long long)t);
    }
}

__global__ __launch_bounds__(kAT) void bpr_commit_kernel(double* __restrict__ dst, const double* __restrict__ src,
                                                        uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kAT + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// The step of one component from its sum: old + lr (sum / c - reg old); c = 0 keeps old.
__device__ __forceinline__ double bpr_step(double old, double sum, double c, double lr, double reg) {
    return c > 0.0 ? old + lr * (sum / c - reg * old) : old;
}

// ---- the three policies of cf_mf_reduce.h ----------------------------------------------------

struct BprUserOp {
    static constexpr int NS = 0;
    static constexpr bool kCountNan = false;
    BprDev f;
    double lr, reg;
    template <int NJ>
    struct Own {
        double row[NJ];
    };
    __host__ __device__ int dim() const { return f.D; }
    __device__ __forceinline__ uint64_t begin(uint32_t v) const { return f.uoff[v]; }
    __device__ __forceinline__ uint64_t end(uint32_t v) const { return f.uoff[v + 1]; }
    template <int NJ>
    __device__ __forceinline__ void load_own(Own<NJ>& own, uint32_t v, int sl) const {
        load_row<NJ>(own.row, f.U + (size_t)v * f.D, f.D, sl);
    }
    template <int NJ>
    __device__ __forceinline__ void edge(Acc<NJ, NS>& acc, const Own<NJ>&, uint64_t e, int sl) const {
        const uint32_t j = f.neg[e];
        if (j == kSkipped) return;
        const double gp = f.g[e];
        double vi[NJ], vj[NJ];
        load_row<NJ>(vi, f.V + (size_t)f.uitem[e] * f.D, f.D, sl);
        load_row<NJ>(vj, f.V + (size_t)j * f.D, f.D, sl);
#pragma unroll
        for (int k = 0; k < NJ; ++k) acc.s[k] = fma(gp, vi[k] - vj[k], acc.s[k]);
        acc.cnt += 1;
    }
    __device__ __forceinline__ void finish_elem(uint32_t v, int d, double sum, const double*, double cnt) const {
        const size_t at = (size_t)v * f.D + d;
        f.Unew[at] = bpr_step(f.U[at], sum, cnt, lr, reg);
    }
    template <int NJ>
    __device__ __forceinline__ void finish_elem_own(const Own<NJ>& own, int jj, uint32_t v, int d, double sum,
                                                    const double*, double cnt) const {
        f.Unew[(size_t)v * f.D + d] = bpr_step(own.row[jj], sum, cnt, lr, reg);
    }
    __device__ __forceinline__ void finish_scalar(uint32_t, const double*, double, unsigned long long*) const {}
    template <int NJ>
    __device__ __forceinline__ void finish_scalar_own(const Own<NJ>&, uint32_t, const double*, double,
                                                      unsigned long long*) const {}
};

// Item side, the triples in which the item is the positive: sums and count into f.stage.
struct BprPosOp {
    static constexpr int NS = 1;
    static constexpr bool kCountNan = false;
    BprDev f;
    template <int NJ>
    struct Own {};
    __host__ __device__ int dim() const { return f.D; }
    __device__ __forceinline__ uint64_t begin(uint32_t v) const { return f.ioff[v]; }
    __device__ __forceinline__ uint64_t end(uint32_t v) const { return f.ioff[v + 1]; }
    template <int NJ>
    __device__ __forceinline__ void load_own(Own<NJ>&, uint32_t, int) const {}
    template <int NJ>
    __device__ __forceinline__ void edge(Acc<NJ, NS>& acc, const Own<NJ>&, uint64_t q, int sl) const {
        const uint32_t p = f.ipos[q];
        if (f.neg[p] == kSkipped) return;
        const double gp = f.g[p];
        double x[NJ];
        load_row<NJ>(x, f.U + (size_t)f.iuser[q] * f.D, f.D, sl);
#pragma unroll
        for (int k = 0; k < NJ; ++k) acc.s[k] = fma(gp, x[k], acc.s[k]);
        acc.x[0] += gp;
        acc.cnt += 1;
    }
    __device__ __forceinline__ void finish_elem(uint32_t v, int d, double sum, const double*, double) const {
        f.stage[(size_t)v * (f.D + 2) + d] = sum;
    }
    template <int NJ>
    __device__ __forceinline__ void finish_elem_own(const Own<NJ>&, int, uint32_t v, int d, double sum, const double* x,
                                                    double cnt) const {
        finish_elem(v, d, sum, x, cnt);
    }
    __device__ __forceinline__ void finish_scalar(uint32_t v, const double* x, double cnt, unsigned long long*) const {
        f.stage[(size_t)v * (f.D + 2) + f.D] = x[0];
        f.stage[(size_t)v * (f.D + 2) + f.D + 1] = cnt;
    }
    template <int NJ>
    __device__ __forceinline__ void finish_scalar_own(const Own<NJ>&, uint32_t v, const double* x, double cnt,
                                                      unsigned long long* counters) const {
        finish_scalar(v, x, cnt, counters);
    }
};

// Item side, the triples in which the item is the negative; finish combines with the staged
// positive sums and writes the pending row and bias.
struct BprNegOp {
    static constexpr int NS = 1;
    static constexpr bool kCountNan = false;
    BprDev f;
    double lr, reg_item, reg_bias;
    template <int NJ>
    struct Own {
        double row[NJ];
    };
    __host__ __device__ int dim() const { return f.D; }
    __device__ __forceinline__ uint64_t begin(uint32_t v) const { return f.noff[v]; }
    __device__ __forceinline__ uint64_t end(uint32_t v) const { return f.noff[v + 1]; }
    template <int NJ>
    __device__ __forceinline__ void load_own(Own<NJ>& own, uint32_t v, int sl) const {
        load_row<NJ>(own.row, f.V + (size_t)v * f.D, f.D, sl);
    }
    template <int NJ>
    __device__ __forceinline__ void edge(Acc<NJ, NS>& acc, const Own<NJ>&, uint64_t k, int sl) const {
        const uint32_t p = f.npos[k];
        const double gp = f.g[p];
        double x[NJ];
        load_row<NJ>(x, f.U + (size_t)f.user_of[p] * f.D, f.D, sl);
#pragma unroll
        for (int t = 0; t < NJ; ++t) acc.s[t] = fma(gp, x[t], acc.s[t]);
        acc.x[0] += gp;
        acc.cnt += 1;
    }
    __device__ __forceinline__ void put(uint32_t v, int d, double old, double sum, double cnt) const {
        const double* st = f.stage + (size_t)v * (f.D + 2);
        f.Vnew[(size_t)v * f.D + d] = bpr_step(old, st[d] - sum, st[f.D + 1] + cnt, lr, reg_item);
    }
    __device__ __forceinline__ void finish_elem(uint32_t v, int d, double sum, const double*, double cnt) const {
        put(v, d, f.V[(size_t)v * f.D + d], sum, cnt);
    }
    template <int NJ>
    __device__ __forceinline__ void finish_elem_own(const Own<NJ>& own, int jj, uint32_t v, int d, double sum,
                                                    const double*, double cnt) const {
        put(v, d, own.row[jj], sum, cnt);
    }
    __device__ __forceinline__ void finish_scalar(uint32_t v, const double* x, double cnt, unsigned long long*) const {
        if (!f.b) return;
        const double* st = f.stage + (size_t)v * (f.D + 2);
        f.bnew[v] = bpr_step(f.b[v], st[f.D] - x[0], st[f.D + 1] + cnt, lr, reg_bias);
    }
    template <int NJ>
    __device__ __forceinline__ void finish_scalar_own(const Own<NJ>&, uint32_t v, const double* x, double cnt,
                                                      unsigned long long* counters) const {
        finish_scalar(v, x, cnt, counters);
    }
};

// ---- host ---------------------------------------------------------------------------------

// What als_compact_kernel needs of a side: every vertex is flagged before each compaction.
struct BprSide {
    uint32_t n;
    const uint64_t* off;
    uint8_t* flag;
    uint8_t* active;
};

struct BprLayout {
    BprDev f;
    BprSide side[3];     // users, items by their positives, items by their negatives
    AlsLists lists[3];
    uint32_t* iota;      // 0 .. nnz-1, the values of the sort
    uint32_t* nkey;      // the sorted negatives
    void* sort_tmp;
    double* ws;          // segment partials
    double* partial;     // loss block partials
    double* loss;
    unsigned long long* counters;
};

// A negative list above kSeg entries has fewer than 2 len / kSeg segments.
inline uint64_t negative_segments(uint64_t nnz) { return 2 * nnz / kSeg + 1; }

void carve_bpr(Carver& c, BprLayout& L, uint32_t nu, uint32_t ni, uint64_t nnz, int D, bool bias, const uint64_t segs[3],
               size_t sort_bytes) {
    BprDev& f = L.f;
    f.nnz = nnz;
    f.n_users = nu;
    f.n_items = ni;
    f.D = D;
    f.uoff = c.take<uint64_t>((size_t)nu + 1);
    f.uitem = c.take<uint32_t>(nnz);
    f.user_of = c.take<uint32_t>(nnz);
    f.ioff = c.take<uint64_t>((size_t)ni + 1);
    f.iuser = c.take<uint32_t>(nnz);
    f.ipos = c.take<uint32_t>(nnz);
    f.U = c.take<double>((size_t)nu * D);
    f.Unew = c.take<double>((size_t)nu * D);
    f.V = c.take<double>((size_t)ni * D);
    f.Vnew = c.take<double>((size_t)ni * D);
    f.b = bias ? c.take<double>(ni) : nullptr;
    f.bnew = bias ? c.take<double>(ni) : nullptr;
    f.neg = c.take<uint32_t>(nnz);
    f.g = c.take<double>(nnz);
    f.noff = c.take<uint64_t>((size_t)ni + 1);
    f.npos = c.take<uint32_t>(nnz);
    f.stage = c.take<double>((size_t)ni * (D + 2));
    const uint32_t n[3] = {nu, ni, ni};
    const uint64_t* off[3] = {f.uoff, f.ioff, f.noff};
    for (int k = 0; k < 3; ++k) {
        L.side[k] = BprSide{n[k], off[k], c.take<uint8_t>(n[k]), c.take<uint8_t>(n[k])};
        carve_lists(c, L.lists[k], n[k], segs[k]);
    }
    L.iota = c.take<uint32_t>(nnz);
    L.nkey = c.take<uint32_t>(nnz);
    L.sort_tmp = c.take<char>(sort_bytes);
    L.ws = c.take<double>((size_t)std::max({segs[0], segs[1], segs[2]}) * (D + 2));
    L.partial = c.take<double>(error_blocks(nnz));
    L.loss = c.take<double>(1);
    L.counters = c.take<unsigned long long>(2);
}

// The user CSR of both entry points (check_csr's two halves) with BPR's own limits between them.
int check_user_lists(cf_ctx* ctx, const char* fn, uint32_t n_users, uint32_t n_items, const uint64_t* user_off,
                     const uint32_t* user_item, uint64_t* nnz_out) {
    const std::string f(fn);
    if (n_users) CF_TRY(check_csr_shape(ctx, fn, "user", n_users, user_off, user_item));
    const uint64_t nnz = n_users ? user_off[n_users] : 0;
    if (n_items == kSkipped) return cf_set_error(ctx, CF_ERANGE, f + ": 2^32 - 1 items");
    if (nnz >= (1ull << 31)) return cf_set_error(ctx, CF_ERANGE, f + ": 2^31 or more edges");
    if (n_users) CF_TRY(check_csr_index(ctx, fn, "user", n_users, user_off, user_item, n_items, true));
    *nnz_out = nnz;
    return CF_OK;
}

// ipos by transposing the user CSR; CF_EINVAL unless the item CSR is that transpose (which makes
// its lists strictly ascending too).
int transpose_positions(cf_ctx* ctx, const char* fn, uint32_t n_users, uint32_t n_items, const uint64_t* user_off,
                        const uint32_t* user_item, const uint64_t* item_off, const uint32_t* item_user,
                        std::vector<uint32_t>& ipos) {
    const std::string f(fn);
    const uint64_t nnz = n_users ? user_off[n_users] : 0;
    if (n_items && !item_off) return cf_set_error(ctx, CF_EINVAL, f + ": null argument");
    if ((n_items ? item_off[n_items] : 0) != nnz)
        return cf_set_error(ctx, CF_EINVAL, f + ": the two CSRs hold different edge counts");
    if (nnz == 0) return CF_OK;
    if (!item_user) return cf_set_error(ctx, CF_EINVAL, f + ": null edge array");
    CF_TRY(check_csr(ctx, fn, "item", n_items, item_off, item_user, n_users));
    if (!transpose_counts_agree(n_users, user_off, user_item, n_items, item_off))
        return cf_set_error(ctx, CF_EINVAL, f + ": the per-vertex edge counts of the user CSR and the item CSR disagree");
    ipos.resize(nnz);
    std::vector<uint64_t> fill(item_off, item_off + n_items);
    for (uint32_t u = 0; u < n_users; ++u)
        for (uint64_t p = user_off[u]; p < user_off[u + 1]; ++p) {
            const uint64_t q = fill[user_item[p]]++;
            if (item_user[q] != u)
                return cf_set_error(ctx, CF_EINVAL,
                                    f + ": the item CSR is not the transpose of the user CSR with ascending lists");
            ipos[q] = (uint32_t)p;
        }
    return CF_OK;
}

template <class T>
int upload(cf_ctx* ctx, const T* dst, const T* src, size_t n) {
    if (n) CF_HIP_CHECK(ctx, hipMemcpy((void*)dst, src, sizeof(T) * n, hipMemcpyHostToDevice));
    return CF_OK;
}

void launch_copy(double* dst, const double* src, uint64_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(bpr_commit_kernel, dim3(blocks_for(n)), dim3(kAT), 0, st, dst, src, n);
}

// All of a side's vertices into its class lists, by the lengths of s.off.
void launch_classes(const BprSide& s, const AlsLists& lists, hipStream_t st) {
    if (s.n) (void)hipMemsetAsync(s.flag, 1, s.n, st);
    launch_compact(s, lists, st);
}

}  // namespace

extern "C" int cf_debug_bpr_tries(void) { return CF_BPR_TRIES; }

extern "C" int cf_bpr_timing(cf_ctx* ctx, float ms[6]) {
    if (!ctx) return CF_EINVAL;
    if (!ms) return cf_set_error(ctx, CF_EINVAL, "cf_bpr_timing: null result");
    for (int k = 0; k < 6; ++k) ms[k] = ctx->bpr_ms[k];
    return CF_OK;
}

extern "C" int cf_bpr_sample(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, const uint64_t* user_off,
                             const uint32_t* user_item, uint64_t seed, uint32_t sweep, uint32_t* neg,
                             uint64_t* n_skipped) {
    if (!ctx) return CF_EINVAL;
    if (n_skipped) *n_skipped = 0;
    uint64_t nnz = 0;
    CF_TRY(check_user_lists(ctx, "cf_bpr_sample", n_users, n_items, user_off, user_item, &nnz));
    if (nnz == 0) return CF_OK;
    if (!neg) return cf_set_error(ctx, CF_EINVAL, "cf_bpr_sample: null result");
    CF_TRY(set_device(ctx));
    BprDev f{};
    unsigned long long* counters = nullptr;
    CF_TRY(carve_workspace(ctx, [&](Carver& c) {
        f.uoff = c.take<uint64_t>((size_t)n_users + 1);
        f.uitem = c.take<uint32_t>(nnz);
        f.user_of = c.take<uint32_t>(nnz);
        f.neg = c.take<uint32_t>(nnz);
        counters = c.take<unsigned long long>(2);
    }));
    f.nnz = nnz;
    f.n_users = n_users;
    f.n_items = n_items;
    CF_TRY(upload(ctx, f.uoff, user_off, (size_t)n_users + 1));
    CF_TRY(upload(ctx, f.uitem, user_item, nnz));
    CF_TRY(upload_edge_owners(ctx, (uint32_t*)f.user_of, n_users, user_off, nnz));
    CF_HIP_CHECK(ctx, hipMemset(counters, 0, 2 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(bpr_sample_kernel<false>, dim3((unsigned)error_blocks(nnz)), dim3(kAT), 0, nullptr, f,
                       sweep_key(seed, sweep), (double*)nullptr, counters);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(neg, f.neg, sizeof(uint32_t) * nnz, hipMemcpyDeviceToHost));
    unsigned long long h[2] = {0, 0};
    CF_HIP_CHECK(ctx, hipMemcpy(h, counters, sizeof(h), hipMemcpyDeviceToHost));
    if (n_skipped) *n_skipped = h[0];
    return CF_OK;
}

extern "C" int cf_bpr_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                          const uint32_t* user_item, const uint64_t* item_off, const uint32_t* item_user,
                          const cf_bpr_params* params, double* U, double* V, double* bias_item, double* loss_trace,
                          cf_bpr_stats* stats) {
    if (!ctx) return CF_EINVAL;
    if (stats) *stats = cf_bpr_stats{};
    if (!params) return cf_set_error(ctx, CF_EINVAL, "cf_bpr_fit: null params");
    if (D == 0) return cf_set_error(ctx, CF_EINVAL, "cf_bpr_fit: D = 0");
    if (D > CF_ALS_MAX_D) return cf_set_error(ctx, CF_ERANGE, "cf_bpr_fit: D above CF_ALS_MAX_D");
    const cf_bpr_params& par = *params;
    if (!std::isfinite(par.lr)) return cf_set_error(ctx, CF_EINVAL, "cf_bpr_fit: lr is not finite");
    for (double reg : {par.reg_user, par.reg_item, par.reg_bias})
        if (!std::isfinite(reg) || reg < 0.0)
            return cf_set_error(ctx, CF_EINVAL, "cf_bpr_fit: a regularization weight that is negative or not finite");
    uint64_t nnz = 0;
    CF_TRY(check_user_lists(ctx, "cf_bpr_fit", n_users, n_items, user_off, user_item, &nnz));
    std::vector<uint32_t> ipos;
    CF_TRY(transpose_positions(ctx, "cf_bpr_fit", n_users, n_items, user_off, user_item, item_off, item_user, ipos));
    if ((n_users && !U) || (n_items && !V)) return cf_set_error(ctx, CF_EINVAL, "cf_bpr_fit: null argument");
    const uint32_t n_sweeps = par.n_sweeps;
    if (n_sweeps > (1u << 24)) return cf_set_error(ctx, CF_ERANGE, "cf_bpr_fit: more than 2^24 sweeps");
    if ((uint64_t)par.first_sweep + n_sweeps > 0xffffffffull)
        return cf_set_error(ctx, CF_ERANGE, "cf_bpr_fit: sweep index above 2^32");
    if (loss_trace) std::fill(loss_trace, loss_trace + 2 * (size_t)n_sweeps, 0.0);
    for (float& t : ctx->bpr_ms) t = 0.0f;
    if (n_sweeps == 0) return CF_OK;
    if (nnz == 0) {   // no triple in any sweep: nothing moves
        if (stats) stats->sweeps = n_sweeps;
        return CF_OK;
    }
    CF_TRY(set_device(ctx));

    // everything the fit needs exists before its first launch
    const uint64_t segs[3] = {total_segments(n_users, user_off), total_segments(n_items, item_off), negative_segments(nnz)};
    if (std::max({segs[0], segs[1], segs[2]}) > 0xffffffffull)
        return cf_set_error(ctx, CF_ERANGE, "cf_bpr_fit: too many segments");
    hipStream_t st = nullptr;
    size_t sort_bytes = 0;
    CF_HIP_CHECK(ctx, lists_by_key(nullptr, sort_bytes, nullptr, nullptr, nullptr, false, nullptr, nnz, n_items, nullptr, 32, st));
    const bool bias = bias_item != nullptr;
    BprLayout L{};
    CF_TRY(carve_workspace(ctx, [&](Carver& c) { carve_bpr(c, L, n_users, n_items, nnz, (int)D, bias, segs, sort_bytes); }));
    const BprDev& f = L.f;
    MfEvents<8> evs;
    for (hipEvent_t& e : evs.e) CF_HIP_CHECK(ctx, hipEventCreate(&e));

    CF_TRY(upload(ctx, f.uoff, user_off, (size_t)n_users + 1));
    CF_TRY(upload(ctx, f.uitem, user_item, nnz));
    CF_TRY(upload_edge_owners(ctx, (uint32_t*)f.user_of, n_users, user_off, nnz));
    CF_TRY(upload(ctx, f.ioff, item_off, (size_t)n_items + 1));
    CF_TRY(upload(ctx, f.iuser, item_user, nnz));
    CF_TRY(upload(ctx, f.ipos, (const uint32_t*)ipos.data(), nnz));
    CF_TRY(upload(ctx, (const double*)f.U, (const double*)U, (size_t)n_users * D));
    CF_TRY(upload(ctx, (const double*)f.V, (const double*)V, (size_t)n_items * D));
    if (bias) CF_TRY(upload(ctx, (const double*)f.b, (const double*)bias_item, n_items));
    for (int k = 0; k < 3; ++k) CF_HIP_CHECK(ctx, hipMemset(L.side[k].active, 0, L.side[k].n));
    hipLaunchKernelGGL(iota_kernel<uint32_t>, dim3(blocks_for(nnz)), dim3(kAT), 0, st, L.iota, nnz);   // once for every sweep

    // the users and the items by their positives: classed once per fit
    uint32_t rec[3][4];
    for (int k = 0; k < 2; ++k) {
        launch_classes(L.side[k], L.lists[k], st);
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(rec[k], L.lists[k].record, sizeof(rec[k]), hipMemcpyDeviceToHost));
        if (rec[k][3] > segs[k]) return cf_set_error(ctx, CF_EHIP, "cf_bpr_fit: segment list overflow");
    }

    const BprUserOp user_op{f, par.lr, par.reg_user};
    const BprPosOp pos_op{f};
    const BprNegOp neg_op{f, par.lr, par.reg_item, par.reg_bias};
    const unsigned blocks = (unsigned)error_blocks(nnz);
    double ms[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint64_t triples = 0, skipped = 0, n_nan = 0;
    uint32_t sweeps = 0;
    while (sweeps < n_sweeps) {
        // 1. negatives, g and the loss of the start-of-sweep factors
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
        CF_HIP_CHECK(ctx, hipMemsetAsync(L.counters, 0, 2 * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(bpr_sample_kernel<true>, dim3(blocks), dim3(kAT), 0, st, f,
                           sweep_key(par.seed, par.first_sweep + sweeps), L.partial, L.counters);
        hipLaunchKernelGGL(als_error_final_kernel, dim3(1), dim3(kAT), 0, st, (const double*)L.partial, (uint64_t)blocks,
                           L.loss);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
        // 2. the negative CSR and its class lists
        size_t tb = sort_bytes;
        // all 32 bits: skipped edges carry kSkipped and sort past noff[n_items]
        CF_HIP_CHECK(ctx, lists_by_key(L.sort_tmp, tb, f.neg, L.nkey, L.iota, false, f.npos, nnz, n_items, f.noff, 32, st));
        launch_classes(L.side[2], L.lists[2], st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[2], st));
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(rec[2], L.lists[2].record, sizeof(rec[2]), hipMemcpyDeviceToHost));   // waits
        if (rec[2][3] > segs[2]) return cf_set_error(ctx, CF_EHIP, "cf_bpr_fit: segment list overflow");
        // 3. the three reductions, all from the start-of-sweep factors
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[3], st));
        launch_reduce(user_op, L.lists[0], rec[0], L.ws, L.counters, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[4], st));
        launch_reduce(pos_op, L.lists[1], rec[1], L.ws, L.counters, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[5], st));
        launch_reduce(neg_op, L.lists[2], rec[2], L.ws, L.counters, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[6], st));
        // 4. commit
        launch_copy(f.U, f.Unew, (uint64_t)n_users * D, st);
        launch_copy(f.V, f.Vnew, (uint64_t)n_items * D, st);
        if (bias) launch_copy(f.b, f.bnew, n_items, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[7], st));
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipEventSynchronize(evs.e[7]));
        unsigned long long h[2] = {0, 0};
        double loss = 0.0;
        CF_HIP_CHECK(ctx, hipMemcpy(h, L.counters, sizeof(h), hipMemcpyDeviceToHost));
        CF_HIP_CHECK(ctx, hipMemcpy(&loss, L.loss, sizeof(double), hipMemcpyDeviceToHost));
        if (loss_trace) {
            loss_trace[2 * (size_t)sweeps] = loss;
            loss_trace[2 * (size_t)sweeps + 1] = (double)(nnz - h[0]);
        }
        triples += nnz - h[0];
        skipped += h[0];
        n_nan += h[1];
        ms[0] += elapsed(evs.e[0], evs.e[1]);
        ms[1] += elapsed(evs.e[1], evs.e[2]);
        for (int k = 0; k < 4; ++k) ms[2 + k] += elapsed(evs.e[3 + k], evs.e[4 + k]);
        ++sweeps;
        if (h[1]) break;   // numeric errors: the caller reports them
    }
    CF_HIP_CHECK(ctx, hipDeviceSynchronize());
    CF_HIP_CHECK(ctx, hipMemcpy(U, f.U, sizeof(double) * (size_t)n_users * D, hipMemcpyDeviceToHost));
    CF_HIP_CHECK(ctx, hipMemcpy(V, f.V, sizeof(double) * (size_t)n_items * D, hipMemcpyDeviceToHost));
    if (bias) CF_HIP_CHECK(ctx, hipMemcpy(bias_item, f.b, sizeof(double) * n_items, hipMemcpyDeviceToHost));
    for (int k = 0; k < 6; ++k) ctx->bpr_ms[k] = (float)ms[k];
    if (stats) {
        stats->sweeps = sweeps;
        stats->triples = triples;
        stats->n_skipped = skipped;
        stats->n_nan = n_nan;
        stats->sample_ms = (float)ms[0];
        stats->reduce_ms = (float)(ms[1] + ms[2] + ms[3] + ms[4]);
        stats->apply_ms = (float)ms[5];
    }
    return CF_OK;
}
