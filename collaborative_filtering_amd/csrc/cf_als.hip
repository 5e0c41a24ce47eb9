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
// Work is shaped by the vertex's TRAIN degree, with cuts that are constants of this file:
//   low   deg <= kLowMax           one wave per vertex, kWaves vertices per workgroup
//   mid   kLowMax < deg <= kSeg    one workgroup per vertex: its waves take contiguous quarters
//                                  of the list, the partial (A, b) are summed in wave order in LDS
//   high  deg > kSeg               the list is cut into segments of kSeg edges; one workgroup per
//                                  segment (as mid) writes its partial to an HBM workspace, and a
//                                  wave per vertex sums the partials in segment order and solves
// Determinism rule: the class, the split points and every summation order of a vertex depend on
// its own degree only -- never on the launch, the active list or other vertices -- and there is
// no floating-point atomic, so a vertex's new factor is the same bits whichever other vertices
// are active and however often a fit is repeated.
//
// The Gram of one wave: D is padded to DP = 8 / 16 / 32 / 64 and lane l owns the TS x TS block
// (TS = DP / 8) at block row l >> 3, block column l & 7 of A, in registers; neighbour rows are
// staged kBatch at a time (coalesced) in wave-private LDS and every lane reads its 2 TS values
// per neighbour from there.  Each element is one fma chain in CSR order.
// The solve is an unpivoted LDL^T of the packed lower triangle (= the upper triangle the
// reference factors, als.cpp:330) with b carried as a border row (the layout of cf_ldlt.hpp),
// done by one wave in LDS for D <= 64.  An exactly zero pivot is skipped as cf_ldlt.hpp
// documents; pivots <= 0 (or NaN) are counted (n_not_pd).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cf_internal.h"
#include "cf_ldlt.hpp"

namespace {

constexpr int kAT = 256;               // threads per workgroup
constexpr int kWaves = kAT / 64;
constexpr int kBatch = 16;             // neighbour rows staged per wave at a time
constexpr int kLowMax = 64;            // low / mid cut (TRAIN degree)
constexpr int kSeg = 2048;             // mid / high cut and the segment length
constexpr int kG = 8;                  // lanes per edge of the dot-product kernels
constexpr int kVPT = 4;                // vertices per thread of the compaction kernels
constexpr int kCompBlock = kAT * kVPT;
constexpr int kErrPerBlock = (kAT / kG) * 8;   // edges per block of the error kernel

__host__ __device__ constexpr int sys_len(int D) { return (D + 1) * (D + 2) / 2; }   // packed rows 0..D

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

// The compacted active lists of the side being updated (ascending vertex order).
struct AlsLists {
    uint32_t* low;
    uint32_t* mid;
    uint32_t* high;
    uint32_t* high_base;   // first workspace slot (= index into seg_*) of each high vertex
    uint32_t* seg_vertex;  // one entry per (high vertex, segment)
    uint32_t* seg_index;
    uint32_t* block_cnt;   // 4 counters per compaction block, then their exclusive scan
    uint32_t* record;      // {low, mid, high, segments} of the last compaction
};

template <int DP>
struct Gram {
    static constexpr int TS = DP / 8;
    double a[TS][TS];
    double b[TS];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int x = 0; x < TS; ++x) {
            b[x] = 0.0;
#pragma unroll
            for (int y = 0; y < TS; ++y) a[x][y] = 0.0;
        }
    }
};

// A += sum x x^T, b += sum obs x over the edges [p0, p1) in order; stage: kBatch * DP doubles of
// wave-private LDS.  Called by a whole wave.
template <int DP>
__device__ __forceinline__ void gram_accumulate(Gram<DP>& g, double* stage, const double* __restrict__ Fo, int D,
                                                const uint32_t* __restrict__ nbr, const float* __restrict__ obs,
                                                uint64_t p0, uint64_t p1, int lane) {
    constexpr int TS = DP / 8;
    const int ti = lane >> 3, tj = lane & 7;
    for (uint64_t p = p0; p < p1; p += kBatch) {
        const int nb = (int)(p1 - p < (uint64_t)kBatch ? p1 - p : (uint64_t)kBatch);
#pragma unroll
        for (int r = 0; r < kBatch * DP / 64; ++r) {
            const int t = lane + 64 * r;
            const int k = t / DP, d = t % DP;
            double v = 0.0;
            if (k < nb && d < D) v = Fo[(size_t)nbr[p + k] * D + d];
            stage[t] = v;
        }
        const float ob = lane < nb ? obs[p + lane] : 0.0f;
        WAVE_SYNC();
        for (int k = 0; k < nb; ++k) {
            double xi[TS], xj[TS];
#pragma unroll
            for (int x = 0; x < TS; ++x) {
                xi[x] = stage[k * DP + ti * TS + x];
                xj[x] = stage[k * DP + tj * TS + x];
            }
            const double o = (double)__shfl(ob, k);
#pragma unroll
            for (int x = 0; x < TS; ++x) {
#pragma unroll
                for (int y = 0; y < TS; ++y) g.a[x][y] = fma(xi[x], xj[y], g.a[x][y]);
                g.b[x] = fma(o, xi[x], g.b[x]);
            }
        }
        WAVE_SYNC();
    }
}

// The wave's partial into the packed system S (rows 0..D-1 = lower triangle of A, row D = b).
template <int DP, bool ADD>
__device__ __forceinline__ void gram_to_system(const Gram<DP>& g, double* S, int D, int lane) {
    constexpr int TS = DP / 8;
    const int ti = lane >> 3, tj = lane & 7;
#pragma unroll
    for (int x = 0; x < TS; ++x) {
        const int i = ti * TS + x;
#pragma unroll
        for (int y = 0; y < TS; ++y) {
            const int q = tj * TS + y;
            if (i < D && q <= i) {
                const int idx = tri(i, q);
                S[idx] = ADD ? S[idx] + g.a[x][y] : g.a[x][y];
            }
        }
        if (tj == 0 && i < D) {
            const int idx = tri(D, i);
            S[idx] = ADD ? S[idx] + g.b[x] : g.b[x];
        }
    }
}

// Unpivoted LDL^T of the D x D system in S with b as the border row D, then L^T x = y: on
// return S[tri(D, d)] = x_d.  One wave; S is LDS.  Returns the number of pivots that are not > 0.
__device__ inline int wave_ldlt_solve(double* S, int D, double reg, int lane) {
    for (int i = lane; i < D; i += 64) S[tri(i, i)] += reg;
    WAVE_SYNC();
    int not_pd = 0;
    for (int j = 0; j < D; ++j) {
        const double dj = S[tri(j, j)];
        if (!(dj > 0.0)) ++not_pd;
        // trailing update of rows j+1..D with the unscaled column j
        for (int i = j + 1 + lane; i <= D; i += 64) {
            const double w = S[tri(i, j)];
            const double lij = dj != 0.0 ? w / dj : 0.0;   // exact-zero pivot: skipped
            const int qe = i < D ? i : D - 1;
            double* Si = S + tri(i, 0);
            for (int q = j + 1; q <= qe; ++q) Si[q] = fma(-lij, S[tri(q, j)], Si[q]);
        }
        WAVE_SYNC();
        for (int i = j + 1 + lane; i <= D; i += 64) {
            const double w = S[tri(i, j)];
            S[tri(i, j)] = dj != 0.0 ? w / dj : 0.0;
        }
        WAVE_SYNC();
    }
    // border row = y = D^-1 L^-1 b; back substitution, column by column
    double* y = S + tri(D, 0);
    for (int i = D - 1; i > 0; --i) {
        const double xi = y[i];
        const double* Li = S + tri(i, 0);
        for (int k = lane; k < i; k += 64) y[k] = fma(-Li[k], xi, y[k]);
        WAVE_SYNC();
    }
    return not_pd;
}

// apply's tail for vertex v with the system in S: solve, residual, store.  One wave.
__device__ inline void wave_apply(double* S, int D, const AlsSide& s, uint32_t v, unsigned long long* not_pd,
                                  int lane) {
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

template <int DP>
constexpr int low_region() {   // doubles of LDS per wave: the staging rows, then the system in their place
    return ((kBatch * DP > sys_len(DP) ? kBatch * DP : sys_len(DP)) + 1) & ~1;
}

// low class: one wave per vertex.
template <int DP>
__global__ __launch_bounds__(kAT) void als_low_kernel(AlsSide s, const double* __restrict__ Fo, int D,
                                                     const uint32_t* __restrict__ list, uint32_t count,
                                                     unsigned long long* not_pd) {
    __shared__ __attribute__((aligned(16))) double lds[kWaves * low_region<DP>()];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t j = blockIdx.x * kWaves + wave;
    if (j >= count) return;   // whole waves leave; no block barrier below
    const uint32_t v = list[j];
    const uint64_t p0 = s.off[v], p1 = s.off[v + 1];
    if (p1 == p0) {   // no TRAIN edge (als.cpp:319)
        if (lane == 0) {
            s.resid[v] = 0.0f;
            s.nupd[v] += 1;
        }
        return;
    }
    double* R = lds + wave * low_region<DP>();
    Gram<DP> g;
    g.clear();
    gram_accumulate<DP>(g, R, Fo, D, s.nbr, s.obs, p0, p1, lane);
    gram_to_system<DP, false>(g, R, D, lane);
    WAVE_SYNC();
    wave_apply(R, D, s, v, not_pd, lane);
}

template <int DP>
constexpr int mid_region() {
    return ((kWaves * kBatch * DP > sys_len(DP) ? kWaves * kBatch * DP : sys_len(DP)) + 1) & ~1;
}

// mid class (SEGMENT = false): one workgroup per vertex, solved here.  high class (SEGMENT =
// true): one workgroup per (vertex, segment); the partial system goes to workspace slot
// blockIdx.x (sys_len(D) doubles per slot).
template <int DP, bool SEGMENT>
__global__ __launch_bounds__(kAT) void als_group_kernel(AlsSide s, const double* __restrict__ Fo, int D,
                                                       const uint32_t* __restrict__ list,
                                                       const uint32_t* __restrict__ seg_index, double* ws,
                                                       unsigned long long* not_pd) {
    __shared__ __attribute__((aligned(16))) double lds[mid_region<DP>()];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t v = list[blockIdx.x];
    uint64_t p0 = s.off[v];
    uint64_t len = s.off[v + 1] - p0;
    if (SEGMENT) {
        const uint64_t first = (uint64_t)seg_index[blockIdx.x] * kSeg;
        p0 += first;
        len = len - first < (uint64_t)kSeg ? len - first : (uint64_t)kSeg;
    }
    const uint64_t chunk = (len + kWaves - 1) / kWaves;
    const uint64_t b = std::min(len, wave * chunk), e = std::min(len, (wave + 1) * chunk);
    Gram<DP> g;
    g.clear();
    gram_accumulate<DP>(g, lds + wave * kBatch * DP, Fo, D, s.nbr, s.obs, p0 + b, p0 + e, lane);
    __syncthreads();   // the staging rows are dead: the system takes their place
    if (wave == 0) gram_to_system<DP, false>(g, lds, D, lane);
    __syncthreads();
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {   // partials summed in wave order
        if (wave == w) gram_to_system<DP, true>(g, lds, D, lane);
        __syncthreads();
    }
    if (SEGMENT) {
        double* slot = ws + (size_t)blockIdx.x * sys_len(D);
        for (int t = threadIdx.x; t < sys_len(D); t += kAT) slot[t] = lds[t];
    } else if (wave == 0) {
        wave_apply(lds, D, s, v, not_pd, lane);
    }
}

// high class, second pass: one wave per vertex sums its segments' partials in segment order.
template <int DP>
__global__ __launch_bounds__(kAT) void als_finish_kernel(AlsSide s, int D, const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ base, uint32_t count,
                                                        const double* __restrict__ ws, unsigned long long* not_pd) {
    __shared__ __attribute__((aligned(16))) double lds[kWaves * ((sys_len(DP) + 1) & ~1)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t j = blockIdx.x * kWaves + wave;
    if (j >= count) return;
    const uint32_t v = list[j];
    const uint64_t deg = s.off[v + 1] - s.off[v];
    const uint32_t nseg = (uint32_t)((deg + kSeg - 1) / kSeg);
    double* S = lds + wave * ((sys_len(DP) + 1) & ~1);
    const int n = sys_len(D);
    const double* slot = ws + (size_t)base[j] * n;
    for (int t = lane; t < n; t += 64) {
        double acc = slot[t];
        for (uint32_t q = 1; q < nseg; ++q) acc += slot[(size_t)q * n + t];
        S[t] = acc;
    }
    WAVE_SYNC();
    wave_apply(S, D, s, v, not_pd, lane);
}

// ---- compaction of one side's flags into the class lists (deterministic scan) ------------

__device__ __forceinline__ int als_class(uint64_t deg) { return deg <= (uint64_t)kLowMax ? 0 : (deg <= (uint64_t)kSeg ? 1 : 2); }

// Exclusive scan of one value per thread over the block (kAT threads); *total = the block sum.
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t* s_wave /* kWaves + 1 */, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();   // s_wave may still be read from the previous call
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t c = s_wave[w];
        if (w < wave) before += c;
        all += c;
    }
    *total = all;
    return before + inc - v;
}

// FILL = false: per-block counters {low, mid, high, segments}.  FILL = true: with their exclusive
// scan in block_cnt, writes the lists, sets active[] and clears flag[].
template <bool FILL>
__global__ __launch_bounds__(kAT) void als_compact_kernel(AlsSide s, AlsLists L) {
    __shared__ uint32_t s_wave[kWaves + 1];
    const uint32_t v0 = (blockIdx.x * (uint32_t)kAT + threadIdx.x) * kVPT;
    uint32_t cnt[4] = {0, 0, 0, 0};
    int cls[kVPT];
    uint32_t nseg[kVPT];
#pragma unroll
    for (int i = 0; i < kVPT; ++i) {
        cls[i] = -1;
        nseg[i] = 0;
        const uint64_t v = (uint64_t)v0 + i;
        if (v < s.n && s.flag[v]) {
            const uint64_t deg = s.off[v + 1] - s.off[v];
            cls[i] = als_class(deg);
            cnt[cls[i]]++;
            if (cls[i] == 2) {
                nseg[i] = (uint32_t)((deg + kSeg - 1) / kSeg);
                cnt[3] += nseg[i];
            }
        }
    }
    uint32_t pre[4], tot[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) pre[c] = block_excl_scan(cnt[c], s_wave, &tot[c]);
    if (!FILL) {
        if (threadIdx.x == 0)
            for (int c = 0; c < 4; ++c) L.block_cnt[(size_t)blockIdx.x * 4 + c] = tot[c];
        return;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) pre[c] += L.block_cnt[(size_t)blockIdx.x * 4 + c];
#pragma unroll
    for (int i = 0; i < kVPT; ++i) {
        const uint64_t v = (uint64_t)v0 + i;
        if (v >= s.n) continue;
        s.active[v] = cls[i] >= 0;
        s.flag[v] = 0;
        if (cls[i] == 0) L.low[pre[0]++] = (uint32_t)v;
        else if (cls[i] == 1) L.mid[pre[1]++] = (uint32_t)v;
        else if (cls[i] == 2) {
            L.high[pre[2]] = (uint32_t)v;
            L.high_base[pre[2]++] = pre[3];
            for (uint32_t q = 0; q < nseg[i]; ++q) {
                L.seg_vertex[pre[3]] = (uint32_t)v;
                L.seg_index[pre[3]++] = q;
            }
        }
    }
}

// Exclusive scan of the per-block counters in block order (one workgroup; counter c by thread c);
// the totals go to the record.
__global__ void als_scan_kernel(AlsLists L, uint32_t n_blocks) {
    const int c = threadIdx.x;
    if (c >= 4) return;
    uint32_t run = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint32_t t = L.block_cnt[(size_t)b * 4 + c];
        L.block_cnt[(size_t)b * 4 + c] = run;
        run += t;
    }
    L.record[c] = run;
}

// ---- dot-product kernels: kG lanes per edge ---------------------------------------------

__device__ __forceinline__ double group_dot(const double* __restrict__ a, const double* __restrict__ b, int D, int sl) {
    double s = 0.0;
    for (int d = sl; d < D; d += kG) s = fma(a[d], b[d], s);
#pragma unroll
    for (int o = kG / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o, kG);
    return s;
}

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

__global__ __launch_bounds__(kAT) void als_predict_kernel(uint64_t n, const uint32_t* __restrict__ user,
                                                         const uint32_t* __restrict__ item, const double* __restrict__ U,
                                                         const double* __restrict__ V, int D, double* pred) {
    const uint64_t e = ((uint64_t)blockIdx.x * kAT + threadIdx.x) / kG;
    const int sl = threadIdx.x & (kG - 1);
    if (e >= n) return;
    const double p = group_dot(U + (size_t)user[e] * D, V + (size_t)item[e] * D, D, sl);
    if (sl == 0) pred[e] = p;
}

// Fixed tree over the block's kAT values in LDS; the result is in v[0].
__device__ inline void block_tree_sum(double* v) {
    for (int o = kAT / 2; o >= 1; o >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < o) v[threadIdx.x] += v[threadIdx.x + o];
    }
    __syncthreads();
}

// error aggregate (als.cpp:424-430), level 1: block b sums the clamped squared errors of edges
// [b kErrPerBlock, (b + 1) kErrPerBlock): group g takes edges g, g + 32, .. in order, then a tree.
__global__ __launch_bounds__(kAT) void als_error_kernel(uint64_t n, const uint32_t* __restrict__ user,
                                                       const uint32_t* __restrict__ item, const float* __restrict__ obs,
                                                       const double* __restrict__ U, const double* __restrict__ V, int D,
                                                       double minval, double maxval, double* partial) {
    __shared__ double s_v[kAT];
    const int grp = threadIdx.x / kG, sl = threadIdx.x & (kG - 1);
    const uint64_t e0 = (uint64_t)blockIdx.x * kErrPerBlock;
    double acc = 0.0;
    for (int r = 0; r < kErrPerBlock / (kAT / kG); ++r) {
        const uint64_t e = e0 + (uint64_t)r * (kAT / kG) + grp;
        if (e >= n) break;   // per group
        double p = group_dot(U + (size_t)user[e] * D, V + (size_t)item[e] * D, D, sl);
        p = fmin(maxval, p);
        p = fmax(minval, p);
        const double d = (double)obs[e] - p;
        acc = fma(d, d, acc);
    }
    s_v[threadIdx.x] = sl == 0 ? acc : 0.0;
    block_tree_sum(s_v);
    if (threadIdx.x == 0) partial[blockIdx.x] = s_v[0];
}

// level 2: one workgroup; thread t sums partials t, t + kAT, .. in order, then the same tree.
__global__ __launch_bounds__(kAT) void als_error_final_kernel(const double* __restrict__ partial, uint64_t n_partial,
                                                             double* out) {
    __shared__ double s_v[kAT];
    double acc = 0.0;
    for (uint64_t i = threadIdx.x; i < n_partial; i += kAT) acc += partial[i];
    s_v[threadIdx.x] = acc;
    block_tree_sum(s_v);
    if (threadIdx.x == 0) *out = s_v[0];
}

// ---- host ---------------------------------------------------------------------------------

// Carves one device allocation (the context's ALS workspace) into aligned arrays.
struct Carver {
    size_t pos = 0;
    char* base = nullptr;
    template <class T>
    T* take(size_t count) {
        const size_t at = pos;
        pos = (pos + sizeof(T) * std::max<size_t>(count, 1) + 255) & ~(size_t)255;
        return base ? reinterpret_cast<T*>(base + at) : nullptr;
    }
};

// The context's ALS workspace with at least `bytes` bytes; grown before any launch of the call.
int als_reserve(cf_ctx* ctx, size_t bytes) {
    if (ctx->als_bytes >= bytes && ctx->d_als) return CF_OK;
    if (ctx->d_als) {
        CF_HIP_CHECK(ctx, hipDeviceSynchronize());
        (void)hipFree(ctx->d_als);
        ctx->d_als = nullptr;
        ctx->als_bytes = 0;
    }
    CF_TRY(cf_malloc_evict(ctx, &ctx->d_als, bytes, "ALS workspace"));
    ctx->als_bytes = bytes;
    return CF_OK;
}

struct FitLayout {
    AlsSide side[2];
    AlsLists lists;
    double* ws;
    unsigned long long* not_pd;
    uint32_t seg_cap;
};

uint64_t total_segments(uint32_t n, const uint64_t* off) {
    uint64_t segs = 0;
    for (uint32_t v = 0; v < n; ++v) {
        const uint64_t deg = off[v + 1] - off[v];
        if (deg > (uint64_t)kSeg) segs += (deg + kSeg - 1) / kSeg;
    }
    return segs;
}

void carve_fit(Carver& c, FitLayout& f, uint32_t n_users, uint32_t n_items, uint64_t nnz, int D, uint64_t seg_cap) {
    const uint32_t n[2] = {n_users, n_items};
    for (int k = 0; k < 2; ++k) {
        AlsSide& s = f.side[k];
        s.n = n[k];
        s.off = c.take<uint64_t>((size_t)n[k] + 1);
        s.nbr = c.take<uint32_t>(nnz);
        s.obs = c.take<float>(nnz);
        s.src = c.take<uint32_t>(nnz);
        s.F = c.take<double>((size_t)n[k] * D);
        s.reg = c.take<double>(n[k]);
        s.nupd = c.take<uint32_t>(n[k]);
        s.resid = c.take<float>(n[k]);
        s.flag = c.take<uint8_t>(n[k]);
        s.active = c.take<uint8_t>(n[k]);
    }
    const size_t nmax = std::max(n_users, n_items);
    f.lists.low = c.take<uint32_t>(nmax);
    f.lists.mid = c.take<uint32_t>(nmax);
    f.lists.high = c.take<uint32_t>(nmax);
    f.lists.high_base = c.take<uint32_t>(nmax);
    f.lists.seg_vertex = c.take<uint32_t>(seg_cap);
    f.lists.seg_index = c.take<uint32_t>(seg_cap);
    f.lists.block_cnt = c.take<uint32_t>(((nmax + kCompBlock - 1) / kCompBlock) * 4);
    f.lists.record = c.take<uint32_t>(4);
    f.ws = c.take<double>((size_t)seg_cap * sys_len(D));
    f.not_pd = c.take<unsigned long long>(1);
    f.seg_cap = (uint32_t)seg_cap;
}

template <int DP>
void launch_update(const FitLayout& f, int k, int D, const uint32_t rec[4], hipStream_t st) {
    const AlsSide& s = f.side[k];
    const double* Fo = f.side[1 - k].F;
    if (rec[0])
        hipLaunchKernelGGL(als_low_kernel<DP>, dim3((rec[0] + kWaves - 1) / kWaves), dim3(kAT), 0, st, s, Fo, D,
                           f.lists.low, rec[0], f.not_pd);
    if (rec[1])
        hipLaunchKernelGGL((als_group_kernel<DP, false>), dim3(rec[1]), dim3(kAT), 0, st, s, Fo, D, f.lists.mid,
                           (const uint32_t*)nullptr, (double*)nullptr, f.not_pd);
    if (rec[2]) {
        hipLaunchKernelGGL((als_group_kernel<DP, true>), dim3(rec[3]), dim3(kAT), 0, st, s, Fo, D, f.lists.seg_vertex,
                           f.lists.seg_index, f.ws, f.not_pd);
        hipLaunchKernelGGL(als_finish_kernel<DP>, dim3((rec[2] + kWaves - 1) / kWaves), dim3(kAT), 0, st, s, D,
                           f.lists.high, f.lists.high_base, rec[2], f.ws, f.not_pd);
    }
}

void launch_compact(const FitLayout& f, int k, hipStream_t st) {
    const AlsSide& s = f.side[k];
    const uint32_t blocks = (uint32_t)(((uint64_t)s.n + kCompBlock - 1) / kCompBlock);
    if (blocks) {
        hipLaunchKernelGGL(als_compact_kernel<false>, dim3(blocks), dim3(kAT), 0, st, s, f.lists);
        hipLaunchKernelGGL(als_scan_kernel, dim3(1), dim3(64), 0, st, f.lists, blocks);
        hipLaunchKernelGGL(als_compact_kernel<true>, dim3(blocks), dim3(kAT), 0, st, s, f.lists);
    } else {
        hipLaunchKernelGGL(als_scan_kernel, dim3(1), dim3(64), 0, st, f.lists, 0u);
    }
}

struct AlsEvents {   // destroyed on every return path
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~AlsEvents() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

// Per-vertex degree counts of one CSR against the other's neighbour lists (the transpose check).
bool transpose_counts_agree(uint32_t n_a, const uint64_t* off_a, const uint32_t* nbr_a, uint32_t n_b,
                            const uint64_t* off_b) {
    std::vector<uint64_t> cnt(n_b, 0);
    for (uint64_t e = 0; e < off_a[n_a]; ++e) cnt[nbr_a[e]]++;
    for (uint32_t v = 0; v < n_b; ++v)
        if (cnt[v] != off_b[v + 1] - off_b[v]) return false;
    return true;
}

int check_csr(cf_ctx* ctx, const char* what, uint32_t n, const uint64_t* off, const uint32_t* nbr, uint32_t n_other) {
    if (off[0] != 0) return cf_set_error(ctx, CF_EINVAL, std::string("cf_als_fit: ") + what + " offsets do not start at 0");
    for (uint32_t v = 0; v < n; ++v)
        if (off[v + 1] < off[v]) return cf_set_error(ctx, CF_EINVAL, std::string("cf_als_fit: ") + what + " offsets decrease");
    for (uint64_t e = 0; e < off[n]; ++e)
        if (nbr[e] >= n_other) return cf_set_error(ctx, CF_EINVAL, std::string("cf_als_fit: ") + what + " index out of range");
    return CF_OK;
}

int check_pairs(cf_ctx* ctx, const char* fn, uint64_t n, const uint32_t* user, const uint32_t* item, const double* U,
                const double* V, uint32_t D, uint32_t n_users, uint32_t n_items) {
    if (D == 0) return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": D = 0");
    if (D > CF_ALS_MAX_D) return cf_set_error(ctx, CF_ERANGE, std::string(fn) + ": D above CF_ALS_MAX_D");
    if (n && (!user || !item || !U || !V)) return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": null argument");
    for (uint64_t e = 0; e < n; ++e)
        if (user[e] >= n_users || item[e] >= n_items)
            return cf_set_error(ctx, CF_EINVAL, std::string(fn) + ": index out of range");
    return CF_OK;
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
    const uint64_t nnz = n_users ? user_off[n_users] : 0;
    const uint64_t nnz_i = n_items ? item_off[n_items] : 0;
    if (nnz != nnz_i) return cf_set_error(ctx, CF_EINVAL, "cf_als_fit: the two CSRs hold different edge counts");
    if (nnz && (!user_item || !user_obs || !item_user || !item_obs))
        return cf_set_error(ctx, CF_EINVAL, "cf_als_fit: null edge array");
    if (n_users) CF_TRY(check_csr(ctx, "user", n_users, user_off, user_item, n_items));
    if (n_items) CF_TRY(check_csr(ctx, "item", n_items, item_off, item_user, n_users));
    if (nnz && (!transpose_counts_agree(n_users, user_off, user_item, n_items, item_off) ||
                !transpose_counts_agree(n_items, item_off, item_user, n_users, user_off)))
        return cf_set_error(ctx, CF_EINVAL, "cf_als_fit: the per-vertex edge counts of the user CSR and the item CSR disagree");
    if (n_users == 0) return CF_OK;   // nothing can be active
    CF_TRY(set_device(ctx));

    // everything the fit needs exists before its first launch
    const uint64_t seg_cap = std::max(total_segments(n_users, user_off), n_items ? total_segments(n_items, item_off) : 0);
    if (seg_cap > 0xffffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_als_fit: too many segments");
    FitLayout f{};
    {
        Carver size;
        carve_fit(size, f, n_users, n_items, nnz, (int)D, seg_cap);
        CF_TRY(als_reserve(ctx, size.pos));
        Carver c;
        c.base = static_cast<char*>(ctx->d_als);
        carve_fit(c, f, n_users, n_items, nnz, (int)D, seg_cap);
    }
    AlsEvents evs;
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
        CF_HIP_CHECK(ctx, hipMemcpy((void*)s.off, h_off[k], sizeof(uint64_t) * ((size_t)n[k] + 1), hipMemcpyHostToDevice));
        if (nnz) {
            CF_HIP_CHECK(ctx, hipMemcpy((void*)s.nbr, h_nbr[k], sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
            CF_HIP_CHECK(ctx, hipMemcpy((void*)s.obs, h_obs[k], sizeof(float) * nnz, hipMemcpyHostToDevice));
            std::vector<uint32_t> src(nnz);
            for (uint32_t v = 0; v < n[k]; ++v)
                for (uint64_t e = h_off[k][v]; e < h_off[k][v + 1]; ++e) src[e] = v;
            CF_HIP_CHECK(ctx, hipMemcpy((void*)s.src, src.data(), sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
        }
        CF_HIP_CHECK(ctx, hipMemcpy(s.F, h_F[k], sizeof(double) * (size_t)n[k] * D, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy((void*)s.reg, h_reg[k], sizeof(double) * n[k], hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy(s.nupd, h_nupd[k], sizeof(uint32_t) * n[k], hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy(s.resid, h_res[k], sizeof(float) * n[k], hipMemcpyHostToDevice));
        if (k == 0 && activate_user) CF_HIP_CHECK(ctx, hipMemcpy(s.flag, activate_user, n[k], hipMemcpyHostToDevice));
        else CF_HIP_CHECK(ctx, hipMemset(s.flag, k == 0 ? 1 : 0, n[k]));
        CF_HIP_CHECK(ctx, hipMemset(s.active, 0, n[k]));
    }
    CF_HIP_CHECK(ctx, hipMemset(f.not_pd, 0, sizeof(unsigned long long)));

    const int DP = D <= 8 ? 8 : (D <= 16 ? 16 : (D <= 32 ? 32 : 64));
    if ((nnz * kG + kAT - 1) / kAT > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_als_fit: too many edges");
    const unsigned scatter_blocks = (unsigned)((nnz * kG + kAT - 1) / kAT);
    uint32_t supersteps = 0;
    uint64_t updates = 0;
    double update_ms = 0.0, scatter_ms = 0.0;
    int k = 0;   // the side being updated: users first (als.cpp:363-367,662)
    launch_compact(f, k, st);
    for (;;) {
        // the one small record of the superstep: the active counts per class and the segments
        uint32_t rec[4];
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(rec, f.lists.record, sizeof(rec), hipMemcpyDeviceToHost));   // waits for the stream
        if (supersteps) {
            float a = 0.0f, b = 0.0f;
            (void)hipEventElapsedTime(&a, evs.e[0], evs.e[1]);
            (void)hipEventElapsedTime(&b, evs.e[1], evs.e[2]);
            update_ms += a;
            scatter_ms += b;
        }
        const uint64_t n_active = (uint64_t)rec[0] + rec[1] + rec[2];
        if (n_active == 0) break;                                   // the run ends when no vertex is active
        if (max_supersteps && supersteps >= max_supersteps) break;
        if (rec[3] > f.seg_cap) return cf_set_error(ctx, CF_EHIP, "cf_als_fit: segment list overflow");
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
        switch (DP) {
            case 8: launch_update<8>(f, k, (int)D, rec, st); break;
            case 16: launch_update<16>(f, k, (int)D, rec, st); break;
            case 32: launch_update<32>(f, k, (int)D, rec, st); break;
            default: launch_update<64>(f, k, (int)D, rec, st); break;
        }
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
        if (nnz && n[1 - k])
            hipLaunchKernelGGL(als_scatter_kernel, dim3(scatter_blocks), dim3(kAT), 0, st, f.side[k], nnz,
                               (const double*)f.side[1 - k].F, (const uint32_t*)f.side[1 - k].nupd, f.side[1 - k].flag,
                               (int)D, tol, max_updates);
        k = 1 - k;
        launch_compact(f, k, st);
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

namespace {

// Uploads the pair list and both factor matrices into the context's ALS workspace.
struct PairLayout {
    uint32_t* user;
    uint32_t* item;
    float* obs;
    double* U;
    double* V;
    double* out;       // predictions, or the block partials followed by the sum
};

int upload_pairs(cf_ctx* ctx, PairLayout& p, uint64_t n, const uint32_t* user, const uint32_t* item, const float* obs,
                 uint32_t nu, uint32_t ni, uint32_t D, const double* U, const double* V, size_t n_out) {
    for (int pass = 0; pass < 2; ++pass) {
        Carver c;
        if (pass) c.base = static_cast<char*>(ctx->d_als);
        p.user = c.take<uint32_t>(n);
        p.item = c.take<uint32_t>(n);
        p.obs = c.take<float>(n);
        p.U = c.take<double>((size_t)nu * D);
        p.V = c.take<double>((size_t)ni * D);
        p.out = c.take<double>(n_out);
        if (!pass) CF_TRY(als_reserve(ctx, c.pos));
    }
    CF_HIP_CHECK(ctx, hipMemcpy(p.user, user, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    CF_HIP_CHECK(ctx, hipMemcpy(p.item, item, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    if (obs) CF_HIP_CHECK(ctx, hipMemcpy(p.obs, obs, sizeof(float) * n, hipMemcpyHostToDevice));
    CF_HIP_CHECK(ctx, hipMemcpy(p.U, U, sizeof(double) * (size_t)nu * D, hipMemcpyHostToDevice));
    CF_HIP_CHECK(ctx, hipMemcpy(p.V, V, sizeof(double) * (size_t)ni * D, hipMemcpyHostToDevice));
    return CF_OK;
}

}  // namespace

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
    const uint64_t blocks = (n_edges + kErrPerBlock - 1) / kErrPerBlock;
    if (blocks > 0x7fffffffull) return cf_set_error(ctx, CF_ERANGE, "cf_als_error: too many edges");
    PairLayout p{};
    CF_TRY(upload_pairs(ctx, p, n_edges, user, item, obs, n_users, n_items, D, U, V, (size_t)blocks + 1));
    hipLaunchKernelGGL(als_error_kernel, dim3((unsigned)blocks), dim3(kAT), 0, nullptr, n_edges, (const uint32_t*)p.user,
                       (const uint32_t*)p.item, (const float*)p.obs, (const double*)p.U, (const double*)p.V, (int)D,
                       minval, maxval, p.out);
    hipLaunchKernelGGL(als_error_final_kernel, dim3(1), dim3(kAT), 0, nullptr, (const double*)p.out, blocks,
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
    hipLaunchKernelGGL(als_predict_kernel, dim3((unsigned)blocks), dim3(kAT), 0, nullptr, n_pairs,
                       (const uint32_t*)p.user, (const uint32_t*)p.item, (const double*)p.U, (const double*)p.V, (int)D,
                       p.out);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(pred, p.out, sizeof(double) * n_pairs, hipMemcpyDeviceToHost));
    return CF_OK;
}
