// cf_mf_reduce.h -- the three-class vertex reduction that cf_sgd.hip and cf_svdpp.hip share.
// Every active vertex reduces the edges of one of its lists to D sums, NS scalar sums and the
// count of accepted edges, and a policy type Op turns those into the vertex's pending values.
//
// One wave works on eight edges at a time: lane group g = lane >> 3 (kG = 8 lanes) takes edges
// g, g + 8, .. of the wave's range, lane sl of the group holds elements sl, sl + 8, .. of every
// row in registers (coalesced 64-byte pieces of a row).  A row is used by exactly one group, so
// it is gathered straight into registers.
// Work is shaped by the degree of the list that is walked, with the cuts of cf_mf_common.h:
//   low   one wave per vertex; mid  one workgroup per vertex, its waves take contiguous quarters
//   and their partials are summed in wave order in LDS; high  segments of kSeg edges, one
//   workgroup per segment (as mid) writes its partial sums [D sums | NS scalars | count] to an HBM
//   workspace and one wave per vertex adds them in segment order.
// This file is where the determinism rule of DESIGN 3.12 is implemented for both models: the
// class, the split points and every summation order of a vertex depend on its own degree only;
// an edge the policy rejects adds nothing and does not move the others; no floating-point
// atomics (the NaN and message counters are integer atomics).
//
// The policy, passed to the kernels by value:
//   NS, kCountNan                 scalar sums per vertex; whether acc.nan goes to counters[0]
//   dim()                         D
//   begin(v), end(v)              the list of vertex v
//   Own<NJ>, load_own(own, v, sl) the vertex's own rows and bias in registers
//   edge(acc, own, e, sl)         adds edge e to acc if the policy accepts it (one lane group)
//   finish_elem(v, d, sum, x, cnt), finish_scalar(v, x, cnt, counters)
//                                 the pending values from the sums, own values read from HBM
//   finish_elem_own(own, jj, ..), finish_scalar_own(own, ..)
//                                 the same for the low class, where `own` is still in registers
// TWO (a template parameter of the kernels and of launch_reduce, false unless asked for) gives
// every vertex a second set of D sums, acc.t, reduced in exactly the orders of the first; the
// policy then supplies finish_elem2(v, d, sum, sum2, x, cnt) and finish_elem2_own(own, jj, v, d,
// sum, sum2, x, cnt) in place of finish_elem / finish_elem_own (cf_nmf.hip's masked denominator).
// Partials in LDS and HBM are then [D sums | D second sums | NS scalars | count].
#pragma once

#include "cf_mf_common.h"

namespace {

template <int NJ>
__device__ __forceinline__ void load_row(double (&x)[NJ], const double* __restrict__ row, int D, int sl) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int d = sl + kG * j;
        x[j] = d < D ? row[d] : 0.0;
    }
}

// The partial sums of one wave: lane (g, sl) holds its group's part until reduce_groups().
template <int NJ, bool TWO>
struct AccSecond {
    double t[NJ];   // TWO: the second D sums, elements sl + 8 j
};
template <int NJ>
struct AccSecond<NJ, false> {};   // an empty base: without TWO, Acc is laid out as it always was
template <int NJ, int NS, bool TWO = false>
struct Acc : AccSecond<NJ, TWO> {
    double s[NJ];   // the D sums, elements sl + 8 j
    double x[NS];   // the scalar sums
    uint32_t cnt;   // accepted edges
    uint32_t nan;   // NaN errors met
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < NJ; ++j) s[j] = 0.0;
        if constexpr (TWO) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) this->t[j] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) x[k] = 0.0;
        cnt = nan = 0;
    }
    // fixed butterfly over the eight groups: afterwards every lane holds the wave's sums
    __device__ __forceinline__ void reduce_groups() {
#pragma unroll
        for (int o = kG; o < 64; o <<= 1) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) s[j] += __shfl_xor(s[j], o);
            if constexpr (TWO) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) this->t[j] += __shfl_xor(this->t[j], o);
            }
#pragma unroll
            for (int k = 0; k < NS; ++k) x[k] += __shfl_xor(x[k], o);
            cnt += __shfl_xor(cnt, o);
            nan += __shfl_xor(nan, o);
        }
    }
};

// acc += the edges [p0, p1) of the vertex that `own` belongs to.  Called by a whole wave.
template <int NJ, class Op, bool TWO>
__device__ __forceinline__ void wave_accumulate(Acc<NJ, Op::NS, TWO>& acc, const typename Op::template Own<NJ>& own,
                                                const Op& op, uint64_t p0, uint64_t p1, int lane) {
    const int g = lane >> 3, sl = lane & (kG - 1);
    for (uint64_t base = p0; base < p1; base += 64 / kG) {
        const uint64_t e = base + g;
        if (e >= p1) continue;   // whole groups
        op.template edge<NJ>(acc, own, e, sl);
    }
}

// counters: [0] NaN errors, [1] messages (finish_scalar's)
template <class Op>
__device__ __forceinline__ void count_nan(unsigned long long* counters, uint32_t nan) {
    if (Op::kCountNan && nan) atomicAdd(&counters[0], (unsigned long long)nan);
}

// low class: one wave per vertex.
template <int NJ, class Op, bool TWO = false>
__global__ __launch_bounds__(kAT) void mf_low_kernel(Op op, const uint32_t* __restrict__ list, uint32_t count_v,
                                                    unsigned long long* counters) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t j = blockIdx.x * kWaves + wave;
    if (j >= count_v) return;   // whole waves leave; no block barrier below
    const uint32_t v = list[j];
    const int sl = lane & (kG - 1), D = op.dim();
    typename Op::template Own<NJ> own;
    op.template load_own<NJ>(own, v, sl);
    Acc<NJ, Op::NS, TWO> acc;
    acc.clear();
    wave_accumulate<NJ>(acc, own, op, op.begin(v), op.end(v), lane);
    acc.reduce_groups();
    if (lane < kG) {
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int d = sl + kG * jj;
            if constexpr (TWO) {
                if (d < D) op.template finish_elem2_own<NJ>(own, jj, v, d, acc.s[jj], acc.t[jj], acc.x, (double)acc.cnt);
            } else {
                if (d < D) op.template finish_elem_own<NJ>(own, jj, v, d, acc.s[jj], acc.x, (double)acc.cnt);
            }
        }
    }
    if (lane == 0) {
        op.template finish_scalar_own<NJ>(own, v, acc.x, (double)acc.cnt, counters);
        count_nan<Op>(counters, acc.nan);
    }
}

// mid class (SEGMENT = false): one workgroup per vertex.  high class (SEGMENT = true): one
// workgroup per (vertex, segment); its D + NS + 1 partial sums go to workspace slot blockIdx.x.
template <int NJ, class Op, bool SEGMENT, bool TWO = false>
__global__ __launch_bounds__(kAT) void mf_group_kernel(Op op, const uint32_t* __restrict__ list,
                                                      const uint32_t* __restrict__ seg_index, double* ws,
                                                      unsigned long long* counters) {
    constexpr int NS = Op::NS;
    __shared__ double part[kWaves][(TWO ? 2 : 1) * CF_ALS_MAX_D + NS + 1];
    __shared__ double tot[(TWO ? 2 : 1) * CF_ALS_MAX_D + NS + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sl = lane & (kG - 1);
    const int D = op.dim();
    const int DS = TWO ? 2 * D : D;   // vector sums per vertex
    const uint32_t v = list[blockIdx.x];
    uint64_t p0 = op.begin(v);
    uint64_t len = op.end(v) - p0;
    if (SEGMENT) {
        const uint64_t first = (uint64_t)seg_index[blockIdx.x] * kSeg;
        p0 += first;
        len = len - first < (uint64_t)kSeg ? len - first : (uint64_t)kSeg;
    }
    const uint64_t chunk = (len + kWaves - 1) / kWaves;
    const uint64_t b = std::min(len, wave * chunk), e = std::min(len, (wave + 1) * chunk);
    typename Op::template Own<NJ> own;
    op.template load_own<NJ>(own, v, sl);
    Acc<NJ, NS, TWO> acc;
    acc.clear();
    wave_accumulate<NJ>(acc, own, op, p0 + b, p0 + e, lane);
    acc.reduce_groups();
    if (lane < kG) {
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int d = sl + kG * jj;
            if (d < D) part[wave][d] = acc.s[jj];
            if constexpr (TWO) {
                if (d < D) part[wave][D + d] = acc.t[jj];
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) part[wave][DS + k] = acc.x[k];
        part[wave][DS + NS] = (double)acc.cnt;
        count_nan<Op>(counters, acc.nan);
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < DS + NS + 1) {   // partials summed in wave order
        double sum = part[0][t];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) sum += part[w][t];
        if (SEGMENT) ws[(size_t)blockIdx.x * (DS + NS + 1) + t] = sum;
        else tot[t] = sum;
    }
    if (SEGMENT) return;
    __syncthreads();
    if constexpr (TWO) {
        if (t < D) op.finish_elem2(v, t, tot[t], tot[D + t], tot + DS, tot[DS + NS]);
    } else {
        if (t < D) op.finish_elem(v, t, tot[t], tot + D, tot[D + NS]);
    }
    if (t == 0) op.finish_scalar(v, tot + DS, tot[DS + NS], counters);
}

// high class, second pass: one wave per vertex adds its segments' partials in segment order.
template <class Op, bool TWO = false>
__global__ __launch_bounds__(kAT) void mf_finish_kernel(Op op, const uint32_t* __restrict__ list,
                                                       const uint32_t* __restrict__ base, uint32_t count_v,
                                                       const double* __restrict__ ws, unsigned long long* counters) {
    constexpr int NS = Op::NS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t j = blockIdx.x * kWaves + wave;
    if (j >= count_v) return;
    const uint32_t v = list[j];
    const int D = op.dim(), DS = TWO ? 2 * D : D, n = DS + NS + 1;
    const uint64_t deg = op.end(v) - op.begin(v);
    const uint32_t nseg = (uint32_t)((deg + kSeg - 1) / kSeg);
    const double* slot = ws + (size_t)base[j] * n;
    double x[NS + 1];   // the scalars and the count: every lane adds these itself, in the same order
#pragma unroll
    for (int k = 0; k <= NS; ++k) x[k] = slot[DS + k];
    for (uint32_t q = 1; q < nseg; ++q) {
#pragma unroll
        for (int k = 0; k <= NS; ++k) x[k] += slot[(size_t)q * n + DS + k];
    }
    for (int d = lane; d < D; d += 64) {
        double sum = slot[d];
        for (uint32_t q = 1; q < nseg; ++q) sum += slot[(size_t)q * n + d];
        if constexpr (TWO) {
            double sum2 = slot[D + d];
            for (uint32_t q = 1; q < nseg; ++q) sum2 += slot[(size_t)q * n + D + d];
            op.finish_elem2(v, d, sum, sum2, x, x[NS]);
        } else {
            op.finish_elem(v, d, sum, x, x[NS]);
        }
    }
    if (lane == 0) op.finish_scalar(v, x, x[NS], counters);
}

// scatter (sgd.cpp:320-329, svdpp.cpp:388-397): an edge whose owner is marked in `on` signals its
// other end; capped: only while that has updates left.  The flag stores are plain and all write
// the same value.  (cf_nmf.hip, where every vertex is always active, leaves it unused.)
__attribute__((unused)) __global__ __launch_bounds__(kAT) void mf_signal_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ nbr,
                                                       uint64_t nnz, const uint8_t* __restrict__ on,
                                                       const uint32_t* __restrict__ nupd_o, uint8_t* flag_o,
                                                       uint64_t max_updates, bool capped) {
    const uint64_t e = (uint64_t)blockIdx.x * kAT + threadIdx.x;
    if (e >= nnz) return;
    if (!on[src[e]]) return;
    const uint32_t w = nbr[e];
    if (!capped || (uint64_t)nupd_o[w] < max_updates) flag_o[w] = 1;
}

// ---- host ---------------------------------------------------------------------------------

// The reduction of the vertices in the class lists L (rec = L's record); ws holds
// rec[3] (D + NS + 1) doubles, with TWO rec[3] (2 D + NS + 1).
template <int NJ, bool TWO, class Op>
void launch_reduce_t(const Op& op, const AlsLists& L, const uint32_t rec[4], double* ws, unsigned long long* counters,
                     hipStream_t st) {
    if (rec[0])
        hipLaunchKernelGGL((mf_low_kernel<NJ, Op, TWO>), dim3((rec[0] + kWaves - 1) / kWaves), dim3(kAT), 0, st, op,
                           (const uint32_t*)L.low, rec[0], counters);
    if (rec[1])
        hipLaunchKernelGGL((mf_group_kernel<NJ, Op, false, TWO>), dim3(rec[1]), dim3(kAT), 0, st, op, (const uint32_t*)L.mid,
                           (const uint32_t*)nullptr, (double*)nullptr, counters);
    if (rec[2]) {
        hipLaunchKernelGGL((mf_group_kernel<NJ, Op, true, TWO>), dim3(rec[3]), dim3(kAT), 0, st, op,
                           (const uint32_t*)L.seg_vertex, (const uint32_t*)L.seg_index, ws, counters);
        hipLaunchKernelGGL((mf_finish_kernel<Op, TWO>), dim3((rec[2] + kWaves - 1) / kWaves), dim3(kAT), 0, st, op,
                           (const uint32_t*)L.high, (const uint32_t*)L.high_base, rec[2], (const double*)ws, counters);
    }
}

template <bool TWO = false, class Op>
void launch_reduce(const Op& op, const AlsLists& L, const uint32_t rec[4], double* ws, unsigned long long* counters,
                   hipStream_t st) {
    const int D = op.dim();
    if (D <= 8) launch_reduce_t<1, TWO>(op, L, rec, ws, counters, st);
    else if (D <= 16) launch_reduce_t<2, TWO>(op, L, rec, ws, counters, st);
    else if (D <= 24) launch_reduce_t<3, TWO>(op, L, rec, ws, counters, st);
    else if (D <= 32) launch_reduce_t<4, TWO>(op, L, rec, ws, counters, st);
    else launch_reduce_t<8, TWO>(op, L, rec, ws, counters, st);
}

}  // namespace
