// cf_als_update.h -- the three-class per-vertex update that cf_als.hip (explicit ALS) and
// cf_ials.hip (implicit-feedback ALS) share.  Every vertex of a class list assembles the packed
// system (A, b) of its edges with the Gram of cf_als_gram.h, and a policy type Op turns the
// assembled system into the stored factor.
//
// Work is shaped by the vertex's TRAIN degree, with cuts that are constants of cf_mf_common.h:
//   low   deg <= kLowMax           one wave per vertex, kWaves vertices per workgroup
//   mid   kLowMax < deg <= kSeg    one workgroup per vertex: its waves take contiguous quarters
//                                  of the list, the partial (A, b) are summed in wave order in LDS
//   high  deg > kSeg               the list is cut into segments of kSeg edges; one workgroup per
//                                  segment (as mid) writes its partial to an HBM workspace, and a
//                                  wave per vertex sums the partials in segment order and solves
// This file is where the determinism rule of DESIGN 3.12 is implemented for both models: the
// class, the split points and every summation order of a vertex depend on its own degree only --
// never on the launch, the active list or other vertices -- and there is no floating-point
// atomic (not_pd is an integer counter), so a vertex's new factor is the same bits whichever
// other vertices are active and however often a fit is repeated.  (SGD and SVD++ share their own
// implementation of the rule, cf_mf_reduce.h.)
//
// The policy, passed to the kernels by value (Fo, the other side's n x D factors, D and the lists
// are separate kernel arguments):
//   kWeighted                     the edge form of gram_accumulate (cf_als_gram.h)
//   s.off, s.nbr                  the CSR of the side being updated
//   edge_obs(), edge_pref()       the per-edge f32 arrays; edge_pref() is read only when kWeighted
//   no_edges(v, D, lane)          what a vertex without edges gets.  One wave
//   apply(S, D, v, not_pd, lane)  the tail: from the assembled system in S (LDS, the layout of
//                                 wave_ldlt_solve) to the stored factor of v.  One wave
#pragma once

#include <type_traits>

#include "cf_als_gram.h"

namespace {

// low class: one wave per vertex.
template <int DP, class Op>
__global__ __launch_bounds__(kAT) void als_low_kernel(Op op, const double* __restrict__ Fo, int D,
                                                     const uint32_t* __restrict__ list, uint32_t count,
                                                     unsigned long long* not_pd) {
    __shared__ __attribute__((aligned(16))) double lds[kWaves * low_region<DP>()];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t j = blockIdx.x * kWaves + wave;
    if (j >= count) return;   // whole waves leave; no block barrier below
    const uint32_t v = list[j];
    const uint64_t p0 = op.s.off[v], p1 = op.s.off[v + 1];
    if (p1 == p0) {
        op.no_edges(v, D, lane);
        return;
    }
    double* R = lds + wave * low_region<DP>();
    Gram<DP> g;
    g.clear();
    gram_accumulate<DP, Op::kWeighted>(g, R, Fo, D, op.s.nbr, op.edge_obs(), op.edge_pref(), p0, p1, lane);
    gram_to_system<DP, false>(g, R, D, lane);
    WAVE_SYNC();
    op.apply(R, D, v, not_pd, lane);
}

// mid class (SEGMENT = false): one workgroup per vertex, solved here.  high class (SEGMENT =
// true): one workgroup per (vertex, segment); the partial system goes to workspace slot
// blockIdx.x (sys_len(D) doubles per slot).
template <int DP, class Op, bool SEGMENT>
__global__ __launch_bounds__(kAT) void als_group_kernel(Op op, const double* __restrict__ Fo, int D,
                                                       const uint32_t* __restrict__ list,
                                                       const uint32_t* __restrict__ seg_index, double* ws,
                                                       unsigned long long* not_pd) {
    __shared__ __attribute__((aligned(16))) double lds[mid_region<DP>()];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t v = list[blockIdx.x];
    uint64_t p0 = op.s.off[v];
    uint64_t len = op.s.off[v + 1] - p0;
    if (SEGMENT) {
        const uint64_t first = (uint64_t)seg_index[blockIdx.x] * kSeg;
        p0 += first;
        len = len - first < (uint64_t)kSeg ? len - first : (uint64_t)kSeg;
    }
    const uint64_t chunk = (len + kWaves - 1) / kWaves;
    const uint64_t b = std::min(len, wave * chunk), e = std::min(len, (wave + 1) * chunk);
    Gram<DP> g;
    g.clear();
    gram_accumulate<DP, Op::kWeighted>(g, lds + wave * kBatch * DP, Fo, D, op.s.nbr, op.edge_obs(), op.edge_pref(), p0 + b,
                                       p0 + e, lane);
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
        op.apply(lds, D, v, not_pd, lane);
    }
}

// high class, second pass: one wave per vertex sums its segments' partials in segment order.
template <int DP, class Op>
__global__ __launch_bounds__(kAT) void als_finish_kernel(Op op, int D, const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ base, uint32_t count,
                                                        const double* __restrict__ ws, unsigned long long* not_pd) {
    __shared__ __attribute__((aligned(16))) double lds[kWaves * ((sys_len(DP) + 1) & ~1)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t j = blockIdx.x * kWaves + wave;
    if (j >= count) return;
    const uint32_t v = list[j];
    const uint64_t deg = op.s.off[v + 1] - op.s.off[v];
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
    op.apply(S, D, v, not_pd, lane);
}

// ---- host ---------------------------------------------------------------------------------

// fn(std::integral_constant<int, DP>) with the DP that D is padded to.
template <class Fn>
void dispatch_dp(int D, Fn fn) {
    if (D <= 8) fn(std::integral_constant<int, 8>{});
    else if (D <= 16) fn(std::integral_constant<int, 16>{});
    else if (D <= 32) fn(std::integral_constant<int, 32>{});
    else fn(std::integral_constant<int, 64>{});
}

// The update of the vertices in the class lists L (rec = L's record) from the other side's
// factors Fo; ws holds rec[3] sys_len(D) doubles.
template <class Op>
void launch_update(const Op& op, const double* Fo, int D, const AlsLists& L, const uint32_t rec[4], double* ws,
                   unsigned long long* not_pd, hipStream_t st) {
    dispatch_dp(D, [&](auto dp) {
        constexpr int DP = decltype(dp)::value;
        if (rec[0])
            hipLaunchKernelGGL((als_low_kernel<DP, Op>), dim3((rec[0] + kWaves - 1) / kWaves), dim3(kAT), 0, st, op, Fo,
                               D, (const uint32_t*)L.low, rec[0], not_pd);
        if (rec[1])
            hipLaunchKernelGGL((als_group_kernel<DP, Op, false>), dim3(rec[1]), dim3(kAT), 0, st, op, Fo, D,
                               (const uint32_t*)L.mid, (const uint32_t*)nullptr, (double*)nullptr, not_pd);
        if (rec[2]) {
            hipLaunchKernelGGL((als_group_kernel<DP, Op, true>), dim3(rec[3]), dim3(kAT), 0, st, op, Fo, D,
                               (const uint32_t*)L.seg_vertex, (const uint32_t*)L.seg_index, ws, not_pd);
            hipLaunchKernelGGL((als_finish_kernel<DP, Op>), dim3((rec[2] + kWaves - 1) / kWaves), dim3(kAT), 0, st, op,
                               D, (const uint32_t*)L.high, (const uint32_t*)L.high_base, rec[2], (const double*)ws,
                               not_pd);
        }
    });
}

}  // namespace
