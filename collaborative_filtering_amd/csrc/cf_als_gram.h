// cf_als_gram.h -- the per-vertex normal equations that cf_als.hip (explicit ALS) and cf_ials.hip
// (implicit-feedback ALS) share: the register block of one wave's Gram, its accumulation over an
// edge range, its transfer into the packed system and the one-wave unpivoted LDL^T.
//
// The Gram of one wave: D is padded to DP = 8 / 16 / 32 / 64 and lane l owns the TS x TS block
// (TS = DP / 8) at block row l >> 3, block column l & 7 of A, in registers; neighbour rows are
// staged kBatch at a time (coalesced) in wave-private LDS and every lane reads its 2 TS values
// per neighbour from there.  Each element is one fma chain in CSR order.
// WEIGHTED = false is explicit ALS: A += x x^T, b += obs x.  WEIGHTED = true is the
// implicit-feedback edge: A += (c - 1) x x^T, b += (c p) x with c = obs[e] (the confidence) and
// p = pref[e], both widened to fp64 first, so c - 1 and c p are exact; the weight c - 1 is
// multiplied into the lane's row values once per edge.  The unweighted instantiation is the
// arithmetic explicit ALS has always done, instruction for instruction.
// Everything has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

#include "cf_ldlt.hpp"
#include "cf_mf_common.h"

namespace {

constexpr int kBatch = 16;             // neighbour rows staged per wave at a time

__host__ __device__ constexpr int sys_len(int D) { return (D + 1) * (D + 2) / 2; }   // packed rows 0..D

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

// A and b over the edges [p0, p1) in order (see the header for the two edge forms); stage:
// kBatch * DP doubles of wave-private LDS; pref is read only when WEIGHTED.  Called by a whole wave.
template <int DP, bool WEIGHTED>
__device__ __forceinline__ void gram_accumulate(Gram<DP>& g, double* stage, const double* __restrict__ Fo, int D,
                                                const uint32_t* __restrict__ nbr, const float* __restrict__ obs,
                                                const float* __restrict__ pref, uint64_t p0, uint64_t p1, int lane) {
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
        float pf = 0.0f;
        if (WEIGHTED) pf = lane < nb ? pref[p + lane] : 0.0f;
        WAVE_SYNC();
        for (int k = 0; k < nb; ++k) {
            double xi[TS], xj[TS];
#pragma unroll
            for (int x = 0; x < TS; ++x) {
                xi[x] = stage[k * DP + ti * TS + x];
                xj[x] = stage[k * DP + tj * TS + x];
            }
            if (WEIGHTED) {
                const double c = (double)__shfl(ob, k);
                const double o = c * (double)__shfl(pf, k);
                const double w = c - 1.0;
#pragma unroll
                for (int x = 0; x < TS; ++x) {
                    const double wx = w * xi[x];
#pragma unroll
                    for (int y = 0; y < TS; ++y) g.a[x][y] = fma(wx, xj[y], g.a[x][y]);
                    g.b[x] = fma(o, xi[x], g.b[x]);
                }
            } else {
                const double o = (double)__shfl(ob, k);
#pragma unroll
                for (int x = 0; x < TS; ++x) {
#pragma unroll
                    for (int y = 0; y < TS; ++y) g.a[x][y] = fma(xi[x], xj[y], g.a[x][y]);
                    g.b[x] = fma(o, xi[x], g.b[x]);
                }
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

// Doubles of LDS of the update kernels: per wave of the low class (the staging rows, then the
// system in their place), and of the whole workgroup of the mid / high class.
template <int DP>
constexpr int low_region() {
    return ((kBatch * DP > sys_len(DP) ? kBatch * DP : sys_len(DP)) + 1) & ~1;
}

template <int DP>
constexpr int mid_region() {
    return ((kWaves * kBatch * DP > sys_len(DP) ? kWaves * kBatch * DP : sys_len(DP)) + 1) & ~1;
}

}  // namespace
