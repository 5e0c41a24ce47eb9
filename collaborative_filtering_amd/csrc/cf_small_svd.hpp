// cf_small_svd.hpp -- full SVD of a small dense fp64 matrix on the host: one-sided (Hestenes)
// Jacobi.  cf_svd_fit calls it once per restart on the m x m upper bidiagonal T of the pass
// (m <= CF_SVD_MAX_NV), where the reference calls Eigen's JacobiSVD (eigen_wrapper.hpp:618-623);
// the convention is that wrapper's: svd(T, a, PT, b) gives T = a diag(b) PT^T, a and PT
// orthogonal, b descending and >= 0.  Signs of the vector pairs are not pinned (nor are Eigen's).
//
// Columns of G = T are rotated in pairs until they are mutually orthogonal, the same rotations
// accumulate in PT; then b_j = |G_j| and a_j = G_j / b_j.  Plane rotations on columns keep small
// singular values to high relative accuracy, which a bidiagonal with a graded diagonal needs.
// A column that has shrunk below eps |T|_F is a null direction and is rotated no further (it would
// never meet a relative criterion); a column whose norm is negligible at the end (b_j <= m eps b_0:
// T is singular) gets its a_j by completing the other columns to an orthonormal basis, so a is
// orthogonal also then.
//
// Plain C++17, no dependencies: compiles stand-alone (tools/small_svd_check.cpp is its program for
// a host sanitizer run; tests reach it through cf_debug_small_svd).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <numeric>
#include <vector>

namespace cfsvd {

constexpr int kMaxSweeps = 60;

// T: m x m row-major (not modified).  a, PT: m x m row-major; b: m.  Returns the sweeps run.
inline int small_svd(int m, const double* T, double* a, double* b, double* PT) {
    if (m <= 0) return 0;
    const size_t M = (size_t)m;
    // column-major working copies: column j at G + j * M
    std::vector<double> G(M * M), V(M * M, 0.0);
    for (size_t i = 0; i < M; ++i)
        for (size_t j = 0; j < M; ++j) G[j * M + i] = T[i * M + j];
    for (size_t j = 0; j < M; ++j) V[j * M + j] = 1.0;
    const double eps = 2.220446049250313e-16;
    const double tol = eps * std::sqrt((double)m);
    double fro2 = 0.0;
    for (double x : G) fro2 += x * x;
    const double dead = eps * eps * fro2;   // a column this short is a null direction: left alone
    int sweeps = 0;
    for (; sweeps < kMaxSweeps; ++sweeps) {
        bool rotated = false;
        for (size_t p = 0; p + 1 < M; ++p) {
            for (size_t q = p + 1; q < M; ++q) {
                double* gp = &G[p * M];
                double* gq = &G[q * M];
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (size_t i = 0; i < M; ++i) {
                    alpha += gp[i] * gp[i];
                    beta += gq[i] * gq[i];
                    gamma += gp[i] * gq[i];
                }
                if (alpha <= dead || beta <= dead) continue;
                if (gamma == 0.0 || std::fabs(gamma) <= tol * std::sqrt(alpha * beta)) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                double* vp = &V[p * M];
                double* vq = &V[q * M];
                for (size_t i = 0; i < M; ++i) {
                    const double x = gp[i], y = gq[i];
                    gp[i] = c * x - s * y;
                    gq[i] = s * x + c * y;
                    const double u = vp[i], w = vq[i];
                    vp[i] = c * u - s * w;
                    vq[i] = s * u + c * w;
                }
            }
        }
        if (!rotated) break;
    }
    std::vector<double> nrm(M);
    for (size_t j = 0; j < M; ++j) {
        double s = 0.0;
        for (size_t i = 0; i < M; ++i) s += G[j * M + i] * G[j * M + i];
        nrm[j] = std::sqrt(s);
    }
    std::vector<size_t> order(M);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return nrm[x] > nrm[y]; });
    const double floor_b = (double)m * eps * nrm[order[0]];
    std::vector<size_t> null_cols;
    for (size_t j = 0; j < M; ++j) {
        const size_t src = order[j];
        b[j] = nrm[src];
        for (size_t i = 0; i < M; ++i) PT[i * M + j] = V[src * M + i];
        if (nrm[src] > floor_b) {
            for (size_t i = 0; i < M; ++i) a[i * M + j] = G[src * M + i] / nrm[src];
        } else {
            null_cols.push_back(j);
        }
    }
    // complete a to an orthonormal basis: the unit vectors e_0, e_1, .. are taken in turn, each cleaned
    // by two Gram-Schmidt passes against the columns that exist, and the first that keeps a squared
    // norm of 1 / (2 m) fills the next missing column.  One sweep over the m unit vectors is enough:
    // their squared remainders add up to the number of missing columns, and the rejected ones hold
    // less than 1/2 of that in all.
    std::vector<char> have(M, 1);
    for (size_t j : null_cols) have[j] = 0;
    std::vector<double> cand(M);
    size_t e = 0;
    for (size_t j : null_cols) {
        double n2 = 0.0;
        while (e < M) {
            std::fill(cand.begin(), cand.end(), 0.0);
            cand[e++] = 1.0;
            for (int pass = 0; pass < 2; ++pass)
                for (size_t k = 0; k < M; ++k) {
                    if (!have[k]) continue;
                    double d = 0.0;
                    for (size_t i = 0; i < M; ++i) d += a[i * M + k] * cand[i];
                    for (size_t i = 0; i < M; ++i) cand[i] -= d * a[i * M + k];
                }
            n2 = 0.0;
            for (size_t i = 0; i < M; ++i) n2 += cand[i] * cand[i];
            if (n2 >= 0.5 / (double)m) break;
        }
        const double n = std::sqrt(n2);
        for (size_t i = 0; i < M; ++i) a[i * M + j] = n > 0.0 ? cand[i] / n : 0.0;
        have[j] = 1;
    }
    return sweeps;
}

}  // namespace cfsvd
