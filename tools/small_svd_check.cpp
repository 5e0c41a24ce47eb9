// small_svd_check -- csrc/cf_small_svd.hpp on its own, for a run under the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Icollaborative_filtering_amd/csrc tools/small_svd_check.cpp -o small_svd_check && ./small_svd_check
// Bidiagonal matrices of orders 1 .. 256, with and without a zero on the diagonal, and the zero
// matrix; prints the sweeps and max|a diag(b) PT^T - T| and fails when that is not roundoff.
#include <cstdio>
#include <random>
#include "cf_small_svd.hpp"
int main() {
    std::mt19937_64 g(1);
    int bad = 0;
    std::uniform_real_distribution<double> u(0.5, 10.0);
    for (int m : {1, 2, 7, 33, 128, 256}) {
        for (int zero = 0; zero < 2; ++zero) {
            std::vector<double> T((size_t)m * m, 0.0), a((size_t)m * m), PT((size_t)m * m), b(m);
            for (int i = 0; i < m; ++i) {
                T[(size_t)i * m + i] = (zero && i == m / 2) ? 0.0 : u(g);
                if (i + 1 < m) T[(size_t)i * m + i + 1] = u(g);
            }
            const int sw = cfsvd::small_svd(m, T.data(), a.data(), b.data(), PT.data());
            double worst = 0.0;
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < m; ++j) {
                    double s = 0.0;
                    for (int k = 0; k < m; ++k) s += a[(size_t)i * m + k] * b[k] * PT[(size_t)j * m + k];
                    worst = std::max(worst, std::fabs(s - T[(size_t)i * m + j]));
                }
            if (!(worst <= 64.0 * m * 2.220446049250313e-16 * b[0])) bad = 1;
            std::printf("m %d zero %d sweeps %d b0 %.6g bmin %.3g max|a b PT^T - T| %.3g\n", m, zero, sw, b[0], b[m - 1], worst);
        }
    }
    // all-zero matrix
    std::vector<double> Z(9, 0.0), a(9), PT(9), b(3);
    const int sw = cfsvd::small_svd(3, Z.data(), a.data(), b.data(), PT.data());
    std::printf("zero matrix sweeps %d b %g %g %g a00 %g\n", sw, b[0], b[1], b[2], a[0]);
    if (b[0] != 0.0 || a[0] != 1.0) bad = 1;
    return bad;
}
