// cf_ease.hip -- EASE (Steck, WWW 2019), the closed-form linear item-item model: the fit
//   G = X^T X + lambda I,  P = G^-1,  B[i][j] = -P[i][j] / P[j][j] (i != j),  B[j][j] = 0
// on the GPU in fp64, B resident in the context, and B as a score source of the panel drivers
// (cf_ease_topn, cf_ease_rank_eval): s(u, j) = sum_t x_t B[i_t][j] over the profile.  DESIGN 3.22.
//
//   ease_gram_kernel    one workgroup per row i of G: item i's users in ascending order (the by-item
//                       CSR: lists_by_key of cf_sort.h over the edge positions, once per fit),
//                       and per user u the lanes stride over u's list, G[i][j] += x_ui x_uj as a plain
//                       read-modify-write (the j of one strictly ascending list differ: no two lanes
//                       collide); __syncthreads() between users orders two users' accesses to one j.
//                       lambda joins the diagonal last.  Work: sum_u deg(u)^2.
//   inversion           in place, blocked Gauss-Jordan without pivoting, block width kEaseB = the
//                       64 x 64 MFMA tile.  Per block step k (k0 = k kEaseB):
//     ease_diag_kernel    one workgroup: D = (A[k][k])^-1 by Gauss-Jordan in LDS (a ragged last block
//                         is padded with the identity), to a side buffer
//     ease_gemm<kRow>     R[:, j] = D A[k][j] for every tile j != k, to a side buffer
//     ease_gemm<kUpdate>  A[i][j] -= A[i][k] R[:, j] for every tile i != k, j != k: one workgroup per
//                         64 x 64 tile, v_mfma_f64_16x16x4_f64 with the operand staging and the lane
//                         maps of topn_score_kernel (cf_topn_panel.h)
//     ease_gemm<kCol>     A[i][k] = -A[i][k] D for every tile i != k
//     ease_rowcopy_kernel A[k][j] = R[:, j], A[k][k] = D
//                       Every element of a step is one MFMA chain of kEaseB terms from zero in a
//                       fixed order: the bytes of P depend on G and kEaseB only.
//   ease_diag_take_kernel / ease_normalise_kernel   d[j] = P[j][j], then B in place
//   ease_score_kernel   grid = column tiles x user rows of the block, rows fastest, so that the
//                       workgroups that read one slab B[:, tile] run together.  A lane owns kEaseCpl
//                       columns in registers, walks the profile with kEaseUnroll rows of B in flight
//                       and stores score_key(s) once: no read-modify-write of the panel, no barrier.
// No floating-point atomics anywhere.

#include <cmath>

#include "cf_sort.h"
#include "cf_topn_panel.h"

namespace {

constexpr int kEaseB = 64;                    // inversion block width = the MFMA tile (kTU = kTI)
constexpr int kEaseCpl = 2;                   // columns per lane of the score kernel
constexpr int kEaseCols = kAT * kEaseCpl;     // items per workgroup of the score kernel
constexpr int kEaseUnroll = 4;                // profile entries in flight per lane
constexpr uint32_t kEaseMaxItems = 1u << 24;
constexpr unsigned kGridY = 65535;

static_assert(kEaseB == kTU && kEaseB == kTI && kEaseB == 2 * kKC, "a block step is one 64 x 64 tile, two staged passes deep");

// ---- Gram ------------------------------------------------------------------------------------------

// Row blockIdx.x of G.  ipos: the edge positions (into the user CSR) of item i, ascending, so the
// users ascend; owner[p]: the user of edge p.
__global__ __launch_bounds__(kAT) void ease_gram_kernel(const uint64_t* __restrict__ ioff, const uint32_t* __restrict__ ipos,
                                                       const uint32_t* __restrict__ owner,
                                                       const uint64_t* __restrict__ uoff, const uint32_t* __restrict__ uitem,
                                                       const float* __restrict__ uobs, int binary, uint32_t n_items,
                                                       double lambda, double* G) {
    const uint32_t i = blockIdx.x;
    double* row = G + (size_t)i * n_items;
    for (uint32_t j = threadIdx.x; j < n_items; j += kAT) row[j] = 0.0;
    __syncthreads();
    const uint64_t e1 = ioff[i + 1];
    for (uint64_t e = ioff[i]; e < e1; ++e) {   // the order is the contract; the same trips for the whole workgroup
        const uint32_t p = ipos[e];
        const uint32_t u = owner[p];
        const double xi = binary ? 1.0 : (double)uobs[p];
        const uint64_t q1 = uoff[u + 1];
        for (uint64_t q = uoff[u] + threadIdx.x; q < q1; q += kAT) {
            const uint32_t j = uitem[q];
            const double xj = binary ? 1.0 : (double)uobs[q];
            if (j < n_items) row[j] = row[j] + xi * xj;   // the product is exact in fp64
        }
        __syncthreads();   // user e + 1 may touch the same j from another lane
    }
    if (threadIdx.x == 0) row[i] = row[i] + lambda;
}

// ---- inversion -------------------------------------------------------------------------------------

// D = (A[k0 .. k0 + kEaseB)^2)^-1, rows and columns past n taken from the identity.  In-place
// Gauss-Jordan over the kEaseB pivots in order; every thread rewrites its own elements from a
// snapshot of the pivot row and column.
__global__ __launch_bounds__(kAT) void ease_diag_kernel(const double* __restrict__ A, uint32_t n, uint32_t k0,
                                                       double* __restrict__ D) {
    __shared__ double s[kEaseB * kEaseB];
    __shared__ double s_row[kEaseB], s_col[kEaseB];
    for (int idx = threadIdx.x; idx < kEaseB * kEaseB; idx += kAT) {
        const int r = idx / kEaseB, c = idx - r * kEaseB;
        const uint64_t gr = (uint64_t)k0 + r, gc = (uint64_t)k0 + c;
        s[idx] = (gr < n && gc < n) ? A[gr * n + gc] : (r == c ? 1.0 : 0.0);
    }
    for (int p = 0; p < kEaseB; ++p) {
        __syncthreads();
        if (threadIdx.x < kEaseB) {
            s_row[threadIdx.x] = s[p * kEaseB + threadIdx.x];
            s_col[threadIdx.x] = s[threadIdx.x * kEaseB + p];
        }
        __syncthreads();
        const double piv = 1.0 / s_row[p];
        for (int idx = threadIdx.x; idx < kEaseB * kEaseB; idx += kAT) {
            const int r = idx / kEaseB, c = idx - r * kEaseB;
            double v;
            if (r == p) v = c == p ? piv : s_row[c] * piv;
            else if (c == p) v = -(s_col[r] * piv);
            else v = s[idx] - s_col[r] * (s_row[c] * piv);
            s[idx] = v;
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < kEaseB * kEaseB; idx += kAT) D[idx] = s[idx];
}

// The three GEMM-shaped parts of block step k over 64 x 64 tiles, depth kEaseB:
//   kRow     tile j = blockIdx.x:               R[:, j]  = D A[k][j]          (j != k)
//   kUpdate  tile (i, j) = (blockIdx.y .., blockIdx.x):  A[i][j] -= A[i][k] R[:, j]   (i != k, j != k)
//   kCol     tile i = blockIdx.x:               A[i][k]  = -A[i][k] D         (i != k)
// Everything read past row or column n is zero.  Wave w owns the 32 x 32 quadrant (w >> 1, w & 1)
// as 2 x 2 MFMA tiles; the lane maps are topn_score_kernel's: left lane l = row (l & 15), depth
// (l >> 4); right lane l = column (l & 15), depth (l >> 4) (the right operand is staged transposed);
// result q of lane l = row (l >> 4) + 4 q, column l & 15.
enum { kRow = 0, kUpdate = 1, kCol = 2 };
template <int MODE>
__global__ __launch_bounds__(kAT) void ease_gemm_kernel(double* A, uint32_t n, uint32_t n_tiles, uint32_t k,
                                                       const double* __restrict__ D, double* R, uint32_t ldr) {
    __shared__ double s_a[kEaseB * kSt];
    __shared__ double s_b[kEaseB * kSt];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wu = (wave >> 1) * 32, wi = (wave & 1) * 32;
    const uint64_t k0 = (uint64_t)k * kEaseB;
    for (uint32_t it = MODE == kUpdate ? blockIdx.y : 0; it < (MODE == kUpdate ? n_tiles : 1u); it += gridDim.y) {
        const uint32_t ti = MODE == kUpdate ? it : blockIdx.x;   // row tile (kUpdate, kCol)
        const uint32_t tj = blockIdx.x;                          // column tile (kRow, kUpdate)
        if ((MODE != kRow && ti == k) || (MODE != kCol && tj == k)) continue;   // the same for the whole workgroup
        const uint64_t i0 = (uint64_t)ti * kEaseB, j0 = (uint64_t)tj * kEaseB;
        d4 acc[2][2];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[x][y] = d4{0.0, 0.0, 0.0, 0.0};
        for (int d0 = 0; d0 < kEaseB; d0 += kKC) {
            __syncthreads();   // the previous pass (or tile) is done with the staged operands
            for (int idx = threadIdx.x; idx < kEaseB * kKC; idx += kAT) {
                {   // left operand: row r, depth d, contiguous along d
                    const int r = idx / kKC, dd = idx - r * kKC, d = d0 + dd;
                    double a;
                    if (MODE == kRow) a = D[r * kEaseB + d];
                    else a = (i0 + r < n && k0 + d < n) ? A[(i0 + r) * n + k0 + d] : 0.0;
                    s_a[r * kSt + dd] = a;
                }
                {   // right operand: depth d, column c, contiguous along c
                    const int dd = idx / kEaseB, c = idx - dd * kEaseB, d = d0 + dd;
                    double b;
                    if (MODE == kRow) b = (k0 + d < n && j0 + c < n) ? A[(k0 + d) * n + j0 + c] : 0.0;
                    else if (MODE == kUpdate) b = R[(size_t)d * ldr + j0 + c];
                    else b = D[d * kEaseB + c];
                    s_b[c * kSt + dd] = b;
                }
            }
            __syncthreads();
            for (int kk = 0; kk < kKC; kk += 4) {
                double av[2], bv[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) av[x] = s_a[(wu + x * 16 + (lane & 15)) * kSt + kk + (lane >> 4)];
#pragma unroll
                for (int y = 0; y < 2; ++y) bv[y] = s_b[(wi + y * 16 + (lane & 15)) * kSt + kk + (lane >> 4)];
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y)
                        acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], bv[y], acc[x][y], 0, 0, 0);
            }
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = wu + x * 16 + (lane >> 4) + 4 * q;
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const int c = wi + y * 16 + (lane & 15);
                    const double v = acc[x][y][q];
                    if (MODE == kRow) {
                        R[(size_t)r * ldr + j0 + c] = v;   // ldr covers whole tiles
                    } else if (MODE == kUpdate) {
                        if (i0 + r < n && j0 + c < n) A[(i0 + r) * n + j0 + c] -= v;
                    } else {
                        if (i0 + r < n && k0 + c < n) A[(i0 + r) * n + k0 + c] = -v;
                    }
                }
            }
    }
}

// Rows k0 .. k0 + kEaseB of A (those below n): R outside the block's own columns, D inside.
__global__ __launch_bounds__(kAT) void ease_rowcopy_kernel(double* __restrict__ A, uint32_t n, uint32_t k0,
                                                          const double* __restrict__ D, const double* __restrict__ R,
                                                          uint32_t ldr) {
    const uint64_t c = (uint64_t)blockIdx.x * kAT + threadIdx.x;
    const uint64_t gr = (uint64_t)k0 + blockIdx.y;
    if (c >= n || gr >= n) return;
    const bool own = c >= k0 && c < (uint64_t)k0 + kEaseB;
    A[gr * n + c] = own ? D[blockIdx.y * kEaseB + (c - k0)] : R[(size_t)blockIdx.y * ldr + c];
}

// ---- normalise -------------------------------------------------------------------------------------

__global__ __launch_bounds__(kAT) void ease_diag_take_kernel(const double* __restrict__ P, uint32_t n, double* __restrict__ d) {
    const uint64_t j = (uint64_t)blockIdx.x * kAT + threadIdx.x;
    if (j < n) d[j] = P[j * n + j];
}

__global__ __launch_bounds__(kAT) void ease_normalise_kernel(double* __restrict__ P, uint32_t n, const double* __restrict__ d) {
    const uint64_t j = (uint64_t)blockIdx.x * kAT + threadIdx.x;
    if (j >= n) return;
    const double dj = d[j];
    for (uint64_t i = blockIdx.y; i < n; i += gridDim.y) P[i * n + j] = i == j ? 0.0 : -P[i * n + j] / dj;
}

// ---- score -----------------------------------------------------------------------------------------

// Workgroup blockIdx.x = tile * nb + row: user sel[b0 + row] (b0 + row without a selection), the
// columns tile kEaseCols + threadIdx.x + c kAT.
__global__ __launch_bounds__(kAT) void ease_score_kernel(const double* __restrict__ B, uint32_t n_items,
                                                        const uint64_t* __restrict__ prof_off,
                                                        const uint32_t* __restrict__ prof_item,
                                                        const float* __restrict__ prof_rating, int binary,
                                                        const uint32_t* __restrict__ sel, uint32_t b0, uint32_t nb,
                                                        uint64_t* __restrict__ panel) {
#pragma clang fp contract(off)
    const uint32_t tile = blockIdx.x / nb, row = blockIdx.x - tile * nb;
    const uint32_t u = sel ? sel[b0 + row] : b0 + row;
    const uint64_t c0 = (uint64_t)tile * kEaseCols + threadIdx.x;
    double acc[kEaseCpl];
#pragma unroll
    for (int c = 0; c < kEaseCpl; ++c) acc[c] = 0.0;
    const uint64_t p1 = prof_off[u + 1];
    for (uint64_t t = prof_off[u]; t < p1; t += kEaseUnroll) {   // the order is the contract
        double x[kEaseUnroll], bv[kEaseUnroll][kEaseCpl];
#pragma unroll
        for (int j = 0; j < kEaseUnroll; ++j) {
            const bool live = t + j < p1;
            const uint32_t it = live ? prof_item[t + j] : 0u;
            x[j] = live ? (binary ? 1.0 : (double)prof_rating[t + j]) : 0.0;
#pragma unroll
            for (int c = 0; c < kEaseCpl; ++c) {
                const uint64_t col = c0 + (uint64_t)c * kAT;
                bv[j][c] = (live && it < n_items && col < n_items) ? B[(size_t)it * n_items + col] : 0.0;
            }
        }
#pragma unroll
        for (int j = 0; j < kEaseUnroll; ++j) {
            if (t + j >= p1) break;
#pragma unroll
            for (int c = 0; c < kEaseCpl; ++c) {
                // written out under the pragma above: the product is rounded, then added (the
                // __dmul_rn / __dadd_rn wrappers are plain operators compiled where contraction is on)
                const double prod = x[j] * bv[j][c];
                acc[c] = acc[c] + prod;
            }
        }
    }
    uint64_t* prow = panel + (size_t)row * n_items;
#pragma unroll
    for (int c = 0; c < kEaseCpl; ++c) {
        const uint64_t col = c0 + (uint64_t)c * kAT;
        if (col < n_items) prow[col] = score_key(acc[c]);
    }
}

// ---- host ------------------------------------------------------------------------------------------

struct EaseFitLayout {
    uint64_t* uoff;
    uint32_t* uitem;
    float* uobs;
    uint32_t* owner;
    uint32_t* iota;
    uint32_t* key;
    uint32_t* ipos;
    uint64_t* ioff;
    char* sort_tmp;
    double* D;
    double* R;
    double* diag;
};

enum { kStageGram = 0, kStageInverse = 1, kStageFit = 2 };

// Gram, inversion and normalisation up to `stage` into d_A (n_items^2 doubles on the device).
int ease_stages(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, const uint64_t* user_off, const uint32_t* user_item,
                const float* user_obs, int binary, double lambda, int stage, double* d_A, float ms[3]) {
    const uint64_t nnz = n_users ? user_off[n_users] : 0;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n_items + kEaseB - 1) / kEaseB);
    const uint32_t ldr = n_tiles * kEaseB;
    hipStream_t st = nullptr;
    size_t sort_bytes = 0;
    const int bits = bits_for(n_items);
    if (nnz)
        CF_HIP_CHECK(ctx, lists_by_key(nullptr, sort_bytes, nullptr, nullptr, nullptr, true, nullptr, nnz, n_items, nullptr,
                                       bits, st));
    EaseFitLayout L{};
    CF_TRY(carve_workspace(ctx, [&](Carver& c) {
        L.uoff = c.take<uint64_t>((size_t)n_users + 1);
        L.uitem = c.take<uint32_t>(nnz);
        L.uobs = c.take<float>(nnz);
        L.owner = c.take<uint32_t>(nnz);
        L.iota = c.take<uint32_t>(nnz);
        L.key = c.take<uint32_t>(nnz);
        L.ipos = c.take<uint32_t>(nnz);
        L.ioff = c.take<uint64_t>((size_t)n_items + 1);
        L.sort_tmp = c.take<char>(sort_bytes);
        L.D = c.take<double>((size_t)kEaseB * kEaseB);
        L.R = c.take<double>((size_t)kEaseB * ldr);
        L.diag = c.take<double>(n_items);
    }));
    if (nnz) {
        CF_HIP_CHECK(ctx, hipMemcpy(L.uoff, user_off, sizeof(uint64_t) * ((size_t)n_users + 1), hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy(L.uitem, user_item, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
        CF_HIP_CHECK(ctx, hipMemcpy(L.uobs, user_obs, sizeof(float) * nnz, hipMemcpyHostToDevice));
        CF_TRY(upload_edge_owners(ctx, L.owner, n_users, user_off, nnz));
    }
    MfEvents<4> evs;
    for (hipEvent_t& e : evs.e) CF_HIP_CHECK(ctx, hipEventCreate(&e));

    CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
    if (nnz) {
        size_t tb = sort_bytes;
        // stable: the positions of one item stay ascending, and with them its users
        CF_HIP_CHECK(ctx, lists_by_key(L.sort_tmp, tb, L.uitem, L.key, L.iota, true, L.ipos, nnz, n_items, L.ioff, bits, st));
    } else {
        CF_HIP_CHECK(ctx, hipMemsetAsync(L.ioff, 0, sizeof(uint64_t) * ((size_t)n_items + 1), st));
    }
    hipLaunchKernelGGL(ease_gram_kernel, dim3(n_items), dim3(kAT), 0, st, (const uint64_t*)L.ioff, (const uint32_t*)L.ipos,
                       (const uint32_t*)L.owner, (const uint64_t*)L.uoff, (const uint32_t*)L.uitem, (const float*)L.uobs,
                       binary ? 1 : 0, n_items, lambda, d_A);
    CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
    CF_HIP_CHECK(ctx, hipGetLastError());

    if (stage >= kStageInverse) {
        const unsigned gy = std::min<unsigned>(n_tiles, kGridY);
        for (uint32_t k = 0; k < n_tiles; ++k) {
            const uint32_t k0 = k * kEaseB;
            hipLaunchKernelGGL(ease_diag_kernel, dim3(1), dim3(kAT), 0, st, (const double*)d_A, n_items, k0, L.D);
            if (n_tiles > 1) {
                hipLaunchKernelGGL(ease_gemm_kernel<kRow>, dim3(n_tiles), dim3(kAT), 0, st, d_A, n_items, n_tiles, k,
                                   (const double*)L.D, L.R, ldr);
                hipLaunchKernelGGL(ease_gemm_kernel<kUpdate>, dim3(n_tiles, gy), dim3(kAT), 0, st, d_A, n_items, n_tiles, k,
                                   (const double*)L.D, L.R, ldr);
                hipLaunchKernelGGL(ease_gemm_kernel<kCol>, dim3(n_tiles), dim3(kAT), 0, st, d_A, n_items, n_tiles, k,
                                   (const double*)L.D, L.R, ldr);
            }
            hipLaunchKernelGGL(ease_rowcopy_kernel, dim3(blocks_for(n_items), kEaseB), dim3(kAT), 0, st, d_A, n_items, k0,
                               (const double*)L.D, (const double*)L.R, ldr);
        }
        CF_HIP_CHECK(ctx, hipGetLastError());
    }
    CF_HIP_CHECK(ctx, hipEventRecord(evs.e[2], st));
    if (stage >= kStageFit) {
        hipLaunchKernelGGL(ease_diag_take_kernel, dim3(blocks_for(n_items)), dim3(kAT), 0, st, (const double*)d_A, n_items,
                           L.diag);
        hipLaunchKernelGGL(ease_normalise_kernel, dim3(blocks_for(n_items), std::min<unsigned>(n_items, kGridY)), dim3(kAT),
                           0, st, d_A, n_items, (const double*)L.diag);
        CF_HIP_CHECK(ctx, hipGetLastError());
    }
    CF_HIP_CHECK(ctx, hipEventRecord(evs.e[3], st));
    CF_HIP_CHECK(ctx, hipStreamSynchronize(st));
    for (int s = 0; s < 3; ++s) ms[s] = elapsed(evs.e[s], evs.e[s + 1]);
    return CF_OK;
}

int ease_check_fit(cf_ctx* ctx, const std::string& fn, uint32_t n_users, uint32_t n_items, const uint64_t* user_off,
                   const uint32_t* user_item, const float* user_obs, double lambda) {
    if (!std::isfinite(lambda) || !(lambda > 0.0)) return cf_set_error(ctx, CF_EINVAL, fn + ": lambda is not finite and > 0");
    if (n_items > kEaseMaxItems) return cf_set_error(ctx, CF_ERANGE, fn + ": more than 2^24 items");
    if (n_users) {
        CF_TRY(check_csr(ctx, fn.c_str(), "user", n_users, user_off, user_item, n_items, true, true, user_obs));
        if (user_off[n_users] >> 32) return cf_set_error(ctx, CF_ERANGE, fn + ": 2^32 or more edges");
    }
    return CF_OK;
}

// cf_ease_gram and cf_debug_ease_inverse: the stages into a buffer of the call's own, then to the host.
int ease_to_host(cf_ctx* ctx, const char* name, uint32_t n_users, uint32_t n_items, const uint64_t* user_off,
                 const uint32_t* user_item, const float* user_obs, int binary, double lambda, int stage, double* out) {
    if (!ctx) return CF_EINVAL;
    const std::string fn = name;
    CF_TRY(ease_check_fit(ctx, fn, n_users, n_items, user_off, user_item, user_obs, lambda));
    if (n_items == 0) return CF_OK;
    if (!out) return cf_set_error(ctx, CF_EINVAL, fn + ": null output");
    CF_TRY(set_device(ctx));
    DevBuf A;
    const size_t bytes = sizeof(double) * (size_t)n_items * n_items;
    CF_TRY(cf_malloc_evict(ctx, &A.p, bytes, "EASE matrix"));
    float ms[3];
    CF_TRY(ease_stages(ctx, n_users, n_items, user_off, user_item, user_obs, binary, lambda, stage,
                       static_cast<double*>(A.p), ms));
    CF_HIP_CHECK(ctx, hipMemcpy(out, A.p, bytes, hipMemcpyDeviceToHost));
    return CF_OK;
}

// The B source of the panel drivers: the profiles in the workspace, B in the context,
// ease_score_kernel over the block's rows and column tiles.
struct EasePanelSource final : ProfilePanelSource {
    int binary = 0;

    int fill(cf_ctx* ctx, hipStream_t st, const uint32_t* d_sel, uint32_t b0, uint32_t nb, uint64_t* d_panel) override {
        const uint64_t tiles = ((uint64_t)n_items + kEaseCols - 1) / kEaseCols;
        if (tiles * nb > 0x7fffffffull)
            return cf_set_error(ctx, CF_ERANGE, "EASE score: users per block x items exceed the launch grid");
        hipLaunchKernelGGL(ease_score_kernel, dim3((unsigned)(tiles * nb)), dim3(kAT), 0, st, (const double*)ctx->d_ease_B,
                           n_items, (const uint64_t*)dev.off, (const uint32_t*)dev.item, (const float*)dev.rating, binary, d_sel,
                           b0, nb, d_panel);
        return CF_OK;
    }
};

// The checks of the B source, before the drivers' own.
int ease_check(cf_ctx* ctx, const std::string& fn, uint32_t n_users, const uint64_t* prof_off, const uint32_t* prof_item,
               const float* prof_rating, int binary, EasePanelSource* src) {
    if (!ctx->d_ease_B) return cf_set_error(ctx, CF_ESTATE, fn + ": no EASE weights resident");
    CF_TRY(check_csr(ctx, fn.c_str(), "profile", n_users, prof_off, prof_item, ctx->ease_n, false, true, prof_rating));
    src->n_users = n_users, src->n_items = ctx->ease_n;
    src->prof_off = prof_off, src->prof_item = prof_item, src->prof_rating = prof_rating;
    src->binary = binary ? 1 : 0;
    return CF_OK;
}

}  // namespace

void cf_ease_free(cf_ctx* ctx) {
    if (ctx->d_ease_B) (void)hipFree(ctx->d_ease_B);
    ctx->d_ease_B = nullptr;
    ctx->ease_n = 0;
}

extern "C" int cf_debug_ease_block(void) { return kEaseB; }
extern "C" int cf_debug_ease_cols(void) { return kEaseCols; }
extern "C" int cf_debug_ease_unroll(void) { return kEaseUnroll; }

extern "C" int cf_ease_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, const uint64_t* user_off,
                           const uint32_t* user_item, const float* user_obs, int binary, double lambda) {
    if (!ctx) return CF_EINVAL;
    CF_TRY(ease_check_fit(ctx, "cf_ease_fit", n_users, n_items, user_off, user_item, user_obs, lambda));
    CF_TRY(set_device(ctx));
    CF_HIP_CHECK(ctx, hipDeviceSynchronize());
    cf_ease_free(ctx);   // the old B makes room for the new one
    for (float& m : ctx->ease_ms) m = 0.0f;
    if (n_items == 0) return CF_OK;
    void* p = nullptr;
    CF_TRY(cf_malloc_evict(ctx, &p, sizeof(double) * (size_t)n_items * n_items, "EASE weights"));
    ctx->d_ease_B = static_cast<double*>(p);
    ctx->ease_n = n_items;
    const int rc = ease_stages(ctx, n_users, n_items, user_off, user_item, user_obs, binary, lambda, kStageFit,
                               ctx->d_ease_B, ctx->ease_ms);
    if (rc != CF_OK) cf_ease_free(ctx);   // never a half-built B
    return rc;
}

extern "C" int cf_ease_gram(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, const uint64_t* user_off,
                            const uint32_t* user_item, const float* user_obs, int binary, double lambda, double* G) {
    return ease_to_host(ctx, "cf_ease_gram", n_users, n_items, user_off, user_item, user_obs, binary, lambda, kStageGram,
                        G);
}

extern "C" int cf_debug_ease_inverse(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, const uint64_t* user_off,
                                     const uint32_t* user_item, const float* user_obs, int binary, double lambda,
                                     double* P) {
    return ease_to_host(ctx, "cf_debug_ease_inverse", n_users, n_items, user_off, user_item, user_obs, binary, lambda,
                        kStageInverse, P);
}

extern "C" int cf_ease_weights(cf_ctx* ctx, uint32_t* n_items, double* B) {
    if (!ctx) return CF_EINVAL;
    if (!ctx->d_ease_B) return cf_set_error(ctx, CF_ESTATE, "cf_ease_weights: no EASE weights resident");
    if (n_items) *n_items = ctx->ease_n;
    if (!B) return CF_OK;
    CF_TRY(set_device(ctx));
    CF_HIP_CHECK(ctx, hipMemcpy(B, ctx->d_ease_B, sizeof(double) * (size_t)ctx->ease_n * ctx->ease_n, hipMemcpyDeviceToHost));
    return CF_OK;
}

extern "C" int cf_ease_upload(cf_ctx* ctx, uint32_t n_items, const double* B) {
    if (!ctx) return CF_EINVAL;
    if (n_items == 0 || !B) return cf_set_error(ctx, CF_EINVAL, "cf_ease_upload: no weights given");
    if (n_items > kEaseMaxItems) return cf_set_error(ctx, CF_ERANGE, "cf_ease_upload: more than 2^24 items");
    CF_TRY(set_device(ctx));
    CF_HIP_CHECK(ctx, hipDeviceSynchronize());
    cf_ease_free(ctx);
    void* p = nullptr;
    const size_t bytes = sizeof(double) * (size_t)n_items * n_items;
    CF_TRY(cf_malloc_evict(ctx, &p, bytes, "EASE weights"));
    const hipError_t e = hipMemcpy(p, B, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return cf_set_error(ctx, CF_EHIP, std::string("cf_ease_upload: ") + hipGetErrorString(e));
    }
    ctx->d_ease_B = static_cast<double*>(p);
    ctx->ease_n = n_items;
    return CF_OK;
}

extern "C" int cf_ease_timing(cf_ctx* ctx, float ms[3]) {
    if (!ctx || !ms) return CF_EINVAL;
    for (int s = 0; s < 3; ++s) ms[s] = ctx->ease_ms[s];
    return CF_OK;
}

extern "C" int cf_ease_topn(cf_ctx* ctx, uint32_t n_users, const uint64_t* prof_off, const uint32_t* prof_item,
                            const float* prof_rating, int binary, const uint64_t* excl_off, const uint32_t* excl_item,
                            uint32_t n_sel, const uint32_t* sel_user, uint32_t N, uint32_t* items, double* scores,
                            uint32_t* count, cf_topn_stats* stats) {
    if (!ctx) return CF_EINVAL;
    EasePanelSource src;
    CF_TRY(ease_check(ctx, "cf_ease_topn", n_users, prof_off, prof_item, prof_rating, binary, &src));
    return cf_topn_drive(ctx, "cf_ease_topn", src, n_users, ctx->ease_n, excl_off, excl_item, n_sel, sel_user, N, items,
                         scores, count, stats);
}

extern "C" int cf_ease_rank_eval(cf_ctx* ctx, uint32_t n_users, const uint64_t* prof_off, const uint32_t* prof_item,
                                 const float* prof_rating, int binary, const uint64_t* excl_off, const uint32_t* excl_item,
                                 const uint64_t* held_off, const uint32_t* held_item, const double* held_w, uint32_t N,
                                 uint32_t* rank, cf_rank_user* users, cf_rank_summary* summary) {
    if (!ctx) return CF_EINVAL;
    EasePanelSource src;
    CF_TRY(ease_check(ctx, "cf_ease_rank_eval", n_users, prof_off, prof_item, prof_rating, binary, &src));
    return cf_rank_drive(ctx, "cf_ease_rank_eval", src, n_users, ctx->ease_n, excl_off, excl_item, held_off, held_item,
                         held_w, N, rank, users, summary);
}
