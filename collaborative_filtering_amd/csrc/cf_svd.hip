// cf_svd.hip -- truncated SVD of the rating matrix by restarted Golub-Kahan-Lanczos on gfx950
// (svd.cpp:304-505 with math.hpp's Axb :98-185 and orthogonalize_vs_all :805-906), fp64 throughout.
//
// Naming.  A is rows x cols; U (rows x nsv) are the left vectors, V (cols x nsv) the right ones.
// The reference swaps the names inside lanczos(): its V[i] (DistSlicedMat V, svd.cpp:313) live on
// the row vertices -- v_0 has `rows` entries, :317-324, and linear_model_saver_U writes them,
// :173-193 -- and its U[i] on the column vertices.  Here P[i] is the row-side vector (the
// reference's V[i]) and Q[i] the column-side one (its U[i]); nothing below uses the inner names.
//
// The pass structure, the restart and the error estimates are stated in cf_abi.h (cf_svd_fit);
// the host loop below follows that text line by line.  The device does four kinds of work, all
// bound by HBM bandwidth:
//
// product   y = M x over one CSR (u64 offsets, u32 neighbour, f32 value): A x over the row CSR,
//           A^T x over the column CSR -- the two CSRs cf_als_fit takes.  x and y are dense fp64
//           vectors, so the gather hits 8 contiguous bytes per entry.  Work is shaped by the row's
//           own degree, with the cuts of cf_mf_common.h and one more (kWaveMax):
//             low    deg <= kLowMax             kG lanes per row, 8 rows per wave
//             wave   kLowMax < deg <= kWaveMax  one wave per row
//             group  kWaveMax < deg <= kSeg     one workgroup per row
//             high   deg > kSeg                 one workgroup per kSeg-long segment writes a partial
//                                               to HBM; one thread per row adds them in segment order
//           In every class lane l of L takes entries l, l + L, .. in order (one fma chain) and the
//           lanes are summed by a fixed xor tree (a workgroup: each wave's tree, then the waves in
//           order), so a row's summation order depends on its degree only.  16 or 32 lanes per row
//           in the wave class measured 4 % and 15 % slower on the probe's graph (mean degree 99).  Every row is active in every product, so
//           the class lists are built once per fit, on the host, from the offsets.
//           Bytes per product: nnz (4 + 4 + 8) + 8 n_out.
// ortho     w against B = the j vectors before it (classical Gram-Schmidt, all coefficients from
//           the same w, math.hpp:862,880), `repeats` times, two streaming passes each:
//             dots   workgroup b owns vertices [b kSlice, (b + 1) kSlice) and writes j partial dot
//                    products to HBM; a second small kernel adds them in a fixed order, one wave
//                    per coefficient (lane l takes blocks l, l + 64, .., then the xor tree)
//             axpy   w -= B c, the coefficients taken in order (math.hpp:834-837); the last repeat
//                    also writes the slice's part of |w|^2
//           then one kernel in which every workgroup adds the |w|^2 parts in the same fixed order,
//           takes the root and divides its slice iff the norm is >= 1e-10 (math.hpp:898); block 0
//           stores the norm (alpha or beta), which the host reads: one 8-byte record per step.
//           Bytes per repeat: 2 (j + 1) 8 n, plus 8 n for the last axpy's store and 16 n to normalise.
//           kSlice is a constant -- never the launch's or the device's -- so the same matrix gives
//           the same bits on any device and in every repeat.
// rotate    X_new = X[:, 0..m) C with C (m x c) in LDS, kRotCols columns per workgroup, one vertex
//           per thread, plain fma chains in t order into a scratch block that is copied back; the
//           restart vector is one more column of the same launch (C = PT[:, 0..kk]).
// residual  the product kernel, then r = y - sigma z with the slice parts of |r|^2.
// No floating-point atomics anywhere.
//
// Layout in HBM: the vectors of a side are column-major, each contiguous, ld = the side's length
// rounded up to 16 doubles (a 128-byte line); the tail [n, ld) of every vector is zero and stays
// zero under every kernel (0 - c 0, 0 / norm, sums of zeros), so the streaming kernels run over
// whole 16-byte pairs without a tail case.  nv + 1 vectors per side (the reference's nsv + nv + 1
// + max_iter slots per vertex are never all used).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cf_internal.h"
// of cf_mf_common.h this file takes the cuts, the block reduction, the workspace helpers and the
// CSR checks; its compaction and pair kernels stay unused here
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "cf_mf_common.h"
#pragma clang diagnostic pop
#include "cf_small_svd.hpp"

namespace {

constexpr int kWaveMax = 512;      // wave / group cut of the product
constexpr int kSlice = 1024;       // vertices per workgroup of the vector kernels: 2 pairs per thread
constexpr int kRotCols = 8;        // output columns per workgroup of the rotation
constexpr double kNormFloor = 1e-10;   // math.hpp:898
static_assert(kSlice == 4 * kAT, "two 16-byte pairs per thread");

// One CSR with its class lists, as the product kernels see it.
struct MvSide {
    uint32_t n;   // rows of this CSR = length of y
    const uint64_t* off;
    const uint32_t* nbr;
    const float* val;
    const uint32_t* low;
    const uint32_t* wave;
    const uint32_t* grp;
    const uint32_t* high;
    const uint32_t* high_base;    // first partial of each high row
    const uint32_t* seg_vertex;   // one entry per (high row, segment)
    const uint32_t* seg_index;
    double* partial;              // one per segment
    uint32_t n_low, n_wave, n_grp, n_high, n_seg;
};

// LANES lanes per row: row `block * (kAT / LANES) + group` of the list.
template <int LANES>
__device__ __forceinline__ void mv_rows(const MvSide& s, const uint32_t* __restrict__ list, uint32_t count, uint32_t block,
                                        const double* __restrict__ x, double* __restrict__ y) {
    const uint32_t j = (block * (uint32_t)kAT + threadIdx.x) / LANES;
    const int sl = threadIdx.x & (LANES - 1);
    if (j >= count) return;   // whole groups leave together
    const uint32_t v = list[j];
    const uint64_t p0 = s.off[v], p1 = s.off[v + 1];
    double acc = 0.0;
#pragma unroll 4
    for (uint64_t p = p0 + sl; p < p1; p += LANES) acc = fma((double)s.val[p], x[s.nbr[p]], acc);
#pragma unroll
    for (int o = LANES / 2; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, LANES);
    if (sl == 0) y[v] = acc;   // a row without entries: exactly 0
}

// low and wave classes in one launch: the first low_blocks workgroups take kG lanes per row, the
// others one wave per row.
__global__ __launch_bounds__(kAT) void svd_mv_rows_kernel(MvSide s, uint32_t low_blocks, const double* __restrict__ x,
                                                         double* __restrict__ y) {
    if (blockIdx.x < low_blocks) mv_rows<kG>(s, s.low, s.n_low, blockIdx.x, x, y);
    else mv_rows<64>(s, s.wave, s.n_wave, blockIdx.x - low_blocks, x, y);
}

// group and high classes in one launch: workgroup b < n_grp takes row grp[b]; the others take one
// (row, segment) each and write the partial to slot b - n_grp.
__global__ __launch_bounds__(kAT) void svd_mv_group_kernel(MvSide s, const double* __restrict__ x, double* __restrict__ y) {
    __shared__ double s_v[kWaves];
    const bool segment = blockIdx.x >= s.n_grp;
    const uint32_t slot = segment ? blockIdx.x - s.n_grp : blockIdx.x;
    const uint32_t v = segment ? s.seg_vertex[slot] : s.grp[slot];
    uint64_t p0 = s.off[v];
    uint64_t len = s.off[v + 1] - p0;
    if (segment) {
        const uint64_t first = (uint64_t)s.seg_index[slot] * kSeg;
        p0 += first;
        len = len - first < (uint64_t)kSeg ? len - first : (uint64_t)kSeg;
    }
    double acc = 0.0;
#pragma unroll 4
    for (uint64_t p = threadIdx.x; p < len; p += kAT) acc = fma((double)s.val[p0 + p], x[s.nbr[p0 + p]], acc);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = s_v[0];
#pragma unroll
        for (int q = 1; q < kWaves; ++q) sum += s_v[q];   // the waves in order
        if (segment) s.partial[slot] = sum;
        else y[v] = sum;
    }
}

// high class, second pass: one thread per row adds its partials in segment order.
__global__ __launch_bounds__(kAT) void svd_mv_finish_kernel(MvSide s, double* __restrict__ y) {
    const uint32_t j = blockIdx.x * (uint32_t)kAT + threadIdx.x;
    if (j >= s.n_high) return;
    const uint32_t v = s.high[j];
    const uint64_t deg = s.off[v + 1] - s.off[v];
    const uint32_t nseg = (uint32_t)((deg + kSeg - 1) / kSeg);
    const double* part = s.partial + s.high_base[j];
    double acc = part[0];
    for (uint32_t q = 1; q < nseg; ++q) acc += part[q];
    y[v] = acc;
}

// ---- vector kernels: workgroup b owns the pairs of vertices [b kSlice, (b + 1) kSlice) ---------

struct Pair2 {
    double2 a, b;   // vertices 2 t, 2 t + 1 of the slice's first and second half
};

__device__ __forceinline__ size_t slice_index(int half) {
    return (size_t)blockIdx.x * kSlice + (size_t)half * (kSlice / 2) + 2 * (size_t)threadIdx.x;
}
__device__ __forceinline__ Pair2 load_pair(const double* __restrict__ v, size_t ld) {
    Pair2 r;
    const size_t i0 = slice_index(0), i1 = slice_index(1);
    r.a = i0 < ld ? *reinterpret_cast<const double2*>(v + i0) : make_double2(0.0, 0.0);
    r.b = i1 < ld ? *reinterpret_cast<const double2*>(v + i1) : make_double2(0.0, 0.0);
    return r;
}
__device__ __forceinline__ void store_pair(double* __restrict__ v, size_t ld, const Pair2& r) {
    const size_t i0 = slice_index(0), i1 = slice_index(1);
    if (i0 < ld) *reinterpret_cast<double2*>(v + i0) = r.a;
    if (i1 < ld) *reinterpret_cast<double2*>(v + i1) = r.b;
}
__device__ __forceinline__ double pair_dot(const Pair2& p, const Pair2& q) {
    return fma(p.a.x, q.a.x, fma(p.a.y, q.a.y, fma(p.b.x, q.b.x, p.b.y * q.b.y)));
}

// dots: partial[i * blocks + b] = B_i . w over the slice of workgroup b.  The thread's four products in
// a fixed order, the wave by an xor tree, the waves in wave order.
__global__ __launch_bounds__(kAT) void svd_dots_kernel(const double* __restrict__ B, size_t ld, int j,
                                                      const double* __restrict__ w, double* __restrict__ partial) {
    __shared__ double s_w[(CF_SVD_MAX_NV + 1) * kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Pair2 wv = load_pair(w, ld);
    for (int i0 = 0; i0 < j; i0 += 4) {   // four vectors' loads in flight; each vector's sum is its own
        Pair2 bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) bv[q] = load_pair(B + (size_t)(i0 + q < j ? i0 + q : i0) * ld, ld);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double acc = pair_dot(bv[q], wv);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0 && i0 + q < j) s_w[(i0 + q) * kWaves + wave] = acc;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < j; i += kAT) {
        double acc = s_w[i * kWaves];
#pragma unroll
        for (int q = 1; q < kWaves; ++q) acc += s_w[i * kWaves + q];
        partial[(size_t)i * gridDim.x + blockIdx.x] = acc;
    }
}

// coef[i] = the sum of partial[i * blocks + b] over the workgroups b: one wave per coefficient, lane
// l takes b = l, l + 64, .. in order, then the xor tree.
__global__ __launch_bounds__(kAT) void svd_dots_sum_kernel(const double* __restrict__ partial, uint32_t n_blocks, int j,
                                                          double* __restrict__ coef) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= j) return;   // whole waves leave
    const double* row = partial + (size_t)i * n_blocks;
    double acc = 0.0;
    for (uint32_t b = lane; b < n_blocks; b += 64) acc += row[b];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) coef[i] = acc;
}

// axpy: w -= sum_i coef[i] B_i, i ascending; NORM: also npart[b] = the slice's part of |w|^2.
template <bool NORM>
__global__ __launch_bounds__(kAT) void svd_axpy_kernel(const double* __restrict__ B, size_t ld, int j,
                                                      const double* __restrict__ coef, double* __restrict__ w,
                                                      double* __restrict__ npart) {
    __shared__ double s_c[CF_SVD_MAX_NV + 1];
    __shared__ double s_v[kAT];
    for (int i = threadIdx.x; i < j; i += kAT) s_c[i] = coef[i];
    __syncthreads();
    Pair2 wv = load_pair(w, ld);
#pragma unroll 4
    for (int i = 0; i < j; ++i) {
        const Pair2 bv = load_pair(B + (size_t)i * ld, ld);
        const double c = s_c[i];
        wv.a.x = fma(-c, bv.a.x, wv.a.x);
        wv.a.y = fma(-c, bv.a.y, wv.a.y);
        wv.b.x = fma(-c, bv.b.x, wv.b.x);
        wv.b.y = fma(-c, bv.b.y, wv.b.y);
    }
    if (j) store_pair(w, ld, wv);
    if (NORM) {
        s_v[threadIdx.x] = pair_dot(wv, wv);
        block_tree_sum(s_v);
        if (threadIdx.x == 0) npart[blockIdx.x] = s_v[0];
    }
}

// The sum of npart[0..n_part) by one workgroup in a fixed order: thread t takes t, t + kAT, ..,
// then the tree.  Every thread returns the sum.
__device__ inline double block_sum_parts(const double* __restrict__ npart, uint32_t n_part, double* s_v) {
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < n_part; i += kAT) acc += npart[i];
    s_v[threadIdx.x] = acc;
    block_tree_sum(s_v);
    return s_v[0];
}

// norm = sqrt(sum npart); w /= norm iff always or norm >= 1e-10; block 0 stores the norm.  Every
// workgroup adds the parts itself, in the same order.
__global__ __launch_bounds__(kAT) void svd_normalize_kernel(double* __restrict__ w, size_t ld,
                                                           const double* __restrict__ npart, uint32_t n_part,
                                                           int always, double* __restrict__ rec) {
    __shared__ double s_v[kAT];
    const double nrm = sqrt(block_sum_parts(npart, n_part, s_v));
    if (blockIdx.x == 0 && threadIdx.x == 0) *rec = nrm;
    if (!always && !(nrm >= kNormFloor)) return;
    Pair2 wv = load_pair(w, ld);
    wv.a.x /= nrm;
    wv.a.y /= nrm;
    wv.b.x /= nrm;
    wv.b.y /= nrm;
    store_pair(w, ld, wv);
}

// npart[b] = the slice's part of |y - sigma z|^2 (svd.cpp:469-473).
__global__ __launch_bounds__(kAT) void svd_resid_kernel(const double* __restrict__ y, const double* __restrict__ z,
                                                       double sigma, size_t ld, double* __restrict__ npart) {
    __shared__ double s_v[kAT];
    Pair2 r = load_pair(y, ld);
    const Pair2 zv = load_pair(z, ld);
    r.a.x -= zv.a.x * sigma;
    r.a.y -= zv.a.y * sigma;
    r.b.x -= zv.b.x * sigma;
    r.b.y -= zv.b.y * sigma;
    s_v[threadIdx.x] = pair_dot(r, r);
    block_tree_sum(s_v);
    if (threadIdx.x == 0) npart[blockIdx.x] = s_v[0];
}

// *rec = sqrt(sum npart): one workgroup.
__global__ __launch_bounds__(kAT) void svd_norm_kernel(const double* __restrict__ npart, uint32_t n_part,
                                                      double* __restrict__ rec) {
    __shared__ double s_v[kAT];
    const double s = block_sum_parts(npart, n_part, s_v);
    if (threadIdx.x == 0) *rec = sqrt(s);
}

// out[:, c] = sum_t X[:, t] C(t, c) for the columns [blockIdx.y kRotCols, ..) of C (m x ncols,
// row-major with stride ldc), t ascending; one vertex per thread.
__global__ __launch_bounds__(kAT) void svd_rotate_kernel(const double* __restrict__ X, size_t ld, int m,
                                                        const double* __restrict__ C, int ldc, int ncols,
                                                        double* __restrict__ out) {
    __shared__ double s_c[CF_SVD_MAX_NV * kRotCols];
    const int c0 = blockIdx.y * kRotCols;
    const int nc = ncols - c0 < kRotCols ? ncols - c0 : kRotCols;
    for (int idx = threadIdx.x; idx < m * kRotCols; idx += kAT) {
        const int t = idx / kRotCols, c = idx % kRotCols;
        s_c[idx] = c < nc ? C[(size_t)t * ldc + c0 + c] : 0.0;
    }
    __syncthreads();
    const size_t v = (size_t)blockIdx.x * kAT + threadIdx.x;
    if (v >= ld) return;
    double acc[kRotCols];
#pragma unroll
    for (int c = 0; c < kRotCols; ++c) acc[c] = 0.0;
    for (int t = 0; t < m; ++t) {
        const double xv = X[(size_t)t * ld + v];
#pragma unroll
        for (int c = 0; c < kRotCols; ++c) acc[c] = fma(xv, s_c[t * kRotCols + c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < kRotCols; ++c)
        if (c < nc) out[(size_t)(c0 + c) * ld + v] = acc[c];
}

// ---- host ---------------------------------------------------------------------------------

inline size_t padded_ld(uint32_t n) { return ((size_t)n + 15) & ~(size_t)15; }
inline uint32_t slice_blocks(size_t ld) { return (uint32_t)((ld + kSlice - 1) / kSlice); }

struct HostLists {
    std::vector<uint32_t> low, wave, grp, high, high_base, seg_vertex, seg_index;
};

// The class lists of one CSR (ascending row order).  false: too many segments.
bool build_lists(uint32_t n, const uint64_t* off, HostLists& h) {
    uint64_t segs = 0;
    for (uint32_t v = 0; v < n; ++v) {
        const uint64_t deg = off[v + 1] - off[v];
        if (deg <= (uint64_t)kLowMax) h.low.push_back(v);
        else if (deg <= (uint64_t)kWaveMax) h.wave.push_back(v);
        else if (deg <= (uint64_t)kSeg) h.grp.push_back(v);
        else {
            const uint64_t nseg = (deg + kSeg - 1) / kSeg;
            if (segs + nseg > 0x7fffffffull) return false;
            h.high.push_back(v);
            h.high_base.push_back((uint32_t)segs);
            for (uint64_t q = 0; q < nseg; ++q) {
                h.seg_vertex.push_back(v);
                h.seg_index.push_back((uint32_t)q);
            }
            segs += nseg;
        }
    }
    return true;
}

struct SideArrays {   // writable views of what MvSide points to
    uint64_t* off;
    uint32_t* nbr;
    float* val;
    uint32_t *low, *wave, *grp, *high, *high_base, *seg_vertex, *seg_index;
};

void carve_side(Carver& c, MvSide& s, SideArrays& a, uint32_t n, uint64_t nnz, const HostLists& h) {
    s.n = n;
    s.off = a.off = c.take<uint64_t>((size_t)n + 1);
    s.nbr = a.nbr = c.take<uint32_t>(nnz);
    s.val = a.val = c.take<float>(nnz);
    s.low = a.low = c.take<uint32_t>(h.low.size());
    s.wave = a.wave = c.take<uint32_t>(h.wave.size());
    s.grp = a.grp = c.take<uint32_t>(h.grp.size());
    s.high = a.high = c.take<uint32_t>(h.high.size());
    s.high_base = a.high_base = c.take<uint32_t>(h.high.size());
    s.seg_vertex = a.seg_vertex = c.take<uint32_t>(h.seg_vertex.size());
    s.seg_index = a.seg_index = c.take<uint32_t>(h.seg_vertex.size());
    s.partial = c.take<double>(h.seg_vertex.size());
    s.n_low = (uint32_t)h.low.size();
    s.n_wave = (uint32_t)h.wave.size();
    s.n_grp = (uint32_t)h.grp.size();
    s.n_high = (uint32_t)h.high.size();
    s.n_seg = (uint32_t)h.seg_vertex.size();
}

template <class T>
int upload(cf_ctx* ctx, T* dst, const T* src, size_t count) {
    if (count) CF_HIP_CHECK(ctx, hipMemcpy(dst, src, sizeof(T) * count, hipMemcpyHostToDevice));
    return CF_OK;
}

int upload_side(cf_ctx* ctx, const SideArrays& a, uint32_t n, uint64_t nnz, const uint64_t* off, const uint32_t* nbr,
                const float* val, const HostLists& h) {
    CF_TRY(upload(ctx, a.off, off, (size_t)n + 1));
    CF_TRY(upload(ctx, a.nbr, nbr, nnz));
    CF_TRY(upload(ctx, a.val, val, nnz));
    CF_TRY(upload(ctx, a.low, h.low.data(), h.low.size()));
    CF_TRY(upload(ctx, a.wave, h.wave.data(), h.wave.size()));
    CF_TRY(upload(ctx, a.grp, h.grp.data(), h.grp.size()));
    CF_TRY(upload(ctx, a.high, h.high.data(), h.high.size()));
    CF_TRY(upload(ctx, a.high_base, h.high_base.data(), h.high_base.size()));
    CF_TRY(upload(ctx, a.seg_vertex, h.seg_vertex.data(), h.seg_vertex.size()));
    CF_TRY(upload(ctx, a.seg_index, h.seg_index.data(), h.seg_index.size()));
    return CF_OK;
}

// y = M x over the CSR of s: at most three launches.
void launch_matvec(const MvSide& s, const double* x, double* y, hipStream_t st) {
    constexpr uint32_t low_rows = kAT / kG, wave_rows = kAT / 64;
    const uint32_t low_blocks = (s.n_low + low_rows - 1) / low_rows, wave_blocks = (s.n_wave + wave_rows - 1) / wave_rows;
    if (low_blocks + wave_blocks)
        hipLaunchKernelGGL(svd_mv_rows_kernel, dim3(low_blocks + wave_blocks), dim3(kAT), 0, st, s, low_blocks, x, y);
    if (s.n_grp + s.n_seg) hipLaunchKernelGGL(svd_mv_group_kernel, dim3(s.n_grp + s.n_seg), dim3(kAT), 0, st, s, x, y);
    if (s.n_high) hipLaunchKernelGGL(svd_mv_finish_kernel, dim3((s.n_high + kAT - 1) / kAT), dim3(kAT), 0, st, s, y);
}

// The vectors of one side and the scratch of the kernels that stream them.
struct VecSide {
    size_t ld;
    uint32_t blocks;      // slice_blocks(ld)
    double* base;         // nv + 1 vectors
    double* tmp;          // one vector (the residual's product)
    double* at(uint32_t i) const { return base + (size_t)i * ld; }
};

struct FitLayout {
    MvSide mv[2];         // 0: the row CSR (y = A x), 1: the column CSR (y = A^T x)
    SideArrays arr[2];
    VecSide vec[2];       // 0: P (row side), 1: Q (column side)
    double* rot;          // (nv + 1) vectors of the longer side
    double* dot_part;     // blocks x (nv + 1)
    double* coef;         // nv + 1
    double* norm_part;    // blocks
    double* cmat;         // nv x (nv + 1)
    double* rec;          // 2 nv + 2 norms
    size_t zero_begin;    // workspace bytes [zero_begin, zero_end): the vectors, cleared before the fit
    size_t zero_end;
};

void carve_fit(Carver& c, FitLayout& f, uint32_t rows, uint32_t cols, uint64_t nnz, uint32_t nv, const HostLists h[2]) {
    carve_side(c, f.mv[0], f.arr[0], rows, nnz, h[0]);
    carve_side(c, f.mv[1], f.arr[1], cols, nnz, h[1]);
    const uint32_t n[2] = {rows, cols};
    f.zero_begin = c.pos;
    for (int k = 0; k < 2; ++k) {
        VecSide& v = f.vec[k];
        v.ld = padded_ld(n[k]);
        v.blocks = slice_blocks(v.ld);
        v.base = c.take<double>(v.ld * ((size_t)nv + 1));
        v.tmp = c.take<double>(v.ld);
    }
    const size_t ldmax = std::max(f.vec[0].ld, f.vec[1].ld);
    const size_t bmax = std::max(f.vec[0].blocks, f.vec[1].blocks);
    f.rot = c.take<double>(ldmax * ((size_t)nv + 1));
    f.zero_end = c.pos;
    f.dot_part = c.take<double>(bmax * ((size_t)nv + 1));
    f.coef = c.take<double>((size_t)nv + 1);
    f.norm_part = c.take<double>(bmax);
    f.cmat = c.take<double>((size_t)nv * ((size_t)nv + 1));
    f.rec = c.take<double>(2 * (size_t)nv + 2);
}

// orthogonalize_vs_all (math.hpp:847-906): vector i of the side against the i vectors before it,
// then the norm into *rec and the division.
void launch_ortho(const FitLayout& f, const VecSide& v, uint32_t i, uint32_t repeats, double* rec, hipStream_t st) {
    double* w = v.at(i);
    const int j = (int)i;
    if (j == 0) {
        hipLaunchKernelGGL(svd_axpy_kernel<true>, dim3(v.blocks), dim3(kAT), 0, st, (const double*)v.base, v.ld, 0,
                           (const double*)f.coef, w, f.norm_part);
    } else {
        for (uint32_t r = 0; r < repeats; ++r) {
            hipLaunchKernelGGL(svd_dots_kernel, dim3(v.blocks), dim3(kAT), 0, st, (const double*)v.base, v.ld, j,
                               (const double*)w, f.dot_part);
            hipLaunchKernelGGL(svd_dots_sum_kernel, dim3((j + kWaves - 1) / kWaves), dim3(kAT), 0, st, (const double*)f.dot_part,
                               v.blocks, j, f.coef);
            if (r + 1 == repeats)
                hipLaunchKernelGGL(svd_axpy_kernel<true>, dim3(v.blocks), dim3(kAT), 0, st, (const double*)v.base, v.ld,
                                   j, (const double*)f.coef, w, f.norm_part);
            else
                hipLaunchKernelGGL(svd_axpy_kernel<false>, dim3(v.blocks), dim3(kAT), 0, st, (const double*)v.base, v.ld,
                                   j, (const double*)f.coef, w, f.norm_part);
        }
    }
    hipLaunchKernelGGL(svd_normalize_kernel, dim3(v.blocks), dim3(kAT), 0, st, w, v.ld, (const double*)f.norm_part,
                       v.blocks, 0, rec);
}

// X[:, first .. first + ncols) = X[:, first .. first + m) C with C (m x ncols, row-major) on the host.
int rotate_side(cf_ctx* ctx, const FitLayout& f, const VecSide& v, uint32_t first, int m, const std::vector<double>& C,
                int ncols, hipStream_t st) {
    CF_HIP_CHECK(ctx, hipMemcpyAsync(f.cmat, C.data(), sizeof(double) * (size_t)m * ncols, hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((v.ld + kAT - 1) / kAT), (unsigned)((ncols + kRotCols - 1) / kRotCols));
    hipLaunchKernelGGL(svd_rotate_kernel, grid, dim3(kAT), 0, st, (const double*)v.at(first), v.ld, m,
                       (const double*)f.cmat, ncols, ncols, f.rot);
    CF_HIP_CHECK(ctx, hipMemcpyAsync(v.at(first), f.rot, sizeof(double) * v.ld * (size_t)ncols, hipMemcpyDeviceToDevice, st));
    CF_HIP_CHECK(ctx, hipStreamSynchronize(st));   // C is read by the copy until here
    return CF_OK;
}

}  // namespace

extern "C" int cf_debug_svd_wave_max(void) { return kWaveMax; }

extern "C" int cf_debug_small_svd(int m, const double* T, double* a, double* b, double* PT) {
    if (m <= 0 || !T || !a || !b || !PT) return CF_EINVAL;
    return cfsvd::small_svd(m, T, a, b, PT);
}

extern "C" int cf_svd_matvec(cf_ctx* ctx, uint32_t n_out, uint32_t n_in, const uint64_t* off, const uint32_t* nbr,
                             const float* val, const double* x, double* y) {
    if (!ctx) return CF_EINVAL;
    if (n_out == 0) return CF_OK;
    if (!off || !y || (n_in && !x)) return cf_set_error(ctx, CF_EINVAL, "cf_svd_matvec: null argument");
    const uint64_t nnz = off[n_out];
    if (nnz && (!nbr || !val)) return cf_set_error(ctx, CF_EINVAL, "cf_svd_matvec: null entry array");
    CF_TRY(check_csr(ctx, "cf_svd_matvec", "matrix", n_out, off, nbr, n_in));
    HostLists h;
    if (!build_lists(n_out, off, h)) return cf_set_error(ctx, CF_ERANGE, "cf_svd_matvec: too many segments");
    CF_TRY(set_device(ctx));
    MvSide s{};
    SideArrays a{};
    double *dx = nullptr, *dy = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Carver c;
        if (pass) c.base = static_cast<char*>(ctx->d_als);
        carve_side(c, s, a, n_out, nnz, h);
        dx = c.take<double>(n_in);
        dy = c.take<double>(n_out);
        if (!pass) CF_TRY(als_reserve(ctx, c.pos));
    }
    CF_TRY(upload_side(ctx, a, n_out, nnz, off, nbr, val, h));
    CF_TRY(upload(ctx, dx, x, (size_t)n_in));
    launch_matvec(s, dx, dy, nullptr);
    CF_HIP_CHECK(ctx, hipGetLastError());
    CF_HIP_CHECK(ctx, hipMemcpy(y, dy, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    return CF_OK;
}

extern "C" int cf_svd_fit(cf_ctx* ctx, uint32_t rows, uint32_t cols, const uint64_t* row_off, const uint32_t* row_col,
                          const float* row_val, const uint64_t* col_off, const uint32_t* col_row, const float* col_val,
                          uint32_t nsv, uint32_t nv, uint32_t max_iter, double tol, uint32_t ortho_repeats,
                          const double* v0, double* sigma, double* errest, double* err, double* U, double* V,
                          uint32_t* kk_pass, double* first_ab, cf_svd_stats* stats) {
    if (!ctx) return CF_EINVAL;
    if (stats) *stats = cf_svd_stats{};
    if (nsv == 0) return cf_set_error(ctx, CF_EINVAL, "cf_svd_fit: nsv = 0");
    if (nv < nsv) return cf_set_error(ctx, CF_EINVAL, "cf_svd_fit: nv < nsv");
    if (ortho_repeats < 1 || ortho_repeats > 3)
        return cf_set_error(ctx, CF_EINVAL, "cf_svd_fit: ortho_repeats must be 1, 2 or 3");
    if (nv > CF_SVD_MAX_NV) return cf_set_error(ctx, CF_ERANGE, "cf_svd_fit: nv above CF_SVD_MAX_NV");
    if (rows == 0 || cols == 0) return CF_OK;
    if (!row_off || !col_off || !v0 || !sigma || !errest || !err || !U || !V)
        return cf_set_error(ctx, CF_EINVAL, "cf_svd_fit: null argument");
    bool v0_zero = true;
    for (uint32_t i = 0; i < rows && v0_zero; ++i) v0_zero = v0[i] == 0.0;
    if (v0_zero) return cf_set_error(ctx, CF_EINVAL, "cf_svd_fit: the initial vector is zero");
    uint64_t nnz = 0;
    CF_TRY(check_two_csr(ctx, "cf_svd_fit", rows, cols, 1, row_off, row_col, row_val, col_off, col_row, col_val, &nnz));
    HostLists h[2];
    if (!build_lists(rows, row_off, h[0]) || !build_lists(cols, col_off, h[1]))
        return cf_set_error(ctx, CF_ERANGE, "cf_svd_fit: too many segments");
    CF_TRY(set_device(ctx));

    // everything the fit needs exists before its first launch
    FitLayout f{};
    {
        Carver size;
        carve_fit(size, f, rows, cols, nnz, nv, h);
        CF_TRY(als_reserve(ctx, size.pos));
        Carver c;
        c.base = static_cast<char*>(ctx->d_als);
        carve_fit(c, f, rows, cols, nnz, nv, h);
    }
    MfEvents<3> evs;
    for (hipEvent_t& e : evs.e) CF_HIP_CHECK(ctx, hipEventCreate(&e));
    hipStream_t st = nullptr;
    CF_TRY(upload_side(ctx, f.arr[0], rows, nnz, row_off, row_col, row_val, h[0]));
    CF_TRY(upload_side(ctx, f.arr[1], cols, nnz, col_off, col_row, col_val, h[1]));
    CF_HIP_CHECK(ctx, hipMemset(static_cast<char*>(ctx->d_als) + f.zero_begin, 0, f.zero_end - f.zero_begin));
    const VecSide& P = f.vec[0];
    const VecSide& Q = f.vec[1];
    CF_TRY(upload(ctx, P.at(0), v0, (size_t)rows));
    // P[0] = v0 / |v0| (svd.cpp:323-324: divided whatever the norm)
    hipLaunchKernelGGL(svd_axpy_kernel<true>, dim3(P.blocks), dim3(kAT), 0, st, (const double*)P.base, P.ld, 0,
                       (const double*)f.coef, P.at(0), f.norm_part);
    hipLaunchKernelGGL(svd_normalize_kernel, dim3(P.blocks), dim3(kAT), 0, st, P.at(0), P.ld,
                       (const double*)f.norm_part, P.blocks, 1, f.rec);

    double ms[3] = {0.0, 0.0, 0.0};   // product, orthogonalisation, rotation
    uint32_t products = 0, passes = 0, nconv = 0, its = 1;
    // one Lanczos step: vector i of side k = (its CSR) x, orthogonalised; returns the norm
    auto step = [&](int k, uint32_t i, const double* x, double* norm) -> int {
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
        launch_matvec(f.mv[k], x, f.vec[k].at(i), st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
        launch_ortho(f, f.vec[k], i, ortho_repeats, f.rec, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[2], st));
        CF_HIP_CHECK(ctx, hipGetLastError());
        CF_HIP_CHECK(ctx, hipMemcpy(norm, f.rec, sizeof(double), hipMemcpyDeviceToHost));   // the step's one record
        float a = 0.0f, b = 0.0f;
        (void)hipEventElapsedTime(&a, evs.e[0], evs.e[1]);
        (void)hipEventElapsedTime(&b, evs.e[1], evs.e[2]);
        ms[0] += a;
        ms[1] += b;
        ++products;
        return CF_OK;
    };

    std::vector<double> alpha(nv), beta(nv), T, a_mat, b_vec, pt_mat, C;
    bool finished = false;
    while (nconv < nsv && its < max_iter) {   // svd.cpp:327: at most max_iter - 1 passes
        const uint32_t k = nconv, n = nv;
        std::fill(alpha.begin(), alpha.end(), 0.0);
        std::fill(beta.begin(), beta.end(), 0.0);
        CF_TRY(step(1, k, P.at(k), &alpha[0]));
        for (uint32_t i = k + 1; i < n; ++i) {
            CF_TRY(step(0, i, Q.at(i - 1), &beta[i - k - 1]));
            CF_TRY(step(1, i, P.at(i), &alpha[i - k]));
        }
        CF_TRY(step(0, n, Q.at(n - 1), &beta[n - k - 1]));
        if (passes == 0 && first_ab) {
            std::copy(alpha.begin(), alpha.end(), first_ab);
            std::copy(beta.begin(), beta.end(), first_ab + nv);
        }

        // the SVD of the bidiagonal T (svd.cpp:378-383) and the error estimates (:393-417)
        const int m = (int)(nv - nconv);
        T.assign((size_t)m * m, 0.0);
        for (int i = 0; i < m; ++i) {
            T[(size_t)i * m + i] = alpha[i];
            if (i + 1 < m) T[(size_t)i * m + i + 1] = beta[i];
        }
        a_mat.resize((size_t)m * m);
        pt_mat.resize((size_t)m * m);
        b_vec.resize(m);
        cfsvd::small_svd(m, T.data(), a_mat.data(), b_vec.data(), pt_mat.data());
        uint32_t kk = 0;
        for (int j = 0; j < m; ++j) {
            sigma[nconv + j] = b_vec[j];
            double e = std::fabs(a_mat[(size_t)(m - 1) * m + j] * beta[m - 1]);
            if (b_vec[j] > tol) e /= b_vec[j];
            errest[nconv + j] = e;
            if (e < tol) ++kk;
        }
        if (nconv + kk >= nsv) finished = true;
        if (kk_pass) kk_pass[passes] = kk;

        // the Ritz vectors of the converged triplets and, unless finished, the new start vector as
        // one more column: P[:, nconv .. nconv + kk] = P[:, nconv .. nv) PT[:, 0 .. kk]
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
        const int pcols = (int)kk + (finished ? 0 : 1);
        if (pcols) {
            C.resize((size_t)m * pcols);
            for (int t = 0; t < m; ++t)
                for (int c = 0; c < pcols; ++c) C[(size_t)t * pcols + c] = pt_mat[(size_t)t * m + c];
            CF_TRY(rotate_side(ctx, f, P, nconv, m, C, pcols, st));
        }
        if (kk) {
            C.resize((size_t)m * kk);
            for (int t = 0; t < m; ++t)
                for (uint32_t c = 0; c < kk; ++c) C[(size_t)t * kk + c] = a_mat[(size_t)t * m + c];
            CF_TRY(rotate_side(ctx, f, Q, nconv, m, C, (int)kk, st));
        }
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
        CF_HIP_CHECK(ctx, hipEventSynchronize(evs.e[1]));
        float r = 0.0f;
        (void)hipEventElapsedTime(&r, evs.e[0], evs.e[1]);
        ms[2] += r;
        nconv += kk;
        ++passes;
        if (finished) break;
        ++its;
    }

    // the residual norms of the reported triplets (svd.cpp:468-484)
    const uint32_t n_out = std::min(nsv, nconv);
    for (uint32_t i = 0; i < n_out; ++i) {
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[0], st));
        launch_matvec(f.mv[1], P.at(i), Q.tmp, st);
        launch_matvec(f.mv[0], Q.at(i), P.tmp, st);
        CF_HIP_CHECK(ctx, hipEventRecord(evs.e[1], st));
        hipLaunchKernelGGL(svd_resid_kernel, dim3(Q.blocks), dim3(kAT), 0, st, (const double*)Q.tmp,
                           (const double*)Q.at(i), sigma[i], Q.ld, f.norm_part);
        hipLaunchKernelGGL(svd_norm_kernel, dim3(1), dim3(kAT), 0, st, (const double*)f.norm_part, Q.blocks, f.rec);
        hipLaunchKernelGGL(svd_resid_kernel, dim3(P.blocks), dim3(kAT), 0, st, (const double*)P.tmp,
                           (const double*)P.at(i), sigma[i], P.ld, f.norm_part);
        hipLaunchKernelGGL(svd_norm_kernel, dim3(1), dim3(kAT), 0, st, (const double*)f.norm_part, P.blocks, f.rec + 1);
        CF_HIP_CHECK(ctx, hipGetLastError());
        double n12[2];
        CF_HIP_CHECK(ctx, hipMemcpy(n12, f.rec, sizeof(n12), hipMemcpyDeviceToHost));
        float a = 0.0f;
        (void)hipEventElapsedTime(&a, evs.e[0], evs.e[1]);
        ms[0] += a;
        products += 2;
        double e = std::sqrt(n12[0] * n12[0] + n12[1] * n12[1]);
        if (sigma[i] > tol) e /= sigma[i];
        err[i] = e;
    }
    CF_HIP_CHECK(ctx, hipDeviceSynchronize());
    if (n_out) {
        CF_HIP_CHECK(ctx, hipMemcpy2D(U, sizeof(double) * rows, P.base, sizeof(double) * P.ld, sizeof(double) * rows,
                                      n_out, hipMemcpyDeviceToHost));
        CF_HIP_CHECK(ctx, hipMemcpy2D(V, sizeof(double) * cols, Q.base, sizeof(double) * Q.ld, sizeof(double) * cols,
                                      n_out, hipMemcpyDeviceToHost));
    }
    if (stats) {
        stats->nconv = nconv;
        stats->passes = passes;
        stats->products = products;
        stats->matvec_ms = (float)ms[0];
        stats->ortho_ms = (float)ms[1];
        stats->rotate_ms = (float)ms[2];
    }
    return CF_OK;
}
