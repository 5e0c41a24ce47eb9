/*
 * cf_abi.h -- C ABI of libcf_mi355x.so, the MI355X-native hot path of
 * Dhole/collaborative_filtering (per-user local-graph Laplacian eigendecomposition,
 * graph-signal rating prediction, kNN item similarity).
 *
 * Conventions
 *   - Every entry point returns CF_OK (0) or a negative CF_E* code; a message is
 *     available from cf_last_error(ctx).  No C++ exception crosses this boundary.
 *   - Plain pointers and sizes only.  Functions without a suffix take HOST pointers
 *     (caller-owned, copied in/out, synchronous).  *_run functions take DEVICE
 *     pointers and a hipStream_t passed as void* (NULL = default stream) and are
 *     asynchronous on that stream.
 *   - One cf_ctx per GPU; a context is not thread-safe (callers serialise).
 *   - Item ids at this boundary are COMPACT indices 0..n_items-1 into the uploaded
 *     item graph; the host layer maps the reference's movie ids onto them.
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   cf_item_graph_upload[_dense] : the dense `weights` matrix load of
 *                                  precompute_local_threads.cpp:253-293 and the
 *                                  out_fin_ graph_loader of local_calc_precomp.cpp:122-136
 *   cf_eigen_batch / cf_eigen_run : compute_eigens(), precompute_local_threads.cpp:100-213
 *                                  (scheduled per user at :306-314)
 *   cf_predict_precomp / cf_predict_run : neigh_program::apply,
 *                                  local_calc_precomp.cpp:217-380 (per (movie,user) rating)
 *   cf_item_cosine               : weights_calc() via graph.transform_edges, knn2.cpp:127-146,206
 *                                  plus the w > 0.01 writer filter knn2.cpp:155-163
 *   cf_local_calc                : vertex_program::apply of local_calc.cpp:262-526 (per
 *                                  movie local graph, eigensolve, per-user w_lim, predict)
 *   cf_knn_predict               : knn_program gather/apply + error_vertex_data,
 *                                  knn3.cpp:185-256
 *   cf_als_fit / _error / _predict : als_vertex_program, error_aggregator and prediction_saver,
 *                                  als.cpp:290-371,424-510
 *   cf_sgd_fit / _error / _predict : sgd_vertex_program / biassgd_vertex_program with their
 *                                  error_aggregator and prediction_saver, sgd.cpp:243-339,344-425
 *                                  and biassgd.cpp:249-347,399-434
 *   cf_svdpp_fit / _predict        : svdpp_vertex_program and prediction_saver, svdpp.cpp:268-397,
 *                                  479-499 (its error_aggregator is cf_sgd_error)
 *   cf_svd_fit / cf_svd_matvec     : lanczos() with Axb and orthogonalize_vs_all, svd.cpp:304-505,
 *                                  math.hpp:98-185,805-906
 *   cf_mf_topn                     : none (the reference saves PREDICT edges only, als.cpp:493-510);
 *                                  the N best unrated items per user from the fitted factors
 *   cf_mf_rank_eval                : none (no program of the reference ranks held-out items); the
 *                                  rank of every held-out edge and precision / recall / NDCG / MAP /
 *                                  MRR / AUC / expected percentile rank from the fitted factors
 *   cf_knn_topn                    : none: knn3 scores listed pairs only
 *   cf_knn_rank_eval               : none: knn3 scores listed pairs only
 *   cf_ease_fit / _topn / _rank_eval : none: the closed-form item-item model (EASE)
 */
#ifndef CF_ABI_H
#define CF_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CF_OK 0
#define CF_EINVAL (-1)  /* bad argument / size */
#define CF_ENOMEM (-2)  /* device or host allocation failed */
#define CF_EHIP (-3)    /* HIP runtime or kernel launch error */
#define CF_ERANGE (-4)  /* problem size outside the supported buckets */
#define CF_ESTATE (-5)  /* missing prerequisite (e.g. no item graph uploaded) */

#define CF_MAX_K 192    /* largest per-user item count handled by the LDS eigen path */
#define CF_SPILL_MAX_K 5000  /* largest k of the spill paths' LDS layouts (fp64, HBM workspace);
                                larger k (no cap, as the reference) takes their HUGE layouts, every
                                k-long vector in HBM, bounded by HBM only (CF_ENOMEM) */

typedef struct cf_ctx cf_ctx;
typedef struct cf_plan cf_plan;

/* ---- context --------------------------------------------------------------- */
int cf_version(void);
/* Number of visible GPUs (0 when none or on error). */
int cf_device_count(void);
int cf_create(int device, cf_ctx** out);
void cf_destroy(cf_ctx* ctx);
/* Waits for the context's device, then frees its cached HBM workspaces (eigen and predictor
 * spill paths, the tridiagonal path, the predictor scratch, the knn2 planes, ALS / SGD / SVD++ / SVD / top-N); each is
 * allocated again, at the size its next call plans, when that call runs.  The spill paths
 * size their workspaces from the device's free HBM, so a workspace the predictor left behind
 * shrinks the next eigen call's and costs it waves: call this between stages of a long-lived
 * context (bench.py's config-5 legs).  No reference counterpart (one call per process there). */
int cf_release_workspaces(cf_ctx* ctx);
const char* cf_last_error(const cf_ctx* ctx);
/* Eigensolver of the k <= CF_MAX_K users: CF_EIGEN_JACOBI (default; one-sided Jacobi in
 * LDS, cf_eigen.hip) or CF_EIGEN_TRIDIAG (Householder + batched QL, cf_eigen_tri.hip). */
#define CF_EIGEN_TRIDIAG 0
#define CF_EIGEN_JACOBI 1
int cf_set_eigen_method(cf_ctx* ctx, int method);
/* Jacobi off-diagonal tolerance scale (default 1.0) and sweep cap (default 30). */
int cf_set_jacobi(cf_ctx* ctx, float tol_scale, int max_sweeps);
/* compute_eigens (precompute_local_threads.cpp:164-166) on the LDS Jacobi path: sweeps until
 * one rotates no pair by more than stop_rel (relative off-diagonal |b_p.b_q| / |b_p||b_q|),
 * then one first-order Gram refinement on the matrix cores for every pair whose eigenvalues
 * are more than delta apart.  Defaults: enable 1, stop_rel 1e-3, delta 1e-2; pairs closer than delta sweep to 8 tol.
 * enable 0 restores the sweeps-only rule (stop after a sweep with no rotation above 16 tol). */
int cf_set_eigen_refine(cf_ctx* ctx, int enable, float stop_rel, float delta);
/* LDS Jacobi, split layout: the sweeps of the users in buckets emax >= the minimum run
 * with the fixed column of every pair in registers and only the traveling half in LDS, several users
 * per CU, and the refinement and epilogue in the full-LDS kernel.  enable: 0 off (everything in the
 * full-LDS kernel), 1 the default minimum bucket (9: k > 128), 5..12 an explicit minimum; env
 * CF_EIGEN_SPLIT sets the same.  Same algorithm, same outputs up to the rotation order inside odd
 * segments.  Same call site as cf_eigen_run. */
int cf_set_eigen_split(cf_ctx* ctx, int enable);
/* LDS Jacobi, full-LDS kernel, buckets 1-8 (k <= 128; DESIGN 3.1's geometry table): lanes per column
 * pair.  0 (default) takes the measured best of every bucket, 4 or 8 forces that count in every
 * bucket 1-8; env CF_EIGEN_LANES sets the same.  The 4-lane form gives a lane the rows of two lanes
 * of the 8-lane form and keeps every reduction's tree, so the outputs are bit-identical either way.
 * Buckets 9-12 and the split layout always use 8. */
int cf_set_eigen_lanes(cf_ctx* ctx, int lanes);
/* Host only (no device): the geometry a lanes setting (0 | 4 | 8) launches for LDS bucket emax (1-12):
 * lanes per pair, threads per block, leading dimension of B in floats, LDS bytes per block, and the
 * users per CU the block and its register budget are sized for.  CF_EINVAL outside those ranges. */
int cf_debug_eigen_geometry(int emax, int lanes_setting, int* lanes, int* threads, int* ld, int* lds_bytes,
                            int* users_per_cu);
/* Predictor fast path, lane packing: mode 1 (default) runs the per-rating systems of
 * n = min(nc, d) <= 14 rows four to a wave and those of 15..30 rows two to a wave; mode 0 gives every
 * rating a wave of its own.  Outputs are bit-identical either way; env CF_PRED_PACK sets the same.
 * Applies to cf_predict_run*, cf_predict_precomp and cf_step_run. */
int cf_set_pred_pack(cf_ctx* ctx, int mode);
/* Host only (no device): builds and verifies the split layout's sweep schedule for k columns in
 * LDS bucket emax (every pair of columns meets once per sweep, no two lane groups touch one LDS
 * slot in a level change, register groups and slots within capacity).  Returns CF_OK and the
 * steps per sweep, levels, and the largest register-group and slot counts of any level, or
 * CF_ERANGE when the split layout does not take k (those users keep the full-LDS kernel). */
int cf_debug_split_schedule(int emax, int k, int* steps, int* levels, int* max_groups, int* max_slots);
/* Complement-mask handoff (default on): an eigen run over a plan (cf_eigen_run, cf_step_run)
 * also writes, per rating, the 3 x 64-bit mask of the user's items that are NOT out-neighbours
 * (w <= 0.1) of that item, from the graph entries it gathers anyway (24 B per rating of HBM,
 * owned by the context); a later cf_predict_run* over the same plan, the same item arrays and the
 * same graph reads them instead of re-gathering k^2 graph entries per user.  Outputs are
 * bit-identical either way.  enable 0 frees nothing but makes every predictor run gather.
 * Replaces the per-rating neighbour scan of local_calc_precomp.cpp:254-265. */
int cf_set_step_masks(cf_ctx* ctx, int enable);
/* cf_local_calc, units with n > CF_MAX_K: bisect != 0 (default) computes the w_lim of a
 * (movie, test user) pair with c <= 184 rated rows from the eigenpairs of the movie's
 * B = L2 L2^T, shared by all its pairs (Haynsworth inertia count, bisection);
 * bisect 0 tridiagonalises each pair's L2_h L2_h^T as local_calc.cpp:425-436 spells it out.
 * Both return sqrt(lambda_min(L2_h L2_h^T)). */
int cf_set_local_wlim(cf_ctx* ctx, int bisect);
/* Diagnostics: enable != 0 allocates device counters that the eigen kernel fills;
 * out8 (optional) receives and resets {sum of sweeps, users, max sweeps, users that
 * hit the sweep cap, assembly cycles, Jacobi cycles, epilogue cycles, tournament
 * steps} (cycles: s_memtime of thread 0).  enable == 0 frees them. */
int cf_debug_stats(cf_ctx* ctx, int enable, uint64_t* out8);
/* Diagnostics of the eigen spill path (k > CF_MAX_K): enable != 0 makes its kernel sum
 * s_memtime cycles of thread 0 per phase; out8 (optional) receives and resets {users,
 * assembly, tridiagonalisation, Q accumulation, QL (total), QL rotation generation
 * (serial part), QL iterations, output} cycles. */
int cf_debug_spill(cf_ctx* ctx, int enable, uint64_t* out8);
/* Diagnostics of the tridiagonal eigen path: enable != 0 makes its kernels count;
 * out8 (optional) receives and resets {rotations, QL iterations, record overflows (users
 * recomputed by Jacobi), users, then thread-0 s_memtime cycles of the reduction kernel:
 * assembly, Householder steps, Q accumulation, and the sum of k}. */
int cf_debug_tri(cf_ctx* ctx, int enable, uint64_t* out8);
/* Diagnostics: predictor phase totals in s_memtime cycles.  out16[0..7], thread 0 of
 * each block: {per-user setup, basis, fast-path ratings, block-wide ratings} cycles,
 * the number of ratings taken by the fast path and by the block-wide paths, then the
 * cycles of the per-user Gbar GEMM and of the block-wide K path (a subset of the
 * block-wide cycles).  out16[8..15], summed over every wave: fast-path cycles in
 * {P/PG/PH gathers and border rows, LDL^T of K, the whole fast phase}, the cycles of
 * completed fast-path ratings whose system has n = min(nc, d) <= 14, 15..30 and > 30 rows
 * (a packed group's cycles once, under its class), and the counts of the first two classes. */
int cf_debug_phases(cf_ctx* ctx, int enable, uint64_t* out16);
/* The predictor's fast-path system bound (rows min(nc, d)) in a k-bucket whose
 * Gram bound is lmax = 16 ceil(k / 16): ratings above it take the block-wide path.  -1 if
 * lmax is out of range.  (Test / diagnostics helper.) */
int cf_debug_predict_nmax(int lmax);
/* Per-bucket device time of compute_eigens (cf_eigen_run / cf_eigen_batch, Jacobi path):
 * enable != 0 records a HIP event pair around every LDS k-bucket launch on the stream it is
 * launched on (bucket e holds 16(e-1) < k <= 16e; e = 12 is eigen_kernel<12, narrow>, the
 * dominant kernel of the C4 step).  ms13 (optional) receives, after the recorded work has
 * finished, the mean milliseconds of each bucket's launch over the eigen runs since the last
 * read (at most the last 16; -1: not launched; [0] unused: the spill bucket runs on its own
 * streams) and clears the record.  Launches of
 * other buckets may co-run on the second stream, so these are the kernels' in-step
 * durations, as a profiler's per-dispatch trace shows them. */
int cf_eigen_bucket_timing(cf_ctx* ctx, int enable, float* ms13);
/* As cf_eigen_bucket_timing; sweeps_ms13[e] (optional) also receives, for buckets that ran in the
 * split layout, the mean ms from the bucket's start to the end of its sweep kernel
 * (split_sweep_kernel<e>; the rest of the bucket is eigen_kernel<e, .., RESUME>), else -1. */
int cf_eigen_bucket_timing_split(cf_ctx* ctx, int enable, float* ms13, float* sweeps_ms13);

/* ---- item graph (out_fin_) ---------------------------------------------------
 * Directed weighted graph exactly as parsed: w(a,b) and w(b,a) are independent.
 * HBM-resident in one of two layouts (cf_set_graph_layout, applies to the next upload):
 *   CF_GRAPH_DENSE (default) n_items x n_items fp32, direct indexing (the reference's own
 *                  dense `weights`, precompute_local_threads.cpp:255; ~250k items per GPU);
 *   CF_GRAPH_CSR   row pointers (u64), ascending columns (u32), weights (f32); every lookup
 *                  is a binary search of the row (the GraphLab out-edge lists,
 *                  local_calc_precomp.cpp:122-136): catalogues whose dense matrix does not fit.
 * Every kernel reads the same floats from either layout, so results are bit-identical.
 * A duplicate (a, b) keeps its LAST weight in input order (precompute_local_threads.cpp:284). */
#define CF_GRAPH_DENSE 0
#define CF_GRAPH_CSR 1
int cf_set_graph_layout(cf_ctx* ctx, int layout);
/* Layout, size and (CSR) stored edges of the resident graph. */
int cf_graph_info(const cf_ctx* ctx, int* layout, uint32_t* n_items, uint64_t* nnz);
int cf_item_graph_upload(cf_ctx* ctx, uint32_t n_items, const uint64_t* row_ptr,
                         const uint32_t* col, const float* w);
/* w_dense: n_items*n_items row-major; on_device != 0 means w_dense is a device
 * pointer that the context adopts by copy. */
int cf_item_graph_upload_dense(cf_ctx* ctx, uint32_t n_items, const float* w_dense,
                               int on_device);
/* Device pointer of the resident dense graph (for *_run callers), or NULL (none, or CSR). */
const float* cf_item_graph_device(const cf_ctx* ctx, uint32_t* n_items);

/* ---- user batch plan -----------------------------------------------------------
 * Buckets users by item count k (host item_off[n_users+1]); reused by eigen and
 * predict runs over the same user batch. */
int cf_plan_create(cf_ctx* ctx, uint32_t n_users, const uint64_t* item_off, cf_plan** out);
void cf_plan_destroy(cf_plan* plan);
/* Eigenvector slot size of a user with k items: k*max(k,2) floats. */
uint64_t cf_evec_slots(uint32_t k);
/* Fills evec_off[n_users] (prefix sum of cf_evec_slots) and returns the total. */
uint64_t cf_evec_offsets(uint32_t n_users, const uint64_t* item_off, uint64_t* evec_off);

/* ---- eigen stage: compute_eigens (precompute_local_threads.cpp:100-213) --------
 * Per user u with k = item_off[u+1]-item_off[u] items (sorted ascending compact ids;
 * that order is the row order of the user's block):
 *   sigs [item_off[u] + i]   i < k  : (float)(sig_min_i + 0.01)             (:169-177)
 *   evals[item_off[u] + j]   j < m  : eigenvalues of L2, ascending          (:164-166,193)
 *   evecs[evec_off[u] + i*m + j]    : eigenvector j, row i (k x m row-major) (:194,205-209)
 *   m_out[u]                        : lim, the stored eigenpair count       (:185-191)
 * k == 1 gives m == 2 with zero padding (reference: uninitialised, :193-194).
 * Device memory is bounded: the users run as the chunks of cf_eigen_batch_stream (below), each
 * chunk's blocks copied into the caller's arrays; only the host arrays scale with n_users. */
int cf_eigen_batch(cf_ctx* ctx, uint32_t n_users, const uint64_t* item_off,
                   const uint32_t* items, const uint64_t* evec_off, int32_t* m_out,
                   float* sigs, float* evals, float* evecs);
int cf_eigen_run(cf_ctx* ctx, const cf_plan* plan, const uint64_t* d_item_off,
                 const uint32_t* d_items, const uint64_t* d_evec_off, int32_t* d_m,
                 float* d_sigs, float* d_evals, float* d_evecs, void* stream);

/* ---- compute_eigens over any number of users at bounded memory ------------------
 * The reference runs one compute_eigens task per user and appends each record to out_eigen_
 * as it completes (precompute_local_threads.cpp:89-98, 306-314), so its memory does not grow
 * with the user count.  cf_eigen_batch_stream cuts users 0..n_users-1 (input order) into
 * contiguous chunks whose eigenvector slots (cf_evec_slots) fit chunk_bytes (0: a fifth of
 * the first context's HBM share, at most a quarter of host RAM (<= 64 GB) over the staging
 * sets), solves each chunk on the next free context (one per GPU, each with the graph
 * uploaded), packs its k x m blocks on the device and calls sink(sink_user, chunk) once per
 * chunk, in user order, from the calling thread, while the devices solve the next chunks.
 * The chunk's arrays live until the sink returns:
 *   item_off[count + 1]    chunk-local (item_off[0] = 0): user first+u has k = item_off[u+1] -
 *                          item_off[u] items, its sigs / evals at item_off[u] (as cf_eigen_batch)
 *   m[count], sigs, evals  as cf_eigen_batch
 *   packed_off[count + 1]  user first+u's k x m row-major block at evecs + packed_off[u]
 * A nonzero sink return stops the call (returned if negative, else CF_EINVAL).  The records
 * equal one cf_eigen_batch over all users bit for bit, for every chunk size and device count.
 * The contexts' eigen workspaces are released at the end (one-shot call).  stats (optional):
 * chunk count, the budget used, the largest chunk's slot bytes, and the peaks of the call's
 * own device bytes (its buffers + the contexts' workspaces) and of the device-wide bytes in
 * use (hipMemGetInfo, after each chunk's solve). */
typedef struct cf_eigen_chunk {
    uint32_t first;
    uint32_t count;
    const uint64_t* item_off;
    const int32_t* m;
    const float* sigs;
    const float* evals;
    const uint64_t* packed_off;
    const float* evecs;
} cf_eigen_chunk;
typedef int (*cf_eigen_sink)(void* sink_user, const cf_eigen_chunk* chunk);
typedef struct cf_eigen_stream_stats {
    uint32_t chunks;
    uint64_t chunk_slot_bytes;
    uint64_t max_chunk_slot_bytes;
    uint64_t own_peak_bytes;
    uint64_t device_peak_bytes;
} cf_eigen_stream_stats;
int cf_eigen_batch_stream(cf_ctx* const* ctxs, int n_dev, uint32_t n_users, const uint64_t* item_off,
                          const uint32_t* items, uint64_t chunk_bytes, cf_eigen_sink sink, void* sink_user,
                          cf_eigen_stream_stats* stats);

/* ---- multi-GPU eigen stage and the out_eigen_ gather ----------
 * Replaces the thread pool of precompute_local_threads.cpp:300-314 and the single shared
 * out_eigen_ (:196-211, read whole by every rank at local_calc_precomp.cpp:485-486,509).
 *
 * cf_cost_split: contiguous split points split[0..n_parts] of users 0..n_users-1 balancing
 * sum(k^3): split[p] = first user whose prefix cost reaches p/n_parts of the total.
 *
 * cf_pack_eigen_run: packs the k x m blocks of users 0..n_users-1 (stored in their
 * cf_evec_slots slots at d_evec_off by cf_eigen_run) into one contiguous run:
 *   d_packed_off[u] = sum_{v<u} k_v m_v  (n_users + 1 entries, u64, device)
 *   d_packed[d_packed_off[u] + i*m_u + j] = d_evecs[d_evec_off[u] + i*m_u + j]
 * With d_packed == NULL only the offsets are written (size the buffer from entry n_users).
 *
 * cf_eigen_batch_multi: cf_eigen_batch over ONE global user set on n_dev contexts (one per
 * GPU, each with the item graph uploaded; several contexts may share a device).  Users are
 * split by cf_cost_split, every context computes and packs its range concurrently, and the
 * ranges are gathered to ctxs[0]'s device by peer copies over xGMI.  Outputs as
 * cf_eigen_batch (m_out, sigs, evals at item_off) except the eigenvectors, which arrive
 * packed: packed_off[n_users + 1] as above and packed_evecs (capacity packed_cap floats;
 * the slot total of cf_evec_offsets always suffices).  split_out (optional, n_dev + 1)
 * receives the ranges.  The records are identical to the one-device run's. */
int cf_cost_split(uint32_t n_users, const uint64_t* item_off, int n_parts, uint32_t* split);
int cf_pack_eigen_run(cf_ctx* ctx, uint32_t n_users, const uint64_t* d_item_off, const int32_t* d_m,
                      const uint64_t* d_evec_off, const float* d_evecs, uint64_t* d_packed_off,
                      float* d_packed, void* stream);
int cf_eigen_batch_multi(cf_ctx* const* ctxs, int n_dev, uint32_t n_users, const uint64_t* item_off,
                         const uint32_t* items, int32_t* m_out, float* sigs, float* evals,
                         uint64_t* packed_off, float* packed_evecs, uint64_t packed_cap,
                         uint32_t* split_out);

/* ---- prediction stage: neigh_program::apply (local_calc_precomp.cpp:217-380) ----
 * For every user u and every row r < k of the user's block (test movie items[r] with
 * test rating ratings[item_off[u]+r]):
 *   mse[item_off[u]+r]  = (float)(rating - clamp(pred,1,5))^2     (:307-327,358)
 *   kk [item_off[u]+r]  = number of the user's items that are out-neighbours of the
 *                         movie with w > 0.1 (:132,254-265,359)
 *   pred[item_off[u]+r] = clamp(pred,1,5) (optional, may be NULL)
 * w_lim for row r:
 *   sig_mode CF_SIGS_COMPAT: sigtab[r]  -- the reference's accumulating sigs_min
 *                            vector (:414,437,440,271) reduces to the global
 *                            concatenation of all records' sigs in file order;
 *   sig_mode CF_SIGS_OWN:    sigtab[item_off[u]+r] -- the user's own sigs.
 * evecs are fp64 (parsed out_eigen_) or fp32 (device-resident eigen output). */
#define CF_SIGS_OWN 0
#define CF_SIGS_COMPAT 1
int cf_predict_precomp(cf_ctx* ctx, uint32_t n_users, const uint64_t* item_off,
                       const uint32_t* items, const float* ratings, const int32_t* m,
                       const double* evals, const uint64_t* evec_off, const double* evecs,
                       const double* sigtab, uint64_t sigtab_len, int sig_mode,
                       float* mse, int32_t* kk, double* pred);
/* cf_predict_precomp over the rows with row_sel[item_off[u] + r] != 0 only (row_sel NULL =
 * every row); the other rows' mse / kk / pred keep the values the caller passed in.  This is
 * the per-vertex sampling of local_calc_precomp --pct (rand() % 100 < pct before apply,
 * local_calc_precomp.cpp:221): unsampled movies cost no per-rating work. */
int cf_predict_precomp_sel(cf_ctx* ctx, uint32_t n_users, const uint64_t* item_off,
                           const uint32_t* items, const float* ratings, const int32_t* m,
                           const double* evals, const uint64_t* evec_off, const double* evecs,
                           const double* sigtab, uint64_t sigtab_len, int sig_mode,
                           const uint8_t* row_sel, float* mse, int32_t* kk, double* pred);
/* cf_predict_precomp_sel over ONE user set on n_dev contexts (one per GPU, each with the item
 * graph uploaded; several may share a device), for local_calc_precomp on several GPUs
 * (local_calc_precomp.cpp:485-486,509: every rank holds the whole out_eigen_).  Users are split
 * by cf_cost_split; each context predicts its range concurrently.  In CF_SIGS_COMPAT mode every
 * range reads the same global sig table, so the outputs are bit-identical to the one-context
 * call.  split_out (optional, n_dev + 1) receives the ranges. */
int cf_predict_precomp_multi(cf_ctx* const* ctxs, int n_dev, uint32_t n_users, const uint64_t* item_off,
                             const uint32_t* items, const float* ratings, const int32_t* m, const double* evals,
                             const uint64_t* evec_off, const double* evecs, const double* sigtab,
                             uint64_t sigtab_len, int sig_mode, const uint8_t* row_sel, float* mse, int32_t* kk,
                             double* pred, uint32_t* split_out);
/* The same two entry points with fp32 eigenvector blocks: the binary out_eigen_ stores fp32
 * values, and keeping them fp32 halves the host copy and the upload.  evals and sigtab are
 * taken as fp32 values (the binary file's own; they are narrowed back exactly).  The kernels
 * widen every value to fp64 on load, so results equal the fp64 entry points' on the widened
 * arrays bit for bit. */
int cf_predict_precomp_sel_f32(cf_ctx* ctx, uint32_t n_users, const uint64_t* item_off,
                               const uint32_t* items, const float* ratings, const int32_t* m,
                               const double* evals, const uint64_t* evec_off, const float* evecs,
                               const double* sigtab, uint64_t sigtab_len, int sig_mode,
                               const uint8_t* row_sel, float* mse, int32_t* kk, double* pred);
int cf_predict_precomp_multi_f32(cf_ctx* const* ctxs, int n_dev, uint32_t n_users, const uint64_t* item_off,
                                 const uint32_t* items, const float* ratings, const int32_t* m, const double* evals,
                                 const uint64_t* evec_off, const float* evecs, const double* sigtab,
                                 uint64_t sigtab_len, int sig_mode, const uint8_t* row_sel, float* mse, int32_t* kk,
                                 double* pred, uint32_t* split_out);
int cf_predict_run_f64(cf_ctx* ctx, const cf_plan* plan, const uint64_t* d_item_off,
                       const uint32_t* d_items, const float* d_ratings, const int32_t* d_m,
                       const double* d_evals, const uint64_t* d_evec_off,
                       const double* d_evecs, const double* d_sigtab, int sig_mode,
                       float* d_mse, int32_t* d_kk, double* d_pred, void* stream);
int cf_predict_run_f32(cf_ctx* ctx, const cf_plan* plan, const uint64_t* d_item_off,
                       const uint32_t* d_items, const float* d_ratings, const int32_t* d_m,
                       const float* d_evals, const uint64_t* d_evec_off,
                       const float* d_evecs, const float* d_sigtab, int sig_mode,
                       float* d_mse, int32_t* d_kk, double* d_pred, void* stream);

/* ---- fused step ------------------------------------------------------------------
 * cf_eigen_run followed by cf_predict_run_f32 on the SAME outputs (sigtab = d_sigs), with the
 * predictor of every k-bucket started as soon as that bucket's eigenpairs exist, on streams of
 * its own, so prediction overlaps the remaining eigen buckets.  Outputs are identical to the
 * two calls in sequence.  Ordered on `stream` like the *_run calls.  cf_step_timing: device
 * time of the last cf_step_run from its start to the last eigen bucket and to its end. */
int cf_step_run(cf_ctx* ctx, const cf_plan* plan, const uint64_t* d_item_off, const uint32_t* d_items,
                const float* d_ratings, const uint64_t* d_evec_off, int32_t* d_m, float* d_sigs,
                float* d_evals, float* d_evecs, int sig_mode, float* d_mse, int32_t* d_kk,
                double* d_pred, void* stream);
int cf_step_timing(cf_ctx* ctx, float* eigen_ms, float* total_ms);

/* ---- kNN stage ------------------------------------------------------------------
 * knn2 weights_calc (knn2.cpp:127-164): for every item pair a != b over the users
 * present in both train lists, cnt > cnt_min ? w = num/(sqrtf(den1)*sqrtf(den2)) : 0,
 * kept iff w > w_min (the reference writes w > 0.01, cnt > 5).  Output is the dense
 * n_items x n_items weight matrix (0 = no out_fin_ edge); symmetric for integer
 * ratings.  user_off/item/rating: per-user train ratings (CSR over users).
 * Integer ratings in [-11, 11] run on int8 MFMA (exact), others on fp32 MFMA.
 * adopt_as_graph != 0 also installs the result as the context's item graph. */
int cf_item_cosine(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, const uint64_t* user_off,
                   const uint32_t* item, const float* rating, float w_min, int cnt_min,
                   int adopt_as_graph, float* w_out);
/* knn2 with the reference's output form: the compacted edge list "a b w" for w > w_min
 * (knn2.cpp:151-164), as CSR over compact source ids: edge_off[n_items + 1], targets ascending
 * in edge_col / edge_w (capacity edge_cap).  The dense similarity matrix is compacted on the
 * device; only the edges cross PCIe.  *n_edges = the edge count; edge_cap too small gives
 * CF_ERANGE with edge_off and *n_edges filled (retry with edge_cap = *n_edges).
 * adopt_as_graph != 0 installs the result as the context's item graph (its layout). */
int cf_item_cosine_edges(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, const uint64_t* user_off,
                         const uint32_t* item, const float* rating, float w_min, int cnt_min, int adopt_as_graph,
                         uint64_t* edge_off, uint32_t* edge_col, float* edge_w, uint64_t edge_cap, uint64_t* n_edges);
/* Optional top-K cap on cf_item_cosine_edges' list (0 = off, the default: the reference has
 * no top-k, its neighbourhoods are thresholds, knn2.cpp:142,157): per source item only the K
 * largest weights are returned (ties at the K-th value: the lower target ids), still in
 * ascending target order; adopt_as_graph installs the capped list.  Selection is a per-row
 * radix select on the device over the exact weights, so the indices are bit-exact. */
int cf_set_knn2_topk(cf_ctx* ctx, uint32_t topk);
int cf_item_cosine_run(cf_ctx* ctx, uint32_t n_users, uint32_t n_items,
                       const uint64_t* d_user_off, const uint32_t* d_item, const float* d_rating,
                       int integer_ratings, float w_min, int cnt_min, float* d_w_out,
                       void* stream);
/* Durations of the last cf_item_cosine(_run) on its stream (HIP events): plane build
 * (rating scan, memset, scatter) and the MFMA similarity kernel; path = 1 one code
 * plane (<= 7 distinct integer ratings), 2 three int8 planes, 3 fp32 planes.
 * Waits for the launch to finish. */
int cf_knn2_timing(cf_ctx* ctx, float* plane_ms, float* gemm_ms, int* path);
/* The 2^24 guard of the last cf_item_cosine(_run) (SURVEY hard part 7): the reference sums
 * num, den1, den2 and cnt in float (knn2.cpp:129-140), which is exact for integer ratings
 * only while every partial sum stays <= 2^24.  max_accumulator = the largest such sum (the
 * per-item sum of r^2 or rater count, which bounds every pair's); exact = 1 when the
 * reference's floats are exact, so its weights equal this kernel's integer-accumulated
 * ones bit for bit, 0 otherwise (always 0 on the fp32 path of real-valued ratings, whose
 * reference sums are in hash order).  Waits for the launch to finish. */
int cf_knn2_exactness(cf_ctx* ctx, double* max_accumulator, int* exact);
/* K-chunk streaming of the one-code-plane knn2 path: when the int8 code
 * plane of all users (n_items x n_users bytes) exceeds ~60% of free HBM, users are processed
 * in chunks with the four int32 products carried per 128 x 128 tile in HBM between chunks
 * (256 KB per tile) and the epilogue on the last chunk: the weights are identical.
 * cf_set_knn2_chunk forces users_per_chunk (rounded down to a multiple of 128; 0 = automatic);
 * cf_knn2_chunks reports the chunk count of the last launch. */
int cf_set_knn2_chunk(cf_ctx* ctx, uint32_t users_per_chunk);
int cf_knn2_chunks(cf_ctx* ctx, int* n_chunks);
/* local_calc vertex_program::apply (local_calc.cpp:262-526) on the uploaded graph (raw
 * out_fin_ weights; edges count iff w > 0.1, graph_loader :113).  Movie unit v lists
 * movie_items[movie_off[v] .. movie_off[v+1]) = [m, the out-neighbours of m with w > 0.1]
 * (compact ids, any order: results are permutation-equivariant).  Units with fewer than 2
 * out-neighbours are skipped (:271-272); up to 191 run on the LDS kernels, more on the fp64
 * spill kernels (HBM workspace; above CF_SPILL_MAX_K - 1 in their HUGE layout).  There is no
 * neighbourhood cap, as in the reference: a unit whose n x n blocks and 2 n^2 fp64 solver slot
 * do not fit in HBM returns CF_ENOMEM.
 * Test ratings: CSR over all n_items compact ids, test_off[n_items + 1], users ascending
 * within an item.  For every test entry t of a processed movie m (test_off[m] <= t <
 * test_off[m+1]): mse[t] (float, :499), kk[t] (rated rows of the local graph), and when
 * non-null pred[t] (clamped), wlim[t] (= sqrt(lambda_min(L2_h L2_h^T)), :436) and lim[t].
 * Entries of movies not processed are left untouched. */
int cf_local_calc(cf_ctx* ctx, uint32_t n_movies, const uint64_t* movie_off,
                  const uint32_t* movie_items, const uint64_t* test_off, const uint32_t* test_user,
                  const float* test_rating, float* mse, int32_t* kk, double* pred, float* wlim,
                  int32_t* lim);
/* knn3 knn_program + error_vertex_data (knn3.cpp:185-256) on the uploaded graph:
 * per test rating (user u, movie items[e]) pred[e] = sum w*r / sum w over u's test
 * items j with w(movie, j) > 0.1 (0 when none); per movie (compact id)
 * movie_mse[i] = (sum over its test ratings of (r - round(pred))^2, 0 if pred < 0.1)
 * / count, and 0 for movies without test ratings.  The "Knn Average MSE" is
 * sum(movie_mse) / num_vertices (computed by the caller, knn3.cpp:263). */
int cf_knn_predict(cf_ctx* ctx, uint32_t n_users, const uint64_t* user_off,
                   const uint32_t* items, const float* ratings, double* pred,
                   float* movie_mse, uint32_t* movie_count);

/* ---- data prep: knn regroup and k-fold split on the GPU --------
 * cf_knn_regroup replaces the three GraphLab programs of knn.cpp (vertex_program :160-205,
 * vertex2/3_program :212-298) and feeds its writers (:303-357).  Input: n ratings in read
 * order with compact ids user[i] < n_users (in the order of the reference's remapped ids,
 * uimax - id, :103) and movie[i] < n_movies (ascending movie id), rating[i], and
 * validate[i] != 0 for the .validate role (NULL = all train, :88-92).  Output per movie m:
 *   train_user/train_rating[train_off[m] .. train_off[m+1]) : its train ratings, users
 *       ascending, one per user (the last one read wins: map assignment, :183-187);
 *   test_*  likewise for the validate role (ratings_test);
 *   edg_movie[edg_off[m] .. edg_off[m+1]) : the sorted unique movies co-rated with m by any
 *       of its raters, both roles, m itself excluded (:224-227, 271-274, 342-351).
 * train_* / test_* need room for n entries, edg_movie for edg_cap; when the co-rated lists
 * need more than edg_cap entries edg_off is still complete and the call returns CF_ERANGE
 * (the device variant drops the excess writes: check d_edg_off[n_movies] <= edg_cap). */
int cf_knn_regroup(cf_ctx* ctx, uint64_t n, uint32_t n_users, uint32_t n_movies, const uint32_t* user,
                   const uint32_t* movie, const float* rating, const uint8_t* validate, uint64_t* train_off,
                   uint32_t* train_user, float* train_rating, uint64_t* test_off, uint32_t* test_user,
                   float* test_rating, uint64_t* edg_off, uint32_t* edg_movie, uint64_t edg_cap);
int cf_knn_regroup_run(cf_ctx* ctx, uint64_t n, uint32_t n_users, uint32_t n_movies, const uint32_t* d_user,
                       const uint32_t* d_movie, const float* d_rating, const uint8_t* d_validate,
                       uint64_t* d_train_off, uint32_t* d_train_user, float* d_train_rating,
                       uint64_t* d_test_off, uint32_t* d_test_user, float* d_test_rating, uint64_t* d_edg_off,
                       uint32_t* d_edg_movie, uint64_t edg_cap, void* stream);
/* User-disjoint k-fold split (fold_cross_validation.py:31-57): rank[u] is user u's position
 * in the shuffled key list (a permutation of 0..n_users-1); order receives the rating indices
 * sorted by (rank[user[i]], i), i.e. the concatenation u0.test, u1.test, ... of the script
 * (each user's lines in read order).  The fold boundaries are rank ranges (host). */
int cf_fold_order(cf_ctx* ctx, uint64_t n, uint32_t n_users, const uint32_t* user, const uint32_t* rank,
                  uint32_t* order);
int cf_fold_order_run(cf_ctx* ctx, uint64_t n, uint32_t n_users, const uint32_t* d_user, const uint32_t* d_rank,
                      uint32_t* d_order, void* stream);
/* Per-user hold-out split and k-core filter (cf_split.hip; no counterpart in the reference, whose
 * only splitter is the user-disjoint one above).  Input: n < 2^31 edges in read order with compact
 * ids user[i] < n_users, item[i] < n_items and, optionally, order_key[i].  Integers throughout.
 *   1. duplicates: of the edges with one (user, item) the last one read is kept (the rule of
 *      cf_knn_regroup); the others are dropped.  A kept edge carries its own order_key.
 *   2. k-core (min_user, min_item; 0 or 1: no limit on that side), in synchronous rounds over the
 *      kept edges: the degree of every vertex is counted over the edges alive after the previous
 *      round, every user below min_user and every item below min_item dies, and so does every edge
 *      with a dead end.  The rounds stop at the first one in which no edge dies; *rounds counts
 *      those in which one did.  What is left is the maximal core, a function of the edge set alone.
 *   3. order within a user: its n_u alive edges by (order_key, item) ascending; with order_key ==
 *      NULL the key is sm(sm(sm(seed) ^ user) ^ item), sm = splitmix64 (as in cf_bpr_fit), a
 *      function of the ids, so a split does not depend on the read order.
 *   4. parts, p = the edge's position in that order, t = max(n_u - min_train, 0):
 *        CF_SPLIT_LEAVE_K  a = K           h_u = min(K, t)                     part = p < h_u
 *        CF_SPLIT_RATIO    a / b, 0<a<b    h_u = min(floor(n_u a / b), t)      part = p < h_u
 *        CF_SPLIT_FOLDS    a = F, 2..254   part = p mod F
 *      part 1 is VALIDATE, part 0 TRAIN; dropped and dead edges get CF_SPLIT_DROPPED.
 * The core runs before the hold-out, so a TRAIN degree may end below the core's limit.
 * cf_kcore is steps 1-2: keep[i] = 1 for the edges alive after the core, in read order.
 * cf_holdout_split is steps 1-4: part[i] in read order and stats[CF_SPLIT_STATS] (may be NULL):
 *   [0] edges kept after duplicates  [1] edges alive after the core  [2] users, [3] items alive
 *   [4] edges of part 0 (TRAIN)  [5] edges of part 1 (VALIDATE)
 *   [6] alive items without a TRAIN edge (0 for folds)  [7] rounds
 * CF_EINVAL: an id out of range, a null array with n > 0, an unknown mode or parameters outside
 * the ranges above; CF_ERANGE: n >= 2^31.  n = 0 is valid.  The _run forms take device arrays
 * (rounds stays a host pointer) and wait for the stream: one word is read back per round. */
#define CF_SPLIT_LEAVE_K 0
#define CF_SPLIT_RATIO 1
#define CF_SPLIT_FOLDS 2
#define CF_SPLIT_DROPPED 255
#define CF_SPLIT_STATS 8
int cf_kcore(cf_ctx* ctx, uint64_t n, uint32_t n_users, uint32_t n_items, const uint32_t* user,
             const uint32_t* item, uint32_t min_user, uint32_t min_item, uint8_t* keep, uint32_t* rounds);
int cf_kcore_run(cf_ctx* ctx, uint64_t n, uint32_t n_users, uint32_t n_items, const uint32_t* d_user,
                 const uint32_t* d_item, uint32_t min_user, uint32_t min_item, uint8_t* d_keep, uint32_t* rounds,
                 void* stream);
int cf_holdout_split(cf_ctx* ctx, uint64_t n, uint32_t n_users, uint32_t n_items, const uint32_t* user,
                     const uint32_t* item, const uint64_t* order_key, uint64_t seed, uint32_t min_user,
                     uint32_t min_item, int mode, uint32_t a, uint32_t b, uint32_t min_train, uint8_t* part,
                     uint64_t* stats);
int cf_holdout_split_run(cf_ctx* ctx, uint64_t n, uint32_t n_users, uint32_t n_items, const uint32_t* d_user,
                         const uint32_t* d_item, const uint64_t* d_order_key, uint64_t seed, uint32_t min_user,
                         uint32_t min_item, int mode, uint32_t a, uint32_t b, uint32_t min_train, uint8_t* d_part,
                         uint64_t* d_stats, void* stream);
/* Device time of the steps of the last cf_kcore(_run) / cf_holdout_split(_run): ms[0] keys, sort,
 * duplicates and the by-item lists, ms[1] the core rounds (with their read-backs), ms[2] the two
 * order sorts, ms[3] parts and stats (ms[2], ms[3] are 0 after cf_kcore); waits. */
int cf_split_timing(cf_ctx* ctx, float ms[4]);
/* Device time (HIP events) of the last cf_knn_regroup(_run) / cf_fold_order(_run) / cf_kcore(_run) /
 * cf_holdout_split(_run); waits. */
int cf_prep_timing(cf_ctx* ctx, float* ms);

/* ---- graph-signal polynomial filters ------------------------ */
#define CF_FILTER_CHEBY 0     /* cheby.cpp:152-274 (Chebyshev recurrence on [0, 2]) */
#define CF_FILTER_BINOMIAL 1  /* binomials.cpp:145-253 (quadratic factors, overlapping windows) */
/* Replaces the degree / init_values / cheby programs (cheby.cpp:152-245) and the degree /
 * binomial_a / binomial_b programs (binomials.cpp:145-250) with their sync-engine loops
 * (cheby.cpp:296-366, binomials.cpp:296-358).  Vertices are compact indices 0..n_vertices-1;
 * topology line l is (va[l], vb[l], w[l]): when w > 0.1 it adds va -> vb and vb -> va
 * (graph_loader, cheby.cpp:88-92), parallel edges kept, self-edges dropped.  signal[i] is
 * the graph_signal value of vertex i (0 where the file has none).  coeff holds n_coeff >= 3
 * values (both programs read coeff[2]).  out[i] = the filtered signal (fp64).  Synchronous:
 * returns after the copy-out. */
int cf_graph_filter(cf_ctx* ctx, int kind, uint32_t n_vertices, uint64_t n_lines, const uint32_t* va,
                    const uint32_t* vb, const double* w, const double* signal, const double* coeff,
                    uint32_t n_coeff, double* out);
/* Device time of the last cf_graph_filter's supersteps (HIP events) and its directed edges. */
int cf_graph_filter_timing(cf_ctx* ctx, float* device_ms, uint64_t* n_edges);
/* The lanes per vertex row (4, 16 or 64) that cf_graph_filter takes for a graph of n_vertices
 * vertices and n_directed_edges kept directed edges (needs no GPU). */
int cf_debug_filter_lanes(uint32_t n_vertices, uint64_t n_directed_edges);

/* ---- ALS matrix factorization (als.cpp:290-371 on the synchronous engine) ----------------
 * R ~ U V^T over a bipartite graph: users 0..n_users-1 (the side with out-edges), items
 * 0..n_items-1, TRAIN edges only.  Superstep 0 updates the users with activate_user[u] != 0
 * (NULL = every user; the reference signals the users with an out-edge of any role,
 * als.cpp:363-367,662); an update of vertex v (apply, als.cpp:313-334) solves
 * (sum x_j x_j^T + reg[v] I) f = sum obs_j x_j over its edges by an unpivoted LDL^T of the upper
 * triangle, sets residual[v] = (float)(|f - old|_1 / D) and nupdates[v] += 1 (a vertex without
 * edges: residual 0, nupdates += 1, factor untouched); then (scatter, als.cpp:343-357) every
 * edge of an updated vertex signals its other end for the next superstep iff
 * (double)((float)|obs - u.v| * residual[v]) > tol and nupdates[other] < max_updates
 * (UINT64_MAX = no cap).  The sides alternate; the run ends when nobody is signalled or after
 * max_supersteps supersteps (0 = no cap).  fp64 throughout, no floating-point atomics: a
 * vertex's new factor is the same bits whichever other vertices are active.
 *   user_off / user_item / user_obs : CSR over users; item_off / item_user / item_obs : its
 *       transpose (the per-vertex counts are checked: CF_EINVAL)
 *   reg_user / reg_item : the value added to the diagonal per vertex (the reference: lambda, or
 *       with regnormal lambda * num_out_edges, which is 0 for every item, als.cpp:323-327)
 *   U [n_users * D], V [n_items * D] : in the initial factors (the reference draws them,
 *       als.cpp:103), out the fitted ones; nupdates_* and residual_* in / out likewise
 * An exactly zero pivot is skipped (cf_ldlt.hpp), pivots <= 0 are counted in n_not_pd; systems
 * that are not positive definite are outside the parity claim (Eigen's ldlt pivots).
 * D > CF_ALS_MAX_D gives CF_ERANGE; n_users == 0 or no edges is a valid call. */
#define CF_ALS_MAX_D 64
typedef struct cf_als_stats {
    uint32_t supersteps;   /* supersteps run */
    uint64_t updates;      /* vertex updates executed ("Updates executed", als.cpp:676) */
    uint64_t n_not_pd;     /* pivots <= 0 met by the solves */
    float update_ms;       /* device time of the update kernels (HIP events) */
    float scatter_ms;      /* device time of the scatter and compaction kernels */
} cf_als_stats;
int cf_als_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
               const uint32_t* user_item, const float* user_obs, const uint64_t* item_off,
               const uint32_t* item_user, const float* item_obs, const double* reg_user,
               const double* reg_item, double tol, uint64_t max_updates, uint32_t max_supersteps, double* U,
               double* V, uint32_t* nupdates_user, uint32_t* nupdates_item, float* residual_user,
               float* residual_item, const uint8_t* activate_user, cf_als_stats* stats);
/* extract_l2_error summed over the edges of one role (als.cpp:424-430,465-473):
 * *sum_sq = sum (obs - clamp(u.v, minval, maxval))^2; the caller divides and takes the root
 * (:475-479).  A fixed two-level reduction: the same inputs give the same bits. */
int cf_als_error(cf_ctx* ctx, uint64_t n_edges, const uint32_t* user, const uint32_t* item, const float* obs,
                 uint32_t n_users, uint32_t n_items, uint32_t D, const double* U, const double* V,
                 double minval, double maxval, double* sum_sq);
/* prediction_saver::save_edge (als.cpp:499-509): pred[p] = U[user[p]] . V[item[p]], unclamped. */
int cf_als_predict(cf_ctx* ctx, uint64_t n_pairs, const uint32_t* user, const uint32_t* item, uint32_t n_users,
                   uint32_t n_items, uint32_t D, const double* U, const double* V, double* pred);
/* The degree cuts of the update kernels (constants of cf_als.hip; test helpers): vertices with
 * more TRAIN edges than the segment length are summed in segments of that length, vertices with
 * at most low_max edges take one wave. */
int cf_debug_als_segment(void);
int cf_debug_als_low_max(void);

/* ---- SGD and bias-SGD matrix factorization (sgd.cpp, biassgd.cpp; synchronous engine, --interval 0)
 * The graph, the six CSR arrays and their checks are those of cf_als_fit.  State: U, V (fp64), for
 * bias-SGD also bias_user, bias_item and params->global_mean (both bias pointers NULL = plain SGD:
 * mean and biases are absent; exactly one NULL is CF_EINVAL), nupdates per vertex, and the step
 * gamma, which starts at params->gamma.
 * User superstep (0, 2, ..) over the active users A (superstep 0: activate_user[u] != 0, NULL =
 * every user), every value read as it was at the start of the superstep.  Per TRAIN edge (u, i),
 * u in A:  p = clamp(mean + bu[u] + bi[i] + U_u . V_i, minval, maxval),  err = (float)(p - obs)
 * (a NaN err counts in n_nan).  Then  U_u += -gamma (sum_e err_e V_i + deg lambda U_u),
 * bu[u] += -gamma (sum_e err_e + deg lambda bu[u]),  nupdates[u] += 1  (a user without edges only
 * gets the increment).  Item i is signalled iff it has an edge to some u in A and
 * nupdates[i] < max_updates; its message is -gamma (sum err_e U_u + cnt lambda V_i) over its cnt
 * edges with u in A and fabs(err_e) > tol (bias: -gamma (sum err_e + cnt lambda bi[i])); a
 * signalled item without such an edge receives zero.  lambda is applied in closed form (deg, cnt
 * times at once), not per edge.  Then gamma *= step_dec (repeated multiplication).
 * Item superstep (1, 3, ..): every signalled item adds its message, nupdates[i] += 1, and the
 * next A is the users with an edge to a signalled item and nupdates[u] < max_updates.
 * The run ends when the next set is empty, after max_supersteps supersteps (0 = no cap; a run cut
 * after a user superstep drops the pending messages), or after a user superstep with n_nan > 0.
 * The reference never stops without a cap (its scatter signals whatever tol is), so
 * max_updates == UINT64_MAX with max_supersteps == 0 is CF_EINVAL.
 * trace (may be NULL): row t < trace_rows receives {sum sq err over TRAIN, over the n_validate
 * VALIDATE edges} right after user superstep t (new U, old V: the moment of the reference's
 * per-iteration RMSE line), by the reduction of cf_sgd_error.
 * Every summation order depends on the vertex's own degree only and there is no floating-point
 * atomic: a repeated fit gives the same bits, and a user's new row does not depend on which other
 * users are active.  Against the reference (thread-dependent orders) parity is to rounding. */
typedef struct cf_sgd_params {
    double lambda, gamma, step_dec, tol, minval, maxval, global_mean;
    uint64_t max_updates;     /* UINT64_MAX = no cap */
    uint32_t max_supersteps;  /* 0 = no cap */
} cf_sgd_params;
typedef struct cf_sgd_stats {
    uint32_t supersteps;   /* supersteps run */
    uint64_t updates;      /* vertex updates executed */
    uint64_t messages;     /* edges with |err| > tol that sent a message */
    uint64_t n_nan;        /* NaN errors met (the reference dies on the first) */
    double gamma_next;     /* the step the next user superstep would use */
    float reduce_ms;       /* device time of the reduction kernels, both sides (HIP events) */
    float apply_ms;        /* device time of the commit, signalling and compaction kernels */
} cf_sgd_stats;
int cf_sgd_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
               const uint32_t* user_item, const float* user_obs, const uint64_t* item_off,
               const uint32_t* item_user, const float* item_obs, const cf_sgd_params* params, double* U, double* V,
               double* bias_user, double* bias_item, uint32_t* nupdates_user, uint32_t* nupdates_item,
               const uint8_t* activate_user, uint64_t n_validate, const uint32_t* val_user, const uint32_t* val_item,
               const float* val_obs, double* trace, uint32_t trace_rows, cf_sgd_stats* stats);
/* Device time of the last cf_sgd_fit's reduction kernels per side (their sum is reduce_ms). */
int cf_sgd_timing(cf_ctx* ctx, float* user_reduce_ms, float* item_reduce_ms);
/* extract_l2_error summed over the edges of one role (sgd.cpp:393-401, biassgd.cpp:399-409):
 * *sum_sq = sum (obs - clamp(mean + bu + bi + u.v, minval, maxval))^2.  With NULL biases the mean
 * is ignored and the sum is cf_als_error's, bit for bit (the same kernels). */
int cf_sgd_error(cf_ctx* ctx, uint64_t n_edges, const uint32_t* user, const uint32_t* item, const float* obs,
                 uint32_t n_users, uint32_t n_items, uint32_t D, const double* U, const double* V,
                 const double* bias_user, const double* bias_item, double global_mean, double minval, double maxval,
                 double* sum_sq);
/* prediction_saver::save_edge: sgd.cpp:413-424 is unclamped (clamp = 0), biassgd.cpp:418-433
 * clamps (clamp != 0). */
int cf_sgd_predict(cf_ctx* ctx, uint64_t n_pairs, const uint32_t* user, const uint32_t* item, uint32_t n_users,
                   uint32_t n_items, uint32_t D, const double* U, const double* V, const double* bias_user,
                   const double* bias_item, double global_mean, int clamp, double minval, double maxval, double* pred);

/* ---- SVD++ matrix factorization (svdpp.cpp:268-397,412-499; synchronous engine, --interval 0)
 * The graph, the six TRAIN CSR arrays and their checks are those of cf_sgd_fit.  imp_off / imp_item
 * is a CSR by user over the non-TRAIN edges (VALIDATE and PREDICT; imp_off NULL = none, item indices
 * are bound-checked).  deg_all(u) = TRAIN degree + implicit degree (num_out_edges: every role) and
 * usrNorm_u = (float)(1 / sqrt(deg_all(u))).
 * State: per user U_u (pvec), W_u (weight), bu, nupdates; per item V_i (pvec), Y_i (weight), bi,
 * nupdates; the five steps {user,item}_bias_step, {user,item}_factor_step, item_factor2_step, which
 * are floats and start at the params' values; the regularisers are floats too.  --lambda, --gamma
 * and --tol of the reference are never used and have no field here.
 * The phase of a vertex is the parity of its OWN nupdates: even = phase 1, odd = phase 2; vertices
 * of both phases can run in the same superstep.
 * User superstep (0, 2, ..) over the active users A (superstep 0: activate_user[u] != 0, NULL =
 * every user), every value read as it was at the start of the superstep:
 *   u in phase 1:  W_u = usrNorm_u * sum Y_i over EVERY edge of u (TRAIN first, then the implicit
 *     list; a user without any edge keeps W_u); every neighbour item of any role is signalled
 *     without the max_updates check; U_u and bu do not change.
 *   u in phase 2, per TRAIN edge (u, i):
 *     p = clamp(mean + bu[u] + bi[i] + U_u . (V_i + Y_i), minval, maxval)   (the ITEM's weight)
 *     err = (float)(obs - p)          (sign opposite to cf_sgd_fit; a NaN err counts in n_nan)
 *     U_u  += sum user_factor_step * err * (V_i - user_factor_reg * U_u)
 *     bu[u] += sum user_bias_step * err       (user_bias_reg multiplies a local 0 in the reference)
 *     and, iff nupdates[i] < max_updates, item i receives, summed over its senders,
 *       dV  = item_factor_step * (err * (U_u + W_u) - item_factor_reg * V_i)
 *       dbi = item_bias_step * err             (item_bias_reg: as user_bias_reg)
 *       dY  = err * V_i * (float)(item_factor2_step * usrNorm_u)
 *             - (double)(float)(item_factor2_step * item_factor2_reg) * Y_i
 *     and every TRAIN item with nupdates < max_updates is signalled (a signal carries zero).
 *     A non-TRAIN edge contributes nothing.  A phase-2 user without a TRAIN edge is unchanged.
 *   Either way nupdates[u] += 1.  The regulariser sums are applied in closed form (once per vertex:
 *   reg * own * sum err on the user side, cnt * reg * own on the item side), not per edge.
 *   Then each of the five steps becomes (float)(step * step_dec).
 * Item superstep (1, 3, ..): every signalled item, in phase 1 discards its messages, in phase 2
 * adds them (V_i += sum dV, Y_i += sum dY, bi += sum dbi); nupdates[i] += 1; the next A is the
 * users of its TRAIN edges with nupdates[u] < max_updates.
 * The run ends when the next set is empty, after max_supersteps supersteps (0 = no cap; a run cut
 * after a user superstep drops the pending messages), or after a user superstep with n_nan > 0.
 * max_updates counts phase-1 and phase-2 updates alike.  The reference never stops without a cap:
 * max_updates == UINT64_MAX with max_supersteps == 0 is CF_EINVAL.
 * trace (may be NULL): row t < trace_rows receives {sum sq err over TRAIN, over the n_validate
 * VALIDATE edges} right after user superstep t of either phase, by the reduction of cf_sgd_error:
 * extract_l2_error (svdpp.cpp:466-476) is mean + bu + bi + U_u . V_i clamped, WITHOUT Y.
 * The reference leaves vertex_data::bias uninitialised (svdpp.cpp:87-89); here the biases are
 * inputs.  Determinism is that of cf_sgd_fit: a vertex's degree class, split points and summation
 * orders depend on its own degree only (the all-role degree in phase 1, the TRAIN degree elsewhere),
 * no floating-point atomics; an edge's err has the same float bits on the user and the item side. */
typedef struct cf_svdpp_params {
    float user_bias_step, user_bias_reg, item_bias_step, item_bias_reg, user_factor_step, user_factor_reg,
        item_factor_step, item_factor_reg, item_factor2_step, item_factor2_reg;
    double step_dec, minval, maxval, global_mean;
    uint64_t max_updates;     /* UINT64_MAX = no cap */
    uint32_t max_supersteps;  /* 0 = no cap */
} cf_svdpp_params;
typedef struct cf_svdpp_stats {
    uint32_t supersteps;   /* supersteps run */
    uint64_t updates;      /* vertex updates executed, of either phase */
    uint64_t messages;     /* TRAIN edges of phase-2 users that sent a message to a phase-2 item */
    uint64_t n_nan;        /* NaN errors met on TRAIN edges (the reference dies on the first) */
    /* the steps the next user superstep would use */
    float user_bias_step, item_bias_step, user_factor_step, item_factor_step, item_factor2_step;
    float reduce_ms;       /* device time of the three reduction kernel kinds (HIP events) */
    float apply_ms;        /* device time of the commit, signalling and compaction kernels */
} cf_svdpp_stats;
int cf_svdpp_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                 const uint32_t* user_item, const float* user_obs, const uint64_t* item_off,
                 const uint32_t* item_user, const float* item_obs, const uint64_t* imp_off, const uint32_t* imp_item,
                 const cf_svdpp_params* params, double* U, double* V, double* W, double* Y, double* bias_user,
                 double* bias_item, uint32_t* nupdates_user, uint32_t* nupdates_item, const uint8_t* activate_user,
                 uint64_t n_validate, const uint32_t* val_user, const uint32_t* val_item, const float* val_obs,
                 double* trace, uint32_t trace_rows, cf_svdpp_stats* stats);
/* Device time of the last cf_svdpp_fit per kernel kind (their sum is reduce_ms). */
int cf_svdpp_timing(cf_ctx* ctx, float* phase1_reduce_ms, float* user_reduce_ms, float* item_reduce_ms);
/* prediction_saver::save_edge (svdpp.cpp:490-493): clamp(mean + bu + bi + U_u . (V_i + Y_i)); always
 * clamped.  The training error is cf_sgd_error (no Y), so there is no cf_svdpp_error. */
int cf_svdpp_predict(cf_ctx* ctx, uint64_t n_pairs, const uint32_t* user, const uint32_t* item, uint32_t n_users,
                     uint32_t n_items, uint32_t D, const double* U, const double* V, const double* Y,
                     const double* bias_user, const double* bias_item, double global_mean, double minval,
                     double maxval, double* pred);

/* ---- truncated SVD of the rating matrix by restarted Golub-Kahan-Lanczos (svd.cpp:304-505) ----
 * A is rows x cols, given as two CSRs of the same entries (row_* by row, col_* by column: u64
 * offsets, u32 neighbour, f32 value; checked like cf_als_fit's).  U (rows x nsv) holds the left
 * vectors, V (cols x nsv) the right ones, both column-major (vector i at U + i * rows).  The
 * reference swaps the names inside lanczos(): its V[i] live on the rows and its U[i] on the columns.
 * Below P[i] is row-side, Q[i] column-side, nv + 1 vectors each; fp64 throughout.
 *   P[0] = v0 / |v0|, nconv = 0, its = 1; while nconv < nsv && its < max_iter (so at most
 *   max_iter - 1 passes), with k = nconv:
 *     Q[k] = A^T P[k], orthogonalised against Q[0..k), normalised: alpha[0]
 *     for i = k+1 .. nv-1:  P[i] = A Q[i-1] against P[0..i): beta[i-k-1];
 *                           Q[i] = A^T P[i] against Q[0..i): alpha[i-k]
 *     P[nv] = A Q[nv-1] against P[0..nv): beta[nv-k-1]
 *     m = nv - nconv; T = bidiag(alpha, beta[0..m-1)) = a diag(b) PT^T (host, one-sided Jacobi, b
 *     descending); sigma[nconv+j] = b[j]; errest[nconv+j] = |a(m-1,j) beta[m-1]|, divided by b[j]
 *     when b[j] > tol; kk = the number of new errest < tol; P[:, nconv..nconv+kk) = P[:, nconv..nv)
 *     PT[:, 0..kk), Q likewise with a; done when nconv + kk >= nsv, else P[nconv+kk] = sum_t
 *     PT(t, kk) P[nconv+t], nconv += kk, its++.
 *   Orthogonalisation: classical Gram-Schmidt, ortho_repeats (1..3) times, all coefficients from the
 *   same vector; the vector is divided by its norm only when the norm is >= 1e-10 (math.hpp:898).
 *   Afterwards, for i < min(nsv, nconv): err[i] = sqrt(|A^T P[i] - sigma_i Q[i]|^2 + |A Q[i] -
 *   sigma_i P[i]|^2), divided by sigma_i when sigma_i > tol.
 * Outputs: sigma[nv], errest[nv] (positions a pass did not reach stay as passed in), err[nsv] and
 * the first min(nsv, nconv) columns of U and V (the rest untouched); kk_pass (optional, max_iter
 * entries) receives kk of every pass, first_ab (optional, 2 nv doubles) the first pass's alpha
 * then beta.  A square matrix with a regularised diagonal is built by the caller as ordinary
 * entries.  Every summation order is fixed by the matrix's own shape (a row's by its degree, a
 * vector's by a constant slice length), no floating-point atomics: equal inputs give equal bits.
 * CF_EINVAL: null argument, nsv == 0, nv < nsv, ortho_repeats outside 1..3, v0 all zero, CSRs that
 * disagree; CF_ERANGE: nv > CF_SVD_MAX_NV.  rows == 0 or cols == 0 is a valid no-op. */
#define CF_SVD_MAX_NV 256
typedef struct cf_svd_stats {
    uint32_t nconv;      /* converged triplets */
    uint32_t passes;     /* restarts run (at most max_iter - 1) */
    uint32_t products;   /* matrix-vector products, the residual checks' included */
    float matvec_ms;     /* device time of the product kernels (HIP events) */
    float ortho_ms;      /* of the orthogonalisation and normalisation kernels */
    float rotate_ms;     /* of the Ritz rotation and restart-vector kernels */
} cf_svd_stats;
int cf_svd_fit(cf_ctx* ctx, uint32_t rows, uint32_t cols, const uint64_t* row_off, const uint32_t* row_col,
               const float* row_val, const uint64_t* col_off, const uint32_t* col_row, const float* col_val,
               uint32_t nsv, uint32_t nv, uint32_t max_iter, double tol, uint32_t ortho_repeats, const double* v0,
               double* sigma, double* errest, double* err, double* U, double* V, uint32_t* kk_pass, double* first_ab,
               cf_svd_stats* stats);
/* The product kernel of cf_svd_fit on its own: y[n_out] = M x[n_in] for the CSR (off, nbr, val) with
 * n_out rows (pass the column CSR for A^T x).  A row's summation order depends on its degree only. */
int cf_svd_matvec(cf_ctx* ctx, uint32_t n_out, uint32_t n_in, const uint64_t* off, const uint32_t* nbr,
                  const float* val, const double* x, double* y);
/* The product kernel's cut between one wave per row and one workgroup per row; the other two cuts
 * are cf_debug_als_low_max (several rows per wave up to it) and cf_debug_als_segment. */
int cf_debug_svd_wave_max(void);
/* The host SVD of cf_svd_fit's bidiagonal T on its own (csrc/cf_small_svd.hpp; needs no GPU):
 * T is m x m row-major; a, PT (m x m row-major) and b (m, descending) with T = a diag(b) PT^T.
 * Returns the number of sweeps, or CF_EINVAL. */
int cf_debug_small_svd(int m, const double* T, double* a, double* b, double* PT);

/* ---- top-N recommendation from fitted factors (no reference counterpart: its programs save only
 * the PREDICT edges, als.cpp:493-510) ----
 * For every selected user the N best candidate items by score.  sel_user NULL selects users
 * 0..n_users-1 (n_sel is ignored); otherwise list j is that of user sel_user[j], j < n_sel.
 *   candidates of user u : every item i that is not in excl_item[excl_off[u] .. excl_off[u+1]) (a CSR
 *       over all n_users; any order, repeats allowed; both pointers NULL = no exclusions)
 *   dot(u, i) = sum over d ascending of U[u,d] V[i,d], on the fp64 matrix cores from a zero
 *       accumulator, D zero-padded to a multiple of 4
 *   score = dot + (bias_item[i] + (mean + bias_user[u])); an absent bias is skipped, not added as 0,
 *       and mean is used only when a bias is given
 *   a NaN score is never listed and counts in n_nan; -0.0 ranks equal to +0.0 (and is reported as +0.0)
 * Outputs per selected user j: count[j] = min(N, non-NaN candidates); items[j N .. j N + count[j])
 * and the matching scores ordered by score descending, ties by ascending item index (the rule of
 * cf_set_knn2_topk); the tail up to N is UINT32_MAX / 0.0.
 * A score's bits depend only on its own two rows and biases and there is no floating-point atomic:
 * a user's list is the same bytes across repeats, for every user-block size, and whichever other
 * users are selected.  The users run in blocks whose n_items keys per user (a panel in the ALS
 * workspace) fit a fixed byte budget; cf_set_topn_block forces the users per block (0 = automatic).
 * CF_ERANGE: D == 0, D > CF_ALS_MAX_D, N > CF_TOPN_MAX_N.  CF_EINVAL: N == 0, exactly one of
 * excl_off / excl_item NULL, a decreasing excl_off, an excl_item >= n_items, a sel_user >= n_users.
 * n_users == 0, n_items == 0 or n_sel == 0 with a non-NULL sel_user is a valid call that writes
 * only count (zeros). */
#define CF_TOPN_MAX_N 1024
typedef struct cf_topn_stats {
    uint32_t blocks;      /* user blocks processed */
    uint64_t n_nan;       /* candidate scores that were NaN (left out of every list) */
    float score_ms;       /* device time of the scoring kernels (HIP events) */
    float select_ms;      /* device time of exclusion, selection and ordering */
} cf_topn_stats;
int cf_mf_topn(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const double* U, const double* V,
               const double* bias_user, const double* bias_item, double mean, const uint64_t* excl_off,
               const uint32_t* excl_item, uint32_t n_sel, const uint32_t* sel_user, uint32_t N, uint32_t* items,
               double* scores, uint32_t* count, cf_topn_stats* stats);
int cf_set_topn_block(cf_ctx* ctx, uint32_t users_per_block);
/* The user and item tile of the scoring kernel (constants of cf_topn.hip; test helpers). */
int cf_debug_topn_tile_users(void);
int cf_debug_topn_tile_items(void);

/* ---- ranking evaluation of fitted factors (no reference counterpart: its programs score listed
 * pairs only, as for cf_mf_topn) ----
 * For every held-out edge (u, i) its exact rank in u's full candidate ordering, and the ranking
 * metrics at cutoff N per user with their means.  Scores, candidates and order are those of
 * cf_mf_topn: score descending, item ascending among equal scores, excluded items and items whose
 * score is NaN are not candidates.  The item at position p of a user's cf_mf_topn list has rank p.
 *   excl_off / excl_item : the training edges, a CSR over all n_users as for cf_mf_topn (any order,
 *       repeats allowed; both NULL = no exclusions)
 *   held_off / held_item : the edges to find, a CSR over all n_users (u64 offsets, u32 items) whose
 *       items are STRICTLY ascending within a user, so no edge can be counted twice
 *   held_w : NULL (all ones) or one weight per held-out edge, used by mpr only
 * Per user u: C = n_cand, the number of candidates.  The held-out items that are candidates get the
 * 0-based ranks r_0 < r_1 < .. < r_(m-1), m = n_rel.  A held-out item that is excluded, or whose
 * score is NaN, gets rank UINT32_MAX; it is not counted in m, it is counted in edges_skipped, and a
 * NaN one also in n_nan_held.  Ranks are a strict total order by the tie rule: no half credit.
 * Per user with m >= 1, at cutoff N (1 <= N <= CF_TOPN_MAX_N):
 *   hits      = #{j : r_j < N}
 *   precision = hits / N                   recall = hits / m
 *   ndcg      = (sum_{r_j < N} 1 / log2(r_j + 2)) / (sum_{t < min(m, N)} 1 / log2(t + 2))
 *   ap        = (1 / min(m, N)) sum_{r_j < N} (j + 1) / (r_j + 1)
 *   rr        = 1 / (r_0 + 1), with no cutoff
 *   auc       = sum_j (C - m - r_j + j) / (m (C - m)); defined only if C > m: otherwise the record
 *               holds 0 and the user is left out of the AUC mean
 *   percentile rank of edge j = r_j / (C - 1), or 0 when C = 1
 * A user with m = 0 is not evaluated: its record is all zeros, n_cand included, and it enters no mean.
 * Summary: the means of precision, recall, ndcg, ap (map), rr (mrr) and auc over the evaluated users,
 * summed in ascending user index; mpr = sum_e w_e pr_e / sum_e w_e over the counted edges in CSR
 * order (0 when the weights sum to 0): the expected percentile rank of Hu, Koren and Volinsky as a
 * fraction in [0, 1], 0 at the top.
 * Only users with a held-out edge are scored, in the user blocks and key panel of cf_mf_topn (same
 * cf_set_topn_block, same byte budget).  The device returns integers only (ranks and candidate
 * counts, integer sums in any order); the metrics are computed on the host from them in the fixed
 * orders above, so every output is the same bytes across repeats and for every user-block size.
 * CF_ERANGE: D == 0, D > CF_ALS_MAX_D, N > CF_TOPN_MAX_N.  CF_EINVAL: N == 0, exactly one of
 * excl_off / excl_item NULL, a NULL held_off (or a NULL held_item with edges), offsets that do not
 * start at 0 or decrease, an excl_item or held_item >= n_items, held items of a user not strictly
 * ascending.  A call with no users, no items or no held-out edges succeeds and writes zeros (user
 * records and summary).  rank: one entry per held-out edge; users: n_users records; summary may be NULL. */
typedef struct cf_rank_user {
    uint32_t n_cand;      /* C: candidates of the user (0 when the user is not evaluated) */
    uint32_t n_rel;       /* m: held-out items that are candidates */
    uint32_t hits;        /* of them, those ranked below N */
    uint32_t reserved;    /* 0 */
    double precision, recall, ndcg, ap, rr, auc;
} cf_rank_user;
typedef struct cf_rank_summary {
    uint32_t users_evaluated;   /* users with m >= 1 */
    uint32_t users_auc;         /* of them, those with C > m (the AUC mean's count) */
    uint64_t edges_counted;     /* held-out edges with a rank */
    uint64_t edges_skipped;     /* held-out edges that are excluded or whose score is NaN */
    uint64_t n_nan_held;        /* of edges_skipped, the NaN ones (not excluded) */
    double precision, recall, ndcg, map, mrr, auc, mpr;
    uint32_t blocks;            /* user blocks processed */
    float score_ms;             /* device time of the scoring kernels (HIP events) */
    float rank_ms;              /* device time of exclusion and rank counting */
} cf_rank_summary;
int cf_mf_rank_eval(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const double* U, const double* V,
                    const double* bias_user, const double* bias_item, double mean, const uint64_t* excl_off,
                    const uint32_t* excl_item, const uint64_t* held_off, const uint32_t* held_item,
                    const double* held_w, uint32_t N, uint32_t* rank, cf_rank_user* users, cf_rank_summary* summary);
/* Held-out items counted per walk of a row, and the keys covered by one trip of that walk (threads
 * x loads in flight per lane): constants of cf_rank.hip; test helpers. */
int cf_debug_rank_targets(void);
int cf_debug_rank_walk(void);

/* ---- top-N recommendation and ranking evaluation from the item graph (no reference counterpart:
 * knn3 scores listed pairs only, knn3.cpp:185-227) ----
 * The neighbourhood model as a score source of cf_mf_topn and cf_mf_rank_eval.  n_items is the
 * resident graph's item count.  User u's profile is prof_item / prof_rating[prof_off[u] ..
 * prof_off[u+1]) = (i_0, r_0), (i_1, r_1), .., in the order given; for every item m of the graph
 *   sw(u, m)  = sum_t [(double) w(m, i_t) > w_min] (double) w(m, i_t)
 *   swr(u, m) = sum_t [(double) w(m, i_t) > w_min] (double) w(m, i_t) * (double) r_t
 * both over t ascending from a zero accumulator in fp64; w(m, i) is row m, column i of the uploaded
 * graph as parsed (fp32): the out-edge of the scored item, the direction of cf_knn_predict.  The
 * graph is not symmetrized, i_t == m is no special case (its weight is what the graph holds), and a
 * profile item listed twice counts twice.
 *   CF_KNN_SCORE_SUM  : score = swr
 *   CF_KNN_SCORE_MEAN : score = sw > 0 ? swr / sw : 0, the prediction of cf_knn_predict with its
 *                       "no neighbour -> 0" rule (knn3.cpp:216) when w_min = 0.1
 * Everything after the score is cf_mf_topn's / cf_mf_rank_eval's contract, unchanged: candidates,
 * exclusions (excl_*), NaN scores (a NaN rating is no error: its scores are NaN, counted and never
 * listed), -0 as +0, the order, N <= CF_TOPN_MAX_N, sel_user, the user blocks (cf_set_topn_block),
 * outputs, tails, stats structs, the held_* rules, the m = 0 user rule and the host-side metric
 * orders.  The summation order is fixed, so a user's outputs are the same bytes across repeats, for
 * every user-block size, for either graph layout and whichever other users are selected; there is
 * no floating-point atomic.  score_ms counts the scoring kernel and, when the call builds them, the
 * graph's in-lists (cached in the context per w_min until the next graph upload).
 * CF_ESTATE: no graph uploaded.  CF_EINVAL: an unknown score_mode, a w_min that is not finite and
 * >= 0, N == 0, a prof_off that is NULL, does not start at 0 or decreases, a prof_item >= n_items,
 * and every exclusion, selection or held-out error of the mf calls.  CF_ERANGE: N > CF_TOPN_MAX_N, a
 * graph of more than 2^24 items.
 * Calls with no users, no selected users or no held-out edges succeed and write zeros as the mf
 * calls do. */
#define CF_KNN_SCORE_SUM 0
#define CF_KNN_SCORE_MEAN 1
int cf_knn_topn(cf_ctx* ctx, uint32_t n_users, const uint64_t* prof_off, const uint32_t* prof_item,
                const float* prof_rating, int score_mode, double w_min, const uint64_t* excl_off,
                const uint32_t* excl_item, uint32_t n_sel, const uint32_t* sel_user, uint32_t N, uint32_t* items,
                double* scores, uint32_t* count, cf_topn_stats* stats);
int cf_knn_rank_eval(cf_ctx* ctx, uint32_t n_users, const uint64_t* prof_off, const uint32_t* prof_item,
                     const float* prof_rating, int score_mode, double w_min, const uint64_t* excl_off,
                     const uint32_t* excl_item, const uint64_t* held_off, const uint32_t* held_item,
                     const double* held_w, uint32_t N, uint32_t* rank, cf_rank_user* users, cf_rank_summary* summary);
/* In-list entries per trip of the scoring kernel's walk (threads x entries in flight per lane): a
 * constant of cf_knn_topn.hip; test helper. */
int cf_debug_knn_topn_walk(void);

/* ---- implicit-feedback ALS (Hu, Koren, Volinsky, ICDM 2008; no reference counterpart: wals.cpp
 * cites the paper and fits observed and sampled edges only) ----
 * Every pair of the n_users x n_items grid is a training example: an edge carries a confidence
 * conf >= 1 and a preference pref (both f32 per edge; repeated edges each count), every other pair
 * is pref 0 with confidence 1.
 *   L(U, V) = sum_{u,i} c_ui (p_ui - U_u.V_i)^2 + sum_u reg_user[u] |U_u|^2 + sum_i reg_item[i] |V_i|^2
 * A sweep is a user half-sweep, then an item half-sweep; a half-sweep sets every vertex v of its
 * side to the exact minimiser: with x the other side's rows and G = sum over all of them of x x^T,
 *   (G + sum_{edges of v} (c - 1) x x^T + reg[v] I) f = sum_{edges of v} (c p) x
 * by the unpivoted LDL^T of cf_als_fit (reg > 0 and c >= 1 make every system positive definite;
 * n_not_pd counts pivots <= 0).  A vertex without edges becomes +0.0 in every component.
 * fp64 throughout and no floating-point atomics: a vertex's new factor depends only on its own edge
 * list, the other side's rows and the bits of G; a repeated fit gives the same bytes.
 *   user_off / user_item / user_conf / user_pref : CSR over users; item_* : its transpose (checked
 *       like cf_als_fit's).  Both pref arrays NULL = every preference is 1; exactly one NULL is
 *       CF_EINVAL, as are a conf < 1 or not finite and a pref not finite
 *   U [n_users * D], V [n_items * D] : in the initial factors, out the fitted ones
 *   loss_trace : NULL, or 2 * n_sweeps doubles: L after each half-sweep
 * D == 0 gives CF_EINVAL, D > CF_ALS_MAX_D CF_ERANGE; n_sweeps == 0 (U, V untouched), no edges and an
 * empty side are valid calls. */
typedef struct cf_ials_stats {
    uint32_t sweeps;       /* sweeps run */
    uint64_t n_not_pd;     /* pivots <= 0 met by the solves */
    float gram_ms;         /* device time of the global Gram kernels (HIP events) */
    float update_ms;       /* device time of the per-vertex update kernels */
    float loss_ms;         /* device time of the loss kernels (0 without a trace) */
} cf_ials_stats;
int cf_ials_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                const uint32_t* user_item, const float* user_conf, const float* user_pref, const uint64_t* item_off,
                const uint32_t* item_user, const float* item_conf, const float* item_pref, const double* reg_user,
                const double* reg_item, uint32_t n_sweeps, double* U, double* V, double* loss_trace,
                cf_ials_stats* stats);
/* *loss = L(U, V) of any factors, evaluated without the unobserved pairs:
 * <U^T U, V^T V>_F + sum over the edges of [c (p - s)^2 - s^2] + the two reg terms, s = U_u.V_i.
 * Fixed reductions: the same inputs give the same bits.  Arguments and checks as cf_ials_fit. */
int cf_ials_loss(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                 const uint32_t* user_item, const float* user_conf, const float* user_pref, const uint64_t* item_off,
                 const uint32_t* item_user, const float* item_conf, const float* item_pref, const double* reg_user,
                 const double* reg_item, const double* U, const double* V, double* loss);
/* G [D * D] = F^T F of the n x D row-major matrix F: slices of cf_debug_ials_gram_rows() rows, summed
 * in slice order; a slice's partial depends on its own rows only.  G is symmetric bit for bit and the
 * same bits in every run; appending rows that are all zero does not change it.  n == 0 gives zeros. */
int cf_mf_gram(cf_ctx* ctx, uint32_t n, uint32_t D, const double* F, double* G);
/* The slice length of the global Gram (a constant of cf_ials.hip; test helper, needs no GPU). */
int cf_debug_ials_gram_rows(void);

/* ---- non-negative matrix factorization under the generalised Kullback-Leibler divergence (Lee and
 * Seung's multiplicative rules).  nmf.cpp sums the rule's numerator over every edge of the graph
 * into one vector for all vertices, which is no factorization; these entry points fit what its
 * header and its pre_iter column sum stand for ----
 * R ~ U V^T, every component >= CF_NMF_EPS.  For an edge (u, i, r), r >= 0 (f32; repeated edges each
 * count), p = U_u.V_i, with 0 log 0 = 0:
 *   CF_NMF_OBSERVED  L = sum_edges [r log(r / p) - r + p]
 *                    U_u[d] <- U_u[d] (sum_{e in N(u)} V_i[d] r / p) / (sum_{e in N(u)} V_i[d])
 *   CF_NMF_GRID      L = sum_edges [r log(r / p) - r] + s_U.s_V,  s_F[d] = sum over ALL rows of F[.][d]
 *                    (every pair of the grid counts, unrated = 0: Poisson factorization)
 *                    U_u[d] <- U_u[d] (sum_{e in N(u)} V_i[d] r / p) / s_V[d]
 * and a component below CF_NMF_EPS becomes CF_NMF_EPS (n_floored counts these).  A sweep is the user
 * half-sweep from the current V, then the item half-sweep from the new U; every value is read as
 * it was at the start of the half-sweep.  An edge with r = 0 adds nothing to a numerator, adds its
 * row to an OBSERVED denominator, and has loss term p (OBSERVED) or 0 (GRID).  A vertex without
 * edges keeps its row bit for bit (OBSERVED) or becomes CF_NMF_EPS in every component (GRID; its
 * row still counts in s_F).
 * fp64 throughout and no floating-point atomics: a vertex's new row depends only on its own edge
 * list, the other side's rows and, in GRID mode, the bits of s; a repeated fit gives the same bytes.
 *   user_off / user_item / user_obs : CSR over users; item_* : its transpose (checked like
 *       cf_als_fit's).  CF_EINVAL: an unknown mode, an obs that is negative or not finite, an initial
 *       factor component that is not finite or below CF_NMF_EPS (a zero never leaves zero)
 *   U [n_users * D], V [n_items * D] : in the initial factors, out the fitted ones
 *   loss_trace : NULL, or 2 * n_sweeps doubles: L after each half-sweep, the same bits as
 *       cf_nmf_loss of the factors at that point
 * D == 0 gives CF_EINVAL, D > CF_ALS_MAX_D CF_ERANGE; n_sweeps == 0 (U, V untouched), no edges and an
 * empty side are valid calls. */
#define CF_NMF_OBSERVED 0
#define CF_NMF_GRID 1
#define CF_NMF_EPS 1e-16
typedef struct cf_nmf_stats {
    uint32_t sweeps;       /* sweeps run */
    uint64_t n_floored;    /* components set to CF_NMF_EPS, over the whole fit */
    float sum_ms;          /* device time of the column-sum kernels before the half-sweeps (HIP events) */
    float update_ms;       /* device time of the per-vertex update kernels */
    float loss_ms;         /* device time of the loss kernels (0 without a trace) */
} cf_nmf_stats;
int cf_nmf_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
               const uint32_t* user_item, const float* user_obs, const uint64_t* item_off, const uint32_t* item_user,
               const float* item_obs, int mode, uint32_t n_sweeps, double* U, double* V, double* loss_trace,
               cf_nmf_stats* stats);
/* *loss = L(U, V) of any factors that pass cf_nmf_fit's checks.  Fixed reductions: the same inputs
 * give the same bits. */
int cf_nmf_loss(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
                const uint32_t* user_item, const float* user_obs, const uint64_t* item_off, const uint32_t* item_user,
                const float* item_obs, int mode, const double* U, const double* V, double* loss);
/* s [D] = the column sums of the n x D row-major matrix F: slices of cf_debug_nmf_sum_rows() rows,
 * summed in slice order; a slice's partial depends on its own rows only.  The same bits in every
 * run; appending rows that are all zero does not change it.  n == 0 gives zeros. */
int cf_mf_colsum(cf_ctx* ctx, uint32_t n, uint32_t D, const double* F, double* s);
/* The slice length of the column sum (a constant of cf_nmf.hip; test helper, needs no GPU). */
int cf_debug_nmf_sum_rows(void);

/* ---- Bayesian Personalized Ranking (Rendle et al., UAI 2009): matrix factorization trained on the
 * pairwise objective  sum ln sigmoid(x_ui - x_uj)  over (user, rated item, unrated item) triples, the
 * smooth form of the AUC cf_mf_rank_eval reports.  No reference counterpart ----
 * Inputs: the positive pairs as the user CSR user_off / user_item and its transpose item_off /
 * item_user.  There are no ratings: an edge is a positive.  Both sides' lists are STRICTLY ASCENDING
 * (an edge cannot appear twice and membership is a binary search); anything else, and CSRs that are
 * not each other's transpose, give CF_EINVAL.  State in fp64: U [n_users x D], V [n_items x D] and
 * the optional bias_item [n_items] (NULL: no bias, every b below is 0 and none is written).
 * Score: x_ui = U_u . V_i + b_i.
 *
 * The sample is integers only; nothing about it depends on a factor.  sm is splitmix64 with the
 * final x ^ (x >> 31) (host/cf_mf_cli.hpp), T = CF_BPR_TRIES.  For sweep index s, user u and the
 * edge at rank r of u's list (its item is i):
 *     key_s   = sm(sm(seed) ^ s)
 *     h(t)    = sm(sm(key_s ^ u) ^ (r * T + t))            t = 0 .. T-1
 *     cand(t) = (uint32)(((h(t) >> 32) * n_items) >> 32)
 *     j       = the first cand(t) that is not in u's list
 * If all T candidates are in the list the edge is SKIPPED this sweep: it has no triple, adds nothing
 * anywhere, and counts in n_skipped.  A user's negatives depend on seed, s, u and its own list only.
 *
 * A sweep (a Jacobi step: every value is read as it was at the start of the sweep).  Per triple
 *     x = U_u . (V_i - V_j) + b_i - b_j,    g = 1 / (1 + exp(x))
 * and with c_u the number of triples of user u, c_i the number of triples in which item i is the
 * positive PLUS the number in which it is the negative:
 *     U_u += lr ((sum_{triples of u} g (V_i - V_j)) / c_u - reg_user U_u)                      c_u > 0
 *     V_i += lr ((sum_{i positive} g U_u - sum_{i negative} g U_u) / c_i - reg_item V_i)       c_i > 0
 *     b_i += lr ((sum_{i positive} g     - sum_{i negative} g    ) / c_i - reg_bias b_i)       c_i > 0
 * A vertex with count 0 keeps its row bit for bit.  The division by the vertex's own count keeps the
 * stationary points of per-triple regularised BPR-OPT and bounds a vertex's step by lr whatever its
 * degree.
 *   loss_trace : NULL, or 2 * n_sweeps doubles; row s = {sum over the sweep's triples of
 *       softplus(-x), (double) number of triples}, from the start-of-sweep factors, by a fixed
 *       two-level reduction
 *   a NaN x counts in n_nan, and the fit ends after a sweep with n_nan > 0 (stats->sweeps tells)
 *   params->first_sweep : the index s of the first sweep; n_sweeps = 5 gives the same bytes as
 *       n_sweeps = 2 followed by first_sweep = 2, n_sweeps = 3 on its results
 * Determinism: a vertex's class, split points and every summation order depend on the
 * length of the list being summed only; no floating-point atomic; a repeated fit gives the same
 * bytes; a user's new row depends on its own list and the item rows only.
 * D == 0 gives CF_EINVAL, D > CF_ALS_MAX_D CF_ERANGE; lr or a reg that is not finite, or a negative
 * reg, CF_EINVAL; n_sweeps == 0 (factors untouched), no edges and an empty side are valid calls. */
#define CF_BPR_TRIES 8
typedef struct cf_bpr_params {
    double lr, reg_user, reg_item, reg_bias;
    uint64_t seed;
    uint32_t first_sweep, n_sweeps;
} cf_bpr_params;
typedef struct cf_bpr_stats {
    uint32_t sweeps;                       /* sweeps run */
    uint64_t triples, n_skipped, n_nan;    /* over those sweeps */
    float sample_ms, reduce_ms, apply_ms;  /* HIP-event device times: sample and gradient kernel; the
                                              negative lists and the three reductions; the commits */
} cf_bpr_stats;
int cf_bpr_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, uint32_t D, const uint64_t* user_off,
               const uint32_t* user_item, const uint64_t* item_off, const uint32_t* item_user,
               const cf_bpr_params* params, double* U, double* V, double* bias_item, double* loss_trace,
               cf_bpr_stats* stats);
/* The sampler alone: neg[p] for every position p of the user CSR, UINT32_MAX = skipped; *n_skipped
 * (may be NULL) counts those.  The lists are checked as cf_bpr_fit checks them. */
int cf_bpr_sample(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, const uint64_t* user_off, const uint32_t* user_item,
                  uint64_t seed, uint32_t sweep, uint32_t* neg, uint64_t* n_skipped);
/* Device times of the last cf_bpr_fit, summed over its sweeps: {sample and gradient, sort + offsets +
 * class lists of the negative CSR, user reduction, item positive reduction, item negative
 * reduction, commit}. */
int cf_bpr_timing(cf_ctx* ctx, float ms[6]);
/* CF_BPR_TRIES as compiled (test helper, needs no GPU). */
int cf_debug_bpr_tries(void);

/* ---- EASE (Steck, "Embarrassingly Shallow Autoencoders for Sparse Data", WWW 2019): the closed-form
 * linear item-item model, as a fit and as a third score source of cf_mf_topn / cf_mf_rank_eval.  No
 * reference counterpart ----
 * Inputs of the fit: the TRAIN edges as a CSR by user (user_off / user_item / user_obs) whose item
 * lists are STRICTLY ASCENDING, lambda > 0 and `binary`: the value of an edge is x = 1 when binary is
 * nonzero, else (double) obs.
 *   G = X^T X + lambda I   G[i][j] = sum over the users in ascending order, from a zero accumulator,
 *                          of x_ui x_uj in fp64 (the product of two floats is exact in a double);
 *                          lambda is added to the diagonal last.  G is symmetric bit for bit.
 *   P = G^-1               in place, by unpivoted block Gauss-Jordan of block width
 *                          cf_debug_ease_block() (every pivot block is a Schur complement of an SPD
 *                          matrix).  The block width is a constant: the bytes of P depend on G only.
 *   B[i][j] = -P[i][j] / P[j][j] for i != j, B[j][j] = 0
 * B is n_items x n_items fp64 row-major and stays resident in the context until the next cf_ease_fit,
 * cf_ease_upload or cf_destroy (cf_release_workspaces leaves it alone).  It is independent of the
 * resident item graph: both can be resident at once.  An item without an edge has G row and column
 * lambda e_j, so its row and column of B are zero; there is no special case.
 * Score of item j for a profile (i_0, x_0), (i_1, x_1), .. (x_t = 1 when binary, else (double) rating):
 *   s(u, j) = sum_t x_t B[i_t][j]   over the profile in the order given, from zero; each product is
 *                                   rounded to double, then added (no fused multiply-add)
 * The profile at scoring time is an argument, as cf_knn_topn's is; it need not be the fit's, and its
 * items need not ascend.  Everything after the score is cf_mf_topn's / cf_mf_rank_eval's contract,
 * unchanged (see cf_knn_topn).  There is no floating-point atomic and every reduction has a fixed
 * order: B and every list are the same bytes across repeats, user-block sizes and selections.
 *   cf_ease_fit      fits and keeps B.  n_items == 0 succeeds and leaves no B resident.
 *   cf_ease_gram     the Gram stage alone, the kernel the fit runs: G [n_items^2] to the host
 *   cf_ease_weights  *n_items = the resident B's size; B == NULL: the size only
 *   cf_ease_upload   any B: signed, NaN allowed
 *   cf_ease_timing   device times of the last fit: {Gram (with the by-item CSR), inversion, normalise}
 * CF_EINVAL: lambda not finite or <= 0; null arrays; an offset array that does not start at 0 or
 * decreases; an item >= n_items; a fit list that is not strictly ascending; cf_ease_upload with
 * n_items == 0; plus every error of the mf calls.  CF_ESTATE: cf_ease_topn / cf_ease_rank_eval /
 * cf_ease_weights with no B resident.  CF_ERANGE: n_items > 2^24, 2^32 or more edges, N >
 * CF_TOPN_MAX_N.  CF_ENOMEM: B does not fit.  Empty calls succeed as the mf calls do. */
int cf_ease_fit(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, const uint64_t* user_off, const uint32_t* user_item,
                const float* user_obs, int binary, double lambda);
int cf_ease_gram(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, const uint64_t* user_off, const uint32_t* user_item,
                 const float* user_obs, int binary, double lambda, double* G);
int cf_ease_weights(cf_ctx* ctx, uint32_t* n_items, double* B);
int cf_ease_upload(cf_ctx* ctx, uint32_t n_items, const double* B);
int cf_ease_topn(cf_ctx* ctx, uint32_t n_users, const uint64_t* prof_off, const uint32_t* prof_item,
                 const float* prof_rating, int binary, const uint64_t* excl_off, const uint32_t* excl_item,
                 uint32_t n_sel, const uint32_t* sel_user, uint32_t N, uint32_t* items, double* scores,
                 uint32_t* count, cf_topn_stats* stats);
int cf_ease_rank_eval(cf_ctx* ctx, uint32_t n_users, const uint64_t* prof_off, const uint32_t* prof_item,
                      const float* prof_rating, int binary, const uint64_t* excl_off, const uint32_t* excl_item,
                      const uint64_t* held_off, const uint32_t* held_item, const double* held_w, uint32_t N,
                      uint32_t* rank, cf_rank_user* users, cf_rank_summary* summary);
int cf_ease_timing(cf_ctx* ctx, float ms[3]);
/* P = G^-1 of the same inputs to the host, the fit without its last stage; the resident B is left as
 * it is.  Test helper. */
int cf_debug_ease_inverse(cf_ctx* ctx, uint32_t n_users, uint32_t n_items, const uint64_t* user_off,
                          const uint32_t* user_item, const float* user_obs, int binary, double lambda, double* P);
/* The inversion's block width, the items per workgroup of the score kernel and the profile entries
 * in flight per lane there: constants of cf_ease.hip; test helpers, need no GPU. */
int cf_debug_ease_block(void);
int cf_debug_ease_cols(void);
int cf_debug_ease_unroll(void);

#ifdef __cplusplus
}
#endif
#endif /* CF_ABI_H */
