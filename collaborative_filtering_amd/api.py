"""Host-side mirror of the reference's hot-path operators over the HIP C ABI.

Names follow the reference (compute_eigens, neigh_program::apply, weights_calc,
knn_program): each function below states the reference interface it stands in for.
Inputs are numpy arrays (host) or torch CUDA tensors for the *_run device paths.
"""
from __future__ import annotations

from ctypes import byref, c_double, c_float, c_int, c_uint32, c_void_p
from dataclasses import dataclass

import numpy as np

from . import _native
from ._native import CF_ERANGE, CF_FILTER_BINOMIAL, CF_FILTER_CHEBY, CF_SIGS_COMPAT, CF_SIGS_OWN, NativeError, ptr


def _check(lib, ctx, rc, what):
    if rc != _native.CF_OK:
        msg = lib.cf_last_error(ctx)
        raise NativeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def evec_offsets(item_off: np.ndarray) -> tuple[np.ndarray, int]:
    """Per-user eigenvector slot offsets: slot size k*max(k,2) floats."""
    k = np.diff(item_off.astype(np.int64))
    slots = k * np.maximum(k, 2)
    off = np.zeros(len(k), dtype=np.uint64)
    if len(k):
        off[1:] = np.cumsum(slots)[:-1]
    return off, int(slots.sum())


@dataclass
class EigenResult:
    """Per-user eigen blocks in the flat layout of cf_eigen_batch (cf_abi.h)."""

    item_off: np.ndarray  # uint64[n_users+1]
    evec_off: np.ndarray  # uint64[n_users]
    m: np.ndarray         # int32[n_users]
    sigs: np.ndarray      # float32[item_off[-1]]
    evals: np.ndarray     # float32[item_off[-1]] (first min(m,k) valid)
    evecs: np.ndarray     # float32 flat (k x m row-major at evec_off[u])

    def block(self, u: int):
        b, e = int(self.item_off[u]), int(self.item_off[u + 1])
        k, m = e - b, int(self.m[u])
        ev = np.zeros(m, dtype=np.float32)
        ev[: min(m, k)] = self.evals[b : b + min(m, k)]
        o = int(self.evec_off[u])
        U = self.evecs[o : o + k * m].reshape(k, m)
        return self.sigs[b:e], ev, U


@dataclass
class AlsResult:
    """Outcome of Context.als_fit: fitted factors, per-vertex update counts and residuals
    (user side, item side) and the cf_als_stats of the run."""

    U: np.ndarray
    V: np.ndarray
    nupdates_user: np.ndarray
    nupdates_item: np.ndarray
    residual_user: np.ndarray
    residual_item: np.ndarray
    supersteps: int
    updates: int
    n_not_pd: int
    update_ms: float
    scatter_ms: float

    @property
    def nupdates(self):
        return self.nupdates_user, self.nupdates_item

    @property
    def residual(self):
        return self.residual_user, self.residual_item


@dataclass
class IalsResult:
    """Outcome of Context.ials_fit: fitted factors, the loss after each half-sweep (2 * n_sweeps
    values) and the cf_ials_stats of the run."""

    U: np.ndarray
    V: np.ndarray
    loss_trace: np.ndarray
    sweeps: int
    n_not_pd: int
    gram_ms: float
    update_ms: float
    loss_ms: float


@dataclass
class NmfResult:
    """Outcome of Context.nmf_fit: fitted factors, the loss after each half-sweep (2 * n_sweeps
    values) and the cf_nmf_stats of the run."""

    U: np.ndarray
    V: np.ndarray
    loss_trace: np.ndarray
    sweeps: int
    n_floored: int
    sum_ms: float
    update_ms: float
    loss_ms: float


@dataclass
class BprResult:
    """Outcome of Context.bpr_fit: fitted factors, the item biases (None without), the trace (one
    row {sum of softplus(-x), triples} per sweep run; empty without) and the cf_bpr_stats of the
    run; stage_ms is cf_bpr_timing: sample, negative lists, user / item positive / item negative
    reduction, commit."""

    U: np.ndarray
    V: np.ndarray
    bias_item: np.ndarray | None
    loss_trace: np.ndarray
    sweeps: int
    triples: int
    n_skipped: int
    n_nan: int
    sample_ms: float
    reduce_ms: float
    apply_ms: float
    stage_ms: np.ndarray


@dataclass
class SgdResult:
    """Outcome of Context.sgd_fit: fitted factors and biases (None for plain SGD), per-vertex
    update counts, the trace (one row {sum sq err TRAIN, sum sq err VALIDATE} per user
    superstep) and the cf_sgd_stats of the run; user_reduce_ms / item_reduce_ms split
    reduce_ms by side (cf_sgd_timing)."""

    U: np.ndarray
    V: np.ndarray
    bias_user: np.ndarray | None
    bias_item: np.ndarray | None
    nupdates_user: np.ndarray
    nupdates_item: np.ndarray
    trace: np.ndarray
    global_mean: float
    supersteps: int
    updates: int
    messages: int
    n_nan: int
    gamma_next: float
    reduce_ms: float
    apply_ms: float
    user_reduce_ms: float
    item_reduce_ms: float

    @property
    def nupdates(self):
        return self.nupdates_user, self.nupdates_item


@dataclass
class SvdppResult:
    """Outcome of Context.svdpp_fit: the four fitted matrices (U, W per user; V, Y per item), the
    biases, per-vertex update counts, the trace (one row {sum sq err TRAIN, sum sq err VALIDATE}
    per user superstep of either phase, without Y) and the cf_svdpp_stats of the run; steps_next
    holds the five steps the next user superstep would use (user_bias, item_bias, user_factor,
    item_factor, item_factor2); the three *_reduce_ms split reduce_ms by kernel kind."""

    U: np.ndarray
    V: np.ndarray
    W: np.ndarray
    Y: np.ndarray
    bias_user: np.ndarray
    bias_item: np.ndarray
    nupdates_user: np.ndarray
    nupdates_item: np.ndarray
    trace: np.ndarray
    global_mean: float
    supersteps: int
    updates: int
    messages: int
    n_nan: int
    steps_next: np.ndarray
    reduce_ms: float
    apply_ms: float
    phase1_reduce_ms: float
    user_reduce_ms: float
    item_reduce_ms: float

    @property
    def nupdates(self):
        return self.nupdates_user, self.nupdates_item


@dataclass
class SvdResult:
    """Outcome of Context.svd_fit: sigma and errest (nv entries; positions no pass reached are
    NaN), err (the residual error of the min(nsv, nconv) reported triplets), U (rows x nsv) and V
    (cols x nsv) with the reported triplets in their first columns, kk of every pass, the first
    pass's alpha and beta, and the cf_svd_stats of the run."""

    sigma: np.ndarray
    errest: np.ndarray
    err: np.ndarray
    U: np.ndarray
    V: np.ndarray
    kk_pass: np.ndarray
    alpha_first: np.ndarray
    beta_first: np.ndarray
    nconv: int
    passes: int
    products: int
    matvec_ms: float
    ortho_ms: float
    rotate_ms: float


@dataclass
class TopnResult:
    """Outcome of Context.mf_topn: per selected user j the count[j] best candidate items
    items[j, :count[j]] with their scores, ordered by score descending and, among equal scores,
    item ascending; the tail of a row is UINT32_MAX / 0.0.  stats is the cf_topn_stats of the
    call (blocks, n_nan, score_ms, select_ms)."""

    items: np.ndarray    # uint32[n_selected, N]
    scores: np.ndarray   # float64[n_selected, N]
    count: np.ndarray    # uint32[n_selected]
    stats: "_native.TopnStats"


@dataclass
class SplitResult:
    """Outcome of Context.holdout_split: part[i] of the i-th edge read (0 TRAIN, 1 VALIDATE, or the fold
    number; CF_SPLIT_DROPPED = 255 for a repeated pair's earlier lines and for edges outside the core)
    and the cf_holdout_split stats as named fields.  In the folds mode train / validate count the
    edges of folds 0 and 1 and items_without_train is 0."""

    part: np.ndarray   # uint8[n], read order
    kept: int                  # edges left after duplicates
    alive: int                 # edges alive after the core
    users_alive: int
    items_alive: int
    train: int
    validate: int
    items_without_train: int   # alive items whose every alive edge was held out
    rounds: int                # core rounds in which an edge died


# cf_rank_user (cf_abi.h) as a numpy record: the per-user arrays of RankEvalResult are its fields
RANK_USER_DTYPE = np.dtype([("n_cand", np.uint32), ("n_rel", np.uint32), ("hits", np.uint32), ("reserved", np.uint32),
                            ("precision", np.float64), ("recall", np.float64), ("ndcg", np.float64),
                            ("ap", np.float64), ("rr", np.float64), ("auc", np.float64)])


@dataclass
class RankEvalResult:
    """Outcome of Context.mf_rank_eval.  rank[e] is the 0-based rank of the caller's e-th held-out
    edge among its user's candidates (UINT32_MAX: the item is excluded or its score is NaN) and
    n_cand[e] that user's candidate count (0 when none of the user's edges has a rank); users is one
    RANK_USER_DTYPE record per user (users["ndcg"], ..; all zeros for a user that is not evaluated);
    summary holds the means over the evaluated users, mpr and the edge counts; stats the
    cf_rank_summary of the call (blocks, score_ms, rank_ms besides the summary's own fields)."""

    rank: np.ndarray     # uint32[n_edges], the caller's edge order
    n_cand: np.ndarray   # uint32[n_edges]
    users: np.ndarray    # RANK_USER_DTYPE[n_users]
    summary: dict
    stats: "_native.RankSummary"


def _csr(row, col, obs, n_rows):
    """Stable CSR of an edge list by row (edges of one row keep their input order)."""
    perm = np.argsort(row, kind="stable")
    off = np.zeros(n_rows + 1, dtype=np.uint64)
    if n_rows:
        off[1:] = np.cumsum(np.bincount(row, minlength=n_rows))
    return off, np.ascontiguousarray(col[perm]), np.ascontiguousarray(obs[perm])


def _exclusion_csr(exclude, n_users):
    """(excl_off, excl_item) of the (user, item) pairs to leave out, or (None, None)."""
    if exclude is None:
        return None, None
    eu = np.ascontiguousarray(exclude[0], dtype=np.uint32)
    ei = np.ascontiguousarray(exclude[1], dtype=np.uint32)
    if len(eu) != len(ei):
        raise ValueError("exclude holds different numbers of users and items")
    if len(eu) and int(eu.max()) >= n_users:
        raise ValueError("excluded user index out of range")
    eoff, eitem, _ = _csr(eu, ei, np.zeros(len(eu), np.float32), n_users)
    if not len(eitem):
        eitem = np.zeros(1, np.uint32)   # a valid pointer for an empty list
    return eoff, eitem


def _held_csr(held, n_users):
    """The held-out (user, item[, weight]) pairs as the CSR the library wants (by user, then item):
    (sorted users, the permutation, held_off, held_item, held_w or None)."""
    hu = np.ascontiguousarray(held[0], dtype=np.uint32)
    hi = np.ascontiguousarray(held[1], dtype=np.uint32)
    hw = None if len(held) < 3 or held[2] is None else np.ascontiguousarray(held[2], dtype=np.float64)
    if len(hu) != len(hi) or (hw is not None and len(hw) != len(hu)):
        raise ValueError("held holds different numbers of users, items and weights")
    if len(hu) and int(hu.max()) >= n_users:
        raise ValueError("held-out user index out of range")
    perm = np.lexsort((hi, hu))   # by user, then item: the CSR the library wants
    su, si = hu[perm], hi[perm]
    if len(su) > 1 and bool(np.any((su[1:] == su[:-1]) & (si[1:] == si[:-1]))):
        raise ValueError("held holds a pair twice")
    hoff = np.zeros(n_users + 1, dtype=np.uint64)
    if n_users:
        hoff[1:] = np.cumsum(np.bincount(su, minlength=n_users))
    hitem = np.ascontiguousarray(si) if len(si) else np.zeros(1, np.uint32)
    hws = None if hw is None else (np.ascontiguousarray(hw[perm]) if len(hw) else np.zeros(1))
    return su, perm, hoff, hitem, hws


def _rank_result(su, perm, rank, users, st):
    """RankEvalResult from the library's CSR-ordered ranks, back in the caller's edge order."""
    out_rank = np.zeros(len(su), dtype=np.uint32)
    out_rank[perm] = rank[: len(su)]
    out_cand = np.zeros(len(su), dtype=np.uint32)
    out_cand[perm] = users["n_cand"][su]
    summary = {k: getattr(st, k) for k in ("users_evaluated", "users_auc", "edges_counted", "edges_skipped",
                                           "n_nan_held", "precision", "recall", "ndcg", "map", "mrr", "auc", "mpr")}
    return RankEvalResult(out_rank, out_cand, users, summary, st)


def _mf_source(U, V, bias_user, bias_item, mean):
    """(n_users, the arguments of cf_mf_topn / cf_mf_rank_eval between n_users and the exclusions)."""
    U = np.ascontiguousarray(U, dtype=np.float64)
    V = np.ascontiguousarray(V, dtype=np.float64)
    if U.ndim != 2 or V.ndim != 2 or U.shape[1] != V.shape[1]:
        raise ValueError("U and V must be n_users x D and n_items x D")
    n_users, n_items, D = U.shape[0], V.shape[0], U.shape[1]
    bu = None if bias_user is None else np.ascontiguousarray(bias_user, dtype=np.float64)
    bi = None if bias_item is None else np.ascontiguousarray(bias_item, dtype=np.float64)
    if (bu is not None and len(bu) != n_users) or (bi is not None and len(bi) != n_items):
        raise ValueError("bias_user / bias_item do not hold one value per user / item")
    return n_users, (n_items, D, U, V, bu, bi, float(mean))


_KNN_SCORE_MODES = {"sum": 0, "mean": 1}   # CF_KNN_SCORE_SUM / CF_KNN_SCORE_MEAN

def _mf_factors(mats, ns, names, shapes):
    """The factor matrices of a fit as C-ordered fp64 copies reshaped to (n, D), and D.  D comes
    from whichever side has vertices (an empty side may come as any empty array)."""
    mats = [np.array(x, dtype=np.float64, order="C") for x in mats]
    dims = {a.size // n for a, n in zip(mats, ns) if n}
    if len(dims) > 1:
        raise ValueError(f"{names} differ in D")
    D = dims.pop() if dims else (mats[0].shape[1] if mats[0].ndim == 2 and mats[0].shape[1] else 1)
    if any(a.size != n * D for a, n in zip(mats, ns)):
        raise ValueError(f"{shapes} do not hold n_users x D / n_items x D values")
    return [a.reshape(n, D) for a, n in zip(mats, ns)], D


def _mf_csr_pair(user, item, obs, n_users, n_items):
    """The user CSR and the item CSR of the TRAIN edges, as the six arrays the fits take."""
    if len(user) and (int(user.max()) >= n_users or int(item.max()) >= n_items):
        raise ValueError("edge index out of range")
    return _csr(user, item, obs, n_users) + _csr(item, user, obs, n_items)


def _mf_nupdates(nupdates, n_users, n_items):
    if nupdates is None:
        return [np.zeros(n_users, np.uint32), np.zeros(n_items, np.uint32)]
    return [np.array(nupdates[0], dtype=np.uint32), np.array(nupdates[1], dtype=np.uint32)]


def _mf_trace_rows(trace, max_updates, max_supersteps):
    """One trace row per user superstep, bounded by whichever cap is set."""
    if not trace:
        return 0
    bounds = [(max_supersteps + 1) // 2] if max_supersteps else []
    if max_updates is not None:
        bounds.append(int(max_updates) + 1)
    return min(bounds) if bounds else 0


def _mf_validate(validate):
    if validate is None or not len(validate[0]):
        return None, None, None
    return (np.ascontiguousarray(validate[0], dtype=np.uint32), np.ascontiguousarray(validate[1], dtype=np.uint32),
            np.ascontiguousarray(validate[2], dtype=np.float32))


class Context:
    """One device context (cf_ctx) holding the HBM-resident item graph."""

    def __init__(self, device: int = 0):
        self.lib = _native.load()
        h = c_void_p()
        rc = self.lib.cf_create(device, byref(h))
        if rc != _native.CF_OK:
            raise NativeError(f"cf_create(device={device}) failed ({rc}); is a GPU visible?")
        self.h = h
        self.n_items = 0

    def close(self):
        if self.h:
            self.lib.cf_destroy(self.h)
            self.h = None

    def release_workspaces(self):
        """cf_release_workspaces: free the cached HBM workspaces (the spill paths size theirs
        from free HBM, so one stage's leftover shrinks the next stage's)."""
        self._chk(self.lib.cf_release_workspaces(self.h), "cf_release_workspaces")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        _check(self.lib, self.h, rc, what)

    def set_eigen_method(self, method: str = "jacobi"):
        """'jacobi' (one-sided Jacobi in LDS, default) or 'tridiag' (Householder + batched QL)."""
        code = {"tridiag": _native.CF_EIGEN_TRIDIAG, "jacobi": _native.CF_EIGEN_JACOBI}[method]
        self._chk(self.lib.cf_set_eigen_method(self.h, code), "cf_set_eigen_method")

    def set_jacobi(self, tol_scale: float = 1.0, max_sweeps: int = 30):
        self._chk(self.lib.cf_set_jacobi(self.h, tol_scale, max_sweeps), "cf_set_jacobi")

    def set_eigen_refine(self, enable: bool = True, stop_rel: float = 1e-3, delta: float = 1e-2):
        """Jacobi sweeps to stop_rel, then the first-order Gram refinement (cf_set_eigen_refine)."""
        self._chk(self.lib.cf_set_eigen_refine(self.h, int(enable), stop_rel, delta), "cf_set_eigen_refine")

    def set_eigen_split(self, enable=True):
        """Jacobi sweeps in the split layout, several users per CU (cf_set_eigen_split): False off,
        True the default buckets, or an int 5..12 = the smallest bucket that takes it."""
        self._chk(self.lib.cf_set_eigen_split(self.h, int(enable)), "cf_set_eigen_split")

    def set_eigen_lanes(self, lanes=0):
        """Lanes per column pair of the full-LDS Jacobi kernel in buckets 1-8 (cf_set_eigen_lanes):
        0 the per-bucket default, 4 or 8 that count everywhere.  Same output bits either way."""
        self._chk(self.lib.cf_set_eigen_lanes(self.h, int(lanes)), "cf_set_eigen_lanes")

    def set_pred_pack(self, mode=1):
        """Predictor fast path: small per-rating systems two or four to a wave (cf_set_pred_pack):
        1 on (default), 0 one rating per wave.  Same output bits either way."""
        self._chk(self.lib.cf_set_pred_pack(self.h, int(mode)), "cf_set_pred_pack")

    def set_local_wlim(self, bisect: bool = True):
        """local_calc spill pairs: w_lim by bisection on the movie's B = L2 L2^T (cf_set_local_wlim)."""
        self._chk(self.lib.cf_set_local_wlim(self.h, int(bisect)), "cf_set_local_wlim")

    def set_step_masks(self, enable: bool = True):
        """Eigen runs hand the predictor its complement masks (cf_set_step_masks)."""
        self._chk(self.lib.cf_set_step_masks(self.h, int(enable)), "cf_set_step_masks")

    def debug_stats(self, enable: bool = True, read: bool = False):
        """Jacobi diagnostics (sweeps, per-phase s_memtime cycles) when read."""
        out = np.zeros(8, dtype=np.uint64) if read else None
        self._chk(self.lib.cf_debug_stats(self.h, int(enable), ptr(out)), "cf_debug_stats")
        if read:
            n = max(int(out[1]), 1)
            return {"sweeps_mean": int(out[0]) / n, "users": int(out[1]), "sweeps_max": int(out[2]),
                    "capped": int(out[3]), "assembly_cyc_per_user": int(out[4]) / n,
                    "jacobi_cyc_per_user": int(out[5]) / n, "epilogue_cyc_per_user": int(out[6]) / n,
                    "jacobi_cyc_per_step": int(out[5]) / max(int(out[7]), 1)}
        return None

    def eigen_bucket_timing(self, enable: bool = True, read: bool = False, sweeps: bool = False):
        """cf_eigen_bucket_timing_split: per k-bucket device ms of the last eigen runs (index = emax);
        with sweeps=True also the split-layout buckets' sweep-kernel share (-1 elsewhere)."""
        out = np.zeros(13, dtype=np.float32) if read else None
        sw = np.zeros(13, dtype=np.float32) if read else None
        self._chk(self.lib.cf_eigen_bucket_timing_split(self.h, int(enable), ptr(out), ptr(sw)),
                  "cf_eigen_bucket_timing_split")
        return (out, sw) if sweeps else out

    def debug_spill(self, enable: bool = True, read: bool = False):
        """Spill-path phase cycles (thread 0 s_memtime sums) when read."""
        out = np.zeros(8, dtype=np.uint64) if read else None
        self._chk(self.lib.cf_debug_spill(self.h, int(enable), ptr(out)), "cf_debug_spill")
        if read:
            n = max(int(out[0]), 1)
            names = ["assembly", "tridiag", "accumulate", "ql", "ql_gen"]
            r = {f"{nm}_cyc_per_user": int(out[i + 1]) / n for i, nm in enumerate(names)}
            r.update(users=int(out[0]), ql_iters_per_user=int(out[6]) / n, output_cyc_per_user=int(out[7]) / n)
            return r
        return None

    def debug_tri(self, enable: bool = True, read: bool = False):
        """Tridiagonal-path QL counters when read."""
        out = np.zeros(8, dtype=np.uint64) if read else None
        self._chk(self.lib.cf_debug_tri(self.h, int(enable), ptr(out)), "cf_debug_tri")
        if read:
            n = max(int(out[3]), 1)
            return {"users": int(out[3]), "rotations_per_user": int(out[0]) / n,
                    "ql_iters_per_user": int(out[1]) / n, "overflow_users": int(out[2]),
                    "assembly_cyc_per_user": int(out[4]) / n, "householder_cyc_per_user": int(out[5]) / n,
                    "q_accum_cyc_per_user": int(out[6]) / n, "k_mean": int(out[7]) / n}
        return None

    def debug_phases(self, enable: bool = True, read: bool = False):
        """Predictor phase cycles {setup, basis, fast, block} and rating counts; see cf_abi.h."""
        out = np.zeros(16, dtype=np.uint64) if read else None
        self._chk(self.lib.cf_debug_phases(self.h, int(enable), ptr(out)), "cf_debug_phases")
        if read:
            names = ["setup", "basis", "fast", "dense", "n_fast", "n_dense", "gram", "wide",
                     "w_gather", "w_ldlt", "w_fast", "cyc_n14", "cyc_n30", "cyc_nbig", "n_n14", "n_n30"]
            return dict(zip(names, map(int, out)))
        return None

    # -- item graph (out_fin_) ---------------------------------------------------
    def upload_graph_dense(self, W):
        """W: n_items x n_items float32 (numpy, or torch CUDA tensor)."""
        n = int(W.shape[0])
        on_dev = int(hasattr(W, "is_cuda") and W.is_cuda)
        if not on_dev:
            W = np.ascontiguousarray(W, dtype=np.float32)
        self._chk(self.lib.cf_item_graph_upload_dense(self.h, n, ptr(W), on_dev), "cf_item_graph_upload_dense")
        self.n_items = n

    def upload_graph_csr(self, n_items: int, row_ptr, col, w):
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        col = np.ascontiguousarray(col, dtype=np.uint32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        self._chk(self.lib.cf_item_graph_upload(self.h, n_items, ptr(row_ptr), ptr(col), ptr(w)),
                  "cf_item_graph_upload")
        self.n_items = n_items

    def set_graph_layout(self, layout: str = "dense"):
        """'dense' (n^2 fp32) or 'csr' (row pointers, ascending columns, weights) for the next
        graph upload (cf_set_graph_layout)."""
        code = {"dense": _native.CF_GRAPH_DENSE, "csr": _native.CF_GRAPH_CSR}[layout]
        self._chk(self.lib.cf_set_graph_layout(self.h, code), "cf_set_graph_layout")

    def graph_info(self):
        """(layout name, n_items, stored edges) of the resident graph."""
        lay, n, nnz = c_int(), c_uint32(), np.zeros(1, np.uint64)
        self._chk(self.lib.cf_graph_info(self.h, byref(lay), byref(n), ptr(nnz)), "cf_graph_info")
        return ("csr" if lay.value == _native.CF_GRAPH_CSR else "dense"), n.value, int(nnz[0])

    def item_cosine_edges(self, n_items, user_off, items, ratings, w_min=0.01, cnt_min=5, adopt=False, topk=0):
        """knn2 as the compacted edge list (cf_item_cosine_edges): (edge_off[n_items + 1],
        targets, weights) per source, targets ascending; topk > 0 keeps the K largest weights
        per source (cf_set_knn2_topk; ties: lower target ids)."""
        self._chk(self.lib.cf_set_knn2_topk(self.h, int(topk)), "cf_set_knn2_topk")
        user_off = np.ascontiguousarray(user_off, dtype=np.uint64)
        items = np.ascontiguousarray(items, dtype=np.uint32)
        ratings = np.ascontiguousarray(ratings, dtype=np.float32)
        eoff = np.zeros(n_items + 1, np.uint64)
        cnt = np.zeros(1, np.uint64)
        cap = 1 << 20
        while True:
            col = np.zeros(cap, np.uint32)
            w = np.zeros(cap, np.float32)
            rc = self.lib.cf_item_cosine_edges(self.h, len(user_off) - 1, n_items, ptr(user_off), ptr(items),
                                               ptr(ratings), float(w_min), int(cnt_min), int(adopt), ptr(eoff),
                                               ptr(col), ptr(w), cap, ptr(cnt))
            if rc == CF_ERANGE and int(cnt[0]) > cap:
                cap = int(cnt[0])
                continue
            self._chk(rc, "cf_item_cosine_edges")
            break
        if adopt:
            self.n_items = n_items
        n = int(cnt[0])
        return eoff, col[:n], w[:n]

    def graph_device_ptr(self) -> int:
        n = c_uint32()
        p = self.lib.cf_item_graph_device(self.h, byref(n))
        return int(p or 0)

    # -- compute_eigens (precompute_local_threads.cpp:100-213) --------------------
    def eigen_batch(self, item_off, items) -> EigenResult:
        item_off = np.ascontiguousarray(item_off, dtype=np.uint64)
        items = np.ascontiguousarray(items, dtype=np.uint32)
        n_users = len(item_off) - 1
        evec_off, total = evec_offsets(item_off)
        n_entries = int(item_off[-1])
        m = np.zeros(n_users, dtype=np.int32)
        sigs = np.zeros(n_entries, dtype=np.float32)
        evals = np.zeros(n_entries, dtype=np.float32)
        evecs = np.zeros(max(total, 1), dtype=np.float32)
        self._chk(self.lib.cf_eigen_batch(self.h, n_users, ptr(item_off), ptr(items), ptr(evec_off), ptr(m),
                                          ptr(sigs), ptr(evals), ptr(evecs)), "cf_eigen_batch")
        return EigenResult(item_off, evec_off, m, sigs, evals, evecs)

    # -- neigh_program::apply (local_calc_precomp.cpp:217-380) --------------------
    def predict_precomp(self, item_off, items, ratings, m, evals, evec_off, evecs, sigtab,
                        sig_mode=CF_SIGS_COMPAT, want_pred=False):
        """All arrays host numpy; evals/sigtab float64 (parsed out_eigen_).  evecs float64 (text
        out_eigen_), or float32 (the binary form's blocks: cf_predict_precomp_sel_f32, same results
        as the widened blocks)."""
        item_off = np.ascontiguousarray(item_off, dtype=np.uint64)
        items = np.ascontiguousarray(items, dtype=np.uint32)
        ratings = np.ascontiguousarray(ratings, dtype=np.float32)
        m = np.ascontiguousarray(m, dtype=np.int32)
        evals = np.ascontiguousarray(evals, dtype=np.float64)
        evec_off = np.ascontiguousarray(evec_off, dtype=np.uint64)
        f32 = np.asarray(evecs).dtype == np.float32
        evecs = np.ascontiguousarray(evecs, dtype=np.float32 if f32 else np.float64)
        sigtab = np.ascontiguousarray(sigtab, dtype=np.float64)
        n_users = len(item_off) - 1
        n = int(item_off[-1])
        mse = np.zeros(n, dtype=np.float32)
        kk = np.zeros(n, dtype=np.int32)
        pred = np.zeros(n, dtype=np.float64) if want_pred else None
        if f32:
            self._chk(self.lib.cf_predict_precomp_sel_f32(self.h, n_users, ptr(item_off), ptr(items), ptr(ratings),
                                                          ptr(m), ptr(evals), ptr(evec_off), ptr(evecs), ptr(sigtab),
                                                          len(sigtab), int(sig_mode), None, ptr(mse), ptr(kk),
                                                          ptr(pred)),
                      "cf_predict_precomp_sel_f32")
        else:
            self._chk(self.lib.cf_predict_precomp(self.h, n_users, ptr(item_off), ptr(items), ptr(ratings), ptr(m),
                                                  ptr(evals), ptr(evec_off), ptr(evecs), ptr(sigtab), len(sigtab),
                                                  int(sig_mode), ptr(mse), ptr(kk), ptr(pred)),
                      "cf_predict_precomp")
        return (mse, kk, pred) if want_pred else (mse, kk)

    # -- weights_calc (knn2.cpp:127-164) -------------------------------------------
    def item_cosine(self, n_items, user_off, items, ratings, w_min=0.01, cnt_min=5, adopt=False,
                    want_matrix=True):
        """Dense item-weight matrix of knn2 from per-user train ratings (CSR)."""
        user_off = np.ascontiguousarray(user_off, dtype=np.uint64)
        items = np.ascontiguousarray(items, dtype=np.uint32)
        ratings = np.ascontiguousarray(ratings, dtype=np.float32)
        W = np.zeros((n_items, n_items), dtype=np.float32) if want_matrix else None
        self._chk(self.lib.cf_item_cosine(self.h, len(user_off) - 1, n_items, ptr(user_off), ptr(items),
                                          ptr(ratings), float(w_min), int(cnt_min), int(adopt), ptr(W)),
                  "cf_item_cosine")
        if adopt:
            self.n_items = n_items
        return W

    def item_cosine_run(self, n_users, n_items, d_user_off, d_item, d_rating, integer, d_w_out,
                        w_min=0.01, cnt_min=5, stream=None):
        """Device-pointer knn2 (cf_item_cosine_run) on torch CUDA tensors."""
        self._chk(self.lib.cf_item_cosine_run(self.h, n_users, n_items, ptr(d_user_off), ptr(d_item),
                                              ptr(d_rating), int(integer), float(w_min), int(cnt_min),
                                              ptr(d_w_out), c_void_p(stream or 0)), "cf_item_cosine_run")

    def knn2_timing(self):
        """(plane_ms, gemm_ms, path) of the last knn2 launch (waits for it)."""
        a, b, c = c_float(), c_float(), c_int()
        self._chk(self.lib.cf_knn2_timing(self.h, byref(a), byref(b), byref(c)),
                  "cf_knn2_timing")
        return a.value, b.value, c.value

    def set_knn2_chunk(self, users_per_chunk: int = 0):
        """Force the knn2 K-chunk size (users, multiple of 128; 0 = automatic by free HBM)."""
        self._chk(self.lib.cf_set_knn2_chunk(self.h, int(users_per_chunk)), "cf_set_knn2_chunk")

    def knn2_chunks(self):
        n = c_int()
        self._chk(self.lib.cf_knn2_chunks(self.h, byref(n)), "cf_knn2_chunks")
        return n.value

    def knn2_exactness(self):
        """(max accumulator, exact) of the last knn2 launch: exact is True when the
        reference's float accumulators (knn2.cpp:129-140) stay <= 2^24 (cf_knn2_exactness)."""
        a, e = c_double(), c_int()
        self._chk(self.lib.cf_knn2_exactness(self.h, byref(a), byref(e)), "cf_knn2_exactness")
        return a.value, bool(e.value)

    # -- data prep: knn regroup (knn.cpp:83-357), k-fold order (fold_cross_validation.py) --
    def knn_regroup(self, n_users, n_movies, user, movie, rating, validate=None, edg_cap=None):
        """GPU regroup of ratings in read order (compact ids): returns a dict of the train and
        test CSR lists per movie (users ascending, last rating read wins) and the sorted unique
        co-rated movie lists (both roles, self excluded).  edg_cap=None sizes the co-rated
        output from a first call (CF_ERANGE) when n_movies^2 is too large to preallocate."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        movie = np.ascontiguousarray(movie, dtype=np.uint32)
        rating = np.ascontiguousarray(rating, dtype=np.float32)
        val = None if validate is None else np.ascontiguousarray(validate, dtype=np.uint8)
        n = len(user)
        out = {k: np.zeros(n_movies + 1, np.uint64) for k in ("train_off", "test_off", "edg_off")}
        for k in ("train_user", "test_user"):
            out[k] = np.zeros(max(n, 1), np.uint32)
        for k in ("train_rating", "test_rating"):
            out[k] = np.zeros(max(n, 1), np.float32)
        cap = int(edg_cap) if edg_cap is not None else min(n_movies * max(n_movies - 1, 0), 1 << 24)
        while True:
            edg = np.zeros(max(cap, 1), np.uint32)
            rc = self.lib.cf_knn_regroup(self.h, n, n_users, n_movies, ptr(user), ptr(movie), ptr(rating),
                                         ptr(val) if val is not None else None, ptr(out["train_off"]),
                                         ptr(out["train_user"]), ptr(out["train_rating"]), ptr(out["test_off"]),
                                         ptr(out["test_user"]), ptr(out["test_rating"]), ptr(out["edg_off"]),
                                         ptr(edg), cap)
            need = int(out["edg_off"][-1])
            if rc == CF_ERANGE and edg_cap is None and need > cap:
                cap = need
                continue
            self._chk(rc, "cf_knn_regroup")
            break
        out["edg_movie"] = edg[:need]
        for k, o in (("train", "train_off"), ("test", "test_off")):
            m = int(out[o][-1])
            out[k + "_user"] = out[k + "_user"][:m]
            out[k + "_rating"] = out[k + "_rating"][:m]
        return out

    def fold_order(self, user, rank):
        """Rating indices ordered by (rank[user[i]], i) on the GPU (cf_fold_order)."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        rank = np.ascontiguousarray(rank, dtype=np.uint32)
        order = np.zeros(max(len(user), 1), np.uint32)
        self._chk(self.lib.cf_fold_order(self.h, len(user), len(rank), ptr(user), ptr(rank), ptr(order)),
                  "cf_fold_order")
        return order[:len(user)]

    # -- per-user hold-out split and k-core filter (cf_split.hip) ----------------------------------
    def kcore(self, n_users, n_items, user, item, min_user=0, min_item=0):
        """(keep bool[n] in read order, rounds): the last edge read of every (user, item) that lies in
        the (min_user, min_item) core of the bipartite graph (cf_kcore; 0 or 1: no limit)."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        if len(user) != len(item):
            raise ValueError("user and item differ in length")
        keep = np.zeros(max(len(user), 1), np.uint8)
        rounds = c_uint32()
        self._chk(self.lib.cf_kcore(self.h, len(user), int(n_users), int(n_items), ptr(user), ptr(item), int(min_user),
                                    int(min_item), ptr(keep), byref(rounds)), "cf_kcore")
        return keep[:len(user)].astype(bool), rounds.value

    def holdout_split(self, n_users, n_items, user, item, *, holdout=None, ratio=None, folds=None, order_key=None,
                      seed=0, min_train=0, min_user=0, min_item=0) -> SplitResult:
        """Per-user split of the edges (read order, compact ids) after dropping repeated pairs and the
        (min_user, min_item) core filter (cf_holdout_split).  Exactly one of holdout=K (leave K out),
        ratio=(num, den) and folds=F.  Within a user the edges are ordered by (order_key, item); without
        order_key the key is a hash of (seed, user, item), so the split does not depend on the read
        order.  The core runs before the hold-out: a TRAIN degree may end below the core's limit."""
        if (holdout is not None) + (ratio is not None) + (folds is not None) != 1:
            raise ValueError("exactly one of holdout, ratio and folds")
        if holdout is not None:
            mode, a, b = _native.CF_SPLIT_LEAVE_K, int(holdout), 0
        elif ratio is not None:
            mode, a, b = _native.CF_SPLIT_RATIO, int(ratio[0]), int(ratio[1])
        else:
            mode, a, b = _native.CF_SPLIT_FOLDS, int(folds), 0
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        key = None if order_key is None else np.ascontiguousarray(order_key, dtype=np.uint64)
        if len(user) != len(item) or (key is not None and len(key) != len(user)):
            raise ValueError("user, item and order_key differ in length")
        part = np.zeros(max(len(user), 1), np.uint8)
        stats = np.zeros(_native.CF_SPLIT_STATS, np.uint64)
        self._chk(self.lib.cf_holdout_split(self.h, len(user), int(n_users), int(n_items), ptr(user), ptr(item),
                                            ptr(key) if key is not None else None, int(seed), int(min_user),
                                            int(min_item), mode, a, b, int(min_train), ptr(part), ptr(stats)),
                  "cf_holdout_split")
        return SplitResult(part[:len(user)], *(int(s) for s in stats))

    def split_timing(self):
        """Device ms of the last kcore / holdout_split by step: (keys + sort + lists, core rounds, order
        sorts, parts + stats)."""
        ms = (c_float * 4)()
        self._chk(self.lib.cf_split_timing(self.h, ms), "cf_split_timing")
        return tuple(ms)

    def prep_timing(self):
        """Device ms of the last regroup / fold-order / kcore / holdout-split call (HIP events)."""
        t = c_float()
        self._chk(self.lib.cf_prep_timing(self.h, byref(t)), "cf_prep_timing")
        return t.value

    # -- knn_program + error_vertex_data (knn3.cpp:185-256) ------------------------
    def knn_predict(self, user_off, items, ratings):
        """Returns (pred per test rating, per-movie MSE float32, per-movie test count)."""
        user_off = np.ascontiguousarray(user_off, dtype=np.uint64)
        items = np.ascontiguousarray(items, dtype=np.uint32)
        ratings = np.ascontiguousarray(ratings, dtype=np.float32)
        n = int(user_off[-1])
        pred = np.zeros(n, dtype=np.float64)
        mse = np.zeros(self.n_items, dtype=np.float32)
        cnt = np.zeros(self.n_items, dtype=np.uint32)
        self._chk(self.lib.cf_knn_predict(self.h, len(user_off) - 1, ptr(user_off), ptr(items), ptr(ratings),
                                          ptr(pred), ptr(mse), ptr(cnt)), "cf_knn_predict")
        return pred, mse, cnt

    def local_calc(self, movie_off, movie_items, test_off, test_user, test_rating):
        """local_calc (a8).  Returns per test entry (mse float32, kk, pred, w_lim, lim);
        entries of movies that are not processed keep mse = NaN, kk = -1."""
        movie_off = np.ascontiguousarray(movie_off, dtype=np.uint64)
        movie_items = np.ascontiguousarray(movie_items, dtype=np.uint32)
        test_off = np.ascontiguousarray(test_off, dtype=np.uint64)
        test_user = np.ascontiguousarray(test_user, dtype=np.uint32)
        test_rating = np.ascontiguousarray(test_rating, dtype=np.float32)
        n = int(test_off[-1])
        mse = np.full(n, np.nan, dtype=np.float32)
        kk = np.full(n, -1, dtype=np.int32)
        pred = np.full(n, np.nan)
        wlim = np.full(n, np.nan, dtype=np.float32)
        lim = np.full(n, -1, dtype=np.int32)
        self._chk(self.lib.cf_local_calc(self.h, len(movie_off) - 1, ptr(movie_off), ptr(movie_items), ptr(test_off),
                                         ptr(test_user), ptr(test_rating), ptr(mse), ptr(kk), ptr(pred), ptr(wlim),
                                         ptr(lim)), "cf_local_calc")
        return mse, kk, pred, wlim, lim

    def graph_filter(self, kind, n_vertices, va, vb, w, signal, coeff):
        """cheby (CF_FILTER_CHEBY) / binomials (CF_FILTER_BINOMIAL) graph-signal filter
        (cheby.cpp:152-274, binomials.cpp:145-253) over topology lines (va, vb, w) on compact
        vertex ids.  Returns (filtered signal fp64, device ms of the supersteps, directed edges)."""
        va = np.ascontiguousarray(va, dtype=np.uint32)
        vb = np.ascontiguousarray(vb, dtype=np.uint32)
        w = np.ascontiguousarray(w, dtype=np.float64)
        signal = np.ascontiguousarray(signal, dtype=np.float64)
        coeff = np.ascontiguousarray(coeff, dtype=np.float64)
        out = np.zeros(int(n_vertices), dtype=np.float64)
        self._chk(self.lib.cf_graph_filter(self.h, int(kind), int(n_vertices), len(w), ptr(va), ptr(vb), ptr(w),
                                           ptr(signal), ptr(coeff), len(coeff), ptr(out)), "cf_graph_filter")
        ms = np.zeros(1, dtype=np.float32)
        ne = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.cf_graph_filter_timing(self.h, ptr(ms), ptr(ne)), "cf_graph_filter_timing")
        return out, float(ms[0]), int(ne[0])

    # -- ALS matrix factorization (als.cpp:290-371) ---------------------------------
    def als_fit(self, user, item, obs, n_users, n_items, U0, V0, *, lam=0.01, regnormal=True, out_degree=None,
                tol=1e-3, max_updates=None, max_supersteps=0, activate_user=None, nupdates=None,
                residual=None) -> "AlsResult":
        """cf_als_fit over the TRAIN edges (user[e], item[e], obs[e]) from the initial factors
        U0 (n_users x D), V0 (n_items x D).  Regularisation per vertex: regnormal=True is the
        reference's default, lambda * num_out_edges -- out_degree per user (every role; None =
        the TRAIN degree) and 0 for every item (als.cpp:323-327); regnormal="degree" is lambda *
        TRAIN degree on both sides; False is plain lambda.  Superstep 0 updates the users with
        activate_user != 0 (None: those with out_degree > 0, als.cpp:363-367).  nupdates /
        residual: optional (user, item) pairs to continue from."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        n_users, n_items = int(n_users), int(n_items)
        (U, V), D = _mf_factors((U0, V0), (n_users, n_items), "U0 and V0", "U0 / V0")
        uoff, uitem, uobs, ioff, iuser, iobs = _mf_csr_pair(user, item, obs, n_users, n_items)
        du = np.diff(uoff.astype(np.int64)).astype(np.float64)
        di = np.diff(ioff.astype(np.int64)).astype(np.float64)
        od = du if out_degree is None else np.asarray(out_degree, dtype=np.float64)
        if regnormal == "degree":
            ru, ri = lam * du, lam * di
        elif regnormal:
            ru, ri = lam * od, np.zeros(n_items)
        else:
            ru, ri = np.full(n_users, float(lam)), np.full(n_items, float(lam))
        ru = np.ascontiguousarray(ru, dtype=np.float64)
        ri = np.ascontiguousarray(ri, dtype=np.float64)
        act = (od > 0) if activate_user is None else np.asarray(activate_user) != 0
        act = np.ascontiguousarray(act, dtype=np.uint8)
        nu = _mf_nupdates(nupdates, n_users, n_items)
        rs = [np.zeros(n_users, np.float32), np.zeros(n_items, np.float32)] if residual is None else \
            [np.array(residual[0], dtype=np.float32), np.array(residual[1], dtype=np.float32)]
        st = _native.AlsStats()
        cap = (1 << 64) - 1 if max_updates is None else int(max_updates)
        self._chk(self.lib.cf_als_fit(self.h, n_users, n_items, int(D), ptr(uoff), ptr(uitem), ptr(uobs), ptr(ioff),
                                      ptr(iuser), ptr(iobs), ptr(ru), ptr(ri), float(tol), cap, int(max_supersteps),
                                      ptr(U), ptr(V), ptr(nu[0]), ptr(nu[1]), ptr(rs[0]), ptr(rs[1]), ptr(act),
                                      byref(st)), "cf_als_fit")
        return AlsResult(U, V, nu[0], nu[1], rs[0], rs[1], int(st.supersteps), int(st.updates), int(st.n_not_pd),
                         float(st.update_ms), float(st.scatter_ms))

    def als_sum_sq_error(self, user, item, obs, U, V, minval=-1e100, maxval=1e100) -> float:
        """cf_als_error: sum over the edges of (obs - clamp(u.v, minval, maxval))^2."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        U = np.ascontiguousarray(U, dtype=np.float64)
        V = np.ascontiguousarray(V, dtype=np.float64)
        out = c_double()
        self._chk(self.lib.cf_als_error(self.h, len(user), ptr(user), ptr(item), ptr(obs), U.shape[0], V.shape[0],
                                        U.shape[1], ptr(U), ptr(V), float(minval), float(maxval), byref(out)),
                  "cf_als_error")
        return out.value

    def als_rmse(self, user, item, obs, U, V, minval=-1e100, maxval=1e100) -> float:
        """RMSE of one role's edges (error_aggregator::finalize, als.cpp:474-483)."""
        n = len(user)
        return float(np.sqrt(self.als_sum_sq_error(user, item, obs, U, V, minval, maxval) / n)) if n else 0.0

    def als_predict(self, user, item, U, V) -> np.ndarray:
        """cf_als_predict: u.v (unclamped) per (user, item) pair (als.cpp:499-509)."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        U = np.ascontiguousarray(U, dtype=np.float64)
        V = np.ascontiguousarray(V, dtype=np.float64)
        pred = np.zeros(len(user), dtype=np.float64)
        self._chk(self.lib.cf_als_predict(self.h, len(user), ptr(user), ptr(item), U.shape[0], V.shape[0], U.shape[1],
                                          ptr(U), ptr(V), ptr(pred)), "cf_als_predict")
        return pred

    # -- implicit-feedback ALS (Hu, Koren, Volinsky 2008) -----------------------------------
    def _ials_graph(self, user, item, conf, pref, n_users, n_items, lam, reg_user, reg_item):
        """The two CSRs (confidence and preference per edge) and the reg arrays as cf_ials_* take
        them: (uoff, uitem, uconf, upref, ioff, iuser, iconf, ipref, ru, ri); pref None = NULLs."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        conf = np.ascontiguousarray(conf, dtype=np.float32)
        uoff, uitem, uconf, ioff, iuser, iconf = _mf_csr_pair(user, item, conf, n_users, n_items)
        upref = ipref = None
        if pref is not None:
            pref = np.ascontiguousarray(pref, dtype=np.float32)
            upref, ipref = _csr(user, item, pref, n_users)[2], _csr(item, user, pref, n_items)[2]
        ru = np.full(n_users, float(lam)) if reg_user is None else np.ascontiguousarray(reg_user, dtype=np.float64)
        ri = np.full(n_items, float(lam)) if reg_item is None else np.ascontiguousarray(reg_item, dtype=np.float64)
        if len(ru) != n_users or len(ri) != n_items:
            raise ValueError("reg_user / reg_item do not hold one value per vertex")
        return uoff, uitem, uconf, upref, ioff, iuser, iconf, ipref, ru, ri

    def ials_fit(self, user, item, conf, n_users, n_items, U0, V0, *, pref=None, lam=0.1, reg_user=None,
                 reg_item=None, n_sweeps=10, trace=True) -> "IalsResult":
        """cf_ials_fit: n_sweeps sweeps of implicit-feedback ALS over the edges (user[e], item[e])
        with confidence conf[e] >= 1 and preference pref[e] (None: all ones); every other pair of
        the grid is preference 0 with confidence 1.  Regularisation per vertex: reg_user /
        reg_item, or lam everywhere.  trace=False skips the loss evaluations."""
        n_users, n_items, n_sweeps = int(n_users), int(n_items), int(n_sweeps)
        (U, V), D = _mf_factors((U0, V0), (n_users, n_items), "U0 and V0", "U0 / V0")
        g = self._ials_graph(user, item, conf, pref, n_users, n_items, lam, reg_user, reg_item)
        loss = np.zeros(2 * n_sweeps, dtype=np.float64) if trace else None
        st = _native.IalsStats()
        self._chk(self.lib.cf_ials_fit(self.h, n_users, n_items, int(D), *[ptr(x) for x in g], n_sweeps, ptr(U), ptr(V),
                                       ptr(loss), byref(st)), "cf_ials_fit")
        return IalsResult(U, V, loss if trace else np.zeros(0), int(st.sweeps), int(st.n_not_pd), float(st.gram_ms),
                          float(st.update_ms), float(st.loss_ms))

    def ials_loss(self, user, item, conf, n_users, n_items, U, V, *, pref=None, lam=0.1, reg_user=None,
                  reg_item=None) -> float:
        """cf_ials_loss: the implicit-feedback loss of any factors over the whole grid."""
        n_users, n_items = int(n_users), int(n_items)
        (U, V), D = _mf_factors((U, V), (n_users, n_items), "U and V", "U / V")
        g = self._ials_graph(user, item, conf, pref, n_users, n_items, lam, reg_user, reg_item)
        out = c_double()
        self._chk(self.lib.cf_ials_loss(self.h, n_users, n_items, int(D), *[ptr(x) for x in g], ptr(U), ptr(V),
                                        byref(out)), "cf_ials_loss")
        return out.value

    def mf_gram(self, F) -> np.ndarray:
        """cf_mf_gram: F^T F (D x D) of an n x D matrix, summed in slices of fixed length."""
        F = np.ascontiguousarray(F, dtype=np.float64)
        if F.ndim != 2 or F.shape[1] == 0:
            raise ValueError("F must be n x D with D >= 1")
        G = np.zeros((F.shape[1], F.shape[1]), dtype=np.float64)
        self._chk(self.lib.cf_mf_gram(self.h, F.shape[0], F.shape[1], ptr(F), ptr(G)), "cf_mf_gram")
        return G

    # -- KL-divergence NMF, observed pairs or the whole grid ----------------------------------
    def _nmf_graph(self, user, item, obs, n_users, n_items, mode):
        """The two CSRs as cf_nmf_* take them and the mode constant."""
        modes = {"observed": _native.CF_NMF_OBSERVED, "grid": _native.CF_NMF_GRID}
        if mode not in modes:
            raise ValueError('mode must be "grid" or "observed"')
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        return _mf_csr_pair(user, item, obs, n_users, n_items), modes[mode]

    def nmf_fit(self, user, item, obs, n_users, n_items, U0, V0, *, mode="grid", n_sweeps=10, trace=True) -> "NmfResult":
        """cf_nmf_fit: n_sweeps sweeps of the multiplicative KL-divergence updates over the edges
        (user[e], item[e], obs[e] >= 0) from positive initial factors (every component >=
        CF_NMF_EPS).  mode="observed" fits the rated pairs only; mode="grid" fits every pair of the
        n_users x n_items grid with the unrated ones equal to 0.  trace=False skips the loss
        evaluations."""
        n_users, n_items, n_sweeps = int(n_users), int(n_items), int(n_sweeps)
        (U, V), D = _mf_factors((U0, V0), (n_users, n_items), "U0 and V0", "U0 / V0")
        g, m = self._nmf_graph(user, item, obs, n_users, n_items, mode)
        loss = np.zeros(2 * n_sweeps, dtype=np.float64) if trace else None
        st = _native.NmfStats()
        self._chk(self.lib.cf_nmf_fit(self.h, n_users, n_items, int(D), *[ptr(x) for x in g], m, n_sweeps, ptr(U), ptr(V),
                                      ptr(loss), byref(st)), "cf_nmf_fit")
        return NmfResult(U, V, loss if trace else np.zeros(0), int(st.sweeps), int(st.n_floored), float(st.sum_ms),
                         float(st.update_ms), float(st.loss_ms))

    def nmf_loss(self, user, item, obs, n_users, n_items, U, V, *, mode="grid") -> float:
        """cf_nmf_loss: the generalised KL loss of any positive factors, in either mode."""
        n_users, n_items = int(n_users), int(n_items)
        (U, V), D = _mf_factors((U, V), (n_users, n_items), "U and V", "U / V")
        g, m = self._nmf_graph(user, item, obs, n_users, n_items, mode)
        out = c_double()
        self._chk(self.lib.cf_nmf_loss(self.h, n_users, n_items, int(D), *[ptr(x) for x in g], m, ptr(U), ptr(V),
                                       byref(out)), "cf_nmf_loss")
        return out.value

    def mf_colsum(self, F) -> np.ndarray:
        """cf_mf_colsum: the column sums (D) of an n x D matrix, summed in slices of fixed length."""
        F = np.ascontiguousarray(F, dtype=np.float64)
        if F.ndim != 2 or F.shape[1] == 0:
            raise ValueError("F must be n x D with D >= 1")
        s = np.zeros(F.shape[1], dtype=np.float64)
        self._chk(self.lib.cf_mf_colsum(self.h, F.shape[0], F.shape[1], ptr(F), ptr(s)), "cf_mf_colsum")
        return s

    # -- Bayesian Personalized Ranking (no reference counterpart) -----------------------------
    @staticmethod
    def _bpr_graph(user, item, n_users, n_items):
        """The positive pairs sorted by (user, item) as the user CSR and its transpose:
        (user_off, user_item, item_off, item_user).  A repeated pair raises ValueError."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        if len(user) != len(item):
            raise ValueError("user and item differ in length")
        if len(user) and (int(user.max()) >= n_users or int(item.max()) >= n_items):
            raise ValueError("edge index out of range")
        p = np.lexsort((item, user))
        user, item = user[p], item[p]
        if len(user) > 1 and bool(np.any((user[1:] == user[:-1]) & (item[1:] == item[:-1]))):
            raise ValueError("a positive pair appears twice")
        none = np.zeros(len(user), np.float32)
        uoff, uitem, _ = _csr(user, item, none, n_users)
        ioff, iuser, _ = _csr(item, user, none, n_items)   # stable: users ascend within an item
        return uoff, uitem, ioff, iuser

    def bpr_fit(self, user, item, n_users, n_items, U0, V0, *, bias0=None, lr=0.05, reg_user=0.01, reg_item=0.01,
                reg_bias=0.01, n_sweeps=10, seed=0, first_sweep=0, trace=True) -> "BprResult":
        """cf_bpr_fit: n_sweeps Jacobi sweeps of BPR over the positive pairs (user[e], item[e]), one
        sampled negative per pair and sweep (cf_abi.h has the rule).  bias0: initial item biases,
        None for a model without.  first_sweep continues an earlier fit: its sweeps draw the
        negatives of sweep indices first_sweep, first_sweep + 1, ..  The pairs may come in any
        order; a repeated pair raises ValueError."""
        n_users, n_items, n_sweeps = int(n_users), int(n_items), int(n_sweeps)
        (U, V), D = _mf_factors((U0, V0), (n_users, n_items), "U0 and V0", "U0 / V0")
        b = None if bias0 is None else np.array(bias0, dtype=np.float64, order="C").reshape(-1)
        if b is not None and len(b) != n_items:
            raise ValueError("bias0 does not hold one value per item")
        if b is not None and not len(b):
            b = np.zeros(1)   # a valid pointer: the model has a bias
        g = self._bpr_graph(user, item, n_users, n_items)
        loss = np.zeros(2 * n_sweeps, dtype=np.float64) if trace else None
        par = _native.BprParams(float(lr), float(reg_user), float(reg_item), float(reg_bias), int(seed), int(first_sweep),
                                n_sweeps)
        st = _native.BprStats()
        self._chk(self.lib.cf_bpr_fit(self.h, n_users, n_items, int(D), *[ptr(x) for x in g], byref(par), ptr(U), ptr(V),
                                      ptr(b), ptr(loss), byref(st)), "cf_bpr_fit")
        ms = np.zeros(6, dtype=np.float32)
        self._chk(self.lib.cf_bpr_timing(self.h, ptr(ms)), "cf_bpr_timing")
        tr = loss.reshape(n_sweeps, 2)[: int(st.sweeps)] if trace else np.zeros((0, 2))
        return BprResult(U, V, None if b is None else b[:n_items], tr, int(st.sweeps), int(st.triples), int(st.n_skipped),
                         int(st.n_nan), float(st.sample_ms), float(st.reduce_ms), float(st.apply_ms), ms)

    def bpr_sample(self, user, item, n_users, n_items, *, seed=0, sweep=0):
        """cf_bpr_sample: (neg, n_skipped) with neg[p] the negative item of the p-th positive pair in
        (user, item) order for that seed and sweep index, 0xFFFFFFFF where the pair is skipped."""
        n_users, n_items = int(n_users), int(n_items)
        uoff, uitem, _, _ = self._bpr_graph(user, item, n_users, n_items)
        neg = np.full(max(len(uitem), 1), 0xFFFFFFFF, dtype=np.uint32)
        skipped = _native.c_uint64()
        self._chk(self.lib.cf_bpr_sample(self.h, n_users, n_items, ptr(uoff), ptr(uitem), int(seed), int(sweep), ptr(neg),
                                         byref(skipped)), "cf_bpr_sample")
        return neg[: len(uitem)], int(skipped.value)

    # -- SGD / bias-SGD matrix factorization (sgd.cpp, biassgd.cpp) ----------------------
    def sgd_fit(self, user, item, obs, n_users, n_items, U0, V0, *, bias=False, lam=0.001, gamma=0.001, step_dec=0.9,
                tol=1e-3, minval=-1e100, maxval=1e100, global_mean=None, bias_user=None, bias_item=None,
                max_updates=None, max_supersteps=0, activate_user=None, nupdates=None, validate=None,
                trace=True) -> "SgdResult":
        """cf_sgd_fit over the TRAIN edges (user[e], item[e], obs[e]) from the initial factors U0
        (n_users x D), V0 (n_items x D).  bias=True is bias-SGD: biases start at bias_user /
        bias_item (None: zeros) and global_mean defaults to the fp64 mean of the TRAIN ratings
        (biassgd.cpp:684-686).  Superstep 0 updates the users with activate_user != 0 (None:
        every user).  One of max_updates / max_supersteps is mandatory (the reference never stops
        without a cap).  validate: optional (user, item, obs) of the VALIDATE edges for the
        trace's second column.  nupdates: optional (user, item) pair to continue from."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        n_users, n_items = int(n_users), int(n_items)
        (U, V), D = _mf_factors((U0, V0), (n_users, n_items), "U0 and V0", "U0 / V0")
        uoff, uitem, uobs, ioff, iuser, iobs = _mf_csr_pair(user, item, obs, n_users, n_items)
        bu = bi = None
        mean = 0.0
        if bias:
            bu = np.zeros(n_users) if bias_user is None else np.array(bias_user, dtype=np.float64)
            bi = np.zeros(n_items) if bias_item is None else np.array(bias_item, dtype=np.float64)
            if global_mean is None:
                mean = float(obs.astype(np.float64).sum() / len(obs)) if len(obs) else 0.0
            else:
                mean = float(global_mean)
        act = None if activate_user is None else np.ascontiguousarray(np.asarray(activate_user) != 0, dtype=np.uint8)
        nu = _mf_nupdates(nupdates, n_users, n_items)
        cap = (1 << 64) - 1 if max_updates is None else int(max_updates)
        max_supersteps = int(max_supersteps)
        rows = _mf_trace_rows(trace, max_updates, max_supersteps)
        tr = np.zeros((max(rows, 1), 2))
        vu, vi, vo = _mf_validate(validate)
        par = _native.SgdParams(float(lam), float(gamma), float(step_dec), float(tol), float(minval), float(maxval),
                                mean, cap, max_supersteps)
        st = _native.SgdStats()
        self._chk(self.lib.cf_sgd_fit(self.h, n_users, n_items, int(D), ptr(uoff), ptr(uitem), ptr(uobs), ptr(ioff),
                                      ptr(iuser), ptr(iobs), byref(par), ptr(U), ptr(V), ptr(bu), ptr(bi), ptr(nu[0]),
                                      ptr(nu[1]), ptr(act), 0 if vu is None else len(vu), ptr(vu), ptr(vi), ptr(vo),
                                      ptr(tr) if rows else None, rows, byref(st)), "cf_sgd_fit")
        ums, ims = c_float(), c_float()
        self._chk(self.lib.cf_sgd_timing(self.h, byref(ums), byref(ims)), "cf_sgd_timing")
        done = min(rows, (int(st.supersteps) + 1) // 2)
        return SgdResult(U, V, bu, bi, nu[0], nu[1], tr[:done].copy(), mean, int(st.supersteps), int(st.updates),
                         int(st.messages), int(st.n_nan), float(st.gamma_next), float(st.reduce_ms), float(st.apply_ms),
                         float(ums.value), float(ims.value))

    def sgd_sum_sq_error(self, user, item, obs, U, V, bias_user=None, bias_item=None, global_mean=0.0,
                         minval=-1e100, maxval=1e100) -> float:
        """cf_sgd_error: sum over the edges of (obs - clamp(mean + bu + bi + u.v, minval, maxval))^2;
        without biases the mean is ignored (plain SGD)."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        U = np.ascontiguousarray(U, dtype=np.float64)
        V = np.ascontiguousarray(V, dtype=np.float64)
        bu = None if bias_user is None else np.ascontiguousarray(bias_user, dtype=np.float64)
        bi = None if bias_item is None else np.ascontiguousarray(bias_item, dtype=np.float64)
        out = c_double()
        self._chk(self.lib.cf_sgd_error(self.h, len(user), ptr(user), ptr(item), ptr(obs), U.shape[0], V.shape[0],
                                        U.shape[1], ptr(U), ptr(V), ptr(bu), ptr(bi), float(global_mean), float(minval),
                                        float(maxval), byref(out)), "cf_sgd_error")
        return out.value

    def sgd_rmse(self, user, item, obs, U, V, bias_user=None, bias_item=None, global_mean=0.0, minval=-1e100,
                 maxval=1e100) -> float:
        """RMSE of one role's edges (error_aggregator::finalize, sgd.cpp:372-387)."""
        n = len(user)
        if not n:
            return 0.0
        return float(np.sqrt(self.sgd_sum_sq_error(user, item, obs, U, V, bias_user, bias_item, global_mean, minval,
                                                   maxval) / n))

    def sgd_predict(self, user, item, U, V, bias_user=None, bias_item=None, global_mean=0.0, clamp=None,
                    minval=-1e100, maxval=1e100) -> np.ndarray:
        """cf_sgd_predict per (user, item) pair.  clamp None: as the reference's savers, clamped
        with biases (biassgd.cpp:423-428), unclamped without (sgd.cpp:418-419)."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        U = np.ascontiguousarray(U, dtype=np.float64)
        V = np.ascontiguousarray(V, dtype=np.float64)
        bu = None if bias_user is None else np.ascontiguousarray(bias_user, dtype=np.float64)
        bi = None if bias_item is None else np.ascontiguousarray(bias_item, dtype=np.float64)
        if clamp is None:
            clamp = bu is not None
        pred = np.zeros(len(user), dtype=np.float64)
        self._chk(self.lib.cf_sgd_predict(self.h, len(user), ptr(user), ptr(item), U.shape[0], V.shape[0], U.shape[1],
                                          ptr(U), ptr(V), ptr(bu), ptr(bi), float(global_mean), int(bool(clamp)),
                                          float(minval), float(maxval), ptr(pred)), "cf_sgd_predict")
        return pred

    # -- SVD++ matrix factorization (svdpp.cpp) ---------------------------------------------
    def svdpp_fit(self, user, item, obs, n_users, n_items, U0, V0, W0, Y0, *, implicit=None, user_bias_step=1e-4,
                  user_bias_reg=1e-4, item_bias_step=1e-4, item_bias_reg=1e-4, user_factor_step=1e-4,
                  user_factor_reg=1e-4, item_factor_step=1e-4, item_factor_reg=1e-4, item_factor2_step=1e-4,
                  item_factor2_reg=1e-4, step_dec=0.9, minval=-1e100, maxval=1e100, global_mean=None, bias_user=None,
                  bias_item=None, max_updates=None, max_supersteps=0, activate_user=None, nupdates=None,
                  validate=None, trace=True) -> "SvdppResult":
        """cf_svdpp_fit over the TRAIN edges (user[e], item[e], obs[e]) from the initial U0, W0
        (n_users x D) and V0, Y0 (n_items x D).  implicit: optional (user, item) pairs of the
        non-TRAIN edges (VALIDATE and PREDICT), which enter W_u and the phase-1 signalling.  The
        ten hyper-parameters are rounded to float32 (svdpp.cpp:49-58).  Biases start at bias_user /
        bias_item (None: zeros); global_mean defaults to the fp64 mean of the TRAIN ratings.  One
        of max_updates / max_supersteps is mandatory; max_updates counts phase-1 and phase-2
        updates alike.  validate, nupdates, activate_user: as sgd_fit."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        n_users, n_items = int(n_users), int(n_items)
        (U, V, W, Y), D = _mf_factors((U0, V0, W0, Y0), (n_users, n_items, n_users, n_items), "U0, V0, W0 and Y0",
                                      "U0 / W0 / V0 / Y0")
        uoff, uitem, uobs, ioff, iuser, iobs = _mf_csr_pair(user, item, obs, n_users, n_items)
        poff = pitem = None
        if implicit is not None and len(implicit[0]):
            pu = np.ascontiguousarray(implicit[0], dtype=np.uint32)
            pi = np.ascontiguousarray(implicit[1], dtype=np.uint32)
            if int(pu.max()) >= n_users:
                raise ValueError("implicit user index out of range")
            poff, pitem, _ = _csr(pu, pi, np.zeros(len(pu), np.float32), n_users)
        bu = np.zeros(n_users) if bias_user is None else np.array(bias_user, dtype=np.float64)
        bi = np.zeros(n_items) if bias_item is None else np.array(bias_item, dtype=np.float64)
        if global_mean is None:
            mean = float(obs.astype(np.float64).sum() / len(obs)) if len(obs) else 0.0
        else:
            mean = float(global_mean)
        act = None if activate_user is None else np.ascontiguousarray(np.asarray(activate_user) != 0, dtype=np.uint8)
        nu = _mf_nupdates(nupdates, n_users, n_items)
        cap = (1 << 64) - 1 if max_updates is None else int(max_updates)
        max_supersteps = int(max_supersteps)
        rows = _mf_trace_rows(trace, max_updates, max_supersteps)
        tr = np.zeros((max(rows, 1), 2))
        vu, vi, vo = _mf_validate(validate)
        par = _native.SvdppParams(user_bias_step, user_bias_reg, item_bias_step, item_bias_reg, user_factor_step,
                                  user_factor_reg, item_factor_step, item_factor_reg, item_factor2_step,
                                  item_factor2_reg, float(step_dec), float(minval), float(maxval), mean, cap,
                                  max_supersteps)
        st = _native.SvdppStats()
        self._chk(self.lib.cf_svdpp_fit(self.h, n_users, n_items, int(D), ptr(uoff), ptr(uitem), ptr(uobs), ptr(ioff),
                                        ptr(iuser), ptr(iobs), ptr(poff), ptr(pitem), byref(par), ptr(U), ptr(V),
                                        ptr(W), ptr(Y), ptr(bu), ptr(bi), ptr(nu[0]), ptr(nu[1]), ptr(act),
                                        0 if vu is None else len(vu), ptr(vu), ptr(vi), ptr(vo),
                                        ptr(tr) if rows else None, rows, byref(st)), "cf_svdpp_fit")
        ms = [c_float(), c_float(), c_float()]
        self._chk(self.lib.cf_svdpp_timing(self.h, byref(ms[0]), byref(ms[1]), byref(ms[2])), "cf_svdpp_timing")
        done = min(rows, (int(st.supersteps) + 1) // 2)
        steps = np.array([st.user_bias_step, st.item_bias_step, st.user_factor_step, st.item_factor_step,
                          st.item_factor2_step], dtype=np.float32)
        return SvdppResult(U, V, W, Y, bu, bi, nu[0], nu[1], tr[:done].copy(), mean, int(st.supersteps),
                           int(st.updates), int(st.messages), int(st.n_nan), steps, float(st.reduce_ms),
                           float(st.apply_ms), float(ms[0].value), float(ms[1].value), float(ms[2].value))

    def svdpp_sum_sq_error(self, user, item, obs, U, V, bias_user, bias_item, global_mean=0.0, minval=-1e100,
                           maxval=1e100) -> float:
        """The reference's SVD++ error (extract_l2_error, svdpp.cpp:466-476) leaves Y out: it is
        cf_sgd_error with the biases."""
        return self.sgd_sum_sq_error(user, item, obs, U, V, bias_user, bias_item, global_mean, minval, maxval)

    def svdpp_rmse(self, user, item, obs, U, V, bias_user, bias_item, global_mean=0.0, minval=-1e100,
                   maxval=1e100) -> float:
        """RMSE of one role's edges (error_aggregator::finalize, svdpp.cpp:440-453)."""
        return self.sgd_rmse(user, item, obs, U, V, bias_user, bias_item, global_mean, minval, maxval)

    def svdpp_predict(self, user, item, U, V, Y, bias_user, bias_item, global_mean=0.0, minval=-1e100,
                      maxval=1e100) -> np.ndarray:
        """cf_svdpp_predict per (user, item) pair: clamp(mean + bu + bi + U_u . (V_i + Y_i)), always
        clamped (svdpp.cpp:490-493)."""
        user = np.ascontiguousarray(user, dtype=np.uint32)
        item = np.ascontiguousarray(item, dtype=np.uint32)
        U = np.ascontiguousarray(U, dtype=np.float64)
        V = np.ascontiguousarray(V, dtype=np.float64)
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        bu = np.ascontiguousarray(bias_user, dtype=np.float64)
        bi = np.ascontiguousarray(bias_item, dtype=np.float64)
        if Y.shape != V.shape:
            raise ValueError("Y and V differ in shape")
        pred = np.zeros(len(user), dtype=np.float64)
        self._chk(self.lib.cf_svdpp_predict(self.h, len(user), ptr(user), ptr(item), U.shape[0], V.shape[0],
                                            U.shape[1], ptr(U), ptr(V), ptr(Y), ptr(bu), ptr(bi), float(global_mean),
                                            float(minval), float(maxval), ptr(pred)), "cf_svdpp_predict")
        return pred

    # -- top-N recommendation from fitted factors (no reference counterpart) ----------
    def set_topn_block(self, users_per_block: int = 0):
        """cf_set_topn_block: users per block of mf_topn (0 = from its fixed byte budget)."""
        self._chk(self.lib.cf_set_topn_block(self.h, int(users_per_block)), "cf_set_topn_block")

    def mf_topn(self, U, V, N, *, bias_user=None, bias_item=None, mean=0.0, exclude=None, users=None) -> "TopnResult":
        """cf_mf_topn: for every user (or every user of `users`, in its order) the N best items by
        U_u . V_i + (bias_item[i] + (mean + bias_user[u])), absent biases skipped, among the items
        that are not in the user's exclusion list.  exclude: (user, item) index arrays of the pairs
        to leave out (any order, repeats allowed).  A NaN score is never listed."""
        n_users, head = _mf_source(U, V, bias_user, bias_item, mean)
        return self._topn("cf_mf_topn", n_users, head, _exclusion_csr(exclude, n_users), users, N)

    def mf_rank_eval(self, U, V, N, held, *, exclude=None, bias_user=None, bias_item=None,
                     mean=0.0) -> "RankEvalResult":
        """cf_mf_rank_eval: the exact rank of every held-out pair among its user's candidates (the
        scores, exclusions and order of mf_topn) and precision / recall / NDCG / AP / RR / AUC at
        cutoff N per user with their means and the expected percentile rank (cf_abi.h has the
        definitions).  held: (user, item[, weight]) arrays of the pairs to find, in any order; a
        repeated pair raises ValueError.  exclude: (user, item) arrays of the training pairs."""
        n_users, head = _mf_source(U, V, bias_user, bias_item, mean)
        return self._rank_eval("cf_mf_rank_eval", n_users, head, _exclusion_csr(exclude, n_users), held, N)

    def _topn(self, name, n_users, head, excl, users, N) -> "TopnResult":
        """The call of a cf_*_topn entry point: `head` = its arguments up to the exclusion CSR
        `excl` (arrays, kept alive here), then the selection, N and the output buffers."""
        N = int(N)
        sel = None if users is None else np.ascontiguousarray(users, dtype=np.uint32)
        n_out = n_users if sel is None else len(sel)
        if sel is not None and not len(sel):
            sel = np.zeros(1, np.uint32)
        items = np.full((n_out, max(N, 0)), 0xFFFFFFFF, dtype=np.uint32)
        scores = np.zeros((n_out, max(N, 0)), dtype=np.float64)
        count = np.zeros(n_out, dtype=np.uint32)
        st = _native.TopnStats()
        args = [ptr(a) if isinstance(a, np.ndarray) else a for a in head]
        self._chk(getattr(self.lib, name)(self.h, n_users, *args, ptr(excl[0]), ptr(excl[1]),
                                          n_out if sel is not None else 0, ptr(sel), N, ptr(items), ptr(scores),
                                          ptr(count), byref(st)), name)
        return TopnResult(items, scores, count, st)

    def _rank_eval(self, name, n_users, head, excl, held, N) -> "RankEvalResult":
        """The call of a cf_*_rank_eval entry point: `head` and `excl` as in _topn, then the
        held-out CSR of `held` (user, item, weight or None), N and the output buffers."""
        su, perm, hoff, hitem, hws = _held_csr(held, n_users)
        rank = np.zeros(max(len(su), 1), dtype=np.uint32)
        users = np.zeros(max(n_users, 1), dtype=RANK_USER_DTYPE)
        st = _native.RankSummary()
        args = [ptr(a) if isinstance(a, np.ndarray) else a for a in head]
        self._chk(getattr(self.lib, name)(self.h, n_users, *args, ptr(excl[0]), ptr(excl[1]), ptr(hoff), ptr(hitem),
                                          ptr(hws), int(N), ptr(rank), ptr(users), byref(st)), name)
        return _rank_result(su, perm, rank, users[:n_users], st)

    # -- top-N and ranking evaluation from the item graph (no reference counterpart) ----
    def _knn_profile(self, user_off, items, ratings, mode, exclude):
        """The arguments cf_knn_topn and cf_knn_rank_eval share."""
        off = np.ascontiguousarray(user_off, dtype=np.uint64)
        it = np.ascontiguousarray(items, dtype=np.uint32)
        rat = np.ascontiguousarray(ratings, dtype=np.float32)
        if len(off) < 1 or len(it) != len(rat) or (len(off) and int(off[-1]) != len(it)):
            raise ValueError("user_off / items / ratings do not describe one profile CSR")
        if mode not in _KNN_SCORE_MODES:
            raise ValueError("mode must be 'sum' or 'mean'")
        n_users = len(off) - 1
        if isinstance(exclude, str):
            if exclude != "profile":
                raise ValueError("exclude must be 'profile', None or (user, item) arrays")
            eoff, eitem = off, (it if len(it) else np.zeros(1, np.uint32))
        else:
            eoff, eitem = _exclusion_csr(exclude, n_users)
        if not len(it):   # valid pointers for an empty profile
            it, rat = np.zeros(1, np.uint32), np.zeros(1, np.float32)
        return n_users, off, it, rat, _KNN_SCORE_MODES[mode], eoff, eitem

    def knn_topn(self, user_off, items, ratings, N, *, mode="sum", w_min=0.1, exclude="profile",
                 users=None) -> "TopnResult":
        """cf_knn_topn: for every user (or every user of `users`, in its order) the N best items of
        the uploaded graph by the item-kNN score of the user's profile (user_off / items / ratings,
        a CSR in the order the sums run): mode "sum" = sum of w(m, i) r over the profile entries with
        w(m, i) > w_min, "mean" = that over the sum of those w (knn_predict's prediction, 0 without a
        neighbour).  exclude: "profile" (the user's own items), None, or (user, item) arrays."""
        n_users, off, it, rat, smode, eoff, eitem = self._knn_profile(user_off, items, ratings, mode, exclude)
        return self._topn("cf_knn_topn", n_users, (off, it, rat, smode, float(w_min)), (eoff, eitem), users, N)

    def knn_rank_eval(self, user_off, items, ratings, N, held, *, mode="sum", w_min=0.1, exclude="profile",
                      weights=None) -> "RankEvalResult":
        """cf_knn_rank_eval: mf_rank_eval with the scores of knn_topn.  held: (user, item) arrays of
        the pairs to find, in any order; weights: one per held pair (mpr only)."""
        n_users, off, it, rat, smode, eoff, eitem = self._knn_profile(user_off, items, ratings, mode, exclude)
        return self._rank_eval("cf_knn_rank_eval", n_users, (off, it, rat, smode, float(w_min)), (eoff, eitem),
                               (held[0], held[1], weights), N)

    # -- EASE: the closed-form item-item model (no reference counterpart) --------------
    @staticmethod
    def _ease_train(user_off, items, ratings):
        """The TRAIN edges of a fit as (n_users, off, items, ratings)."""
        off = np.ascontiguousarray(user_off, dtype=np.uint64)
        it = np.ascontiguousarray(items, dtype=np.uint32)
        rat = np.ascontiguousarray(ratings, dtype=np.float32)
        if len(off) < 1 or len(it) != len(rat) or int(off[-1]) != len(it):
            raise ValueError("user_off / items / ratings do not describe one TRAIN CSR")
        if not len(it):   # valid pointers for an empty edge list
            it, rat = np.zeros(1, np.uint32), np.zeros(1, np.float32)
        return len(off) - 1, off, it, rat

    def ease_fit(self, user_off, items, ratings, n_items, lam, *, binary=False) -> np.ndarray:
        """cf_ease_fit: G = X^T X + lam I, P = G^-1, B = -P / diag(P) with a zero diagonal, from
        the TRAIN edges as a CSR by user (item lists strictly ascending; the value of an edge is 1
        when `binary`, else its rating).  B stays resident in the context for ease_topn /
        ease_rank_eval / ease_weights.  Returns ease_timing()."""
        n_users, off, it, rat = self._ease_train(user_off, items, ratings)
        self._chk(self.lib.cf_ease_fit(self.h, n_users, int(n_items), ptr(off), ptr(it), ptr(rat), int(bool(binary)),
                                       float(lam)), "cf_ease_fit")
        return self.ease_timing()

    def ease_gram(self, user_off, items, ratings, n_items, lam, *, binary=False) -> np.ndarray:
        """cf_ease_gram: the fit's Gram stage alone, G [n_items, n_items] in float64."""
        n_users, off, it, rat = self._ease_train(user_off, items, ratings)
        G = np.zeros((int(n_items), int(n_items)), dtype=np.float64)
        self._chk(self.lib.cf_ease_gram(self.h, n_users, int(n_items), ptr(off), ptr(it), ptr(rat), int(bool(binary)),
                                        float(lam), ptr(G) if G.size else None), "cf_ease_gram")
        return G

    def ease_inverse(self, user_off, items, ratings, n_items, lam, *, binary=False) -> np.ndarray:
        """cf_debug_ease_inverse: P = G^-1 as the fit computes it, before the normalisation (the
        resident B is left as it is)."""
        n_users, off, it, rat = self._ease_train(user_off, items, ratings)
        P = np.zeros((int(n_items), int(n_items)), dtype=np.float64)
        self._chk(self.lib.cf_debug_ease_inverse(self.h, n_users, int(n_items), ptr(off), ptr(it), ptr(rat),
                                                 int(bool(binary)), float(lam), ptr(P) if P.size else None),
                  "cf_debug_ease_inverse")
        return P

    def ease_weights(self) -> np.ndarray:
        """cf_ease_weights: the resident B [n_items, n_items] in float64."""
        n = c_uint32(0)
        self._chk(self.lib.cf_ease_weights(self.h, byref(n), None), "cf_ease_weights")
        B = np.zeros((int(n.value), int(n.value)), dtype=np.float64)
        self._chk(self.lib.cf_ease_weights(self.h, byref(n), ptr(B)), "cf_ease_weights")
        return B

    def ease_upload(self, B):
        """cf_ease_upload: any square float64 B (signed, NaN allowed) as the resident weights."""
        B = np.ascontiguousarray(B, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != B.shape[1]:
            raise ValueError("B must be n_items x n_items")
        self._chk(self.lib.cf_ease_upload(self.h, B.shape[0], ptr(B) if B.size else None), "cf_ease_upload")

    def ease_timing(self) -> np.ndarray:
        """cf_ease_timing: device ms of the last ease_fit: Gram, inversion, normalisation."""
        ms = np.zeros(3, dtype=np.float32)
        self._chk(self.lib.cf_ease_timing(self.h, ptr(ms)), "cf_ease_timing")
        return ms

    def _ease_profile(self, user_off, items, ratings, exclude):
        """The arguments cf_ease_topn and cf_ease_rank_eval share: those of the graph source but its mode."""
        n_users, off, it, rat, _, eoff, eitem = self._knn_profile(user_off, items, ratings, "sum", exclude)
        return n_users, off, it, rat, eoff, eitem

    def ease_topn(self, user_off, items, ratings, N, *, binary=False, exclude="profile", users=None) -> "TopnResult":
        """cf_ease_topn: for every user (or every user of `users`, in its order) the N best items by
        s(u, j) = sum_t x_t B[i_t][j] over the user's profile (user_off / items / ratings, in the
        order the sum runs; x = 1 when `binary`, else the rating) with the resident B.  The profile
        need not be the fit's: any user can be scored.  exclude: "profile" (the user's own items),
        None, or (user, item) arrays."""
        n_users, off, it, rat, eoff, eitem = self._ease_profile(user_off, items, ratings, exclude)
        return self._topn("cf_ease_topn", n_users, (off, it, rat, int(bool(binary))), (eoff, eitem), users, N)

    def ease_rank_eval(self, user_off, items, ratings, N, held, *, binary=False, exclude="profile",
                       weights=None) -> "RankEvalResult":
        """cf_ease_rank_eval: mf_rank_eval with the scores of ease_topn.  held: (user, item) arrays of
        the pairs to find, in any order; weights: one per held pair (mpr only)."""
        n_users, off, it, rat, eoff, eitem = self._ease_profile(user_off, items, ratings, exclude)
        return self._rank_eval("cf_ease_rank_eval", n_users, (off, it, rat, int(bool(binary))), (eoff, eitem),
                               (held[0], held[1], weights), N)

    # -- truncated SVD by restarted Lanczos (svd.cpp:304-505) ------------------------
    @staticmethod
    def svd_entries(row, col, val, rows, cols, regularization=0.0):
        """The entries cf_svd_fit sees.  A square matrix keeps its diagonal apart in the reference
        (A_ii, the last line of a vertex wins, svd.cpp:276-280) and adds --regularization to it
        (math.hpp:137-138): here entry (i, i) = (float)(A_ii + regularization) wherever that is not
        0.  For a non-square matrix the regularization is ignored, as there."""
        row = np.ascontiguousarray(row, dtype=np.uint32)
        col = np.ascontiguousarray(col, dtype=np.uint32)
        val = np.ascontiguousarray(val, dtype=np.float32)
        if int(rows) != int(cols):
            return row, col, val
        diag = np.zeros(int(rows), dtype=np.float64)
        on = row == col
        diag[row[on]] = val[on]   # the last one wins
        diag += float(regularization)
        keep = np.flatnonzero(diag != 0.0).astype(np.uint32)
        return (np.concatenate([row[~on], keep]), np.concatenate([col[~on], keep]),
                np.concatenate([val[~on], diag[keep].astype(np.float32)]))

    def svd_fit(self, row, col, val, rows, cols, nsv, nv, max_iter=10, tol=1e-8, ortho_repeats=3, v0=None,
                regularization=0.0, seed=0) -> "SvdResult":
        """cf_svd_fit: the leading nsv singular triplets of the rows x cols matrix with entries
        (row[e], col[e], val[e]) from nv Lanczos vectors per restart.  v0 (rows entries) is the
        start vector; None draws it uniform in [0, 1) from `seed` (the reference: randu)."""
        rows, cols, nsv, nv = int(rows), int(cols), int(nsv), int(nv)
        row, col, val = self.svd_entries(row, col, val, rows, cols, regularization)
        if len(row) and (int(row.max()) >= rows or int(col.max()) >= cols):
            raise ValueError("entry index out of range")
        roff, rcol, rval = _csr(row, col, val, rows)
        coff, crow, cval = _csr(col, row, val, cols)
        v0 = np.random.default_rng(seed).random(rows) if v0 is None else np.ascontiguousarray(v0, dtype=np.float64)
        if v0.size != rows:
            raise ValueError("v0 does not hold `rows` values")
        sigma, errest = np.full(max(nv, 1), np.nan), np.full(max(nv, 1), np.nan)
        err = np.full(max(nsv, 1), np.nan)
        U = np.zeros((max(nsv, 1), rows), dtype=np.float64)   # column-major rows x nsv
        V = np.zeros((max(nsv, 1), cols), dtype=np.float64)
        kk = np.zeros(max(int(max_iter), 1), dtype=np.uint32)
        ab = np.full(2 * max(nv, 1), np.nan)
        st = _native.SvdStats()
        self._chk(self.lib.cf_svd_fit(self.h, rows, cols, ptr(roff), ptr(rcol), ptr(rval), ptr(coff), ptr(crow),
                                      ptr(cval), nsv, nv, int(max_iter), float(tol), int(ortho_repeats), ptr(v0),
                                      ptr(sigma), ptr(errest), ptr(err), ptr(U), ptr(V), ptr(kk), ptr(ab), byref(st)),
                  "cf_svd_fit")
        return SvdResult(sigma[:nv], errest[:nv], err[:nsv], U[:nsv].T, V[:nsv].T, kk[:int(st.passes)].copy(),
                         ab[:nv].copy(), ab[max(nv, 1):max(nv, 1) + nv].copy(), int(st.nconv), int(st.passes),
                         int(st.products), float(st.matvec_ms), float(st.ortho_ms), float(st.rotate_ms))

    def svd_matvec(self, off, nbr, val, n_out, n_in, x) -> np.ndarray:
        """cf_svd_matvec: y = M x for the CSR (off, nbr, val) with n_out rows and n_in columns."""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        nbr = np.ascontiguousarray(nbr, dtype=np.uint32)
        val = np.ascontiguousarray(val, dtype=np.float32)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if len(off) != int(n_out) + 1 or x.size != int(n_in):
            raise ValueError("off / x do not match n_out / n_in")
        y = np.zeros(int(n_out), dtype=np.float64)
        self._chk(self.lib.cf_svd_matvec(self.h, int(n_out), int(n_in), ptr(off), ptr(nbr), ptr(val), ptr(x), ptr(y)),
                  "cf_svd_matvec")
        return y

    # -- device-resident paths (torch CUDA tensors) -------------------------------
    def plan(self, item_off_host) -> "Plan":
        return Plan(self, item_off_host)

    def pack_eigen_run(self, n_users, d_item_off, d_m, d_evec_off, d_evecs, d_packed_off, d_packed=None,
                       stream=None):
        """cf_pack_eigen_run: packed offsets (and, with d_packed, the packed k x m blocks)
        of the eigen output for the out_eigen_ gather."""
        self._chk(self.lib.cf_pack_eigen_run(self.h, int(n_users), ptr(d_item_off), ptr(d_m), ptr(d_evec_off),
                                             ptr(d_evecs), ptr(d_packed_off), ptr(d_packed), c_void_p(stream or 0)),
                  "cf_pack_eigen_run")


def cost_split_native(item_off, n_parts: int) -> np.ndarray:
    """cf_cost_split: n_parts + 1 contiguous split points balancing sum(k^3)."""
    item_off = np.ascontiguousarray(item_off, dtype=np.uint64)
    split = np.zeros(n_parts + 1, dtype=np.uint32)
    rc = _native.load().cf_cost_split(len(item_off) - 1, ptr(item_off), int(n_parts), ptr(split))
    if rc != _native.CF_OK:
        raise NativeError(f"cf_cost_split failed ({rc})")
    return split.astype(np.int64)


def eigen_batch_multi(ctxs, item_off, items):
    """cf_eigen_batch_multi over contexts `ctxs` (each with the graph uploaded): returns
    (EigenResult with packed evecs: evec_off = packed offsets, split points)."""
    lib = _native.load()
    item_off = np.ascontiguousarray(item_off, dtype=np.uint64)
    items = np.ascontiguousarray(items, dtype=np.uint32)
    n_users = len(item_off) - 1
    _, cap = evec_offsets(item_off)
    n = int(item_off[-1])
    m = np.zeros(n_users, dtype=np.int32)
    sigs = np.zeros(n, dtype=np.float32)
    evals = np.zeros(n, dtype=np.float32)
    poff = np.zeros(n_users + 1, dtype=np.uint64)
    evecs = np.zeros(max(cap, 1), dtype=np.float32)
    split = np.zeros(len(ctxs) + 1, dtype=np.uint32)
    arr = (c_void_p * len(ctxs))(*[c.h for c in ctxs])
    rc = lib.cf_eigen_batch_multi(arr, len(ctxs), n_users, ptr(item_off), ptr(items), ptr(m), ptr(sigs), ptr(evals),
                                  ptr(poff), ptr(evecs), cap, ptr(split))
    _check(lib, ctxs[0].h, rc, "cf_eigen_batch_multi")
    return EigenResult(item_off, poff[:-1].copy(), m, sigs, evals, evecs[: int(poff[-1])]), split.astype(np.int64)


def eigen_batch_stream(ctxs, item_off, items, on_chunk, chunk_bytes=0):
    """cf_eigen_batch_stream: compute_eigens over users 0..n-1 in memory-bounded chunks
    (precompute_local_threads.cpp:89-98, 306-314: one task per user, each record appended as it
    completes).  on_chunk(first, m, sigs, evals, packed_off, evecs) receives numpy COPIES of each
    chunk's arrays in user order (item_off chunk-local); a returned nonzero int stops the call.
    Returns the stream stats as a dict."""
    lib = _native.load()
    if isinstance(ctxs, Context):
        ctxs = [ctxs]
    item_off = np.ascontiguousarray(item_off, dtype=np.uint64)
    items = np.ascontiguousarray(items, dtype=np.uint32)
    n_users = len(item_off) - 1
    err = []

    def sink(_user, cp):
        c = cp.contents
        try:
            n = int(c.count)
            off = np.ctypeslib.as_array(c.item_off, shape=(n + 1,)).copy()
            po = np.ctypeslib.as_array(c.packed_off, shape=(n + 1,)).copy()
            ne, npk = int(off[-1]), int(po[-1])
            m = np.ctypeslib.as_array(c.m, shape=(n,)).copy() if n else np.zeros(0, np.int32)
            sg = np.ctypeslib.as_array(c.sigs, shape=(ne,)).copy() if ne else np.zeros(0, np.float32)
            ev = np.ctypeslib.as_array(c.evals, shape=(ne,)).copy() if ne else np.zeros(0, np.float32)
            vv = np.ctypeslib.as_array(c.evecs, shape=(npk,)).copy() if npk else np.zeros(0, np.float32)
            r = on_chunk(int(c.first), off, m, sg, ev, po, vv)
            return int(r or 0)
        except Exception as e:   # noqa: BLE001 -- reported after the call
            err.append(e)
            return 1

    cb = _native.EIGEN_SINK(sink)
    st = _native.EigenStreamStats()
    arr = (c_void_p * len(ctxs))(*[c.h for c in ctxs])
    rc = lib.cf_eigen_batch_stream(arr, len(ctxs), n_users, ptr(item_off), ptr(items), int(chunk_bytes), cb, None,
                                   byref(st))
    if err:
        raise err[0]
    _check(lib, ctxs[0].h, rc, "cf_eigen_batch_stream")
    return {"chunks": st.chunks, "chunk_slot_bytes": st.chunk_slot_bytes,
            "max_chunk_slot_bytes": st.max_chunk_slot_bytes, "own_peak_bytes": st.own_peak_bytes,
            "device_peak_bytes": st.device_peak_bytes}


def eigen_stream_result(ctxs, item_off, items, chunk_bytes=0):
    """eigen_batch_stream gathered into one EigenResult with packed evecs (evec_off = packed
    offsets, as eigen_batch_multi returns), plus the stats."""
    item_off = np.ascontiguousarray(item_off, dtype=np.uint64)
    n_users = len(item_off) - 1
    n = int(item_off[-1])
    m = np.zeros(n_users, dtype=np.int32)
    sigs = np.zeros(n, dtype=np.float32)
    evals = np.zeros(n, dtype=np.float32)
    poff = np.zeros(n_users + 1, dtype=np.uint64)
    parts = []
    run = [0]

    def on_chunk(first, off, mm, sg, ev, po, vv):
        cnt = len(mm)
        e0 = int(item_off[first])
        m[first:first + cnt] = mm
        sigs[e0:e0 + len(sg)] = sg
        evals[e0:e0 + len(ev)] = ev
        poff[first:first + cnt + 1] = po + run[0]
        run[0] += int(po[-1])
        parts.append(vv)
        return 0

    st = eigen_batch_stream(ctxs, item_off, items, on_chunk, chunk_bytes)
    evecs = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    return EigenResult(item_off, poff[:-1].copy(), m, sigs, evals, evecs), st


def predict_precomp_multi(ctxs, item_off, items, ratings, m, evals, evec_off, evecs, sigtab,
                          sig_mode=CF_SIGS_COMPAT, row_sel=None, want_pred=False):
    """cf_predict_precomp_multi: neigh_program::apply over one user set on contexts `ctxs`
    (each with the graph uploaded; users range-split by k^3, the global compat table on every
    context).  Host numpy arrays as Context.predict_precomp; returns (mse, kk[, pred], split)."""
    lib = _native.load()
    item_off = np.ascontiguousarray(item_off, dtype=np.uint64)
    items = np.ascontiguousarray(items, dtype=np.uint32)
    ratings = np.ascontiguousarray(ratings, dtype=np.float32)
    m = np.ascontiguousarray(m, dtype=np.int32)
    evals = np.ascontiguousarray(evals, dtype=np.float64)
    evec_off = np.ascontiguousarray(evec_off, dtype=np.uint64)
    f32 = np.asarray(evecs).dtype == np.float32   # binary out_eigen_ blocks: the _f32 entry point
    evecs = np.ascontiguousarray(evecs, dtype=np.float32 if f32 else np.float64)
    sigtab = np.ascontiguousarray(sigtab, dtype=np.float64)
    sel = None if row_sel is None else np.ascontiguousarray(row_sel, dtype=np.uint8)
    n_users = len(item_off) - 1
    n = int(item_off[-1])
    mse = np.zeros(n, dtype=np.float32)
    kk = np.zeros(n, dtype=np.int32)
    pred = np.zeros(n, dtype=np.float64) if want_pred else None
    split = np.zeros(len(ctxs) + 1, dtype=np.uint32)
    arr = (c_void_p * len(ctxs))(*[c.h for c in ctxs])
    fn = lib.cf_predict_precomp_multi_f32 if f32 else lib.cf_predict_precomp_multi
    rc = fn(arr, len(ctxs), n_users, ptr(item_off), ptr(items), ptr(ratings), ptr(m), ptr(evals), ptr(evec_off),
            ptr(evecs), ptr(sigtab), len(sigtab), int(sig_mode), ptr(sel), ptr(mse), ptr(kk), ptr(pred), ptr(split))
    _check(lib, ctxs[0].h, rc, "cf_predict_precomp_multi" + ("_f32" if f32 else ""))
    out = (mse, kk, pred) if want_pred else (mse, kk)
    return out + (split.astype(np.int64),)


class Plan:
    """cf_plan: users bucketed by item count, reusable across eigen/predict runs."""

    def __init__(self, ctx: Context, item_off_host):
        self.ctx = ctx
        item_off_host = np.ascontiguousarray(item_off_host, dtype=np.uint64)
        h = c_void_p()
        ctx._chk(ctx.lib.cf_plan_create(ctx.h, len(item_off_host) - 1, ptr(item_off_host), byref(h)),
                 "cf_plan_create")
        self.h = h

    def close(self):
        if self.h:
            self.ctx.lib.cf_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def eigen_run(self, d_item_off, d_items, d_evec_off, d_m, d_sigs, d_evals, d_evecs, stream=None):
        c = self.ctx
        c._chk(c.lib.cf_eigen_run(c.h, self.h, ptr(d_item_off), ptr(d_items), ptr(d_evec_off), ptr(d_m),
                                  ptr(d_sigs), ptr(d_evals), ptr(d_evecs), c_void_p(stream or 0)),
               "cf_eigen_run")

    def step_run(self, d_item_off, d_items, d_ratings, d_evec_off, d_m, d_sigs, d_evals, d_evecs, sig_mode,
                 d_mse, d_kk, d_pred=None, stream=None):
        """cf_step_run: eigen + predictor (fp32 eigen outputs, sigtab = d_sigs) with per-bucket overlap."""
        c = self.ctx
        c._chk(c.lib.cf_step_run(c.h, self.h, ptr(d_item_off), ptr(d_items), ptr(d_ratings), ptr(d_evec_off),
                                 ptr(d_m), ptr(d_sigs), ptr(d_evals), ptr(d_evecs), int(sig_mode), ptr(d_mse),
                                 ptr(d_kk), ptr(d_pred), c_void_p(stream or 0)), "cf_step_run")

    def step_timing(self):
        """(eigen_ms, total_ms) of the last cf_step_run (waits for it)."""
        a, b = c_float(), c_float()
        self.ctx._chk(self.ctx.lib.cf_step_timing(self.ctx.h, byref(a), byref(b)), "cf_step_timing")
        return a.value, b.value

    def predict_run(self, d_item_off, d_items, d_ratings, d_m, d_evals, d_evec_off, d_evecs, d_sigtab,
                    sig_mode, d_mse, d_kk, d_pred=None, stream=None, fp64=False):
        c = self.ctx
        fn = c.lib.cf_predict_run_f64 if fp64 else c.lib.cf_predict_run_f32
        c._chk(fn(c.h, self.h, ptr(d_item_off), ptr(d_items), ptr(d_ratings), ptr(d_m), ptr(d_evals),
                  ptr(d_evec_off), ptr(d_evecs), ptr(d_sigtab), int(sig_mode), ptr(d_mse), ptr(d_kk),
                  ptr(d_pred), c_void_p(stream or 0)), "cf_predict_run")


__all__ = ["Context", "Plan", "EigenResult", "AlsResult", "SgdResult", "NmfResult", "BprResult", "evec_offsets", "cost_split_native", "eigen_batch_multi",
           "predict_precomp_multi", "CF_SIGS_OWN", "CF_SIGS_COMPAT", "CF_FILTER_CHEBY",
           "CF_FILTER_BINOMIAL"]
