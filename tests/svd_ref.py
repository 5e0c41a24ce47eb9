"""Checker for cf_svd_fit: a plain numpy fp64 restatement of the restarted Golub-Kahan-Lanczos
pass structure that include/cf_abi.h states (P[i] row side, Q[i] column side, classical
Gram-Schmidt with all coefficients from the same vector, the 1e-10 rule, the bidiagonal T of a
pass, errest from beta[m - 1], Ritz rotation, restart without a coupling term, residual errors).
Not a port: written from that description; np.linalg.svd stands in for the host Jacobi.  Also
holds the matrices the SVD tests share."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import als_ref as ar

NORM_FLOOR = 1e-10

# What test_gpu_svd.py holds the device to: relative to |alpha| and |beta| of the first pass, to
# sigma_1 for the converged sigma, absolute for max|U^T U - I| and max|V^T V - I|.
# test_svd_ref.py::test_drift_sets_the_device_bounds measures the checker against itself and
# requires each bound to leave a margin of at least MARGIN over the drift it sees.
BOUND_ALPHA_BETA = 1e-12
BOUND_SIGMA = 2e-13
BOUND_ORTH = 1e-12
MARGIN = 200


@dataclass
class RefResult:
    sigma: np.ndarray           # nv entries, NaN where no pass reached
    errest: np.ndarray
    err: np.ndarray             # min(nsv, nconv) entries
    resid: np.ndarray           # sqrt(n1^2 + n2^2) of the same triplets, not divided
    U: np.ndarray               # rows x min(nsv, nconv)
    V: np.ndarray
    nconv: int = 0
    passes: int = 0
    products: int = 0
    kk_pass: list = field(default_factory=list)
    alpha_first: np.ndarray | None = None
    beta_first: np.ndarray | None = None
    margin: float = np.inf      # smallest |errest - tol| / tol any pass saw


class Matrix:
    """A x and A^T x as sums over the entries in their given order (bincount adds in that order,
    so a permutation of the entries is another summation order)."""

    def __init__(self, row, col, val, rows, cols, perm=None):
        row = np.asarray(row, dtype=np.int64)
        col = np.asarray(col, dtype=np.int64)
        val = np.asarray(val, dtype=np.float32).astype(np.float64)   # values pass through float
        if perm is not None:
            row, col, val = row[perm], col[perm], val[perm]
        self.row, self.col, self.val, self.rows, self.cols = row, col, val, int(rows), int(cols)

    def mul(self, x):     # A x
        return np.bincount(self.row, weights=self.val * x[self.col], minlength=self.rows)

    def tmul(self, x):    # A^T x
        return np.bincount(self.col, weights=self.val * x[self.row], minlength=self.cols)

    def dense(self):
        D = np.zeros((self.rows, self.cols))
        np.add.at(D, (self.row, self.col), self.val)
        return D


def add_diagonal(row, col, val, n, regularization):
    """The entries of a square matrix as cf_svd_fit sees them: entry (i, i) = (float)(A_ii +
    regularization) wherever that is not 0 (the last diagonal line of a vertex wins)."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    val = np.asarray(val, dtype=np.float32)
    diag = np.zeros(n)
    on = row == col
    diag[row[on]] = val[on]
    diag += regularization
    keep = np.flatnonzero(diag != 0.0)
    return (np.concatenate([row[~on], keep]), np.concatenate([col[~on], keep]),
            np.concatenate([val[~on], diag[keep].astype(np.float32)]))


def orthonormalise(X, i, repeats):
    """Vector i of X (columns) against the i columns before it; returns the norm."""
    w = X[:, i]
    if i:
        B = X[:, :i]
        for _ in range(repeats):
            c = B.T @ w          # all coefficients from the same w
            w -= B @ c
    nrm = float(np.sqrt(w @ w))
    if nrm >= NORM_FLOOR:
        w /= nrm
    return nrm


def fit(row, col, val, rows, cols, nsv, nv, max_iter=10, tol=1e-8, ortho_repeats=3, v0=None, perm=None) -> RefResult:
    A = Matrix(row, col, val, rows, cols, perm)
    P = np.zeros((rows, nv + 1))
    Q = np.zeros((cols, nv + 1))
    v0 = np.asarray(v0, dtype=np.float64)
    P[:, 0] = v0 / np.sqrt(v0 @ v0)
    sigma, errest = np.full(nv, np.nan), np.full(nv, np.nan)
    out = RefResult(sigma, errest, np.zeros(0), np.zeros(0), np.zeros((rows, 0)), np.zeros((cols, 0)))
    nconv, its = 0, 1
    while nconv < nsv and its < max_iter:
        k, n = nconv, nv
        alpha, beta = np.zeros(n), np.zeros(n)
        Q[:, k] = A.tmul(P[:, k])
        alpha[0] = orthonormalise(Q, k, ortho_repeats)
        for i in range(k + 1, n):
            P[:, i] = A.mul(Q[:, i - 1])
            beta[i - k - 1] = orthonormalise(P, i, ortho_repeats)
            Q[:, i] = A.tmul(P[:, i])
            alpha[i - k] = orthonormalise(Q, i, ortho_repeats)
        P[:, n] = A.mul(Q[:, n - 1])
        beta[n - k - 1] = orthonormalise(P, n, ortho_repeats)
        out.products += 2 * (n - k)
        if out.passes == 0:
            out.alpha_first, out.beta_first = alpha.copy(), beta.copy()
        m = nv - nconv
        T = np.diag(alpha[:m]) + np.diag(beta[:m - 1], 1)
        a, b, PTt = np.linalg.svd(T)       # T = a diag(b) PT^T
        PT = PTt.T
        kk = 0
        for j in range(m):
            sigma[nconv + j] = b[j]
            e = abs(a[m - 1, j] * beta[m - 1])
            if b[j] > tol:
                e /= b[j]
            errest[nconv + j] = e
            out.margin = min(out.margin, abs(e - tol) / tol)
            kk += e < tol
        finished = nconv + kk >= nsv
        out.kk_pass.append(int(kk))
        start = None if finished else P[:, nconv:nconv + m] @ PT[:, kk]
        if kk:
            P[:, nconv:nconv + kk] = P[:, nconv:nconv + m] @ PT[:, :kk]
            Q[:, nconv:nconv + kk] = Q[:, nconv:nconv + m] @ a[:, :kk]
        nconv += kk
        out.passes += 1
        if finished:
            break
        P[:, nconv] = start
        its += 1
    out.nconv = nconv
    n_out = min(nsv, nconv)
    out.U, out.V = P[:, :n_out].copy(), Q[:, :n_out].copy()
    out.resid, out.err = residuals(A, out.U, out.V, sigma[:n_out], tol)
    out.products += 2 * n_out
    return out


def residuals(A, U, V, sigma, tol):
    """(sqrt(n1^2 + n2^2), the same divided by sigma_i when sigma_i > tol) per triplet, with
    n1 = |A^T u_i - sigma_i v_i| and n2 = |A v_i - sigma_i u_i|."""
    n = len(sigma)
    resid, err = np.zeros(n), np.zeros(n)
    for i in range(n):
        r1 = A.tmul(U[:, i]) - sigma[i] * V[:, i]
        r2 = A.mul(V[:, i]) - sigma[i] * U[:, i]
        resid[i] = np.sqrt(r1 @ r1 + r2 @ r2)
        err[i] = resid[i] / sigma[i] if sigma[i] > tol else resid[i]
    return resid, err


def truth_bound(resid, sigma_max):
    """|sigma_i - sigma_i(dense)| <= this.  z = (u; v) / sqrt(2) is a unit vector for the symmetric
    H = [[0, A], [A^T, 0]], whose eigenvalues are +-sigma_j(A) and zeros, and |H z - sigma z| =
    sqrt(n1^2 + n2^2) / sqrt(2): an exact eigenvalue lies within that of sigma.  The factor sqrt(2)
    that is not taken covers |z| != 1 (the vectors' norms are within 1e-12 of 1); 64 eps sigma_1 is
    for the roundoff of the dense LAPACK values and of the residual's own evaluation."""
    return resid + 64 * np.finfo(np.float64).eps * sigma_max


# ---- the shared matrices ---------------------------------------------------------------------

CASES = {
    # name: (rows, cols, min raters per item, nsv, nv, max_iter, tol, regularization)
    "A": (96, 40, 0, 4, 12, 40, 1e-8, 0.0),
    "C": (200, 12, 60, 3, 8, 40, 1e-8, 0.0),
    "S": (40, 40, 0, 3, 10, 40, 1e-8, 0.5),    # square, with diagonal entries
}


def case_inputs(name):
    """(row, col, val, rows, cols, v0, spec) with the diagonal of the square case already folded in."""
    rows, cols, minr, nsv, nv, max_iter, tol, reg = CASES[name]
    g = ar.make_graph(rows, cols, seed=7, min_raters=minr)
    row, col, val = g.user.astype(np.int64), g.item.astype(np.int64), g.obs
    if rows == cols:
        off, d = row != col, np.arange(3, rows, 3)   # the graph's own diagonal entries give way to these
        row, col = np.concatenate([row[off], d]), np.concatenate([col[off], d])
        val = np.concatenate([val[off], (1 + d % 5).astype(np.float32)])
    v0 = np.random.default_rng(5).random(rows)
    return row, col, val, rows, cols, v0, dict(nsv=nsv, nv=nv, max_iter=max_iter, tol=tol, regularization=reg)


def case_entries(name):
    """The entries the solver sees (the square case's regularised diagonal folded in)."""
    row, col, val, rows, cols, v0, spec = case_inputs(name)
    if rows == cols:
        row, col, val = add_diagonal(row, col, val, rows, spec["regularization"])
    return row, col, val


_REF_CACHE = {}


def case_reference(name, ortho_repeats=3) -> RefResult:
    """The checker's run of a case, computed once and shared (callers must not modify it)."""
    key = (name, ortho_repeats)
    if key not in _REF_CACHE:
        _, _, _, rows, cols, v0, spec = case_inputs(name)
        row, col, val = case_entries(name)
        _REF_CACHE[key] = fit(row, col, val, rows, cols, spec["nsv"], spec["nv"], spec["max_iter"], spec["tol"],
                              ortho_repeats, v0)
    return _REF_CACHE[key]


def dense_sigma(name):
    row, col, val = case_entries(name)
    rows, cols = CASES[name][0], CASES[name][1]
    return np.linalg.svd(Matrix(row, col, val, rows, cols).dense(), compute_uv=False)
