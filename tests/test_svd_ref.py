"""CPU self-tests of the SVD checker (tests/svd_ref.py), the drift measurement that sets the
device bounds of test_gpu_svd.py, and the host Jacobi of csrc/cf_small_svd.hpp through
cf_debug_small_svd (a pure host entry point: no GPU needed)."""
import numpy as np
import pytest

import svd_ref as sr
from collaborative_filtering_amd import _native
from collaborative_filtering_amd._native import ptr

from svd_ref import BOUND_ALPHA_BETA, BOUND_ORTH, BOUND_SIGMA, MARGIN


def test_hand_worked_3x4():
    """nsv = nv = 3 on a 3 x 4 matrix of rank 3: P[0..3) spans the whole row space, so the last
    beta vanishes, one pass converges everything and the values of T are those of A."""
    A = np.array([[2.0, 0.0, 1.0, 0.0], [0.0, 3.0, 0.0, 1.0], [1.0, 0.0, 0.0, 4.0]])
    row, col = np.nonzero(A)
    r = sr.fit(row, col, A[row, col], 3, 4, nsv=3, nv=3, max_iter=5, tol=1e-8, v0=np.array([1.0, 2.0, 3.0]))
    want = np.linalg.svd(A, compute_uv=False)
    assert r.nconv == 3 and r.passes == 1 and r.kk_pass == [3]
    assert np.all(np.abs(r.sigma - want) <= 1e-12 * want)
    assert r.beta_first[2] < 1e-13 and np.all(r.err < 1e-13)
    assert np.max(np.abs(r.U.T @ A @ r.V - np.diag(r.sigma))) < 1e-13


def test_zero_passes():
    row, col, val, rows, cols, v0, _ = sr.case_inputs("A")
    r = sr.fit(row, col, val, rows, cols, 2, 4, max_iter=1, v0=v0)
    assert r.passes == 0 and r.nconv == 0 and np.all(np.isnan(r.sigma)) and r.U.shape == (rows, 0)


@pytest.mark.parametrize("name", list(sr.CASES))
def test_checker_converges_and_meets_the_residual_bound(name):
    spec = sr.case_inputs(name)[6]
    r = sr.case_reference(name)
    # a condition on the inputs, before anything else
    assert r.nconv >= spec["nsv"] and r.passes < spec["max_iter"] - 1, (r.nconv, r.passes)
    assert r.margin >= 0.1, r.margin   # every errest far from tol: kk per pass is decided
    want = sr.dense_sigma(name)[:spec["nsv"]]
    got = r.sigma[:spec["nsv"]]
    print(name, "sigma", got, "|sigma - dense|", np.abs(got - want), "bound", sr.truth_bound(r.resid, want[0]))
    assert np.all(np.abs(got - want) <= sr.truth_bound(r.resid, want[0]))
    assert np.all(r.err < spec["tol"])
    assert np.all(np.abs(np.linalg.norm(r.U, axis=0) - 1) < 1e-12) and np.all(np.abs(np.linalg.norm(r.V, axis=0) - 1) < 1e-12)


def test_sigma_is_filled_for_unconverged_positions_too():
    r = sr.case_reference("A")
    assert r.kk_pass[0] < sr.CASES["A"][4] and not np.any(np.isnan(r.sigma))   # the first pass wrote all nv


def test_drift_sets_the_device_bounds():
    """The checker against itself with the entries in another order (another summation order of
    every product) and v0 perturbed by 1e-15 relative.  Measured here (printed by -s): first-pass
    alpha and beta drift by up to 1.7e-15 / 1.9e-15 relative, the converged sigma by 4.8e-16
    sigma_1, and max|U^T U - I|, max|V^T V - I| of the checker are 2.7e-15 / 1.0e-15; the
    unconverged tail of sigma drifts by 1e-9 sigma_1 and is therefore not compared."""
    worst = dict(ab=0.0, sigma=0.0, orth=0.0)
    for name in sr.CASES:
        _, _, _, rows, cols, v0, spec = sr.case_inputs(name)
        row, col, val = sr.case_entries(name)
        rng = np.random.default_rng(99)
        perm = rng.permutation(len(row))
        v0p = v0 * (1 + 1e-15 * rng.standard_normal(rows))
        a = sr.case_reference(name)
        b = sr.fit(row, col, val, rows, cols, spec["nsv"], spec["nv"], spec["max_iter"], spec["tol"], 3, v0p, perm)
        assert a.kk_pass == b.kk_pass and a.nconv == b.nconv
        d_alpha = np.max(np.abs(a.alpha_first - b.alpha_first) / np.abs(a.alpha_first))
        d_beta = np.max(np.abs(a.beta_first - b.beta_first) / np.abs(a.beta_first))
        d_sigma = np.max(np.abs(a.sigma[:a.nconv] - b.sigma[:a.nconv])) / a.sigma[0]
        d_tail = np.max(np.abs(a.sigma - b.sigma)) / a.sigma[0]
        orth = max(np.max(np.abs(a.U.T @ a.U - np.eye(a.U.shape[1]))), np.max(np.abs(a.V.T @ a.V - np.eye(a.V.shape[1]))))
        print(name, "first pass alpha", a.alpha_first, "beta", a.beta_first, "sigma", a.sigma)
        print(name, "drift: alpha", d_alpha, "beta", d_beta, "converged sigma / sigma_1", d_sigma,
              "all sigma / sigma_1", d_tail, "orthogonality defect", orth)
        worst["ab"] = max(worst["ab"], d_alpha, d_beta)
        worst["sigma"] = max(worst["sigma"], d_sigma)
        worst["orth"] = max(worst["orth"], orth)
    assert MARGIN * worst["ab"] <= BOUND_ALPHA_BETA
    assert MARGIN * worst["sigma"] <= BOUND_SIGMA
    assert MARGIN * worst["orth"] <= BOUND_ORTH


# ---- the host Jacobi ------------------------------------------------------------------------

def small_svd(T):
    m = T.shape[0]
    T = np.ascontiguousarray(T, dtype=np.float64)
    a, PT, b = np.zeros((m, m)), np.zeros((m, m)), np.zeros(m)
    sweeps = _native.load().cf_debug_small_svd(m, ptr(T), ptr(a), ptr(b), ptr(PT))
    assert sweeps >= 0
    return a, b, PT


def bidiagonal(m, seed, zero_at=None):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 10.0, m)
    if zero_at is not None:
        d[zero_at] = 0.0
    return np.diag(d) + np.diag(rng.uniform(0.5, 10.0, m - 1), 1)


@pytest.mark.parametrize("m,zero_at", [(1, None), (2, None), (7, None), (7, 3), (33, None), (33, 32)])
def test_host_jacobi_matches_lapack(m, zero_at):
    T = bidiagonal(m, seed=m, zero_at=zero_at)
    a, b, PT = small_svd(T)
    want = np.linalg.svd(T, compute_uv=False)
    eps = np.finfo(np.float64).eps
    print(m, zero_at, "max|b - lapack|", np.max(np.abs(b - want)), "|a b PT^T - T|", np.linalg.norm(a @ np.diag(b) @ PT.T - T))
    assert np.all(np.diff(b) <= 0) and np.all(b >= 0)
    assert np.max(np.abs(b - want)) <= 8 * m * eps * want[0]
    assert np.linalg.norm(a @ np.diag(b) @ PT.T - T) <= 8 * m * eps * np.linalg.norm(T)
    assert np.max(np.abs(a.T @ a - np.eye(m))) <= 8 * m * eps and np.max(np.abs(PT.T @ PT - np.eye(m))) <= 8 * m * eps


def test_host_jacobi_keeps_small_values_to_relative_accuracy():
    """A graded bidiagonal: the smallest value is 1e-12 of the largest and still has 10 digits."""
    T = np.diag([1.0, 1e-4, 1e-8, 1e-12]) + np.diag([0.5, 0.5e-4, 0.5e-8], 1)
    _, b, _ = small_svd(T)
    want = np.linalg.svd(T, compute_uv=False)   # bidiagonal: LAPACK is relatively accurate too
    assert np.all(np.abs(b - want) <= 1e-10 * want)


def test_host_jacobi_rejects_bad_arguments():
    z = np.zeros(4)
    lib = _native.load()
    assert lib.cf_debug_small_svd(0, ptr(z), ptr(z), ptr(z), ptr(z)) == _native.CF_EINVAL
    assert lib.cf_debug_small_svd(2, None, ptr(z), ptr(z), ptr(z)) == _native.CF_EINVAL
