"""ALS matrix factorization on the GPU (cf_als_fit / cf_als_error / cf_als_predict) against the
numpy checker tests/als_ref.py.

The cases' schedules are decided far from any rounding (the checker's run keeps every priority
at least 1e-6 relative away from tol and every solved system positive definite with
lambda_min / lambda_max >= 1e-6), so update counts and supersteps are compared exactly.
Factor bound: 1e-10 * max|factor| -- on the CPU the checker against itself with the edge order
permuted and the initial factors perturbed by 1e-15 relative drifts by a few 1e-13 on these
cases, which leaves a few hundred times that for another summation tree and an unpivoted
factorisation."""
import ctypes

import numpy as np
import pytest

import als_ref as ar
from collaborative_filtering_amd import _native
from collaborative_filtering_amd._native import ptr

pytestmark = pytest.mark.gpu

SPEC = {c: dict(regnormal=ar.CASES[c][3], lam=ar.CASES[c][4], tol=ar.CASES[c][5], max_updates=ar.CASES[c][6])
        for c in ar.CASES}
_FITS = {}


def device_fit(ctx, name, **over):
    g, U0, V0, *_ = ar.case_inputs(name)
    kw = dict(SPEC[name], out_degree=g.out_degree)
    kw.update(over)
    return ctx.als_fit(g.user, g.item, g.obs, g.n_users, g.n_items, U0, V0, **kw)


def case_fit(ctx, name):
    """The device's run of a case, computed once and shared (not modified by the tests)."""
    if name not in _FITS:
        _FITS[name] = device_fit(ctx, name)
    return _FITS[name]


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_case_matches_checker(gpu_ctx, name):
    g, U0, V0, *_ = ar.case_inputs(name)
    ref = ar.case_reference(name)
    # conditions on the input, not on the device
    assert ref.margin >= 1e-6 and ref.min_eig_ratio >= 1e-6, (ref.margin, ref.min_eig_ratio)
    deg = np.bincount(g.item, minlength=g.n_items)
    assert deg.max() > _native.load().cf_debug_als_low_max() >= deg[deg > 0].min()   # both wave and workgroup paths
    r = case_fit(gpu_ctx, name)
    print(name, "supersteps", r.supersteps, ref.supersteps, "updates", r.updates, ref.updates)
    assert np.array_equal(r.nupdates_user, ref.nupdates_user)
    assert np.array_equal(r.nupdates_item, ref.nupdates_item)
    assert r.supersteps == ref.supersteps and r.updates == ref.updates
    for got, want in ((r.U, ref.U), (r.V, ref.V)):
        err = np.max(np.abs(got - want))
        print(name, "max|dF|", err, "max|F|", np.max(np.abs(want)))
        assert err <= 1e-10 * np.max(np.abs(want))
    for got, want in ((r.residual_user, ref.residual_user), (r.residual_item, ref.residual_item)):
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.maximum(1e-6 * np.abs(want), 1e-12))
    assert r.n_not_pd == 0


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_error_and_predictions(gpu_ctx, name):
    g, *_ = ar.case_inputs(name)
    r = case_fit(gpu_ctx, name)
    for u, i, o in ((g.user, g.item, g.obs), (g.vuser, g.vitem, g.vobs)):
        want = np.sqrt(ar.sum_sq_error(u, i, o, r.U, r.V, 1.0, 5.0) / len(u))
        got = gpu_ctx.als_rmse(u, i, o, r.U, r.V, 1.0, 5.0)
        unclamped = np.sqrt(ar.sum_sq_error(u, i, o, r.U, r.V, -1e100, 1e100) / len(u))
        print(name, "rmse", got, want, "unclamped", unclamped)
        assert abs(got - want) <= 1e-12 * want
    rng = np.random.default_rng(3)
    pu = rng.integers(0, g.n_users, 50).astype(np.uint32)
    pi = rng.integers(0, g.n_items, 50).astype(np.uint32)
    got = gpu_ctx.als_predict(pu, pi, r.U, r.V)
    prod = r.U[pu] * r.V[pi]
    want, scale = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    # 1e-13 relative to the dot itself wherever the terms do not cancel (|u.v| >= 0.1 sum|u_d v_d|).
    # Where they do, no summation order can promise that: a D-term dot product is only within
    # D * 2^-53 * sum|u_d v_d| of the exact one, so those pairs are held to 1e-13 of that sum.
    plain = np.abs(want) >= 0.1 * scale
    print(name, "pairs held to 1e-13 |u.v|:", int(plain.sum()), "of", len(want))
    assert plain.sum() >= 10
    assert np.all(np.abs(got - want)[plain] <= 1e-13 * np.abs(want)[plain])
    assert np.all(np.abs(got - want)[~plain] <= 1e-13 * scale[~plain])


def test_clamping_is_exercised(gpu_ctx):
    g, *_ = ar.case_inputs("A")
    r = case_fit(gpu_ctx, "A")
    U, V = 3.0 * r.U, r.V   # predictions well outside [1, 5]
    want = ar.sum_sq_error(g.vuser, g.vitem, g.vobs, U, V, 1.0, 5.0)
    assert want != ar.sum_sq_error(g.vuser, g.vitem, g.vobs, U, V, -1e100, 1e100)
    got = gpu_ctx.als_sum_sq_error(g.vuser, g.vitem, g.vobs, U, V, 1.0, 5.0)
    assert abs(got - want) <= 1e-12 * want


def test_edge_semantics(gpu_ctx):
    g, U0, V0, *_ = ar.case_inputs("A")
    r = case_fit(gpu_ctx, "A")
    assert r.nupdates_user[0] == 0 and np.array_equal(r.U[0], U0[0])   # no edges at all: never signalled
    assert r.nupdates_user[2] == 1 and r.residual_user[2] == 0.0 and np.array_equal(r.U[2], U0[2])   # VALIDATE only
    assert r.nupdates_item[-1] == 0 and np.array_equal(r.V[-1], V0[-1])   # an item nobody rated
    one = device_fit(gpu_ctx, "A", max_supersteps=1)
    assert one.supersteps == 1 and np.array_equal(one.V, V0) and not np.any(one.nupdates_item)
    assert np.all(one.nupdates_user[g.out_degree > 0] == 1)
    ref = ar.case_reference("A")
    assert np.max(np.abs(one.U - ref.snapshots[0][0])) <= 1e-10 * np.max(np.abs(ref.snapshots[0][0]))


def test_repeat_is_bit_identical(gpu_ctx):
    a, b = case_fit(gpu_ctx, "A"), device_fit(gpu_ctx, "A")
    for x, y in ((a.U, b.U), (a.V, b.V), (a.residual_user, b.residual_user), (a.residual_item, b.residual_item),
                 (a.nupdates_user, b.nupdates_user), (a.nupdates_item, b.nupdates_item)):
        assert x.tobytes() == y.tobytes()


def test_independent_of_the_active_set(gpu_ctx):
    g, *_ = ar.case_inputs("A")
    full = device_fit(gpu_ctx, "A", max_supersteps=1)
    even = (np.arange(g.n_users) % 2 == 0) & (g.out_degree > 0)
    part = device_fit(gpu_ctx, "A", max_supersteps=1, activate_user=even)
    assert part.U[even].tobytes() == full.U[even].tobytes()
    assert part.residual_user[even].tobytes() == full.residual_user[even].tobytes()
    assert not np.any(part.nupdates_user[~even])


@pytest.mark.parametrize("D", [8, 13, 33])   # the high class at DP = 8, 16 and 64
def test_segmented_vertex(gpu_ctx, D):
    """One item rated by 2 * segment + 37 users: its Gram is summed from three segment partials.
    Every user has this one edge, so after the user half-sweep all user factors are parallel to
    the item's initial factor and the item's Gram has rank one: only the regularisation keeps
    the system well conditioned.  lambda * degree on both sides keeps lambda_min / lambda_max
    above 1e-3, the conditioning of the four cases the 1e-10 bound was derived on (plain
    lambda = 0.05 would give 3e-6, where rounding alone is worth 1e-9)."""
    seg = _native.load().cf_debug_als_segment()
    n_users = 2 * seg + 37
    rng = np.random.default_rng(5)
    user = rng.permutation(n_users).astype(np.uint32)
    item = np.zeros(n_users, np.uint32)
    obs = rng.integers(1, 6, n_users).astype(np.float32)
    U0, V0 = rng.uniform(-1, 1, (n_users, D)), rng.uniform(-1, 1, (1, D))
    ru, ri = ar.reg_arrays(user, item, n_users, 1, 0.05, "degree")
    ref = ar.fit(user, item, obs, n_users, 1, U0, V0, ru, ri, tol=1e-3, max_supersteps=2)
    assert ref.supersteps == 2 and ref.nupdates_item[0] == 1 and ref.min_eig_ratio >= 1e-3, ref.min_eig_ratio
    runs = [gpu_ctx.als_fit(user, item, obs, n_users, 1, U0, V0, lam=0.05, regnormal="degree", max_supersteps=2)
            for _ in range(2)]
    r = runs[0]
    assert r.supersteps == 2 and r.nupdates_item[0] == 1 and r.n_not_pd == 0
    assert np.max(np.abs(r.U - ref.U)) <= 1e-10 * np.max(np.abs(ref.U))
    print("segmented item: max|dV|", np.max(np.abs(r.V - ref.V)), "max|V|", np.max(np.abs(ref.V)))
    assert np.max(np.abs(r.V - ref.V)) <= 1e-10 * np.max(np.abs(ref.V))
    assert runs[1].V.tobytes() == r.V.tobytes() and runs[1].U.tobytes() == r.U.tobytes()


def test_argument_checks(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.h

    def call(n_users, n_items, D, uoff, uitem, ioff, iuser):
        nnz = len(uitem)
        obs = np.ones(max(nnz, 1), np.float32)
        U, V = np.zeros((max(n_users, 1), D)), np.zeros((max(n_items, 1), D))
        z = lambda n, t: np.zeros(max(n, 1), t)   # noqa: E731
        st = _native.AlsStats()
        return lib.cf_als_fit(h, n_users, n_items, D, ptr(uoff), ptr(uitem), ptr(obs), ptr(ioff), ptr(iuser), ptr(obs),
                              ptr(z(n_users, np.float64)), ptr(z(n_items, np.float64)), 1e-3, (1 << 64) - 1, 0, ptr(U),
                              ptr(V), ptr(z(n_users, np.uint32)), ptr(z(n_items, np.uint32)), ptr(z(n_users, np.float32)),
                              ptr(z(n_items, np.float32)), None, ctypes.byref(st)), st

    u64, u32 = np.uint64, np.uint32
    uoff, uitem = np.array([0, 1, 2], u64), np.array([0, 0], u32)
    ioff, iuser = np.array([0, 2], u64), np.array([0, 1], u32)
    assert call(2, 1, 4, uoff, uitem, ioff, iuser)[0] == _native.CF_OK
    assert call(2, 1, 65, uoff, uitem, ioff, iuser)[0] == _native.CF_ERANGE
    assert call(2, 1, 4, uoff, uitem, np.array([0, 1], u64), iuser)[0] == _native.CF_EINVAL   # edge totals differ
    assert call(2, 2, 4, uoff, uitem, np.array([0, 1, 2], u64), iuser)[0] == _native.CF_EINVAL   # per-item counts differ
    rc, st = call(0, 0, 4, np.zeros(1, u64), np.zeros(0, u32), np.zeros(1, u64), np.zeros(0, u32))
    assert rc == _native.CF_OK and st.supersteps == 0 and st.updates == 0
    rc, st = call(2, 1, 4, np.zeros(3, u64), np.zeros(0, u32), np.zeros(2, u64), np.zeros(0, u32))   # no edges
    assert rc == _native.CF_OK and st.supersteps == 1 and st.updates == 2


def test_python_layer_accepts_an_empty_side(gpu_ctx):
    """n_users == 0 is a valid no-op at the ABI; the Python layer passes it through."""
    r = gpu_ctx.als_fit([], [], [], 0, 0, np.zeros((0, 4)), np.zeros((0, 4)))
    assert r.supersteps == 0 and r.updates == 0 and r.U.shape == (0, 4) and r.V.shape == (0, 4)
    V0 = np.arange(12.0).reshape(3, 4)
    r = gpu_ctx.als_fit([], [], [], 0, 3, np.zeros(0), V0)
    assert r.supersteps == 0 and np.array_equal(r.V, V0) and r.U.shape == (0, 4)


def test_workspace_release(gpu_ctx):
    """The ALS workspace is one of the cached workspaces: released, then allocated again."""
    a = case_fit(gpu_ctx, "C")
    gpu_ctx.release_workspaces()
    b = device_fit(gpu_ctx, "C")
    assert a.U.tobytes() == b.U.tobytes() and a.V.tobytes() == b.V.tobytes()
