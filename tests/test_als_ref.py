"""The ALS checker (tests/als_ref.py) checks itself on the CPU."""
import numpy as np

import als_ref as ar


def low_rank_problem(n_users=30, n_items=12, D=3, seed=0):
    """obs = U* V*^T with small-integer factors: every rating is exactly a float."""
    rng = np.random.default_rng(seed)
    Us = rng.integers(-3, 4, (n_users, D)).astype(np.float64)
    Vs = rng.integers(-3, 4, (n_items, D)).astype(np.float64)
    user, item = [], []
    for u in range(n_users):   # every user degree >= D, every item degree >= D
        its = rng.choice(n_items, size=D + 3, replace=False)
        user += [u] * len(its)
        item += its.tolist()
    user, item = np.array(user, np.uint32), np.array(item, np.uint32)
    obs = np.einsum("ij,ij->i", Us[user], Vs[item]).astype(np.float32)
    assert np.array_equal(obs.astype(np.float64), np.einsum("ij,ij->i", Us[user], Vs[item]))
    return user, item, obs, Us, Vs


def test_exact_low_rank_user_sweep_recovers_factors():
    user, item, obs, Us, Vs = low_rank_problem()
    n_users, n_items = Us.shape[0], Vs.shape[0]
    # every user's neighbour factors must span R^D for lambda = 0
    for u in range(n_users):
        assert np.linalg.matrix_rank(Vs[item[user == u]]) == Vs.shape[1]
    U0 = np.random.default_rng(1).uniform(-1, 1, Us.shape)
    z = np.zeros
    r = ar.fit(user, item, obs, n_users, n_items, U0, Vs, z(n_users), z(n_items), tol=1e-3, max_supersteps=1)
    assert r.supersteps == 1 and r.updates == n_users
    assert np.max(np.abs(r.U - Us)) <= 1e-10
    assert np.array_equal(r.V, Vs)


def test_single_update_equals_ridge_lstsq():
    rng = np.random.default_rng(2)
    X = rng.uniform(-1, 1, (9, 5))
    obs = rng.integers(1, 6, 9).astype(np.float32)
    reg = 0.35
    got, ratio = ar.update_vertex(X, obs, reg)
    aug = np.vstack([X, np.sqrt(reg) * np.eye(5)])
    want = np.linalg.lstsq(aug, np.concatenate([obs.astype(np.float64), np.zeros(5)]), rcond=None)[0]
    assert np.max(np.abs(got - want)) <= 1e-12 and 0 < ratio <= 1


def test_scheduling_edge_cases():
    g, U0, V0, ru, ri, tol, mu = ar.case_inputs("A")
    assert g.out_degree[0] == 0 and np.sum(g.user == 1) == 1 and g.out_degree[2] == 3 and not np.any(g.user == 2)
    assert np.sum(g.item == 0) == g.n_users - 2 and not np.any(g.item == g.n_items - 1)
    assert 0.10 < len(g.vuser) / (len(g.user) + len(g.vuser)) < 0.20
    r = ar.case_reference("A")
    assert r.nupdates_user[0] == 0 and np.array_equal(r.U[0], U0[0])
    assert r.nupdates_user[2] == 1 and r.residual_user[2] == 0 and np.array_equal(r.U[2], U0[2])
    assert r.nupdates_item[-1] == 0 and np.array_equal(r.V[-1], V0[-1])
    assert r.nupdates_user.max() <= mu and r.nupdates_item.max() <= mu
    assert r.residual_user.dtype == np.float32
    one = ar.fit(g.user, g.item, g.obs, g.n_users, g.n_items, U0, V0, ru, ri, tol=tol, max_updates=mu,
                 max_supersteps=1, activate_user=g.out_degree > 0)
    assert one.supersteps == 1 and np.array_equal(one.V, V0) and not np.any(one.nupdates_item)
    assert np.array_equal(one.U, r.snapshots[0][0])


def test_sides_alternate_and_run_ends():
    r = ar.case_reference("D")   # no update cap: runs until nobody is signalled
    assert r.supersteps > 12 and r.margin >= 1e-6 and r.min_eig_ratio >= 1e-6
    # superstep s updates users when s is even, items when odd
    for s in range(1, len(r.snapshots)):
        dU = np.any(r.snapshots[s][0] != r.snapshots[s - 1][0])
        dV = np.any(r.snapshots[s][1] != r.snapshots[s - 1][1])
        assert (dU, dV) == ((True, False) if s % 2 == 0 else (False, True))


def test_cases_are_far_from_rounding():
    for name in ("A", "B", "C"):
        r = ar.case_reference(name)
        assert r.margin >= 1e-6 and r.min_eig_ratio >= 1e-6, (name, r.margin, r.min_eig_ratio)
    g, *_ = ar.case_inputs("C")
    deg = np.bincount(g.item, minlength=g.n_items)
    assert deg[:-1].min() >= 42   # unregularised items (reference regnormal): well determined


def test_permuted_edges_drift_is_far_below_the_device_bound():
    """The basis of the GPU tests' 1e-10 bound: another edge order and initial factors perturbed
    by 1e-15 relative move the checker's own result by far less."""
    g, U0, V0, ru, ri, tol, mu = ar.case_inputs("A")
    rng = np.random.default_rng(9)
    p = rng.permutation(len(g.user))
    r2 = ar.fit(g.user[p], g.item[p], g.obs[p], g.n_users, g.n_items, U0 * (1 + 1e-15), V0 * (1 - 1e-15), ru, ri,
                tol=tol, max_updates=mu, activate_user=g.out_degree > 0)
    r = ar.case_reference("A")
    assert np.array_equal(r2.nupdates_user, r.nupdates_user) and r2.supersteps == r.supersteps
    drift = max(np.max(np.abs(r2.U - r.U)), np.max(np.abs(r2.V - r.V)))
    assert drift <= 1e-11 * max(np.max(np.abs(r.U)), np.max(np.abs(r.V))), drift
