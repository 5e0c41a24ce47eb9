"""The numpy checker of the EASE entry points (tests/ease_ref.py) against the model's own
definition: the constrained least squares it solves, the hand-worked 2-item case, the item without
an edge and the summation order of a score (CPU only)."""
import numpy as np
import pytest

import ease_ref as er


def random_train(rng, n_users, n_items, density, kind="int", skip=None):
    """A user CSR with strictly ascending item lists (none holds item `skip`); ratings integer,
    half-integer or float32."""
    lists = [np.flatnonzero((rng.random(n_items) < density) & (np.arange(n_items) != skip)) for _ in range(n_users)]
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.uint64)
    items = np.concatenate(lists + [np.zeros(0, np.int64)]).astype(np.uint32)
    if kind == "int":
        ratings = rng.integers(1, 6, len(items)).astype(np.float32)
    elif kind == "half":
        ratings = (rng.integers(1, 11, len(items)) / 2).astype(np.float32)
    else:
        ratings = rng.normal(3.0, 1.0, len(items)).astype(np.float32)
    return off, items, ratings


@pytest.mark.parametrize("binary", [False, True])
def test_gram_is_xtx_plus_lambda_and_symmetric(binary):
    rng = np.random.default_rng(1)
    off, items, ratings = random_train(rng, 50, 23, 0.2, "float")
    G = er.gram(off, items, ratings, 23, 0.75, binary)
    X = er.dense(off, items, ratings, 23, binary)
    assert np.array_equal(G, G.T)
    assert np.allclose(G, X.T @ X + 0.75 * np.eye(23), rtol=1e-14, atol=0)
    if binary:   # integers: exact in any order
        assert np.array_equal(G, X.T @ X + 0.75 * np.eye(23))


@pytest.mark.parametrize("binary", [False, True])
def test_weights_solve_the_constrained_least_squares(binary):
    """B minimises |X - X B|^2 + lam |B|^2 subject to diag(B) = 0: the gradient G B - X^T X vanishes
    off the diagonal (on it stands the multiplier).  Independent of the closed form."""
    rng = np.random.default_rng(2)
    n = 31
    off, items, ratings = random_train(rng, 120, n, 0.15, "half")
    lam = 2.0
    G = er.gram(off, items, ratings, n, lam, binary)
    B = er.weights(G)
    assert not np.diag(B).any()
    X = er.dense(off, items, ratings, n, binary)
    grad = G @ B - X.T @ X
    offdiag = ~np.eye(n, dtype=bool)
    scale = np.abs(G).max() * max(1.0, np.abs(B).max())
    assert np.abs(grad[offdiag]).max() <= 1e-12 * scale
    assert np.abs(np.diag(grad)).min() > 1e-3   # the constraint is active: the multipliers are not zero
    # and it is a minimum among matrices with a zero diagonal
    def loss(M):
        return ((X - X @ M) ** 2).sum() + lam * (M ** 2).sum()
    for _ in range(5):
        E = rng.normal(0, 1e-3, (n, n))
        np.fill_diagonal(E, 0.0)
        assert loss(B + E) > loss(B)


def test_item_without_an_edge_has_a_zero_row_and_column():
    rng = np.random.default_rng(3)
    n = 12
    off, items, ratings = random_train(rng, 40, n, 0.3, skip=5)
    G = er.gram(off, items, ratings, n, 0.5)
    assert G[5, 5] == 0.5 and not np.delete(G[5], 5).any() and not np.delete(G[:, 5], 5).any()
    B = er.weights(G)
    assert not B[5].any() and not B[:, 5].any()
    assert np.abs(B).max() > 0


def test_two_items_by_hand():
    # users {0, 1} and {0}, binary, lam = 1: G = [[3, 1], [1, 2]], P = [[2, -1], [-1, 3]] / 5
    off = np.array([0, 2, 3], np.uint64)
    items = np.array([0, 1, 0], np.uint32)
    G = er.gram(off, items, np.array([4.0, 2.0, 5.0], np.float32), 2, 1.0, binary=True)
    assert G.tolist() == [[3.0, 1.0], [1.0, 2.0]]
    B = er.weights(G)
    assert B[0, 0] == 0.0 and B[1, 1] == 0.0
    assert abs(B[0, 1] - 1.0 / 3.0) < 1e-15 and abs(B[1, 0] - 0.5) < 1e-15
    # with the ratings: G = [[16 + 25 + 1, 8], [8, 4 + 1]]
    G = er.gram(off, items, np.array([4.0, 2.0, 5.0], np.float32), 2, 1.0)
    assert G.tolist() == [[42.0, 8.0], [8.0, 5.0]]
    B = er.weights(G)   # P = [[5, -8], [-8, 42]] / 146
    assert abs(B[0, 1] - 8.0 / 42.0) < 1e-15 and abs(B[1, 0] - 8.0 / 5.0) < 1e-15


def test_score_runs_in_profile_order_product_then_sum():
    e = 2.0 ** -53
    B = np.zeros((3, 3))
    B[:, 0] = (1.0, e, e)   # 1 + e + e = 1 in this order, e + e + 1 = 1 + 2 e in the other
    off = np.array([0, 3, 6], np.uint64)
    items = np.array([0, 1, 2, 2, 1, 0], np.uint32)
    S = er.score_matrix(B, off, items, np.ones(6, np.float32))
    assert S[0, 0] == 1.0 and S[1, 0] == 1.0 + 2 * e
    # the product is rounded before the sum: 3 (1 + 2 e) = 3 + 6 e rounds to 3 + 8 e, and adding
    # -3 leaves 8 e; a fused multiply-add would leave 6 e
    B2 = np.zeros((2, 2))
    B2[0, 1], B2[1, 1] = -3.0, 1.0 + 2 * e
    off2 = np.array([0, 2], np.uint64)
    S2 = er.score_matrix(B2, off2, np.array([0, 1], np.uint32), np.array([1.0, 3.0], np.float32))
    assert S2[0, 1] == 8 * e
    # binary ignores the ratings
    S3 = er.score_matrix(B2, off2, np.array([0, 1], np.uint32), np.array([1.0, 3.0], np.float32), binary=True)
    assert S3[0, 1] == -3.0 + (1.0 + 2 * e)


def test_topn_and_evaluate_delegate_with_the_profile_excluded():
    rng = np.random.default_rng(5)
    n = 9
    B = rng.normal(0, 1, (n, n))
    off, items, ratings = random_train(rng, 6, n, 0.4)
    got = er.topn(B, off, items, ratings, 4)
    S = er.score_matrix(B, off, items, ratings)
    for u in range(6):
        own = set(items[int(off[u]):int(off[u + 1])].tolist())
        listed = got[0][u, : got[2][u]].tolist()
        assert not own & set(listed)
        cand = [j for j in range(n) if j not in own]
        assert listed == sorted(cand, key=lambda j: (-S[u, j], j))[:4]
    held = (np.array([0, 3]), np.array([got[0][0, 1], got[0][3, 0]]))
    rank = er.evaluate(B, off, items, ratings, 4, held)[0]
    assert rank.tolist() == [1, 0]
