"""The numpy checker of cf_knn_topn (knn_topn_ref.py) on hand-computed graphs (CPU only).  Every
graph here is directional and every expected score would come out differently from W transposed."""
import numpy as np

import knn_topn_ref as kr

MAX = 0xFFFFFFFF


def profile(*users):
    """users: lists of (item, rating) -> (off, items, ratings)."""
    off = np.cumsum([0] + [len(u) for u in users]).astype(np.uint64)
    items = np.array([i for u in users for i, _ in u], dtype=np.uint32)
    ratings = np.array([r for u in users for _, r in u], dtype=np.float32)
    return off, items, ratings


def star():
    """Centre 0 and leaves 1..4: every leaf points at the centre with 0.5, the centre at every leaf with 0.25."""
    W = np.zeros((5, 5), np.float32)
    W[1:, 0] = 0.5
    W[0, 1:] = 0.25
    return W


def test_star_graph_uses_the_out_edges_of_the_scored_item():
    W = star()
    off, items, ratings = profile([(0, 4.0)], [(1, 2.0)])
    S = kr.score_matrix(W, off, items, ratings)
    # user 0 rated the centre: every leaf m scores W[m, 0] * 4 = 2 (transposed: 0.25 * 4 = 1)
    assert S[0].tolist() == [0.0, 2.0, 2.0, 2.0, 2.0]
    # user 1 rated leaf 1: only the centre has an out-edge to it, W[0, 1] * 2 (transposed: W[1, 0] * 2 = 1)
    assert S[1].tolist() == [0.5, 0.0, 0.0, 0.0, 0.0]
    assert not np.array_equal(S, kr.score_matrix(W.T, off, items, ratings))
    lists, scores, count, n_nan = kr.topn(W, off, items, ratings, 3)
    assert lists.tolist() == [[1, 2, 3], [0, 2, 3]]   # ties by item ascending, the profile left out
    assert scores.tolist() == [[2.0, 2.0, 2.0], [0.5, 0.0, 0.0]]
    assert count.tolist() == [3, 3] and n_nan == 0
    assert kr.topn(W, off, items, ratings, 5, exclude=None)[0].tolist() == [[1, 2, 3, 4, 0], [0, 1, 2, 3, 4]]


def test_two_cliques():
    W = np.zeros((6, 6), np.float32)
    W[:3, :3] = 0.5
    W[3:, 3:] = 0.25
    np.fill_diagonal(W, 0.0)
    off, items, ratings = profile([(0, 4.0), (3, 2.0)], [])
    S = kr.score_matrix(W, off, items, ratings)
    assert S.tolist() == [[0.0, 2.0, 2.0, 0.0, 0.5, 0.5], [0.0] * 6]
    lists, scores, count, _ = kr.topn(W, off, items, ratings, 6)
    assert lists.tolist() == [[1, 2, 4, 5, MAX, MAX], [0, 1, 2, 3, 4, 5]]   # empty profile: the lowest ids at score 0
    assert scores[0].tolist() == [2.0, 2.0, 0.5, 0.5, 0.0, 0.0] and count.tolist() == [4, 6]
    M = kr.score_matrix(W, off, items, ratings, mode="mean")
    assert M.tolist() == [[0.0, 4.0, 4.0, 0.0, 2.0, 2.0], [0.0] * 6]


W3 = np.array([[0.0, 0.5, 0.0], [0.0, 0.0, 0.25], [0.75, 0.0, 0.0]], np.float32)


def test_asymmetric_three_items_both_modes():
    off, items, ratings = profile([(0, 2.0), (1, 4.0)])
    # m = 0: W[0, 1] = 0.5 -> sw 0.5, swr 2;  m = 1: no out-edge into the profile;  m = 2: W[2, 0] = 0.75 -> sw 0.75, swr 1.5
    sw, swr = kr.sums(W3, off, items, ratings, 0.1)
    assert sw.tolist() == [[0.5, 0.0, 0.75]] and swr.tolist() == [[2.0, 0.0, 1.5]]
    assert kr.score_matrix(W3, off, items, ratings, "sum").tolist() == [[2.0, 0.0, 1.5]]
    assert kr.score_matrix(W3, off, items, ratings, "mean").tolist() == [[4.0, 0.0, 2.0]]
    # the transposed scatter would give m = 1: W[0, 1] * 2 = 1 and m = 2: W[1, 2] * 4 = 1
    assert kr.score_matrix(W3.T, off, items, ratings, "sum").tolist() == [[0.0, 1.0, 1.0]]
    # a profile item listed twice counts twice
    off2, items2, ratings2 = profile([(0, 2.0), (1, 4.0), (0, 2.0)])
    assert kr.score_matrix(W3, off2, items2, ratings2, "sum").tolist() == [[2.0, 0.0, 3.0]]
    assert kr.score_matrix(W3, off2, items2, ratings2, "mean").tolist() == [[4.0, 0.0, 2.0]]


def knn3_formula(W, off, items, ratings):
    """knn3.cpp:185-227 per listed pair, as tests/test_gpu_knn.py's knn3_reference states it: over
    the user's own items j with (double) w(m, j) > 0.1, pred = sum w r / sum w, 0 without a neighbour."""
    pred = np.zeros(len(items))
    for u in range(len(off) - 1):
        b, e = int(off[u]), int(off[u + 1])
        for t in range(b, e):
            sw = swr = 0.0
            for j in range(b, e):
                w = float(W[items[t], items[j]])
                if w > 0.1:
                    sw += w
                    swr += w * float(ratings[j])
            pred[t] = swr / sw if sw > 0.0 else 0.0
    return pred


def test_mean_mode_on_own_items_is_knn3():
    rng = np.random.default_rng(7)
    n = 23
    W = (rng.random((n, n)) * (rng.random((n, n)) < 0.4)).astype(np.float32)
    np.fill_diagonal(W, 0.0)
    W[5, :] = 0.05   # an item without a neighbour above the threshold
    users = [[(int(i), float(np.round(rng.normal(3, 2), 2))) for i in np.sort(rng.choice(n, k, replace=False))]
             for k in (1, 4, 9, 15)]
    users.append([(5, 3.0), (6, 1.0)])
    off, items, ratings = profile(*users)
    S = kr.score_matrix(W, off, items, ratings, mode="mean", w_min=0.1)
    own = S[np.repeat(np.arange(len(users)), np.diff(off.astype(np.int64))), items.astype(np.int64)]
    assert np.array_equal(own, knn3_formula(W, off, items, ratings))
    assert own[int(off[4])] == 0.0   # item 5 for the last user: no neighbour -> 0


def test_threshold_is_strict_at_a_dyadic_w_min():
    W = np.zeros((3, 3), np.float32)
    W[1, 0] = 0.125
    W[2, 0] = 0.125 + 2.0 ** -20
    off, items, ratings = profile([(0, 1.0)])
    assert kr.score_matrix(W, off, items, ratings, w_min=0.125).tolist() == [[0.0, 0.0, 0.125 + 2.0 ** -20]]
    assert kr.score_matrix(W, off, items, ratings, w_min=0.0).tolist() == [[0.0, 0.125, 0.125 + 2.0 ** -20]]


def test_nan_rating_and_negative_zero():
    off, items, ratings = profile([(0, np.nan)], [(0, -0.0)])
    lists, scores, count, n_nan = kr.topn(W3, off, items, ratings, 3)
    assert n_nan == 1 and count.tolist() == [1, 2]   # user 0: item 2 is NaN, item 0 excluded
    assert lists.tolist() == [[1, MAX, MAX], [1, 2, MAX]]
    assert not np.signbit(scores).any()


def test_rank_eval_agrees_with_the_lists():
    off, items, ratings = profile([(0, 2.0)], [(1, 4.0), (2, 1.0)])
    held = (np.array([0, 0, 1]), np.array([2, 0, 0]))
    rank, n_cand, users, s = kr.evaluate(W3, off, items, ratings, 2, held)
    # user 0: candidates 1 (0), 2 (1.5) -> item 2 has rank 0, item 0 is its own profile: skipped
    # user 1: W[0, 1] * 4 = 2 -> the only candidate, rank 0
    assert rank.tolist() == [0, MAX, 0] and n_cand.tolist() == [2, 2, 1]
    assert s["edges_counted"] == 2 and s["edges_skipped"] == 1 and s["users_evaluated"] == 2
